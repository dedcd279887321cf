/*
 * fabber_device_spatial_noise_model.h - the spatial VB kernels for a model library's DEVICE body under AR(1) noise and
 * under a noise pattern.
 *
 * fabber_device_spatial_model.h gives a body the spatial kernels of white noise with one precision. Under the engine's
 * other noise policies (vb_spatial_noise.h) the same two kernels of the family evaluate the model - the set-up kernel
 * and the second sweep - and everything else (a_K, the first sweep in both of its forms, the result image) is the
 * engine's own for the parameter count and the policy. This header compiles those two around the SAME body, for one
 * parameter count per macro line:
 *
 *     FABBER_DEVICE_MODEL("invrec", InvRec)                     // the wave kernels: required, the route of voxelwise VB
 *     FABBER_DEVICE_SPATIAL_MODEL("invrec", InvRec, 3)          // spatial VB, white noise with one precision
 *     FABBER_DEVICE_SPATIAL_NOISE_MODEL("invrec", InvRec, 3, FVB_SPATIAL_NOISE_AR1 | FVB_SPATIAL_NOISE_PHIS)
 *
 * The first line is required: an entry without a wave body of the same name is never used. The second is not: the
 * white-noise spatial kernels are an entry of their own. Several lines per name are allowed, each for 1 <= P <= 6. It is
 * a header of its own because it includes the kernels of every policy: a library that does not want them does not pay
 * for them. Compile as fabber_device_model.h says.
 *
 * The last argument is a compile-time mask of the families to instantiate; a family left out costs nothing:
 *
 *   FVB_SPATIAL_NOISE_AR1   AR(1) noise with one echo (the reference's noise=ar, num-echoes=1): the policy SpAr1<P>.
 *                           Kernel table spatial<NAME,P,ar1>.
 *   FVB_SPATIAL_NOISE_PHIS  white noise with 2 to 4 precisions (noise-pattern): the policies SpPattern<P,2> and
 *                           SpPattern<P,4> (3 precisions run the latter). Kernel tables spatial<NAME,P,pattern2> and
 *                           spatial<NAME,P,pattern4>.
 *
 * The engine takes these kernels for a configuration when an entry for (name, n_params) whose mask covers the noise
 * model is registered. Two echoes, 5 to 8 precisions, other parameter counts and a volume cut into z-slabs over several
 * devices keep the host route (-40 from the engine, after which method=spatialvb evaluates the model's host code as
 * before). The initial posterior is an image, as fabber_device_spatial_model.h says. The body is evaluated pointwise.
 *
 * The body is the struct of fabber_device_model.h, unchanged, with eval declared __forceinline__. It receives the
 * model's constants and - where the model declares uses_suppdata - the supplementary data of the voxel its lane works
 * on, as in the kernels of voxelwise VB.
 *
 * The macro, at namespace scope:
 *   - instantiates five kernels per policy of the families in the mask: the set-up kernel and the second sweep with and
 *     without the free energy, each in the plain form and in the form that completes the split first sweep;
 *   - defines their launcher in this library's code object. The engine hands it the noise kind, which kernel, the grid
 *     and the dynamic LDS bytes of the launch (a pattern kernel's class bytes, one per timepoint): the launcher passes
 *     that count on and computes none. Asked for a kind outside the mask it answers -40 with a message and launches
 *     nothing;
 *   - registers { name, FVB_ABI_VERSION, sizeof(SpatialArgs), P, mask, rows of each policy's state image, launcher } with
 *     the engine from a static object whose destructor unregisters it. A refused registration (reported on stderr)
 *     leaves the model on the host route under these noise models.
 */
#ifndef FABBER_DEVICE_SPATIAL_NOISE_MODEL_H
#define FABBER_DEVICE_SPATIAL_NOISE_MODEL_H

#include "fabber_device_lane_model.h" /* fvb::LibraryLane: the body as a model of the lane-per-voxel kernels */
#include "../fabber_core_amd/csrc/vb_spatial_noise.h"

#include <cstdio>

namespace fvb
{
// The kernels of one macro line, looked up by what the engine asks for. A family outside FAMILIES is a discarded
// statement: its kernels are never instantiated.
template <class Eval, int P, int FAMILIES>
struct LibrarySpatialNoise
{
    static_assert(P >= 1 && P <= 6, "FABBER_DEVICE_SPATIAL_NOISE_MODEL: the spatial kernels of a library body exist for 1 to 6 parameters");
    static_assert(FAMILIES != 0 && (FAMILIES & ~(FVB_SPATIAL_NOISE_AR1 | FVB_SPATIAL_NOISE_PHIS)) == 0,
        "FABBER_DEVICE_SPATIAL_NOISE_MODEL: the mask names at least one of FVB_SPATIAL_NOISE_AR1 and FVB_SPATIAL_NOISE_PHIS and nothing else");
    typedef typename LibraryLane<Eval>::template Model<P> M;
    static constexpr bool ar1 = (FAMILIES & FVB_SPATIAL_NOISE_AR1) != 0, phis = (FAMILIES & FVB_SPATIAL_NOISE_PHIS) != 0;

    template <class NZ>
    static SpatialKernelFn kernel(int32_t which, bool need_f)
    {
        switch (which)
        {
        case FVB_SPATIAL_KERNEL_SETUP:
            return vb_spatial_setup_nz_kernel<M, P, NZ>;
        case FVB_SPATIAL_KERNEL_NOISE:
            return need_f ? (SpatialKernelFn)vb_spatial_noise_nz_kernel<M, P, true, false, NZ>
                          : (SpatialKernelFn)vb_spatial_noise_nz_kernel<M, P, false, false, NZ>;
        case FVB_SPATIAL_KERNEL_NOISE_SPLIT:
            return need_f ? (SpatialKernelFn)vb_spatial_noise_nz_kernel<M, P, true, true, NZ>
                          : (SpatialKernelFn)vb_spatial_noise_nz_kernel<M, P, false, true, NZ>;
        }
        return nullptr;
    }
    // covered: the kind is one of this line's families (its kernel may still be NULL: no such `which`)
    static SpatialKernelFn kernel_of(int32_t kind, int32_t which, bool need_f, bool &covered)
    {
        covered = false;
        if constexpr (ar1)
            if (kind == FVB_SPNZ_AR1)
            {
                covered = true;
                return kernel<SpAr1<P> >(which, need_f);
            }
        if constexpr (phis)
        {
            if (kind == FVB_SPNZ_PATTERN2)
            {
                covered = true;
                return kernel<SpPattern<P, 2> >(which, need_f);
            }
            if (kind == FVB_SPNZ_PATTERN4)
            {
                covered = true;
                return kernel<SpPattern<P, 4> >(which, need_f);
            }
        }
        return nullptr;
    }
    static constexpr int32_t state_rows_ar1()
    {
        if constexpr (ar1)
            return SpLayout<P>::ROWS + SpAr1<P>::EXTRA_ROWS;
        else
            return 0;
    }
    template <int N>
    static constexpr int32_t state_rows_phis()
    {
        if constexpr (phis)
            return SpLayout<P>::ROWS + SpPattern<P, N>::EXTRA_ROWS;
        else
            return 0;
    }

    static int32_t launch(const char *model, int32_t kind, int32_t which, int32_t need_f, const void *spatial_args, uint32_t grid,
        uint32_t lds_bytes, void *stream, char *err, int32_t err_len)
    {
        const SpatialArgs &sa = *static_cast<const SpatialArgs *>(spatial_args);
        bool covered = false;
        const SpatialKernelFn fn = kernel_of(kind, which, need_f != 0, covered);
        if (!covered)
        {
            if (err && err_len > 0)
                snprintf(err, (size_t)err_len, "spatial kernels of device model '%s' with %d parameters: not compiled for noise kind %d (its mask is %d)",
                    model, P, (int)kind, FAMILIES);
            return -40;
        }
        hipError_t e = hipErrorInvalidValue;
        if (fn)
        {
            hipLaunchKernelGGL(fn, dim3(grid), dim3(64), lds_bytes, static_cast<hipStream_t>(stream), sa);
            e = hipGetLastError();
        }
        if (e != hipSuccess && err && err_len > 0)
            snprintf(err, (size_t)err_len, "spatial kernel %d (noise kind %d) of a device model: %s", (int)which, (int)kind,
                fn ? hipGetErrorString(e) : "no such kernel");
        return e == hipSuccess ? 0 : -100 - (int)e;
    }
};
} // namespace fvb

// (FVB_SPATIAL_NZ_CASE is the engine's own table entry of a built-in model: the same kernels under the same policies)
#define FABBER_DEVICE_SPATIAL_NOISE_MODEL(NAME, EVAL, NPARAMS, FAMILIES)                                                      \
    static int32_t FABBER_DEVICE_CAT(fabber_device_spatial_noise_launch_, __LINE__)(int32_t kind, int32_t which, int32_t need_f, \
        const void *spatial_args, uint32_t grid, uint32_t lds_bytes, void *stream, char *err, int32_t err_len)                \
    {                                                                                                                         \
        return fvb::LibrarySpatialNoise<EVAL, NPARAMS, (FAMILIES)>::launch(NAME, kind, which, need_f, spatial_args, grid,      \
            lds_bytes, stream, err, err_len);                                                                                 \
    }                                                                                                                         \
    static fvb::DeviceRegistration<fvb_device_spatial_noise_model> FABBER_DEVICE_CAT(fabber_device_spatial_noise_registration_, __LINE__)( \
        fvb_device_spatial_noise_model{ NAME, FVB_ABI_VERSION, (uint32_t)sizeof(fvb::SpatialArgs), NPARAMS, (FAMILIES),        \
            fvb::LibrarySpatialNoise<EVAL, NPARAMS, (FAMILIES)>::state_rows_ar1(),                                            \
            fvb::LibrarySpatialNoise<EVAL, NPARAMS, (FAMILIES)>::state_rows_phis<2>(),                                        \
            fvb::LibrarySpatialNoise<EVAL, NPARAMS, (FAMILIES)>::state_rows_phis<4>(),                                        \
            &FABBER_DEVICE_CAT(fabber_device_spatial_noise_launch_, __LINE__) },                                              \
        NPARAMS, &fabber_vb_register_device_spatial_noise_model, &fabber_vb_unregister_device_spatial_noise_model,            \
        "AR(1) / noise-pattern spatial kernels of ", "under spatial VB with these noise models the model is evaluated on the host");

#endif /* FABBER_DEVICE_SPATIAL_NOISE_MODEL_H */
