/*
 * fabber_device_spatial_wave_noise_model.h - the wave-per-voxel spatial VB kernels for a model library's DEVICE body under
 * a NOISE PATTERN, any parameter count.
 *
 * fabber_device_spatial_wave_model.h compiles the set-up kernel and the second sweep of the wave-per-voxel spatial family
 * around a body for white noise with one precision; fabber_device_spatial_noise_model.h compiles the lane kernels under 2
 * to 4 precisions for 1 to 6 parameters. A model with more parameters - several compartments, several exponentials - and
 * noise-pattern=12... (several echoes, repeats or inversion times, each with its own noise precision) had no spatial
 * kernels at all. This header compiles the same two kernels of the wave-per-voxel family in their form for N = 2 to
 * FVB_MAX_PHIS (8) noise precisions around the SAME body: class moments J'Q_k J, J'Q_k r, r'Q_k r, the residual and the
 * trace per class, one Gamma posterior per class. One line per model, no parameter count:
 *
 *     FABBER_DEVICE_MODEL("multicomp", MultiComp)                                                   // required
 *     FABBER_DEVICE_SPATIAL_WAVE_NOISE_MODEL("multicomp", MultiComp, FVB_SPATIAL_WAVE_NOISE_PHIS)   // noise patterns
 *
 * The first line is required: an entry without a wave body of the same name is never used. The line of
 * fabber_device_spatial_wave_model.h is NOT required (a name without it keeps -40 under white noise with one precision).
 * FAMILIES is a compile-time mask of the noise policies the kernels are compiled for, as in
 * fabber_device_spatial_noise_model.h: FVB_SPATIAL_WAVE_NOISE_PHIS = white noise with 2 to FVB_MAX_PHIS precisions.
 * FVB_SPATIAL_WAVE_NOISE_AR1 is reserved and the engine refuses a mask with it: the family's kernels under AR(1) noise have
 * a header and a registry of their own (fabber_device_spatial_wave_ar_model.h).
 *
 * A name may have lines of fabber_device_spatial_noise_model.h as well: for a parameter count with such a line and 2 to 4
 * precisions the engine takes the lane kernels (spatial<NAME,P,pattern2>), for every other count and for 5 to 8
 * precisions these (the kernel table's name is spatial<NAME,wave,phisN>, N the run's number of precisions). The body is
 * the struct of fabber_device_model.h, unchanged; constants and supplementary rows reach it as on the one-precision route.
 *
 * The state image carries every class's statistics (5 724 rows at 32 parameters and 8 precisions, 46 KB per voxel) and
 * the kernels' LDS is the layout for (P, N) (89.8 KB at 32 parameters and 8 precisions, of 160 KB): the engine refuses a
 * run the device cannot hold, with the figure.
 *
 * The macro, at namespace scope:
 *   - instantiates the set-up kernel and the second sweep with and without the free energy in the form for N classes
 *     (the a_K kernels, the first sweep and the result image are the engine's own for any model);
 *   - defines their launcher in this library's code object. The engine works out the grid - one 64-lane workgroup per
 *     voxel - and the LDS bytes; the launcher answers -40 and starts nothing when they are fewer than this library's
 *     layout for (P, N) needs;
 *   - registers { name, FVB_ABI_VERSION, sizeof(SpatialArgs), sizeof(WaveLayout), the double count of the LDS layout at
 *     FVB_MAX_PARAMS parameters and FVB_MAX_PHIS precisions, mask, launcher } with the engine from a static object whose
 *     destructor unregisters it. A library built against other headers than the engine is refused at registration
 *     (fabber_vb_last_error says why).
 *
 * Compile as fabber_device_model.h says. The remarks there about naming the body struct, linking and unloading apply.
 */
#ifndef FABBER_DEVICE_SPATIAL_WAVE_NOISE_MODEL_H
#define FABBER_DEVICE_SPATIAL_WAVE_NOISE_MODEL_H

#include "fabber_device_registration.h"
#include "../fabber_core_amd/csrc/vb_spatial_wave_model.h"

#include <cstdio>

namespace fvb
{
// the launcher of one body: starts the kernel the engine asks for with the engine's grid and LDS bytes
template <class Eval, int FAMILIES>
int32_t device_spatial_wave_noise_model_launch(int32_t which, int32_t need_f, const void *spatial_args, uint32_t grid, uint32_t lds_bytes,
    void *stream, char *err, int32_t err_len)
{
    const SpatialArgs &sa = *static_cast<const SpatialArgs *>(spatial_args);
    const int P = sa.ka.cfg.n_params, N = sa.ka.cfg.n_phis;
    const bool covered = (FAMILIES & FVB_SPATIAL_WAVE_NOISE_PHIS) != 0 && sa.ka.cfg.noise == FVB_NOISE_WHITE && N >= 2 && N <= FVB_MAX_PHIS;
    // (the kernels place their arrays by this library's layout: never start one with fewer bytes than it addresses)
    if (!covered || P < 1 || P > FVB_MAX_PARAMS || lds_bytes < sp_wave_model_layout(P, N).bytes)
        return device_launch_result(-40, "wave-per-voxel spatial kernels of a device model under a noise pattern: " + std::to_string(P)
                + " parameters and " + std::to_string(N) + " noise precisions with " + std::to_string(lds_bytes)
                + " bytes of LDS is no launch of this family (mask " + std::to_string(FAMILIES) + ")", err, err_len);
    SpatialKernelFn fn = nullptr;
    if constexpr ((FAMILIES & FVB_SPATIAL_WAVE_NOISE_PHIS) != 0)
    {
        switch (which)
        {
        case FVB_SPATIAL_KERNEL_SETUP:
            fn = vb_spatial_wave_classes_setup_kernel<Eval>;
            break;
        case FVB_SPATIAL_KERNEL_NOISE:
            fn = need_f ? (SpatialKernelFn)vb_spatial_wave_classes_noise_kernel<Eval, true>
                        : (SpatialKernelFn)vb_spatial_wave_classes_noise_kernel<Eval, false>;
            break;
        } // (FVB_SPATIAL_KERNEL_NOISE_SPLIT: the family has no split form)
    }
    hipError_t e = hipErrorInvalidValue;
    if (fn)
    {
        e = hipSuccess;
        if (lds_bytes > 64 * 1024) // (more dynamic LDS than a kernel gets without asking)
            e = hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e == hipSuccess)
        {
            hipLaunchKernelGGL(fn, dim3(grid), dim3(64), lds_bytes, static_cast<hipStream_t>(stream), sa);
            e = hipGetLastError();
        }
    }
    if (e != hipSuccess && err && err_len > 0)
        snprintf(err, (size_t)err_len, "wave-per-voxel spatial kernel %d of a device model under a noise pattern: %s", (int)which,
            fn ? hipGetErrorString(e) : "no such kernel");
    return e == hipSuccess ? 0 : -100 - (int)e;
}

// (the entry's key has no parameter count)
inline int32_t unregister_device_spatial_wave_noise_model(const char *name, int32_t)
{
    return fabber_vb_unregister_device_spatial_wave_noise_model(name);
}
} // namespace fvb

#define FABBER_DEVICE_SPATIAL_WAVE_NOISE_MODEL(NAME, EVAL, FAMILIES)                                                           \
    static fvb::DeviceRegistration<fvb_device_spatial_wave_noise_model> FABBER_DEVICE_CAT(fabber_device_spatial_wave_noise_registration_, __LINE__)( \
        fvb_device_spatial_wave_noise_model{ NAME, FVB_ABI_VERSION, (uint32_t)sizeof(fvb::SpatialArgs), (uint32_t)sizeof(fvb::WaveLayout), \
            (uint32_t)fvb::sp_wave_model_layout(FVB_MAX_PARAMS, FVB_MAX_PHIS).n_doubles, (FAMILIES),                           \
            &fvb::device_spatial_wave_noise_model_launch<EVAL, (FAMILIES)> },                                                  \
        0, &fabber_vb_register_device_spatial_wave_noise_model, &fvb::unregister_device_spatial_wave_noise_model,              \
        "wave-per-voxel noise-pattern spatial kernels of ", "under spatial VB with a noise pattern the model has no kernels of this family");

#endif /* FABBER_DEVICE_SPATIAL_WAVE_NOISE_MODEL_H */
