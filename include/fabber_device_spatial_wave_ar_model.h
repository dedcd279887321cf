/*
 * fabber_device_spatial_wave_ar_model.h - the wave-per-voxel spatial VB kernels for a model library's DEVICE body under
 * AR(1) NOISE, any parameter count.
 *
 * fabber_device_spatial_wave_model.h compiles the set-up kernel and the second sweep of the wave-per-voxel spatial family
 * around a body for white noise with one precision, fabber_device_spatial_wave_noise_model.h for noise patterns;
 * fabber_device_spatial_noise_model.h compiles the lane kernels under AR(1) noise for 1 to 6 parameters. A model with more
 * parameters - several compartments, several exponentials - under noise=ar was evaluated by its host code under
 * method=spatialvb. This header compiles the same two kernels in their AR(1) form around the SAME body: one echo, no cross
 * terms (2 AR coefficients of which the first is updated, one noise precision). One line per model, no parameter count:
 *
 *     FABBER_DEVICE_MODEL("multicomp", MultiComp)                  // required
 *     FABBER_DEVICE_SPATIAL_WAVE_AR_MODEL("multicomp", MultiComp)  // spatial VB under AR(1) noise, 1 to FVB_MAX_PARAMS
 *
 * The first line is required: an entry without a wave body of the same name is never used. The lines of
 * fabber_device_spatial_wave_model.h and fabber_device_spatial_wave_noise_model.h are NOT required (a name without them
 * keeps -40 under white noise). A name may have lines of fabber_device_spatial_noise_model.h with FVB_SPATIAL_NOISE_AR1 as
 * well: for a parameter count with such a line the engine takes the lane kernels (spatial<NAME,P,ar1>), for every other
 * count these (the kernel table's name is spatial<NAME,wave,ar1>). Two echoes and ar1-cross-terms other than none keep the
 * host route (-40 from the engine); masked timepoints are refused under AR(1) noise as in the reference. The body is the
 * struct of fabber_device_model.h, unchanged; constants and supplementary rows reach it as on the white-noise route.
 *
 * The state image carries the alpha posterior, the diagonal and lag-1 moments of the linearisation and its first and last
 * rows behind the rows of the one-precision image (2 415 rows at 32 parameters, 19 KB per voxel) and the kernels' LDS is
 * the layout with the AR areas (67.5 KB at 32 parameters, of 160 KB): the engine refuses a run the device cannot hold,
 * with the figure.
 *
 * The macro, at namespace scope:
 *   - instantiates the set-up kernel and the second sweep with and without the free energy in their AR(1) form (the a_K
 *     kernels, the first sweep and the result image are the engine's own for any model);
 *   - defines their launcher in this library's code object. The engine works out the grid - one 64-lane workgroup per
 *     voxel - and the LDS bytes; the launcher answers -40 and starts nothing when they are fewer than this library's
 *     layout for the parameter count needs;
 *   - registers { name, FVB_ABI_VERSION, sizeof(SpatialArgs), sizeof(WaveLayout), the double count of the LDS layout at
 *     FVB_MAX_PARAMS parameters, launcher } with the engine from a static object whose destructor unregisters it. A
 *     library built against other headers than the engine is refused at registration (fabber_vb_last_error says why).
 *
 * Compile as fabber_device_model.h says. The remarks there about naming the body struct, linking and unloading apply.
 */
#ifndef FABBER_DEVICE_SPATIAL_WAVE_AR_MODEL_H
#define FABBER_DEVICE_SPATIAL_WAVE_AR_MODEL_H

#include "fabber_device_registration.h"
#include "../fabber_core_amd/csrc/vb_spatial_wave_ar.h"

#include <cstdio>

namespace fvb
{
// the launcher of one body: starts the kernel the engine asks for with the engine's grid and LDS bytes
template <class Eval>
int32_t device_spatial_wave_ar_model_launch(int32_t which, int32_t need_f, const void *spatial_args, uint32_t grid, uint32_t lds_bytes,
    void *stream, char *err, int32_t err_len)
{
    const SpatialArgs &sa = *static_cast<const SpatialArgs *>(spatial_args);
    const int P = sa.ka.cfg.n_params;
    const bool covered = sa.ka.cfg.noise == FVB_NOISE_AR1 && sa.ka.cfg.n_phis == 1 && sa.ka.cfg.ar_cross_terms == 0;
    // (the kernels place their arrays by this library's layout: never start one with fewer bytes than it addresses)
    if (!covered || P < 1 || P > FVB_MAX_PARAMS || lds_bytes < sp_wave_ar_model_layout(P).bytes)
        return device_launch_result(-40, "wave-per-voxel spatial kernels of a device model under AR(1) noise: " + std::to_string(P)
                + " parameters with " + std::to_string(lds_bytes) + " bytes of LDS is no launch of this family (one echo, no cross terms)",
            err, err_len);
    SpatialKernelFn fn = nullptr;
    switch (which)
    {
    case FVB_SPATIAL_KERNEL_SETUP:
        fn = vb_spatial_wave_ar_setup_kernel<Eval>;
        break;
    case FVB_SPATIAL_KERNEL_NOISE:
        fn = need_f ? (SpatialKernelFn)vb_spatial_wave_ar_noise_kernel<Eval, true> : (SpatialKernelFn)vb_spatial_wave_ar_noise_kernel<Eval, false>;
        break;
    } // (FVB_SPATIAL_KERNEL_NOISE_SPLIT: the family has no split form)
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
        snprintf(err, (size_t)err_len, "wave-per-voxel spatial kernel %d of a device model under AR(1) noise: %s", (int)which,
            fn ? hipGetErrorString(e) : "no such kernel");
    return e == hipSuccess ? 0 : -100 - (int)e;
}

// (the entry's key has no parameter count)
inline int32_t unregister_device_spatial_wave_ar_model(const char *name, int32_t)
{
    return fabber_vb_unregister_device_spatial_wave_ar_model(name);
}
} // namespace fvb

#define FABBER_DEVICE_SPATIAL_WAVE_AR_MODEL(NAME, EVAL)                                                                        \
    static fvb::DeviceRegistration<fvb_device_spatial_wave_ar_model> FABBER_DEVICE_CAT(fabber_device_spatial_wave_ar_registration_, __LINE__)( \
        fvb_device_spatial_wave_ar_model{ NAME, FVB_ABI_VERSION, (uint32_t)sizeof(fvb::SpatialArgs), (uint32_t)sizeof(fvb::WaveLayout), \
            (uint32_t)fvb::sp_wave_ar_model_layout(FVB_MAX_PARAMS).n_doubles, &fvb::device_spatial_wave_ar_model_launch<EVAL> }, \
        0, &fabber_vb_register_device_spatial_wave_ar_model, &fvb::unregister_device_spatial_wave_ar_model,                    \
        "wave-per-voxel AR(1) spatial kernels of ", "under spatial VB with AR(1) noise the model has no kernels of this family");

#endif /* FABBER_DEVICE_SPATIAL_WAVE_AR_MODEL_H */
