/*
 * fabber_device_spatial_model.h - the spatial VB kernels for a model library's DEVICE body.
 *
 * fabber_device_model.h and fabber_device_lane_model.h give a body the kernels of voxelwise VB. Under method=spatialvb
 * such a model was evaluated by its host code: every iteration downloaded the means, ran 2 P + 1 Evaluate calls per voxel
 * on host threads and uploaded the linearisations. Of the spatial family only two kernels evaluate the model - the set-up
 * kernel and the second sweep (noise update, re-centre, free energy); the a_K kernels, the first sweep in both of its
 * forms and the result image are the engine's own for any model. This header compiles those two around the SAME body,
 * for one parameter count per macro line:
 *
 *     FABBER_DEVICE_MODEL("invrec", InvRec)             // the wave kernels: required, the route of voxelwise VB
 *     FABBER_DEVICE_SPATIAL_MODEL("invrec", InvRec, 3)  // spatial VB with exactly 3 parameters
 *
 * Several lines per name are allowed, each for 1 <= P <= 6 (the range of the library lane kernels). The first line is
 * required: a spatial entry without a wave body of the same name is never used. It is a header of its own because it
 * includes the spatial kernels: a library that does not want them does not pay for them. Compile as fabber_device_model.h
 * says; a macro line takes some tens of seconds.
 *
 * The body is the struct of fabber_device_model.h, unchanged, with eval declared __forceinline__ (see
 * fabber_device_lane_model.h: the kernels are one lane per voxel and keep the parameter vector in registers).
 *
 * The engine takes these kernels for a configuration when an entry for (name, n_params) is registered and the noise is
 * white with one precision; the kernel table's name is spatial<NAME,P>. Noise patterns of 2 to 4 precisions and AR(1)
 * noise with one echo are a macro line of fabber_device_spatial_noise_model.h (FABBER_DEVICE_SPATIAL_NOISE_MODEL); without
 * it they, and in any case two echoes, 5 to 8 precisions and a volume cut into z-slabs over several devices, keep the host
 * route (-40 from the engine, after which method=spatialvb evaluates the model's host code as before). Other parameter
 * counts keep it too unless the library has the line of fabber_device_spatial_wave_model.h (FABBER_DEVICE_SPATIAL_WAVE_MODEL:
 * one wavefront per voxel, any count up to FVB_MAX_PARAMS under white noise with one precision; an entry of THIS header
 * for the run's count comes first). A body that reads the voxel's supplementary data (fvb::supp_at, spec.uses_suppdata) receives the rows of
 * the voxel its lane works on, as in the kernels of voxelwise VB. The initial posterior is an image (init_mvn): these
 * kernels know no library's InitVoxelPosterior. It comes from the model's host code, or - where the library also uses the
 * macro of fabber_device_init_model.h - from the kernel the engine launches ahead of the set-up kernel. The body is evaluated pointwise, as in the lane kernels.
 *
 * The macro, at namespace scope:
 *   - instantiates five kernels for the body: the set-up kernel and the second sweep with and without the free energy,
 *     each in the plain form and in the form that completes the split first sweep;
 *   - defines their launcher in this library's code object (the engine works out the grid and the LDS bytes, the launcher
 *     starts the kernel it is asked for; no device function crosses a code object);
 *   - registers { name, FVB_ABI_VERSION, sizeof(SpatialArgs), P, rows of the state image, launcher } with the engine from
 *     a static object whose destructor unregisters it. A refused registration (fabber_vb_last_error says why) leaves the
 *     model on the host route under spatial VB.
 *
 * vb_spatial.h defines templates and inline functions only: a library may include this header in several of its
 * sources. The remarks of fabber_device_model.h about naming the body struct, linking and unloading apply.
 */
#ifndef FABBER_DEVICE_SPATIAL_MODEL_H
#define FABBER_DEVICE_SPATIAL_MODEL_H

#include "fabber_device_lane_model.h" /* fvb::LibraryLane: the body as a model of the lane-per-voxel kernels */
#include "../fabber_core_amd/csrc/vb_spatial.h"

#include <cstdio>

namespace fvb
{
// the launcher of one (body, P): starts the kernel the engine asks for with the engine's grid and LDS bytes
template <class Model, int P>
int32_t device_spatial_model_launch(int32_t which, int32_t need_f, const void *spatial_args, uint32_t grid, uint32_t lds_bytes,
    void *stream, char *err, int32_t err_len)
{
    const SpatialArgs &sa = *static_cast<const SpatialArgs *>(spatial_args);
    SpatialKernelFn fn = nullptr;
    switch (which)
    {
    case FVB_SPATIAL_KERNEL_SETUP:
        fn = vb_spatial_setup_kernel<Model, P>;
        break;
    case FVB_SPATIAL_KERNEL_NOISE:
        fn = need_f ? (SpatialKernelFn)vb_spatial_noise_kernel<Model, P, true> : (SpatialKernelFn)vb_spatial_noise_kernel<Model, P, false>;
        break;
    case FVB_SPATIAL_KERNEL_NOISE_SPLIT:
        fn = need_f ? (SpatialKernelFn)vb_spatial_noise_kernel<Model, P, true, true>
                    : (SpatialKernelFn)vb_spatial_noise_kernel<Model, P, false, true>;
        break;
    }
    hipError_t e = hipErrorInvalidValue;
    if (fn)
    {
        hipLaunchKernelGGL(fn, dim3(grid), dim3(64), lds_bytes, static_cast<hipStream_t>(stream), sa);
        e = hipGetLastError();
    }
    if (e != hipSuccess && err && err_len > 0)
        snprintf(err, (size_t)err_len, "spatial kernel %d of a device model: %s", (int)which, fn ? hipGetErrorString(e) : "no such kernel");
    return e == hipSuccess ? 0 : -100 - (int)e;
}
} // namespace fvb

#define FABBER_DEVICE_SPATIAL_MODEL(NAME, EVAL, NPARAMS)                                                                     \
    static_assert((NPARAMS) >= 1 && (NPARAMS) <= 6, "FABBER_DEVICE_SPATIAL_MODEL: the spatial kernels of a library body exist for 1 to 6 parameters"); \
    static fvb::DeviceRegistration<fvb_device_spatial_model> FABBER_DEVICE_CAT(fabber_device_spatial_registration_, __LINE__)( \
        fvb_device_spatial_model{ NAME, FVB_ABI_VERSION, (uint32_t)sizeof(fvb::SpatialArgs), NPARAMS, fvb::SpLayout<NPARAMS>::ROWS, \
            &fvb::device_spatial_model_launch<fvb::LibraryLane<EVAL>::Model<NPARAMS>, NPARAMS> },                              \
        NPARAMS, &fabber_vb_register_device_spatial_model, &fabber_vb_unregister_device_spatial_model, "spatial kernels of ",  \
        "under spatial VB the model is evaluated on the host");

#endif /* FABBER_DEVICE_SPATIAL_MODEL_H */
