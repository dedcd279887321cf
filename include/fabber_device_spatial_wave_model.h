/*
 * fabber_device_spatial_wave_model.h - the spatial VB kernels for a model library's DEVICE body with any parameter count.
 *
 * fabber_device_spatial_model.h compiles the spatial kernels that keep one voxel per lane around a body, one macro line
 * per parameter count from 1 to 6. The models with more parameters - several compartments, several exponentials - were
 * evaluated by their host code under method=spatialvb: every iteration downloaded the means, ran 2 P + 1 Evaluate calls
 * per voxel on host threads and uploaded a [voxels][timepoints][P + 1] linearisation. This header compiles the two kernels
 * of the WAVE-per-voxel spatial family that read the model's linearisation - the set-up kernel and the second sweep
 * (noise update, re-centre, free energy) - around the SAME body, which they linearise in the kernel by the reference's
 * central differences. The parameter count is a runtime value of this family, so there is one line per model and no count:
 *
 *     FABBER_DEVICE_MODEL("multicomp", MultiComp)               // the wave kernels: required, the route of voxelwise VB
 *     FABBER_DEVICE_SPATIAL_WAVE_MODEL("multicomp", MultiComp)  // spatial VB, 1 to FVB_MAX_PARAMS (32) parameters
 *
 * The first line is required: a spatial entry without a wave body of the same name is never used. A name may have lines
 * of fabber_device_spatial_model.h as well: for a parameter count with such a line the engine takes the lane kernels
 * (spatial<NAME,P>, the split first sweep), for every other count these (the kernel table's name is spatial<NAME,wave>).
 * The body is the struct of fabber_device_model.h, unchanged. It is evaluated with one timepoint per lane, 64 timepoints at
 * a time, from parameter vectors in LDS; it receives the model's constants and, with spec.uses_suppdata, the supplementary
 * rows of the voxel the wavefront works on.
 *
 * The engine takes these kernels under white noise with one precision. Noise patterns of 2 to 8 precisions have a line of
 * their own (fabber_device_spatial_wave_noise_model.h: the same two kernels in their form for several precisions; a name
 * with this line alone keeps -40 under a pattern), and so has AR(1) noise with one echo and no cross terms
 * (fabber_device_spatial_wave_ar_model.h). AR(1) noise with two echoes or cross terms, a volume cut into z-slabs over
 * several devices and more than FVB_MAX_PARAMS parameters keep the host route (-40 from the engine, after which method=spatialvb evaluates the
 * model's host code as before). The initial posterior is an image (init_mvn): from
 * the library's kernel for it where the library uses the macro of fabber_device_init_model.h, else from the model's host
 * code.
 *
 * The macro, at namespace scope:
 *   - instantiates the set-up kernel and the second sweep with and without the free energy for the body (the a_K kernels,
 *     the first sweep and the result image are the engine's own for any model);
 *   - defines their launcher in this library's code object (the engine works out the grid - one 64-lane workgroup per
 *     voxel - and the LDS bytes; no device function crosses a code object);
 *   - registers { name, FVB_ABI_VERSION, sizeof(SpatialArgs), sizeof(WaveLayout), the double count of the family's LDS
 *     layout at FVB_MAX_PARAMS parameters, launcher } with the engine from a static object whose destructor unregisters
 *     it. A library built against other headers than the engine is refused at registration (fabber_vb_last_error says
 *     why) and the model stays on the host route under spatial VB.
 *
 * Compile as fabber_device_model.h says. The remarks there about naming the body struct, linking and unloading apply.
 */
#ifndef FABBER_DEVICE_SPATIAL_WAVE_MODEL_H
#define FABBER_DEVICE_SPATIAL_WAVE_MODEL_H

#include "fabber_device_registration.h"
#include "../fabber_core_amd/csrc/vb_spatial_wave_model.h"

#include <cstdio>

namespace fvb
{
// the launcher of one body: starts the kernel the engine asks for with the engine's grid and LDS bytes
template <class Eval>
int32_t device_spatial_wave_model_launch(int32_t which, int32_t need_f, const void *spatial_args, uint32_t grid, uint32_t lds_bytes,
    void *stream, char *err, int32_t err_len)
{
    const SpatialArgs &sa = *static_cast<const SpatialArgs *>(spatial_args);
    const int P = sa.ka.cfg.n_params;
    // (the kernels place their arrays by this library's layout: never start one with fewer bytes than it addresses)
    if (P < 1 || P > FVB_MAX_PARAMS || lds_bytes < sp_wave_model_layout(P).bytes)
        return device_launch_result(-40, "wave-per-voxel spatial kernels of a device model: " + std::to_string(P) + " parameters with "
                + std::to_string(lds_bytes) + " bytes of LDS is no launch of this family", err, err_len);
    SpatialKernelFn fn = nullptr;
    switch (which)
    {
    case FVB_SPATIAL_KERNEL_SETUP:
        fn = vb_spatial_wave_setup_kernel<Eval>;
        break;
    case FVB_SPATIAL_KERNEL_NOISE:
        fn = need_f ? (SpatialKernelFn)vb_spatial_wave_noise_kernel<Eval, true> : (SpatialKernelFn)vb_spatial_wave_noise_kernel<Eval, false>;
        break;
    } // (FVB_SPATIAL_KERNEL_NOISE_SPLIT: the family has no split form)
    hipError_t e = hipErrorInvalidValue;
    if (fn)
    {
        hipLaunchKernelGGL(fn, dim3(grid), dim3(64), lds_bytes, static_cast<hipStream_t>(stream), sa);
        e = hipGetLastError();
    }
    if (e != hipSuccess && err && err_len > 0)
        snprintf(err, (size_t)err_len, "wave-per-voxel spatial kernel %d of a device model: %s", (int)which, fn ? hipGetErrorString(e) : "no such kernel");
    return e == hipSuccess ? 0 : -100 - (int)e;
}

// (the entry's key has no parameter count)
inline int32_t unregister_device_spatial_wave_model(const char *name, int32_t)
{
    return fabber_vb_unregister_device_spatial_wave_model(name);
}
} // namespace fvb

#define FABBER_DEVICE_SPATIAL_WAVE_MODEL(NAME, EVAL)                                                                           \
    static fvb::DeviceRegistration<fvb_device_spatial_wave_model> FABBER_DEVICE_CAT(fabber_device_spatial_wave_registration_, __LINE__)( \
        fvb_device_spatial_wave_model{ NAME, FVB_ABI_VERSION, (uint32_t)sizeof(fvb::SpatialArgs), (uint32_t)sizeof(fvb::WaveLayout), \
            (uint32_t)fvb::sp_wave_model_layout(FVB_MAX_PARAMS).n_doubles, &fvb::device_spatial_wave_model_launch<EVAL> },     \
        0, &fabber_vb_register_device_spatial_wave_model, &fvb::unregister_device_spatial_wave_model,                          \
        "wave-per-voxel spatial kernels of ", "under spatial VB the model is evaluated on the host");

#endif /* FABBER_DEVICE_SPATIAL_WAVE_MODEL_H */
