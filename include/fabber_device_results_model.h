/*
 * fabber_device_results_model.h - model fit and residuals from a model library's DEVICE body.
 *
 * The other headers of this family give a body the kernels that FIT (fabber_device_model.h, fabber_device_lane_model.h,
 * fabber_device_nlls_model.h, fabber_device_spatial_model.h). The result images save-model-fit and save-residuals are
 * one more evaluation of the model per voxel and timepoint, at the posterior means; without this header they come from
 * the model's host code, one voxel after the other. This header compiles the engine's result-image kernel (one lane per
 * voxel, any parameter count) around the SAME body:
 *
 *     FABBER_DEVICE_MODEL("invrec", InvRec)          // the wave kernels: required
 *     FABBER_DEVICE_RESULTS_MODEL("invrec", InvRec)  // model fit and residuals on the device
 *
 * One line per model. The first line is required: a results entry without a wave body of the same name is never used.
 * Compile as fabber_device_model.h says; a macro line takes a few seconds.
 *
 * The body is the struct of fabber_device_model.h, unchanged. It is evaluated at the model-space posterior means for
 * t = 0 .. n_times - 1; whatever it returns is the image value, a non-finite prediction included (the residual is then
 * non-finite too). The body's own guard - `if (t >= a.n_consts) return NaN` - is what keeps its reads inside the
 * constants block: the engine does not know how many constants a body needs.
 *
 * With an entry registered, fabber_vb_postproc_host / _device compute modelfit and residuals of a configuration that names
 * the body (FVB_MODEL_PLUGIN) - fabber_vb_postproc_kernel_name says "postproc<NAME>" - and method=vb, spatialvb and nlls
 * take the two images from there, also where the fit itself ran on the model's host code (a library without spatial
 * kernels or minimisers). Without one the engine refuses such a request (-85) and the host code provides the images, as
 * it does with the host-model option. save-model-extras stays host code; the initial posterior too, without the macro
 * of fabber_device_init_model.h.
 *
 * The macro, at namespace scope, once per model:
 *   - instantiates the kernel for the body, for up to FVB_MAX_PARAMS and up to FVB_MAX_PARAMS_EXT parameters;
 *   - defines its launcher in this library's code object (grid, launch, the engine's error texts; no device function
 *     crosses a code object);
 *   - registers { name, FVB_ABI_VERSION, sizeof(fvb_config), sizeof(fvb_postproc), launcher } with the engine from a static
 *     object whose destructor unregisters it. A refused registration (fabber_vb_last_error says why) leaves the two images
 *     to the host code.
 *
 * vb_postproc_kernel.h defines templates and inline functions only: a library may include this header in several of its
 * sources. The remarks of fabber_device_model.h about naming the body struct, linking and unloading apply.
 */
#ifndef FABBER_DEVICE_RESULTS_MODEL_H
#define FABBER_DEVICE_RESULTS_MODEL_H

#include "fabber_device_registration.h"
#include "../fabber_core_amd/csrc/vb_postproc_kernel.h"

namespace fvb
{
// the launcher of one body: the engine's arguments as fabber_vb_postproc_device validated them
template <class Eval>
int32_t device_results_model_launch(const fvb_config *cfg, const void *data, const double *mvn, const fvb_postproc *pp, int32_t n_noise,
    void *stream, char *err, int32_t err_len)
{
    if (!cfg || !mvn || !pp)
        return device_launch_result(-22, "configuration, mvn or postproc outputs are NULL", err, err_len);
    if (cfg->n_voxels <= 0)
        return 0;
    const hipError_t e = launch_postproc<Eval>(*cfg, data, mvn, *pp, n_noise, static_cast<hipStream_t>(stream));
    return device_launch_result(e == hipSuccess ? 0 : -100 - (int)e, std::string("launching the result-image kernel: ") + hipGetErrorString(e), err,
        err_len);
}

// (the key of a results entry has no parameter count)
inline int32_t unregister_device_results_model(const char *name, int32_t)
{
    return fabber_vb_unregister_device_results_model(name);
}
} // namespace fvb

#define FABBER_DEVICE_RESULTS_MODEL(NAME, EVAL)                                                                                \
    static fvb::DeviceRegistration<fvb_device_results_model> FABBER_DEVICE_CAT(fabber_device_results_registration_, __LINE__)( \
        fvb_device_results_model{ NAME, FVB_ABI_VERSION, (uint32_t)sizeof(fvb_config), (uint32_t)sizeof(fvb_postproc),          \
            &fvb::device_results_model_launch<EVAL> },                                                                          \
        0, &fabber_vb_register_device_results_model, &fvb::unregister_device_results_model, "result-image kernel of ",          \
        "model fit and residuals come from the model's host code");

#endif /* FABBER_DEVICE_RESULTS_MODEL_H */
