/*
 * fabber_device_init_model.h - the initial posterior of a model library's DEVICE body on the device.
 *
 * The other headers of this family give a body the kernels that fit and the result-image kernel
 * (fabber_device_model.h, fabber_device_lane_model.h, fabber_device_lane_noise_model.h, fabber_device_nlls_model.h,
 * fabber_device_spatial_model.h, fabber_device_results_model.h). Those kernels know no library's InitVoxelPosterior:
 * without this header a fit with FVB_MODEL_PLUGIN needs the initial posterior as fvb_config.init_mvn, which
 * fabber_dorun builds on the host - PassData, GetInitialPosterior and a scatter, one voxel after the other on one
 * thread. This header compiles the engine's initial-posterior kernel (one lane per voxel, any parameter count) around
 * the body:
 *
 *     FABBER_DEVICE_MODEL("invrec", InvRec)       // the wave kernels: required
 *     FABBER_DEVICE_INIT_MODEL("invrec", InvRec)  // the initial posterior on the device
 *
 * One line per model. The first line is required: an init entry without a wave body of the same name is never used.
 * Compile as fabber_device_model.h says; a macro line takes a few seconds.
 *
 * The body is the struct of fabber_device_model.h with one more static member next to eval:
 *
 *     // M0 starts at the largest magnitude of the series
 *     static __device__ void init_posterior(const fvb::ModelArgs &a, int P, const fvb::VoxelSeries &y, double *means, double *vars)
 *     {
 *         double m = 0;
 *         for (int t = 0; t < y.T; t++)
 *             m = fabs(y(t)) > m ? fabs(y(t)) : m;
 *         if (m > 0)
 *             means[0] = m;
 *     }
 *
 * y(t), t = 0 .. y.T - 1, is the voxel's series read in place (float or double, converted to double): all samples, the
 * masked timepoints included, as FwdModel::PassData hands them to the host code. On entry means[i] and vars[i],
 * i = 0 .. P - 1, hold what FwdModel::GetInitialPosterior sets before it calls InitVoxelPosterior, in MODEL space: the
 * mean is the image prior's value at this voxel where the parameter's prior type is an image, else the mean of the
 * parameter's initial posterior; the variance is that posterior's. The hook overwrites what the model's host
 * InitVoxelPosterior overwrites - WITH THE SAME OPERATIONS IN THE SAME ORDER, comparisons included (a NaN sample is
 * skipped by `x > m` and taken by `!(x <= m)`): the two routes then start from the same bits up to the logarithm of
 * the LOG and FRACTIONAL transforms, which the kernel applies afterwards (FwdModel::ToFabber). a.consts / a.n_consts are
 * the model's constants, as in eval; the hook never reads past them. The voxel's supplementary data (the `suppdata`
 * option; DeviceModelSpec::uses_suppdata) is there too, as in eval: fvb::supp_at(a, k) for k < a.n_supp, which is 0
 * where the run has none.
 *
 * What the hook cannot express: the off-diagonal covariances of the parameters (the image has zeros there) and the
 * voxel's co-ordinates. A model whose InitVoxelPosterior needs one of them brings NO init entry: the
 * engine then answers a fit without init_mvn with -52 as before, and fabber_dorun builds the image from the model's host
 * code as before.
 *
 * With an entry registered, fabber_vb_run_device / _run_host / _run_host_multi and fabber_vb_run_spatial_* accept a
 * configuration that names the body (FVB_MODEL_PLUGIN) WITHOUT init_mvn: the kernel writes the image into a work buffer
 * of the run, on the run's stream, ahead of the fit. A given init_mvn (continue-from-mvn) always wins, and the entry is
 * then not consulted. fabber_vb_init_posterior_device / _host write the image alone;
 * fabber_vb_init_posterior_kernel_name says "init<NAME>". method=nlls starts from the parameters' initial posterior and
 * the host-model routes from the host code: neither uses the entry.
 *
 * The macro, at namespace scope, once per model:
 *   - instantiates the kernel for the body, for up to FVB_MAX_PARAMS and up to FVB_MAX_PARAMS_EXT parameters;
 *   - defines its launcher in this library's code object (grid, launch, the engine's error texts; no device function
 *     crosses a code object);
 *   - registers { name, FVB_ABI_VERSION, sizeof(fvb_config), launcher } with the engine from a static object whose
 *     destructor unregisters it. A refused registration (fabber_vb_last_error says why) leaves the initial posterior to
 *     the model's host code.
 *
 * vb_init_kernel.h defines templates and inline functions only: a library may include this header in several of its
 * sources. The remarks of fabber_device_model.h about naming the body struct, linking and unloading apply.
 */
#ifndef FABBER_DEVICE_INIT_MODEL_H
#define FABBER_DEVICE_INIT_MODEL_H

#include "fabber_device_registration.h"
#include "../fabber_core_amd/csrc/vb_init_kernel.h"

namespace fvb
{
// the launcher of one body: the engine's arguments as fabber_vb_init_posterior_device validated them
template <class Body>
int32_t device_init_model_launch(const fvb_config *cfg, const void *data, double *init_mvn, void *stream, char *err, int32_t err_len)
{
    if (!cfg || !data || !init_mvn)
        return device_launch_result(-22, "configuration, data or the image to write are NULL", err, err_len);
    if (cfg->n_voxels <= 0)
        return 0;
    const hipError_t e = launch_init_posterior<Body>(*cfg, data, init_mvn, static_cast<hipStream_t>(stream));
    return device_launch_result(e == hipSuccess ? 0 : -100 - (int)e, std::string("launching the initial-posterior kernel: ") + hipGetErrorString(e),
        err, err_len);
}

// (the key of an init entry has no parameter count)
inline int32_t unregister_device_init_model(const char *name, int32_t)
{
    return fabber_vb_unregister_device_init_model(name);
}
} // namespace fvb

#define FABBER_DEVICE_INIT_MODEL(NAME, BODY)                                                                              \
    static fvb::DeviceRegistration<fvb_device_init_model> FABBER_DEVICE_CAT(fabber_device_init_registration_, __LINE__)(  \
        fvb_device_init_model{ NAME, FVB_ABI_VERSION, (uint32_t)sizeof(fvb_config), &fvb::device_init_model_launch<BODY> }, \
        0, &fabber_vb_register_device_init_model, &fvb::unregister_device_init_model, "initial-posterior kernel of ",     \
        "the initial posterior comes from the model's host code");

#endif /* FABBER_DEVICE_INIT_MODEL_H */
