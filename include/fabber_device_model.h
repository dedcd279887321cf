/*
 * fabber_device_model.h - give a forward model of a model library a DEVICE body.
 *
 * A model library is loaded at run time and its models are evaluated on the host unless the library also supplies
 * a body the engine's kernels can call. Device functions cannot be called across code objects, so the library does
 * not hand over a function: it compiles the engine's wave-per-voxel kernels (one wavefront per voxel, any parameter
 * count, white noise with any pattern and AR(1) noise) around its own evaluator into its OWN code object, and registers
 * a host launcher for them. This header is HIP C++: compile the file that uses it with
 *
 *     hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -fno-fast-math -I <this directory> ...
 *
 * The body is a stateless struct:
 *
 *     struct InvRec
 *     {
 *         // prediction at timepoint index t (0-based) for MODEL-space parameters p[0 .. P-1], i.e. what
 *         // FwdModel::EvaluateModel receives after the parameter transforms
 *         static __device__ double eval(const fvb::ModelArgs &a, int P, int t, const double *p)
 *         {
 *             FVB_MODEL_FP // the floating-point contraction setting of the built-in bodies
 *             if (t >= a.n_consts) // the engine does not know how many constants a body needs: the body never reads
 *                 return __builtin_nan(""); // past the block (a non-finite prediction stops the voxel with its status)
 *             return p[0] * (1.0 - 2.0 * p[2] * exp(-a.consts[t] / p[1]));
 *         }
 *     };
 *     FABBER_DEVICE_MODEL("invrec", InvRec)
 *
 * a.consts / a.n_consts are the model's constants (a list of inversion times, a dose, a TR): read-only device memory,
 * the same for every voxel, filled from DeviceModelSpec::constants (fvb_config.model_consts).
 *
 * a.supp / a.n_supp / a.supp_stride are THIS voxel's supplementary data - the `suppdata` option of a run, what the host
 * class finds in FwdModel::suppdata after PassData: a per-voxel input curve (a voxelwise arterial input function, a
 * reference curve), a per-voxel B1 or T1 that is not a parameter. Read entry k with the accessor
 *
 *     fvb::supp_at(a, k)      // = a.supp[k * a.supp_stride], a double; k = 0 .. a.n_supp - 1
 *
 * under the rule of the constants: the engine does not know how many rows a body needs, so the body checks
 * k < a.n_supp itself and answers a non-finite prediction instead of reading past the block (a.supp is NULL and
 * a.n_supp 0 where a run has no supplementary data):
 *
 *         if (t >= a.n_supp)
 *             return __builtin_nan("");
 *         return p[0] * fvb::supp_at(a, t) * exp(-p[1] * double(t) * a.dopt0);
 *
 * The rows are read-only device memory laid out [row][voxel] (fvb_config.model_supp, n_model_supp): in the lane kernels
 * a read is one coalesced 8-byte load per lane, in the wave kernels one load of an address that is the same for the
 * whole wavefront. The host side asks for them with spec.uses_suppdata = true (DeviceModelSpec); the engine then hands
 * the body the run's supplementary data, all rows, on every route of this family of headers, spatial VB included: the
 * kernels of fabber_device_spatial_model.h and fabber_device_spatial_noise_model.h set them for the voxel their lane
 * works on, those of fabber_device_spatial_wave_model.h for the voxel of their wavefront. Without the spatial line for the run's parameter count and noise model, method=spatialvb runs such a model
 * on the host route (the log says so).
 *
 * The expression must be
 * the one the model's host EvaluateModel computes - the host code still provides the initial posterior unless the
 * library also uses the macro of fabber_device_init_model.h, the extra outputs of save-model-extras, model fit and
 * residuals unless the library also uses the macro of fabber_device_results_model.h, and the whole fit wherever the device body is not used (the host-model option, spatial
 * VB unless the library also uses the macros of fabber_device_spatial_model.h / fabber_device_spatial_noise_model.h /
 * fabber_device_spatial_wave_model.h, and method=nlls unless it uses those of
 * fabber_device_nlls_model.h).
 *
 * The macro, at namespace scope, once per model:
 *   - instantiates the white-noise kernel (with and without the free energy) and the four AR(1) kernels for the body;
 *   - defines the launcher (LDS attribute above 64 KB, one workgroup per voxel, the engine's error texts);
 *   - registers { name, FVB_ABI_VERSION, sizeof(KernelArgs), sizeof(WaveLayout), launcher } with the engine from a
 *     static object whose destructor unregisters it. A library built against other headers than the engine is refused
 *     at registration (fabber_vb_last_error says why) and its models run on the host.
 *
 * Name the body struct uniquely or put it in an anonymous namespace: the kernels and the launcher are template
 * instantiations on it, and two libraries in one process whose bodies share a global name would share those symbols
 * (the first loaded wins). Link the library against the engine library the process uses - another copy of it has
 * another registry - and keep it loaded while a run that uses the body is under way.
 *
 * The host side of the model announces the body through FwdModel::GetDeviceModel: spec.device_model = "invrec",
 * spec.constants = the constants.
 *
 * The lane-per-voxel kernels (one voxel per lane: the engine's throughput kernels, for white noise with one precision
 * from a few thousand voxels up) are compiled around the same body by fabber_device_lane_model.h, one macro line per
 * parameter count, next to the line above. The NLLS minimisers of method=nlls (one wavefront or one lane per voxel, the
 * whole minimisation in one launch) are compiled around it by fabber_device_nlls_model.h in the same way, the two
 * kernels of spatial VB that evaluate the model by fabber_device_spatial_model.h (white noise with one precision) and
 * fabber_device_spatial_noise_model.h (AR(1) noise, noise patterns) for 1 to 6 parameters and by
 * fabber_device_spatial_wave_model.h for any count up to FVB_MAX_PARAMS (one wavefront per voxel, white noise with one
 * precision), and the result-image kernel (model fit
 * and residuals) by fabber_device_results_model.h, and the initial-posterior kernel - around one more member of the body,
 * init_posterior - by fabber_device_init_model.h.
 */
#ifndef FABBER_DEVICE_MODEL_H
#define FABBER_DEVICE_MODEL_H

#include "fabber_device_registration.h"
#include "../fabber_core_amd/csrc/vb_wave_launch.h"

namespace fvb
{
template <class Eval>
int32_t device_model_launch(const void *kernel_args, void *stream, char *err, int32_t err_len)
{
    static const WaveKernelSet set = wave_model_kernels<Eval>();
    std::string msg;
    const int rc = launch_wave_set(set, *static_cast<const KernelArgs *>(kernel_args), static_cast<hipStream_t>(stream), msg);
    return device_launch_result(rc, msg, err, err_len);
}

// (the wave body's key has no parameter count)
inline int32_t unregister_device_model(const char *name, int32_t)
{
    return fabber_vb_unregister_device_model(name);
}
} // namespace fvb

#define FABBER_DEVICE_MODEL(NAME, EVAL)                                                                                        \
    static fvb::DeviceRegistration<fvb_device_model> FABBER_DEVICE_CAT(fabber_device_model_registration_, __LINE__)(           \
        fvb_device_model{ NAME, FVB_ABI_VERSION, (uint32_t)sizeof(fvb::KernelArgs), (uint32_t)sizeof(fvb::WaveLayout),          \
            &fvb::device_model_launch<EVAL> },                                                                                  \
        0, &fabber_vb_register_device_model, &fvb::unregister_device_model, "", "the model runs on the host");

#endif /* FABBER_DEVICE_MODEL_H */
