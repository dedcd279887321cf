/*
 * fabber_device_nlls_model.h - the NLLS minimisers (method=nlls) for a model library's DEVICE body.
 *
 * fabber_device_model.h gives a body the wave-per-voxel VB kernels and fabber_device_lane_model.h the lane-per-voxel
 * ones; under method=nlls such a model is still evaluated on the host - one kernel launch per trial point, the
 * linearisations computed by host threads and uploaded for every step - unless its library also compiles the engine's
 * NLLS minimisers (csrc/vb_nlls_kernel.h: the whole minimisation of every voxel in ONE launch) around the SAME body:
 *
 *     FABBER_DEVICE_MODEL("invrec", InvRec)               // the wave VB kernels: required, as before
 *     FABBER_DEVICE_NLLS_MODEL("invrec", InvRec)          // the wave-per-voxel minimiser, any parameter count
 *     FABBER_DEVICE_NLLS_LANE_MODEL("invrec", InvRec, 3)  // the lane-per-voxel minimiser for exactly 3 parameters
 *
 * Several lane lines per name are allowed (a model with a variable parameter count names the counts worth having), each
 * for 1 <= P <= 6. The first two lines are required: method=nlls takes the device route only for a name that has a body
 * in the registry of FABBER_DEVICE_MODEL and the wave minimiser, and a lane entry without the wave minimiser is never
 * used. It is a header of its own because it includes the NLLS kernels: a library that does not want them does not pay
 * for them, and behaves exactly as before (method=nlls on the host route, -61 from fabber_nlls_run_host).
 * Compile as fabber_device_model.h says.
 *
 * The body is the struct of fabber_device_model.h, unchanged:
 *
 *     static __device__ __forceinline__ double eval(const fvb::ModelArgs &a, int P, int t, const double *p)
 *
 * Declare eval __forceinline__. The lane minimiser keeps a voxel's parameter vector in registers and calls eval 2 P + 1
 * times per timepoint; a body that is not inlined receives it through a pointer, which puts the vector into scratch
 * memory for every call. Inlined, P is a constant and loops over it unroll.
 *
 * The engine takes the lane minimiser under the rule of the built-in models: a lane entry for (name, n_params) is
 * registered, the kernel variant is not `wave`, and the variant is `lane`, or there are at least 4096 voxels, or the series
 * does not fit the LDS of the wave kernel. (The 4096 is the built-in models' threshold; it has not been measured for
 * library bodies.) Everything else runs the wave minimiser. fabber_nlls_kernel_name says which: nlls<NAME,P> or
 * nlls_wave<NAME>. The starting estimate is fvb_config.post_mean, as for the built-in models; no initial posterior image
 * is needed.
 *
 * Each macro, at namespace scope:
 *   - instantiates its kernel for the body (nlls_wave_kernel<Eval>; nlls_lane_kernel<LibraryLane<Eval>::Model<P>, P>);
 *   - defines its launcher in this library's code object (csrc/vb_nlls_launch.h: the LDS attribute above 64 KB, one
 *     workgroup per voxel or one lane per voxel, the engine's error texts);
 *   - registers { name, FVB_ABI_VERSION, sizeof(NllsArgs), sizeof(WaveLayout), P (0 = wave), launcher } with the engine
 *     from a static object whose destructor unregisters it. A refused registration (fabber_vb_last_error says why)
 *     leaves the model where it was: on the host route, or on the wave minimiser.
 *
 * The remarks of fabber_device_model.h apply: name the body struct uniquely or put it in an anonymous namespace (the
 * kernels and launchers are template instantiations on it), link the library against the engine library the process
 * uses - another copy of it has another registry - and keep it loaded while a run that uses the body is under way.
 */
#ifndef FABBER_DEVICE_NLLS_MODEL_H
#define FABBER_DEVICE_NLLS_MODEL_H

#include "fabber_device_lane_model.h" /* fvb::LibraryLane: the body as a model of the lane kernels */
#ifndef FVB_NLLS_TEMPLATES_ONLY
#define FVB_NLLS_TEMPLATES_ONLY /* the kernel templates of vb_nlls_kernel.h, not the engine's own step kernel */
#endif
#include "../fabber_core_amd/csrc/vb_nlls_launch.h"

namespace fvb
{
// lane / wave: the one kernel of the macro line, the other NULL
inline int32_t device_nlls_model_launch(NllsKernelFn lane, NllsWaveKernelFn wave, const void *nlls_args, void *stream, char *err, int32_t err_len)
{
    std::string msg;
    const int rc = launch_nlls_kernel(lane, wave, lane ? NLLS_VARIANT_LANE : NLLS_VARIANT_WAVE, *static_cast<const NllsArgs *>(nlls_args),
        static_cast<hipStream_t>(stream), msg);
    return device_launch_result(rc, msg, err, err_len);
}

template <class Eval>
int32_t device_nlls_wave_launch(const void *nlls_args, void *stream, char *err, int32_t err_len)
{
    return device_nlls_model_launch(nullptr, nlls_wave_kernel<Eval>, nlls_args, stream, err, err_len);
}

template <class Eval, int P>
int32_t device_nlls_lane_launch(const void *nlls_args, void *stream, char *err, int32_t err_len)
{
    static_assert(P >= 1 && P <= 6, "FABBER_DEVICE_NLLS_LANE_MODEL: the lane minimisers of a library body exist for 1 to 6 parameters");
    return device_nlls_model_launch(nlls_lane_kernel<typename LibraryLane<Eval>::template Model<P>, P>, nullptr, nlls_args, stream, err, err_len);
}

// the descriptor of one macro line (n_params 0: the wave minimiser)
inline fvb_device_nlls_model device_nlls_model(const char *name, int32_t n_params, fvb_device_nlls_launch_fn launch)
{
    return fvb_device_nlls_model{ name, FVB_ABI_VERSION, (uint32_t)sizeof(NllsArgs), (uint32_t)sizeof(WaveLayout), n_params, launch };
}
} // namespace fvb

#define FABBER_DEVICE_NLLS_MODEL(NAME, EVAL)                                                                                   \
    static fvb::DeviceRegistration<fvb_device_nlls_model> FABBER_DEVICE_CAT(fabber_device_nlls_registration_, __LINE__)(       \
        fvb::device_nlls_model(NAME, 0, &fvb::device_nlls_wave_launch<EVAL>), 0, &fabber_vb_register_device_nlls_model,         \
        &fabber_vb_unregister_device_nlls_model, "NLLS minimiser of ", "method=nlls evaluates the model on the host");
#define FABBER_DEVICE_NLLS_LANE_MODEL(NAME, EVAL, NPARAMS)                                                                     \
    static_assert((NPARAMS) >= 1 && (NPARAMS) <= 6,                                                                            \
        "FABBER_DEVICE_NLLS_LANE_MODEL: the lane minimisers of a library body exist for 1 to 6 parameters");                  \
    static fvb::DeviceRegistration<fvb_device_nlls_model> FABBER_DEVICE_CAT(fabber_device_nlls_lane_registration_, __LINE__)(  \
        fvb::device_nlls_model(NAME, NPARAMS, &fvb::device_nlls_lane_launch<EVAL, NPARAMS>), NPARAMS,                           \
        &fabber_vb_register_device_nlls_model, &fabber_vb_unregister_device_nlls_model, "lane NLLS minimiser of ",             \
        "the wave minimiser is used");

#endif /* FABBER_DEVICE_NLLS_MODEL_H */
