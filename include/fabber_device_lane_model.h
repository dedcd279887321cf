/*
 * fabber_device_lane_model.h - the lane-per-voxel kernels for a model library's DEVICE body.
 *
 * fabber_device_model.h gives a body the wave-per-voxel kernels (one wavefront per voxel): any parameter count, every
 * noise model, and about 3 M voxels/s at most. The lane-per-voxel kernels (one voxel per lane, 64 voxels per wavefront)
 * are what the engine runs its built-in models on from a few thousand voxels up. This header compiles them around the
 * SAME body, for one parameter count per macro line:
 *
 *     FABBER_DEVICE_MODEL("invrec", InvRec)          // the wave kernels: the route of everything not covered below
 *     FABBER_DEVICE_LANE_MODEL("invrec", InvRec, 3)  // the lane kernels for exactly 3 parameters
 *
 * Several lines per name are allowed (a model with a variable parameter count names the counts worth having), each for
 * 1 <= P <= 6. The first line is required: a lane entry without a wave body of the same name is never used. It is a
 * header of its own because it includes the lane kernels: a library that does not want them does not pay for them.
 * Compile as fabber_device_model.h says; a macro line takes some tens of seconds.
 *
 * The body is the struct of fabber_device_model.h, unchanged:
 *
 *     static __device__ __forceinline__ double eval(const fvb::ModelArgs &a, int P, int t, const double *p)
 *
 * Declare eval __forceinline__. The lane kernel keeps a voxel's parameter vector in registers and calls eval 2 P + 1
 * times per timepoint; a body that is not inlined receives it through a pointer, which puts the vector into scratch
 * memory for every call. Inlined, P is a constant and loops over it unroll.
 *
 * The engine takes the lane route for a configuration when a lane entry for (name, n_params) is registered, the noise
 * is white with one precision, the kernel variant is not `wave`, and the size rule of the built-in models holds (variant
 * `lane`, or at least 4096 voxels, or fewer than 400 model evaluations per pass). AR(1) noise with one echo and noise
 * patterns of 2 to 4 precisions have lane kernels of their own, which a library compiles with a line of
 * fabber_device_lane_noise_model.h (FABBER_DEVICE_LANE_NOISE_MODEL); without that line they run the wave kernels of
 * FABBER_DEVICE_MODEL, as everything else does - two echoes, 5 to 8 precisions, other parameter counts, small volumes.
 * The kernel's name is lane<NAME,P> / lane<NAME,P,F>.
 *
 * A SWEEP OF THE BODY'S OWN (optional). A linearisation needs 2 P + 1 predictions per timepoint: g = f(p) and, for every
 * parameter i, f with entry i replaced by p2[i] and by p3[i]. Without more from the body the kernels call eval for each of
 * them. A body whose predictions share work ALONG t (a geometric sequence, a running sum, a convolution built up sample
 * by sample) can say so with a nested member template, and every lane family of these headers - white noise, AR(1), noise
 * patterns, the spatial lane kernels - then linearises through it:
 *
 *     template <int P> struct Sweep
 *     {
 *         // members: the state of ONE linearisation of ONE voxel; it lives in registers across the pass
 *         __device__ __forceinline__ void init(const fvb::ModelArgs &a, const double (&p)[P], const double (&p2)[P],
 *             const double (&p3)[P]);
 *         // g = f(p); f2[i] / f3[i] = f(p with entry i replaced by p2[i] / p3[i]), all at timepoint t
 *         __device__ __forceinline__ void step(const fvb::ModelArgs &a, int t, bool exact, const double (&p)[P],
 *             const double (&p2)[P], const double (&p3)[P], double &g, double (&f2)[P], double (&f3)[P]);
 *     };
 *
 * The contract (fvb::LibrarySweep below is the engine's side of it):
 *   - init comes first; after it step is called for t = 0, 1, 2, ... in this order, every timepoint once (a masked
 *     timepoint included), with the p, p2, p3 that init saw;
 *   - `exact` is wave-uniform. It is true at the first step after init; at EVERY step of a pass the engine wants evaluated
 *     as precisely as the body can (the first precise_passes linearisations of a run and the passes that form a Jacobian
 *     made that way again); otherwise at least once in every 8 consecutive timepoints (FVB_EXP_RESYNC: where t is a
 *     multiple of 8);
 *   - an exact step returns what 2 P + 1 calls of eval return, to rounding; a step that is not exact may use what the step
 *     at t - 1 left (what a recurrence adds in rounding is bounded by the 7 steps between two exact ones);
 *   - the sweep is deterministic: a linearisation that is formed again (the residual passes) gives the same values;
 *   - the body hands over no derivatives: the engine forms J from the two perturbed sums, (f2[i] - f3[i]) * rden[i], as
 *     for every model (vb_models.h says why a structured quotient was measured and dropped);
 *   - the sweep reads a.consts and fvb::supp_at as eval does, with the same checks of n_consts / n_supp.
 * Everything else evaluates the body pointwise through eval, so a body with a sweep still needs a correct eval: the rescue
 * passes of the lane kernels, the wave-per-voxel kernels, the NLLS minimisers, the result-image and initial-posterior
 * kernels. A body without the member is evaluated pointwise throughout, by the same kernel code as before the member
 * existed. Registration is the same macro line either way.
 *
 * The macro, at namespace scope:
 *   - instantiates the eight white-noise lane kernels for the body (in-place feed, float tiles and double tiles, each
 *     with and without the free energy, and the two tile-fed ones of a run whose detector only counts iterations);
 *   - defines their launcher in this library's code object (one lane per voxel, the engine's error texts);
 *   - registers { name, FVB_ABI_VERSION, sizeof(KernelArgs), P, rows of the save buffer, launcher } with the engine from
 *     a static object whose destructor unregisters it. A refused registration (fabber_vb_last_error says why) leaves the
 *     model on the wave kernels.
 *
 * The remarks of fabber_device_model.h about naming the body struct, linking and unloading apply.
 */
#ifndef FABBER_DEVICE_LANE_MODEL_H
#define FABBER_DEVICE_LANE_MODEL_H

#include "fabber_device_registration.h"
#include "../fabber_core_amd/csrc/vb_lane_launch.h"

#include <type_traits>

namespace fvb
{
// does the body bring `template <int P> struct Sweep`?
template <class Eval, int P, class = void>
struct body_has_sweep : std::false_type
{
};
template <class Eval, int P>
struct body_has_sweep<Eval, P, std::void_t<typename Eval::template Sweep<P>>> : std::true_type
{
};

// The body's sweep behind the sweep interface of the lane kernels (vb_models.h; ExpModel<P>::Sweep is the built-in model
// of it). When a step is exact is decided here, from what the kernels ask: every step of a precise pass, and otherwise
// the timepoints that are multiples of FVB_EXP_RESYNC - the kernels' streaming loop (recentre_tiles) knows those at compile
// time and says so through step_fast<EXACT>. init clears the flag because one call site (the AR(1) residual pass) never
// sets it. step_acc (the half-ulp exp of the spatial set-up kernels) is asked of the exponential model only.
template <class Eval, int P>
struct LibrarySweep
{
    typename Eval::template Sweep<P> body;
    bool precise; // every step exact (wave-uniform)
    __device__ __forceinline__ void init(const ModelArgs &a, const double (&tp)[P], const double (&tp2)[P], const double (&tp3)[P])
    {
        precise = false;
        body.init(a, tp, tp2, tp3);
    }
    __device__ __forceinline__ void set_precise(bool p)
    {
        precise = p;
    }
    __device__ __forceinline__ void eval(const ModelArgs &a, int t, const double (&tp)[P], const double (&tp2)[P], const double (&tp3)[P],
        double &g, double (&f2)[P], double (&f3)[P])
    {
        body.step(a, t, precise || (t % FVB_EXP_RESYNC) == 0, tp, tp2, tp3, g, f2, f3);
    }
    // J_i = (f2_i - f3_i) * rden_i from the two perturbed sums, as PointwiseSweep forms it
    __device__ __forceinline__ void jacobian(const double (&f2)[P], const double (&f3)[P], const double (&rden)[P], double (&J)[P])
    {
        FVB_MODEL_FP
#pragma unroll
        for (int i = 0; i < P; i++)
            J[i] = (f2[i] - f3[i]) * rden[i];
    }
    __device__ __forceinline__ void eval_jac(const ModelArgs &a, int t, const double (&tp)[P], const double (&tp2)[P], const double (&tp3)[P],
        const double (&rden)[P], double &g, double (&J)[P])
    {
        double f2[P], f3[P];
        eval(a, t, tp, tp2, tp3, g, f2, f3);
        jacobian(f2, f3, rden, J);
    }
    template <bool EXACT>
    __device__ __forceinline__ void step_fast(const ModelArgs &a, int t, const double (&tp)[P], const double (&tp2)[P], const double (&tp3)[P],
        const double (&rden)[P], double &g, double (&J)[P])
    {
        double f2[P], f3[P];
        body.step(a, t, EXACT, tp, tp2, tp3, g, f2, f3);
        jacobian(f2, f3, rden, J);
    }
    __device__ __forceinline__ void step_any(const ModelArgs &a, int t, const double (&tp)[P], const double (&tp2)[P], const double (&tp3)[P],
        const double (&rden)[P], double &g, double (&J)[P], bool prec)
    {
        double f2[P], f3[P];
        body.step(a, t, prec || (t % FVB_EXP_RESYNC) == 0, tp, tp2, tp3, g, f2, f3);
        jacobian(f2, f3, rden, J);
    }
};

// the body as a model of the lane kernels (vb_models.h): P a constant, the body's sweep or else the pointwise one, the
// initial posterior from the host (init_mvn)
template <class Eval>
struct LibraryLane
{
    template <int P>
    struct Model
    {
        static constexpr bool host_evaluated = false;
        static constexpr int model_id = FVB_MODEL_PLUGIN;
        // (LibrarySweep<Eval, P> is only named here: it is not instantiated for a body without the member)
        typedef std::conditional_t<body_has_sweep<Eval, P>::value, LibrarySweep<Eval, P>, PointwiseSweep<Model<P>, P>> Sweep;
        static __device__ __forceinline__ double eval(const ModelArgs &a, int t, const double (&p)[P])
        {
            return Eval::eval(a, P, t, p);
        }
        static __device__ __forceinline__ void init_posterior(const ModelArgs &, double, double (&)[P])
        {
        }
        static constexpr bool needs_data_max = false;
    };
};

typedef LaneKernelInfo (*LaneKernelsFn)(bool need_f);

inline int32_t device_lane_model_launch(LaneKernelsFn kernels, const void *kernel_args, int32_t feed, int32_t counting, void *stream,
    char *err, int32_t err_len)
{
    const KernelArgs &ka = *static_cast<const KernelArgs *>(kernel_args);
    std::string msg;
    const int rc = launch_lane_kernel(kernels(ka.cfg.need_f != 0), ka, feed, counting != 0, 0, static_cast<hipStream_t>(stream), msg);
    return device_launch_result(rc, msg, err, err_len);
}
} // namespace fvb

// (FVB_LANE_CASE is the engine's own table entry of a built-in model: the same eight kernels, the same names)
#define FABBER_DEVICE_LANE_MODEL(NAME, EVAL, NPARAMS)                                                                        \
    static_assert((NPARAMS) >= 1 && (NPARAMS) <= 6, "FABBER_DEVICE_LANE_MODEL: the lane kernels of a library body exist for 1 to 6 parameters"); \
    static fvb::LaneKernelInfo FABBER_DEVICE_CAT(fabber_device_lane_kernels_, __LINE__)(bool need_f)              \
    {                                                                                                                        \
        using namespace fvb;                                                                                                 \
        switch (NPARAMS)                                                                                                     \
        {                                                                                                                    \
            FVB_LANE_CASE(LibraryLane<EVAL>::Model, NAME, NPARAMS)                                                           \
        }                                                                                                                    \
        return LaneKernelInfo{ nullptr, 0, nullptr };                                                                        \
    }                                                                                                                        \
    static int32_t FABBER_DEVICE_CAT(fabber_device_lane_launch_, __LINE__)(                                       \
        const void *kernel_args, int32_t feed, int32_t counting, void *stream, char *err, int32_t err_len)                   \
    {                                                                                                                        \
        return fvb::device_lane_model_launch(&FABBER_DEVICE_CAT(fabber_device_lane_kernels_, __LINE__), kernel_args, feed, \
            counting, stream, err, err_len);                                                                                 \
    }                                                                                                                        \
    static fvb::DeviceRegistration<fvb_device_lane_model> FABBER_DEVICE_CAT(fabber_device_lane_registration_, __LINE__)(      \
        fvb_device_lane_model{ NAME, FVB_ABI_VERSION, (uint32_t)sizeof(fvb::KernelArgs), NPARAMS, fvb::lane_save_rows<NPARAMS>(), \
            &FABBER_DEVICE_CAT(fabber_device_lane_launch_, __LINE__) },                                                      \
        NPARAMS, &fabber_vb_register_device_lane_model, &fabber_vb_unregister_device_lane_model, "lane kernels of ",         \
        "the model runs on the wave kernels");

#endif /* FABBER_DEVICE_LANE_MODEL_H */
