// fwdmodel_sweep_models.hip - a model library whose device bodies bring a SWEEP of their own (the optional member
// `template <int P> struct Sweep` of include/fabber_device_lane_model.h), written only against the public headers. The lane
// kernels of every family linearise through the sweep; the wave kernels, the rescue passes and everything else evaluate
// the same bodies pointwise through eval.
//
//   "multiexp_sw"    : y(t) = sum_i amp_i exp(-r_i t), t = 0, dt, 2 dt, ... - the host class and eval of
//                      test_device_models.h. Its sweep restates the recurrence of the built-in exponential model: the three
//                      rates of every exponential (r, r + d, r - d) are evaluated where a step is exact and advanced by one
//                      multiplication with exp(-r dt) where it is not; the sums add their terms in the order of eval.
//                      Lane kernels for P = 2 and 4, AR(1) / noise-pattern lane kernels for P = 2, the spatial kernels of
//                      white noise and of AR(1) / noise patterns for P = 2.
//   "multiexp_swchk" : the same arithmetic (a device body only: no host class of this name). Its sweep also keeps count of
//                      what the contract promises - init before the first step, the first step exact, the timepoints in
//                      order, fewer than 8 steps since the last exact one - and answers a NaN g from the step that finds
//                      it broken on: the voxel then stops with a non-zero status. Lane kernels and AR(1) / noise-pattern
//                      lane kernels for P = 2.
//
// FABBER_TEST_PART = 1 .. 9 lets the kernels be compiled side by side (1: host class and multiexp_sw's wave kernels; 2 / 3:
// multiexp_sw's lane kernels for P = 2 / 4; 4: its AR(1) / noise-pattern lane kernels; 5 / 6: its spatial kernels of white
// noise / of AR(1) and noise patterns; 7 / 8: multiexp_swchk's lane kernels / AR(1) and noise-pattern lane kernels; 9: its
// wave kernels); undefined = everything.
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 1
#define FABBER_TEST_HOST 1
#define FABBER_TEST_SW_WAVE 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 2
#define FABBER_TEST_SW_LANE_2 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 3
#define FABBER_TEST_SW_LANE_4 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 4
#define FABBER_TEST_SW_LANENZ 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 5
#define FABBER_TEST_SW_SP 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 6
#define FABBER_TEST_SW_SPN 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 7
#define FABBER_TEST_SWCHK_LANE 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 8
#define FABBER_TEST_SWCHK_LANENZ 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 9
#define FABBER_TEST_SWCHK_WAVE 1
#endif

// The test of the order contract compares multiexp_swchk's kernels with multiexp_sw's BIT FOR BIT, i.e. two instantiations
// of the same kernel text. Under the compiler's default (contraction wherever it likes) that is not a property the text
// has: in a sum of two products, a * b + c * d, the compiler chooses which product goes into the fused multiply-add, per
// instantiation (the order of the operands of a commutative add after its passes), and the AR(1) kernels' cross moments
// are such sums - their two instantiations differed in the last bit of a few voxels after two iterations and in the
// eighth digit after ten, for series of 8, 9, 24 and 25 timepoints only. So the two parts with the AR(1) / noise-pattern
// kernels are compiled with contraction OFF outside the model code: the bodies, their sweeps and the engine's model-side
// code say FVB_MODEL_FP themselves and keep theirs. lane_ar1<multiexp_sw,2> is therefore the arithmetic of the built-in
// lane_ar1<exp,2> up to that, not bit for bit (the tests print which); the white-noise parts are compiled as any
// library's and are the built-in kernels' arithmetic bit for bit.
#if defined(FABBER_TEST_PART) && (FABBER_TEST_PART == 4 || FABBER_TEST_PART == 8)
#pragma clang fp contract(off)
#endif

#include "fabber_device_model.h"
#include "fabber_device_lane_model.h" /* fvb::body_has_sweep */
#if defined(FABBER_TEST_SW_LANENZ) || defined(FABBER_TEST_SWCHK_LANENZ)
#include "fabber_device_lane_noise_model.h"
#endif
#if defined(FABBER_TEST_SW_SP)
#include "fabber_device_spatial_model.h"
#endif
#if defined(FABBER_TEST_SW_SPN)
#include "fabber_device_spatial_noise_model.h"
#endif

// ---- device bodies ----------------------------------------------------------------------------------------------
namespace // (a body's kernels and launchers are template instantiations on it: keep its name to this library)
{
// CHECKED: the sweep keeps the contract's books (multiexp_swchk)
template <bool CHECKED>
struct MultiExpSweepBody
{
    // a.iopt0 = num-exps (P = 2 num-exps), a.dopt0 = dt: MultiExpBody::eval of test_device_models.h
    static __device__ __forceinline__ double eval(const fvb::ModelArgs &a, int P, int t, const double *p)
    {
        FVB_MODEL_FP
        const double tt = double(t) * a.dopt0;
        double res = 0;
        for (int i = 0; i < P / 2; i++)
        {
            double val = p[2 * i] * exp(-p[2 * i + 1] * tt);
            res += val;
        }
        return res;
    }

    template <int P>
    struct Sweep
    {
        static_assert(P % 2 == 0, "two parameters per exponential");
        static constexpr int N = P / 2;
        // exp(-rate t dt) at the current timepoint and exp(-rate dt), for the rates of p, p2 and p3
        double e0[N], e2[N], e3[N], s0[N], s2[N], s3[N];
        // the contract's books (CHECKED only; the members of a sweep that never reads them cost nothing)
        bool inited = false, first = true, broken = false;
        int prev_t = -1, since_exact = 0;

        __device__ __forceinline__ void init(const fvb::ModelArgs &a, const double (&p)[P], const double (&p2)[P], const double (&p3)[P])
        {
            FVB_MODEL_FP
#pragma unroll
            for (int i = 0; i < N; i++)
            {
                s0[i] = exp(-p[2 * i + 1] * a.dopt0);
                s2[i] = exp(-p2[2 * i + 1] * a.dopt0);
                s3[i] = exp(-p3[2 * i + 1] * a.dopt0);
            }
            inited = true;
            first = true;
            prev_t = -1;
            since_exact = 0;
        }

        __device__ __forceinline__ void step(const fvb::ModelArgs &a, int t, bool exact, const double (&p)[P], const double (&p2)[P],
            const double (&p3)[P], double &g, double (&f2)[P], double (&f3)[P])
        {
            FVB_MODEL_FP
            if (CHECKED)
            {
                if (!inited || (first && !exact) || t != prev_t + 1)
                    broken = true;
                since_exact = exact ? 0 : since_exact + 1;
                if (since_exact >= 8)
                    broken = true;
                first = false;
                prev_t = t;
            }
            if (exact) // wave-uniform
            {
                const double tt = double(t) * a.dopt0;
#pragma unroll
                for (int i = 0; i < N; i++)
                {
                    e0[i] = exp(-p[2 * i + 1] * tt);
                    e2[i] = exp(-p2[2 * i + 1] * tt);
                    e3[i] = exp(-p3[2 * i + 1] * tt);
                }
            }
            else
            {
#pragma unroll
                for (int i = 0; i < N; i++)
                {
                    e0[i] *= s0[i];
                    e2[i] *= s2[i];
                    e3[i] *= s3[i];
                }
            }
            // (a broken contract poisons an INPUT of the sums: g, computed from it like every other g, is NaN, and the
            // arithmetic after this line is multiexp_sw's, operation for operation)
            if (CHECKED)
            {
                if (broken)
                    e0[0] = __builtin_nan("");
            }
            // the sums add their terms in the order of eval: res = amp_1 e_1 (+ 0, which changes nothing), res += amp_j e_j
            double val[N];
#pragma unroll
            for (int j = 0; j < N; j++)
                val[j] = p[2 * j] * e0[j];
            double res = val[0];
#pragma unroll
            for (int j = 1; j < N; j++)
                res += val[j];
            g = res;
#pragma unroll
            for (int i = 0; i < N; i++)
            {
                double a2 = (i == 0) ? p2[0] * e0[0] : val[0];
                double a3 = (i == 0) ? p3[0] * e0[0] : val[0];
                double r2 = (i == 0) ? p[0] * e2[0] : val[0];
                double r3 = (i == 0) ? p[0] * e3[0] : val[0];
#pragma unroll
                for (int j = 1; j < N; j++)
                {
                    a2 += (j == i) ? p2[2 * i] * e0[i] : val[j];
                    a3 += (j == i) ? p3[2 * i] * e0[i] : val[j];
                    r2 += (j == i) ? p[2 * i] * e2[i] : val[j];
                    r3 += (j == i) ? p[2 * i] * e3[i] : val[j];
                }
                f2[2 * i] = a2;
                f3[2 * i] = a3;
                f2[2 * i + 1] = r2;
                f3[2 * i + 1] = r3;
            }
        }
    };
};
typedef MultiExpSweepBody<false> MultiExpSwBody;
typedef MultiExpSweepBody<true> MultiExpSwChkBody;

// a tree without the feature does not compile this library
static_assert(fvb::body_has_sweep<MultiExpSwBody, 2>::value && fvb::body_has_sweep<MultiExpSwChkBody, 2>::value,
    "the bodies of this library bring a sweep");
static_assert(std::is_same<fvb::LibraryLane<MultiExpSwBody>::Model<4>::Sweep, fvb::LibrarySweep<MultiExpSwBody, 4>>::value,
    "the lane kernels linearise through it");
} // namespace

#define FABBER_TEST_OWN_BODIES 1
#define FABBER_TEST_MULTIEXP "multiexp_sw"
#define FABBER_TEST_INVREC "invrec_sw" // (the header's second model: its host class is compiled, the library does not list it)
#define FABBER_TEST_WITH "a device body that brings its own sweep along t"
// the header's loader hooks are those of its own two models: this library writes its own below
#define get_num_models fabber_test_header_num_models
#define get_model_name fabber_test_header_model_name
#define get_new_instance_func fabber_test_header_new_instance_func
#include "test_device_models.h"
#undef get_num_models
#undef get_model_name
#undef get_new_instance_func

#ifdef FABBER_TEST_HOST
// the three hooks fabber_load_models reads (fwdmodel.cc:25-27)
extern "C" {
int get_num_models()
{
    return 1;
}
const char *get_model_name(int index)
{
    return index == 0 ? "multiexp_sw" : 0;
}
NewInstanceFptr get_new_instance_func(const char *name)
{
    return std::string(name) == "multiexp_sw" ? MultiExpFwdModel::NewInstance : 0;
}
}
#endif

#ifdef FABBER_TEST_SW_WAVE
FABBER_DEVICE_MODEL("multiexp_sw", MultiExpSwBody)
#endif
#ifdef FABBER_TEST_SWCHK_WAVE
FABBER_DEVICE_MODEL("multiexp_swchk", MultiExpSwChkBody)
#endif
#ifdef FABBER_TEST_SW_LANE_2
FABBER_DEVICE_LANE_MODEL("multiexp_sw", MultiExpSwBody, 2)
#endif
#ifdef FABBER_TEST_SW_LANE_4
FABBER_DEVICE_LANE_MODEL("multiexp_sw", MultiExpSwBody, 4)
#endif
#ifdef FABBER_TEST_SW_LANENZ
FABBER_DEVICE_LANE_NOISE_MODEL("multiexp_sw", MultiExpSwBody, 2, FVB_LANE_NOISE_AR1 | FVB_LANE_NOISE_PHIS)
#endif
#ifdef FABBER_TEST_SW_SP
FABBER_DEVICE_SPATIAL_MODEL("multiexp_sw", MultiExpSwBody, 2)
#endif
#ifdef FABBER_TEST_SW_SPN
FABBER_DEVICE_SPATIAL_NOISE_MODEL("multiexp_sw", MultiExpSwBody, 2, FVB_SPATIAL_NOISE_AR1 | FVB_SPATIAL_NOISE_PHIS)
#endif
#ifdef FABBER_TEST_SWCHK_LANE
FABBER_DEVICE_LANE_MODEL("multiexp_swchk", MultiExpSwChkBody, 2)
#endif
#ifdef FABBER_TEST_SWCHK_LANENZ
FABBER_DEVICE_LANE_NOISE_MODEL("multiexp_swchk", MultiExpSwChkBody, 2, FVB_LANE_NOISE_AR1 | FVB_LANE_NOISE_PHIS)
#endif
