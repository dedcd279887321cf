// fwdmodel_device_models.hip - a model library whose models bring their own DEVICE bodies, written only against the
// public headers (fabber_core/*.h for the host side, include/fabber_device_model.h for the bodies). Every model has
// a host EvaluateModel - used for the initial posterior, the result images and every route the device body does not
// serve - and a device body that computes the same expression.
//
//   "multiexp_dev" : y(t) = sum_i amp_i exp(-r_i t), t = 0, dt, 2 dt, ... (the sum of exponentials of
//                    fwdmodel_multiexp.cc: options dt, num-exps; rates LOG-transformed; data-dependent initial posterior)
//   "invrec"       : inversion recovery, y(t) = M0 (1 - 2 a exp(-TI_t / T1)); the inversion times are the options
//                    ti1, ti2, ... and reach the device body through the constants block; T1 LOG-transformed, the
//                    inversion efficiency a FRACTIONAL
//
// The kernels of a body take about a minute to compile: FABBER_TEST_PART = 1 (host classes + multiexp_dev's body) and
// 2 (invrec's body) let the two halves be compiled side by side; undefined = everything.
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 1
#define FABBER_TEST_HOST 1
#define FABBER_TEST_MULTIEXP_WAVE 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 2
#define FABBER_TEST_INVREC_WAVE 1
#endif

#include "fabber_device_model.h"

// ---- device bodies ----------------------------------------------------------------------------------------------
#ifdef FABBER_TEST_MULTIEXP_WAVE
namespace // (a body's kernels and launcher are template instantiations on it: keep its name to this library)
{
struct MultiExpBody
{
    // a.iopt0 = num-exps (P = 2 num-exps), a.dopt0 = dt
    static __device__ double eval(const fvb::ModelArgs &a, int P, int t, const double *p)
    {
        FVB_MODEL_FP
        const double tt = double(t) * a.dopt0;
        double res = 0;
        for (int i = 0; i < P / 2; i++)
            res += p[2 * i] * exp(-p[2 * i + 1] * tt);
        return res;
    }
};
} // namespace
FABBER_DEVICE_MODEL("multiexp_dev", MultiExpBody)
#endif

#ifdef FABBER_TEST_INVREC_WAVE
namespace
{
struct InvRecBody
{
    // p = (M0, T1, a); a.consts = the inversion times, one per timepoint. Nothing but the body knows how many constants
    // it needs: a timepoint without one is a non-finite prediction (the voxel stops with the non-finite-offset status,
    // where the host code's EvaluateModel throws), never a read past the block
    static __device__ double eval(const fvb::ModelArgs &a, int, int t, const double *p)
    {
        FVB_MODEL_FP
        if (t >= a.n_consts)
            return __builtin_nan("");
        return p[0] * (1.0 - 2.0 * p[2] * exp(-a.consts[t] / p[1]));
    }
};
} // namespace
FABBER_DEVICE_MODEL("invrec", InvRecBody)
#endif

#define FABBER_TEST_OWN_BODIES 1 // (above: not inlined by force, each compiled in its part only)
#define FABBER_TEST_MULTIEXP "multiexp_dev"
#define FABBER_TEST_INVREC "invrec"
#define FABBER_TEST_WITH "a device body"
#include "test_device_models.h"
