// fwdmodel_init_models.hip - a model library whose device bodies also bring the initial-posterior kernel (the model's
// InitVoxelPosterior on the device), written only against the public headers (fabber_core/*.h for the host side,
// include/fabber_device_model.h, include/fabber_device_lane_model.h, include/fabber_device_lane_noise_model.h,
// include/fabber_device_spatial_model.h and include/fabber_device_init_model.h for the bodies). The bodies are those of
// test_device_models.h with the hook added: it mirrors the host classes' InitVoxelPosterior there, operation by operation.
//
//   "multiexp_init"   : y(t) = sum_i amp_i exp(-r_i t), t = 0, dt, 2 dt, ... (options dt, num-exps; rates
//                       LOG-transformed); the first amplitude starts at the first sample. Lane kernels for one
//                       exponential (P = 2) under white noise, AR(1) noise and noise patterns, spatial kernels for P = 2
//   "invrec_init"     : inversion recovery, y(t) = M0 (1 - 2 a exp(-TI_t / T1)), the inversion times in the constants
//                       block; T1 LOG-transformed, a FRACTIONAL; M0 starts at the largest magnitude of the series
//   "multiexp_noinit" : the body of multiexp_init WITHOUT an init entry (and without host class): a run without init_mvn is
//                       refused, as before
//
// FABBER_TEST_PART = 1 .. 7 lets the sets of kernels be compiled side by side (1: host classes and multiexp_init's wave
// kernels, 2: invrec_init's wave kernels, 3: multiexp_noinit's, 4: multiexp_init's lane kernels for P = 2, 5: its AR(1) and
// noise-pattern lane kernels for P = 2, 6: its spatial kernels for P = 2, 7: the initial-posterior kernels of both - the
// last part, so that a library without its init lines is the same source without that part); undefined = everything.
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 1
#define FABBER_TEST_HOST 1
#define FABBER_TEST_MULTIEXP_WAVE 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 2
#define FABBER_TEST_INVREC_WAVE 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 3
#define FABBER_TEST_NOINIT_WAVE 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 4
#define FABBER_TEST_MULTIEXP_LANE_2 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 5
#define FABBER_TEST_MULTIEXP_LANENZ_2 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 6
#define FABBER_TEST_MULTIEXP_SP_2 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 7
#define FABBER_TEST_INIT 1
#endif

#if defined(FABBER_TEST_MULTIEXP_WAVE) || defined(FABBER_TEST_INVREC_WAVE) || defined(FABBER_TEST_NOINIT_WAVE)
#include "fabber_device_model.h"
#endif
#if defined(FABBER_TEST_MULTIEXP_LANE_2)
#include "fabber_device_lane_model.h"
#endif
#if defined(FABBER_TEST_MULTIEXP_LANENZ_2)
#include "fabber_device_lane_noise_model.h"
#endif
#if defined(FABBER_TEST_MULTIEXP_SP_2)
#include "fabber_device_spatial_model.h"
#endif
#if defined(FABBER_TEST_INIT)
#include "fabber_device_init_model.h"
#endif

#define FABBER_TEST_MULTIEXP "multiexp_init"
#define FABBER_TEST_INVREC "invrec_init"
#define FABBER_TEST_WITH "a device body and its initial-posterior kernel"
#include "test_device_models.h"

namespace
{
#ifdef FABBER_TEST_INIT
// MultiExpFwdModel::InitVoxelPosterior: the first amplitude starts at the first sample
struct MultiExpInitBody : MultiExpBody
{
    static __device__ __forceinline__ void init_posterior(const fvb::ModelArgs &, int, const fvb::VoxelSeries &y, double *means, double *)
    {
        means[0] = y(0);
    }
};
// InvRecFwdModel::InitVoxelPosterior: M0 starts at the largest magnitude of the series (`>`: a NaN sample is skipped)
struct InvRecInitBody : InvRecBody
{
    static __device__ __forceinline__ void init_posterior(const fvb::ModelArgs &, int, const fvb::VoxelSeries &y, double *means, double *)
    {
        double m = 0;
        for (int t = 0; t < y.T; t++)
            m = fabs(y(t)) > m ? fabs(y(t)) : m;
        if (m > 0)
            means[0] = m;
    }
};
#else
// (the fit kernels never call the hook: the parts without the init kernels use the bodies as they are)
typedef MultiExpBody MultiExpInitBody;
typedef InvRecBody InvRecInitBody;
#endif
} // namespace

#ifdef FABBER_TEST_MULTIEXP_WAVE
FABBER_DEVICE_MODEL(FABBER_TEST_MULTIEXP, MultiExpInitBody)
#endif
#ifdef FABBER_TEST_INVREC_WAVE
FABBER_DEVICE_MODEL(FABBER_TEST_INVREC, InvRecInitBody)
#endif
#ifdef FABBER_TEST_NOINIT_WAVE
FABBER_DEVICE_MODEL("multiexp_noinit", MultiExpBody)
#endif
#ifdef FABBER_TEST_MULTIEXP_LANE_2
FABBER_DEVICE_LANE_MODEL(FABBER_TEST_MULTIEXP, MultiExpInitBody, 2)
#endif
#ifdef FABBER_TEST_MULTIEXP_LANENZ_2
FABBER_DEVICE_LANE_NOISE_MODEL(FABBER_TEST_MULTIEXP, MultiExpInitBody, 2, FVB_LANE_NOISE_AR1 | FVB_LANE_NOISE_PHIS)
#endif
#ifdef FABBER_TEST_MULTIEXP_SP_2
FABBER_DEVICE_SPATIAL_MODEL(FABBER_TEST_MULTIEXP, MultiExpInitBody, 2)
#endif
#ifdef FABBER_TEST_INIT
FABBER_DEVICE_INIT_MODEL(FABBER_TEST_MULTIEXP, MultiExpInitBody)
FABBER_DEVICE_INIT_MODEL(FABBER_TEST_INVREC, InvRecInitBody)
#endif
