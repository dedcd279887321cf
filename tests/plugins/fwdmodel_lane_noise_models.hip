// fwdmodel_lane_noise_models.hip - a model library whose device bodies bring the lane-per-voxel kernels of AR(1) noise and
// of noise patterns, written only against the public headers (fabber_core/*.h for the host side,
// include/fabber_device_model.h and include/fabber_device_lane_noise_model.h for the bodies). Every model has a host
// EvaluateModel, a device body for the wave-per-voxel kernels and the lane kernels named below; white noise with one
// precision (no FABBER_DEVICE_LANE_MODEL line here), two echoes, 5 to 8 precisions and every other parameter count stay
// on the wave kernels.
//
//   "multiexp_lanenz" : y(t) = sum_i amp_i exp(-r_i t) as in fwdmodel_lane_models.hip; one exponential (P = 2): both
//                       families; two (P = 4): AR(1) only, so that the mask decides something
//   "invrec_lanenz"   : inversion recovery as in fwdmodel_lane_models.hip (the inversion times in the constants block);
//                       its three parameters: both families
//
// FABBER_TEST_PART = 1 .. 5 lets the five sets of kernels be compiled side by side (1: host classes and multiexp_lanenz's
// wave kernels, 2: invrec_lanenz's wave kernels, 3 / 4: multiexp_lanenz's lane kernels for P = 2 / 4, 5: invrec_lanenz's
// lane kernels); undefined = everything.
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 1
#define FABBER_TEST_HOST 1
#define FABBER_TEST_MULTIEXP_WAVE 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 2
#define FABBER_TEST_INVREC_WAVE 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 3
#define FABBER_TEST_MULTIEXP_LANENZ_2 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 4
#define FABBER_TEST_MULTIEXP_LANENZ_4 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 5
#define FABBER_TEST_INVREC_LANENZ 1
#endif

#if defined(FABBER_TEST_MULTIEXP_WAVE) || defined(FABBER_TEST_INVREC_WAVE)
#include "fabber_device_model.h"
#endif
#if defined(FABBER_TEST_MULTIEXP_LANENZ_2) || defined(FABBER_TEST_MULTIEXP_LANENZ_4) || defined(FABBER_TEST_INVREC_LANENZ)
#include "fabber_device_lane_noise_model.h"
#endif

#define FABBER_TEST_MULTIEXP "multiexp_lanenz"
#define FABBER_TEST_INVREC "invrec_lanenz"
#define FABBER_TEST_WITH "a device body and its lane kernels under AR(1) noise and noise patterns"
#include "test_device_models.h"

#ifdef FABBER_TEST_MULTIEXP_WAVE
FABBER_DEVICE_MODEL(FABBER_TEST_MULTIEXP, MultiExpBody)
#endif
#ifdef FABBER_TEST_INVREC_WAVE
FABBER_DEVICE_MODEL(FABBER_TEST_INVREC, InvRecBody)
#endif
#ifdef FABBER_TEST_MULTIEXP_LANENZ_2
FABBER_DEVICE_LANE_NOISE_MODEL(FABBER_TEST_MULTIEXP, MultiExpBody, 2, FVB_LANE_NOISE_AR1 | FVB_LANE_NOISE_PHIS)
#endif
#ifdef FABBER_TEST_MULTIEXP_LANENZ_4
FABBER_DEVICE_LANE_NOISE_MODEL(FABBER_TEST_MULTIEXP, MultiExpBody, 4, FVB_LANE_NOISE_AR1)
#endif
#ifdef FABBER_TEST_INVREC_LANENZ
FABBER_DEVICE_LANE_NOISE_MODEL(FABBER_TEST_INVREC, InvRecBody, 3, FVB_LANE_NOISE_AR1 | FVB_LANE_NOISE_PHIS)
#endif
