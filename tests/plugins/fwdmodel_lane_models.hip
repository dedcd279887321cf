// fwdmodel_lane_models.hip - a model library whose device bodies also bring the lane-per-voxel kernels, written only
// against the public headers (fabber_core/*.h for the host side, include/fabber_device_model.h and
// include/fabber_device_lane_model.h for the bodies). Every model has a host EvaluateModel, a device body for the
// wave-per-voxel kernels and lane kernels for the parameter counts named below; every other count, noise patterns, AR(1)
// noise and small volumes stay on the wave kernels.
//
//   "multiexp_lane" : y(t) = sum_i amp_i exp(-r_i t), t = 0, dt, 2 dt, ... (options dt, num-exps; rates LOG-transformed;
//                     data-dependent initial posterior); lane kernels for one and two exponentials (P = 2, 4)
//   "invrec_lane"   : inversion recovery, y(t) = M0 (1 - 2 a exp(-TI_t / T1)); the inversion times are the options
//                     ti1, ti2, ... and reach the device body through the constants block; T1 LOG-transformed, the
//                     inversion efficiency a FRACTIONAL; lane kernels for its three parameters
//
// FABBER_TEST_PART = 1 .. 5 lets the five sets of kernels be compiled side by side (1: host classes and multiexp_lane's
// wave kernels, 2: invrec_lane's wave kernels, 3 / 4: multiexp_lane's lane kernels for P = 2 / 4, 5: invrec_lane's lane
// kernels); undefined = everything.
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 1
#define FABBER_TEST_HOST 1
#define FABBER_TEST_MULTIEXP_WAVE 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 2
#define FABBER_TEST_INVREC_WAVE 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 3
#define FABBER_TEST_MULTIEXP_LANE_2 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 4
#define FABBER_TEST_MULTIEXP_LANE_4 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 5
#define FABBER_TEST_INVREC_LANE 1
#endif

#if defined(FABBER_TEST_MULTIEXP_WAVE) || defined(FABBER_TEST_INVREC_WAVE)
#include "fabber_device_model.h"
#endif
#if defined(FABBER_TEST_MULTIEXP_LANE_2) || defined(FABBER_TEST_MULTIEXP_LANE_4) || defined(FABBER_TEST_INVREC_LANE)
#include "fabber_device_lane_model.h"
#endif

#define FABBER_TEST_MULTIEXP "multiexp_lane"
#define FABBER_TEST_INVREC "invrec_lane"
#define FABBER_TEST_WITH "a device body and its lane kernels"
#include "test_device_models.h"

#ifdef FABBER_TEST_MULTIEXP_WAVE
FABBER_DEVICE_MODEL(FABBER_TEST_MULTIEXP, MultiExpBody)
#endif
#ifdef FABBER_TEST_INVREC_WAVE
FABBER_DEVICE_MODEL(FABBER_TEST_INVREC, InvRecBody)
#endif
#ifdef FABBER_TEST_MULTIEXP_LANE_2
FABBER_DEVICE_LANE_MODEL(FABBER_TEST_MULTIEXP, MultiExpBody, 2)
#endif
#ifdef FABBER_TEST_MULTIEXP_LANE_4
FABBER_DEVICE_LANE_MODEL(FABBER_TEST_MULTIEXP, MultiExpBody, 4)
#endif
#ifdef FABBER_TEST_INVREC_LANE
FABBER_DEVICE_LANE_MODEL(FABBER_TEST_INVREC, InvRecBody, 3)
#endif
