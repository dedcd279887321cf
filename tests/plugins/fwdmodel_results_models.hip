// fwdmodel_results_models.hip - a model library whose device bodies also bring the result-image kernel (model fit and
// residuals on the device), written only against the public headers (fabber_core/*.h for the host side,
// include/fabber_device_model.h, include/fabber_device_lane_model.h and include/fabber_device_results_model.h for the
// bodies). Every model has a host EvaluateModel - the host loop of the result images to compare with, and the route of
// the FIT under method=spatialvb and method=nlls, for which this library brings no kernels - a device body for the
// wave-per-voxel kernels and a results entry.
//
//   "multiexp_res" : y(t) = sum_i amp_i exp(-r_i t), t = 0, dt, 2 dt, ... (options dt, num-exps; rates LOG-transformed;
//                    data-dependent initial posterior): the expression of the built-in exponential model; lane kernels
//                    for one exponential (P = 2)
//   "invrec_res"   : inversion recovery, y(t) = M0 (1 - 2 a exp(-TI_t / T1)); the inversion times are the options
//                    ti1, ti2, ... and reach the device body through the constants block; T1 LOG-transformed, the
//                    inversion efficiency a FRACTIONAL
//
// FABBER_TEST_PART = 1 .. 4 lets the four sets of kernels be compiled side by side (1: host classes and multiexp_res's
// wave kernels, 2: invrec_res's wave kernels, 3: multiexp_res's lane kernels for P = 2, 4: the result-image kernels of
// both); undefined = everything.
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
#define FABBER_TEST_RESULTS 1
#endif

#if defined(FABBER_TEST_MULTIEXP_WAVE) || defined(FABBER_TEST_INVREC_WAVE)
#include "fabber_device_model.h"
#endif
#if defined(FABBER_TEST_MULTIEXP_LANE_2)
#include "fabber_device_lane_model.h"
#endif
#if defined(FABBER_TEST_RESULTS)
#include "fabber_device_results_model.h"
#endif

#define FABBER_TEST_MULTIEXP "multiexp_res"
#define FABBER_TEST_INVREC "invrec_res"
#define FABBER_TEST_WITH "a device body and its result-image kernel"
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
#ifdef FABBER_TEST_RESULTS
FABBER_DEVICE_RESULTS_MODEL(FABBER_TEST_MULTIEXP, MultiExpBody)
FABBER_DEVICE_RESULTS_MODEL(FABBER_TEST_INVREC, InvRecBody)
#endif
