// fwdmodel_spatial_models.hip - a model library whose device bodies also bring the spatial VB kernels
// (method=spatialvb), written only against the public headers (fabber_core/*.h for the host side,
// include/fabber_device_model.h and include/fabber_device_spatial_model.h for the bodies). Every model has a host
// EvaluateModel - the host route of spatial VB to compare with - a device body for the wave-per-voxel kernels and
// spatial entries for the parameter counts named below; every other count, noise patterns and AR(1) noise keep the host
// route under spatial VB.
//
//   "multiexp_sp" : y(t) = sum_i amp_i exp(-r_i t), t = 0, dt, 2 dt, ... (options dt, num-exps; rates LOG-transformed;
//                   data-dependent initial posterior): the expression of the built-in exponential model; spatial entries
//                   for one and two exponentials (P = 2, 4)
//   "invrec_sp"   : inversion recovery, y(t) = M0 (1 - 2 a exp(-TI_t / T1)); the inversion times are the options
//                   ti1, ti2, ... and reach the device body through the constants block; T1 LOG-transformed, the
//                   inversion efficiency a FRACTIONAL; a spatial entry for its three parameters
//
// FABBER_TEST_PART = 1 .. 5 lets the five sets of kernels be compiled side by side (1: host classes and multiexp_sp's
// wave kernels, 2: invrec_sp's wave kernels, 3 / 4: multiexp_sp's spatial kernels for P = 2 / 4, 5: invrec_sp's spatial
// kernels); undefined = everything.
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 1
#define FABBER_TEST_HOST 1
#define FABBER_TEST_MULTIEXP_WAVE 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 2
#define FABBER_TEST_INVREC_WAVE 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 3
#define FABBER_TEST_MULTIEXP_SP_2 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 4
#define FABBER_TEST_MULTIEXP_SP_4 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 5
#define FABBER_TEST_INVREC_SP 1
#endif

#if defined(FABBER_TEST_MULTIEXP_WAVE) || defined(FABBER_TEST_INVREC_WAVE)
#include "fabber_device_model.h"
#endif
#if defined(FABBER_TEST_MULTIEXP_SP_2) || defined(FABBER_TEST_MULTIEXP_SP_4) || defined(FABBER_TEST_INVREC_SP)
#include "fabber_device_spatial_model.h"
#endif

#define FABBER_TEST_MULTIEXP "multiexp_sp"
#define FABBER_TEST_INVREC "invrec_sp"
#define FABBER_TEST_WITH "a device body and its spatial VB kernels"
#include "test_device_models.h"

#ifdef FABBER_TEST_MULTIEXP_WAVE
FABBER_DEVICE_MODEL(FABBER_TEST_MULTIEXP, MultiExpBody)
#endif
#ifdef FABBER_TEST_INVREC_WAVE
FABBER_DEVICE_MODEL(FABBER_TEST_INVREC, InvRecBody)
#endif
#ifdef FABBER_TEST_MULTIEXP_SP_2
FABBER_DEVICE_SPATIAL_MODEL(FABBER_TEST_MULTIEXP, MultiExpBody, 2)
#endif
#ifdef FABBER_TEST_MULTIEXP_SP_4
FABBER_DEVICE_SPATIAL_MODEL(FABBER_TEST_MULTIEXP, MultiExpBody, 4)
#endif
#ifdef FABBER_TEST_INVREC_SP
FABBER_DEVICE_SPATIAL_MODEL(FABBER_TEST_INVREC, InvRecBody, 3)
#endif
