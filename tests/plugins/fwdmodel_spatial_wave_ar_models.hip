// fwdmodel_spatial_wave_ar_models.hip - a model library whose device bodies bring the WAVE-per-voxel spatial VB kernels
// under AR(1) NOISE (include/fabber_device_spatial_wave_ar_model.h: any parameter count up to FVB_MAX_PARAMS, one echo, no
// cross terms), written only against the public headers. None of the names has the white-noise line of
// fabber_device_spatial_wave_model.h or the pattern line of fabber_device_spatial_wave_noise_model.h: the AR line needs
// neither.
//
//   "multiexp_spwa"      : the sum of exponentials of test_device_models.h (P = 2 num-exps), the wave AR line only
//   "linear_spwa"        : y(t) = sum_i p[i] consts[t P + i], the body of fwdmodel_spatial_wave_models.hip's linear_spw (a
//                          device body only: no host class of this name)
//   "suppconv_spwa"      : the body of fwdmodel_supp_models.hip, which reads the voxel's supplementary data (P = 2; a device
//                          body only)
//   "multiexp_spwa_both" : the sum of exponentials with a lane spatial noise line for P = 4 (the AR(1) family) next to the
//                          wave AR line (a device body only)
//
// FABBER_TEST_PART = 1 .. 6 lets the kernels be compiled side by side (1: host class and the wave kernels of voxelwise VB
// for the sum of exponentials, 2: the spatial wave AR kernels of multiexp_spwa and multiexp_spwa_both, 3: those of
// linear_spwa and suppconv_spwa, 4: the lane spatial AR(1) kernels of multiexp_spwa_both for P = 4, 5 and 6: the wave
// kernels of voxelwise VB for linear_spwa and for suppconv_spwa); undefined = everything.
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 1
#define FABBER_TEST_HOST 1
#define FABBER_TEST_SPWA_BODIES 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 2
#define FABBER_TEST_SPWA_EXP 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 3
#define FABBER_TEST_SPWA_LINEAR 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 4
#define FABBER_TEST_SPWA_LANE 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 5
#define FABBER_TEST_SPWA_BODY_LINEAR 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 6
#define FABBER_TEST_SPWA_BODY_SUPP 1
#endif

#include "fabber_device_model.h"
#if defined(FABBER_TEST_SPWA_EXP) || defined(FABBER_TEST_SPWA_LINEAR)
#include "fabber_device_spatial_wave_ar_model.h"
#endif
#if defined(FABBER_TEST_SPWA_LANE)
#include "fabber_device_spatial_noise_model.h"
#endif

#define FABBER_TEST_MULTIEXP "multiexp_spwa"
#define FABBER_TEST_INVREC "invrec_spwa" // (the header's second model: its host class is compiled, the library does not list it)
#define FABBER_TEST_WITH "the wave-per-voxel spatial VB kernels under AR(1) noise"
// the header's loader hooks are those of its own two models: this library writes its own below
#define get_num_models fabber_test_header_num_models
#define get_model_name fabber_test_header_model_name
#define get_new_instance_func fabber_test_header_new_instance_func
#include "test_device_models.h"
#undef get_num_models
#undef get_model_name
#undef get_new_instance_func

// SuppConvBody, the body alone (no part of that source is 99: no host class, no hooks, no macro line)
#pragma push_macro("FABBER_TEST_PART")
#undef FABBER_TEST_PART
#define FABBER_TEST_PART 99
#pragma push_macro("FABBER_TEST_HOST")
#undef FABBER_TEST_HOST
#include "fwdmodel_supp_models.hip"
#pragma pop_macro("FABBER_TEST_HOST")
#pragma pop_macro("FABBER_TEST_PART")

namespace
{
struct LinearSpwaBody
{
    static __device__ __forceinline__ double eval(const fvb::ModelArgs &a, int P, int t, const double *p)
    {
        FVB_MODEL_FP
        if ((t + 1) * P > a.n_consts)
            return __builtin_nan("");
        const double *row = a.consts + (size_t)t * P; // (the expression of the built-in linear model: the same order and zeros)
        double s = 0;
        for (int j = 0; j < P; j++)
            s += row[j] * (p[j] - 0.0);
        return s + 0.0;
    }
};
} // namespace

#ifdef FABBER_TEST_HOST
// the three hooks fabber_load_models reads (fwdmodel.cc:25-27)
extern "C" {
int get_num_models()
{
    return 1;
}
const char *get_model_name(int index)
{
    return index == 0 ? "multiexp_spwa" : 0;
}
NewInstanceFptr get_new_instance_func(const char *name)
{
    return std::string(name) == "multiexp_spwa" ? MultiExpFwdModel::NewInstance : 0;
}
}
#endif

#ifdef FABBER_TEST_SPWA_BODIES
FABBER_DEVICE_MODEL("multiexp_spwa", MultiExpBody)
FABBER_DEVICE_MODEL("multiexp_spwa_both", MultiExpBody)
#endif
#ifdef FABBER_TEST_SPWA_BODY_LINEAR
FABBER_DEVICE_MODEL("linear_spwa", LinearSpwaBody)
#endif
#ifdef FABBER_TEST_SPWA_BODY_SUPP
FABBER_DEVICE_MODEL("suppconv_spwa", SuppConvBody)
#endif
#ifdef FABBER_TEST_SPWA_EXP
FABBER_DEVICE_SPATIAL_WAVE_AR_MODEL("multiexp_spwa", MultiExpBody)
FABBER_DEVICE_SPATIAL_WAVE_AR_MODEL("multiexp_spwa_both", MultiExpBody)
#endif
#ifdef FABBER_TEST_SPWA_LINEAR
FABBER_DEVICE_SPATIAL_WAVE_AR_MODEL("linear_spwa", LinearSpwaBody)
FABBER_DEVICE_SPATIAL_WAVE_AR_MODEL("suppconv_spwa", SuppConvBody)
#endif
#ifdef FABBER_TEST_SPWA_LANE
FABBER_DEVICE_SPATIAL_NOISE_MODEL("multiexp_spwa_both", MultiExpBody, 4, FVB_SPATIAL_NOISE_AR1)
#endif
