// fwdmodel_spatial_noise_models.hip - a model library whose device bodies bring the spatial VB kernels (method=spatialvb)
// of every noise model a library can compile them for, written only against the public headers (fabber_core/*.h for the
// host side, include/fabber_device_*.h for the bodies). Every model has a host EvaluateModel - the host route of spatial VB
// to compare with - a device body for the wave-per-voxel kernels, a white-noise spatial entry and an AR(1) / noise-pattern
// spatial entry, each for its two parameters.
//
//   "multiexp_spn" : y(t) = amp exp(-r t), t = 0, dt, 2 dt, ... (option dt; the rate LOG-transformed; data-dependent
//                    initial posterior): the expression of the built-in exponential model with one exponential
//   "suppconv_sp"  : y_t = amp sum_{s = 0 .. t} supp_s exp(-r ((t - s) dt)) - an exponential residue function convolved
//                    with the voxel's input curve (the `suppdata` option of a run), the model of
//                    fwdmodel_supp_models.hip. For the unit impulse supp = (1, 0, 0, ...) this is the built-in
//                    exponential model's expression, term by term. A timepoint without a supplementary row is a
//                    non-finite prediction, never a read past the block. It also brings the result-image and the
//                    initial-posterior kernel.
//
// FABBER_TEST_PART = 1 .. 5 lets the sets of kernels be compiled side by side (1: host classes and both wave kernels,
// 2: both white-noise spatial entries, 3: multiexp_spn's AR(1) / noise-pattern spatial entry, 4: suppconv_sp's, 5:
// suppconv_sp's result-image and initial-posterior kernel); undefined = everything.
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 1
#define FABBER_TEST_HOST 1
#define FABBER_TEST_WAVE 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 2
#define FABBER_TEST_SP_WHITE 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 3
#define FABBER_TEST_MULTIEXP_SPN 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 4
#define FABBER_TEST_SUPP_SPN 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 5
#define FABBER_TEST_SUPP_IMAGES 1
#endif

#if defined(FABBER_TEST_WAVE)
#include "fabber_device_model.h"
#endif
#if defined(FABBER_TEST_SP_WHITE)
#include "fabber_device_spatial_model.h"
#endif
#if defined(FABBER_TEST_MULTIEXP_SPN) || defined(FABBER_TEST_SUPP_SPN)
#include "fabber_device_spatial_noise_model.h"
#endif
#if defined(FABBER_TEST_SUPP_IMAGES)
#include "fabber_device_results_model.h"
#include "fabber_device_init_model.h"
#endif

// ---- device bodies ----------------------------------------------------------------------------------------------
namespace // (a body's kernels and launchers are template instantiations on it: keep its name to this library)
{
struct MultiExpBody
{
    // a.dopt0 = dt: the expression of the built-in exponential model
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
};
struct SuppConvBody
{
    // p = (amp, r); a.dopt0 = dt; the voxel's input curve through fvb::supp_at
    static __device__ __forceinline__ double eval(const fvb::ModelArgs &a, int, int t, const double *p)
    {
        FVB_MODEL_FP
        if (t >= a.n_supp)
            return __builtin_nan("");
        double sum = 0;
        for (int s = 0; s <= t; s++)
        {
            const double tt = double(t - s) * a.dopt0;
            sum += fvb::supp_at(a, s) * exp(-p[1] * tt);
        }
        return p[0] * sum;
    }
#ifdef FABBER_TEST_SUPP_IMAGES
    // SuppConvFwdModel::InitVoxelPosterior
    static __device__ __forceinline__ void init_posterior(const fvb::ModelArgs &a, int, const fvb::VoxelSeries &y, double *means, double *)
    {
        if (a.n_supp < 1)
            return;
        const double s0 = fvb::supp_at(a, 0);
        if (s0 != 0)
            means[0] = y(0) / s0;
    }
#endif
};
} // namespace

// ---- host side --------------------------------------------------------------------------------------------------
#ifdef FABBER_TEST_HOST
#include "fabber_core/fwdmodel.h"
#include "fabber_core/priors.h"
#include "fabber_core/transforms.h"

#include <cmath>
#include <string>
#include <vector>

namespace
{
// what the two models share: the option dt and the parameters (amp, r) of the test libraries' exponential models
class TwoParameterFwdModel : public FwdModel
{
public:
    void GetOptions(std::vector<OptionSpec> &opts) const
    {
        OptionSpec dt = { "dt", OPT_FLOAT, "Time between samples", OPT_REQ, "" };
        opts.push_back(dt);
    }
    std::string ModelVersion() const
    {
        return "test";
    }
    void Initialize(FabberRunData &args)
    {
        FwdModel::Initialize(args);
        m_dt = args.GetDouble("dt", 0);
    }

protected:
    void GetParameterDefaults(std::vector<Parameter> &params) const
    {
        params.clear();
        params.push_back(Parameter(0, "amp", DistParams(1, 1e6), DistParams(1, 1e6)));
        params.push_back(Parameter(1, "r", DistParams(1, 100), DistParams(1, 1.5), PRIOR_NORMAL, TRANSFORM_LOG()));
    }
    double m_dt;
};

class MultiExpFwdModel : public TwoParameterFwdModel
{
public:
    static FwdModel *NewInstance()
    {
        return new MultiExpFwdModel();
    }
    std::string GetDescription() const
    {
        return "one decaying exponential amp exp(-r t), with a device body and its spatial VB kernels for every noise model";
    }
    void EvaluateModel(const NEWMAT::ColumnVector &params, NEWMAT::ColumnVector &result, const std::string & = "") const
    {
        result.ReSize(data.Nrows());
        for (int t = 1; t <= result.Nrows(); t++)
            result(t) = params(1) * std::exp(-params(2) * (double(t - 1) * m_dt));
    }
    // data-dependent initial posterior: the amplitude starts at the first sample
    void InitVoxelPosterior(MVNDist &posterior) const
    {
        posterior.means(1) = data(1);
    }
    bool GetDeviceModel(DeviceModelSpec &spec) const
    {
        spec.device_model = "multiexp_spn";
        spec.iopt[0] = 1;
        spec.dopt[0] = m_dt;
        return true;
    }
};

class SuppConvFwdModel : public TwoParameterFwdModel
{
public:
    static FwdModel *NewInstance()
    {
        return new SuppConvFwdModel();
    }
    std::string GetDescription() const
    {
        return "an exponential residue function convolved with the voxel's input curve (suppdata), with a device body that reads it "
               "and its spatial VB kernels for every noise model";
    }
    void EvaluateModel(const NEWMAT::ColumnVector &params, NEWMAT::ColumnVector &result, const std::string & = "") const
    {
        if (suppdata.Nrows() < data.Nrows())
            throw InvalidOptionValue("suppdata", stringify(suppdata.Nrows()) + " rows", "One row of supplementary data per timepoint is needed");
        result.ReSize(data.Nrows());
        for (int t = 1; t <= result.Nrows(); t++)
        {
            double sum = 0;
            for (int s = 1; s <= t; s++)
            {
                const double tt = double(t - s) * m_dt;
                sum += suppdata(s) * std::exp(-params(2) * tt);
            }
            result(t) = params(1) * sum;
        }
    }
    // data-dependent initial posterior: the amplitude that explains the first sample
    void InitVoxelPosterior(MVNDist &posterior) const
    {
        if (suppdata.Nrows() < 1)
            return;
        const double s0 = suppdata(1);
        if (s0 != 0)
            posterior.means(1) = data(1) / s0;
    }
    bool GetDeviceModel(DeviceModelSpec &spec) const
    {
        spec.device_model = "suppconv_sp";
        spec.dopt[0] = m_dt;
        spec.uses_suppdata = true;
        return true;
    }
};
} // namespace

// the three hooks fabber_load_models reads (fwdmodel.cc:25-27)
extern "C" {
int get_num_models()
{
    return 2;
}
const char *get_model_name(int index)
{
    return index == 0 ? "multiexp_spn" : (index == 1 ? "suppconv_sp" : 0);
}
NewInstanceFptr get_new_instance_func(const char *name)
{
    if (std::string(name) == "multiexp_spn")
        return MultiExpFwdModel::NewInstance;
    return std::string(name) == "suppconv_sp" ? SuppConvFwdModel::NewInstance : 0;
}
}
#endif

#ifdef FABBER_TEST_WAVE
FABBER_DEVICE_MODEL("multiexp_spn", MultiExpBody)
FABBER_DEVICE_MODEL("suppconv_sp", SuppConvBody)
#endif
#ifdef FABBER_TEST_SP_WHITE
FABBER_DEVICE_SPATIAL_MODEL("multiexp_spn", MultiExpBody, 2)
FABBER_DEVICE_SPATIAL_MODEL("suppconv_sp", SuppConvBody, 2)
#endif
#ifdef FABBER_TEST_MULTIEXP_SPN
FABBER_DEVICE_SPATIAL_NOISE_MODEL("multiexp_spn", MultiExpBody, 2, FVB_SPATIAL_NOISE_AR1 | FVB_SPATIAL_NOISE_PHIS)
#endif
#ifdef FABBER_TEST_SUPP_SPN
FABBER_DEVICE_SPATIAL_NOISE_MODEL("suppconv_sp", SuppConvBody, 2, FVB_SPATIAL_NOISE_AR1 | FVB_SPATIAL_NOISE_PHIS)
#endif
#ifdef FABBER_TEST_SUPP_IMAGES
FABBER_DEVICE_RESULTS_MODEL("suppconv_sp", SuppConvBody)
FABBER_DEVICE_INIT_MODEL("suppconv_sp", SuppConvBody)
#endif
