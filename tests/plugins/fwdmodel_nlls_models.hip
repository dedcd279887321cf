// fwdmodel_nlls_models.hip - a model library whose device bodies also bring the NLLS minimisers (method=nlls), written
// only against the public headers (fabber_core/*.h for the host side, include/fabber_device_model.h and
// include/fabber_device_nlls_model.h for the bodies). Every model has a host EvaluateModel, a device body for the
// wave-per-voxel VB kernels, the wave-per-voxel minimiser and lane-per-voxel minimisers for the parameter counts named
// below; every other count and small volumes stay on the wave minimiser.
//
//   "multiexp_nlls" : y(t) = sum_i amp_i exp(-r_i t), t = 0, dt, 2 dt, ... (options dt, num-exps; rates LOG-transformed):
//                     the expression of the built-in exponential model; lane minimisers for one and two exponentials
//                     (P = 2, 4)
//   "invrec_nlls"   : inversion recovery, y(t) = M0 (1 - 2 a exp(-TI_t / T1)); the inversion times are the options
//                     ti1, ti2, ... and reach the device body through the constants block; T1 LOG-transformed, the
//                     inversion efficiency a FRACTIONAL; lane minimiser for its three parameters
//
// FABBER_TEST_PART = 1 .. 5 lets the five sets of kernels be compiled side by side (1: host classes, multiexp_nlls's wave
// VB kernels and wave minimiser, 2: the same kernels of invrec_nlls, 3 / 4: multiexp_nlls's lane minimisers for P = 2 / 4,
// 5: invrec_nlls's lane minimiser); undefined = everything.
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
#include "fabber_device_nlls_model.h"

// ---- device bodies ----------------------------------------------------------------------------------------------
namespace // (a body's kernels and launchers are template instantiations on it: keep its name to this library)
{
struct MultiExpNllsBody
{
    // a.iopt0 = num-exps (P = 2 num-exps), a.dopt0 = dt: the expression of the built-in exponential model
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
struct InvRecNllsBody
{
    // p = (M0, T1, a); a.consts = the inversion times, one per timepoint. A timepoint without one is a non-finite
    // prediction (the voxel stops with the non-finite-offset status), never a read past the block
    static __device__ __forceinline__ double eval(const fvb::ModelArgs &a, int, int t, const double *p)
    {
        FVB_MODEL_FP
        if (t >= a.n_consts)
            return __builtin_nan("");
        return p[0] * (1.0 - 2.0 * p[2] * exp(-a.consts[t] / p[1]));
    }
};
} // namespace
#ifdef FABBER_TEST_MULTIEXP_WAVE
FABBER_DEVICE_MODEL("multiexp_nlls", MultiExpNllsBody)
FABBER_DEVICE_NLLS_MODEL("multiexp_nlls", MultiExpNllsBody)
#endif
#ifdef FABBER_TEST_INVREC_WAVE
FABBER_DEVICE_MODEL("invrec_nlls", InvRecNllsBody)
FABBER_DEVICE_NLLS_MODEL("invrec_nlls", InvRecNllsBody)
#endif
#ifdef FABBER_TEST_MULTIEXP_LANE_2
FABBER_DEVICE_NLLS_LANE_MODEL("multiexp_nlls", MultiExpNllsBody, 2)
#endif
#ifdef FABBER_TEST_MULTIEXP_LANE_4
FABBER_DEVICE_NLLS_LANE_MODEL("multiexp_nlls", MultiExpNllsBody, 4)
#endif
#ifdef FABBER_TEST_INVREC_LANE
FABBER_DEVICE_NLLS_LANE_MODEL("invrec_nlls", InvRecNllsBody, 3)
#endif

// ---- host side --------------------------------------------------------------------------------------------------
#ifdef FABBER_TEST_HOST
#include "fabber_core/fwdmodel.h"
#include "fabber_core/priors.h"
#include "fabber_core/transforms.h"

#include <cmath>
#include <string>
#include <vector>

class MultiExpNllsFwdModel : public FwdModel
{
public:
    static FwdModel *NewInstance()
    {
        return new MultiExpNllsFwdModel();
    }
    void GetOptions(std::vector<OptionSpec> &opts) const
    {
        OptionSpec dt = { "dt", OPT_FLOAT, "Time between samples", OPT_REQ, "" };
        OptionSpec num = { "num-exps", OPT_INT, "Number of exponentials", OPT_NONREQ, "1" };
        opts.push_back(dt);
        opts.push_back(num);
    }
    std::string GetDescription() const
    {
        return "sum of decaying exponentials: amp1 exp(-r1 t) + amp2 exp(-r2 t) + ... (with a device body and its NLLS minimisers)";
    }
    std::string ModelVersion() const
    {
        return "test";
    }
    void Initialize(FabberRunData &args)
    {
        FwdModel::Initialize(args);
        m_dt = args.GetDouble("dt", 0);
        m_num = args.GetIntDefault("num-exps", 1, 1);
    }
    void EvaluateModel(const NEWMAT::ColumnVector &params, NEWMAT::ColumnVector &result, const std::string & = "") const
    {
        result.ReSize(data.Nrows());
        for (int t = 1; t <= result.Nrows(); t++)
        {
            const double tt = double(t - 1) * m_dt;
            double sum = 0;
            for (int i = 0; i < m_num; i++)
                sum += params(2 * i + 1) * std::exp(-params(2 * i + 2) * tt);
            result(t) = sum;
        }
    }
    // data-dependent initial posterior: the first amplitude starts at the first sample
    void InitVoxelPosterior(MVNDist &posterior) const
    {
        posterior.means(1) = data(1);
    }
    bool GetDeviceModel(DeviceModelSpec &spec) const
    {
        spec.device_model = "multiexp_nlls";
        spec.iopt[0] = m_num;
        spec.dopt[0] = m_dt;
        return true;
    }

protected:
    void GetParameterDefaults(std::vector<Parameter> &params) const
    {
        params.clear();
        for (int i = 0; i < m_num; i++)
        {
            params.push_back(Parameter(2 * i, "amp" + stringify(i + 1), DistParams(1, 1e6), DistParams(1, 1e6)));
            params.push_back(Parameter(2 * i + 1, "r" + stringify(i + 1), DistParams(1, 100), DistParams(1, 1.5), PRIOR_NORMAL,
                TRANSFORM_LOG())); // (a LOG-transformed variance of exactly 1 is log(1) = 0 in Fabber space: a singular posterior)
        }
    }
    double m_dt;
    int m_num;
};

class InvRecNllsFwdModel : public FwdModel
{
public:
    static FwdModel *NewInstance()
    {
        return new InvRecNllsFwdModel();
    }
    void GetOptions(std::vector<OptionSpec> &opts) const
    {
        OptionSpec ti = { "ti<n>", OPT_FLOAT, "Inversion times, one per timepoint: ti1, ti2, ...", OPT_REQ, "" };
        opts.push_back(ti);
    }
    std::string GetDescription() const
    {
        return "inversion recovery: M0 (1 - 2 a exp(-TI / T1)) (with a device body and its NLLS minimisers)";
    }
    std::string ModelVersion() const
    {
        return "test";
    }
    void Initialize(FabberRunData &args)
    {
        FwdModel::Initialize(args);
        m_tis = args.GetDoubleList("ti", 0);
        if (m_tis.empty())
            throw InvalidOptionValue("ti1", "", "The inversion times ti1, ti2, ... are required");
    }
    void EvaluateModel(const NEWMAT::ColumnVector &params, NEWMAT::ColumnVector &result, const std::string & = "") const
    {
        if (data.Nrows() != (int)m_tis.size())
            throw InvalidOptionValue("ti<n>", stringify(m_tis.size()) + " values", "One inversion time per timepoint is needed");
        result.ReSize(data.Nrows());
        for (int t = 1; t <= result.Nrows(); t++)
            result(t) = params(1) * (1.0 - 2.0 * params(3) * std::exp(-m_tis[t - 1] / params(2)));
    }
    // M0 starts at the largest magnitude of the series
    void InitVoxelPosterior(MVNDist &posterior) const
    {
        double m = 0;
        for (int t = 1; t <= data.Nrows(); t++)
            m = std::fabs(data(t)) > m ? std::fabs(data(t)) : m;
        if (m > 0)
            posterior.means(1) = m;
    }
    bool GetDeviceModel(DeviceModelSpec &spec) const
    {
        spec.device_model = "invrec_nlls";
        spec.constants = m_tis;
        return true;
    }

protected:
    void GetParameterDefaults(std::vector<Parameter> &params) const
    {
        params.clear();
        params.push_back(Parameter(0, "M0", DistParams(1, 1e6), DistParams(1, 1e6)));
        params.push_back(Parameter(1, "T1", DistParams(1, 100), DistParams(1, 1.5), PRIOR_NORMAL, TRANSFORM_LOG()));
        params.push_back(Parameter(2, "a", DistParams(0.8, 4), DistParams(0.8, 1), PRIOR_NORMAL, TRANSFORM_FRACTIONAL()));
    }
    std::vector<double> m_tis;
};

// the three hooks fabber_load_models reads (fwdmodel.cc:25-27)
extern "C" {
int get_num_models()
{
    return 2;
}
const char *get_model_name(int index)
{
    return index == 0 ? "multiexp_nlls" : (index == 1 ? "invrec_nlls" : 0);
}
NewInstanceFptr get_new_instance_func(const char *name)
{
    if (std::string(name) == "multiexp_nlls")
        return MultiExpNllsFwdModel::NewInstance;
    return std::string(name) == "invrec_nlls" ? InvRecNllsFwdModel::NewInstance : 0;
}
}
#endif
