// test_device_models.h - the two models of the test libraries with device bodies (fwdmodel_device_models.hip,
// fwdmodel_lane_models.hip, fwdmodel_nlls_models.hip, fwdmodel_spatial_models.hip), written only against the public
// headers: their device bodies, their host classes and the hooks of a model library.
//
//   FABBER_TEST_MULTIEXP : y(t) = sum_i amp_i exp(-r_i t), t = 0, dt, 2 dt, ... (options dt, num-exps; rates
//                          LOG-transformed; data-dependent initial posterior): the expression of the built-in
//                          exponential model
//   FABBER_TEST_INVREC   : inversion recovery, y(t) = M0 (1 - 2 a exp(-TI_t / T1)); the inversion times are the options
//                          ti1, ti2, ... and reach the device body through the constants block; T1 LOG-transformed, the
//                          inversion efficiency a FRACTIONAL
//
// The including file defines the two names as its library registers them (string literals) and FABBER_TEST_WITH, what
// the models' descriptions say they come with; it includes the header of include/ whose macros it uses first, this file
// next, and then writes its macro lines for MultiExpBody and InvRecBody. FABBER_TEST_HOST: the host classes and the
// hooks are compiled (one part of a library). FABBER_TEST_OWN_BODIES: the including file writes the bodies itself.
#ifndef FABBER_TEST_DEVICE_MODELS_H
#define FABBER_TEST_DEVICE_MODELS_H

#ifndef FABBER_TEST_OWN_BODIES
// ---- device bodies ----------------------------------------------------------------------------------------------
namespace // (a body's kernels and launchers are template instantiations on it: keep its name to this library)
{
struct MultiExpBody
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
struct InvRecBody
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
#endif

// ---- host side --------------------------------------------------------------------------------------------------
#ifdef FABBER_TEST_HOST
#include "fabber_core/fwdmodel.h"
#include "fabber_core/priors.h"
#include "fabber_core/transforms.h"

#include <cmath>
#include <string>
#include <vector>

namespace // (the libraries are loaded side by side: each keeps its classes to itself)
{
class MultiExpFwdModel : public FwdModel
{
public:
    static FwdModel *NewInstance()
    {
        return new MultiExpFwdModel();
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
        return "sum of decaying exponentials: amp1 exp(-r1 t) + amp2 exp(-r2 t) + ... (with " FABBER_TEST_WITH ")";
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
        spec.device_model = FABBER_TEST_MULTIEXP;
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

class InvRecFwdModel : public FwdModel
{
public:
    static FwdModel *NewInstance()
    {
        return new InvRecFwdModel();
    }
    void GetOptions(std::vector<OptionSpec> &opts) const
    {
        OptionSpec ti = { "ti<n>", OPT_FLOAT, "Inversion times, one per timepoint: ti1, ti2, ...", OPT_REQ, "" };
        opts.push_back(ti);
    }
    std::string GetDescription() const
    {
        return "inversion recovery: M0 (1 - 2 a exp(-TI / T1)) (with " FABBER_TEST_WITH ")";
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
        spec.device_model = FABBER_TEST_INVREC;
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
} // namespace

// the three hooks fabber_load_models reads (fwdmodel.cc:25-27)
extern "C" {
int get_num_models()
{
    return 2;
}
const char *get_model_name(int index)
{
    return index == 0 ? FABBER_TEST_MULTIEXP : (index == 1 ? FABBER_TEST_INVREC : 0);
}
NewInstanceFptr get_new_instance_func(const char *name)
{
    if (std::string(name) == FABBER_TEST_MULTIEXP)
        return MultiExpFwdModel::NewInstance;
    return std::string(name) == FABBER_TEST_INVREC ? InvRecFwdModel::NewInstance : 0;
}
}
#endif

#endif /* FABBER_TEST_DEVICE_MODELS_H */
