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

// ---- device bodies ----------------------------------------------------------------------------------------------
namespace // (a body's kernels and launchers are template instantiations on it: keep its name to this library)
{
struct MultiExpSpBody
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
struct InvRecSpBody
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
FABBER_DEVICE_MODEL("multiexp_sp", MultiExpSpBody)
#endif
#ifdef FABBER_TEST_INVREC_WAVE
FABBER_DEVICE_MODEL("invrec_sp", InvRecSpBody)
#endif
#ifdef FABBER_TEST_MULTIEXP_SP_2
FABBER_DEVICE_SPATIAL_MODEL("multiexp_sp", MultiExpSpBody, 2)
#endif
#ifdef FABBER_TEST_MULTIEXP_SP_4
FABBER_DEVICE_SPATIAL_MODEL("multiexp_sp", MultiExpSpBody, 4)
#endif
#ifdef FABBER_TEST_INVREC_SP
FABBER_DEVICE_SPATIAL_MODEL("invrec_sp", InvRecSpBody, 3)
#endif

// ---- host side --------------------------------------------------------------------------------------------------
#ifdef FABBER_TEST_HOST
#include "fabber_core/fwdmodel.h"
#include "fabber_core/priors.h"
#include "fabber_core/transforms.h"

#include <cmath>
#include <string>
#include <vector>

class MultiExpSpFwdModel : public FwdModel
{
public:
    static FwdModel *NewInstance()
    {
        return new MultiExpSpFwdModel();
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
        return "sum of decaying exponentials: amp1 exp(-r1 t) + amp2 exp(-r2 t) + ... (with a device body and its spatial VB kernels)";
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
        spec.device_model = "multiexp_sp";
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

class InvRecSpFwdModel : public FwdModel
{
public:
    static FwdModel *NewInstance()
    {
        return new InvRecSpFwdModel();
    }
    void GetOptions(std::vector<OptionSpec> &opts) const
    {
        OptionSpec ti = { "ti<n>", OPT_FLOAT, "Inversion times, one per timepoint: ti1, ti2, ...", OPT_REQ, "" };
        opts.push_back(ti);
    }
    std::string GetDescription() const
    {
        return "inversion recovery: M0 (1 - 2 a exp(-TI / T1)) (with a device body and its spatial VB kernels)";
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
        spec.device_model = "invrec_sp";
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
    return index == 0 ? "multiexp_sp" : (index == 1 ? "invrec_sp" : 0);
}
NewInstanceFptr get_new_instance_func(const char *name)
{
    if (std::string(name) == "multiexp_sp")
        return MultiExpSpFwdModel::NewInstance;
    return std::string(name) == "invrec_sp" ? InvRecSpFwdModel::NewInstance : 0;
}
}
#endif
