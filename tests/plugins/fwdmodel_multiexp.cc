// fwdmodel_multiexp.cc - a model library in the shape of the reference's example library: a sum of decaying
// exponentials, written only against the public plugin surface, with no device body and no knowledge of the
// GPU engine. It reaches the model factory both ways a library written for the reference does:
//
//   "multiexp" : static registration, FactoryRegistration<FwdModelFactory, ...> (fabber_core/factories.h)
//   "exp"      : the three extern "C" hooks fabber_load_models reads (fwdmodel.cc:25-27)
//
// y(t) = sum_i amp_i * exp(-r_i t),  t = 0, dt, 2 dt, ...  (i = 1 .. num-exps; dt required, r_i LOG-transformed)
#include "fabber_core/factories.h"
#include "fabber_core/fwdmodel.h"
#include "fabber_core/priors.h"
#include "fabber_core/transforms.h"

#include <cmath>
#include <string>
#include <vector>

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
        return "sum of decaying exponentials: amp1 exp(-r1 t) + amp2 exp(-r2 t) + ...";
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
            double sum = 0;
            for (int i = 0; i < m_num; i++)
                sum += params(2 * i + 1) * std::exp(-params(2 * i + 2) * (t - 1) * m_dt);
            result(t) = sum;
        }
    }
    // data-dependent initial posterior: the first amplitude starts at the first sample
    void InitVoxelPosterior(MVNDist &posterior) const
    {
        posterior.means(1) = data(1);
    }

protected:
    void GetParameterDefaults(std::vector<Parameter> &params) const
    {
        params.clear();
        for (int i = 0; i < m_num; i++)
        {
            params.push_back(Parameter(2 * i, "amp" + stringify(i + 1), DistParams(1, 1e6), DistParams(1, 1e6)));
            params.push_back(Parameter(2 * i + 1, "r" + stringify(i + 1), DistParams(1, 100), DistParams(1, 1), PRIOR_NORMAL,
                TRANSFORM_LOG()));
        }
    }
    double m_dt;
    int m_num;
};

static FactoryRegistration<FwdModelFactory, MultiExpFwdModel> registration("multiexp");

extern "C" {
int get_num_models()
{
    return 1;
}
const char *get_model_name(int index)
{
    return index == 0 ? "exp" : 0;
}
NewInstanceFptr get_new_instance_func(const char *name)
{
    return std::string(name) == "exp" ? MultiExpFwdModel::NewInstance : 0;
}
}
