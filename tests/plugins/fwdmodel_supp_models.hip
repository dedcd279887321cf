// fwdmodel_supp_models.hip - a model library whose device body reads the voxel's SUPPLEMENTARY DATA (the `suppdata`
// option of a run: a per-voxel input curve), written only against the public headers (fabber_core/*.h for the host side,
// include/fabber_device_*.h for the body).
//
//   "suppconv" : y_t = amp sum_{s = 0 .. t} supp_s exp(-r ((t - s) dt)) - a residue function convolved with the voxel's
//                input curve, the shape of DSC and DCE models with a voxelwise arterial input function. Option dt; amp
//                untransformed, r LOG-transformed (the parameter defaults of the test libraries' multiexp model). For the
//                unit impulse supp = (1, 0, 0, ...) this is the built-in exponential model's expression, term by term:
//                the same association of -r (t dt), the weighted terms added up before the amplitude multiplies them.
//                A timepoint without a supplementary row is a non-finite prediction, never a read past the block.
//                The amplitude starts at data_0 / supp_0 where supp_0 is not zero.
//
// FABBER_TEST_PART = 1 .. 6 lets the sets of kernels be compiled side by side (1: host class and wave kernels, 2: lane
// kernels for P = 2, 3: AR(1) and noise-pattern lane kernels for P = 2, 4: the wave minimiser of method=nlls, 5: its lane
// minimiser for P = 2, 6: the result-image and the initial-posterior kernel); undefined = everything.
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 1
#define FABBER_TEST_HOST 1
#define FABBER_TEST_SUPP_WAVE 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 2
#define FABBER_TEST_SUPP_LANE 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 3
#define FABBER_TEST_SUPP_LANENZ 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 4
#define FABBER_TEST_SUPP_NLLS_WAVE 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 5
#define FABBER_TEST_SUPP_NLLS_LANE 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 6
#define FABBER_TEST_SUPP_IMAGES 1
#endif

#if defined(FABBER_TEST_SUPP_WAVE)
#include "fabber_device_model.h"
#endif
#if defined(FABBER_TEST_SUPP_LANE)
#include "fabber_device_lane_model.h"
#endif
#if defined(FABBER_TEST_SUPP_LANENZ)
#include "fabber_device_lane_noise_model.h"
#endif
#if defined(FABBER_TEST_SUPP_NLLS_WAVE) || defined(FABBER_TEST_SUPP_NLLS_LANE)
#include "fabber_device_nlls_model.h"
#endif
#if defined(FABBER_TEST_SUPP_IMAGES)
#include "fabber_device_results_model.h"
#include "fabber_device_init_model.h"
#endif

// ---- device body ------------------------------------------------------------------------------------------------
namespace // (a body's kernels and launchers are template instantiations on it: keep its name to this library)
{
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
class SuppConvFwdModel : public FwdModel
{
public:
    static FwdModel *NewInstance()
    {
        return new SuppConvFwdModel();
    }
    void GetOptions(std::vector<OptionSpec> &opts) const
    {
        OptionSpec dt = { "dt", OPT_FLOAT, "Time between samples", OPT_REQ, "" };
        opts.push_back(dt);
    }
    std::string GetDescription() const
    {
        return "an exponential residue function convolved with the voxel's input curve (suppdata), with a device body that reads it";
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
        spec.device_model = "suppconv";
        spec.dopt[0] = m_dt;
        spec.uses_suppdata = true;
        return true;
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
} // namespace

// the three hooks fabber_load_models reads (fwdmodel.cc:25-27)
extern "C" {
int get_num_models()
{
    return 1;
}
const char *get_model_name(int index)
{
    return index == 0 ? "suppconv" : 0;
}
NewInstanceFptr get_new_instance_func(const char *name)
{
    return std::string(name) == "suppconv" ? SuppConvFwdModel::NewInstance : 0;
}
}
#endif

#ifdef FABBER_TEST_SUPP_WAVE
FABBER_DEVICE_MODEL("suppconv", SuppConvBody)
#endif
#ifdef FABBER_TEST_SUPP_LANE
FABBER_DEVICE_LANE_MODEL("suppconv", SuppConvBody, 2)
#endif
#ifdef FABBER_TEST_SUPP_LANENZ
FABBER_DEVICE_LANE_NOISE_MODEL("suppconv", SuppConvBody, 2, FVB_LANE_NOISE_AR1 | FVB_LANE_NOISE_PHIS)
#endif
#ifdef FABBER_TEST_SUPP_NLLS_WAVE
FABBER_DEVICE_NLLS_MODEL("suppconv", SuppConvBody)
#endif
#ifdef FABBER_TEST_SUPP_NLLS_LANE
FABBER_DEVICE_NLLS_LANE_MODEL("suppconv", SuppConvBody, 2)
#endif
#ifdef FABBER_TEST_SUPP_IMAGES
FABBER_DEVICE_RESULTS_MODEL("suppconv", SuppConvBody)
FABBER_DEVICE_INIT_MODEL("suppconv", SuppConvBody)
#endif
