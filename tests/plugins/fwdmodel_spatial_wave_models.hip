// fwdmodel_spatial_wave_models.hip - a model library whose device bodies bring the WAVE-per-voxel spatial VB kernels
// (include/fabber_device_spatial_wave_model.h: any parameter count up to FVB_MAX_PARAMS), written only against the public
// headers.
//
//   "multiexp_spw"  : the sum of exponentials of test_device_models.h (P = 2 num-exps), the wave line only
//   "linear_spw"    : y(t) = sum_i p[i] consts[t P + i] - the design travels in the constants block, row by row; a
//                     timepoint whose row is not wholly inside the block is a non-finite prediction, never a read past it.
//                     Option basis (the design matrix of model=linear)
//   "suppconv_spw"  : the body of fwdmodel_supp_models.hip, which reads the voxel's supplementary data (P = 2): the wave
//                     line and no lane spatial line, so two parameters take the wave-per-voxel kernels
//   "multiexp_both" : the sum of exponentials with a lane spatial line for P = 2 next to the wave line (a device body
//                     only: no host class of this name)
//
// FABBER_TEST_PART = 1 .. 6 lets the kernels be compiled side by side (1: host classes and the wave kernels of voxelwise VB
// for the sum of exponentials, 2: the spatial wave kernels of multiexp_spw and multiexp_both, 3: those of linear_spw and
// suppconv_spw, 4: the lane spatial kernels of multiexp_both for P = 2, 5 and 6: the wave kernels of voxelwise VB for
// linear_spw and for suppconv_spw); undefined = everything.
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 1
#define FABBER_TEST_HOST 1
#define FABBER_TEST_SPW_BODIES 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 2
#define FABBER_TEST_SPW_EXP 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 3
#define FABBER_TEST_SPW_LINEAR 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 4
#define FABBER_TEST_SPW_LANE 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 5
#define FABBER_TEST_SPW_BODY_LINEAR 1
#endif
#if !defined(FABBER_TEST_PART) || FABBER_TEST_PART == 6
#define FABBER_TEST_SPW_BODY_SUPP 1
#endif

#include "fabber_device_model.h"
#if defined(FABBER_TEST_SPW_EXP) || defined(FABBER_TEST_SPW_LINEAR)
#include "fabber_device_spatial_wave_model.h"
#endif
#if defined(FABBER_TEST_SPW_LANE)
#include "fabber_device_spatial_model.h"
#endif

#define FABBER_TEST_MULTIEXP "multiexp_spw"
#define FABBER_TEST_INVREC "invrec_spw" // (the header's second model: its host class is compiled, the library does not list it)
#define FABBER_TEST_WITH "the wave-per-voxel spatial VB kernels"
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
struct LinearSpwBody
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

// ---- host side --------------------------------------------------------------------------------------------------
#ifdef FABBER_TEST_HOST
#include "fabber_core/tools.h"

namespace
{
class LinearSpwFwdModel : public FwdModel
{
public:
    static FwdModel *NewInstance()
    {
        return new LinearSpwFwdModel();
    }
    void GetOptions(std::vector<OptionSpec> &opts) const
    {
        OptionSpec basis = { "basis", OPT_MATRIX, "Design matrix", OPT_REQ, "" };
        opts.push_back(basis);
    }
    std::string GetDescription() const
    {
        return "a linear combination of the columns of a design matrix (with " FABBER_TEST_WITH ")";
    }
    std::string ModelVersion() const
    {
        return "test";
    }
    void Initialize(FabberRunData &args)
    {
        FwdModel::Initialize(args);
        m_design = fabber::read_matrix_file(args.GetString("basis"));
    }
    void EvaluateModel(const NEWMAT::ColumnVector &params, NEWMAT::ColumnVector &result, const std::string & = "") const
    {
        result.ReSize(m_design.Nrows());
        for (int t = 1; t <= m_design.Nrows(); t++)
        {
            double s = 0;
            for (int j = 1; j <= m_design.Ncols(); j++)
                s += m_design(t, j) * params(j);
            result(t) = s;
        }
    }
    bool GetDeviceModel(DeviceModelSpec &spec) const
    {
        spec.device_model = "linear_spw";
        spec.constants.clear();
        for (int t = 1; t <= m_design.Nrows(); t++)
            for (int j = 1; j <= m_design.Ncols(); j++)
                spec.constants.push_back(m_design(t, j));
        return true;
    }

protected:
    void GetParameterDefaults(std::vector<Parameter> &params) const
    {
        params.clear();
        for (int i = 0; i < m_design.Ncols(); i++)
            params.push_back(Parameter(i, "Parameter_" + stringify(i + 1), DistParams(0, 1e12), DistParams(0, 1e12)));
    }
    NEWMAT::Matrix m_design;
};

// the host class of fwdmodel_supp_models.hip's "suppconv" under this library's name
class SuppConvSpwFwdModel : public FwdModel
{
public:
    static FwdModel *NewInstance()
    {
        return new SuppConvSpwFwdModel();
    }
    void GetOptions(std::vector<OptionSpec> &opts) const
    {
        OptionSpec dt = { "dt", OPT_FLOAT, "Time between samples", OPT_REQ, "" };
        opts.push_back(dt);
    }
    std::string GetDescription() const
    {
        return "an exponential residue function convolved with the voxel's input curve (suppdata) (with " FABBER_TEST_WITH ")";
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
                sum += suppdata(s) * std::exp(-params(2) * (double(t - s) * m_dt));
            result(t) = params(1) * sum;
        }
    }
    bool GetDeviceModel(DeviceModelSpec &spec) const
    {
        spec.device_model = "suppconv_spw";
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
    return 3;
}
const char *get_model_name(int index)
{
    return index == 0 ? "multiexp_spw" : (index == 1 ? "linear_spw" : (index == 2 ? "suppconv_spw" : 0));
}
NewInstanceFptr get_new_instance_func(const char *name)
{
    if (std::string(name) == "multiexp_spw")
        return MultiExpFwdModel::NewInstance;
    if (std::string(name) == "linear_spw")
        return LinearSpwFwdModel::NewInstance;
    return std::string(name) == "suppconv_spw" ? SuppConvSpwFwdModel::NewInstance : 0;
}
}
#endif

#ifdef FABBER_TEST_SPW_BODIES
FABBER_DEVICE_MODEL("multiexp_spw", MultiExpBody)
FABBER_DEVICE_MODEL("multiexp_both", MultiExpBody)
#endif
#ifdef FABBER_TEST_SPW_BODY_LINEAR
FABBER_DEVICE_MODEL("linear_spw", LinearSpwBody)
#endif
#ifdef FABBER_TEST_SPW_BODY_SUPP
FABBER_DEVICE_MODEL("suppconv_spw", SuppConvBody)
#endif
#ifdef FABBER_TEST_SPW_EXP
FABBER_DEVICE_SPATIAL_WAVE_MODEL("multiexp_spw", MultiExpBody)
FABBER_DEVICE_SPATIAL_WAVE_MODEL("multiexp_both", MultiExpBody)
#endif
#ifdef FABBER_TEST_SPW_LINEAR
FABBER_DEVICE_SPATIAL_WAVE_MODEL("linear_spw", LinearSpwBody)
FABBER_DEVICE_SPATIAL_WAVE_MODEL("suppconv_spw", SuppConvBody)
#endif
#ifdef FABBER_TEST_SPW_LANE
FABBER_DEVICE_SPATIAL_MODEL("multiexp_both", MultiExpBody, 2)
#endif
