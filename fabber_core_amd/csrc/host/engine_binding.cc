// engine_binding.cc - see engine_binding.h
#include "engine_binding.h"

#include "priors.h"

#include <cstring>

using namespace std;
using NEWMAT::Matrix;

const void *engine_series(FabberRunData &rundata, bool as_matrix, int32_t &data_f64, int &rows, int &cols)
{
    const float *f32 = as_matrix ? NULL : rundata.GetMainVoxelDataF32(rows, cols);
    if (f32)
    {
        data_f64 = 0;
        return f32;
    }
    const Matrix &data = rundata.GetMainVoxelData();
    rows = data.Nrows();
    cols = data.Ncols();
    data_f64 = 1; // (rows = timepoints, columns = voxels)
    return data.Store();
}

void engine_suppdata(FabberRunData &rundata, fvb_config &cfg)
{
    const Matrix &supp = rundata.GetVoxelSuppData();
    const bool per_voxel = cfg.n_voxels > 0 && supp.Ncols() == cfg.n_voxels && supp.Nrows() > 0;
    cfg.model_supp = per_voxel ? supp.Store() : NULL;
    cfg.n_model_supp = per_voxel ? supp.Nrows() : 0;
}

const void *EngineBinding::Begin(FwdModel *model, FabberRunData &rundata)
{
    memset(&cfg, 0, sizeof(cfg));
    cfg.abi_version = FVB_ABI_VERSION;
    int rows = 0, cols = 0;
    const void *series = engine_series(rundata, false, cfg.data_f64, rows, cols);
    cfg.n_voxels = cols;
    cfg.n_times = rows;
    params.clear();
    model->GetParameters(rundata, params);
    if (params.size() > FVB_MAX_PARAMS_EXT)
        throw FabberInternalError("Models with more than " + stringify(FVB_MAX_PARAMS_EXT) + " parameters are not supported by the MI355X engine");
    cfg.n_params = (int)params.size();
    return series;
}

void EngineBinding::BindModel(FwdModel *model, FabberRunData &rundata, AcceptBody accept_body)
{
    DeviceModelSpec spec;
    has_device_model = model->GetDeviceModel(spec) && !rundata.GetBool("host-model");
    library_device_model = false;
    if (has_device_model && !spec.device_model.empty())
    {
        // (the block with the body named in it becomes cfg only once the technique has accepted the body)
        fvb_config named = cfg;
        const bool fits = spec.device_model.size() < sizeof(cfg.device_model);
        if (fits)
        {
            named.model = FVB_MODEL_PLUGIN;
            strncpy(named.device_model, spec.device_model.c_str(), sizeof(named.device_model) - 1);
            constants = spec.constants;
            named.model_consts = constants.empty() ? NULL : constants.data();
            named.n_model_consts = (int32_t)constants.size();
            if (spec.uses_suppdata)
                engine_suppdata(rundata, named);
        }
        has_device_model = library_device_model = accept_body(named, spec.device_model) && fits;
        if (library_device_model)
            cfg = named;
    }
    if (!has_device_model)
    {
        spec = DeviceModelSpec();
        spec.model = FVB_MODEL_HOSTJAC;
    }
    if (library_device_model)
        spec.model = FVB_MODEL_PLUGIN;
    uses_suppdata = library_device_model && spec.uses_suppdata;
    cfg.model = spec.model;
    for (int i = 0; i < 4; i++)
    {
        cfg.model_iopt[i] = spec.iopt[i];
        cfg.model_dopt[i] = spec.dopt[i];
    }
    if (spec.model == FVB_MODEL_LINEAR)
    {
        if (spec.design.Nrows() != cfg.n_times && cfg.n_voxels > 0)
            throw InvalidOptionValue("basis", stringify(spec.design.Nrows()) + " rows",
                "Design matrix length does not match the data (" + stringify(cfg.n_times) + " timepoints)");
        design = spec.design;
        cfg.design = design.Store();
    }
}

EngineBinding::Slots EngineBinding::ParameterSlots()
{
    if (!Wide())
        return { cfg.transform, cfg.prior_type, cfg.prior_mean, cfg.prior_var, cfg.prior_prec, cfg.post_mean, cfg.post_var, cfg.image_prior };
    // beyond FVB_MAX_PARAMS the per-parameter entries travel as a table (the wave-per-voxel kernels take such problems:
    // a built-in model - the engine says so where that is not the case)
    const int P = cfg.n_params;
    wide_ints.assign((size_t)2 * P, 0);
    wide_doubles.assign((size_t)5 * P, 0);
    wide_images.assign(P, (const double *)NULL);
    double *const d = wide_doubles.data();
    const Slots s = { wide_ints.data(), wide_ints.data() + P, d, d + P, d + 2 * P, d + 3 * P, d + 4 * P, wide_images.data() };
    wide = fvb_param_table{ s.transform, s.prior_type, s.prior_mean, s.prior_var, s.prior_prec, s.post_mean, s.post_var, s.image_prior };
    cfg.params_ext = &wide;
    return s;
}

void EngineBinding::BindParameters(FabberRunData &rundata, const MVNDist *minimiser_start)
{
    const Slots s = ParameterSlots();
    image_priors.assign(cfg.n_params, vector<double>());
    for (int k = 0; k < cfg.n_params; k++)
    {
        const Parameter &p = params[k];
        s.transform[k] = p.transform->DeviceCode();
        if (minimiser_start)
        {
            s.post_mean[k] = minimiser_start->means(k + 1); // Fabber space, as it is (inference_nlls.cc:131)
            continue;
        }
        s.prior_type[k] = Prior::DeviceCode(p.prior_type);
        s.prior_mean[k] = p.prior.mean();
        s.prior_var[k] = p.prior.var();
        s.prior_prec[k] = p.prior.prec();
        s.post_mean[k] = p.post.mean();
        s.post_var[k] = p.post.var();
        if (p.prior_type == PRIOR_IMAGE)
        {
            const Matrix &img = rundata.GetVoxelData(p.options.find("image")->second);
            if (img.Ncols() != cfg.n_voxels || img.Nrows() < 1)
                throw InvalidOptionValue("image prior", p.name, "Image prior must have one value per voxel");
            image_priors[k].resize(cfg.n_voxels);
            for (int v = 0; v < cfg.n_voxels; v++)
                image_priors[k][v] = img.at0(0, v);
            s.image_prior[k] = image_priors[k].data();
        }
    }
}

void engine_status_pass(const vector<int> &status, const Matrix &coords, bool halt, bool halt_in_setup, const char *const *reasons,
    int n_reasons, const char *const words[4], EasyLog *m_log)
{
    int n_bad = 0;
    for (int v = 0; v < (int)status.size(); v++)
    {
        const int code = status[v] & 0xff;
        if (code == 0)
            continue;
        const string msg = reasons[code < n_reasons ? code : 4];
        if (n_bad < 20)
            LOG << words[0] << v + 1 << " at " << coords.at0(0, v) << " " << coords.at0(1, v) << " " << coords.at0(2, v)
                << words[1] << msg << endl;
        n_bad++;
        if (halt || (halt_in_setup && (status[v] & 0x100) != 0))
            throw FabberInternalError(msg);
    }
    if (n_bad)
        LOG << words[2] << n_bad << words[3] << endl;
}
