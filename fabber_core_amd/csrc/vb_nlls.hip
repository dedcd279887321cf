/*
 * vb_nlls.hip - instantiations and C ABI of the non-linear least squares kernel
 * (vb_nlls_kernel.h; method=nlls, inference_nlls.cc), and the registry of the minimisers that model libraries compile
 * around their device bodies (include/fabber_device_nlls_model.h).
 */
#include "vb_nlls_launch.h"

#include "vb_device_registry.h"

#include <string>
#include <vector>

using namespace fvb;

namespace fvb
{
#define FVB_NLLS_CASE(MODEL, TAG, PP)                                                                        \
    case PP:                                                                                                 \
        return NllsKernelInfo{ nlls_lane_kernel<MODEL<PP>, PP>, "nlls<" TAG "," #PP ">" };

NllsKernelInfo get_nlls_kernel(int model, int P)
{
    switch (model)
    {
    case FVB_MODEL_POLY:
        switch (P)
        {
            FVB_NLLS_CASE(PolyModel, "poly", 1)
            FVB_NLLS_CASE(PolyModel, "poly", 2)
            FVB_NLLS_CASE(PolyModel, "poly", 3)
            FVB_NLLS_CASE(PolyModel, "poly", 4)
            FVB_NLLS_CASE(PolyModel, "poly", 5)
            FVB_NLLS_CASE(PolyModel, "poly", 6)
        }
        break;
    case FVB_MODEL_LINEAR:
        switch (P)
        {
            FVB_NLLS_CASE(LinearModel, "linear", 1)
            FVB_NLLS_CASE(LinearModel, "linear", 2)
            FVB_NLLS_CASE(LinearModel, "linear", 3)
            FVB_NLLS_CASE(LinearModel, "linear", 4)
            FVB_NLLS_CASE(LinearModel, "linear", 5)
            FVB_NLLS_CASE(LinearModel, "linear", 6)
        }
        break;
    case FVB_MODEL_EXP:
        switch (P)
        {
            FVB_NLLS_CASE(ExpModel, "exp", 2)
            FVB_NLLS_CASE(ExpModel, "exp", 4)
            FVB_NLLS_CASE(ExpModel, "exp", 6)
        }
        break;
    }
    return NllsKernelInfo{ nullptr, nullptr };
}

// The NLLS minimisers of device bodies that model libraries have registered (include/fabber_device_nlls_model.h), by
// (name, parameter count; 0 = the wave-per-voxel minimiser).
template <> struct DeviceRegistryTraits<fvb_device_nlls_model>
{
    static constexpr const char *noun = "device NLLS model", *is = "is";
    static constexpr int first_code = -70;
    static std::vector<DeviceStructSize> sizes(const fvb_device_nlls_model &m)
    {
        return { { "NllsArgs", m.nlls_args_size, sizeof(NllsArgs) }, { "WaveLayout", m.wave_layout_size, sizeof(WaveLayout) } };
    }
    static const char *bad_params(const fvb_device_nlls_model &m)
    {
        return (m.n_params < 0 || m.n_params > 6) ? "0 = the wave minimiser; the lane minimisers of a library body exist for 1 to 6" : nullptr;
    }
    static std::string entry(const std::string &name, int n_params)
    {
        return n_params == 0 ? "the wave NLLS minimiser of a device model named '" + name + "'"
                             : "the lane NLLS minimiser of a device model named '" + name + "' with " + std::to_string(n_params) + " parameters";
    }
    static std::string absent(const std::string &name, int n_params)
    {
        return entry(name, n_params) + " is not registered";
    }
};
} // namespace fvb

namespace
{
// what a configuration runs on
struct NllsRoute
{
    bool lane = false;
    NllsKernelInfo builtin = { nullptr, nullptr };  // the built-in model's lane minimiser, if it has one for the count
    fvb_device_nlls_launch_fn library = nullptr;    // FVB_MODEL_PLUGIN: the launcher of the entry taken
    std::string name;                               // fabber_nlls_kernel_name
};

// the configuration's side of the checks, and the route
// (nl: the minimiser's settings, checked where a run checks them; NULL = the configuration alone)
int select_nlls(const fvb_config *cfg, NllsRoute &route, const fvb_nlls *nl = nullptr)
{
    if (!cfg)
        return api_fail(-1, "config is NULL");
    if (cfg->abi_version != FVB_ABI_VERSION)
        return api_fail(-2, "fvb_config.abi_version mismatch");
    if (cfg->n_voxels < 0 || cfg->n_times <= 0)
        return api_fail(-3, "bad n_voxels / n_times");
    if (cfg->n_params <= 0 || cfg->n_params > (cfg->params_ext ? FVB_MAX_PARAMS_EXT : FVB_MAX_PARAMS))
        return api_fail(-4, "n_params out of range (more than FVB_MAX_PARAMS parameters: fvb_config.params_ext)");
    if (cfg->model == FVB_MODEL_LINEAR && !cfg->design)
        return api_fail(-10, "linear model needs a design matrix");
    if (cfg->model == FVB_MODEL_EXP && (cfg->n_params != 2 * cfg->model_iopt[0]))
        return api_fail(-11, "exp model: n_params != 2 * num-exps");
    if (cfg->model == FVB_MODEL_POLY && (cfg->n_params != cfg->model_iopt[0] + 1))
        return api_fail(-12, "poly model: n_params != degree + 1");
    if (nl && (nl->max_iterations < 0 || !(nl->lambda0 > 0) || !(nl->lambda_max > 0)))
        return api_fail(-60, "bad minimiser settings");
    const bool wave_fits = nlls_wave_layout(*cfg).bytes <= WAVE_LDS_PER_WORKGROUP_MAX;
    const char *no_kernel = "no NLLS kernel for this problem: no lane instantiation for the model / parameter count and the "
                            "series does not fit the 160 KB of LDS the wave-per-voxel kernel needs";
    if (cfg->model == FVB_MODEL_PLUGIN) // a body of a model library: with the NLLS entries its library registered
    {
        if (int rc = check_device_model_config(cfg))
            return rc;
        const std::string name = config_device_model(cfg);
        DeviceRegistry<fvb_device_nlls_model> &entries = DeviceRegistry<fvb_device_nlls_model>::instance();
        fvb_device_nlls_model wave, lane;
        if (!entries.find(name, 0, &wave))
            return api_fail(-61, "method=nlls needs a forward model with a device body");
        const bool has_lane = cfg->n_params <= 6 && !cfg->params_ext && entries.find(name, cfg->n_params, &lane);
        route.lane = nlls_takes_lane(has_lane, api_variant(), *cfg);
        if (!route.lane && !wave_fits)
            return api_fail(-61, no_kernel);
        route.library = route.lane ? lane.launch : wave.launch;
        route.name = route.lane ? "nlls<" + name + "," + std::to_string(cfg->n_params) + ">" : "nlls_wave<" + name + ">";
        return 0;
    }
    if (cfg->model != FVB_MODEL_POLY && cfg->model != FVB_MODEL_LINEAR && cfg->model != FVB_MODEL_EXP)
        return api_fail(-61, "method=nlls needs a forward model with a device body");
    if (!cfg->params_ext)
        route.builtin = get_nlls_kernel(cfg->model, cfg->n_params);
    if (!route.builtin.fn && !wave_fits)
        return api_fail(-61, no_kernel);
    route.lane = nlls_takes_lane(route.builtin.fn != nullptr, api_variant(), *cfg);
    route.name = route.lane ? route.builtin.name : "nlls_wave";
    return 0;
}

int validate_nlls(const fvb_config *cfg, const fvb_nlls *nl, NllsRoute &route)
{
    if (!cfg || !nl)
        return api_fail(-1, "config is NULL");
    return select_nlls(cfg, route, nl);
}
thread_local std::string g_nlls_kernel_name;
} // namespace

extern "C" {

void fabber_nlls_defaults(fvb_nlls *nl)
{
    nl->lm = 0;
    nl->max_iterations = 200;
    nl->cf_tolerance = 1e-8;
    nl->lambda0 = 0.1;
    nl->lambda_max = 1e20;
}

int32_t fabber_vb_register_device_nlls_model(const fvb_device_nlls_model *model)
{
    return DeviceRegistry<fvb_device_nlls_model>::instance().add(model);
}

int32_t fabber_vb_unregister_device_nlls_model(const char *name, int32_t n_params)
{
    return DeviceRegistry<fvb_device_nlls_model>::instance().remove(name, n_params);
}

int32_t fabber_vb_device_nlls_model_count(void)
{
    return DeviceRegistry<fvb_device_nlls_model>::instance().count();
}

const char *fabber_vb_device_nlls_model_name(int32_t i)
{
    return DeviceRegistry<fvb_device_nlls_model>::instance().name(i);
}

int32_t fabber_vb_device_nlls_model_params(int32_t i)
{
    return DeviceRegistry<fvb_device_nlls_model>::instance().params(i, -1);
}

const char *fabber_nlls_kernel_name(const fvb_config *cfg)
{
    NllsRoute route;
    if (select_nlls(cfg, route) != 0)
        return "";
    g_nlls_kernel_name = route.name;
    return g_nlls_kernel_name.c_str();
}

int32_t fabber_nlls_run_device(const fvb_config *cfg, const fvb_nlls *nl, const void *data, const fvb_outputs *out,
    void *stream, int32_t n_unmasked)
{
    NllsRoute route;
    int rc = validate_nlls(cfg, nl, route);
    if (rc)
        return rc;
    if (!out || !out->mvn)
        return api_fail(-20, "outputs.mvn is required");
    if (cfg->n_voxels == 0)
        return 0;
    if (!data)
        return api_fail(-21, "data is NULL");
    NllsArgs na;
    memset(&na, 0, sizeof(na));
    na.ka.cfg = *cfg;
    na.ka.out = *out;
    na.ka.data = data;
    na.ka.n_unmasked = n_unmasked;
    na.nl = *nl;
    if (route.library) // the minimiser lives in the model library's code object
    {
        char err[512] = "";
        rc = route.library(&na, stream, err, (int32_t)sizeof(err));
        return rc ? api_fail(rc, err[0] ? err : "the NLLS launcher of the device model failed") : 0;
    }
    std::string err;
    rc = launch_nlls_kernel(route.builtin.fn, nlls_wave_kernel<BuiltinEval>, route.lane ? NLLS_VARIANT_LANE : NLLS_VARIANT_WAVE, na,
        (hipStream_t)stream, err);
    return rc ? api_fail(rc, err) : 0;
}

int32_t fabber_nlls_run_host(const fvb_config *cfg, const fvb_nlls *nl, const void *data, const fvb_outputs *out,
    int32_t device)
{
    NllsRoute route;
    int rc = validate_nlls(cfg, nl, route);
    if (rc)
        return rc;
    if (!out || !out->mvn)
        return api_fail(-20, "outputs.mvn is required");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return api_fail(-30, "no HIP device available (the engine has no CPU fallback)");
    FVB_HIP_CHECK(hipSetDevice(device));
    const size_t V = (size_t)cfg->n_voxels, T = (size_t)cfg->n_times;
    if (V == 0)
        return 0;
    if (!data)
        return api_fail(-21, "data is NULL");
    const int P = cfg->n_params;
    const size_t rows = (size_t)P * (P + 1) / 2 + P + 1;
    StagedProblem staged;
    if ((rc = staged.stage_in(cfg, data, out, rows, 0, V, nullptr, from_malloc(), STAGE_NLLS)) != 0)
        return rc;
    rc = fabber_nlls_run_device(&staged.d, nl, staged.b_data.p, &staged.dout, nullptr, count_unmasked(T, cfg->phi_index));
    if (rc)
        return rc;
    FVB_HIP_CHECK(hipDeviceSynchronize());
    return staged.stage_out(out, nullptr);
}

// method=nlls with a forward model that exists only as host code: the minimiser's iterations run on the device,
// one launch of nlls_wave_step_kernel per trial point; the caller's callback evaluates the model (prediction and
// Jacobian about the trial point, as LinearizedFwdModel::ReCentre - NLLSCF::cf / grad / hess of
// inference_nlls.cc:223-290 use nothing else) for the voxels still running, in batches of two buffers so that the
// host works on the next batch while the device steps the current one.
int32_t fabber_nlls_run_hostmodel_host(const fvb_config *cfg, const fvb_nlls *nl, const void *data, const fvb_outputs *out,
    int32_t device, fvb_linearise_fn linearise, void *user)
{
    if (!cfg || !nl)
        return api_fail(-1, "config is NULL");
    if (cfg->abi_version != FVB_ABI_VERSION)
        return api_fail(-2, "fvb_config.abi_version mismatch");
    if (cfg->n_voxels < 0 || cfg->n_times <= 0)
        return api_fail(-3, "bad n_voxels / n_times");
    if (cfg->n_params <= 0 || cfg->n_params > FVB_MAX_PARAMS)
        return api_fail(-4, "n_params out of range");
    if (cfg->model != FVB_MODEL_HOSTJAC)
        return api_fail(-61, "fabber_nlls_run_hostmodel_host is for models evaluated on the host (FVB_MODEL_HOSTJAC)");
    if (nl->max_iterations < 0 || !(nl->lambda0 > 0) || !(nl->lambda_max > 0))
        return api_fail(-60, "bad minimiser settings");
    if (!linearise)
        return api_fail(-50, "linearisation callback is NULL");
    if (!out || !out->mvn)
        return api_fail(-20, "outputs.mvn is required");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return api_fail(-30, "no HIP device available (the engine has no CPU fallback)");
    FVB_HIP_CHECK(hipSetDevice(device));
    const size_t V = (size_t)cfg->n_voxels, T = (size_t)cfg->n_times;
    if (V == 0)
        return 0;
    if (!data)
        return api_fail(-21, "data is NULL");
    const int P = cfg->n_params;
    const size_t rows = (size_t)P * (P + 1) / 2 + P + 1;
    const WaveLayout L = wave_layout((int)T, P, 1);
    if (L.bytes > 160 * 1024)
        return api_fail(-41, "NLLS step kernel: " + std::to_string(L.bytes) + " bytes of LDS needed exceed the 160 KB of a gfx950 CU");

    fvb_config host_model = *cfg;
    host_model.design = nullptr;
    StagedProblem staged;
    int rc = staged.stage_in(&host_model, data, out, rows, 0, V, nullptr, from_malloc(), STAGE_NLLS);
    if (rc)
        return rc;
    NllsHmArgs ha;
    memset(&ha, 0, sizeof(ha));
    ha.na.ka.cfg = staged.d;
    ha.na.ka.out = staged.dout;
    ha.na.ka.data = staged.b_data.p;
    ha.na.ka.n_unmasked = count_unmasked(T, cfg->phi_index);
    ha.na.nl = *nl;
    ha.L = L;
    ha.persist_doubles = L.part - L.b;
    DevMem b_persist, b_scalars;
    FVB_HIP_CHECK(b_persist.alloc(sizeof(double) * (size_t)ha.persist_doubles * V, nullptr, from_malloc()));
    FVB_HIP_CHECK(b_scalars.alloc(sizeof(NllsHmScalars) * V, nullptr, from_malloc()));
    FVB_HIP_CHECK(hipMemset(b_scalars.p, 0, sizeof(NllsHmScalars) * V)); // phase 0 = new
    HostModelLoop loop;
    if ((rc = loop.open(cfg)) != 0)
        return rc;
    ha.persist = (double *)b_persist.p;
    ha.scalars = (NllsHmScalars *)b_scalars.p;
    ha.means_out = (double *)loop.b_means.p;
    ha.phase_out = (int32_t *)loop.b_phase.p;
    if (L.bytes > 64 * 1024)
        FVB_HIP_CHECK(hipFuncSetAttribute((const void *)nlls_wave_step_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.bytes));

    std::vector<double> means((size_t)P * V);
    for (size_t v = 0; v < V; v++)
        for (int i = 0; i < P; i++)
            means[v * P + i] = cfg->post_mean[i]; // the starting estimate, Fabber space (inference_nlls.cc:131)
    // one launch per trial point: the first linearisation, then at most max_iterations trials
    const long max_steps = (long)nl->max_iterations + 2;
    rc = loop.run(linearise, user, means, 3, max_steps, "host-model NLLS loop did not terminate",
        [&](const double *lin, const int32_t *batch_ids, size_t nb, hipStream_t stream) {
            ha.lin = lin;
            ha.batch_ids = batch_ids;
            hipLaunchKernelGGL(nlls_wave_step_kernel, dim3((unsigned)nb), dim3(64), L.bytes, stream, ha);
        });
    if (rc)
        return rc;
    return staged.stage_out(out, nullptr);
}

} // extern "C"
