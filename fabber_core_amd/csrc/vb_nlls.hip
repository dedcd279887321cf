/*
 * vb_nlls.hip - instantiations and C ABI of the non-linear least squares kernel
 * (vb_nlls_kernel.h; method=nlls, inference_nlls.cc).
 */
#include "vb_nlls_kernel.h"

#include "vb_host_stage.h"

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
} // namespace fvb

namespace
{
int validate_nlls(const fvb_config *cfg, const fvb_nlls *nl)
{
    if (!cfg || !nl)
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
    if (nl->max_iterations < 0 || !(nl->lambda0 > 0) || !(nl->lambda_max > 0))
        return api_fail(-60, "bad minimiser settings");
    if (cfg->model != FVB_MODEL_POLY && cfg->model != FVB_MODEL_LINEAR && cfg->model != FVB_MODEL_EXP)
        return api_fail(-61, "method=nlls needs a forward model with a device body");
    if (!get_nlls_kernel(cfg->model, cfg->n_params).fn && wave_layout(cfg->n_times, cfg->n_params, 1).bytes > 160 * 1024)
        return api_fail(-61, "no NLLS kernel for this problem: no lane instantiation for the model / parameter count and the "
                             "series does not fit the 160 KB of LDS the wave-per-voxel kernel needs");
    return 0;
}
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

int32_t fabber_nlls_run_device(const fvb_config *cfg, const fvb_nlls *nl, const void *data, const fvb_outputs *out,
    void *stream, int32_t n_unmasked)
{
    int rc = validate_nlls(cfg, nl);
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
    const NllsKernelInfo k = get_nlls_kernel(cfg->model, cfg->n_params);
    const WaveLayout L = wave_layout(cfg->n_times, cfg->n_params, 1);
    // lane per voxel where an instantiation exists and there are enough voxels to fill the chip
    // (as the VB kernels, vb_api.cc); wave per voxel otherwise
    const bool wave_fits = L.bytes <= 160 * 1024;
    const int variant = api_variant();
    if (k.fn && variant != 2 && (variant == 1 || cfg->n_voxels >= 4096 || !wave_fits))
    {
        const unsigned grid = (unsigned)((cfg->n_voxels + 63) / 64);
        hipLaunchKernelGGL(k.fn, dim3(grid), dim3(64), 0, (hipStream_t)stream, na);
    }
    else
    {
        if (L.bytes > 64 * 1024)
            FVB_HIP_CHECK(hipFuncSetAttribute((const void *)nlls_wave_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.bytes));
        hipLaunchKernelGGL(nlls_wave_kernel, dim3((unsigned)cfg->n_voxels), dim3(64), L.bytes, (hipStream_t)stream, na, L);
    }
    FVB_HIP_CHECK(hipGetLastError());
    return 0;
}

int32_t fabber_nlls_run_host(const fvb_config *cfg, const fvb_nlls *nl, const void *data, const fvb_outputs *out,
    int32_t device)
{
    int rc = validate_nlls(cfg, nl);
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
