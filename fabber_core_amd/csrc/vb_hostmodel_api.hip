/*
 * vb_hostmodel_api.hip - driver of voxelwise VB with a host-evaluated forward model
 * (vb_hostmodel.h): alternates the caller's linearisation callback with one step launch until
 * every voxel is done.
 */
#include "vb_hostmodel_ar.h"

#include "vb_host_stage.h"

#include <string>
#include <vector>

using namespace fvb;

extern "C" int32_t fabber_vb_run_hostmodel_host(const fvb_config *cfg, const void *data, const fvb_outputs *out, int32_t device,
    fvb_linearise_fn linearise, void *user)
{
    int rc = api_validate(cfg, false);
    if (rc)
        return rc;
    if (!linearise)
        return api_fail(-50, "linearisation callback is NULL");
    const bool ar = cfg->noise == FVB_NOISE_AR1;
    if (!cfg->init_mvn)
        return api_fail(-52, "host-evaluated models need the initial posterior as init_mvn (the model's InitVoxelPosterior runs on the host)");
    if (!out || !out->mvn)
        return api_fail(-20, "outputs.mvn is required");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return api_fail(-30, "no HIP device available (the VB engine has no CPU fallback)");
    FVB_HIP_CHECK(hipSetDevice(device));
    const size_t V = (size_t)cfg->n_voxels, T = (size_t)cfg->n_times;
    if (V == 0)
        return 0;
    if (!data)
        return api_fail(-21, "data is NULL");
    const int P = cfg->n_params, N = cfg->n_phis;
    const int n = P + (ar ? 2 + cfg->ar_cross_terms + N : N), rows = n * (n + 1) / 2 + n + 1;
    const WaveLayout L = wave_layout((int)T, P, N, ar);
    if (L.bytes > 160 * 1024)
        return api_fail(-41, "host-model step kernel: " + std::to_string(L.bytes) + " bytes of LDS needed exceed the 160 KB of a gfx950 CU");
    fvb_config host_model = *cfg;
    host_model.design = nullptr;
    StagedProblem staged;
    if ((rc = staged.stage_in(&host_model, data, out, (size_t)rows, 0, V, nullptr, from_malloc(), STAGE_VB)) != 0)
        return rc;

    HmArgs ha;
    memset(&ha, 0, sizeof(ha));
    ha.ka.cfg = staged.d;
    ha.ka.out = staged.dout;
    ha.ka.data = staged.b_data.p;
    ha.ka.save = nullptr;
    const int n_unmasked = count_unmasked(T, cfg->phi_index);
    ha.ka.n_unmasked = n_unmasked;
    if (ar && n_unmasked != (int)T)
        return api_fail(-15, "Masked time points are not supported for the AR noise model"); // noisemodel_ar.cc:351-355
    ha.ka.residual_mode = 1;
    ha.ka.residual_tol = 0;
    ha.L = L;
    ha.persist_doubles = L.part - L.b;
    DevMem b_persist, b_scalars;
    FVB_HIP_CHECK(b_persist.alloc(sizeof(double) * (size_t)ha.persist_doubles * V, nullptr, from_malloc()));
    // the step kernel: white noise, or AR(1) with the alpha posterior kept per (echoes, alphas)
    typedef void (*StepFn)(const HmArgs);
    StepFn fn = cfg->need_f ? vb_wave_step_kernel<true> : vb_wave_step_kernel<false>;
    size_t scalars_bytes = sizeof(HmScalars);
    if (ar)
    {
        switch (N * 10 + 2 + cfg->ar_cross_terms)
        {
#define FVB_AR_STEP(KEY, NPHI, NA)                                                                           \
    case KEY:                                                                                                \
        fn = cfg->need_f ? vb_wave_ar_step_kernel<NPHI, NA, true> : vb_wave_ar_step_kernel<NPHI, NA, false>;  \
        scalars_bytes = sizeof(HmArScalars<NPHI, NA>);                                                       \
        break;
            FVB_AR_STEP(12, 1, 2)
            FVB_AR_STEP(22, 2, 2)
            FVB_AR_STEP(23, 2, 3)
            FVB_AR_STEP(24, 2, 4)
#undef FVB_AR_STEP
        default:
            return api_fail(-40, "AR(1) noise: num-echoes must be 1 or 2, cross terms need two echoes");
        }
    }
    FVB_HIP_CHECK(b_scalars.alloc(scalars_bytes * V, nullptr, from_malloc()));
    FVB_HIP_CHECK(hipMemset(b_scalars.p, 0, scalars_bytes * V)); // phase = HM_NEW
    HostModelLoop loop;
    if ((rc = loop.open(cfg)) != 0)
        return rc;
    ha.persist = (double *)b_persist.p;
    ha.scalars = (HmScalars *)b_scalars.p;
    ha.ar_scalars = b_scalars.p;
    ha.means_out = (double *)loop.b_means.p;
    ha.phase_out = (int32_t *)loop.b_phase.p;

    if (L.bytes > 64 * 1024)
        FVB_HIP_CHECK(hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.bytes));

    std::vector<double> means((size_t)P * V); // the starting estimate: the means of the initial posterior
    {
        const int nCov = n * (n + 1) / 2;
        for (size_t v = 0; v < V; v++)
            for (int i = 0; i < P; i++)
                means[v * P + i] = cfg->init_mvn[(size_t)(nCov + i) * V + v];
    }
    // every iteration needs one step, a revert one more, trial / LM modes extra iterations
    const long max_steps = ((long)cfg->max_iterations + 2) * 12 + 8;
    rc = loop.run(linearise, user, means, HM_DONE, max_steps, "host-model loop did not terminate",
        [&](const double *lin, const int32_t *batch_ids, size_t nb, hipStream_t stream) {
            ha.lin = lin;
            ha.batch_ids = batch_ids;
            hipLaunchKernelGGL(fn, dim3((unsigned)nb), dim3(64), L.bytes, stream, ha);
        });
    if (rc)
        return rc;
    return staged.stage_out(out, nullptr);
}
