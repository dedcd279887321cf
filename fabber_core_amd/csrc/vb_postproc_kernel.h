/*
 * vb_postproc_kernel.h - the result-image kernel: InferenceTechnique::SaveResults (inference.cc:112-281) and the noise
 * images of Vb::SaveResults (inference_vb.cc:981-989) from the packed MVN image, one lane per voxel.
 *
 * The kernel is a template on the evaluator of the model fit - the concept of vb_wave_kernel.h:
 *     static __device__ double eval(const ModelArgs &a, int P, int t, const double *model_space_params)
 * The engine instantiates it for BuiltinEval (vb_api.hip); a model library compiles it around its device body in its own
 * code object (include/fabber_device_results_model.h). Templates and inline functions only.
 *
 * 256 lanes per workgroup, lane = voxel: every load of the MVN image and of the series and every store of an image is
 * coalesced over voxels. The model-space means are a per-lane array indexed by the run-time parameter count, which the
 * compiler keeps in scratch (MAXP doubles per lane); the kernel moves (P + T) doubles per voxel and evaluates the model T
 * times, which hides it.
 */
#pragma once

#include "vb_wave_kernel.h"

namespace fvb
{
// MAXP: FVB_MAX_PARAMS, or FVB_MAX_PARAMS_EXT for a configuration with a parameter table (cfg.params_ext, device memory)
template <class Eval, int MAXP>
__global__ __launch_bounds__(256) void vb_postproc_kernel(
    const fvb_config cfg, const void *data, const double *mvn, const fvb_postproc pp, const int n_noise)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= cfg.n_voxels)
        return;
    const size_t V = (size_t)cfg.n_voxels;
    const int P = cfg.n_params, n = P + n_noise, T = cfg.n_times;
    const int nCov = n * (n + 1) / 2;
    double means[MAXP];
    for (int p = 0; p < P; p++)
    {
        const double m = mvn[(size_t)(nCov + p) * V + v];
        const double var = mvn[(size_t)(p * (p + 1) / 2 + p) * V + v];
        const int tr = cfg.params_ext ? cfg.params_ext->transform[p] : cfg.transform[p];
        // FwdModel::ToModel, fwdmodel.cc:326-337
        const double mm = to_model(tr, m);
        const double mv = to_model_var(tr, var);
        const double sd = sqrt(mv);
        means[p] = mm; // model-space value, what EvaluateModel receives
        if (pp.mean)
            pp.mean[(size_t)p * V + v] = mm;
        if (pp.var)
            pp.var[(size_t)p * V + v] = mv;
        if (pp.std)
            pp.std[(size_t)p * V + v] = sd;
        if (pp.zstat)
            pp.zstat[(size_t)p * V + v] = mm / sd;
    }
    for (int i = 0; i < n_noise; i++) // inference_vb.cc:981-989
    {
        const int q = P + i;
        if (pp.noise_mean)
            pp.noise_mean[(size_t)i * V + v] = mvn[(size_t)(nCov + q) * V + v];
        if (pp.noise_std)
            pp.noise_std[(size_t)i * V + v] = sqrt(mvn[(size_t)(q * (q + 1) / 2 + q) * V + v]);
    }
    if (pp.modelfit || pp.residuals) // inference.cc:181-243
    {
        ModelArgs ma;
        ma.iopt0 = cfg.model_iopt[0];
        ma.dopt0 = cfg.model_dopt[0];
        ma.design = cfg.design;
        ma.consts = cfg.model_consts;
        ma.n_consts = cfg.n_model_consts;
        set_model_supp(ma, cfg, v);
        ma.model = cfg.model;
        for (int t = 0; t < T; t++)
        {
            // (a non-finite prediction is an image value like any other: a body answers a timepoint past its constants so)
            const double fit = Eval::eval(ma, P, t, means);
            if (pp.modelfit)
                pp.modelfit[(size_t)t * V + v] = fit;
            if (pp.residuals)
            {
                const size_t idx = (size_t)t * V + v;
                const double y = cfg.data_f64 ? ((const double *)data)[idx] : (double)((const float *)data)[idx];
                pp.residuals[idx] = y - fit;
            }
        }
    }
}

// The launch both code objects share: the engine's for BuiltinEval, a library's for its body. 0, or the HIP error.
template <class Eval>
inline hipError_t launch_postproc(const fvb_config &cfg, const void *data, const double *mvn, const fvb_postproc &pp, int n_noise,
    hipStream_t stream)
{
    const unsigned grid = (unsigned)((cfg.n_voxels + 255) / 256);
    if (cfg.n_params > FVB_MAX_PARAMS)
        hipLaunchKernelGGL((vb_postproc_kernel<Eval, FVB_MAX_PARAMS_EXT>), dim3(grid), dim3(256), 0, stream, cfg, data, mvn, pp, n_noise);
    else
        hipLaunchKernelGGL((vb_postproc_kernel<Eval, FVB_MAX_PARAMS>), dim3(grid), dim3(256), 0, stream, cfg, data, mvn, pp, n_noise);
    return hipGetLastError();
}
} // namespace fvb
