/*
 * vb_init_kernel.h - the initial-posterior kernel: Vb::BuildInitialMvn (inference_vb.cc) for a model whose
 * InitVoxelPosterior exists as device code, one lane per voxel. It writes the packed MVN image [rows][voxel] the fit
 * kernels read as fvb_config.init_mvn: FwdModel::GetInitialPosterior (fwdmodel.cc:284-313) for the parameters, the noise
 * model's initial posterior as its mean and variance, 1 in the last row, 0 everywhere else.
 *
 * The kernel is a template on the body - the struct of include/fabber_device_model.h with one more member,
 *     static __device__ void init_posterior(const ModelArgs &a, int P, const VoxelSeries &y, double *means, double *vars)
 * (include/fabber_device_init_model.h has the contract). Only a model library instantiates it, in its own code object:
 * the engine's built-in models initialise themselves inside their fit kernels. Templates and inline functions only.
 *
 * 256 lanes per workgroup, lane = voxel: every load of the series and of an image prior and every store of a row is
 * coalesced over voxels. No LDS, no atomics, no cross-lane traffic. The model-space means and variances are two per-lane
 * arrays indexed by the run-time parameter count, which the compiler keeps in scratch (2 MAXP doubles per lane), as the
 * result-image kernel keeps its means. The kernel reads what the body reads of the series - at most T samples per
 * voxel - and writes rows = n (n + 1) / 2 + n + 1 doubles per voxel, n = parameters + noise entries: it is bound by
 * those stores.
 */
#pragma once

#include "vb_wave_kernel.h"

namespace fvb
{
// One voxel's series, read in place from the caller's [T][V] image (float or double): all T samples, the masked
// timepoints included - the reference hands the model the whole series (FwdModel::PassData).
struct VoxelSeries
{
    const void *column; // sample 0 of this voxel; sample t is t * V elements further on
    size_t V;           // the row stride, in elements
    int T;
    int f64; // the element type: wave-uniform
    __device__ __forceinline__ double operator()(int t) const
    {
        const size_t at = (size_t)t * V;
        return f64 ? ((const double *)column)[at] : (double)((const float *)column)[at];
    }
};

// what the kernel is launched with (cfg by value, as the fit kernels' KernelArgs carries it: FVB_KPARAM reads it)
struct InitArgs
{
    fvb_config cfg;
    const void *data; // [T][V], cfg.data_f64 says which type
    double *init_mvn; // [rows][V], every element is written
};

// MAXP: FVB_MAX_PARAMS, or FVB_MAX_PARAMS_EXT for a configuration with a parameter table (cfg.params_ext, device memory).
// The parameter count itself is a run-time value.
template <class Body, int MAXP>
__global__ __launch_bounds__(256) void vb_init_posterior_kernel(const InitArgs ia)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= ia.cfg.n_voxels)
        return;
    const size_t V = (size_t)ia.cfg.n_voxels;
    // noise entries of the MVN: white = the precisions; AR(1) = the alphas, then the precisions (noisemodel_ar.cc:287-300)
    const int NA = (ia.cfg.noise == FVB_NOISE_AR1) ? 2 + ia.cfg.ar_cross_terms : 0;
    const int P = ia.cfg.n_params, N = ia.cfg.n_phis, n = P + NA + N;
    const int nCov = n * (n + 1) / 2;
    double *out = ia.init_mvn + v;

    // FwdModel::GetInitialPosterior, fwdmodel.cc:284-306: what the hook finds, in MODEL space
    double means[MAXP], vars[MAXP];
    for (int i = 0; i < P; i++)
    {
        means[i] = (FVB_KPARAM(ia, prior_type, i) == FVB_PRIOR_IMAGE) ? FVB_KPARAM(ia, image_prior, i)[v] : FVB_KPARAM(ia, post_mean, i);
        vars[i] = FVB_KPARAM(ia, post_var, i);
    }
    ModelArgs ma;
    ma.iopt0 = ia.cfg.model_iopt[0];
    ma.dopt0 = ia.cfg.model_dopt[0];
    ma.design = ia.cfg.design;
    ma.lin = nullptr;
    ma.lin_T = 0;
    ma.exp_table = nullptr;
    ma.consts = ia.cfg.model_consts;
    ma.n_consts = ia.cfg.n_model_consts;
    set_model_supp(ma, ia.cfg, v);
    ma.model = ia.cfg.model;
    VoxelSeries y;
    y.column = (const char *)ia.data + (size_t)v * (ia.cfg.data_f64 ? sizeof(double) : sizeof(float));
    y.V = V;
    y.T = ia.cfg.n_times;
    y.f64 = ia.cfg.data_f64;
    Body::init_posterior(ma, P, y, means, vars); // FwdModel::InitVoxelPosterior

    // The column, row by row (row of (q, j), j <= q: q (q + 1) / 2 + j), as BuildInitialMvn fills it
    for (int q = 0; q < n; q++)
    {
        const int a = q - P, k = q - P - NA;
        const bool alpha_given = a >= 0 && a < NA && (ia.cfg.ar_alpha_given & 2);
        double diag, mean;
        if (q < P) // FwdModel::ToFabber, fwdmodel.cc:315-324
        {
            const int tr = FVB_KPARAM(ia, transform, q);
            mean = to_fabber(tr, means[q]);
            diag = to_fabber_var(tr, vars[q]);
        }
        else if (a < NA) // Ar1cNoiseModel's initial alpha posterior N(0, 1e4 I) (noisemodel_ar.cc:379-403), or the given one
        {
            mean = alpha_given ? ia.cfg.ar_alpha_post_mean[a] : 0.0;
            diag = alpha_given ? ia.cfg.ar_alpha_post_cov[a][a] : 1e4;
        }
        else // GammaDist mean and variance, as OutputAsMVN
        {
            const double b = ia.cfg.noise_post_b[k], c = ia.cfg.noise_post_c[k];
            mean = b * c;
            diag = b * b * c;
        }
        const size_t row0 = (size_t)(q * (q + 1) / 2);
        for (int j = 0; j < q; j++)
            out[(row0 + j) * V] = (alpha_given && j >= P) ? ia.cfg.ar_alpha_post_cov[a][j - P] : 0.0;
        out[(row0 + q) * V] = diag;
        out[(size_t)(nCov + q) * V] = mean;
    }
    out[(size_t)(nCov + n) * V] = 1.0;
}

// The launch, from the library's code object. 0, or the HIP error.
template <class Body>
inline hipError_t launch_init_posterior(const fvb_config &cfg, const void *data, double *init_mvn, hipStream_t stream)
{
    InitArgs ia;
    ia.cfg = cfg;
    ia.data = data;
    ia.init_mvn = init_mvn;
    const unsigned grid = (unsigned)((cfg.n_voxels + 255) / 256);
    if (cfg.n_params > FVB_MAX_PARAMS)
        hipLaunchKernelGGL((vb_init_posterior_kernel<Body, FVB_MAX_PARAMS_EXT>), dim3(grid), dim3(256), 0, stream, ia);
    else
        hipLaunchKernelGGL((vb_init_posterior_kernel<Body, FVB_MAX_PARAMS>), dim3(grid), dim3(256), 0, stream, ia);
    return hipGetLastError();
}
} // namespace fvb
