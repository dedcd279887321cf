/*
 * vb_spatial_wave_model.h - the wave-per-voxel spatial family (vb_spatial_wave.h) around the device body of a model
 * library: the set-up kernel and the second sweep with the body linearised in the kernel instead of the host's rows.
 *
 * Only the source of a chunk differs from the host-model kernels (SpwBodyRows for SpwHostRows): where those copy
 * SPW_TC timepoints of the host's g and J into LDS, these evaluate the body 2 P + 1 times per timepoint, one timepoint of
 * the chunk per lane, by the central differences of LinearizedFwdModel::ReCentre as wave_recentre<Eval> codes them
 * (vb_wave_kernel.h: the delta rule, to_model per parameter, rden = 1 / (c2 - c3), FVB_MODEL_FP, the finiteness tests).
 * The sums over t, the residual, the noise update, the free energy, the state image and every store are the functions of
 * vb_spatial_wave.h themselves, so the two routes differ by the rounding of g and J alone.
 *
 * There is no stored linearisation: the second sweep's residual about the centre the moments belong to (L.ml as
 * loaded) evaluates the body again - 2 P + 1 more evaluations per timepoint and iteration instead of a [V][T][P + 1]
 * buffer (55 GB at 128^3 voxels, T = 100, P = 32).
 *
 * LDS: sp_wave_layout(P) and behind it the (2 P + 1) P doubles of the centre and perturbed parameter vectors and P
 * doubles of rden (sp_wave_model_layout): 57.8 KB at P = 32. All lanes of the wavefront read the SAME vector entry in an
 * evaluation (they differ in t): a broadcast, no bank conflict whatever the vectors' stride; J keeps its odd row stride
 * Ps, and every offset of sp_wave_layout is unchanged, so the engine's own first sweep works on the same state in LDS.
 *
 * Under a noise pattern (N = 2 ... FVB_MAX_PHIS precisions; include/fabber_device_spatial_wave_noise_model.h) the same two
 * kernels in their CLASSES form: the layout is sp_wave_layout(P, N) with the same vectors behind it, 89.8 KB at P = 32,
 * N = 8 of the 160 KB a workgroup may have (one workgroup per compute unit then).
 */
#pragma once

#include "vb_spatial_wave.h"

namespace fvb
{
// sp_wave_layout(P) with the parameter vectors of the 2 P + 1 evaluations behind it. The two fields are ones the family
// does not use otherwise: W = the vectors [2 P + 1][P] (wave_layout's pv; this layout's pv are 3 P per-parameter terms),
// rden [P]. The engine works the launch's LDS bytes out with this function and the library's kernels place their arrays
// with it: include/fabber_device_spatial_wave_model.h registers the double count at FVB_MAX_PARAMS as a probe.
FVB_HD WaveLayout sp_wave_model_layout(int P, int N = 1)
{
    WaveLayout L = sp_wave_layout(P, N);
    int o = L.n_doubles;
    L.W = o;
    o += (2 * P + 1) * P;
    L.rden = o;
    o += P;
    L.n_doubles = o;
    L.bytes = sizeof(double) * (size_t)o;
    return L;
}

#if defined(__HIPCC__)

// The linearisation of a library's body about L.ml, chunk by chunk (see SpwHostRows)
template <class Eval>
struct SpwBodyRows
{
    ModelArgs ma; // the constants, and this voxel's supplementary rows
    __device__ __forceinline__ SpwBodyRows(const SpatialArgs &sa, int v, bool) : ma(wave_model_args<Eval>(sa.ka, v))
    {
    }
    static __device__ __forceinline__ WaveLayout layout(int P, int N = 1)
    {
        return sp_wave_model_layout(P, N);
    }
    // the 2 P + 1 model-space parameter vectors and rden (fwdmodel_linear.cc:157-161, fwdmodel.cc:375-379), as wave_recentre
    __device__ __forceinline__ void centre(const KernelArgs &ka, WaveCtx &cx) const
    {
        const WaveLayout &L = cx.L;
        const int P = L.P;
        double *sh = cx.sh;
        FVB_WAVE_FOR(i, P)
        {
            const int tr = FVB_KPARAM(ka, transform, i);
            const double centre = sh[L.ml + i];
            double delta = centre * 1e-5;
            if (delta < 0)
                delta = -delta;
            if (delta < 1e-10)
                delta = 1e-10;
            const double c2 = centre + delta;
            const double c3 = centre - delta;
            const double tp = to_model(tr, centre);
            const double tp2 = to_model(tr, c2);
            const double tp3 = to_model(tr, c3);
            sh[L.rden + i] = 1.0 / (c2 - c3);
            sh[L.W + i] = tp;
            for (int j = 0; j < P; j++)
            {
                sh[L.W + (1 + 2 * j) * P + i] = (i == j) ? tp2 : tp;
                sh[L.W + (2 + 2 * j) * P + i] = (i == j) ? tp3 : tp;
            }
        }
        wave_sync();
    }
    // spw_stage_chunk's contract: J rows and r = y - g of the chunk in LDS, zeros for a masked timepoint, every g and J
    // tested for finiteness (masked timepoints included). Lane t evaluates timepoint t0 + t.
    __device__ __forceinline__ void chunk(const KernelArgs &ka, WaveCtx &cx, const uint8_t *phi_index, int t0, int n, bool &bad_offset,
        bool &bad_jac) const
    {
        const WaveLayout &L = cx.L;
        const int P = L.P, Ps = L.Ps;
        double *sh = cx.sh;
        FVB_WAVE_FOR(t, n)
        {
            const bool unmasked = phi_index ? (phi_index[t0 + t] != 255) : true;
            const double g = Eval::eval(ma, P, t0 + t, sh + L.W);
            bad_offset |= !is_finite(g);
            for (int i = 0; i < P; i++)
            {
                FVB_MODEL_FP
                const double f2 = Eval::eval(ma, P, t0 + t, sh + L.W + (1 + 2 * i) * P);
                const double f3 = Eval::eval(ma, P, t0 + t, sh + L.W + (2 + 2 * i) * P);
                const double Jti = (f2 - f3) * sh[L.rden + i];
                bad_jac |= !is_finite(Jti);
                sh[L.J + t * Ps + i] = unmasked ? Jti : 0.0;
            }
            sh[L.r + t] = unmasked ? load_data(ka, (size_t)(t0 + t) * cx.V + cx.v) - g : 0.0;
        }
        wave_sync();
    }
};

template <class Eval>
__global__ __launch_bounds__(64) void vb_spatial_wave_setup_kernel(const SpatialArgs sa)
{
    spw_setup<SpwBodyRows<Eval> >(sa);
}

template <class Eval, bool NEEDF>
__global__ __launch_bounds__(64) void vb_spatial_wave_noise_kernel(const SpatialArgs sa)
{
    spw_noise<SpwBodyRows<Eval>, NEEDF>(sa);
}

// ... and for N = cfg.n_phis > 1 noise precisions
template <class Eval>
__global__ __launch_bounds__(64) void vb_spatial_wave_classes_setup_kernel(const SpatialArgs sa)
{
    spw_setup<SpwBodyRows<Eval>, true>(sa);
}

template <class Eval, bool NEEDF>
__global__ __launch_bounds__(64) void vb_spatial_wave_classes_noise_kernel(const SpatialArgs sa)
{
    spw_noise<SpwBodyRows<Eval>, NEEDF, true>(sa);
}

#endif // __HIPCC__
} // namespace fvb
