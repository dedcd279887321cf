/*
 * vb_spatial_wave.h - spatial VB (vb_spatial.h) for host-evaluated models with up to FVB_MAX_PARAMS parameters, one
 * WAVEFRONT per voxel.
 *
 * The lane form keeps a voxel's whole state in one lane's registers: at P = 32 that would be Sigma and J'J at 528
 * doubles each. Here a 64-lane workgroup takes one voxel and keeps its P x P work in LDS, with the device functions
 * of the voxelwise wave kernel (vb_wave_kernel.h: wave_sweep_inverse for Lambda^-1 and log|det Lambda|,
 * wave_update_theta, wave_update_noise, wave_free_energy):
 *
 *   vb_spatial_wave_setup_kernel   vb_spatial_setup_kernel    initial posterior, moments about the centre (lin_cur)
 *   vb_spatial_wide_ak_*_kernel    vb_spatial_ak_*_kernel     the same segments, added in the same order (lane form)
 *   vb_spatial_wave_theta_kernel   vb_spatial_theta_kernel    one level per launch: priors, F "before", UpdateTheta, F "theta"
 *   vb_spatial_wave_noise_kernel   vb_spatial_noise_kernel    residual and trace about lin_cur (summed directly over t),
 *                                                             UpdateNoise, the re-centre's moments (lin_next), F, status
 *   vb_spatial_wide_pack_kernel    vb_spatial_pack_kernel     result image (lane form: its stores are coalesced)
 *
 * The state image has SpLayout's row order with a runtime P (SpWideLayout), so its moments form is the lane form's:
 * the first sweep reads J'J, J'r and r'r only. J'J and J'r come from the host's linearisation rows [T][P]: chunks of
 * SPW_TC timepoints of J are staged in LDS and every lane adds its share of the P (P + 1) / 2 + P + 1 sums over t in
 * order, so T has no limit here. fp64 throughout; sums run in orders of their own (the lane form's rounding is not
 * reproduced bit for bit - the oracle is the yardstick).
 *
 * The set-up kernel and the second sweep are templates on where a chunk of the linearisation comes from (SpwHostRows
 * below: the host's rows): vb_spatial_wave_model.h builds them around the device body of a model library, which they
 * linearise in the kernel.
 */
#pragma once

#include "vb_spatial.h"
#include "vb_wave_kernel.h"

namespace fvb
{
// Row offsets of the state image for a runtime P, in SpLayout<P>'s order
struct SpWideLayout
{
    int P, PT, M, SIG, LOGDET, PM, PPREC, B, C, A, U, S, ML, ROWS;
};

FVB_HD SpWideLayout sp_wide_layout(int P)
{
    SpWideLayout L;
    L.P = P;
    L.PT = P * (P + 1) / 2;
    L.M = 0;
    L.SIG = L.M + P;
    L.LOGDET = L.SIG + L.PT;
    L.PM = L.LOGDET + 1;
    L.PPREC = L.PM + P;
    L.B = L.PPREC + P;
    L.C = L.B + 1;
    L.A = L.C + 1;
    L.U = L.A + L.PT;
    L.S = L.U + P;
    L.ML = L.S + 1;
    L.ROWS = L.ML + P;
    return L;
}

// Under a noise pattern (N = 2 ... FVB_MAX_PHIS precisions) the statistics of every class follow the rows above, in the
// order of SpPattern<P, N> (vb_spatial_noise.h): b_k, c_k, A_k, u_k, s_k. The rows B, C, A, U, S above are not used then;
// the a_K kernels read M and SIG only and work on either image.
struct SpWideClassRows
{
    int NB, NC, AK, UK, SK, ROWS;
};

FVB_HD SpWideClassRows sp_wide_class_rows(int P, int N)
{
    const SpWideLayout S = sp_wide_layout(P);
    SpWideClassRows R;
    R.NB = S.ROWS;
    R.NC = R.NB + N;
    R.AK = R.NC + N;
    R.UK = R.AK + N * S.PT;
    R.SK = R.UK + N * P;
    R.ROWS = R.SK + N;
    return R;
}

// rows of the state image: 5 724 at P = 32, N = 8 (46 KB per voxel)
FVB_HD int sp_wide_state_rows(int P, int N)
{
    return N > 1 ? sp_wide_class_rows(P, N).ROWS : sp_wide_layout(P).ROWS;
}

// Under AR(1) noise with one echo and no cross terms (vb_spatial_wave_ar.h) the rows of SpAr1<P> (vb_spatial_noise.h)
// follow the rows above, in that policy's order: the alpha posterior (means, c11, c12, c22, a1, a2), the diagonal and
// lag-1 moments Ad, C, ud, uc, sd, sc and the first and last rows J1, JT, r1, rT. The rows A, U, S above hold the EFFECTIVE
// moments J'QJ, J'Q(y - g), (y - g)'Q(y - g) then and B, C phi's posterior: the first sweep without F and the a_K
// kernels work on this image as on the one-precision image.
struct SpWideArRows
{
    int AL, AD, CC, UD, UC, SD, SC, J1, JT, R1, RT, ROWS;
};

FVB_HD SpWideArRows sp_wide_ar_rows(int P)
{
    const SpWideLayout S = sp_wide_layout(P);
    SpWideArRows R;
    R.AL = S.ROWS;
    R.AD = R.AL + 7;
    R.CC = R.AD + S.PT;
    R.UD = R.CC + S.PT;
    R.UC = R.UD + P;
    R.SD = R.UC + P;
    R.SC = R.SD + 1;
    R.J1 = R.SC + 1;
    R.JT = R.J1 + P;
    R.R1 = R.JT + P;
    R.RT = R.R1 + 1;
    R.ROWS = R.RT + 1;
    return R;
}

// rows of the state image under AR(1) noise: 2 415 at P = 32 (19 KB per voxel)
FVB_HD int sp_wide_ar_state_rows(int P)
{
    return sp_wide_ar_rows(P).ROWS;
}

// timepoints of J staged in LDS at a time (one per lane where a pass works on timepoints)
constexpr int SPW_TC = 64;
// N > 1: the chunk's unmasked timepoints listed class by class (spw_class_lists), SPW_TC + 16 int32
constexpr int SPW_CLASS_LIST_DOUBLES = (SPW_TC + 16) / 2;

// LDS of one voxel, in doubles: the WaveLayout fields the shared wave functions read, a chunk of J [SPW_TC][Ps] and its
// residuals, a row of per-timepoint terms and 3 P doubles of per-parameter terms (pv). The other fields of WaveLayout
// are not used here. At P = 32: 40.9 KB. With N > 1 noise precisions A, u, s, kq, trs, cnt, b, c are N-fold, where the
// shared wave functions index them (L.A + phi * PT, L.u + phi * P, L.s + phi ...), and the class lists of a chunk follow
// Sig (field z); with N = 1 every offset and the size are those of the one-precision layout. At P = 32, N = 8: 72.9 KB.
FVB_HD WaveLayout sp_wave_layout(int P, int N = 1)
{
    WaveLayout L = {};
    L.T = SPW_TC;
    L.P = P;
    L.N = N;
    L.Ps = P | 1; // odd row stride: lanes reading one column of consecutive rows hit distinct banks
    L.PT = P * (P + 1) / 2;
    L.PP = P * P;
    int o = 0;
#define FVB_WL(field, n)                                                                                     \
    L.field = o;                                                                                             \
    o += (n);
    FVB_WL(J, SPW_TC * L.Ps)
    FVB_WL(r, SPW_TC)
    FVB_WL(part, 64)
    FVB_WL(pv, 3 * P)
    FVB_WL(A, N * L.PT)
    FVB_WL(u, N * P)
    FVB_WL(s, N)
    FVB_WL(kq, N)
    FVB_WL(trs, N)
    FVB_WL(cnt, N)
    FVB_WL(b, N)
    FVB_WL(c, N)
    FVB_WL(m, P)
    FVB_WL(ml, P)
    FVB_WL(pm, P)
    FVB_WL(pprec, P)
    FVB_WL(rhs, P)
    FVB_WL(Lam, L.PP)
    FVB_WL(Sig, L.PP)
    FVB_WL(z, N > 1 ? SPW_CLASS_LIST_DOUBLES : 0)
#undef FVB_WL
    L.n_doubles = o;
    L.bytes = sizeof(double) * (size_t)o;
    return L;
}

#if defined(__HIPCC__)

// the entries one lane accumulates in spw_moments: P (P + 1) / 2 + P + 1 <= 561 at P = 32, 64 lanes
constexpr int SPW_MAX_SLOTS = (FVB_MAX_PARAMS * (FVB_MAX_PARAMS + 1) / 2 + FVB_MAX_PARAMS + 1 + 63) / 64;

__device__ __forceinline__ void spw_init_ctx(WaveCtx &cx, int v, size_t V, const WaveLayout &L)
{
    extern __shared__ double spw_lds[];
    cx.L = L;
    cx.sh = spw_lds;
    cx.phi = nullptr;
    cx.lane = threadIdx.x;
    cx.v = v;
    cx.V = V;
    cx.lin = nullptr;
    cx.covValid = true;
    cx.precValid = false;
    cx.logdetLam = 0;
    cx.sv_prec = false;
}

// the voxel's state rows -> LDS (sp_load): Sigma unpacked to a full P x P matrix
__device__ __forceinline__ void spw_load(const SpatialArgs &sa, WaveCtx &cx)
{
    const WaveLayout &L = cx.L;
    const SpWideLayout S = sp_wide_layout(L.P);
    const int P = L.P;
    const size_t V = cx.V;
    const double *p = sa.state + cx.v;
    double *sh = cx.sh;
    const bool classes = L.N > 1; // (the statistics are the class rows' then)
    FVB_WAVE_FOR(i, P)
    {
        sh[L.m + i] = p[(size_t)(S.M + i) * V];
        sh[L.pm + i] = p[(size_t)(S.PM + i) * V];
        sh[L.pprec + i] = p[(size_t)(S.PPREC + i) * V];
        if (!classes)
            sh[L.u + i] = p[(size_t)(S.U + i) * V];
        sh[L.ml + i] = p[(size_t)(S.ML + i) * V];
    }
    FVB_WAVE_FOR(e, L.PP)
    sh[L.Sig + e] = p[(size_t)(S.SIG + tri(e / P, e % P)) * V];
    if (classes)
    {
        const SpWideClassRows R = sp_wide_class_rows(P, L.N);
        FVB_WAVE_FOR(e, L.N * L.PT)
        sh[L.A + e] = p[(size_t)(R.AK + e) * V];
        FVB_WAVE_FOR(e, L.N * P)
        sh[L.u + e] = p[(size_t)(R.UK + e) * V];
        FVB_WAVE_FOR(k, L.N)
        {
            sh[L.b + k] = p[(size_t)(R.NB + k) * V];
            sh[L.c + k] = p[(size_t)(R.NC + k) * V];
            sh[L.s + k] = p[(size_t)(R.SK + k) * V];
        }
    }
    else
    {
        FVB_WAVE_FOR(e, L.PT)
        sh[L.A + e] = p[(size_t)(S.A + e) * V];
        if (cx.lane == 0)
        {
            sh[L.b] = p[(size_t)S.B * V];
            sh[L.c] = p[(size_t)S.C * V];
            sh[L.s] = p[(size_t)S.S * V];
        }
    }
    cx.logdetLam = p[(size_t)S.LOGDET * V];
    cx.covValid = true;
    cx.precValid = false;
    wave_sync();
}

// sp_store_theta: means, prior, Sigma (packed again), log|det Lambda|
__device__ __forceinline__ void spw_store_theta(const SpatialArgs &sa, WaveCtx &cx)
{
    const WaveLayout &L = cx.L;
    const SpWideLayout S = sp_wide_layout(L.P);
    const int P = L.P;
    const size_t V = cx.V;
    double *p = sa.state + cx.v;
    const double *sh = cx.sh;
    FVB_WAVE_FOR(i, P)
    {
        p[(size_t)(S.M + i) * V] = sh[L.m + i];
        p[(size_t)(S.PM + i) * V] = sh[L.pm + i];
        p[(size_t)(S.PPREC + i) * V] = sh[L.pprec + i];
    }
    FVB_WAVE_FOR(e, L.PT)
    {
        int i = 0;
        while ((i + 1) * (i + 2) / 2 <= e)
            i++;
        const int j = e - i * (i + 1) / 2;
        p[(size_t)(S.SIG + e) * V] = sh[L.Sig + i * P + j];
    }
    if (cx.lane == 0)
        p[(size_t)S.LOGDET * V] = cx.logdetLam;
}

// sp_store_noise: noise posterior and the moments with their centre
__device__ __forceinline__ void spw_store_noise(const SpatialArgs &sa, WaveCtx &cx)
{
    const WaveLayout &L = cx.L;
    const SpWideLayout S = sp_wide_layout(L.P);
    const int P = L.P;
    const size_t V = cx.V;
    double *p = sa.state + cx.v;
    const double *sh = cx.sh;
    if (L.N > 1)
    {
        const SpWideClassRows R = sp_wide_class_rows(P, L.N);
        FVB_WAVE_FOR(i, P)
        p[(size_t)(S.ML + i) * V] = sh[L.ml + i];
        FVB_WAVE_FOR(e, L.N * L.PT)
        p[(size_t)(R.AK + e) * V] = sh[L.A + e];
        FVB_WAVE_FOR(e, L.N * P)
        p[(size_t)(R.UK + e) * V] = sh[L.u + e];
        FVB_WAVE_FOR(k, L.N)
        {
            p[(size_t)(R.NB + k) * V] = sh[L.b + k];
            p[(size_t)(R.NC + k) * V] = sh[L.c + k];
            p[(size_t)(R.SK + k) * V] = sh[L.s + k];
        }
        return;
    }
    FVB_WAVE_FOR(i, P)
    {
        p[(size_t)(S.U + i) * V] = sh[L.u + i];
        p[(size_t)(S.ML + i) * V] = sh[L.ml + i];
    }
    FVB_WAVE_FOR(e, L.PT)
    p[(size_t)(S.A + e) * V] = sh[L.A + e];
    if (cx.lane == 0)
    {
        p[(size_t)S.B * V] = sh[L.b];
        p[(size_t)S.C * V] = sh[L.c];
        p[(size_t)S.S * V] = sh[L.s];
    }
}

// One chunk [t0, t0 + n) of the host's linearisation (g [T], then J [T][P]) into LDS: J rows, and r = y - g in L.r.
// Masked timepoints stage zeros (they add +0 to every sum); every g and J is tested for finiteness
// (fwdmodel_linear.cc:134-140,174-181), masked timepoints included.
__device__ __forceinline__ void spw_stage_chunk(const KernelArgs &ka, WaveCtx &cx, const double *lin, const uint8_t *phi_index, int t0,
    int n, bool &bad_offset, bool &bad_jac)
{
    const WaveLayout &L = cx.L;
    const int T = ka.cfg.n_times, P = L.P, Ps = L.Ps;
    double *sh = cx.sh;
    const double *Jrows = lin + (size_t)T + (size_t)t0 * P; // the chunk's n P entries are contiguous
    FVB_WAVE_FOR(q, n * P)
    {
        const int t = q / P, i = q - t * P;
        const double Jti = Jrows[q];
        bad_jac |= !is_finite(Jti);
        const bool unmasked = phi_index ? (phi_index[t0 + t] != 255) : true;
        sh[L.J + t * Ps + i] = unmasked ? Jti : 0.0;
    }
    FVB_WAVE_FOR(t, n)
    {
        const double g = lin[t0 + t];
        bad_offset |= !is_finite(g);
        const bool unmasked = phi_index ? (phi_index[t0 + t] != 255) : true;
        sh[L.r + t] = unmasked ? load_data(ka, (size_t)(t0 + t) * cx.V + cx.v) - g : 0.0;
    }
    wave_sync();
}

// Where the set-up kernel and the second sweep take the model's linearisation from, chunk by chunk - what they are
// templates on (Rows):
//   Rows(sa, v, next)    voxel v's source; next = false: the linearisation the moments in the state belong to
//   layout(P, N)         the LDS layout of the kernels built around the source (sp_wave_layout, or an extension of it)
//   centre(ka, cx)       once before the chunks of a pass: the linearisation is about the centre in L.ml
//   chunk(ka, cx, phi_index, t0, n, bad_offset, bad_jac)    spw_stage_chunk's contract for the chunk [t0, t0 + n)
// SpwHostRows: the rows the host computed (HostLin of vb_spatial_api.hip). vb_spatial_wave_model.h has the source that
// evaluates a model library's device body.
struct SpwHostRows
{
    const double *lin;
    __device__ __forceinline__ SpwHostRows(const SpatialArgs &sa, int v, bool next)
        : lin((next ? sa.lin_next : sa.lin_cur) + (size_t)v * sa.ka.cfg.n_times * (sa.ka.cfg.n_params + 1))
    {
    }
    static __device__ __forceinline__ WaveLayout layout(int P, int N = 1)
    {
        return sp_wave_layout(P, N);
    }
    __device__ __forceinline__ void centre(const KernelArgs &, WaveCtx &) const
    {
    }
    __device__ __forceinline__ void chunk(const KernelArgs &ka, WaveCtx &cx, const uint8_t *phi_index, int t0, int n, bool &bad_offset,
        bool &bad_jac) const
    {
        spw_stage_chunk(ka, cx, lin, phi_index, t0, n, bad_offset, bad_jac);
    }
};

// The moments about the linearisation of `rows` (recentre with HostLinModel): A = J'J, u = J'r, s = r'r over the unmasked
// timepoints, each a sum over t in order. The centre (L.ml) is the caller's. Returns the re-centre's status.
template <class Rows>
__device__ __forceinline__ int spw_moments(const KernelArgs &ka, WaveCtx &cx, const Rows &rows)
{
    const WaveLayout &L = cx.L;
    const int T = ka.cfg.n_times, P = L.P, Ps = L.Ps, PT = L.PT;
    const int E = PT + P + 1;
    double *sh = cx.sh;
    const uint8_t *phi_index = (ka.n_unmasked == T) ? nullptr : ka.cfg.phi_index;
    // this lane's entries e = lane + 64 k: (a, b) of J'J (a >= b), (a, -1) of J'r, (-1, -1) r'r, a = -2: none
    int ea[SPW_MAX_SLOTS], eb[SPW_MAX_SLOTS];
    double acc[SPW_MAX_SLOTS];
#pragma unroll
    for (int k = 0; k < SPW_MAX_SLOTS; k++)
    {
        const int e = cx.lane + 64 * k;
        acc[k] = 0;
        if (e < PT)
        {
            int a = 0;
            while ((a + 1) * (a + 2) / 2 <= e)
                a++;
            ea[k] = a;
            eb[k] = e - a * (a + 1) / 2;
        }
        else if (e < PT + P)
        {
            ea[k] = e - PT;
            eb[k] = -1;
        }
        else
        {
            ea[k] = (e == E - 1) ? -1 : -2;
            eb[k] = -1;
        }
    }
    bool bad_offset = false, bad_jac = false;
    rows.centre(ka, cx);
    for (int t0 = 0; t0 < T; t0 += SPW_TC)
    {
        const int n = (T - t0 < SPW_TC) ? T - t0 : SPW_TC;
        rows.chunk(ka, cx, phi_index, t0, n, bad_offset, bad_jac);
#pragma unroll
        for (int k = 0; k < SPW_MAX_SLOTS; k++)
        {
            const int a = ea[k], b = eb[k];
            if (a >= 0 && b >= 0)
            {
                for (int t = 0; t < n; t++)
                    acc[k] += sh[L.J + t * Ps + a] * sh[L.J + t * Ps + b];
            }
            else if (a >= 0)
            {
                for (int t = 0; t < n; t++)
                    acc[k] += sh[L.J + t * Ps + a] * sh[L.r + t];
            }
            else if (a == -1)
            {
                for (int t = 0; t < n; t++)
                    acc[k] += sh[L.r + t] * sh[L.r + t];
            }
        }
        wave_sync(); // (the next chunk overwrites the staged one)
    }
#pragma unroll
    for (int k = 0; k < SPW_MAX_SLOTS; k++)
    {
        const int e = cx.lane + 64 * k;
        if (e < PT)
            sh[L.A + e] = acc[k];
        else if (e < PT + P)
            sh[L.u + e - PT] = acc[k];
        else if (e == E - 1)
            sh[L.s] = acc[k];
    }
    wave_sync();
    const bool any_offset = __any(bad_offset), any_jac = __any(bad_jac);
    return any_offset ? FVB_BAD_OFFSET : (any_jac ? FVB_BAD_JACOBIAN : FVB_OK);
}

// tr(Sigma J'J) (noisemodel_white.cc:252,417): a row sum per lane, the rows added in order by every lane. k: the noise
// class whose moments are meant (the only one, 0, under one precision)
__device__ __forceinline__ double spw_trace_SA(WaveCtx &cx, int k = 0)
{
    const WaveLayout &L = cx.L;
    const int P = L.P, Ak = L.A + k * L.PT;
    double *sh = cx.sh;
    FVB_WAVE_FOR(i, P)
    {
        double s = 0;
        for (int j = 0; j < P; j++)
            s += sh[L.Sig + i * P + j] * sh[Ak + tri(i, j)];
        sh[L.pv + i] = s;
    }
    wave_sync();
    double tr = 0;
    for (int i = 0; i < P; i++)
        tr += sh[L.pv + i];
    wave_sync();
    return tr;
}

// k'k from the moments, k'k = s - 2 d'u + d'A d with d = m - ml, and tr(Sigma A) (residual_terms): what F "theta" reads
// (k: the noise class, as spw_trace_SA)
__device__ __forceinline__ void spw_moment_residual(WaveCtx &cx, double &kk, double &trSA, int k = 0)
{
    const WaveLayout &L = cx.L;
    const int P = L.P, Ak = L.A + k * L.PT, uk = L.u + k * P;
    double *sh = cx.sh;
    FVB_WAVE_FOR(i, P)
    {
        const double di = sh[L.m + i] - sh[L.ml + i];
        double dA = 0, tr = 0;
        for (int j = 0; j < P; j++)
        {
            dA += sh[Ak + tri(i, j)] * (sh[L.m + j] - sh[L.ml + j]);
            tr += sh[L.Sig + i * P + j] * sh[Ak + tri(i, j)];
        }
        sh[L.pv + i] = di * sh[uk + i];
        sh[L.pv + P + i] = di * dA;
        sh[L.pv + 2 * P + i] = tr;
    }
    wave_sync();
    double du = 0, dAd = 0;
    trSA = 0;
    for (int i = 0; i < P; i++)
    {
        du += sh[L.pv + i];
        dAd += sh[L.pv + P + i];
        trSA += sh[L.pv + 2 * P + i];
    }
    kk = sh[L.s + k] - 2 * du + dAd;
    wave_sync();
}

// k'k with k = y - g(ml) + J (ml - m) summed directly over the unmasked timepoints in order (noisemodel_white.cc:235,252),
// g and J from the linearisation the moments in the state belong to
template <class Rows>
__device__ __forceinline__ double spw_direct_residual(const KernelArgs &ka, WaveCtx &cx, const Rows &rows)
{
    const WaveLayout &L = cx.L;
    const int T = ka.cfg.n_times, P = L.P, Ps = L.Ps;
    double *sh = cx.sh;
    const uint8_t *phi_index = (ka.n_unmasked == T) ? nullptr : ka.cfg.phi_index;
    FVB_WAVE_FOR(i, P)
    sh[L.pv + i] = sh[L.ml + i] - sh[L.m + i];
    bool bad_offset = false, bad_jac = false; // (the set-up or the previous re-centre has reported these already)
    double kk = 0;
    rows.centre(ka, cx);
    for (int t0 = 0; t0 < T; t0 += SPW_TC)
    {
        const int n = (T - t0 < SPW_TC) ? T - t0 : SPW_TC;
        rows.chunk(ka, cx, phi_index, t0, n, bad_offset, bad_jac);
        FVB_WAVE_FOR(t, n)
        {
            double Jd = 0;
            for (int i = 0; i < P; i++)
                Jd += sh[L.J + t * Ps + i] * sh[L.pv + i];
            const double k = sh[L.r + t] + Jd; // (a masked timepoint: r = 0 and J = 0)
            sh[L.part + t] = k * k;
        }
        wave_sync();
        for (int t = 0; t < n; t++)
            kk += sh[L.part + t];
        wave_sync();
    }
    return kk;
}

// ---- N > 1 noise precisions (noise-pattern, noisemodel_white.cc:166-273): the sums over t class by class -----------------
// The class of a timepoint is the same for every voxel, so the chunk's unmasked timepoints are listed class by class once
// per chunk (in LDS: ord [SPW_TC], the lists one after another in order of t; cst [N + 1], where each begins) and every
// sum over the timepoints of a class walks its list. The partial sums are carried in the LDS class areas between chunks:
// no accumulator is indexed by a class. Masked timepoints are in no list.
__device__ __forceinline__ void spw_class_lists(const KernelArgs &ka, WaveCtx &cx, int t0, int n)
{
    const WaveLayout &L = cx.L;
    int *ord = (int *)(cx.sh + L.z), *cst = ord + SPW_TC;
    const int lane = cx.lane;
    const int mine = (lane < n) ? (ka.cfg.phi_index ? (int)ka.cfg.phi_index[t0 + lane] : 0) : 255;
    int start = 0;
    for (int k = 0; k < L.N; k++)
    {
        const unsigned long long in_k = __ballot(mine == k);
        if (mine == k) // (start + rank < n <= SPW_TC)
            ord[start + __popcll(in_k & ((1ull << lane) - 1ull))] = lane;
        if (lane == 0)
            cst[k] = start;
        start += __popcll(in_k);
    }
    if (lane == 0)
        cst[L.N] = start;
    wave_sync();
}

// spw_moments per class: A_k = J'Q_k J, u_k = J'Q_k r, s_k = r'Q_k r, each a sum over the class's timepoints in order
template <class Rows>
__device__ __forceinline__ int spw_moments_classes(const KernelArgs &ka, WaveCtx &cx, const Rows &rows)
{
    const WaveLayout &L = cx.L;
    const int T = ka.cfg.n_times, P = L.P, Ps = L.Ps, PT = L.PT, N = L.N;
    const int E = PT + P + 1;
    double *sh = cx.sh;
    const int *ord = (const int *)(sh + L.z), *cst = ord + SPW_TC;
    const uint8_t *phi_index = (ka.n_unmasked == T) ? nullptr : ka.cfg.phi_index;
    FVB_WAVE_FOR(e, N * PT)
    sh[L.A + e] = 0;
    FVB_WAVE_FOR(e, N * P)
    sh[L.u + e] = 0;
    FVB_WAVE_FOR(k, N)
    sh[L.s + k] = 0;
    wave_sync();
    // this lane's entries e = lane + 64 k, as spw_moments has them: the product x[t] y[t] of two columns of the staged
    // chunk (a column of J with stride Ps, or r), and where the entry of class 0 lies with the step to the next class
    int xa[SPW_MAX_SLOTS], xb[SPW_MAX_SLOTS], dst[SPW_MAX_SLOTS];
#pragma unroll
    for (int k = 0; k < SPW_MAX_SLOTS; k++)
    {
        const int e = cx.lane + 64 * k;
        xa[k] = xb[k] = L.r;
        dst[k] = -1; // none
        if (e < PT)
        {
            int a = 0;
            while ((a + 1) * (a + 2) / 2 <= e)
                a++;
            xa[k] = L.J + a;
            xb[k] = L.J + e - a * (a + 1) / 2;
            dst[k] = L.A + e;
        }
        else if (e < PT + P)
        {
            xa[k] = L.J + e - PT;
            dst[k] = L.u + e - PT;
        }
        else if (e == E - 1)
            dst[k] = L.s;
    }
    bool bad_offset = false, bad_jac = false;
    rows.centre(ka, cx);
    for (int t0 = 0; t0 < T; t0 += SPW_TC)
    {
        const int n = (T - t0 < SPW_TC) ? T - t0 : SPW_TC;
        rows.chunk(ka, cx, phi_index, t0, n, bad_offset, bad_jac);
        spw_class_lists(ka, cx, t0, n);
#pragma unroll
        for (int k = 0; k < SPW_MAX_SLOTS; k++)
        {
            if (dst[k] < 0)
                continue;
            const int e = cx.lane + 64 * k;
            const int sa_ = (xa[k] == L.r) ? 1 : Ps, sb_ = (xb[k] == L.r) ? 1 : Ps;
            const int step = (e < PT) ? PT : ((e < PT + P) ? P : 1);
            for (int c = 0; c < N; c++)
            {
                const int q0 = cst[c], q1 = cst[c + 1];
                if (q0 == q1)
                    continue;
                double acc = sh[dst[k] + c * step];
                for (int q = q0; q < q1; q++)
                {
                    const int t = ord[q];
                    acc += sh[xa[k] + t * sa_] * sh[xb[k] + t * sb_];
                }
                sh[dst[k] + c * step] = acc;
            }
        }
        wave_sync(); // (the next chunk overwrites the staged one and its lists)
    }
    const bool any_offset = __any(bad_offset), any_jac = __any(bad_jac);
    return any_offset ? FVB_BAD_OFFSET : (any_jac ? FVB_BAD_JACOBIAN : FVB_OK);
}

// spw_direct_residual per class into L.kq: lane k carries the sum of class k from chunk to chunk
template <class Rows>
__device__ __forceinline__ void spw_direct_residual_classes(const KernelArgs &ka, WaveCtx &cx, const Rows &rows)
{
    const WaveLayout &L = cx.L;
    const int T = ka.cfg.n_times, P = L.P, Ps = L.Ps, N = L.N;
    double *sh = cx.sh;
    const int *ord = (const int *)(sh + L.z), *cst = ord + SPW_TC;
    const uint8_t *phi_index = (ka.n_unmasked == T) ? nullptr : ka.cfg.phi_index;
    FVB_WAVE_FOR(i, P)
    sh[L.pv + i] = sh[L.ml + i] - sh[L.m + i];
    bool bad_offset = false, bad_jac = false; // (the set-up or the previous re-centre has reported these already)
    double kk = 0;
    rows.centre(ka, cx);
    for (int t0 = 0; t0 < T; t0 += SPW_TC)
    {
        const int n = (T - t0 < SPW_TC) ? T - t0 : SPW_TC;
        rows.chunk(ka, cx, phi_index, t0, n, bad_offset, bad_jac);
        spw_class_lists(ka, cx, t0, n);
        FVB_WAVE_FOR(t, n)
        {
            double Jd = 0;
            for (int i = 0; i < P; i++)
                Jd += sh[L.J + t * Ps + i] * sh[L.pv + i];
            const double k = sh[L.r + t] + Jd;
            sh[L.part + t] = k * k;
        }
        wave_sync();
        if (cx.lane < N)
            for (int q = cst[cx.lane]; q < cst[cx.lane + 1]; q++)
                kk += sh[L.part + ord[q]];
        wave_sync();
    }
    if (cx.lane < N)
        sh[L.kq + cx.lane] = kk;
    wave_sync();
}

// tr(Sigma A_k) of every class into L.trs, and the class counts (the trace of Q_k) into L.cnt
__device__ __forceinline__ void spw_class_traces(const SpatialArgs &sa, WaveCtx &cx)
{
    const WaveLayout &L = cx.L;
    for (int k = 0; k < L.N; k++)
    {
        const double tr = spw_trace_SA(cx, k);
        if (cx.lane == 0)
        {
            cx.sh[L.trs + k] = tr;
            cx.sh[L.cnt + k] = sa.nz_count[k];
        }
    }
    wave_sync();
}

// the residual at the linearisation centre, k'Q_k k = s_k
__device__ __forceinline__ void spw_class_residual_at_centre(WaveCtx &cx)
{
    FVB_WAVE_FOR(k, cx.L.N)
    cx.sh[cx.L.kq + k] = cx.sh[cx.L.s + k];
    wave_sync();
}

// the free energy's residual terms (one noise precision) into LDS for wave_free_energy / wave_update_noise
__device__ __forceinline__ void spw_set_residual(const KernelArgs &ka, WaveCtx &cx, double kk, double trSA)
{
    if (cx.lane == 0)
    {
        cx.sh[cx.L.kq] = kk;
        cx.sh[cx.L.trs] = trSA;
        cx.sh[cx.L.cnt] = (double)ka.n_unmasked;
    }
    wave_sync();
}

// ---- setup: Vb::SetupPerVoxelDists (inference_vb.cc:207-247), one workgroup per voxel ------------------------------
// CLASSES: the form for N = cfg.n_phis > 1 noise precisions (class rows of the state image, N-fold LDS class areas)
template <class Rows, bool CLASSES = false>
__device__ __forceinline__ void spw_setup(const SpatialArgs &sa)
{
    const KernelArgs &ka = sa.ka;
    const int v = blockIdx.x;
    const size_t V = (size_t)ka.cfg.n_voxels;
    if (v >= ka.cfg.n_voxels)
        return;
    const int P = ka.cfg.n_params;
    const int N = CLASSES ? ka.cfg.n_phis : 1;
    WaveCtx cx;
    spw_init_ctx(cx, v, V, Rows::layout(P, N));
    const WaveLayout &L = cx.L;
    const SpWideLayout S = sp_wide_layout(P);
    double *sh = cx.sh;
    if (ka.cfg.init_mvn)
    {
        const int n = P + N, nCov = n * (n + 1) / 2;
        const double *src = ka.cfg.init_mvn + v;
        FVB_WAVE_FOR(e, L.PP)
        sh[L.Sig + e] = src[(size_t)tri(e / P, e % P) * V];
        FVB_WAVE_FOR(i, P)
        sh[L.m + i] = src[(size_t)(nCov + i) * V];
        if (CLASSES)
        {
            FVB_WAVE_FOR(k, N) // WhiteParams::InputFromMVN, noisemodel_white.cc:70-79
            {
                const double nm = src[(size_t)(nCov + P + k) * V];
                const double nv = src[(size_t)tri(P + k, P + k) * V];
                const double b = nv / nm;
                sh[L.b + k] = b;
                sh[L.c + k] = nm / b;
            }
        }
        else if (cx.lane == 0)
        {
            const double nm = src[(size_t)(nCov + P) * V];
            const double nv = src[(size_t)tri(P, P) * V];
            const double b = nv / nm; // GammaDist::SetMeanVariance, dist_gamma.cc:29-33
            sh[L.b] = b;
            sh[L.c] = nm / b;
        }
    }
    else
    {
        FVB_WAVE_FOR(e, L.PP)
        sh[L.Sig + e] = 0;
        wave_sync();
        FVB_WAVE_FOR(i, P)
        {
            const int tr = ka.cfg.transform[i];
            const double mean = (ka.cfg.prior_type[i] == FVB_PRIOR_IMAGE) ? ka.cfg.image_prior[i][v] : ka.cfg.post_mean[i];
            sh[L.m + i] = to_fabber(tr, mean);
            sh[L.Sig + i * P + i] = to_fabber_var(tr, ka.cfg.post_var[i]);
        }
        if (CLASSES)
        {
            FVB_WAVE_FOR(k, N)
            {
                sh[L.b + k] = ka.cfg.noise_post_b[k];
                sh[L.c + k] = ka.cfg.noise_post_c[k];
            }
        }
        else if (cx.lane == 0)
        {
            sh[L.b] = ka.cfg.noise_post_b[0];
            sh[L.c] = ka.cfg.noise_post_c[0];
        }
    }
    FVB_WAVE_FOR(i, P)
    {
        sh[L.pm + i] = 0;
        sh[L.pprec + i] = 1;
        // the centre: the posterior means, or the locked centres (inference_vb.cc:225-232)
        sh[L.ml + i] = sa.locked_centres ? sa.locked_centres[(size_t)i * V + v] : sh[L.m + i];
    }
    wave_sync();
    cx.logdetLam = 0;
    const int status = CLASSES ? spw_moments_classes(ka, cx, Rows(sa, v, true)) : spw_moments(ka, cx, Rows(sa, v, true));
    if (cx.lane == 0)
        sa.status[v] = status ? (status | 0x100) : 0;
    spw_store_theta(sa, cx);
    spw_store_noise(sa, cx);
}

// The kernels that are no templates are the engine's alone (vb_spatial_wave.hip defines FVB_SPATIAL_WAVE_ENGINE): a model
// library includes this header in several of its sources for the templates (vb_spatial_wave_model.h) and must not
// define them again.
#if defined(FVB_SPATIAL_WAVE_ENGINE)
__global__ __launch_bounds__(64) void vb_spatial_wave_setup_kernel(const SpatialArgs sa)
{
    spw_setup<SpwHostRows>(sa);
}

// ---- CalculateaK (priors.cc:221-344), runtime P: the lane form's segments, sums and order -------------------------
__global__ __launch_bounds__(256) void vb_spatial_wide_ak_partial_kernel(const SpatialArgs sa)
{
    const KernelArgs &ka = sa.ka;
    const int P = ka.cfg.n_params;
    const SpWideLayout S = sp_wide_layout(P);
    const size_t V = (size_t)ka.cfg.n_voxels;
    const int dims = sa.spatial_dims;
    __shared__ double red[256];
    for (int k = 0; k < P; k++)
    {
        const int type = ka.cfg.prior_type[k];
        if (!is_spatial_type(type))
            continue;
        double trace_term = 0, term2 = 0;
        for (int v = sa.seg_start[blockIdx.x] + threadIdx.x; v < sa.seg_start[blockIdx.x + 1]; v += 256)
        {
            if (sa.status[v] != 0) // ignored voxels (priors.cc:237-240) ...
                continue;
            const double sigmaK = sa.state[(size_t)(S.SIG + tri(k, k)) * V + v];
            const double wK = sa.state[(size_t)(S.M + k) * V + v];
            int nn = 0;
            double SwK = 0;
            for (int i = 0; i < 6; i++)
            {
                const int u = sa.nn[(size_t)v * 6 + i];
                if (u >= 0 && sa.status[u] == 0) // ... are also gone from every neighbour list (IgnoreVoxel)
                {
                    nn++;
                    SwK += wK - sa.state[(size_t)(S.M + k) * V + u];
                }
            }
            if (type == FVB_PRIOR_SPATIAL_m)
                trace_term += sigmaK * dims * 2;
            else if (type == FVB_PRIOR_SPATIAL_M)
                trace_term += sigmaK * (nn + 1e-8);
            else if (type == FVB_PRIOR_SPATIAL_p)
                trace_term += sigmaK * (4 * dims * dims + 2 * dims);
            else
                trace_term += sigmaK * (nn * nn + nn);
            if (type == FVB_PRIOR_SPATIAL_p || type == FVB_PRIOR_SPATIAL_m)
                SwK += wK * (dims * 2 - nn);
            if (type == FVB_PRIOR_SPATIAL_m || type == FVB_PRIOR_SPATIAL_M)
                term2 += SwK * wK;
            else
                term2 += SwK * SwK;
        }
        for (int which = 0; which < 2; which++)
        {
            red[threadIdx.x] = which ? term2 : trace_term;
            __syncthreads();
            for (int s = 128; s > 0; s >>= 1)
            {
                if ((int)threadIdx.x < s)
                    red[threadIdx.x] += red[threadIdx.x + s];
                __syncthreads();
            }
            if (threadIdx.x == 0)
                sa.partials[((size_t)blockIdx.x * P + k) * 2 + which] = red[0];
            __syncthreads();
        }
    }
}

// the segments' partial sums added in segment order; lane 2 k + which (2 P <= 64 lanes)
__global__ __launch_bounds__(64) void vb_spatial_wide_ak_reduce_kernel(const SpatialArgs sa)
{
    constexpr int CHUNK = 512;
    __shared__ double rows[CHUNK];
    const int P = sa.ka.cfg.n_params;
    const int k = threadIdx.x >> 1, which = threadIdx.x & 1;
    const bool mine = k < P && is_spatial_type(sa.ka.cfg.prior_type[k < P ? k : 0]);
    const int per_block = 2 * P;
    const int blocks_per_chunk = CHUNK / per_block;
    double acc = 0;
    for (int b0 = 0; b0 < sa.n_blocks; b0 += blocks_per_chunk)
    {
        const int nb = (sa.n_blocks - b0 < blocks_per_chunk) ? sa.n_blocks - b0 : blocks_per_chunk;
        for (int i = threadIdx.x; i < nb * per_block; i += 64)
            rows[i] = sa.partials[(size_t)b0 * per_block + i];
        __syncthreads();
        if (mine)
            for (int b = 0; b < nb; b++)
                acc += rows[b * per_block + 2 * k + which];
        __syncthreads();
    }
    if (k < P)
        sa.ak_sums[2 * k + which] = mine ? acc : 0.0;
}

__global__ void vb_spatial_wide_ak_final_kernel(const SpatialArgs sa)
{
    const KernelArgs &ka = sa.ka;
    const int k = threadIdx.x;
    if (k >= ka.cfg.n_params || !is_spatial_type(ka.cfg.prior_type[k]))
        return;
    const double trace_term = sa.ak_sums[2 * k + 0], term2 = sa.ak_sums[2 * k + 1];
    const double gk = 1 / (0.5 * trace_term + 0.5 * term2 + 1 / sa.q1);
    const double hK = sa.n_voxels_global * 0.5 + sa.q2;
    double aK = gk * hK;
    if (aK < 1e-50)
        aK = 1e-50;
    double aKMax = aK * sa.spatial_speed;
    if (aKMax < 0.5)
        aKMax = 0.5;
    if ((sa.spatial_speed > 0) && (aK > aKMax))
        aK = aKMax;
    sa.aK[k] = aK;
}
#endif // FVB_SPATIAL_WAVE_ENGINE

// SpatialPrior::ApplyToMVN (priors.cc:362-482) and the other priors of voxel cx.v, one parameter per lane, as
// vb_spatial_theta_kernel codes them (second_order_rec, the status tests on the END points of second-neighbour
// paths). Returns Fprior: the ARD terms added in parameter order.
__device__ __forceinline__ double spw_apply_priors(const SpatialArgs &sa, WaveCtx &cx, int it)
{
    const KernelArgs &ka = sa.ka;
    const WaveLayout &L = cx.L;
    const SpWideLayout S = sp_wide_layout(L.P);
    const int P = L.P, v = cx.v, dims = sa.spatial_dims;
    const size_t V = cx.V;
    double *sh = cx.sh;
    int n1[6];
    bool ok1[6], live1[6];
#pragma unroll
    for (int a = 0; a < 6; a++)
    {
        const int u = sa.nn[(size_t)v * 6 + a];
        n1[a] = (u < 0) ? v : u;
        ok1[a] = (u >= 0);
    }
#pragma unroll
    for (int a = 0; a < 6; a++)
        live1[a] = ok1[a] && (sa.status[n1[a]] == 0);
    FVB_WAVE_FOR(k, P)
    {
        const int type = ka.cfg.prior_type[k];
        double fk = 0;
        if (is_spatial_type(type))
        {
            const double *mk = sa.state + (size_t)(S.M + k) * V;
            int nn = 0, nn2 = 0;
            double contrib_nn = 0, contrib_nn2 = 0;
            for (int a = 0; a < 6; a++)
                if (live1[a])
                {
                    nn++;
                    contrib_nn += mk[n1[a]];
                }
            if (type == FVB_PRIOR_SPATIAL_P || type == FVB_PRIOR_SPATIAL_p)
            {
                for (int a = 0; a < 6; a++)
                {
                    if (!ok1[a])
                        continue;
                    for (int b = 0; b < 6; b++)
                    {
                        const int w = sa.nn[(size_t)n1[a] * 6 + b];
                        if (w >= 0 && w != v && sa.status[w] == 0)
                        {
                            nn2++;
                            contrib_nn2 += -mk[w];
                        }
                    }
                }
            }
            if (type == FVB_PRIOR_SPATIAL_p || type == FVB_PRIOR_SPATIAL_m)
            {
                nn = 2 * dims;
                nn2 = 4 * dims * dims - nn;
            }
            const double aK = sa.aK[k];
            double spatial_prec;
            if (type == FVB_PRIOR_SPATIAL_M)
                spatial_prec = aK * (nn + 1e-8);
            else if (type == FVB_PRIOR_SPATIAL_m)
                spatial_prec = aK * nn;
            else
                spatial_prec = aK * (nn * nn + nn);
            const double prec0 = ka.cfg.prior_prec[k], mean0 = ka.cfg.prior_mean[k];
            const double pprec = (type == FVB_PRIOR_SPATIAL_p || type == FVB_PRIOR_SPATIAL_m) ? spatial_prec : prec0 + spatial_prec;
            double spatial_mean;
            if (type == FVB_PRIOR_SPATIAL_m || type == FVB_PRIOR_SPATIAL_M)
                spatial_mean = contrib_nn * (1 / double(nn));
            else if (nn != 0)
                spatial_mean = second_order_mean(contrib_nn, contrib_nn2, second_order_rec(nn, nn2)); // (priors.cc:455)
            else
                spatial_mean = 0;
            const double pcov = 1.0 / pprec;
            sh[L.pprec + k] = pprec;
            sh[L.pm + k] = (type == FVB_PRIOR_SPATIAL_m || type == FVB_PRIOR_SPATIAL_M)
                ? pcov * spatial_prec * spatial_mean
                : second_order_pm(pcov, spatial_prec, spatial_mean, prec0, mean0);
        }
        else if (type == FVB_PRIOR_ARD) // priors.cc:150-181
        {
            const double mk = sh[L.m + k];
            const double new_cov = mk * mk + sh[L.Sig + k * P + k];
            sh[L.pprec + k] = 1.0 / ((it == 0) ? ka.cfg.prior_var[k] : new_cov);
            sh[L.pm + k] = ka.cfg.prior_mean[k];
            const double bb = 2 / new_cov;
            fk = -1.5 * (log(bb) + digamma(0.5)) - 0.5 - gammaln(0.5) - 0.5 * log(bb);
        }
        else if (type == FVB_PRIOR_IMAGE)
        {
            sh[L.pm + k] = ka.cfg.image_prior[k][v];
            sh[L.pprec + k] = ka.cfg.prior_prec[k];
        }
        else
        {
            sh[L.pm + k] = ka.cfg.prior_mean[k];
            sh[L.pprec + k] = ka.cfg.prior_prec[k];
        }
        sh[L.pv + k] = fk;
    }
    wave_sync();
    double Fprior = 0;
    for (int k = 0; k < P; k++)
        if (ka.cfg.prior_type[k] == FVB_PRIOR_ARD)
            Fprior += sh[L.pv + k];
    wave_sync();
    return Fprior;
}

// ---- first sweep, one level: priors + UpdateTheta (inference_vb.cc:614-672), one workgroup per voxel of the level ----
template <bool NEEDF, bool CLASSES = false>
__global__ __launch_bounds__(64) void vb_spatial_wave_theta_kernel(const SpatialArgs *__restrict__ sap, int level_begin,
    int level_count, int it)
{
    const SpatialArgs &sa = *sap;
    const KernelArgs &ka = sa.ka;
    const int i = blockIdx.x;
    if (i >= level_count)
        return;
    const int v = sa.order[level_begin + i];
    // an ignored voxel still has its priors applied; only the last voxel's are observable (its F term is reused)
    const bool ignored = sa.status[v] != 0;
    if (ignored && v != sa.owned_end - 1)
        return;
    WaveCtx cx;
    spw_init_ctx(cx, v, (size_t)ka.cfg.n_voxels, sp_wave_layout(ka.cfg.n_params, CLASSES ? ka.cfg.n_phis : 1));
    spw_load(sa, cx);
    const double Fprior = spw_apply_priors(sa, cx, it);
    if (v == sa.owned_end - 1 && cx.lane == 0)
        *sa.fprior_last = Fprior;
    if (ignored)
        return;
    if (NEEDF) // F "before" (:643): the means are still the linearisation centre, k'k = s
    {
        if (CLASSES)
        {
            spw_class_traces(sa, cx);
            spw_class_residual_at_centre(cx);
        }
        else
            spw_set_residual(ka, cx, cx.sh[cx.L.s], spw_trace_SA(cx));
        double F;
        bool finite = true;
        const bool ok = wave_free_energy(ka, cx, Fprior, F, finite);
        if (!ok || !finite)
        {
            if (cx.lane == 0)
                sa.status[v] = ok ? FVB_BAD_FREE_ENERGY : FVB_BAD_RESULT;
            return;
        }
    }
    int status = FVB_OK;
    if (!wave_update_theta(cx, 0.0)) // LMalpha = 0 in the spatial loop (:649)
        status = FVB_BAD_RESULT;
    if (NEEDF && status == FVB_OK) // F "theta" (:651)
    {
        double kk, trSA;
        if (CLASSES)
        {
            for (int k = 0; k < cx.L.N; k++) // s_k - 2 d'u_k + d'A_k d and tr(Sigma A_k); L.cnt is F "before"'s
            {
                spw_moment_residual(cx, kk, trSA, k);
                if (cx.lane == 0)
                {
                    cx.sh[cx.L.kq + k] = kk;
                    cx.sh[cx.L.trs + k] = trSA;
                }
            }
            wave_sync();
        }
        else
        {
            spw_moment_residual(cx, kk, trSA);
            spw_set_residual(ka, cx, kk, trSA);
        }
        double F;
        bool finite = true;
        const bool ok = wave_free_energy(ka, cx, Fprior, F, finite);
        if (!ok || !finite)
            status = ok ? FVB_BAD_FREE_ENERGY : FVB_BAD_RESULT;
    }
    if (status != FVB_OK && cx.lane == 0)
        sa.status[v] = status;
    spw_store_theta(sa, cx);
}

// ---- second sweep: UpdateNoise, ReCentre, F (inference_vb.cc:674-722), one workgroup per owned voxel ----------------
template <class Rows, bool NEEDF, bool CLASSES = false>
__device__ __forceinline__ void spw_noise(const SpatialArgs &sa)
{
    const KernelArgs &ka = sa.ka;
    const int v = sa.owned_begin + blockIdx.x;
    if (v >= sa.owned_end)
        return;
    if (sa.status[v] != 0)
        return;
    const int P = ka.cfg.n_params;
    WaveCtx cx;
    spw_init_ctx(cx, v, (size_t)ka.cfg.n_voxels, Rows::layout(P, CLASSES ? ka.cfg.n_phis : 1));
    spw_load(sa, cx);
    const WaveLayout &L = cx.L;
    double *sh = cx.sh;
    // the residual about the centre the moments belong to ...
    double kk = 0, trSA = 0;
    if (CLASSES) // (per class, in L.kq / L.trs / L.cnt)
    {
        spw_direct_residual_classes(ka, cx, Rows(sa, v, false));
        spw_class_traces(sa, cx);
    }
    else
    {
        kk = spw_direct_residual(ka, cx, Rows(sa, v, false));
        trSA = spw_trace_SA(cx);
        spw_set_residual(ka, cx, kk, trSA);
    }
    wave_update_noise(ka, cx);
    // ... and the re-centre about the means of this iteration's first sweep
    int status = FVB_OK;
    if (!sa.locked_linear) // inference_vb.cc:695-696
    {
        FVB_WAVE_FOR(i, P)
        sh[L.ml + i] = sh[L.m + i];
        wave_sync();
        if (CLASSES)
        {
            status = spw_moments_classes(ka, cx, Rows(sa, v, true));
            spw_class_residual_at_centre(cx);
            spw_class_traces(sa, cx);
        }
        else
        {
            status = spw_moments(ka, cx, Rows(sa, v, true));
            kk = sh[L.s]; // the centre is the mean now: k = y - g
            trSA = spw_trace_SA(cx);
        }
    }
    if (status == FVB_OK && NEEDF)
    {
        // only the last of the four F evaluations per iteration is observable; it uses the prior term of the LAST
        // voxel of the first sweep (inference_vb.cc:612,689,702)
        if (!CLASSES)
            spw_set_residual(ka, cx, kk, trSA);
        cx.covValid = true;
        cx.precValid = false;
        double F;
        bool finite = true;
        if (!wave_free_energy(ka, cx, *sa.fprior_last, F, finite))
            status = FVB_BAD_RESULT;
        else if (!finite)
            status = FVB_BAD_FREE_ENERGY;
        else if (ka.out.free_energy && cx.lane == 0)
            ka.out.free_energy[v] = F;
    }
    if (status != FVB_OK && cx.lane == 0)
        sa.status[v] = status;
    spw_store_noise(sa, cx);
}
template <bool NEEDF>
__global__ __launch_bounds__(64) void vb_spatial_wave_noise_kernel(const SpatialArgs sa)
{
    spw_noise<SpwHostRows, NEEDF>(sa);
}

// ---- result image (inference_vb.cc:757-762), lane per voxel ---------------------------------------------------------
#if defined(FVB_SPATIAL_WAVE_ENGINE)
__global__ __launch_bounds__(256) void vb_spatial_wide_pack_kernel(const SpatialArgs sa)
{
    const KernelArgs &ka = sa.ka;
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= ka.cfg.n_voxels)
        return;
    const int P = ka.cfg.n_params;
    const SpWideLayout S = sp_wide_layout(P);
    const size_t V = (size_t)ka.cfg.n_voxels;
    // (N > 1 precisions in this family: white noise under a pattern, the class rows of the state image; AR(1) noise:
    // alpha_1, alpha_2 and phi)
    const bool ar = ka.cfg.noise == FVB_NOISE_AR1;
    const int N = ar ? 3 : ((ka.cfg.noise == FVB_NOISE_WHITE && ka.cfg.n_phis > 1) ? ka.cfg.n_phis : 1);
    const int n = P + N, nCov = n * (n + 1) / 2;
    const double *p = sa.state + v;
    double *dst = ka.out.mvn + v;
    for (int i = 0; i < S.PT; i++)
        dst[(size_t)i * V] = p[(size_t)(S.SIG + i) * V];
    for (int i = 0; i < P; i++)
        dst[(size_t)(nCov + i) * V] = p[(size_t)(S.M + i) * V];
    if (ar) // Ar1cParams::OutputAsMVN (noisemodel_ar.cc:287-300), as SpAr1's pack_noise
    {
        const double *al = p + (size_t)sp_wide_ar_rows(P).AL * V;
        const double b = p[(size_t)S.B * V], c = p[(size_t)S.C * V];
        for (int r = P; r < n; r++)
            for (int cc = 0; cc <= r; cc++)
                dst[(size_t)tri(r, cc) * V] = 0.0;
        dst[(size_t)tri(P, P) * V] = al[2 * V];
        dst[(size_t)tri(P + 1, P) * V] = al[3 * V];
        dst[(size_t)tri(P + 1, P + 1) * V] = al[4 * V];
        dst[(size_t)tri(P + 2, P + 2) * V] = b * b * c;
        dst[(size_t)(nCov + P) * V] = al[0];
        dst[(size_t)(nCov + P + 1) * V] = al[V];
        dst[(size_t)(nCov + P + 2) * V] = b * c;
    }
    else if (N > 1) // noisemodel_white.cc:55-68, in the order of SpPattern's pack_noise
    {
        const SpWideClassRows R = sp_wide_class_rows(P, N);
        for (int k = 0; k < N; k++)
        {
            const double b = p[(size_t)(R.NB + k) * V], c = p[(size_t)(R.NC + k) * V];
            for (int j = 0; j < P + k; j++)
                dst[(size_t)tri(P + k, j) * V] = 0.0;
            dst[(size_t)tri(P + k, P + k) * V] = b * b * c;
            dst[(size_t)(nCov + P + k) * V] = b * c;
        }
    }
    else
    {
        for (int j = 0; j < P; j++)
            dst[(size_t)tri(P, j) * V] = 0.0;
        const double b = p[(size_t)S.B * V], c = p[(size_t)S.C * V];
        dst[(size_t)tri(P, P) * V] = b * b * c;
        dst[(size_t)(nCov + P) * V] = b * c;
    }
    dst[(size_t)(nCov + n) * V] = 1.0;
    if (ka.out.status)
        ka.out.status[v] = sa.status[v];
    if (ka.out.iterations)
        ka.out.iterations[v] = sa.it;
    if (ka.out.free_energy && !ka.cfg.need_f)
        ka.out.free_energy[v] = 1234.5678;
}
#endif // FVB_SPATIAL_WAVE_ENGINE

#endif // __HIPCC__

} // namespace fvb
