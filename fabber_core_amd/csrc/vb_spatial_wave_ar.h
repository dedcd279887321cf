/*
 * vb_spatial_wave_ar.h - the wave-per-voxel spatial family (vb_spatial_wave.h, vb_spatial_wave_model.h) under AR(1) noise
 * with one echo and no cross terms: 2 alphas of which the first is updated, one phi (Ar1cNoiseModel, noisemodel_ar.cc) -
 * the case of SpAr1<P> (vb_spatial_noise.h) for a runtime parameter count up to FVB_MAX_PARAMS.
 *
 * The scheme is the lane policy's. The reference's T x T alpha matrices are three diagonals (vb_lane_ar_kernel.h); the
 * state image keeps, behind the rows of the one-precision image, the alpha posterior, the diagonal moments Ad = sum J_t J_t',
 * ud = sum J_t r_t, sd = sum r_t^2, the lag-1 moments C = sum (J_t J_{t+1}' + J_{t+1} J_t'), uc = sum (J_t r_{t+1} + J_{t+1} r_t),
 * sc = sum r_t r_{t+1} and the first and last rows (sp_wide_ar_rows). The rows A, U, S hold the EFFECTIVE moments J'QJ,
 * J'Q(y - g), (y - g)'Q(y - g) with Q = M00 + E[a] M10 + E[a^2] M20 and B, C phi's posterior, so the engine's first sweep
 * without F (wave_update_theta with one precision) and the a_K kernels run unchanged.
 *
 *   spw_ar_setup<Rows>          initial alpha / phi posterior (hard-coded, given, or the rows of init_mvn), Precalculate,
 *                               the moments about the initial centre
 *   spw_ar_noise<Rows, NEEDF>   the second sweep: k'M_w k summed directly over t, tr(Sigma J'M_w J) from the moments,
 *                               UpdateAlpha + UpdatePhi, the re-centre's moments, the effective moments, F, status
 *   vb_spatial_wave_ar_theta_kernel   the engine's first sweep with F: F "before" from the at-centre forms, F "theta" from
 *                               the moment forms (d = m - ml), as SpAr1::sweep_F
 *
 * A chunk of SPW_TC timepoints of J and r is staged in LDS at a time (Rows::chunk). The lag pair (t0 - 1, t0) straddles two
 * chunks: the last row of J and the last r of a chunk are carried in LDS across the refill (a row of zeros before the
 * first chunk, as the lane form's previous row at t = 0) and every sum adds its terms in timepoint order. The residual
 * k_{t - 1} is carried in a register: every lane adds the same terms in the same order. Masked timepoints do not occur
 * (noisemodel_ar.cc:351-355). The scalars of UpdateAlpha, UpdatePhi and the free energy are computed by every lane from
 * the same operands: control flow stays wave-uniform.
 */
#pragma once

#include "vb_lane_ar_kernel.h"
#include "vb_spatial_wave_model.h"

namespace fvb
{
// sp_wave_model_layout(P) with the AR areas behind it, in fields the family does not use otherwise: XJ = Ad [PT],
// JS = C [PT], band = ud, uc, J1, JT [4 P], W2 = the carried row (J [P], then r), sv_m = sd, sc, r1, rT. Every offset of
// sp_wave_layout and sp_wave_model_layout is unchanged. At P = 32: 67.5 KB.
FVB_HD WaveLayout sp_wave_ar_model_layout(int P)
{
    WaveLayout L = sp_wave_model_layout(P);
    int o = L.n_doubles;
    L.XJ = o;
    o += L.PT;
    L.JS = o;
    o += L.PT;
    L.band = o;
    o += 4 * P;
    L.W2 = o;
    o += P + 1;
    L.sv_m = o;
    o += 4;
    L.n_doubles = o;
    L.bytes = sizeof(double) * (size_t)o;
    return L;
}

#if defined(__HIPCC__)

// where the AR statistics lie in LDS
struct SpwArAreas
{
    int Ad, C, ud, uc, J1, JT, carry, sd, sc, r1, rT;
    __device__ __forceinline__ SpwArAreas(const WaveLayout &L)
        : Ad(L.XJ), C(L.JS), ud(L.band), uc(L.band + L.P), J1(L.band + 2 * L.P), JT(L.band + 3 * L.P), carry(L.W2), sd(L.sv_m),
          sc(L.sv_m + 1), r1(L.sv_m + 2), rT(L.sv_m + 3)
    {
    }
};

// the alpha posterior of voxel cx.v, by every lane (one address: a broadcast)
__device__ __forceinline__ void spw_ar_load_alpha(const SpatialArgs &sa, const WaveCtx &cx, ArAlpha &al)
{
    const double *p = sa.state + (size_t)sp_wide_ar_rows(cx.L.P).AL * cx.V + cx.v;
    al.mean[0] = p[0];
    al.mean[1] = p[cx.V];
    al.c11 = p[2 * cx.V];
    al.c12 = p[3 * cx.V];
    al.c22 = p[4 * cx.V];
    al.a1 = p[5 * cx.V];
    al.a2 = p[6 * cx.V];
}

// the AR rows of the state image -> LDS (SpAr1::load_full)
__device__ __forceinline__ void spw_ar_load(const SpatialArgs &sa, WaveCtx &cx)
{
    const WaveLayout &L = cx.L;
    const SpWideArRows R = sp_wide_ar_rows(L.P);
    const SpwArAreas X(L);
    const int P = L.P;
    const size_t V = cx.V;
    const double *p = sa.state + cx.v;
    double *sh = cx.sh;
    FVB_WAVE_FOR(e, L.PT)
    {
        sh[X.Ad + e] = p[(size_t)(R.AD + e) * V];
        sh[X.C + e] = p[(size_t)(R.CC + e) * V];
    }
    FVB_WAVE_FOR(i, P)
    {
        sh[X.ud + i] = p[(size_t)(R.UD + i) * V];
        sh[X.uc + i] = p[(size_t)(R.UC + i) * V];
        sh[X.J1 + i] = p[(size_t)(R.J1 + i) * V];
        sh[X.JT + i] = p[(size_t)(R.JT + i) * V];
    }
    if (cx.lane == 0)
    {
        sh[X.sd] = p[(size_t)R.SD * V];
        sh[X.sc] = p[(size_t)R.SC * V];
        sh[X.r1] = p[(size_t)R.R1 * V];
        sh[X.rT] = p[(size_t)R.RT * V];
    }
    wave_sync();
}

// SpAr1::store_full
__device__ __forceinline__ void spw_ar_store(const SpatialArgs &sa, WaveCtx &cx, const ArAlpha &al)
{
    const WaveLayout &L = cx.L;
    const SpWideArRows R = sp_wide_ar_rows(L.P);
    const SpwArAreas X(L);
    const int P = L.P;
    const size_t V = cx.V;
    double *p = sa.state + cx.v;
    const double *sh = cx.sh;
    FVB_WAVE_FOR(e, L.PT)
    {
        p[(size_t)(R.AD + e) * V] = sh[X.Ad + e];
        p[(size_t)(R.CC + e) * V] = sh[X.C + e];
    }
    FVB_WAVE_FOR(i, P)
    {
        p[(size_t)(R.UD + i) * V] = sh[X.ud + i];
        p[(size_t)(R.UC + i) * V] = sh[X.uc + i];
        p[(size_t)(R.J1 + i) * V] = sh[X.J1 + i];
        p[(size_t)(R.JT + i) * V] = sh[X.JT + i];
    }
    if (cx.lane == 0)
    {
        double *a = p + (size_t)R.AL * V;
        a[0] = al.mean[0];
        a[V] = al.mean[1];
        a[2 * V] = al.c11;
        a[3 * V] = al.c12;
        a[4 * V] = al.c22;
        a[5 * V] = al.a1;
        a[6 * V] = al.a2;
        p[(size_t)R.SD * V] = sh[X.sd];
        p[(size_t)R.SC * V] = sh[X.sc];
        p[(size_t)R.R1 * V] = sh[X.r1];
        p[(size_t)R.RT * V] = sh[X.rT];
    }
}

// J'MJ, J'Mr, r'Mr for M in { M00 (w = 0), M10 (w = 1), M20 (w = 2) } from the moments in LDS (ar_JMJ, ar_JMr, ar_rMr)
__device__ __forceinline__ double spw_ar_JMJ(const double *sh, const SpwArAreas &X, int w, int i, int j)
{
    if (w == 0)
        return sh[X.Ad + tri(i, j)] - sh[X.J1 + i] * sh[X.J1 + j];
    if (w == 2)
        return sh[X.Ad + tri(i, j)] - sh[X.JT + i] * sh[X.JT + j];
    return -sh[X.C + tri(i, j)];
}
__device__ __forceinline__ double spw_ar_JMr(const double *sh, const SpwArAreas &X, int w, int i)
{
    if (w == 0)
        return sh[X.ud + i] - sh[X.J1 + i] * sh[X.r1];
    if (w == 2)
        return sh[X.ud + i] - sh[X.JT + i] * sh[X.rT];
    return -sh[X.uc + i];
}
__device__ __forceinline__ double spw_ar_rMr(const double *sh, const SpwArAreas &X, int w)
{
    if (w == 0)
        return sh[X.sd] - sh[X.r1] * sh[X.r1];
    if (w == 2)
        return sh[X.sd] - sh[X.rT] * sh[X.rT];
    return -2 * sh[X.sc];
}

// The AR moments about the linearisation of `rows` (recentre_ar_feed): spw_moments' entries, each with its lag-1 partner,
// summed over t in order; the carried row makes the pair across a chunk boundary. Returns the re-centre's status.
template <class Rows>
__device__ __forceinline__ int spw_ar_moments(const KernelArgs &ka, WaveCtx &cx, const Rows &rows)
{
    const WaveLayout &L = cx.L;
    const SpwArAreas X(L);
    const int T = ka.cfg.n_times, P = L.P, Ps = L.Ps, PT = L.PT;
    const int E = PT + P + 1;
    double *sh = cx.sh;
    // this lane's entries e = lane + 64 k: two columns x, y of the staged chunk (a column of J with stride Ps, or r) and
    // of the carried row; x = -1: none
    int xa[SPW_MAX_SLOTS], xb[SPW_MAX_SLOTS];
    double acc[SPW_MAX_SLOTS], lag[SPW_MAX_SLOTS];
#pragma unroll
    for (int k = 0; k < SPW_MAX_SLOTS; k++)
    {
        const int e = cx.lane + 64 * k;
        acc[k] = lag[k] = 0;
        xa[k] = xb[k] = P; // r (column P of the carried row)
        if (e < PT)
        {
            int a = 0;
            while ((a + 1) * (a + 2) / 2 <= e)
                a++;
            xa[k] = a;
            xb[k] = e - a * (a + 1) / 2;
        }
        else if (e < PT + P)
            xa[k] = e - PT;
        else if (e != E - 1)
            xa[k] = -1;
    }
    FVB_WAVE_FOR(i, P + 1)
    sh[X.carry + i] = 0; // (the previous row is zero at t = 0)
    bool bad_offset = false, bad_jac = false;
    rows.centre(ka, cx);
    for (int t0 = 0; t0 < T; t0 += SPW_TC)
    {
        const int n = (T - t0 < SPW_TC) ? T - t0 : SPW_TC;
        rows.chunk(ka, cx, nullptr, t0, n, bad_offset, bad_jac);
#pragma unroll
        for (int k = 0; k < SPW_MAX_SLOTS; k++)
        {
            if (xa[k] < 0)
                continue;
            // column c of row t: J[t][c], or r[t] for c = P
            const int oa = (xa[k] == P) ? L.r : L.J + xa[k], sa_ = (xa[k] == P) ? 1 : Ps;
            const int ob = (xb[k] == P) ? L.r : L.J + xb[k], sb_ = (xb[k] == P) ? 1 : Ps;
            const bool rr = xa[k] == P; // r'r: the lag sum is sum r_{t-1} r_t, not symmetrised
            double pa = sh[X.carry + xa[k]], pb = sh[X.carry + xb[k]];
            for (int t = 0; t < n; t++)
            {
                const double ca = sh[oa + t * sa_], cb = sh[ob + t * sb_];
                acc[k] += ca * cb;
                lag[k] += rr ? pa * ca : pa * cb + ca * pb;
                pa = ca;
                pb = cb;
            }
        }
        if (t0 == 0)
        {
            FVB_WAVE_FOR(i, P)
            sh[X.J1 + i] = sh[L.J + i];
            if (cx.lane == 0)
                sh[X.r1] = sh[L.r];
        }
        wave_sync(); // (every lane has read the carried row)
        FVB_WAVE_FOR(i, P)
        sh[X.carry + i] = sh[L.J + (n - 1) * Ps + i];
        if (cx.lane == 0)
            sh[X.carry + P] = sh[L.r + n - 1];
        wave_sync(); // (the next chunk overwrites the staged one)
    }
#pragma unroll
    for (int k = 0; k < SPW_MAX_SLOTS; k++)
    {
        const int e = cx.lane + 64 * k;
        if (e < PT)
        {
            sh[X.Ad + e] = acc[k];
            sh[X.C + e] = lag[k];
        }
        else if (e < PT + P)
        {
            sh[X.ud + e - PT] = acc[k];
            sh[X.uc + e - PT] = lag[k];
        }
        else if (e == E - 1)
        {
            sh[X.sd] = acc[k];
            sh[X.sc] = lag[k];
        }
    }
    FVB_WAVE_FOR(i, P)
    sh[X.JT + i] = sh[X.carry + i];
    if (cx.lane == 0)
        sh[X.rT] = sh[X.carry + P];
    wave_sync();
    const bool any_offset = __any(bad_offset), any_jac = __any(bad_jac);
    return any_offset ? FVB_BAD_OFFSET : (any_jac ? FVB_BAD_JACOBIAN : FVB_OK);
}

// k'M00 k, k'M10 k, k'M20 k with k = y - g(ml) + J (ml - m) summed directly over t in order (exact_residual_ar_feed), g
// and J from the linearisation the moments in the state belong to; k_{t - 1} crosses a chunk boundary in a register
template <class Rows>
__device__ __forceinline__ void spw_ar_direct_residual(const KernelArgs &ka, WaveCtx &cx, const Rows &rows, ArForms &f)
{
    const WaveLayout &L = cx.L;
    const int T = ka.cfg.n_times, P = L.P, Ps = L.Ps;
    double *sh = cx.sh;
    FVB_WAVE_FOR(i, P)
    sh[L.pv + i] = sh[L.ml + i] - sh[L.m + i];
    bool bad_offset = false, bad_jac = false; // (the set-up or the previous re-centre has reported these already)
    double sum_all = 0, cross = 0, k_first = 0, k_prev = 0;
    rows.centre(ka, cx);
    for (int t0 = 0; t0 < T; t0 += SPW_TC)
    {
        const int n = (T - t0 < SPW_TC) ? T - t0 : SPW_TC;
        rows.chunk(ka, cx, nullptr, t0, n, bad_offset, bad_jac);
        FVB_WAVE_FOR(t, n)
        {
            double Jd = 0;
            for (int i = 0; i < P; i++)
                Jd += sh[L.J + t * Ps + i] * sh[L.pv + i];
            sh[L.part + t] = sh[L.r + t] + Jd;
        }
        wave_sync();
        if (t0 == 0)
            k_first = sh[L.part];
        for (int t = 0; t < n; t++)
        {
            const double k = sh[L.part + t];
            sum_all += k * k;
            cross += k_prev * k;
            k_prev = k;
        }
        wave_sync();
    }
    f.kk[0] = sum_all - k_first * k_first;
    f.kk[2] = sum_all - k_prev * k_prev;
    f.kk[1] = -2 * cross;
}

// tr(Sigma J'M_w J), w = 0, 1, 2, from the moments: a row of the P x P contraction per lane, the rows added in order
__device__ __forceinline__ void spw_ar_traces(WaveCtx &cx, ArForms &f)
{
    const WaveLayout &L = cx.L;
    const SpwArAreas X(L);
    const int P = L.P;
    double *sh = cx.sh;
    FVB_WAVE_FOR(i, P)
    {
        double t0 = 0, t1 = 0, t2 = 0;
        for (int j = 0; j < P; j++)
        {
            const double sij = sh[L.Sig + i * P + j];
            t0 += sij * spw_ar_JMJ(sh, X, 0, i, j);
            t1 += sij * spw_ar_JMJ(sh, X, 1, i, j);
            t2 += sij * spw_ar_JMJ(sh, X, 2, i, j);
        }
        sh[L.pv + i] = t0;
        sh[L.pv + P + i] = t1;
        sh[L.pv + 2 * P + i] = t2;
    }
    wave_sync();
    f.tr[0] = f.tr[1] = f.tr[2] = 0;
    for (int i = 0; i < P; i++)
    {
        f.tr[0] += sh[L.pv + i];
        f.tr[1] += sh[L.pv + P + i];
        f.tr[2] += sh[L.pv + 2 * P + i];
    }
    wave_sync();
}

// with the linearisation centred on the current means (d = 0): k = r (ar_residuals_at_centre)
__device__ __forceinline__ void spw_ar_forms_at_centre(WaveCtx &cx, ArForms &f)
{
    const SpwArAreas X(cx.L);
    spw_ar_traces(cx, f);
    for (int w = 0; w < 3; w++)
        f.kk[w] = spw_ar_rMr(cx.sh, X, w);
}

// k'M_w k = r'M_w r - 2 d'J'M_w r + d'J'M_w J d with d = m - ml, and the traces (ar_forms): what F "theta" reads
__device__ __forceinline__ void spw_ar_moment_forms(WaveCtx &cx, ArForms &f)
{
    const WaveLayout &L = cx.L;
    const SpwArAreas X(L);
    const int P = L.P;
    double *sh = cx.sh;
    spw_ar_traces(cx, f);
    for (int w = 0; w < 3; w++)
    {
        FVB_WAVE_FOR(i, P)
        {
            const double di = sh[L.m + i] - sh[L.ml + i];
            double dA = 0;
            for (int j = 0; j < P; j++)
                dA += spw_ar_JMJ(sh, X, w, i, j) * (sh[L.m + j] - sh[L.ml + j]);
            sh[L.pv + i] = di * spw_ar_JMr(sh, X, w, i);
            sh[L.pv + P + i] = di * dA;
        }
        wave_sync();
        double du = 0, dAd = 0;
        for (int i = 0; i < P; i++)
        {
            du += sh[L.pv + i];
            dAd += sh[L.pv + P + i];
        }
        f.kk[w] = spw_ar_rMr(sh, X, w) - 2 * du + dAd;
        wave_sync();
    }
}

// The effective moments into the one-precision areas (SpAr1::effective): A = J'QJ, u = J'Q(y - g), s = (y - g)'Q(y - g)
// with the marginal Q of the alpha posterior
__device__ __forceinline__ void spw_ar_effective(WaveCtx &cx, const ArAlpha &al)
{
    const WaveLayout &L = cx.L;
    const SpwArAreas X(L);
    const int P = L.P;
    double *sh = cx.sh;
    FVB_WAVE_FOR(e, L.PT)
    {
        int i = 0;
        while ((i + 1) * (i + 2) / 2 <= e)
            i++;
        const int j = e - i * (i + 1) / 2;
        sh[L.A + e] = spw_ar_JMJ(sh, X, 0, i, j) + al.a1 * spw_ar_JMJ(sh, X, 1, i, j) + al.a2 * spw_ar_JMJ(sh, X, 2, i, j);
    }
    FVB_WAVE_FOR(i, P)
    sh[L.u + i] = spw_ar_JMr(sh, X, 0, i) + al.a1 * spw_ar_JMr(sh, X, 1, i) + al.a2 * spw_ar_JMr(sh, X, 2, i);
    if (cx.lane == 0)
        sh[L.s] = spw_ar_rMr(sh, X, 0) + al.a1 * spw_ar_rMr(sh, X, 1) + al.a2 * spw_ar_rMr(sh, X, 2);
    wave_sync();
}

// UpdateAlpha + UpdatePhi (noisemodel_ar.cc:447-556) by every lane: update_noise_ar itself, which reads and writes of
// the voxel's state phi's posterior alone. Returns its status; the new (b, c) are in LDS.
__device__ __forceinline__ int spw_ar_update_noise(const KernelArgs &ka, WaveCtx &cx, ArAlpha &al, const ArForms &f)
{
    const WaveLayout &L = cx.L;
    VoxelState<1> ph;
    ph.b = cx.sh[L.b];
    ph.c = cx.sh[L.c];
    const int status = update_noise_ar<1>(ka, ph, al, f);
    wave_sync(); // (every lane has read b and c)
    if (cx.lane == 0)
    {
        cx.sh[L.b] = ph.b;
        cx.sh[L.c] = ph.c;
    }
    wave_sync();
    return status;
}

// Ar1cNoiseModel::CalcFreeEnergy (noisemodel_ar.cc:643-747) as calc_free_energy_ar evaluates it; every lane computes the
// same scalar
__device__ __forceinline__ bool spw_ar_free_energy(const KernelArgs &ka, WaveCtx &cx, const ArAlpha &al, const ArForms &f, double Fprior,
    double &F, bool &finite)
{
    const bool ok = wave_ensure_prec(cx);
    const WaveLayout &L = cx.L;
    const int P = L.P;
    const double *sh = cx.sh;
    const double T = (double)ka.cfg.n_times;
    const double si = sh[L.b], ci = sh[L.c], siPrior = ka.cfg.noise_prior_b[0], ciPrior = ka.cfg.noise_prior_c[0];
    const double phibar = si * ci;
    const double logdetAlphaPrec = -log(fabs(al.c11 * al.c22 - al.c12 * al.c12));
    const double expectedLogAlphaDist = 0.5 * logdetAlphaPrec - 0.5 * 2 * (LOG_2PI + 1);
    const double expectedLogThetaDist = 0.5 * cx.logdetLam - 0.5 * P * (LOG_2PI + 1);
    const double dg = digamma(ci) + log(si);
    const double expectedLogPhiDist = -gammaln(ci) - ci * log(si) - ci + (ci - 1) * dg;
    double parts = dg * ((T - 1) * 0.5 + ciPrior - 1);                                // [0]
    parts += -2 * gammaln(ciPrior) - 2 * ciPrior * log(siPrior) - si * ci / siPrior; // [9]
    parts += -LOG_2PI * (T - 1 + 0.5 * 2 + 0.5 * P);                                 // [1]
    const double kQk = f.kk[0] + al.a1 * f.kk[1] + al.a2 * f.kk[2];
    const double trQ = f.tr[0] + al.a1 * f.tr[1] + al.a2 * f.tr[2];
    parts += -0.5 * phibar * kQk - 0.5 * phibar * trQ;                               // [2]
    double logdetPrior = 0, quad = 0, trSL0 = 0;
    for (int i = 0; i < P; i++)
    {
        logdetPrior += log(fabs(sh[L.pprec + i]));
        const double dm = sh[L.m + i] - sh[L.pm + i];
        quad += dm * sh[L.pprec + i] * dm;
        trSL0 += sh[L.Sig + i * P + i] * sh[L.pprec + i];
    }
    parts += 0.5 * logdetPrior; // [3]
    parts += -0.5 * quad;       // [4]
    parts += -0.5 * trSL0;      // [5]
    if (ka.cfg.ar_alpha_given & 1) // the prior of noise-initial-prior (:720-729)
    {
        const double p11 = ka.cfg.ar_alpha_prior_prec[0][0], p12 = ka.cfg.ar_alpha_prior_prec[0][1], p22 = ka.cfg.ar_alpha_prior_prec[1][1];
        const double d1 = al.mean[0] - ka.cfg.ar_alpha_prior_mean[0], d2 = al.mean[1] - ka.cfg.ar_alpha_prior_mean[1];
        parts += 0.5 * log(fabs(p11 * p22 - p12 * p12));                     // [6]
        parts += -0.5 * (d1 * p11 * d1 + 2 * d1 * p12 * d2 + d2 * p22 * d2); // [7]
        parts += -0.5 * (al.c11 * p11 + 2 * al.c12 * p12 + al.c22 * p22);    // [8]
    }
    else
    {
        parts += 0.5 * 2 * log(AR_ALPHA_PRIOR_PREC);                                               // [6]
        parts += -0.5 * AR_ALPHA_PRIOR_PREC * (al.mean[0] * al.mean[0] + al.mean[1] * al.mean[1]); // [7]
        parts += -0.5 * AR_ALPHA_PRIOR_PREC * (al.c11 + al.c22);                                   // [8]
    }
    F = -expectedLogAlphaDist - expectedLogThetaDist - expectedLogPhiDist + parts;
    finite = is_finite(F);
    F += Fprior;
    return ok;
}

// ---- setup: Vb::SetupPerVoxelDists (inference_vb.cc:207-247) with SpAr1::init_noise, one workgroup per voxel ----------
template <class Rows>
__device__ __forceinline__ void spw_ar_setup(const SpatialArgs &sa)
{
    const KernelArgs &ka = sa.ka;
    const int v = blockIdx.x;
    const size_t V = (size_t)ka.cfg.n_voxels;
    if (v >= ka.cfg.n_voxels)
        return;
    const int P = ka.cfg.n_params;
    WaveCtx cx;
    spw_init_ctx(cx, v, V, sp_wave_ar_model_layout(P));
    const WaveLayout &L = cx.L;
    double *sh = cx.sh;
    ArAlpha al;
    double b, c;
    if (ka.cfg.init_mvn) // MVNDist::Load, GetSubmatrix, Ar1cParams::InputFromMVN (noisemodel_ar.cc:302-316)
    {
        const int n = P + 3, nCov = n * (n + 1) / 2;
        const double *src = ka.cfg.init_mvn + v;
        FVB_WAVE_FOR(e, L.PP)
        sh[L.Sig + e] = src[(size_t)tri(e / P, e % P) * V];
        FVB_WAVE_FOR(i, P)
        sh[L.m + i] = src[(size_t)(nCov + i) * V];
        al.mean[0] = src[(size_t)(nCov + P) * V];
        al.mean[1] = src[(size_t)(nCov + P + 1) * V];
        al.c11 = src[(size_t)tri(P, P) * V];
        al.c12 = src[(size_t)tri(P + 1, P) * V];
        al.c22 = src[(size_t)tri(P + 1, P + 1) * V];
        const double nm = src[(size_t)(nCov + P + 2) * V];
        const double nv = src[(size_t)tri(P + 2, P + 2) * V];
        b = nv / nm; // GammaDist::SetMeanVariance, dist_gamma.cc:29-33
        c = nm / b;
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
        ar_initial_alpha(ka, al); // HardcodedInitialDists (noisemodel_ar.cc:379-403), or noise-initial-posterior
        b = ka.cfg.noise_post_b[0];
        c = ka.cfg.noise_post_c[0];
    }
    // Ar1cNoiseModel::Precalculate (noisemodel_ar.cc:749-769)
    al.a1 = al.mean[0];
    al.a2 = al.c11 + al.mean[0] * al.mean[0];
    c = ka.cfg.noise_prior_c[0] + ((double)ka.cfg.n_times - 1) * 0.5;
    if (cx.lane == 0)
    {
        sh[L.b] = b;
        sh[L.c] = c;
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
    const int status = spw_ar_moments(ka, cx, Rows(sa, v, true));
    if (cx.lane == 0)
        sa.status[v] = status ? (status | 0x100) : 0;
    spw_ar_effective(cx, al);
    spw_store_theta(sa, cx);
    spw_store_noise(sa, cx);
    spw_ar_store(sa, cx, al);
}

// ---- second sweep: UpdateNoise, ReCentre, F (inference_vb.cc:674-722) as vb_spatial_noise_nz_kernel<SpAr1> ---------------
template <class Rows, bool NEEDF>
__device__ __forceinline__ void spw_ar_noise(const SpatialArgs &sa)
{
    const KernelArgs &ka = sa.ka;
    const int v = sa.owned_begin + blockIdx.x;
    if (v >= sa.owned_end)
        return;
    if (sa.status[v] != 0)
        return;
    const int P = ka.cfg.n_params;
    WaveCtx cx;
    spw_init_ctx(cx, v, (size_t)ka.cfg.n_voxels, sp_wave_ar_model_layout(P));
    spw_load(sa, cx); // (the effective moments)
    spw_ar_load(sa, cx);
    const WaveLayout &L = cx.L;
    double *sh = cx.sh;
    ArAlpha al;
    spw_ar_load_alpha(sa, cx, al);
    // the residual forms about the centre the moments belong to, the traces from the stored moments ...
    ArForms f;
    spw_ar_traces(cx, f);
    spw_ar_direct_residual(ka, cx, Rows(sa, v, false), f);
    int status = spw_ar_update_noise(ka, cx, al, f);
    // ... and the re-centre about the means of this iteration's first sweep
    if (status == FVB_OK && !sa.locked_linear) // inference_vb.cc:695-696
    {
        FVB_WAVE_FOR(i, P)
        sh[L.ml + i] = sh[L.m + i];
        wave_sync();
        status = spw_ar_moments(ka, cx, Rows(sa, v, true));
    }
    if (status == FVB_OK && NEEDF)
    {
        // only the last of the four F evaluations per iteration is observable; it uses the prior term of the LAST
        // voxel of the first sweep (inference_vb.cc:612,689,702)
        if (!sa.locked_linear)
            spw_ar_forms_at_centre(cx, f); // (the centre is the mean now: k = y - g)
        cx.covValid = true;
        cx.precValid = false;
        double F;
        bool finite = true;
        if (!spw_ar_free_energy(ka, cx, al, f, *sa.fprior_last, F, finite))
            status = FVB_BAD_RESULT;
        else if (!finite)
            status = FVB_BAD_FREE_ENERGY;
        else if (ka.out.free_energy && cx.lane == 0)
            ka.out.free_energy[v] = F;
    }
    if (status != FVB_OK && cx.lane == 0)
        sa.status[v] = status;
    spw_ar_effective(cx, al);
    spw_store_noise(sa, cx);
    spw_ar_store(sa, cx, al);
}

template <class Eval>
__global__ __launch_bounds__(64) void vb_spatial_wave_ar_setup_kernel(const SpatialArgs sa)
{
    spw_ar_setup<SpwBodyRows<Eval> >(sa);
}

template <class Eval, bool NEEDF>
__global__ __launch_bounds__(64) void vb_spatial_wave_ar_noise_kernel(const SpatialArgs sa)
{
    spw_ar_noise<SpwBodyRows<Eval>, NEEDF>(sa);
}

// ---- first sweep with F, one level: vb_spatial_wave_theta_kernel<true> with the AR free energy (SpAr1::sweep_F) ----------
// (without F the first sweep does not depend on the noise model: the engine's vb_spatial_wave_theta_kernel<false>)
#if defined(FVB_SPATIAL_WAVE_ENGINE)
__global__ __launch_bounds__(64) void vb_spatial_wave_ar_theta_kernel(const SpatialArgs *__restrict__ sap, int level_begin, int level_count,
    int it)
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
    spw_init_ctx(cx, v, (size_t)ka.cfg.n_voxels, sp_wave_ar_model_layout(ka.cfg.n_params));
    spw_load(sa, cx);
    const double Fprior = spw_apply_priors(sa, cx, it);
    if (v == sa.owned_end - 1 && cx.lane == 0)
        *sa.fprior_last = Fprior;
    if (ignored)
        return;
    spw_ar_load(sa, cx);
    ArAlpha al;
    spw_ar_load_alpha(sa, cx, al);
    ArForms f;
    {
        // F "before" (:643): the means are still the linearisation centre
        spw_ar_forms_at_centre(cx, f);
        double F;
        bool finite = true;
        const bool ok = spw_ar_free_energy(ka, cx, al, f, Fprior, F, finite);
        if (!ok || !finite)
        {
            if (cx.lane == 0)
                sa.status[v] = ok ? FVB_BAD_FREE_ENERGY : FVB_BAD_RESULT;
            return;
        }
    }
    int status = FVB_OK;
    if (!wave_update_theta(cx, 0.0)) // (the effective moments; LMalpha = 0 in the spatial loop, :649)
        status = FVB_BAD_RESULT;
    if (status == FVB_OK) // F "theta" (:651)
    {
        spw_ar_moment_forms(cx, f);
        double F;
        bool finite = true;
        const bool ok = spw_ar_free_energy(ka, cx, al, f, Fprior, F, finite);
        if (!ok || !finite)
            status = ok ? FVB_BAD_FREE_ENERGY : FVB_BAD_RESULT;
    }
    if (status != FVB_OK && cx.lane == 0)
        sa.status[v] = status;
    spw_store_theta(sa, cx);
}
#endif // FVB_SPATIAL_WAVE_ENGINE

#endif // __HIPCC__
} // namespace fvb
