// The depth step of one column of the period maps: the small dense regularised Gauss-Newton step that moves a column's
// Vs(z) towards its K observed phase / group velocities, given the column's curve pv and its combined depth kernels S = d c / d Vs
// (ray_kernels.hip: k_sen_combine).  M = nz - 1 unknowns (the bottom depth is kept, as dsa_model_update keeps it), K data in slot order.
//
//   used     datum k is used iff wt_k > 0, obs_k > 0 and pv_k > 0 (pv = 0: the curve has no root); the S of any other datum is never read
//   data     a_k = (double)wt_k, r_k = (double)obs_k - pv_k, rho_k = a_k r_k, g_kl = a_k S_kl (one rounding)
//            N_ll' = sum_k g_kl g_kl' (l' <= l), b_l = sum_k g_kl rho_k, chi2 = sum_k rho_k rho_k, over the used k ascending, from 0.0
//   smooth   N_ll' = N_ll' + smooth^2 (double)column_ltl(M, l, l'), then on the diagonal + damp^2, in that order
//   factor   N = L D L^T without a square root, column by column; a pivot that is not finite or <= 0 flags the column (flag 1)
//   solve    forward with p ascending, the division by d, back with i descending and p ascending, every sum subtracted term by term
//   apply    fp32: s = (float)delta clipped to +-dvmax, v = v + s clamped to [minvel, maxvel], dsa_model_update's comparisons
//
// fp64 under -ffp-contract=off: one rounding per operation, no square root, IEEE division -- every figure has one value whatever computes
// it.  One copy of the arithmetic: the functions take (lane, nlanes, sync) and share their loops out over the lanes of one wavefront
// (column_kernels.hip: k_column_step, sync = a barrier of the block) or run them on one (tests/hostcheck_columns.cpp: lane 0 of 1, sync a
// no-op).  Every figure is one sequential chain of its own, so the lane mapping cannot change a bit.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define DSA_CS __host__ __device__ __forceinline__
#else
#define DSA_CS static inline
#endif

namespace dsa {

constexpr int kColumnMaxM = 63;        // nz <= 64 (Engine::dispersion_setup)
constexpr int kColumnMaxK = 60;        // kMaxPeriods

enum { kColumnOk = 0, kColumnNotPositive = 1, kColumnNoData = 2 };

// packed lower triangle, row by row: (i, j) with j <= i
DSA_CS int column_tri(int i, int j) { return i * (i + 1) / 2 + j; }
DSA_CS int column_tri_size(int M) { return M * (M + 1) / 2; }
// the row of packed entry e
DSA_CS int column_tri_row(int e)
{
    int i = 0;
    while (column_tri(i + 1, 0) <= e) ++i;
    return i;
}

// Entry (l, l') of L^T L in closed form.  L: for M >= 2 a top row (1, -1) on unknowns 0, 1 and a bottom row (-1, 1) on M-2, M-1; for
// M >= 3 the rows (-1, 2, -1) centred on 1 .. M-2.  M = 1: no rows.
DSA_CS int column_ltl(int M, int l, int lp)
{
    if (M < 2 || l < 0 || lp < 0 || l >= M || lp >= M) return 0;
    const int lo = l < lp ? l : lp, dist = l < lp ? lp - l : l - lp;
    #define DSA_CS_CENTRE(c) (((c) >= 1 && (c) <= M - 2) ? 1 : 0)
    int v = 0;
    if (dist == 0) v = (lo <= 1 ? 1 : 0) + (lo >= M - 2 ? 1 : 0) + 4 * DSA_CS_CENTRE(lo) + DSA_CS_CENTRE(lo - 1) + DSA_CS_CENTRE(lo + 1);
    else if (dist == 1) v = -(lo == 0 ? 1 : 0) - (lo == M - 2 ? 1 : 0) - 2 * DSA_CS_CENTRE(lo) - 2 * DSA_CS_CENTRE(lo + 1);
    else if (dist == 2) v = DSA_CS_CENTRE(lo + 1);
    #undef DSA_CS_CENTRE
    return v;
}

// one column's inputs where they lie: element k of obs / wt / pv at k * stride, S_kl at l * s_lstride + k * s_kstride.  wt may be null (1).
struct ColumnIn {
    int M, K;
    const float* obs; long long obs_stride;
    const float* wt; long long wt_stride;
    const double* pv; long long pv_stride;
    const double* S; long long s_lstride, s_kstride;
};

// work arrays of one column: tri (the packed N, then L below the diagonal), G (K x M, g_kl at k M + l), a and rho (K), b (M: the right-hand
// side, then the solution), v and d (M)
struct ColumnWork { double *tri, *G, *a, *rho, *b, *v, *d; };

DSA_CS size_t column_work_doubles(int M, int K) { return (size_t)column_tri_size(M) + (size_t)K * M + 2 * (size_t)K + 3 * (size_t)M; }

DSA_CS ColumnWork column_work(double* base, int M, int K)
{
    ColumnWork w;
    w.tri = base; base += column_tri_size(M);
    w.G = base; base += (size_t)K * M;
    w.a = base; base += K;
    w.rho = base; base += K;
    w.b = base; base += M;
    w.v = base; base += M;
    w.d = base;
    return w;
}

// the data part and the regularisation: w.tri = N, w.b = b.  Returns nused; *chi2 is the weighted misfit.  Every lane returns the same.
template <class Sync>
DSA_CS int column_assemble(const ColumnIn& in, double lambda2, double mu2, const ColumnWork& w, double* chi2, int lane, int nlanes, Sync sync)
{
    const int M = in.M, K = in.K;
    for (int k = lane; k < K; k += nlanes) {
        const float o = in.obs[k * in.obs_stride], wt = in.wt ? in.wt[k * in.wt_stride] : 1.0f;
        const double p = in.pv[k * in.pv_stride];
        const bool used = wt > 0.0f && o > 0.0f && p > 0.0;
        const double a = used ? (double)wt : 0.0;
        w.a[k] = a;
        w.rho[k] = used ? a * ((double)o - p) : 0.0;
    }
    sync();
    for (int e = lane; e < K * M; e += nlanes) {
        const int k = e / M, l = e - k * M;
        w.G[e] = w.a[k] > 0.0 ? w.a[k] * in.S[l * in.s_lstride + k * in.s_kstride] : 0.0;
    }
    sync();
    for (int e = lane; e < column_tri_size(M); e += nlanes) {
        const int l = column_tri_row(e), lp = e - column_tri(l, 0);
        double s = 0.0;
        for (int k = 0; k < K; ++k)
            if (w.a[k] > 0.0) s += w.G[k * M + l] * w.G[k * M + lp];
        s = s + lambda2 * (double)column_ltl(M, l, lp);
        if (l == lp) s = s + mu2;
        w.tri[e] = s;
    }
    for (int l = lane; l < M; l += nlanes) {
        double s = 0.0;
        for (int k = 0; k < K; ++k)
            if (w.a[k] > 0.0) s += w.G[k * M + l] * w.rho[k];
        w.b[l] = s;
    }
    int nused = 0;
    double c = 0.0;
    for (int k = 0; k < K; ++k)
        if (w.a[k] > 0.0) { ++nused; c += w.rho[k] * w.rho[k]; }
    *chi2 = c;
    sync();
    return nused;
}

// N = L D L^T in place: w.tri keeps N's diagonal and gets L below it, w.d the pivots.  Stops at a pivot that is not finite or <= 0 and
// returns kColumnNotPositive.  Every lane returns the same.
template <class Sync>
DSA_CS int column_factor(int M, const ColumnWork& w, int lane, int nlanes, Sync sync)
{
    for (int j = 0; j < M; ++j) {
        for (int p = lane; p < j; p += nlanes) w.v[p] = w.tri[column_tri(j, p)] * w.d[p];
        sync();
        double dj = w.tri[column_tri(j, j)];
        for (int p = 0; p < j; ++p) dj -= w.tri[column_tri(j, p)] * w.v[p];
        if (!(isfinite(dj) && dj > 0.0)) return kColumnNotPositive;          // (every lane holds the same dj: all leave together)
        if (lane == 0) w.d[j] = dj;
        for (int i = j + 1 + lane; i < M; i += nlanes) {
            double s = w.tri[column_tri(i, j)];
            for (int p = 0; p < j; ++p) s -= w.tri[column_tri(i, p)] * w.v[p];
            w.tri[column_tri(i, j)] = s / dj;
        }
        sync();
    }
    return kColumnOk;
}

// L D L^T delta = b in place in w.b.  Forward: b_i loses L_ip b_p for p ascending (column by column: every i takes its terms in that
// order); b_i / d_i; back: i descending, b_i loses L_pi b_p for p = i+1 .. M-1 ascending -- a chain through the solution, on lane 0.
template <class Sync>
DSA_CS void column_solve(int M, const ColumnWork& w, int lane, int nlanes, Sync sync)
{
    for (int p = 0; p + 1 < M; ++p) {
        const double bp = w.b[p];
        for (int i = p + 1 + lane; i < M; i += nlanes) w.b[i] -= w.tri[column_tri(i, p)] * bp;
        sync();
    }
    for (int i = lane; i < M; i += nlanes) w.b[i] = w.b[i] / w.d[i];
    sync();
    if (lane == 0)
        for (int i = M - 2; i >= 0; --i) {
            double s = w.b[i];
            for (int p = i + 1; p < M; ++p) s -= w.tri[column_tri(p, i)] * w.b[p];
            w.b[i] = s;
        }
    sync();
}

// the clipped step and the stepped value, fp32, dsa_model_update's order of operations and comparisons
DSA_CS float column_clip(double delta, float dvmax)
{
    float s = (float)delta;
    if (s >= dvmax) s = dvmax;
    if (s <= -dvmax) s = -dvmax;
    return s;
}

DSA_CS float column_stepped(float v, float s, float minvel, float maxvel)
{
    v = v + s;
    if (v < minvel) v = minvel;
    if (v > maxvel) v = maxvel;
    return v;
}

// factor, solve, apply on an assembled system (w.tri, w.b): the column's M values vels[l * v_stride] are stepped in place and dv[l *
// dv_stride] gets the clipped steps -- or, where the factorisation stops, the values stay and dv gets zeros.  dv may be null.  Returns the flag.
template <class Sync>
DSA_CS int column_finish(int M, const ColumnWork& w, float dvmax, float minvel, float maxvel, float* vels, long long v_stride, float* dv,
                         long long dv_stride, int lane, int nlanes, Sync sync)
{
    const int flag = column_factor(M, w, lane, nlanes, sync);
    if (flag == kColumnOk) column_solve(M, w, lane, nlanes, sync);
    for (int l = lane; l < M; l += nlanes) {
        const float s = flag == kColumnOk ? column_clip(w.b[l], dvmax) : 0.0f;
        if (dv) dv[l * dv_stride] = s;
        if (flag == kColumnOk) vels[l * v_stride] = column_stepped(vels[l * v_stride], s, minvel, maxvel);
    }
    return flag;
}

// the whole step of one column.  A column without a used datum is left alone (kColumnNoData, chi2 = 0, dv = 0) whatever damp is.
template <class Sync>
DSA_CS int column_step(const ColumnIn& in, float smooth, float damp, float dvmax, float minvel, float maxvel, const ColumnWork& w, float* vels,
                       long long v_stride, float* dv, long long dv_stride, int* nused, double* chi2, int lane, int nlanes, Sync sync)
{
    const double lambda2 = (double)smooth * (double)smooth, mu2 = (double)damp * (double)damp;
    *nused = column_assemble(in, lambda2, mu2, w, chi2, lane, nlanes, sync);
    if (*nused == 0) {
        if (dv) for (int l = lane; l < in.M; l += nlanes) dv[l * dv_stride] = 0.0f;
        return kColumnNoData;
    }
    return column_finish(in.M, w, dvmax, minvel, maxvel, vels, v_stride, dv, dv_stride, lane, nlanes, sync);
}

}  // namespace dsa
