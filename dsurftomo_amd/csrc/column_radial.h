// The radially anisotropic depth step of one column of the period maps: column_system.h's step with two models on one
// set of depths, Vsv seen by the Rayleigh data and Vsh seen by the Love data, tied by a penalty on the change of their difference.
// 2M unknowns x = [dVsv_0 .. dVsv_M-1 ; dVsh_0 .. dVsh_M-1], M = nz - 1 (the bottom depth of both models is kept), K data in slot order;
// slot k is a Love slot iff bit k of the mask `love` is set.
//
//   used     column_system.h's rule; a_k, rho_k as there
//   data     g_kl = a_k S_kl with S_kl = d c_k / d Vsv_l (k_sen_combine's rule on the Vsv model) at a Rayleigh slot, d c_k / d Vsh_l (the rule
//            on the Vsh model) at a Love slot -- one compact K x M array: a Rayleigh datum touches only the Vsv block, a Love datum only the
//            Vsh block (the cross sensitivities are neglected)
//   minimise |G x - rho|^2 + smooth^2 (|L x_v|^2 + |L x_h|^2) + damp^2 |x|^2 + aniso^2 |(v_h + x_h) - (v_v + x_v)|^2
//   N        packed lower triangle of size 2M, the Vsv block first.  Inside a block: the sum over that block's used k ascending of g_kl g_kl'
//            from 0.0, + smooth^2 (double)column_ltl(M, l, l'), on the diagonal + damp^2, then + aniso^2.  Row in the Vsh block, column in the
//            Vsv block: 0.0 - aniso^2 where l = l', else 0.0
//   b        d_l = (double)vsh_l - (double)vsv_l; Vsv block: sum_k g_kl rho_k over its used k, then + aniso^2 d_l; Vsh block: its sum, then
//            - aniso^2 d_l (one product and one sum each)
//   chi2, nused   per wave type (0 Rayleigh, 1 Love), over the used k ascending
//   factor, solve, clip, step   column_factor / column_solve on 2M, column_clip / column_stepped on both models
//   flags    1: a pivot that is not finite or <= 0; 2: no datum of either type used, whatever damp and aniso are.  Both leave the column alone
//            and dv zero.  One wave type without a used datum still steps: its block is held by the regulariser and the tie.
//
// At aniso = 0 every cross term is +0.0 and every added term 0.0, so each block's step has the bits of column_step on that block's data.
// fp64 under -ffp-contract=off, functions of (lane, nlanes, sync), every figure one sequential chain of its own: column_system.h's contract.
#pragma once

#include "column_system.h"

namespace dsa {

constexpr int kRadialMaxUnknowns = 2 * kColumnMaxM;        // 126

// one column's inputs where they lie: obs / wt / pv as ColumnIn's; Sv / Sh: the combined sensitivities on the Vsv and on the Vsh model, element
// (l, k) of either at l * s_lstride + k * s_kstride -- Sv is read at the used Rayleigh slots only, Sh at the used Love slots only
struct RadialIn {
    int M, K;
    unsigned long long love;
    const float* obs; long long obs_stride;
    const float* wt; long long wt_stride;
    const double* pv; long long pv_stride;
    const double* Sv; const double* Sh; long long s_lstride, s_kstride;
};

// the work arrays: ColumnWork's with tri, b, v and d sized for 2M unknowns and G compact (K x M)
DSA_CS size_t radial_work_doubles(int M, int K) { return (size_t)column_tri_size(2 * M) + (size_t)K * M + 2 * (size_t)K + 6 * (size_t)M; }

DSA_CS ColumnWork radial_work(double* base, int M, int K)
{
    ColumnWork w;
    w.tri = base; base += column_tri_size(2 * M);
    w.G = base; base += (size_t)K * M;
    w.a = base; base += K;
    w.rho = base; base += K;
    w.b = base; base += 2 * M;
    w.v = base; base += 2 * M;
    w.d = base;
    return w;
}

DSA_CS bool radial_is_love(unsigned long long love, int k) { return ((love >> k) & 1ull) != 0ull; }

// w.tri = N, w.b = b.  nused[2] and chi2[2]: Rayleigh, Love.  vsv / vsh: the column's M values of the two models at l * v_stride.  Every lane
// gets the same nused and chi2.
template <class Sync>
DSA_CS void radial_assemble(const RadialIn& in, double lambda2, double mu2, double gamma2, const float* vsv, const float* vsh, long long v_stride,
                            const ColumnWork& w, int* nused, double* chi2, int lane, int nlanes, Sync sync)
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
        const double* S = radial_is_love(in.love, k) ? in.Sh : in.Sv;
        w.G[e] = w.a[k] > 0.0 ? w.a[k] * S[l * in.s_lstride + k * in.s_kstride] : 0.0;
    }
    sync();
    for (int e = lane; e < column_tri_size(2 * M); e += nlanes) {
        const int i = column_tri_row(e), j = e - column_tri(i, 0);
        double s = 0.0;
        if (i >= M && j < M) {
            if (i - M == j) s = s - gamma2;
        } else {
            const bool lv = i >= M;
            const int l = lv ? i - M : i, lp = lv ? j - M : j;
            for (int k = 0; k < K; ++k)
                if (w.a[k] > 0.0 && radial_is_love(in.love, k) == lv) s += w.G[k * M + l] * w.G[k * M + lp];
            s = s + lambda2 * (double)column_ltl(M, l, lp);
            if (l == lp) { s = s + mu2; s = s + gamma2; }
        }
        w.tri[e] = s;
    }
    for (int i = lane; i < 2 * M; i += nlanes) {
        const bool lv = i >= M;
        const int l = lv ? i - M : i;
        double s = 0.0;
        for (int k = 0; k < K; ++k)
            if (w.a[k] > 0.0 && radial_is_love(in.love, k) == lv) s += w.G[k * M + l] * w.rho[k];
        const double d = (double)vsh[l * v_stride] - (double)vsv[l * v_stride];
        const double t = gamma2 * d;
        w.b[i] = lv ? s - t : s + t;
    }
    int nr = 0, nl = 0;
    double cr = 0.0, cl = 0.0;
    for (int k = 0; k < K; ++k)
        if (w.a[k] > 0.0) {
            if (radial_is_love(in.love, k)) { ++nl; cl += w.rho[k] * w.rho[k]; }
            else { ++nr; cr += w.rho[k] * w.rho[k]; }
        }
    nused[0] = nr; nused[1] = nl;
    chi2[0] = cr; chi2[1] = cl;
    sync();
}

// factor, solve, apply on an assembled system of 2M unknowns: both models are stepped in place, dv_v / dv_h (null, or M values at l *
// dv_stride) get the clipped steps -- or, where the factorisation stops, the models stay and the steps are zeros.  Returns the flag.
template <class Sync>
DSA_CS int radial_finish(int M, const ColumnWork& w, float dvmax, float minvel, float maxvel, float* vsv, float* vsh, long long v_stride, float* dv_v,
                         float* dv_h, long long dv_stride, int lane, int nlanes, Sync sync)
{
    const int flag = column_factor(2 * M, w, lane, nlanes, sync);
    if (flag == kColumnOk) column_solve(2 * M, w, lane, nlanes, sync);
    for (int i = lane; i < 2 * M; i += nlanes) {
        const bool lv = i >= M;
        const int l = lv ? i - M : i;
        float* vel = lv ? vsh : vsv;
        float* dv = lv ? dv_h : dv_v;
        const float s = flag == kColumnOk ? column_clip(w.b[i], dvmax) : 0.0f;
        if (dv) dv[l * dv_stride] = s;
        if (flag == kColumnOk) vel[l * v_stride] = column_stepped(vel[l * v_stride], s, minvel, maxvel);
    }
    return flag;
}

// the whole step of one column
template <class Sync>
DSA_CS int radial_step(const RadialIn& in, float smooth, float damp, float aniso, float dvmax, float minvel, float maxvel, const ColumnWork& w, float* vsv,
                       float* vsh, long long v_stride, float* dv_v, float* dv_h, long long dv_stride, int* nused, double* chi2, int lane, int nlanes, Sync sync)
{
    const double lambda2 = (double)smooth * (double)smooth, mu2 = (double)damp * (double)damp, gamma2 = (double)aniso * (double)aniso;
    radial_assemble(in, lambda2, mu2, gamma2, vsv, vsh, v_stride, w, nused, chi2, lane, nlanes, sync);
    if (nused[0] + nused[1] == 0) {
        for (int l = lane; l < in.M; l += nlanes) {
            if (dv_v) dv_v[l * dv_stride] = 0.0f;
            if (dv_h) dv_h[l * dv_stride] = 0.0f;
        }
        return kColumnNoData;
    }
    return radial_finish(in.M, w, dvmax, minvel, maxvel, vsv, vsh, v_stride, dv_v, dv_h, dv_stride, lane, nlanes, sync);
}

}  // namespace dsa
