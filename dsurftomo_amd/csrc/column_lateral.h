// The laterally coupled depth step of the period maps: column_system.h's step of every interior column, with a penalty
// on the difference of the stepped model between neighbouring columns, solved by preconditioned conjugate gradients whose preconditioner is
// the columns' own factored normal matrices.  column_system.h is included as it is: M = nz - 1, K, the used data, a_k, rho_k, g_kl,
// N_c = G^T G + smooth^2 L^T L + damp^2 I and b_c = G^T rho are its figures, bit for bit.
//
//   columns   interior column b = bj nvx + bi (nvx = nx - 2, nvy = ny - 2) is column c = (bj + 1) nx + bi + 1 of the (nz, ny, nx) model
//   active    a column whose column_factor succeeds; with lateral = 0 a column without a used datum is not active (flag 2), with
//             lateral > 0 it is (N_c the regulariser alone, b_c = 0, nused 0, flag 0).  A failed pivot is flag 1: not active
//   edges     lateral > 0 only: between active columns at b - 1, b + 1, b - nvx, b + nvx inside the interior, visited in that order; the
//             outer ring is never a neighbour.  deg_c: the number of c's edges.  lam2 = (double)lateral * (double)lateral
//   minimise  sum_c [ |G_c x_c - rho_c|^2 + smooth^2 |L x_c|^2 + damp^2 |x_c|^2 ] + lateral^2 sum_edges |(v_c + x_c) - (v_c' + x_c')|^2
//   bt        bt_c[l] = b_c[l] - lam2 s, s = the sum over c's edges in their order, from 0.0, of ((double)v_c[l] - (double)v_c'[l])
//   A y       q_c[l] = t + lam2 ((double)deg_c y_c[l] - s): t = sum_j N_c[l][j] y_c[j], j ascending from 0.0; s = the sum over the edges of
//             y_c'[l] from 0.0
//   M^-1      column_solve with the column's factor, on a copy of the right-hand side
//   dots      per column sum_l u[l] w[l], l ascending from 0.0 (0.0 for a column that is not active); a global sum is 64 chains -- chain t
//             adds the columns' figures with b = t, t + 64, ... ascending from 0.0 -- added with t ascending from 0.0
//   PCG       x = M^-1 bt; rz0 = bt^T x; thr = tol^2 rz0; r = bt - A x; z = M^-1 r; rz = r^T z; p_old = 0, beta = 0; itn = 0.
//             The criterion rz <= thr is looked at now (istop 1) and after every iteration; lateral = 0 stops here whatever rz is.
//             iteration: p = z + beta p_old; q = A p; alpha = rz / p^T q; x = x + alpha p; r = r - alpha q; z = M^-1 r;
//                        beta = r^T z / rz; rz = r^T z; itn = itn + 1; rz <= thr: istop 1, else itn >= maxit: istop 2
//   apply     column_clip and column_stepped on x of every active column; the others keep their values and report dv = 0
//
// The directions are kept twice (p of the even and of the odd iterations): a column computes its neighbours' new p from their z and old p
// itself, by the expression they use, so that no column waits for another.  The scalars, the iteration count and the done flag lie with
// the vectors; every per-iteration function returns at once when done is set, so x is frozen from the iteration that met the criterion,
// however many more are started.
//
// The phases of the loop -- the store-and-factor tail of the set-up, residual, direction, update -- are written once, over a system `sys`
// that supplies lateral_view(sys), its LateralWs, and lateral_operator(sys, ...), its A y: this header's own system is the LateralWs itself;
// column_radial_lateral.h adds one of 2M unknowns per column.  The operators stay two functions: their floating-point chains differ.  fp64 under -ffp-contract=off, functions of (lane, nlanes, sync), every figure one sequential chain from
// 0.0 in the stated order: column_system.h's contract.
#pragma once

#include "column_system.h"

namespace dsa {

constexpr int kLateralChains = 64;

enum { kLatRz = 0, kLatRz0, kLatThr, kLatAlpha, kLatBeta, kLatScalars = 8 };          // the doubles
enum { kLatItn = 0, kLatDone, kLatStop, kLatInts = 4 };                               // the ints
enum { kLatSumRz0 = 0, kLatSumFirst, kLatSumPq, kLatSumRz };                          // what a global sum is for

// the workspace: per interior column N, the factor (column_factor's triangle), and eight vectors; one figure per column for the dots; the
// scalars; one flag per column
DSA_CS size_t lateral_column_doubles(int M) { return 2 * (size_t)column_tri_size(M) + 8 * (size_t)M; }

DSA_CS size_t lateral_ws_doubles(int nvx, int nvy, int M)
{
    const size_t n = (size_t)nvx * nvy;
    return n * lateral_column_doubles(M) + n + kLatScalars + (n + kLatInts + 1) / 2;
}

struct LateralWs {
    int nvx, nvy, M, edges;
    double lam2;
    double* cols;
    double* part;
    double* sc;
    int* ic;
    int* active;
};

// edges: whether the columns are coupled at all (this system: lateral > 0)
DSA_CS LateralWs lateral_ws(double* base, int nvx, int nvy, int M, float lateral, bool edges)
{
    const size_t n = (size_t)nvx * nvy;
    LateralWs ws;
    ws.nvx = nvx; ws.nvy = nvy; ws.M = M;
    ws.edges = edges ? 1 : 0;
    ws.lam2 = (double)lateral * (double)lateral;
    ws.cols = base; base += n * lateral_column_doubles(M);
    ws.part = base; base += n;
    ws.sc = base; base += kLatScalars;
    ws.ic = reinterpret_cast<int*>(base);
    ws.active = ws.ic + kLatInts;
    return ws;
}

DSA_CS LateralWs lateral_ws(double* base, int nvx, int nvy, int M, float lateral) { return lateral_ws(base, nvx, nvy, M, lateral, lateral > 0.0f); }

DSA_CS const LateralWs& lateral_view(const LateralWs& ws) { return ws; }

struct LateralColumn { double *N, *F, *d, *b, *x, *r, *z, *q, *p0, *p1; };

DSA_CS LateralColumn lateral_column(const LateralWs& ws, int b)
{
    double* base = ws.cols + (size_t)b * lateral_column_doubles(ws.M);
    const int T = column_tri_size(ws.M), M = ws.M;
    LateralColumn c;
    c.N = base; c.F = base + T; base += 2 * (size_t)T;
    c.d = base; c.b = base + M; c.x = base + 2 * M; c.r = base + 3 * M; c.z = base + 4 * M; c.q = base + 5 * M; c.p0 = base + 6 * M; c.p1 = base + 7 * M;
    return c;
}

DSA_CS double* lateral_p(const LateralColumn& c, int which) { return which ? c.p1 : c.p0; }

// the column of the model that interior column b is
DSA_CS long long lateral_model_column(const LateralWs& ws, int b)
{
    const int bj = b / ws.nvx, bi = b - bj * ws.nvx;
    return (long long)(bj + 1) * (ws.nvx + 2) + (bi + 1);
}

// edge e = 0 .. 3 of column b (-1, +1, -nvx, +nvx): the neighbour, or -1 where there is no edge
DSA_CS int lateral_neighbour(const LateralWs& ws, int b, int e)
{
    if (!ws.edges) return -1;
    const int bj = b / ws.nvx, bi = b - bj * ws.nvx;
    int nb = -1;
    if (e == 0) { if (bi > 0) nb = b - 1; }
    else if (e == 1) { if (bi + 1 < ws.nvx) nb = b + 1; }
    else if (e == 2) { if (bj > 0) nb = b - ws.nvx; }
    else { if (bj + 1 < ws.nvy) nb = b + ws.nvx; }
    if (nb >= 0 && !ws.active[nb]) nb = -1;
    return nb;
}

// dst = M^-1 src: column_solve with the column's factor on a copy of src
template <class Sync>
DSA_CS void lateral_precondition(int M, const LateralColumn& c, const double* src, double* dst, int lane, int nlanes, Sync sync)
{
    for (int l = lane; l < M; l += nlanes) dst[l] = src[l];
    sync();
    ColumnWork g;
    g.tri = c.F; g.d = c.d; g.b = dst; g.G = nullptr; g.a = nullptr; g.rho = nullptr; g.v = nullptr;
    column_solve(M, g, lane, nlanes, sync);
}

// the column's figure of a dot product, the same on every lane
DSA_CS double lateral_dot(int M, const double* u, const double* w)
{
    double s = 0.0;
    for (int l = 0; l < M; ++l) s += u[l] * w[l];
    return s;
}

// element l of the vector the operator is applied to, at a neighbour: its x (what = 0), or its new direction z + beta p_old
DSA_CS double lateral_operand(const LateralColumn& c, int l, int what, double beta, int pold)
{
    return what == 0 ? c.x[l] : c.z[l] + beta * lateral_p(c, pold)[l];
}

// c.q = (A y)_c, y_c = own
DSA_CS void lateral_operator(const LateralWs& ws, int b, const LateralColumn& c, const double* own, int what, double beta, int pold, int lane, int nlanes)
{
    const int M = ws.M;
    for (int l = lane; l < M; l += nlanes) {
        double t = 0.0;
        for (int j = 0; j < M; ++j) t += c.N[j <= l ? column_tri(l, j) : column_tri(j, l)] * own[j];
        double s = 0.0;
        int deg = 0;
        for (int e = 0; e < 4; ++e) {
            const int nb = lateral_neighbour(ws, b, e);
            if (nb >= 0) { ++deg; s += lateral_operand(lateral_column(ws, nb), l, what, beta, pold); }
        }
        c.q[l] = t + ws.lam2 * ((double)deg * own[l] - s);
    }
}

// The tail of a set-up of column b, after the system's assembly in the work arrays w (nused: the column's used data, all kinds): N (copied
// before the factorisation overwrites it) and b_c to the workspace, column_factor of ws.M unknowns, the factor to the workspace, the
// column's active flag.  Returns the column's flag.  Every lane returns the same.
template <class Sync>
DSA_CS int lateral_store_factor(const LateralWs& ws, int b, const ColumnWork& w, int nused, int lane, int nlanes, Sync sync)
{
    if (nused == 0 && !ws.edges) {
        if (lane == 0) ws.active[b] = 0;
        return kColumnNoData;
    }
    const int M = ws.M, T = column_tri_size(M);
    const LateralColumn c = lateral_column(ws, b);
    for (int e = lane; e < T; e += nlanes) c.N[e] = w.tri[e];
    for (int l = lane; l < M; l += nlanes) c.b[l] = w.b[l];
    sync();
    const int flag = column_factor(M, w, lane, nlanes, sync);
    if (flag == kColumnOk) {
        for (int e = lane; e < T; e += nlanes) c.F[e] = w.tri[e];
        for (int l = lane; l < M; l += nlanes) c.d[l] = w.d[l];
    }
    if (lane == 0) ws.active[b] = flag == kColumnOk ? 1 : 0;
    return flag;
}

// Set-up of column b: assemble in the work arrays w (column_work), then lateral_store_factor.  Returns the column's flag; *nused and *chi2
// are column_assemble's.  Every lane returns the same.
template <class Sync>
DSA_CS int lateral_setup(const ColumnIn& in, float smooth, float damp, const ColumnWork& w, const LateralWs& ws, int b, int* nused, double* chi2, int lane,
                         int nlanes, Sync sync)
{
    const double lambda2 = (double)smooth * (double)smooth, mu2 = (double)damp * (double)damp;
    *nused = column_assemble(in, lambda2, mu2, w, chi2, lane, nlanes, sync);
    return lateral_store_factor(ws, b, w, *nused, lane, nlanes, sync);
}

// bt_c in place of b_c, x_c = M^-1 bt_c, p_old = 0, the column's figure of bt^T x.  vels: the model, element l of column c at l * v_stride + c.
template <class Sync>
DSA_CS void lateral_start(const LateralWs& ws, int b, const float* vels, long long v_stride, int lane, int nlanes, Sync sync)
{
    if (!ws.active[b]) {
        if (lane == 0) ws.part[b] = 0.0;
        return;
    }
    const int M = ws.M;
    const LateralColumn c = lateral_column(ws, b);
    const float* v = vels + lateral_model_column(ws, b);
    for (int l = lane; l < M; l += nlanes) {
        double s = 0.0;
        for (int e = 0; e < 4; ++e) {
            const int nb = lateral_neighbour(ws, b, e);
            if (nb >= 0) s += (double)v[l * v_stride] - (double)vels[l * v_stride + lateral_model_column(ws, nb)];
        }
        if (ws.edges) c.b[l] = c.b[l] - ws.lam2 * s;
        c.p0[l] = 0.0;
        c.p1[l] = 0.0;
    }
    sync();
    lateral_precondition(M, c, c.b, c.x, lane, nlanes, sync);
    if (lane == 0) ws.part[b] = lateral_dot(M, c.b, c.x);
}

// r = bt - A x, z = M^-1 r, the column's figure of r^T z
template <class Sys, class Sync>
DSA_CS void lateral_residual(const Sys& sys, int b, int lane, int nlanes, Sync sync)
{
    const LateralWs& ws = lateral_view(sys);
    if (!ws.active[b]) {
        if (lane == 0) ws.part[b] = 0.0;
        return;
    }
    const int M = ws.M;
    const LateralColumn c = lateral_column(ws, b);
    lateral_operator(sys, b, c, c.x, 0, 0.0, 0, lane, nlanes);
    sync();
    for (int l = lane; l < M; l += nlanes) c.r[l] = c.b[l] - c.q[l];
    sync();
    lateral_precondition(M, c, c.r, c.z, lane, nlanes, sync);
    if (lane == 0) ws.part[b] = lateral_dot(M, c.r, c.z);
}

// first half of an iteration: p = z + beta p_old (kept beside p_old), q = A p, the column's figure of p^T q
template <class Sys, class Sync>
DSA_CS void lateral_direction(const Sys& sys, int b, int lane, int nlanes, Sync sync)
{
    const LateralWs& ws = lateral_view(sys);
    if (ws.ic[kLatDone]) return;
    if (!ws.active[b]) {
        if (lane == 0) ws.part[b] = 0.0;
        return;
    }
    const int M = ws.M, pold = ws.ic[kLatItn] & 1;
    const double beta = ws.sc[kLatBeta];
    const LateralColumn c = lateral_column(ws, b);
    double* p = lateral_p(c, 1 - pold);
    for (int l = lane; l < M; l += nlanes) p[l] = lateral_operand(c, l, 1, beta, pold);
    sync();
    lateral_operator(sys, b, c, p, 1, beta, pold, lane, nlanes);
    sync();
    if (lane == 0) ws.part[b] = lateral_dot(M, p, c.q);
}

// second half, the same for every system: x = x + alpha p, r = r - alpha q, z = M^-1 r, the column's figure of r^T z
template <class Sync>
DSA_CS void lateral_update(const LateralWs& ws, int b, int lane, int nlanes, Sync sync)
{
    if (ws.ic[kLatDone]) return;
    if (!ws.active[b]) {
        if (lane == 0) ws.part[b] = 0.0;
        return;
    }
    const int M = ws.M;
    const double alpha = ws.sc[kLatAlpha];
    const LateralColumn c = lateral_column(ws, b);
    const double* p = lateral_p(c, 1 - (ws.ic[kLatItn] & 1));
    for (int l = lane; l < M; l += nlanes) {
        c.x[l] = c.x[l] + alpha * p[l];
        c.r[l] = c.r[l] - alpha * c.q[l];
    }
    sync();
    lateral_precondition(M, c, c.r, c.z, lane, nlanes, sync);
    if (lane == 0) ws.part[b] = lateral_dot(M, c.r, c.z);
}

// the global sum of the columns' figures in its fixed shape; chains: kLateralChains doubles that every lane sees.  Every lane returns the same.
template <class Sync>
DSA_CS double lateral_sum(const LateralWs& ws, double* chains, int lane, int nlanes, Sync sync)
{
    const int n = ws.nvx * ws.nvy;
    for (int t = lane; t < kLateralChains; t += nlanes) {
        double s = 0.0;
        for (int b = t; b < n; b += kLateralChains) s += ws.part[b];
        chains[t] = s;
    }
    sync();
    double s = 0.0;
    for (int t = 0; t < kLateralChains; ++t) s += chains[t];
    sync();
    return s;
}

// what one lane does with a global sum: the scalars of the iteration, the count, the criterion
DSA_CS void lateral_scalars(const LateralWs& ws, int what, double sum, double tol, int maxit)
{
    if (what == kLatSumRz0) {
        ws.sc[kLatRz0] = sum;
        ws.sc[kLatThr] = (tol * tol) * sum;
        ws.sc[kLatAlpha] = 0.0;
        ws.sc[kLatBeta] = 0.0;
        ws.ic[kLatItn] = 0; ws.ic[kLatDone] = 0; ws.ic[kLatStop] = 0;
    } else if (what == kLatSumFirst) {
        ws.sc[kLatRz] = sum;
        if (!ws.edges || sum <= ws.sc[kLatThr]) { ws.ic[kLatDone] = 1; ws.ic[kLatStop] = 1; }
    } else if (what == kLatSumPq) {
        ws.sc[kLatAlpha] = ws.sc[kLatRz] / sum;
    } else {
        ws.sc[kLatBeta] = sum / ws.sc[kLatRz];
        ws.sc[kLatRz] = sum;
        const int itn = ws.ic[kLatItn] + 1;
        ws.ic[kLatItn] = itn;
        if (sum <= ws.sc[kLatThr]) { ws.ic[kLatDone] = 1; ws.ic[kLatStop] = 1; }
        else if (itn >= maxit) { ws.ic[kLatDone] = 1; ws.ic[kLatStop] = 2; }
    }
}

// a global sum and what follows from it.  The sums of an iteration are not taken once done is set.
template <class Sync>
DSA_CS void lateral_reduce(const LateralWs& ws, int what, double tol, int maxit, double* chains, int lane, int nlanes, Sync sync)
{
    if ((what == kLatSumPq || what == kLatSumRz) && ws.ic[kLatDone]) return;
    const double s = lateral_sum(ws, chains, lane, nlanes, sync);
    if (lane == 0) lateral_scalars(ws, what, s, tol, maxit);
}

// the clipped step of column b and its stepped values; a column that is not active keeps its values and reports zeros.  The ws.M unknowns
// are one block of the model vels0 (Mb = ws.M), or two blocks of Mb = ws.M / 2 rows: vels0's, then vels1's.  dv0 / dv1: null, or the blocks'
// steps, element l of column c at l * dv_stride + c.
DSA_CS void lateral_finish_blocks(const LateralWs& ws, int b, int Mb, float dvmax, float minvel, float maxvel, float* vels0, float* vels1, long long v_stride,
                                  float* dv0, float* dv1, long long dv_stride, int lane, int nlanes)
{
    const long long col = lateral_model_column(ws, b);
    const bool on = ws.active[b] != 0;
    const LateralColumn c = lateral_column(ws, b);
    for (int i = lane; i < ws.M; i += nlanes) {
        const bool second = i >= Mb;
        const int l = second ? i - Mb : i;
        float* vel = second ? vels1 : vels0;
        float* dv = second ? dv1 : dv0;
        const float s = on ? column_clip(c.x[i], dvmax) : 0.0f;
        if (dv) dv[l * dv_stride + col] = s;
        if (on) vel[l * v_stride + col] = column_stepped(vel[l * v_stride + col], s, minvel, maxvel);
    }
}

// this system's finish: one block.  dv may be null.
DSA_CS void lateral_finish(const LateralWs& ws, int b, float dvmax, float minvel, float maxvel, float* vels, long long v_stride, float* dv, long long dv_stride,
                           int lane, int nlanes)
{
    lateral_finish_blocks(ws, b, ws.M, dvmax, minvel, maxvel, vels, nullptr, v_stride, dv, nullptr, dv_stride, lane, nlanes);
}

// info (4 doubles): itn, istop, rz0, the last rz
DSA_CS void lateral_info(const LateralWs& ws, double* info)
{
    info[0] = (double)ws.ic[kLatItn]; info[1] = (double)ws.ic[kLatStop]; info[2] = ws.sc[kLatRz0]; info[3] = ws.sc[kLatRz];
}

}  // namespace dsa
