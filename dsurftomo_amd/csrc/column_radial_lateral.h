// The laterally coupled radial depth step of the period maps: column_radial.h's step of every interior column -- the
// unknowns x_c = [dVsv_0 .. dVsv_M-1 ; dVsh_0 .. dVsh_M-1], B = 2M of them -- with column_lateral.h's penalty on the difference of each stepped
// model between neighbouring columns and a second penalty on the difference of the stepped anisotropy field Vsh - Vsv, solved by
// column_lateral.h's preconditioned conjugate gradients.  column_system.h, column_radial.h and column_lateral.h are included as they are:
// N_c, b_c, nused and chi2 per wave type are radial_assemble's figures (the tie aniso of the column's own two models among them), bit for bit;
// the workspace is column_lateral.h's with M := B, lateral_ws_doubles(nvx, nvy, 2M) doubles; the column index b, lateral_model_column, the edge
// order (b - 1, b + 1, b - nvx, b + nvx) and the ring rule are column_lateral.h's.
//
//   edges     exist iff lateral > 0 or lateral_aniso > 0; w2 = (double)lateral * (double)lateral, wa2 = (double)lateral_aniso * (double)lateral_aniso
//   active    a column whose column_factor(2M) succeeds; with edges a column without a used datum of either type is active too (nused 0, 0,
//             flag 0: N_c the regulariser, damp and tie alone, b_c the tie's; no kernel of an unused datum is read), without edges it is flag 2
//             as in column_radial.h.  A failed pivot is flag 1: not active, left alone, no edge touches it
//   minimise  sum_c [column_radial.h's objective of c]
//             + w2 sum_edges [ |(vsv_c + xv_c) - (vsv_c' + xv_c')|^2 + |(vsh_c + xh_c) - (vsh_c' + xh_c')|^2 ]
//             + wa2 sum_edges |(a_c + u_c) - (a_c' + u_c')|^2,   a = vsh - vsv of the models as they are, u = xh - xv
//   bt        per depth l, every edge sum from 0.0 in edge order:
//               s_v = sum (double)vsv_c[l] - (double)vsv_c'[l];  s_h the same on vsh;
//               s_a = sum ((double)vsh_c[l] - (double)vsv_c[l]) - ((double)vsh_c'[l] - (double)vsv_c'[l])
//               bt_v[l] = (b_v[l] - w2 s_v) + wa2 s_a;   bt_h[l] = (b_h[l] - w2 s_h) - wa2 s_a          (b_c as it is where there are no edges)
//   A y       row i of the B-vector: f = t + w2 ((double)deg y_c[i] - s) -- column_lateral.h's figure: t = sum_j N_c[i][j] y_c[j], j ascending from
//             0.0; s = the edge sum of y_c'[i] from 0.0 -- then, with l the depth of row i, u = y_c[M + l] - y_c[l], su = the edge sum from 0.0
//             of (y_c'[M + l] - y_c'[l]) and g = wa2 ((double)deg u - su):  q_c[i] = f - g in the Vsv block, f + g in the Vsh block
//   M^-1, dots, PCG   column_lateral.h's, word for word: its phases lateral_store_factor, lateral_residual, lateral_direction and lateral_update
//             run on this system through lateral_view and the lateral_operator overload below, its lateral_sum, lateral_scalars,
//             lateral_reduce and lateral_info on the B-sized workspace; without edges the loop stops at itn 0 whatever rz is, and rz is the
//             residual of that direct solve
//   apply     lateral_finish_blocks over two blocks of rows: column_clip and column_stepped on both blocks of x of every active column; the others
//             keep their values and report dv = 0
//
// A neighbour's operand during an iteration is its new direction z + beta p_old, computed here by the neighbour's own expression
// (lateral_operand), so no column waits for another.  Without edges every output and both stepped models are radial_step's bit for bit.
// fp64 under -ffp-contract=off, functions of (lane, nlanes, sync), every figure one sequential chain from 0.0 in the stated order:
// column_system.h's contract.
#pragma once

#include "column_system.h"
#include "column_radial.h"
#include "column_lateral.h"

namespace dsa {

// the workspace of B = 2M unknowns per column, and the second weight
struct RadialLateralWs {
    LateralWs ws;          // ws.M = 2M, ws.lam2 = w2, ws.edges as above
    int M;
    double wa2;
};

DSA_CS size_t radial_lateral_ws_doubles(int nvx, int nvy, int M) { return lateral_ws_doubles(nvx, nvy, 2 * M); }

DSA_CS RadialLateralWs radial_lateral_ws(double* base, int nvx, int nvy, int M, float lateral, float lateral_aniso)
{
    RadialLateralWs rl;
    rl.ws = lateral_ws(base, nvx, nvy, 2 * M, lateral, lateral > 0.0f || lateral_aniso > 0.0f);
    rl.M = M;
    rl.wa2 = (double)lateral_aniso * (double)lateral_aniso;
    return rl;
}

DSA_CS const LateralWs& lateral_view(const RadialLateralWs& rl) { return rl.ws; }

// Set-up of column b: radial_assemble in the work arrays w (radial_work), then lateral_store_factor on the 2M unknowns.  vsv / vsh: the
// column's values at l * v_stride.  Returns the column's flag; nused[2] and chi2[2] are radial_assemble's.  Every lane returns the same.
template <class Sync>
DSA_CS int radial_lateral_setup(const RadialIn& in, float smooth, float damp, float aniso, const float* vsv, const float* vsh, long long v_stride,
                                const ColumnWork& w, const RadialLateralWs& rl, int b, int* nused, double* chi2, int lane, int nlanes, Sync sync)
{
    const double lambda2 = (double)smooth * (double)smooth, mu2 = (double)damp * (double)damp, gamma2 = (double)aniso * (double)aniso;
    radial_assemble(in, lambda2, mu2, gamma2, vsv, vsh, v_stride, w, nused, chi2, lane, nlanes, sync);
    return lateral_store_factor(rl.ws, b, w, nused[0] + nused[1], lane, nlanes, sync);
}

// bt_c in place of b_c, x_c = M^-1 bt_c, p_old = 0, the column's figure of bt^T x.  vsv / vsh: the models, element l of column c at l * v_stride + c.
template <class Sync>
DSA_CS void radial_lateral_start(const RadialLateralWs& rl, int b, const float* vsv, const float* vsh, long long v_stride, int lane, int nlanes, Sync sync)
{
    const LateralWs& ws = rl.ws;
    if (!ws.active[b]) {
        if (lane == 0) ws.part[b] = 0.0;
        return;
    }
    const int M = rl.M, B = ws.M;
    const LateralColumn c = lateral_column(ws, b);
    const long long col = lateral_model_column(ws, b);
    for (int i = lane; i < B; i += nlanes) {
        const bool lv = i >= M;
        const int l = lv ? i - M : i;
        const float* own = lv ? vsh : vsv;
        const long long at = l * v_stride;
        double s = 0.0, sa = 0.0;
        for (int e = 0; e < 4; ++e) {
            const int nb = lateral_neighbour(ws, b, e);
            if (nb >= 0) {
                const long long ncolm = lateral_model_column(ws, nb);
                s += (double)own[at + col] - (double)own[at + ncolm];
                sa += ((double)vsh[at + col] - (double)vsv[at + col]) - ((double)vsh[at + ncolm] - (double)vsv[at + ncolm]);
            }
        }
        if (ws.edges) {
            const double t = c.b[i] - ws.lam2 * s;
            c.b[i] = lv ? t - rl.wa2 * sa : t + rl.wa2 * sa;
        }
        c.p0[i] = 0.0;
        c.p1[i] = 0.0;
    }
    sync();
    lateral_precondition(B, c, c.b, c.x, lane, nlanes, sync);
    if (lane == 0) ws.part[b] = lateral_dot(B, c.b, c.x);
}

// The system's operator, under the name column_lateral.h's phases call: c.q = (A y)_c, y_c = own; what, beta, pold: lateral_operand's, for the
// neighbours.  Not column_lateral.h's operator with a second term: f - g and f + g are chains of their own.
DSA_CS void lateral_operator(const RadialLateralWs& rl, int b, const LateralColumn& c, const double* own, int what, double beta, int pold, int lane, int nlanes)
{
    const LateralWs& ws = rl.ws;
    const int M = rl.M, B = ws.M;
    for (int i = lane; i < B; i += nlanes) {
        const bool lv = i >= M;
        const int l = lv ? i - M : i;
        double t = 0.0;
        for (int j = 0; j < B; ++j) t += c.N[j <= i ? column_tri(i, j) : column_tri(j, i)] * own[j];
        double s = 0.0, su = 0.0;
        int deg = 0;
        for (int e = 0; e < 4; ++e) {
            const int nb = lateral_neighbour(ws, b, e);
            if (nb >= 0) {
                const LateralColumn n = lateral_column(ws, nb);
                ++deg;
                s += lateral_operand(n, i, what, beta, pold);
                su += lateral_operand(n, M + l, what, beta, pold) - lateral_operand(n, l, what, beta, pold);
            }
        }
        const double f = t + ws.lam2 * ((double)deg * own[i] - s);
        const double u = own[M + l] - own[l];
        const double g = rl.wa2 * ((double)deg * u - su);
        c.q[i] = lv ? f + g : f - g;
    }
}

// column_lateral.h's phases on this system, under the names the step's callers use: r = bt - A x, z = M^-1 r; the first half of an
// iteration (the second is lateral_update); the finish over both models.  dv_v / dv_h: null, or the blocks' steps.
template <class Sync>
DSA_CS void radial_lateral_residual(const RadialLateralWs& rl, int b, int lane, int nlanes, Sync sync) { lateral_residual(rl, b, lane, nlanes, sync); }

template <class Sync>
DSA_CS void radial_lateral_direction(const RadialLateralWs& rl, int b, int lane, int nlanes, Sync sync) { lateral_direction(rl, b, lane, nlanes, sync); }

DSA_CS void radial_lateral_finish(const RadialLateralWs& rl, int b, float dvmax, float minvel, float maxvel, float* vsv, float* vsh, long long v_stride, float* dv_v,
                                  float* dv_h, long long dv_stride, int lane, int nlanes)
{
    lateral_finish_blocks(rl.ws, b, rl.M, dvmax, minvel, maxvel, vsv, vsh, v_stride, dv_v, dv_h, dv_stride, lane, nlanes);
}

}  // namespace dsa
