// The depth resolution of the radially anisotropic column step: what the regularised normal matrix of
// column_radial.h's step says about its own answer -- section 22's figures carried to the 2M unknowns of section 23, with the leakage between
// the two models and the variance of their difference.  M = nz - 1.  Unknown i in [0, 2M): its block is 0 (Vsv) for i < M and 1 (Vsh) for
// i >= M, its depth index l(i) = i mod M.  Datum k has the type tau(k): 0 Rayleigh, 1 Love, by the mask `love`.  The used data, a_k and
// g_kl are radial_assemble's, N and its factor radial_assemble's and column_factor's on 2M, unchanged.  Row k of the expanded G^ is g_k in
// block tau(k) and 0.0 elsewhere.
//
//   T        K x 2M: row k solves N t = g^_k with column_solve's arithmetic exactly -- forward with p ascending, the division by d, back with
//            i descending and p ascending (column_resolution_solve_rhs, the one copy).  Rows of unused data are 0.0.  One lane per datum,
//            stored datum-fastest, T[i K + k], as section 22's.
//   R        = T^T G^: R_ij = sum_k T_ki g_{k,l(j)} over the used k with tau(k) = block(j), ascending, from 0.0.  Column j is the answer to a
//            spike in unknown j.
//   per j    six measures, with i ascending within each block: 0 R_jj; 1 m1_own = sum R_ij^2 over i in j's block; 2 m2_own = sum R_ij^2 dz^2,
//            dz = (double)depz[l(i)] - (double)depz[l(j)], in section 22's forms r2 = r r and r2 (dz dz); 3 m1_cross = sum R_ij^2 over i in the
//            other block, the energy a spike in j puts into the other model; 4 R_cross = R_{j~ j}, j~ the co-located unknown of the other
//            block; 5 var_j = sum_k T_kj T_kj over all used k ascending
//   per l    two pair measures over all used k ascending: 0 cov_l = sum_k T_{k,l} T_{k,M+l}; 1 vard_l = sum_k d d with d = T_{k,M+l} - T_{k,l},
//            the variance of dVsh - dVsv for unit variance of the weighted data
//   per k    the leverage h_k = sum_l g_kl T_{k, tau(k) M + l}, l ascending; 0.0 for an unused datum
//   column   trace[0] = sum R_jj over the Vsv block, trace[1] over the Vsh block, j ascending; nused[2] as the radial step's
//   flags    2: no datum of either type used, whatever damp and aniso are; 1: a pivot that is not finite or <= 0.  In both every output of the
//            column is 0.0.  One wave type without a used datum still resolves: its block's R_jj are 0.
//
// At aniso = 0 every cross term of N is +0.0 (column_radial.h), so every cross term of the factor and of T is a zero and every term they
// add to a chain is 0.0: measures 0, 1, 2 and 5 of the Vsv block and the Rayleigh leverages have the bits of column_resolution.h on the Vsv
// model with the Love data unused, those of the Vsh block and the Love leverages the bits of column_resolution.h on the Vsh model with the
// Rayleigh data unused; m1_cross, R_cross and cov are zeros, and vard_l = var_l + var_{M+l} up to the last rounding (it is a sum of d d,
// not of two sums).
//
// column_system.h's contract: __host__ __device__, fp64 under -ffp-contract=off, (lane, nlanes, sync), every figure one sequential chain of
// its own from 0.0 in a stated order, so the lane mapping -- and nlanes, which 2M = 126 makes worth choosing -- cannot change a bit.
#pragma once

#include "column_radial.h"
#include "column_resolution.h"

namespace dsa {

// doubles of work: column_radial.h's arrays, then T (2M x K)
DSA_CS size_t radial_resolution_doubles(int M, int K) { return radial_work_doubles(M, K) + 2 * (size_t)M * K; }

DSA_CS double* radial_resolution_t(double* base, int M, int K) { return base + radial_work_doubles(M, K); }

// where one column's outputs lie: measure q (0 .. 5) of unknown j at measures[q * m_qstride + j * m_jstride], pair measure q (0 cov, 1 vard)
// of depth l at pair[q * p_qstride + l * p_lstride], h_k at leverage[k * h_stride], R_ij at R[(i * 2M + j) * r_stride] (R may be null: the
// store is skipped, nothing else)
struct RadialResOut {
    double* measures; long long m_qstride, m_jstride;
    double* pair; long long p_qstride, p_lstride;
    double* leverage; long long h_stride;
    double* R; long long r_stride;
};

// element i of the right-hand side of datum k: g_k in the block of its type, 0.0 elsewhere
struct RadialRowOfG {
    const double* G; int M; unsigned long long love;
    DSA_CS_MEMBER double operator()(int k, int i) const
    {
        const bool lv = i >= M;
        return radial_is_love(love, k) == lv ? G[k * M + (lv ? i - M : i)] : 0.0;
    }
};

// the measures, the pair measures and the leverages from T and w.G; w.b gets the R_jj.  trace[2]: the same on every lane.
template <class Sync>
DSA_CS void radial_resolution_reduce(int M, int K, unsigned long long love, const float* depz, const ColumnWork& w, const double* T, const RadialResOut& out,
                                     double* trace, int lane, int nlanes, Sync sync)
{
    const int n = 2 * M;
    for (int j = lane; j < n; j += nlanes) {
        const bool jv = j >= M;
        const int lj = jv ? j - M : j, jt = jv ? j - M : j + M;
        double m1 = 0.0, m2 = 0.0, mx = 0.0, rjj = 0.0, rx = 0.0;
        for (int i = 0; i < n; ++i) {
            double r = 0.0;
            for (int k = 0; k < K; ++k)
                if (w.a[k] > 0.0 && radial_is_love(love, k) == jv) r += T[i * K + k] * w.G[k * M + lj];
            const double r2 = r * r;
            if ((i >= M) == jv) {
                m1 += r2;
                const double dz = (double)depz[i >= M ? i - M : i] - (double)depz[lj];
                m2 += r2 * (dz * dz);
            } else {
                mx += r2;
            }
            if (i == j) rjj = r;
            if (i == jt) rx = r;
            if (out.R) out.R[((long long)i * n + j) * out.r_stride] = r;
        }
        double var = 0.0;
        for (int k = 0; k < K; ++k)
            if (w.a[k] > 0.0) var += T[j * K + k] * T[j * K + k];
        out.measures[0 * out.m_qstride + j * out.m_jstride] = rjj;
        out.measures[1 * out.m_qstride + j * out.m_jstride] = m1;
        out.measures[2 * out.m_qstride + j * out.m_jstride] = m2;
        out.measures[3 * out.m_qstride + j * out.m_jstride] = mx;
        out.measures[4 * out.m_qstride + j * out.m_jstride] = rx;
        out.measures[5 * out.m_qstride + j * out.m_jstride] = var;
        w.b[j] = rjj;
    }
    for (int l = lane; l < M; l += nlanes) {
        double cov = 0.0, vard = 0.0;
        for (int k = 0; k < K; ++k)
            if (w.a[k] > 0.0) {
                const double tv = T[l * K + k], th = T[(M + l) * K + k];
                cov += tv * th;
                const double d = th - tv;
                vard += d * d;
            }
        out.pair[0 * out.p_qstride + l * out.p_lstride] = cov;
        out.pair[1 * out.p_qstride + l * out.p_lstride] = vard;
    }
    for (int k = lane; k < K; k += nlanes) {
        double h = 0.0;
        if (w.a[k] > 0.0) {
            const int first = radial_is_love(love, k) ? M : 0;
            for (int l = 0; l < M; ++l) h += w.G[k * M + l] * T[(first + l) * K + k];
        }
        out.leverage[k * out.h_stride] = h;
    }
    sync();
    double tv = 0.0, th = 0.0;
    for (int j = 0; j < M; ++j) tv += w.b[j];
    for (int j = M; j < n; ++j) th += w.b[j];
    trace[0] = tv; trace[1] = th;
}

// every output of one column 0.0
DSA_CS void radial_resolution_zero(int M, int K, const RadialResOut& out, double* trace, int lane, int nlanes)
{
    const int n = 2 * M;
    for (int j = lane; j < n; j += nlanes)
        for (int q = 0; q < 6; ++q) out.measures[q * out.m_qstride + j * out.m_jstride] = 0.0;
    for (int l = lane; l < M; l += nlanes)
        for (int q = 0; q < 2; ++q) out.pair[q * out.p_qstride + l * out.p_lstride] = 0.0;
    for (int k = lane; k < K; k += nlanes) out.leverage[k * out.h_stride] = 0.0;
    if (out.R)
        for (int e = lane; e < n * n; e += nlanes) out.R[(long long)e * out.r_stride] = 0.0;
    trace[0] = 0.0; trace[1] = 0.0;
}

// factor, T, reduce on an assembled system of 2M unknowns (w.tri, w.G, w.a): the flag; where the factorisation stops every output is 0.0
template <class Sync>
DSA_CS int radial_resolution_finish(int M, int K, unsigned long long love, const float* depz, const ColumnWork& w, double* T, const RadialResOut& out,
                                    double* trace, int lane, int nlanes, Sync sync)
{
    const int flag = column_factor(2 * M, w, lane, nlanes, sync);
    if (flag != kColumnOk) {
        radial_resolution_zero(M, K, out, trace, lane, nlanes);
        return flag;
    }
    RadialRowOfG rhs;
    rhs.G = w.G; rhs.M = M; rhs.love = love;
    column_resolution_solve_rhs(2 * M, K, w, rhs, T, lane, nlanes, sync);
    radial_resolution_reduce(M, K, love, depz, w, T, out, trace, lane, nlanes, sync);
    return flag;
}

// the whole of one column: radial_assemble, factor, T, reduce.  depz: the M depths of the unknowns (fp32, the models'); vsv / vsh: the
// column's values of the two models (they enter b only, which no figure here reads).  T: 2M * K doubles (radial_resolution_t).  Returns
// the flag; nused[2] and trace[2] are the same on every lane.
template <class Sync>
DSA_CS int radial_resolution(const RadialIn& in, const float* depz, float smooth, float damp, float aniso, const float* vsv, const float* vsh, long long v_stride,
                             const ColumnWork& w, double* T, const RadialResOut& out, double* trace, int* nused, int lane, int nlanes, Sync sync)
{
    const double lambda2 = (double)smooth * (double)smooth, mu2 = (double)damp * (double)damp, gamma2 = (double)aniso * (double)aniso;
    double chi2[2];
    radial_assemble(in, lambda2, mu2, gamma2, vsv, vsh, v_stride, w, nused, chi2, lane, nlanes, sync);
    if (nused[0] + nused[1] == 0) {
        radial_resolution_zero(in.M, in.K, out, trace, lane, nlanes);
        return kColumnNoData;
    }
    return radial_resolution_finish(in.M, in.K, in.love, depz, w, T, out, trace, lane, nlanes, sync);
}

}  // namespace dsa
