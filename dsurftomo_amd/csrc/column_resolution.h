// The depth resolution of one column of the period maps: what the regularised normal matrix of column_system.h's step
// says about its own answer.  Definitions of section 21: M unknowns, K data in slot order, the used data, g_kl = a_k S_kl,
// N = G^T G + smooth^2 L^T L + damp^2 I -- assembled and factored by column_assemble and column_factor, unchanged.
//
//   T        the generalised inverse, K x M: row k solves N t = g_k (row k of G) with column_solve's arithmetic exactly -- forward with p
//            ascending, the division by d, back with i descending and p ascending.  Rows of unused data are 0.0.  No M x M inverse is formed.
//   R        = T^T G (section 12's convention: column j is the point-spread function of unknown j), R_lj = sum_k T_kl g_kj
//   per j    with l ascending: r2 = R_lj R_lj, m1 += r2, dz = (double)depz[l] - (double)depz[j], m2 += r2 (dz dz); the outputs R_jj, m1, m2 and
//            var_j = sum_k T_kj T_kj, the variance of unknown j for unit variance of the weighted data (the diagonal of N^-1 G^T G N^-1)
//   per k    the leverage h_k = sum_l g_kl T_kl, l ascending: the diagonal of the data resolution matrix G T^T; 0 for an unused datum
//   column   trace = sum_j R_jj, j ascending
// Every sum over k runs over the used k ascending, every sum from 0.0.  nused = 0 is kColumnNoData, a pivot that is not finite or <= 0
// kColumnNotPositive; in both every output of the column is 0.0.
//
// column_system.h's contract: __host__ __device__, fp64 under -ffp-contract=off, (lane, nlanes, sync), every figure one sequential chain of
// its own, so the lane mapping cannot change a bit.  The solves go one lane per datum (K <= 60 < 64): each lane runs the whole chain of
// its right-hand side, so the serial back substitutions of the K solves run side by side.  The lanes' vectors are stored datum-fastest,
// T[i * Kpad + k]: at step (i, p) of a solve the lanes read the same entry of the factor (a broadcast) and element i of their own vector,
// consecutive doubles -- the 32 lanes of one half of a ds_read_b64 cover 64 consecutive dwords, every bank once, whatever Kpad is; so
// Kpad = K.  The reductions go one lane per unknown (R, var) and one per datum (h).
#pragma once

#include "column_system.h"

namespace dsa {

DSA_CS int column_resolution_kpad(int K) { return K; }

// doubles of work: column_system.h's arrays, then T (M x Kpad)
DSA_CS size_t column_resolution_doubles(int M, int K) { return column_work_doubles(M, K) + (size_t)M * column_resolution_kpad(K); }

DSA_CS double* column_resolution_t(double* base, int M, int K) { return base + column_work_doubles(M, K); }

// where one column's outputs lie: measure q (0 R_jj, 1 m1, 2 m2, 3 var) of unknown j at measures[q * m_qstride + j * m_jstride], h_k at
// leverage[k * h_stride], R_lj at R[(l * M + j) * r_stride] (R may be null: the store is skipped, nothing else)
struct ColumnResOut {
    double* measures; long long m_qstride, m_jstride;
    double* leverage; long long h_stride;
    double* R; long long r_stride;
};

// DSA_CS for a member function
#if defined(__HIPCC__)
#define DSA_CS_MEMBER __host__ __device__ __forceinline__
#else
#define DSA_CS_MEMBER inline
#endif

// element i of the right-hand side of datum k: row k of G
struct ColumnRowOfG {
    const double* G; int M;
    DSA_CS_MEMBER double operator()(int k, int i) const { return G[k * M + i]; }
};

// T on a factored system of M unknowns (w.tri, w.d) with w.a assembled: lane k runs the solve of datum k on the right-hand side
// rhs(k, 0 .. M-1).  The one copy of the per-datum solve: section 22's on row k of G, section 26's on 2M unknowns.
template <class Rhs, class Sync>
DSA_CS void column_resolution_solve_rhs(int M, int K, const ColumnWork& w, const Rhs& rhs, double* T, int lane, int nlanes, Sync sync)
{
    const int Kp = column_resolution_kpad(K);
    for (int k = lane; k < K; k += nlanes) {
        if (!(w.a[k] > 0.0)) {
            for (int i = 0; i < M; ++i) T[i * Kp + k] = 0.0;
            continue;
        }
        for (int i = 0; i < M; ++i) T[i * Kp + k] = rhs(k, i);
        for (int p = 0; p + 1 < M; ++p) {
            const double tp = T[p * Kp + k];
            for (int i = p + 1; i < M; ++i) T[i * Kp + k] -= w.tri[column_tri(i, p)] * tp;
        }
        for (int i = 0; i < M; ++i) T[i * Kp + k] = T[i * Kp + k] / w.d[i];
        for (int i = M - 2; i >= 0; --i) {
            double s = T[i * Kp + k];
            for (int p = i + 1; p < M; ++p) s -= w.tri[column_tri(p, i)] * T[p * Kp + k];
            T[i * Kp + k] = s;
        }
    }
    sync();
}

// T of section 22: the right-hand sides are the rows of w.G
template <class Sync>
DSA_CS void column_resolution_solve(int M, int K, const ColumnWork& w, double* T, int lane, int nlanes, Sync sync)
{
    ColumnRowOfG rhs;
    rhs.G = w.G; rhs.M = M;
    column_resolution_solve_rhs(M, K, w, rhs, T, lane, nlanes, sync);
}

// the measures, the leverages and the trace from T and w.G; w.b gets the R_jj.  Every lane returns the same trace.
template <class Sync>
DSA_CS double column_resolution_reduce(int M, int K, const float* depz, const ColumnWork& w, const double* T, const ColumnResOut& out, int lane, int nlanes,
                                       Sync sync)
{
    const int Kp = column_resolution_kpad(K);
    for (int j = lane; j < M; j += nlanes) {
        double m1 = 0.0, m2 = 0.0, rjj = 0.0;
        for (int l = 0; l < M; ++l) {
            double r = 0.0;
            for (int k = 0; k < K; ++k)
                if (w.a[k] > 0.0) r += T[l * Kp + k] * w.G[k * M + j];
            const double r2 = r * r;
            m1 += r2;
            const double dz = (double)depz[l] - (double)depz[j];
            m2 += r2 * (dz * dz);
            if (l == j) rjj = r;
            if (out.R) out.R[((long long)l * M + j) * out.r_stride] = r;
        }
        double var = 0.0;
        for (int k = 0; k < K; ++k)
            if (w.a[k] > 0.0) var += T[j * Kp + k] * T[j * Kp + k];
        out.measures[0 * out.m_qstride + j * out.m_jstride] = rjj;
        out.measures[1 * out.m_qstride + j * out.m_jstride] = m1;
        out.measures[2 * out.m_qstride + j * out.m_jstride] = m2;
        out.measures[3 * out.m_qstride + j * out.m_jstride] = var;
        w.b[j] = rjj;
    }
    for (int k = lane; k < K; k += nlanes) {
        double h = 0.0;
        if (w.a[k] > 0.0)
            for (int l = 0; l < M; ++l) h += w.G[k * M + l] * T[l * Kp + k];
        out.leverage[k * out.h_stride] = h;
    }
    sync();
    double trace = 0.0;
    for (int j = 0; j < M; ++j) trace += w.b[j];
    return trace;
}

// every output of one column 0.0
DSA_CS void column_resolution_zero(int M, int K, const ColumnResOut& out, int lane, int nlanes)
{
    for (int j = lane; j < M; j += nlanes)
        for (int q = 0; q < 4; ++q) out.measures[q * out.m_qstride + j * out.m_jstride] = 0.0;
    for (int k = lane; k < K; k += nlanes) out.leverage[k * out.h_stride] = 0.0;
    if (out.R)
        for (int e = lane; e < M * M; e += nlanes) out.R[(long long)e * out.r_stride] = 0.0;
}

// factor, T, reduce on an assembled system (w.tri, w.G, w.a): the flag; where the factorisation stops every output is 0.0
template <class Sync>
DSA_CS int column_resolution_finish(int M, int K, const float* depz, const ColumnWork& w, double* T, const ColumnResOut& out, double* trace, int lane, int nlanes,
                                    Sync sync)
{
    const int flag = column_factor(M, w, lane, nlanes, sync);
    if (flag != kColumnOk) {
        column_resolution_zero(M, K, out, lane, nlanes);
        *trace = 0.0;
        return flag;
    }
    column_resolution_solve(M, K, w, T, lane, nlanes, sync);
    *trace = column_resolution_reduce(M, K, depz, w, T, out, lane, nlanes, sync);
    return flag;
}

// the whole of one column: assemble, factor, T, reduce.  depz: the M depths of the unknowns (fp32, the model's).  T: M * Kpad doubles
// (column_resolution_t).  Returns the flag; *nused and *trace are the same on every lane.  A column without a used datum is kColumnNoData
// whatever damp is.
template <class Sync>
DSA_CS int column_resolution(const ColumnIn& in, const float* depz, float smooth, float damp, const ColumnWork& w, double* T, const ColumnResOut& out,
                             double* trace, int* nused, int lane, int nlanes, Sync sync)
{
    const double lambda2 = (double)smooth * (double)smooth, mu2 = (double)damp * (double)damp;
    double chi2 = 0.0;
    *nused = column_assemble(in, lambda2, mu2, w, &chi2, lane, nlanes, sync);
    if (*nused == 0) {
        column_resolution_zero(in.M, in.K, out, lane, nlanes);
        *trace = 0.0;
        return kColumnNoData;
    }
    return column_resolution_finish(in.M, in.K, depz, w, T, out, trace, lane, nlanes, sync);
}

}  // namespace dsa
