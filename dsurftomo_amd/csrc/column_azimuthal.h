// The depth inversion of the 2 psi terms of one column of the period maps: the A1(T), A2(T) of
// c(psi) = c0 + A1 cos 2 psi + A2 sin 2 psi, which maps --azimuthal leaves per period, inverted for gc(z) = Gc/L and gs(z) = Gs/L.  M = nz - 1
// unknowns per component, K data in slot order, as everywhere in the column family.
//
//   Z        the depth factor of section 18, Z_kl = sen_vs_kl (double)(0.5f v_l) (ray_kernels.hip: k_sen_azimuthal), handed in as ColumnIn::S
//   used     datum k is used iff the isotropic step would use it (wt_k > 0, c0_k > 0, pv_k > 0) and slot k is a Rayleigh slot; the caller
//            hands in effective weights that are 0 at a Love slot, so a Love slot is a slot of weight 0 and column_assemble's rule is the
//            whole rule.  The Z, A1, A2 of an unused datum are never read.
//   system   column_assemble on (c0, the effective weights, pv, Z): a_k, G_kl = a_k Z_kl, N = G^T G + smooth^2 L^T L + damp^2 I; its b and chi2
//            are not used.  rhoc_k = a_k (double)A1_k, rhos_k = a_k (double)A2_k; bc_l = sum_k G_kl rhoc_k, bs_l likewise;
//            chi2_before = (sum_k rhoc_k^2, sum_k rhos_k^2)
//   solve    column_factor once; gc and gs solve L D L^T x = b with column_solve's chain (forward with p ascending, the division by d, back
//            with i descending and p ascending).  column_resolution_solve_rhs states that chain per lane; here one loop hands K + 2 chains to
//            the lanes -- the K rows of G (T of section 22) and the two right-hand sides -- so with K + 2 <= 62 lanes of a wavefront all of
//            them run side by side and the call adds no serial chain to section 22's
//   fit      f_k = sum_l G_kl g_l (l ascending); chi2_after = (sum_k (rhoc_k - fc_k)^2, sum_k (rhos_k - fs_k)^2)
//   measures R_jj, m1, m2, var_j and the leverages h_k: column_resolution_reduce, unchanged -- gc and gs share the operator, so one set
//            serves both; var_j is the variance of gc_j and of gs_j for unit variance of the weighted A1 and A2
// Every sum over k runs over the used k ascending, every sum from 0.0.  nused = 0 is kColumnNoData, a pivot that is not finite or <= 0
// kColumnNotPositive; in both every output of the column is 0.0.
//
// column_system.h's contract: __host__ __device__, fp64 under -ffp-contract=off, no libm, no square root, IEEE division, (lane, nlanes, sync),
// every figure one sequential chain of its own, so the lane mapping cannot change a bit.
#pragma once

#include "column_system.h"
#include "column_resolution.h"

namespace dsa {

// doubles of work: column_resolution.h's arrays (the step's, then T), then X (M x 2: the right-hand sides, then gc | gs, x_l of component q
// at 2 l + q), rhoc and rhos (K each)
DSA_CS size_t column_azimuthal_doubles(int M, int K) { return column_resolution_doubles(M, K) + 2 * (size_t)M + 2 * (size_t)K; }

struct ColumnAziWork { ColumnWork w; double *T, *X, *rc, *rs; };

DSA_CS ColumnAziWork column_azimuthal_work(double* base, int M, int K)
{
    ColumnAziWork z;
    z.w = column_work(base, M, K);
    z.T = column_resolution_t(base, M, K);
    z.X = base + column_resolution_doubles(M, K);
    z.rc = z.X + 2 * (size_t)M;
    z.rs = z.rc + K;
    return z;
}

// one column's inputs: col as the step's with wt the effective weights (0 at a Love slot; null: 1 everywhere) and S = Z; element k of A1 /
// A2 at k * a_stride
struct ColumnAziIn {
    ColumnIn col;
    const float *a1, *a2; long long a_stride;
};

// where one column's outputs lie: g_l of component q (0 gc, 1 gs) at g[q * g_qstride + l * g_lstride]; chi2 entry q (0 before c, 1 before
// s, 2 after c, 3 after s) at chi2[q * chi2_stride]; the measures and leverages as section 22's (res.R is not read)
struct ColumnAziOut {
    double* g; long long g_qstride, g_lstride;
    double* chi2; long long chi2_stride;
    ColumnResOut res;
};

// every output of one column 0.0
DSA_CS void column_azimuthal_zero(int M, int K, const ColumnAziOut& out, int lane, int nlanes)
{
    ColumnResOut res = out.res;
    res.R = nullptr;
    column_resolution_zero(M, K, res, lane, nlanes);
    for (int e = lane; e < 2 * M; e += nlanes) out.g[(e / M) * out.g_qstride + (e % M) * out.g_lstride] = 0.0;
    for (int q = lane; q < 4; q += nlanes) out.chi2[q * out.chi2_stride] = 0.0;
}

// column_solve's chain on the M values x[0], x[stride], ...: what column_resolution_solve_rhs does to the vector of one lane
DSA_CS void column_azimuthal_chain(int M, const ColumnWork& w, double* x, int stride)
{
    for (int p = 0; p + 1 < M; ++p) {
        const double tp = x[p * stride];
        for (int i = p + 1; i < M; ++i) x[i * stride] -= w.tri[column_tri(i, p)] * tp;
    }
    for (int i = 0; i < M; ++i) x[i * stride] = x[i * stride] / w.d[i];
    for (int i = M - 2; i >= 0; --i) {
        double s = x[i * stride];
        for (int p = i + 1; p < M; ++p) s -= w.tri[column_tri(p, i)] * x[p * stride];
        x[i * stride] = s;
    }
}

// T and the two solutions on a factored system: chain k < K is datum k's row of T (zeros for an unused datum), chains K and K + 1 turn the
// right-hand sides in X into gc and gs
template <class Sync>
DSA_CS void column_azimuthal_solve(int M, int K, const ColumnAziWork& z, int lane, int nlanes, Sync sync)
{
    const int Kp = column_resolution_kpad(K);
    for (int s = lane; s < K + 2; s += nlanes) {
        if (s >= K) { column_azimuthal_chain(M, z.w, z.X + (s - K), 2); continue; }
        if (!(z.w.a[s] > 0.0)) {
            for (int i = 0; i < M; ++i) z.T[i * Kp + s] = 0.0;
            continue;
        }
        for (int i = 0; i < M; ++i) z.T[i * Kp + s] = z.w.G[s * M + i];
        column_azimuthal_chain(M, z.w, z.T + s, Kp);
    }
    sync();
}

// rhoc, rhos, the two right-hand sides (into X) and chi2_before on an assembled system (w.a, w.G).  Every lane gets the same before[2].
template <class Sync>
DSA_CS void column_azimuthal_rhs(int M, int K, const float* a1, const float* a2, long long a_stride, const ColumnAziWork& z, double* before, int lane, int nlanes,
                                 Sync sync)
{
    const ColumnWork& w = z.w;
    for (int k = lane; k < K; k += nlanes) {
        const bool used = w.a[k] > 0.0;
        z.rc[k] = used ? w.a[k] * (double)a1[k * a_stride] : 0.0;
        z.rs[k] = used ? w.a[k] * (double)a2[k * a_stride] : 0.0;
    }
    sync();
    for (int e = lane; e < 2 * M; e += nlanes) {
        const int l = e >> 1;
        const double* rho = (e & 1) ? z.rs : z.rc;
        double s = 0.0;
        for (int k = 0; k < K; ++k)
            if (w.a[k] > 0.0) s += w.G[k * M + l] * rho[k];
        z.X[e] = s;
    }
    double c = 0.0, s = 0.0;
    for (int k = 0; k < K; ++k)
        if (w.a[k] > 0.0) { c += z.rc[k] * z.rc[k]; s += z.rs[k] * z.rs[k]; }
    before[0] = c; before[1] = s;
    sync();
}

// factor, T and the two solutions, the measures, the fit on an assembled system (w.tri, w.G, w.a) with its right-hand sides
// (column_azimuthal_rhs): the flag; where the factorisation stops every output is 0.0
template <class Sync>
DSA_CS int column_azimuthal_finish(int M, int K, const float* depz, const ColumnAziWork& z, const double* before, const ColumnAziOut& out, int lane, int nlanes,
                                   Sync sync)
{
    const ColumnWork& w = z.w;
    const int flag = column_factor(M, w, lane, nlanes, sync);
    if (flag != kColumnOk) {
        column_azimuthal_zero(M, K, out, lane, nlanes);
        return flag;
    }
    column_azimuthal_solve(M, K, z, lane, nlanes, sync);
    ColumnResOut res = out.res;
    res.R = nullptr;
    (void)column_resolution_reduce(M, K, depz, w, z.T, res, lane, nlanes, sync);
    for (int e = lane; e < 2 * M; e += nlanes) out.g[(e & 1) * out.g_qstride + (e >> 1) * out.g_lstride] = z.X[e];
    // the residuals of the fit take the place of rho
    for (int k = lane; k < K; k += nlanes) {
        if (!(w.a[k] > 0.0)) continue;
        double fc = 0.0, fs = 0.0;
        for (int l = 0; l < M; ++l) { fc += w.G[k * M + l] * z.X[2 * l]; fs += w.G[k * M + l] * z.X[2 * l + 1]; }
        z.rc[k] = z.rc[k] - fc;
        z.rs[k] = z.rs[k] - fs;
    }
    sync();
    if (lane == 0) {
        double after_c = 0.0, after_s = 0.0;
        for (int k = 0; k < K; ++k)
            if (w.a[k] > 0.0) { after_c += z.rc[k] * z.rc[k]; after_s += z.rs[k] * z.rs[k]; }
        out.chi2[0 * out.chi2_stride] = before[0];
        out.chi2[1 * out.chi2_stride] = before[1];
        out.chi2[2 * out.chi2_stride] = after_c;
        out.chi2[3 * out.chi2_stride] = after_s;
    }
    return flag;
}

// the whole of one column.  depz: the M depths of the unknowns (fp32, the model's).  Returns the flag; *nused is the same on every lane.  A
// column without a used datum is kColumnNoData whatever damp is.
template <class Sync>
DSA_CS int column_azimuthal(const ColumnAziIn& in, const float* depz, float smooth, float damp, const ColumnAziWork& z, const ColumnAziOut& out, int* nused,
                            int lane, int nlanes, Sync sync)
{
    const int M = in.col.M, K = in.col.K;
    const double lambda2 = (double)smooth * (double)smooth, mu2 = (double)damp * (double)damp;
    double unused = 0.0;
    *nused = column_assemble(in.col, lambda2, mu2, z.w, &unused, lane, nlanes, sync);
    if (*nused == 0) {
        column_azimuthal_zero(M, K, out, lane, nlanes);
        return kColumnNoData;
    }
    double before[2];
    column_azimuthal_rhs(M, K, in.a1, in.a2, in.a_stride, z, before, lane, nlanes, sync);
    return column_azimuthal_finish(M, K, depz, z, before, out, lane, nlanes, sync);
}

}  // namespace dsa
