// The resolution of the laterally coupled depth step: point-spread functions, rows of the averaging kernel, variances
// and test models of column_lateral.h's system, every one a solve A x = f of section 24's operator by section 24's preconditioned conjugate
// gradients with another right-hand side -- a batch of members that lie side by side, one lane per member.  column_lateral.h is included as
// it is: the set-up (N_c, the factor, the active flags, the edges, lam2), the operator, the preconditioner, the dots, the 64-chain global sum,
// thr = tol^2 rz0, istop and the even / odd directions are its figures, bit for bit; the model-difference term of bt is absent (bt = f).
//
//   H_c      = G_c^T G_c, packed: column_assemble's triangle at lambda2 = mu2 = 0.0 -- the Gram chain of the used data alone
//   H m      (H m)_c[l] = sum_j H_c[l][j] m[j], j ascending from 0.0
//   member s kind[s], index[s]; its own alpha, beta, rz, rz0, thr, itn, done, istop.  A member that is done is frozen while others go on.
//     0 PSF    spike at unknown index = b M + l: f_c = H_c e_l in column b (the chain above with m = e_l), 0.0 elsewhere
//     1 unit   f = e_index; after the solve u = H x (the same chain): row index of R = A^-1 H; var = x^T u
//     2 model  f = H m, m row index of models ((rows, M, nint) doubles, depth slowest)
//     3 given  f = row index of models
//     any other kind (the padding of the last lane group): f = 0.0, which stops at iteration 0
//            An entry of f in a column that is not active is 0.0.
//   u        x (kinds 0, 2, 3) or H x (kind 1); 0.0 in a column that is not active
//   measures kinds 0 and 1, centre (b0, l0) = (index / M, index % M): per column, l ascending from 0.0, r2 = u u:
//            m1 += r2; mz += r2 (dz dz), dz = (double)depz[l] - (double)depz[l0]; mx += r2 (di di), my += r2 (dj dj), di = bi - bi0,
//            dj = bj - bj0 in cells; var += x[l] u[l] (kind 1; 0.0 for kind 0) -- then each in section 24's global sum;
//            val = u[b0][l0]; own = column b0's figure of m1.  Kinds 2 and 3 report zeros.
//
// The member vectors f, x, r, z, q, p0, p1 are laid member-fastest: element (b, l, s) at (b M + l) Sc + s, Sc the chunk's member count
// rounded up to 64; the per-member scalars and ints the same way.  The functions take (lane, nlanes, sync) and share the 64 members of lane
// group g out over the lanes: on the device lane = member (column_kernels.hip: k_latres_*, one wavefront per column and group), on a CPU lane 0
// of 1 runs them one after another (tests/hostcheck_column_lateral_resolution.cpp).  Every member's arithmetic is one sequential chain of its
// own, so the lane mapping, the member's place in the batch and its neighbours in it cannot change a bit.  fp64 under -ffp-contract=off.
//
// The loop's phases are written a second time here, beside column_lateral.h's: there a column's vectors are contiguous and the lanes share
// out l, with barriers inside the solve; here they are strided by Sc, the lanes share out the members and a lane runs column_solve's chain
// alone on a copy in the work arrays (element l of slot t at l * 64 + t).  The expressions are column_lateral.h's, operation by operation.
#pragma once

#include "column_lateral.h"

namespace dsa {

constexpr int kLatResGroup = 64;
enum { kLatResPsf = 0, kLatResUnit, kLatResModel, kLatResGiven, kLatResKinds };
enum { kLatResVal = 0, kLatResM1, kLatResMz, kLatResMx, kLatResMy, kLatResOwn, kLatResVar, kLatResMeasures };
enum { kLatResFigM1 = 0, kLatResFigMz, kLatResFigMx, kLatResFigMy, kLatResFigVar, kLatResFigures };
constexpr int kLatResVectors = 7;

DSA_CS int latres_round(int count) { return (count + kLatResGroup - 1) / kLatResGroup * kLatResGroup; }

// what one member of a chunk takes: its seven vectors, a figure per column for the dots, five for the measures, its scalars; its ints, kind
// and index
DSA_CS size_t latres_member_doubles(int nvx, int nvy, int M)
{
    const size_t n = (size_t)nvx * nvy;
    return kLatResVectors * n * (size_t)M + n + kLatResFigures * n + kLatScalars;
}
DSA_CS size_t latres_member_bytes(int nvx, int nvy, int M) { return latres_member_doubles(nvx, nvy, M) * sizeof(double) + (kLatInts + 2) * sizeof(int); }
// doubles that hold a chunk of Sc members, the ints included
DSA_CS size_t latres_batch_doubles(int nvx, int nvy, int M, int Sc) { return (latres_member_bytes(nvx, nvy, M) * (size_t)Sc + sizeof(double) - 1) / sizeof(double); }
// doubles of the work arrays of one column and lane group: N, the factor and d (or H) staged, two operand vectors per member
DSA_CS size_t latres_work_doubles(int M) { return 2 * (size_t)column_tri_size(M) + (size_t)M + 2 * (size_t)M * kLatResGroup; }

struct LatResBatch {
    LateralWs ws;                   // the shared set-up of section 24: N_c, the factor, the active flags
    const double* H;                // (nint, T)
    const float* depz;
    const double* models;           // (rows, M, nint), or null
    int Sc;
    double *f, *x, *r, *z, *q, *p0, *p1;
    double *part, *fig, *sc;
    int *ic, *kind, *index;
};

DSA_CS LatResBatch latres_batch(const LateralWs& ws, const double* H, const float* depz, const double* models, double* base, int Sc)
{
    const size_t n = (size_t)ws.nvx * ws.nvy, v = n * (size_t)ws.M * (size_t)Sc;
    LatResBatch B;
    B.ws = ws; B.H = H; B.depz = depz; B.models = models; B.Sc = Sc;
    B.f = base; B.x = base + v; B.r = base + 2 * v; B.z = base + 3 * v; B.q = base + 4 * v; B.p0 = base + 5 * v; B.p1 = base + 6 * v;
    base += kLatResVectors * v;
    B.part = base; base += n * (size_t)Sc;
    B.fig = base; base += kLatResFigures * n * (size_t)Sc;
    B.sc = base; base += (size_t)kLatScalars * Sc;
    B.ic = reinterpret_cast<int*>(base);
    B.kind = B.ic + (size_t)kLatInts * Sc;
    B.index = B.kind + Sc;
    return B;
}

DSA_CS size_t latres_at(const LatResBatch& B, int b, int l, int s) { return ((size_t)b * B.ws.M + l) * (size_t)B.Sc + s; }
DSA_CS double latres_sym(const double* tri, int l, int j) { return tri[j <= l ? column_tri(l, j) : column_tri(j, l)]; }

// the work arrays: st (N, then the factor, then d -- or H alone), w1, w2
struct LatResWork { double *st, *w1, *w2; };
DSA_CS LatResWork latres_work(double* base, int M)
{
    LatResWork w;
    w.st = base; w.w1 = base + 2 * (size_t)column_tri_size(M) + M; w.w2 = w.w1 + (size_t)M * kLatResGroup;
    return w;
}

// N, the factor and d of an active column b to st; every lane sees them after the barrier
template <class Sync>
DSA_CS void latres_stage_factor(const LateralWs& ws, int b, double* st, int lane, int nlanes, Sync sync)
{
    const LateralColumn c = lateral_column(ws, b);
    const int T = column_tri_size(ws.M);
    for (int e = lane; e < 2 * T; e += nlanes) st[e] = c.N[e];          // (the factor follows N)
    for (int l = lane; l < ws.M; l += nlanes) st[2 * T + l] = c.d[l];
    sync();
}

template <class Sync>
DSA_CS void latres_stage_gram(const LatResBatch& B, int b, double* st, int lane, int nlanes, Sync sync)
{
    const int T = column_tri_size(B.ws.M);
    for (int e = lane; e < T; e += nlanes) st[e] = B.H[(size_t)b * T + e];
    sync();
}

// column_solve's chain of one member, in place in w (element i at i * 64)
DSA_CS void latres_solve(int M, const double* F, const double* d, double* w)
{
    const int G = kLatResGroup;
    for (int p = 0; p + 1 < M; ++p) {
        const double bp = w[p * G];
        for (int i = p + 1; i < M; ++i) w[i * G] -= F[column_tri(i, p)] * bp;
    }
    for (int i = 0; i < M; ++i) w[i * G] = w[i * G] / d[i];
    for (int i = M - 2; i >= 0; --i) {
        double s = w[i * G];
        for (int p = i + 1; p < M; ++p) s -= F[column_tri(p, i)] * w[p * G];
        w[i * G] = s;
    }
}

// element l of (A y)_b of member s: lateral_operator's expression; own: y_b (element j at j * 64)
DSA_CS double latres_operator(const LatResBatch& B, int b, int s, const double* N, const double* own, int l, int what, double beta, int pold)
{
    const int M = B.ws.M, G = kLatResGroup;
    double t = 0.0;
    for (int j = 0; j < M; ++j) t += latres_sym(N, l, j) * own[j * G];
    double sum = 0.0;
    int deg = 0;
    const double* p = pold ? B.p1 : B.p0;
    for (int e = 0; e < 4; ++e) {
        const int nb = lateral_neighbour(B.ws, b, e);
        if (nb >= 0) {
            ++deg;
            const size_t a = latres_at(B, nb, l, s);
            sum += what == 0 ? B.x[a] : B.z[a] + beta * p[a];
        }
    }
    return t + B.ws.lam2 * ((double)deg * own[l * G] - sum);
}

// (H m)_b[l]: the chain over j ascending from 0.0; m: element j at j * stride
DSA_CS double latres_gram_row(int M, const double* H, int l, const double* m, size_t stride)
{
    double v = 0.0;
    for (int j = 0; j < M; ++j) v += latres_sym(H, l, j) * m[j * stride];
    return v;
}

// the right-hand sides of column b, lane group g.  st: the work array that H_b is staged in
template <class Sync>
DSA_CS void latres_form(const LatResBatch& B, int b, int g, const LatResWork& w, int lane, int nlanes, Sync sync)
{
    const int M = B.ws.M, G = kLatResGroup, n = B.ws.nvx * B.ws.nvy;
    const bool on = B.ws.active[b] != 0;
    if (on) latres_stage_gram(B, b, w.st, lane, nlanes, sync);
    for (int t = lane; t < G; t += nlanes) {
        const int s = g * G + t, kind = B.kind[s], idx = B.index[s];
        double* m = w.w1 + t;
        if (on && kind == kLatResPsf)
            for (int j = 0; j < M; ++j) m[j * G] = idx == b * M + j ? 1.0 : 0.0;
        for (int l = 0; l < M; ++l) {
            double v = 0.0;
            if (on) {
                if (kind == kLatResPsf) { if (idx / M == b) v = latres_gram_row(M, w.st, l, m, G); }
                else if (kind == kLatResUnit) v = idx == b * M + l ? 1.0 : 0.0;
                else if (kind == kLatResModel) v = latres_gram_row(M, w.st, l, B.models + (size_t)idx * M * n + b, (size_t)n);
                else if (kind == kLatResGiven) v = B.models[((size_t)idx * M + l) * n + b];
            }
            B.f[latres_at(B, b, l, s)] = v;
        }
    }
}

// x = M^-1 f, the column's figure of f^T x (p_old = 0: the caller's zeros)
template <class Sync>
DSA_CS void latres_start(const LatResBatch& B, int b, int g, const LatResWork& w, int lane, int nlanes, Sync sync)
{
    const int M = B.ws.M, G = kLatResGroup, T = column_tri_size(M);
    const bool on = B.ws.active[b] != 0;
    if (on) latres_stage_factor(B.ws, b, w.st, lane, nlanes, sync);
    for (int t = lane; t < G; t += nlanes) {
        const int s = g * G + t;
        if (!on) { B.part[(size_t)b * B.Sc + s] = 0.0; continue; }
        double* x = w.w2 + t;
        for (int l = 0; l < M; ++l) x[l * G] = B.f[latres_at(B, b, l, s)];
        latres_solve(M, w.st + T, w.st + 2 * T, x);
        double dot = 0.0;
        for (int l = 0; l < M; ++l) {
            const size_t a = latres_at(B, b, l, s);
            B.x[a] = x[l * G];
            dot += B.f[a] * x[l * G];
        }
        B.part[(size_t)b * B.Sc + s] = dot;
    }
}

// r = f - A x, z = M^-1 r, the column's figure of r^T z
template <class Sync>
DSA_CS void latres_residual(const LatResBatch& B, int b, int g, const LatResWork& w, int lane, int nlanes, Sync sync)
{
    const int M = B.ws.M, G = kLatResGroup, T = column_tri_size(M);
    const bool on = B.ws.active[b] != 0;
    if (on) latres_stage_factor(B.ws, b, w.st, lane, nlanes, sync);
    for (int t = lane; t < G; t += nlanes) {
        const int s = g * G + t;
        if (!on) { B.part[(size_t)b * B.Sc + s] = 0.0; continue; }
        double *own = w.w1 + t, *z = w.w2 + t;
        for (int l = 0; l < M; ++l) own[l * G] = B.x[latres_at(B, b, l, s)];
        for (int l = 0; l < M; ++l) {
            const size_t a = latres_at(B, b, l, s);
            const double q = latres_operator(B, b, s, w.st, own, l, 0, 0.0, 0);
            const double r = B.f[a] - q;
            B.r[a] = r;
            z[l * G] = r;
        }
        for (int l = 0; l < M; ++l) own[l * G] = z[l * G];
        latres_solve(M, w.st + T, w.st + 2 * T, z);
        double dot = 0.0;
        for (int l = 0; l < M; ++l) {
            B.z[latres_at(B, b, l, s)] = z[l * G];
            dot += own[l * G] * z[l * G];
        }
        B.part[(size_t)b * B.Sc + s] = dot;
    }
}

// first half of an iteration: p = z + beta p_old, q = A p, the column's figure of p^T q.  A member that is done is left alone.
template <class Sync>
DSA_CS void latres_direction(const LatResBatch& B, int b, int g, const LatResWork& w, int lane, int nlanes, Sync sync)
{
    const int M = B.ws.M, G = kLatResGroup;
    const bool on = B.ws.active[b] != 0;
    if (on) latres_stage_factor(B.ws, b, w.st, lane, nlanes, sync);
    for (int t = lane; t < G; t += nlanes) {
        const int s = g * G + t;
        if (B.ic[kLatDone * B.Sc + s]) continue;
        if (!on) { B.part[(size_t)b * B.Sc + s] = 0.0; continue; }
        const int pold = B.ic[kLatItn * B.Sc + s] & 1;
        const double beta = B.sc[kLatBeta * B.Sc + s];
        const double* po = pold ? B.p1 : B.p0;
        double* pn = pold ? B.p0 : B.p1;
        double* own = w.w1 + t;
        for (int l = 0; l < M; ++l) {
            const size_t a = latres_at(B, b, l, s);
            const double p = B.z[a] + beta * po[a];
            pn[a] = p;
            own[l * G] = p;
        }
        double dot = 0.0;
        for (int l = 0; l < M; ++l) {
            const double q = latres_operator(B, b, s, w.st, own, l, 1, beta, pold);
            B.q[latres_at(B, b, l, s)] = q;
            dot += own[l * G] * q;
        }
        B.part[(size_t)b * B.Sc + s] = dot;
    }
}

// second half: x = x + alpha p, r = r - alpha q, z = M^-1 r, the column's figure of r^T z
template <class Sync>
DSA_CS void latres_update(const LatResBatch& B, int b, int g, const LatResWork& w, int lane, int nlanes, Sync sync)
{
    const int M = B.ws.M, G = kLatResGroup, T = column_tri_size(M);
    const bool on = B.ws.active[b] != 0;
    if (on) latres_stage_factor(B.ws, b, w.st, lane, nlanes, sync);
    for (int t = lane; t < G; t += nlanes) {
        const int s = g * G + t;
        if (B.ic[kLatDone * B.Sc + s]) continue;
        if (!on) { B.part[(size_t)b * B.Sc + s] = 0.0; continue; }
        const double alpha = B.sc[kLatAlpha * B.Sc + s];
        const double* p = (B.ic[kLatItn * B.Sc + s] & 1) ? B.p0 : B.p1;
        double *keep = w.w1 + t, *z = w.w2 + t;
        for (int l = 0; l < M; ++l) {
            const size_t a = latres_at(B, b, l, s);
            B.x[a] = B.x[a] + alpha * p[a];
            const double r = B.r[a] - alpha * B.q[a];
            B.r[a] = r;
            keep[l * G] = r;
            z[l * G] = r;
        }
        latres_solve(M, w.st + T, w.st + 2 * T, z);
        double dot = 0.0;
        for (int l = 0; l < M; ++l) {
            B.z[latres_at(B, b, l, s)] = z[l * G];
            dot += keep[l * G] * z[l * G];
        }
        B.part[(size_t)b * B.Sc + s] = dot;
    }
}

// lateral_sum's shape on the figures of member s: part[b * Sc + s]
DSA_CS double latres_sum(const double* part, int n, int Sc, int s)
{
    double total = 0.0;
    for (int t = 0; t < kLateralChains; ++t) {
        double c = 0.0;
        for (int b = t; b < n; b += kLateralChains) c += part[(size_t)b * Sc + s];
        total += c;
    }
    return total;
}

// a global sum of every member of lane group g and what follows from it: lateral_reduce and lateral_scalars per member
DSA_CS void latres_reduce(const LatResBatch& B, int g, int what, double tol, int maxit, int lane, int nlanes)
{
    const int Sc = B.Sc, n = B.ws.nvx * B.ws.nvy;
    for (int t = lane; t < kLatResGroup; t += nlanes) {
        const int s = g * kLatResGroup + t;
        if ((what == kLatSumPq || what == kLatSumRz) && B.ic[kLatDone * Sc + s]) continue;
        const double sum = latres_sum(B.part, n, Sc, s);
        if (what == kLatSumRz0) {
            B.sc[kLatRz0 * Sc + s] = sum;
            B.sc[kLatThr * Sc + s] = (tol * tol) * sum;
            B.sc[kLatAlpha * Sc + s] = 0.0;
            B.sc[kLatBeta * Sc + s] = 0.0;
            B.ic[kLatItn * Sc + s] = 0; B.ic[kLatDone * Sc + s] = 0; B.ic[kLatStop * Sc + s] = 0;
        } else if (what == kLatSumFirst) {
            B.sc[kLatRz * Sc + s] = sum;
            if (!B.ws.edges || sum <= B.sc[kLatThr * Sc + s]) { B.ic[kLatDone * Sc + s] = 1; B.ic[kLatStop * Sc + s] = 1; }
        } else if (what == kLatSumPq) {
            B.sc[kLatAlpha * Sc + s] = B.sc[kLatRz * Sc + s] / sum;
        } else {
            B.sc[kLatBeta * Sc + s] = sum / B.sc[kLatRz * Sc + s];
            B.sc[kLatRz * Sc + s] = sum;
            const int itn = B.ic[kLatItn * Sc + s] + 1;
            B.ic[kLatItn * Sc + s] = itn;
            if (sum <= B.sc[kLatThr * Sc + s]) { B.ic[kLatDone * Sc + s] = 1; B.ic[kLatStop * Sc + s] = 1; }
            else if (itn >= maxit) { B.ic[kLatDone * Sc + s] = 1; B.ic[kLatStop * Sc + s] = 2; }
        }
    }
}

// after the loop: u of column b into the q vectors, and the column's figures of the measures
template <class Sync>
DSA_CS void latres_measure(const LatResBatch& B, int b, int g, const LatResWork& w, int lane, int nlanes, Sync sync)
{
    const int M = B.ws.M, G = kLatResGroup, Sc = B.Sc, n = B.ws.nvx * B.ws.nvy;
    const bool on = B.ws.active[b] != 0;
    if (on) latres_stage_gram(B, b, w.st, lane, nlanes, sync);
    const int bj = b / B.ws.nvx, bi = b - bj * B.ws.nvx;
    for (int t = lane; t < G; t += nlanes) {
        const int s = g * G + t, kind = B.kind[s], idx = B.index[s];
        const bool measured = kind == kLatResPsf || kind == kLatResUnit;
        double fig[kLatResFigures] = { 0.0, 0.0, 0.0, 0.0, 0.0 };
        if (!on) {
            for (int l = 0; l < M; ++l) B.q[latres_at(B, b, l, s)] = 0.0;
        } else {
            double* x = w.w1 + t;
            for (int l = 0; l < M; ++l) x[l * G] = B.x[latres_at(B, b, l, s)];
            const int b0 = measured ? idx / M : 0, l0 = measured ? idx - b0 * M : 0;
            const int bj0 = b0 / B.ws.nvx, bi0 = b0 - bj0 * B.ws.nvx;
            const double di = (double)(bi - bi0), dj = (double)(bj - bj0);
            for (int l = 0; l < M; ++l) {
                const double u = kind == kLatResUnit ? latres_gram_row(M, w.st, l, x, G) : x[l * G];
                B.q[latres_at(B, b, l, s)] = u;
                if (measured) {
                    const double r2 = u * u;
                    const double dz = (double)B.depz[l] - (double)B.depz[l0];
                    fig[kLatResFigM1] += r2;
                    fig[kLatResFigMz] += r2 * (dz * dz);
                    fig[kLatResFigMx] += r2 * (di * di);
                    fig[kLatResFigMy] += r2 * (dj * dj);
                    if (kind == kLatResUnit) fig[kLatResFigVar] += x[l * G] * u;
                }
            }
        }
        for (int q = 0; q < kLatResFigures; ++q) B.fig[((size_t)q * n + b) * Sc + s] = fig[q];
    }
}

// the measures of every member of lane group g: measures (Sc, 7)
DSA_CS void latres_measures(const LatResBatch& B, int g, double* measures, int lane, int nlanes)
{
    const int M = B.ws.M, Sc = B.Sc, n = B.ws.nvx * B.ws.nvy;
    for (int t = lane; t < kLatResGroup; t += nlanes) {
        const int s = g * kLatResGroup + t, kind = B.kind[s], idx = B.index[s];
        double* out = measures + (size_t)s * kLatResMeasures;
        if (kind != kLatResPsf && kind != kLatResUnit) {
            for (int q = 0; q < kLatResMeasures; ++q) out[q] = 0.0;
            continue;
        }
        const int b0 = idx / M, l0 = idx - b0 * M;
        out[kLatResVal] = B.q[latres_at(B, b0, l0, s)];
        out[kLatResM1] = latres_sum(B.fig + (size_t)kLatResFigM1 * n * Sc, n, Sc, s);
        out[kLatResMz] = latres_sum(B.fig + (size_t)kLatResFigMz * n * Sc, n, Sc, s);
        out[kLatResMx] = latres_sum(B.fig + (size_t)kLatResFigMx * n * Sc, n, Sc, s);
        out[kLatResMy] = latres_sum(B.fig + (size_t)kLatResFigMy * n * Sc, n, Sc, s);
        out[kLatResOwn] = B.fig[((size_t)kLatResFigM1 * n + b0) * Sc + s];
        out[kLatResVar] = kind == kLatResUnit ? latres_sum(B.fig + (size_t)kLatResFigVar * n * Sc, n, Sc, s) : 0.0;
    }
}

// H_c of column b: column_assemble at lambda2 = mu2 = 0.0 in the work arrays w, its triangle to H (nint, T).  A column that is not active
// gets zeros (its H is never read).
template <class Sync>
DSA_CS void latres_gram(const ColumnIn& in, const ColumnWork& w, const LateralWs& ws, int b, double* H, int lane, int nlanes, Sync sync)
{
    const int T = column_tri_size(ws.M);
    if (!ws.active[b]) {
        for (int e = lane; e < T; e += nlanes) H[(size_t)b * T + e] = 0.0;
        return;
    }
    double chi2 = 0.0;
    (void)column_assemble(in, 0.0, 0.0, w, &chi2, lane, nlanes, sync);
    for (int e = lane; e < T; e += nlanes) H[(size_t)b * T + e] = w.tri[e];
}

}  // namespace dsa
