// Monte-Carlo radial depth inversion: C Metropolis chains per column of [Vsv ; Vsh], 2M = 2 (nz - 1) unknowns (the
// bottom depth of both models is kept), K data in slot order.  The chains are the models of a radial multi-model dispersion stage: a
// Rayleigh slot's curve is of the chain's Vsv, a Love slot's of its Vsh (slot k is a Love slot iff bit k of `love` is set, column_radial.h's
// meaning).  This header is the rest of a sweep and the finish; column_sample.h's generator, sample_neglog, sample_psi, sample_interior and
// layouts are used as they are.
//
//   boxes     per model and depth, fp32: lo = max(minvel, v0 - width), hi = min(maxvel, v0 + width), v0 the model's own start; minvel > 0
//   used      once per column on chain 0's curves, sample_used's rule; nused_r / nused_l count the Rayleigh / Love data.  Neither: flag 2,
//             never moved.  One type missing: the column samples, the prior and the tie hold that block
//   data      phi = sum rho_k^2 over the used k ascending from 0.0, rho_k = (double)wt_k ((double)obs_k - pv_k)
//   prior     psi = (sample_psi(Vsv) + sample_psi(Vsh)) + gam2 sum_l t_l^2, t_l = (double)vh_l - (double)vv_l, l ascending from 0.0;
//             lam2 = smooth^2, gam2 = aniso^2
//   set-up    chain 0 is the start; chain q > 0: unknown i = 0 .. 2M-1 (Vsv first) gets v0 + (float)(spread (2u - 1)) clipped to its box, draw
//             (column, q, 0, i).  A chain with a used datum without a root goes back to both starts with chain 0's phi and psi
//   proposal  draw 0: i = min((int)(u n), n - 1), n = 3M with pairs, 2M without; kind = i / M (0 a Vsv node, 1 a Vsh node, 2 a pair),
//             l = i - kind M; draw 1: delta = step (2u - 1).  Kinds 0 and 1 move one value by (float)delta in fp32, kind 2 moves Vsv_l and
//             Vsh_l by the same (float)delta -- the direction the tie does not penalise.  Any moved value outside its box: only the mark
//             (and the kind's proposal count) is written.  Else pnode = i, pold_v / pold_h the two old values at l, the new ones written
//   accept    sample_accept_any's rule and draw 2 on phi' + psi' against phi + psi; a rejection restores what the kind moved
//   counters  (4, chain, column) as column_sample.h's; kinds (6, chain, column): proposed per kind, then accepted per kind
//   moments   in the sweeps after burn, per chain and depth: d_v = (double)vv - (double)v0v, d_h likewise: S1v, S2v, S1h, S2h; Pvh += d_v d_h;
//             x = (double)vh / (double)vv, xi = x x, xi0 the same of the starts, d_xi = xi - xi0: X1 += d_xi, X2 += d_xi^2; npos += 1 where
//             vh > vv; phisum, nkept, the best phi + psi and both its models (the first wins a tie)
//   finish    per (column, depth), chains ascending -- see sample_radial_finish
//
// fp64 under -ffp-contract=off, no libm, no square root, IEEE division; one thread per (column, chain) (column_kernels.hip:
// k_sample_radial_*) or a loop over them (tests/hostcheck_column_sample_radial.cpp); a thread's sums are its own sequential chains from 0.0
// and no thread reads what another writes in the same launch.
// Layouts, column fastest everywhere: both model stores and the per-depth sums (depth, chain, column); the maps (chain, map, column); obs /
// wt (map, column); per-chain figures (chain, column).
#pragma once

#include "column_sample.h"

namespace dsa {

enum { kSampleKindVsv = 0, kSampleKindVsh = 1, kSampleKindPair = 2, kSampleKinds = 3, kSampleKindCounters = 6 };      // proposed [kind], accepted [3 + kind]
// the finish: per (column, depth) sixteen doubles, per column three doubles (column_sample.h's) and fifteen ints
enum { kSrMeanV = 0, kSrVarV = 1, kSrWV = 2, kSrBV = 3, kSrMeanH = 4, kSrVarH = 5, kSrWH = 6, kSrBH = 7, kSrMeanX = 8, kSrVarX = 9, kSrWX = 10, kSrBX = 11,
       kSrBestV = 12, kSrBestH = 13, kSrCov = 14, kSrShare = 15, kSrNodeFigures = 16 };
enum { kSrNusedR = 0, kSrNusedL = 1, kSrFlag = 2, kSrSumAccepted = 3, kSrSumKinds = 7, kSrReseeded = 13, kSrNkept = 14, kSrColumnCounts = 15 };

// the whole state of a radial sample stage and its inputs, where they lie
struct SampleRadialView {
    int nx, ny, nz, K, C, burn, pairs;
    long long ncol;
    unsigned long long seed, love;
    double lam2, gam2, step, spread, two_t;            // smooth^2, aniso^2, step, spread, 2 temperature
    float width, minvel, maxvel;
    const float* obs; const float* wt;                 // (K, ncol); wt may be null (1)
    const float* v0v; const float* v0h;                // (nz, ncol): the start models
    const double* pv;                                  // (C, K, ncol): the stage's map store
    float* vv; float* vh;                              // (nz, C, ncol): the stage's two model stores
    double* phi; double* psi;                          // (C, ncol)
    int* cnt; int* kcnt;                               // (4, C, ncol), (6, C, ncol)
    double* S1v; double* S2v; double* S1h; double* S2h; double* Pvh; double* X1; double* X2;      // (M, C, ncol)
    int* npos;                                         // (M, C, ncol)
    double* phisum; int* nkept;                        // (C, ncol)
    double* best_e; float* best_vv; float* best_vh;    // (C, ncol), (M, C, ncol)
    int* pnode; float* pold_v; float* pold_h; int* pmark;      // (C, ncol): the last sweep's proposal
    int* reseed;                                       // (C, ncol)
    unsigned long long* used;                          // (ncol)
    int* nused_r; int* nused_l; int* flag;             // (ncol)
    double* phi0;                                      // (ncol): phi of the start
};

DSA_CS long long sample_radial_at(const SampleRadialView& S, long long c, int q) { return (long long)q * S.ncol + c; }
DSA_CS long long sample_radial_node(const SampleRadialView& S, long long c, int q, int l) { return ((long long)l * S.C + q) * S.ncol + c; }

// the box of the start value b
DSA_CS void sample_radial_box(const SampleRadialView& S, float b, float* lo, float* hi)
{
    float a = b - S.width, z = b + S.width;
    if (a < S.minvel) a = S.minvel;
    if (z > S.maxvel) z = S.maxvel;
    *lo = a; *hi = z;
}

// the used mask of column c from the curves of chain 0, sample_used's rule; the Rayleigh and the Love data counted apart
DSA_CS unsigned long long sample_radial_used(const SampleRadialView& S, long long c, int* nused_r, int* nused_l)
{
    unsigned long long used = 0ull;
    int nr = 0, nl = 0;
    for (int k = 0; k < S.K; ++k) {
        const float o = S.obs[(long long)k * S.ncol + c], w = S.wt ? S.wt[(long long)k * S.ncol + c] : 1.0f;
        const double p = S.pv[(long long)k * S.ncol + c];
        if (w > 0.0f && o > 0.0f && p > 0.0) {
            used |= 1ull << k;
            if ((S.love >> k) & 1ull) ++nl; else ++nr;
        }
    }
    *nused_r = nr; *nused_l = nl;
    return used;
}

// phi of chain q over the used data, sample_phi's arithmetic
DSA_CS double sample_radial_phi(const SampleRadialView& S, long long c, int q, unsigned long long used, bool* noroot)
{
    double phi = 0.0;
    bool bad = false;
    for (int k = 0; k < S.K; ++k) {
        if (!((used >> k) & 1ull)) continue;
        const double p = S.pv[((long long)q * S.K + k) * S.ncol + c];
        if (!(p > 0.0)) { bad = true; continue; }
        const double a = S.wt ? (double)S.wt[(long long)k * S.ncol + c] : 1.0;
        const double r = (double)S.obs[(long long)k * S.ncol + c] - p;
        const double rho = a * r;
        phi += rho * rho;
    }
    *noroot = bad;
    return phi;
}

// psi of chain q: the two models' roughness and the tie
DSA_CS double sample_radial_psi(const SampleRadialView& S, long long c, int q)
{
    const int M = S.nz - 1;
    const long long stride = (long long)S.C * S.ncol, e0 = sample_radial_node(S, c, q, 0);
    const double pv = sample_psi(M, S.lam2, S.vv + e0, stride), ph = sample_psi(M, S.lam2, S.vh + e0, stride);
    double s = 0.0;
    for (int l = 0; l < M; ++l) {
        const double t = (double)S.vh[e0 + l * stride] - (double)S.vv[e0 + l * stride];
        s += t * t;
    }
    return (pv + ph) + S.gam2 * s;
}

// the set-up before its dispersion runs: both stores of every chain, every figure of the state cleared
DSA_CS void sample_radial_setup_models(const SampleRadialView& S, long long c, int q)
{
    const int M = S.nz - 1;
    const bool moves = q > 0 && sample_interior(S.nx, S.ny, c);
    for (int b = 0; b < 2; ++b) {
        const float* v0 = b ? S.v0h : S.v0v;
        float* v = b ? S.vh : S.vv;
        for (int l = 0; l < S.nz; ++l) {
            const float s = v0[(long long)l * S.ncol + c];
            float x = s;
            if (moves && l < M) {
                const double u = sample_unit(sample_bits(S.seed, (unsigned long long)c, (unsigned long long)q, 0ull, (unsigned long long)(b * M + l)));
                float lo, hi;
                sample_radial_box(S, s, &lo, &hi);
                x = x + (float)(S.spread * (2.0 * u - 1.0));
                if (x < lo) x = lo;
                if (x > hi) x = hi;
            }
            v[sample_radial_node(S, c, q, l)] = x;
        }
    }
    const long long at = sample_radial_at(S, c, q), stride = (long long)S.C * S.ncol;
    S.phi[at] = 0.0; S.psi[at] = 0.0; S.phisum[at] = 0.0; S.nkept[at] = 0; S.best_e[at] = 0.0;
    S.pnode[at] = 0; S.pold_v[at] = 0.0f; S.pold_h[at] = 0.0f; S.pmark[at] = kSampleIdle; S.reseed[at] = 0;
    for (int w = 0; w < kSampleCounters; ++w) S.cnt[w * stride + at] = 0;
    for (int w = 0; w < kSampleKindCounters; ++w) S.kcnt[w * stride + at] = 0;
    for (int l = 0; l < M; ++l) {
        const long long e = sample_radial_node(S, c, q, l);
        S.S1v[e] = 0.0; S.S2v[e] = 0.0; S.S1h[e] = 0.0; S.S2h[e] = 0.0; S.Pvh[e] = 0.0; S.X1[e] = 0.0; S.X2[e] = 0.0; S.npos[e] = 0;
        S.best_vv[e] = 0.0f; S.best_vh[e] = 0.0f;
    }
    if (q == 0) { S.used[c] = 0ull; S.nused_r[c] = 0; S.nused_l[c] = 0; S.flag[c] = kColumnOk; S.phi0[c] = 0.0; }
}

DSA_CS void sample_radial_to_start(const SampleRadialView& S, long long c, int q)
{
    for (int l = 0; l < S.nz - 1; ++l) {
        S.vv[sample_radial_node(S, c, q, l)] = S.v0v[(long long)l * S.ncol + c];
        S.vh[sample_radial_node(S, c, q, l)] = S.v0h[(long long)l * S.ncol + c];
    }
}

// the set-up after its dispersion runs (sample_setup_state's rules).  The ring is left alone.
DSA_CS void sample_radial_setup_state(const SampleRadialView& S, long long c, int q)
{
    if (!sample_interior(S.nx, S.ny, c)) return;
    const long long at = sample_radial_at(S, c, q);
    int nr = 0, nl = 0;
    const unsigned long long used = sample_radial_used(S, c, &nr, &nl);
    const int nused = nr + nl;
    bool noroot = false;
    const double phi_start = nused ? sample_radial_phi(S, c, 0, used, &noroot) : 0.0;
    if (q == 0) { S.used[c] = used; S.nused_r[c] = nr; S.nused_l[c] = nl; S.flag[c] = nused ? kColumnOk : kColumnNoData; S.phi0[c] = phi_start; }
    if (nused == 0) { sample_radial_to_start(S, c, q); return; }
    double phi = q == 0 ? phi_start : sample_radial_phi(S, c, q, used, &noroot);
    if (noroot) {
        sample_radial_to_start(S, c, q);
        S.reseed[at] = 1;
        phi = phi_start;
    }
    S.phi[at] = phi;
    S.psi[at] = sample_radial_psi(S, c, q);
}

DSA_CS bool sample_radial_idle(const SampleRadialView& S, long long c) { return !sample_interior(S.nx, S.ny, c) || S.flag[c] != kColumnOk; }

// the proposal of sweep `sweep` (>= 1), before its dispersion runs
DSA_CS void sample_radial_propose(const SampleRadialView& S, long long c, int q, int sweep)
{
    const long long at = sample_radial_at(S, c, q);
    if (sample_radial_idle(S, c)) { S.pmark[at] = kSampleIdle; return; }
    const int M = S.nz - 1, n = (S.pairs ? 3 : 2) * M;
    const double u0 = sample_unit(sample_bits(S.seed, (unsigned long long)c, (unsigned long long)q, (unsigned long long)sweep, 0ull));
    const double u1 = sample_unit(sample_bits(S.seed, (unsigned long long)c, (unsigned long long)q, (unsigned long long)sweep, 1ull));
    int i = (int)(u0 * (double)n);
    if (i > n - 1) i = n - 1;
    const int kind = i / M, l = i - kind * M;
    const float fd = (float)(S.step * (2.0 * u1 - 1.0));
    const long long e = sample_radial_node(S, c, q, l);
    const float old_v = S.vv[e], old_h = S.vh[e];
    const float new_v = old_v + fd, new_h = old_h + fd;
    S.kcnt[(long long)kind * S.C * S.ncol + at] += 1;
    bool outside = false;
    float lo, hi;
    if (kind != kSampleKindVsh) {
        sample_radial_box(S, S.v0v[(long long)l * S.ncol + c], &lo, &hi);
        if (new_v < lo || new_v > hi) outside = true;
    }
    if (kind != kSampleKindVsv) {
        sample_radial_box(S, S.v0h[(long long)l * S.ncol + c], &lo, &hi);
        if (new_h < lo || new_h > hi) outside = true;
    }
    if (outside) { S.pmark[at] = kSampleOutOfBox; return; }
    S.pnode[at] = i; S.pold_v[at] = old_v; S.pold_h[at] = old_h;
    if (kind != kSampleKindVsh) S.vv[e] = new_v;
    if (kind != kSampleKindVsv) S.vh[e] = new_h;
    S.pmark[at] = kSamplePending;
}

// the Metropolis test of sweep `sweep` after its dispersion runs, and the sweep's share of the moments
DSA_CS void sample_radial_accept(const SampleRadialView& S, long long c, int q, int sweep)
{
    const long long at = sample_radial_at(S, c, q);
    const int mark = S.pmark[at];
    if (mark == kSampleIdle) return;
    const int M = S.nz - 1;
    const long long stride = (long long)S.C * S.ncol;
    int* cnt = S.cnt + at;
    if (mark == kSampleOutOfBox) {
        cnt[kSampleCntOutOfBox * stride] += 1; cnt[kSampleCntRejected * stride] += 1;
    } else {
        const int kind = S.pnode[at] / M, l = S.pnode[at] - kind * M;
        bool noroot = false;
        const double phi_new = sample_radial_phi(S, c, q, S.used[c], &noroot);
        bool accepted = false;
        double psi_new = 0.0;
        if (!noroot) {
            psi_new = sample_radial_psi(S, c, q);
            const double delta = (phi_new + psi_new) - (S.phi[at] + S.psi[at]);
            if (delta == delta) {
                if (delta <= 0.0) accepted = true;
                else {
                    const unsigned long long k = sample_bits(S.seed, (unsigned long long)c, (unsigned long long)q, (unsigned long long)sweep, 2ull);
                    accepted = k == 0ull || delta / S.two_t < sample_neglog(k);
                }
            }
        }
        if (accepted) {
            S.phi[at] = phi_new; S.psi[at] = psi_new;
            cnt[kSampleCntAccepted * stride] += 1;
            S.kcnt[(kSampleKinds + kind) * stride + at] += 1;
            S.pmark[at] = kSampleAccepted;
        } else {
            const long long e = sample_radial_node(S, c, q, l);
            if (kind != kSampleKindVsh) S.vv[e] = S.pold_v[at];
            if (kind != kSampleKindVsv) S.vh[e] = S.pold_h[at];
            cnt[kSampleCntRejected * stride] += 1;
            if (noroot) cnt[kSampleCntNoRoot * stride] += 1;
            S.pmark[at] = noroot ? kSampleNoRoot : kSampleRejected;
        }
    }
    if (sweep <= S.burn) return;
    for (int l = 0; l < M; ++l) {
        const long long e = sample_radial_node(S, c, q, l);
        const float fv = S.vv[e], fh = S.vh[e];
        const double s_v = (double)S.v0v[(long long)l * S.ncol + c], s_h = (double)S.v0h[(long long)l * S.ncol + c];
        const double dv = (double)fv - s_v, dh = (double)fh - s_h;
        S.S1v[e] += dv; S.S2v[e] += dv * dv;
        S.S1h[e] += dh; S.S2h[e] += dh * dh;
        S.Pvh[e] += dv * dh;
        const double x = (double)fh / (double)fv, x0 = s_h / s_v;
        const double dx = x * x - x0 * x0;
        S.X1[e] += dx; S.X2[e] += dx * dx;
        if (fh > fv) S.npos[e] += 1;
    }
    const double energy = S.phi[at] + S.psi[at];
    S.phisum[at] += S.phi[at];
    if (S.nkept[at] == 0 || energy < S.best_e[at]) {
        S.best_e[at] = energy;
        for (int l = 0; l < M; ++l) {
            const long long e = sample_radial_node(S, c, q, l);
            S.best_vv[e] = S.vv[e]; S.best_vh[e] = S.vh[e];
        }
    }
    S.nkept[at] += 1;
}

// sample_finish's four figures of one quantity at (column c, depth l) from its sums s1, s2 (M, C, ncol): out[0 .. 3] the pooled mean offset,
// the pooled variance, W, B; chains ascending, every sum from 0.0; n > 0
DSA_CS void sample_radial_pool(const SampleRadialView& S, long long c, int l, int n, const double* s1, const double* s2, double* pm_out, double* var, double* W,
                               double* B)
{
    const int C = S.C;
    const double dn = (double)n, dc = (double)C;
    double a1 = 0.0, a2 = 0.0, sw = 0.0, sm = 0.0;
    for (int q = 0; q < C; ++q) {
        const long long e = sample_radial_node(S, c, q, l);
        const double m = s1[e] / dn;
        a1 += s1[e];
        a2 += s2[e];
        sw += s2[e] / dn - m * m;
        sm += m;
    }
    const double pm = a1 / (dn * dc), mbar = sm / dc;
    double sb = 0.0;
    for (int q = 0; q < C; ++q) {
        const double d = s1[sample_radial_node(S, c, q, l)] / dn - mbar;
        sb += d * d;
    }
    *pm_out = pm;
    *var = a2 / (dn * dc) - pm * pm;
    *W = sw / dc;
    *B = C > 1 ? sb / (dc - 1.0) : 0.0;
}

// The finish of (column c, depth l < M), sample_finish's formulas on each of Vsv, Vsh and xi.  nodes (16, M, ncol): mean, variance, W, B of
// Vsv, of Vsh and of xi (a mean is the start's value -- v0v, v0h, xi0 = (v0h / v0v)^2 -- plus the pooled offset), the best model's Vsv and
// Vsh (the chain with the smallest best phi + psi, the first at a tie), the pooled covariance sum Pvh / (n C) - m_v m_h, the share sum npos /
// (n C).  The thread of l = 0 also writes cols (3, ncol): phi of the start, the best phi + psi, the mean kept phi; and counts (15, ncol):
// nused_r, nused_l, flag, the four counters and the six kind counters summed over the chains, reseeded, nkept.  Without a kept sweep every
// figure of nodes, the best phi + psi and the mean kept phi are 0.
DSA_CS void sample_radial_finish(const SampleRadialView& S, long long c, int l, double* nodes, double* cols, int* counts)
{
    const int M = S.nz - 1, C = S.C;
    const int n = S.nkept[sample_radial_at(S, c, 0)];
    const double dn = (double)n, dc = (double)C;
    const long long fs = (long long)M * S.ncol, at = (long long)l * S.ncol + c;      // figure f of the node at nodes[f * fs + at]
    int best_q = 0;
    for (int q = 1; q < C; ++q)
        if (S.best_e[sample_radial_at(S, c, q)] < S.best_e[sample_radial_at(S, c, best_q)]) best_q = q;
    if (n > 0) {
        double pmv, pmh, pmx, var, W, B;
        sample_radial_pool(S, c, l, n, S.S1v, S.S2v, &pmv, &var, &W, &B);
        const double s_v = (double)S.v0v[at], s_h = (double)S.v0h[at];
        nodes[kSrMeanV * fs + at] = s_v + pmv; nodes[kSrVarV * fs + at] = var; nodes[kSrWV * fs + at] = W; nodes[kSrBV * fs + at] = B;
        sample_radial_pool(S, c, l, n, S.S1h, S.S2h, &pmh, &var, &W, &B);
        nodes[kSrMeanH * fs + at] = s_h + pmh; nodes[kSrVarH * fs + at] = var; nodes[kSrWH * fs + at] = W; nodes[kSrBH * fs + at] = B;
        sample_radial_pool(S, c, l, n, S.X1, S.X2, &pmx, &var, &W, &B);
        const double x0 = s_h / s_v;
        nodes[kSrMeanX * fs + at] = x0 * x0 + pmx; nodes[kSrVarX * fs + at] = var; nodes[kSrWX * fs + at] = W; nodes[kSrBX * fs + at] = B;
        double sp = 0.0;
        long long np = 0;
        for (int q = 0; q < C; ++q) {
            sp += S.Pvh[sample_radial_node(S, c, q, l)];
            np += S.npos[sample_radial_node(S, c, q, l)];
        }
        nodes[kSrBestV * fs + at] = (double)S.best_vv[sample_radial_node(S, c, best_q, l)];
        nodes[kSrBestH * fs + at] = (double)S.best_vh[sample_radial_node(S, c, best_q, l)];
        nodes[kSrCov * fs + at] = sp / (dn * dc) - pmv * pmh;
        nodes[kSrShare * fs + at] = (double)np / (dn * dc);
    } else {
        for (int f = 0; f < kSrNodeFigures; ++f) nodes[f * fs + at] = 0.0;
    }
    if (l != 0) return;
    double phis = 0.0;
    int reseeded = 0;
    for (int q = 0; q < C; ++q) {
        reseeded += S.reseed[sample_radial_at(S, c, q)];
        phis += S.phisum[sample_radial_at(S, c, q)];
    }
    for (int w = 0; w < kSampleCounters; ++w) {
        int s = 0;
        for (int q = 0; q < C; ++q) s += S.cnt[((long long)w * C + q) * S.ncol + c];
        counts[(kSrSumAccepted + w) * S.ncol + c] = s;
    }
    for (int w = 0; w < kSampleKindCounters; ++w) {
        int s = 0;
        for (int q = 0; q < C; ++q) s += S.kcnt[((long long)w * C + q) * S.ncol + c];
        counts[(kSrSumKinds + w) * S.ncol + c] = s;
    }
    cols[kSamplePhiStart * S.ncol + c] = S.phi0[c];
    cols[kSampleBestE * S.ncol + c] = n > 0 ? S.best_e[sample_radial_at(S, c, best_q)] : 0.0;
    cols[kSampleMeanPhi * S.ncol + c] = n > 0 ? phis / (dn * dc) : 0.0;
    counts[kSrNusedR * S.ncol + c] = S.nused_r[c];
    counts[kSrNusedL * S.ncol + c] = S.nused_l[c];
    counts[kSrFlag * S.ncol + c] = S.flag[c];
    counts[kSrReseeded * S.ncol + c] = reseeded;
    counts[kSrNkept * S.ncol + c] = n;
}

}  // namespace dsa
