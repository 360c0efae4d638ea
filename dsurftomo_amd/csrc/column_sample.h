// Monte-Carlo depth inversion of the period maps: C Metropolis chains per column of Vs(z), M = nz - 1 unknowns (the
// bottom depth is kept), K data in slot order.  The chains are the models of a multi-model dispersion stage; this header is the rest of a
// sweep -- the proposal, the misfit, the prior, the Metropolis test, the running moments -- and the finish.
//
//   box       per depth, fp32: lo_l = max(minvel, v0_l - width), hi_l = min(maxvel, v0_l + width)
//   numbers   counter-based: x = seed; for w in (column, chain, sweep, draw): x = mix(x + 0x9E3779B97F4A7C15 + w), mix splitmix64's
//             finaliser; k = x >> 11, u = k 2^-53 (exact).  Sweep 0 is the set-up (draw = the depth), the sweeps count from 1
//             (draw 0: the node, 1: the step, 2: the Metropolis test)
//   neglog    sample_neglog(k) = -ln(k 2^-53), k >= 1: exponent and mantissa by integer operations, the mantissa m in [sqrt(1/2), sqrt(2)),
//             ln m = 2 s (1 + s^2/3 + ... + s^22/23), s = (m - 1) / (m + 1), eleven terms whatever k; plain fp64, no libm
//   used      decided once per column on chain 0's curves at the set-up: wt_k > 0, obs_k > 0 and pv_k > 0.  nused = 0: flag 2, never moved
//   data      a_k = (double)wt_k, r_k = (double)obs_k - pv_k, rho_k = a_k r_k, phi = sum rho_k^2 over the used k ascending, from 0.0
//   prior     psi = (double)smooth^2 sum_rows (L v)^2_row, column_system.h's L, v in double; a row is summed from 0.0 over its unknowns
//             ascending; the rows in order: top, the centred rows 1 .. M-2, bottom
//   proposal  l = min((int)(u M), M - 1), delta = step (2u - 1), v' = v_l + (float)delta in fp32; outside [lo_l, hi_l]: nothing is written
//   accept    any used pv <= 0 (or NaN): no root, rejected.  Delta = (phi' + psi') - (phi + psi); accepted when Delta is not NaN and
//             (Delta <= 0 or k == 0 or Delta / (2 temperature) < sample_neglog(k)); a rejection puts the node's old value back
//   moments   in the sweeps after burn, per chain and depth: d = (double)v_l - (double)v0_l, S1 += d, S2 += d d; phisum += phi, nkept += 1;
//             the smallest phi + psi of the kept sweeps and its model (the first one wins a tie)
//   finish    per (column, depth), chains ascending -- see sample_finish
//
// Block proposals, switched on beside the above by a SampleBlockView; without one, or with block_every = 0, every bit is
// the above's:
//   shape     per column, once: column_system.h's column_assemble and column_factor on the column's curve and combined depth kernels, N = G^T G
//             + smooth^2 L^T L + damp^2 I = L D L^T; kept: the packed triangle as column_factor leaves it (N's diagonal, L below it),
//             r_l = sample_rsqrt(d_l), the flag (dsa_columns_step's: 2 without a used datum, 1 at a bad pivot; then tri and r stay 0)
//   rsqrt     sample_rsqrt(d) = 1 / sqrt(d): the exponent halved by integer operations, a seed from the mantissa's bits, six Newton steps
//             whatever d; plain fp64, no libm
//   kind      sweep s >= 1 is a block sweep iff block_every > 0 and s % block_every == 0; in one, a chain of a column whose shape flag is 0
//             makes a block proposal, any other chain the single-node proposal above
//   block     draws 3 + l: z_l = 2u - 1, y_l = z_l r_l; L^T delta = y by column_solve's back substitution (i descending, the terms p = i+1 ..
//             M-1 subtracted ascending); v'_l = v_l + (float)(block_scale delta_l) in fp32.  Any v'_l outside its box: only the mark is
//             written.  Else pold_all gets the M old values, v the M new ones, pnode = -1.  The Metropolis test is the one above (draw 2);
//             a rejection puts all M values back.  Block counters (3, chain, column): proposed, accepted, out of box
//
// Posterior marginals, switched on beside the above by a SampleMarginalView; they observe the kept sweeps and write
// nothing of the above:
//   bin       of a value v at depth l: dlo = (double)lo_l, w = (double)hi_l - dlo; w <= 0 (or NaN): bin 0; else x = (((double)v - dlo) / w)
//             nbins, b = 0 for x < 0, nbins - 1 for x >= nbins, else (int)x (chain 0 starts at the unclipped start: an end bin)
//   counts    where the moments are taken (a chain that is not idle, a sweep after burn, the Metropolis test settled): hist (bin, depth,
//             chain, column) += 1 for every depth; with the covariance P (column_tri(i, j), chain, column) += d_i d_j, j <= i, d the
//             moments' own: P's diagonal has the bits of S2
//   finish    per (column, depth): the pooled counts, the mode, the quantiles -- see sample_marginal_finish; per (column, triangle entry):
//             the pooled covariance -- see sample_marginal_cov_finish
// One thread per counter or sum (k_sample_hist: (depth, chain, column); k_sample_cov: (entry, chain, column)), launched after the sweep's
// Metropolis test.
//
// fp64 under -ffp-contract=off, no square root, IEEE division: one value per figure whatever computes it.  One thread per (column, chain)
// (column_kernels.hip: k_sample_*) or a loop over them (tests/hostcheck_column_sample.cpp); a thread's sums are its own sequential chains and
// no thread reads what another writes in the same launch, so the mapping cannot change a bit.
// Layouts, column fastest everywhere: models and S1 / S2 / bestv (depth, chain, column); the maps (chain, map, column); obs / wt (map,
// column); per-chain figures (chain, column); counters (4, chain, column): accepted, rejected (of any kind), out of box, no root.
#pragma once

#include "column_system.h"

namespace dsa {

// what the last sweep did with a chain's proposal
enum { kSampleIdle = -1, kSamplePending = 0, kSampleOutOfBox = 1, kSampleAccepted = 2, kSampleRejected = 3, kSampleNoRoot = 4 };
enum { kSampleCntAccepted = 0, kSampleCntRejected = 1, kSampleCntOutOfBox = 2, kSampleCntNoRoot = 3, kSampleCounters = 4 };
enum { kSampleBlkProposed = 0, kSampleBlkAccepted = 1, kSampleBlkOutOfBox = 2, kSampleBlockCounters = 3 };
// the finish: per (column, depth) five doubles, per column three doubles and eight ints
enum { kSampleMean = 0, kSampleVar = 1, kSampleW = 2, kSampleB = 3, kSampleBest = 4, kSampleNodeFigures = 5 };
enum { kSamplePhiStart = 0, kSampleBestE = 1, kSampleMeanPhi = 2, kSampleColumnFigures = 3 };
enum { kSampleNused = 0, kSampleFlag = 1, kSampleSumAccepted = 2, kSampleSumRejected = 3, kSampleSumOutOfBox = 4, kSampleSumNoRoot = 5, kSampleReseeded = 6,
       kSampleNkept = 7, kSampleColumnCounts = 8 };

// the whole state of a sample stage and its inputs, where they lie
struct SampleView {
    int nx, ny, nz, K, C, burn;
    long long ncol;
    unsigned long long seed;
    double lam2, step, spread, two_t;                  // smooth^2, step, spread, 2 temperature
    float width, minvel, maxvel;
    const float* obs; const float* wt;                 // (K, ncol); wt may be null (1)
    const float* v0;                                   // (nz, ncol): the start model
    const double* pv;                                  // (C, K, ncol): the stage's map store
    float* v;                                          // (nz, C, ncol): the stage's model store
    double* phi; double* psi;                          // (C, ncol)
    int* cnt;                                          // (4, C, ncol)
    double* S1; double* S2;                            // (M, C, ncol)
    double* phisum; int* nkept;                        // (C, ncol)
    double* best_e; float* best_v;                     // (C, ncol), (M, C, ncol)
    int* pnode; float* pold; int* pmark;               // (C, ncol): the last sweep's proposal
    int* reseed;                                       // (C, ncol): 1 where the set-up put the chain back to the start
    unsigned long long* used;                          // (ncol): bit k set where datum k is used
    int* nused; int* flag;                             // (ncol)
    double* phi0;                                      // (ncol): phi of the start
};

// the block proposals' state, passed beside the view: the shape of every column and what a block sweep keeps
struct SampleBlockView {
    const double* tri;                                 // (column_tri_size(M), ncol): N's diagonal, L below it, column_tri's order
    const double* r;                                   // (M, ncol): r_l = sample_rsqrt(d_l)
    const int* flag;                                   // (ncol): the shape's flag
    float* pold_all;                                   // (M, C, ncol): the values a block proposal replaced
    int* cnt;                                          // (3, C, ncol): block proposals made, accepted, out of the box
    int block_every;                                   // 0: no block sweeps
    double block_scale;
};

// the posterior marginals' state, passed beside the view while they are switched on
struct SampleMarginalView {
    int nbins;                                         // 2 .. 256: equal bins of every node's box
    unsigned* hist;                                    // (nbins, M, C, ncol): the kept sweeps of a chain per bin
    double* P;                                         // (column_tri_size(M), C, ncol): sum of d_i d_j over the kept sweeps, j <= i; null: no covariance
};

DSA_CS unsigned long long sample_mix(unsigned long long x)
{
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// the 53 bits of draw (column, chain, sweep, draw)
DSA_CS unsigned long long sample_bits(unsigned long long seed, unsigned long long column, unsigned long long chain, unsigned long long sweep, unsigned long long draw)
{
    unsigned long long x = seed;
    x = sample_mix(x + 0x9E3779B97F4A7C15ull + column);
    x = sample_mix(x + 0x9E3779B97F4A7C15ull + chain);
    x = sample_mix(x + 0x9E3779B97F4A7C15ull + sweep);
    x = sample_mix(x + 0x9E3779B97F4A7C15ull + draw);
    return x >> 11;
}

// u = k 2^-53, exact: k < 2^53
DSA_CS double sample_unit(unsigned long long k) { return (double)k * 1.1102230246251565404e-16; }

DSA_CS double sample_from_bits(unsigned long long b)
{
    double d;
    __builtin_memcpy(&d, &b, sizeof d);
    return d;
}

// -ln(k 2^-53) for 1 <= k < 2^53
DSA_CS double sample_neglog(unsigned long long k)
{
    const int p = 63 - __builtin_clzll(k);                                      // the top bit: k = 1.f x 2^p
    const unsigned long long frac = (k << (52 - p)) & 0x000FFFFFFFFFFFFFull;    // f, 52 bits
    int n = p - 53;
    unsigned long long ex = 1023ull;
    if (frac > 0x0006A09E667F3BCCull) { ex = 1022ull; n += 1; }                 // m > sqrt(2): halve it
    const double m = sample_from_bits((ex << 52) | frac);
    const double s = (m - 1.0) / (m + 1.0), z = s * s;
    double t = 1.0 / 23.0;
    t = t * z + 1.0 / 21.0;
    t = t * z + 1.0 / 19.0;
    t = t * z + 1.0 / 17.0;
    t = t * z + 1.0 / 15.0;
    t = t * z + 1.0 / 13.0;
    t = t * z + 1.0 / 11.0;
    t = t * z + 1.0 / 9.0;
    t = t * z + 1.0 / 7.0;
    t = t * z + 1.0 / 5.0;
    t = t * z + 1.0 / 3.0;
    t = t * z + 1.0;
    const double lnm = 2.0 * s * t, dn = (double)n;
    const double r = dn * 6.93147180369123816490e-01 + (lnm + dn * 1.90821492927058770002e-10);      // ln 2 in two parts
    return -r;
}

// 1 / sqrt(d) for a normal positive finite d.  d = m 4^h with m in [1, 4) by integer operations on the exponent; the seed is the bits of m
// halved and taken from a constant (relative error below 3.5 %), six Newton steps y = y (1.5 - (m / 2) y y) whatever d (the fourth is at
// rounding level already), the result y 2^-h, an exact scaling.  Within 1e-15 relative of 1 / math.sqrt(d) (measured: tests/
// test_hostcheck_column_sample_block.py); its last bit is not claimed, only that it is the same whatever computes it.  Outside that range
// the sign is ignored, a zero or subnormal is read as if it had the hidden bit, an infinity or NaN as a number of exponent 1024: a finite
// positive value that is not 1 / sqrt(d).  column_factor's pivots are finite and > 0.
DSA_CS double sample_rsqrt(double d)
{
    unsigned long long b;
    __builtin_memcpy(&b, &d, sizeof b);
    const int e = (int)((b >> 52) & 0x7FFull) - 1023, odd = e & 1, h = (e - odd) / 2;
    const unsigned long long mb = ((unsigned long long)(1023 + odd) << 52) | (b & 0x000FFFFFFFFFFFFFull);
    const double m = sample_from_bits(mb), hm = 0.5 * m;
    double y = sample_from_bits(0x5FE6EB50C7B537A9ull - (mb >> 1));
    y = y * (1.5 - hm * y * y);
    y = y * (1.5 - hm * y * y);
    y = y * (1.5 - hm * y * y);
    y = y * (1.5 - hm * y * y);
    y = y * (1.5 - hm * y * y);
    y = y * (1.5 - hm * y * y);
    return y * sample_from_bits((unsigned long long)(1023 - h) << 52);
}

DSA_CS bool sample_interior(int nx, int ny, long long c)
{
    const int j = (int)(c / nx), i = (int)(c - (long long)j * nx);
    return i >= 1 && i <= nx - 2 && j >= 1 && j <= ny - 2;
}

DSA_CS long long sample_at(const SampleView& S, long long c, int q) { return (long long)q * S.ncol + c; }
DSA_CS long long sample_node(const SampleView& S, long long c, int q, int l) { return ((long long)l * S.C + q) * S.ncol + c; }

DSA_CS void sample_box(const SampleView& S, long long c, int l, float* lo, float* hi)
{
    const float b = S.v0[(long long)l * S.ncol + c];
    float a = b - S.width, z = b + S.width;
    if (a < S.minvel) a = S.minvel;
    if (z > S.maxvel) z = S.maxvel;
    *lo = a; *hi = z;
}

// the used mask of column c from the curves of chain 0
DSA_CS unsigned long long sample_used(const SampleView& S, long long c, int* nused)
{
    unsigned long long used = 0ull;
    int n = 0;
    for (int k = 0; k < S.K; ++k) {
        const float o = S.obs[(long long)k * S.ncol + c], w = S.wt ? S.wt[(long long)k * S.ncol + c] : 1.0f;
        const double p = S.pv[(long long)k * S.ncol + c];
        if (w > 0.0f && o > 0.0f && p > 0.0) { used |= 1ull << k; ++n; }
    }
    *nused = n;
    return used;
}

// phi of chain q over the used data; *noroot where a used datum has no root (the value returned is then not a misfit)
DSA_CS double sample_phi(const SampleView& S, long long c, int q, unsigned long long used, bool* noroot)
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

// psi of the M values v[l * stride]
DSA_CS double sample_psi(int M, double lam2, const float* v, long long stride)
{
    if (M < 2) return 0.0;
    double s = 0.0;
    {
        double t = 0.0;
        t += (double)v[0];
        t -= (double)v[stride];
        s += t * t;
    }
    for (int l = 1; l <= M - 2; ++l) {
        double t = 0.0;
        t -= (double)v[(l - 1) * stride];
        t += 2.0 * (double)v[l * stride];
        t -= (double)v[(l + 1) * stride];
        s += t * t;
    }
    {
        double t = 0.0;
        t -= (double)v[(M - 2) * stride];
        t += (double)v[(M - 1) * stride];
        s += t * t;
    }
    return lam2 * s;
}

// the set-up before its dispersion runs: chain 0 is the start, chain q > 0 the start spread by draws (c, q, 0, l) and clipped to the box; the
// ring's chains are all the start; the bottom depth is the start's; every figure of the state is cleared
DSA_CS void sample_setup_models(const SampleView& S, long long c, int q)
{
    const int M = S.nz - 1;
    const bool moves = q > 0 && sample_interior(S.nx, S.ny, c);
    for (int l = 0; l < S.nz; ++l) {
        float x = S.v0[(long long)l * S.ncol + c];
        if (moves && l < M) {
            const double u = sample_unit(sample_bits(S.seed, (unsigned long long)c, (unsigned long long)q, 0ull, (unsigned long long)l));
            float lo, hi;
            sample_box(S, c, l, &lo, &hi);
            x = x + (float)(S.spread * (2.0 * u - 1.0));
            if (x < lo) x = lo;
            if (x > hi) x = hi;
        }
        S.v[sample_node(S, c, q, l)] = x;
    }
    const long long at = sample_at(S, c, q);
    S.phi[at] = 0.0; S.psi[at] = 0.0; S.phisum[at] = 0.0; S.nkept[at] = 0; S.best_e[at] = 0.0;
    S.pnode[at] = 0; S.pold[at] = 0.0f; S.pmark[at] = kSampleIdle; S.reseed[at] = 0;
    for (int w = 0; w < kSampleCounters; ++w) S.cnt[((long long)w * S.C + q) * S.ncol + c] = 0;
    for (int l = 0; l < M; ++l) { S.S1[sample_node(S, c, q, l)] = 0.0; S.S2[sample_node(S, c, q, l)] = 0.0; S.best_v[sample_node(S, c, q, l)] = 0.0f; }
    if (q == 0) { S.used[c] = 0ull; S.nused[c] = 0; S.flag[c] = kColumnOk; S.phi0[c] = 0.0; }
}

// the set-up after its dispersion runs: the used mask from chain 0's curves (every chain of the column computes the same; chain 0 stores
// it), phi and psi of the chain; a chain with a used datum without a root goes back to the start with chain 0's phi and psi; a column
// without a used datum is flagged and all its chains go back to the start.  The ring is left alone.
DSA_CS void sample_setup_state(const SampleView& S, long long c, int q)
{
    if (!sample_interior(S.nx, S.ny, c)) return;
    const int M = S.nz - 1;
    const long long at = sample_at(S, c, q);
    int nused = 0;
    const unsigned long long used = sample_used(S, c, &nused);
    bool noroot = false;
    const double phi_start = nused ? sample_phi(S, c, 0, used, &noroot) : 0.0;
    if (q == 0) { S.used[c] = used; S.nused[c] = nused; S.flag[c] = nused ? kColumnOk : kColumnNoData; S.phi0[c] = phi_start; }
    if (nused == 0) {
        for (int l = 0; l < M; ++l) S.v[sample_node(S, c, q, l)] = S.v0[(long long)l * S.ncol + c];
        return;
    }
    double phi = q == 0 ? phi_start : sample_phi(S, c, q, used, &noroot);
    if (noroot) {
        for (int l = 0; l < M; ++l) S.v[sample_node(S, c, q, l)] = S.v0[(long long)l * S.ncol + c];
        S.reseed[at] = 1;
        phi = phi_start;
    }
    S.phi[at] = phi;
    S.psi[at] = sample_psi(M, S.lam2, S.v + sample_node(S, c, q, 0), (long long)S.C * S.ncol);
}

// a chain that is never moved: the ring's and a flagged column's
DSA_CS bool sample_idle(const SampleView& S, long long c) { return !sample_interior(S.nx, S.ny, c) || S.flag[c] != kColumnOk; }

// the proposal of sweep `sweep` (>= 1), before its dispersion runs
DSA_CS void sample_propose(const SampleView& S, long long c, int q, int sweep)
{
    const long long at = sample_at(S, c, q);
    if (sample_idle(S, c)) { S.pmark[at] = kSampleIdle; return; }
    const int M = S.nz - 1;
    const double u0 = sample_unit(sample_bits(S.seed, (unsigned long long)c, (unsigned long long)q, (unsigned long long)sweep, 0ull));
    const double u1 = sample_unit(sample_bits(S.seed, (unsigned long long)c, (unsigned long long)q, (unsigned long long)sweep, 1ull));
    int l = (int)(u0 * (double)M);
    if (l > M - 1) l = M - 1;
    const double delta = S.step * (2.0 * u1 - 1.0);
    const float old = S.v[sample_node(S, c, q, l)];
    const float x = old + (float)delta;
    float lo, hi;
    sample_box(S, c, l, &lo, &hi);
    S.pnode[at] = l; S.pold[at] = old;
    if (x < lo || x > hi) { S.pmark[at] = kSampleOutOfBox; return; }
    S.v[sample_node(S, c, q, l)] = x;
    S.pmark[at] = kSamplePending;
}

// a block sweep, and a chain that makes a block proposal in it
DSA_CS bool sample_block_sweep(const SampleBlockView& B, int sweep) { return B.block_every > 0 && sweep % B.block_every == 0; }
DSA_CS bool sample_block_chain(const SampleBlockView& B, long long c, int sweep) { return sample_block_sweep(B, sweep) && B.flag[c] == kColumnOk; }

// the proposal of sweep `sweep` (>= 1) where block proposals are switched on: the block proposal of a chain of a column with a shape in a
// block sweep, the single-node proposal above for every other
DSA_CS void sample_propose_block(const SampleView& S, const SampleBlockView& B, long long c, int q, int sweep)
{
    const long long at = sample_at(S, c, q);
    if (sample_idle(S, c)) { S.pmark[at] = kSampleIdle; return; }
    if (!sample_block_chain(B, c, sweep)) { sample_propose(S, c, q, sweep); return; }
    const int M = S.nz - 1;
    double delta[kColumnMaxM];
    for (int i = M - 1; i >= 0; --i) {
        const double u = sample_unit(sample_bits(S.seed, (unsigned long long)c, (unsigned long long)q, (unsigned long long)sweep, (unsigned long long)(3 + i)));
        double s = (2.0 * u - 1.0) * B.r[(long long)i * S.ncol + c];
        for (int p = i + 1; p < M; ++p) s -= B.tri[(long long)column_tri(p, i) * S.ncol + c] * delta[p];
        delta[i] = s;
    }
    bool outside = false;
    for (int l = 0; l < M; ++l) {
        const float x = S.v[sample_node(S, c, q, l)] + (float)(B.block_scale * delta[l]);
        float lo, hi;
        sample_box(S, c, l, &lo, &hi);
        if (x < lo || x > hi) outside = true;
    }
    if (outside) { S.pmark[at] = kSampleOutOfBox; return; }
    for (int l = 0; l < M; ++l) {
        const long long e = sample_node(S, c, q, l);
        const float old = S.v[e];
        B.pold_all[e] = old;
        S.v[e] = old + (float)(B.block_scale * delta[l]);
    }
    S.pnode[at] = -1;
    S.pmark[at] = kSamplePending;
}

// the Metropolis test of sweep `sweep` after its dispersion runs, and the sweep's share of the moments.  Block: B is read, a chain that made
// a block proposal counts it in B's counters too and a rejection puts all its M values back; without Block, B is not looked at.
template <bool Block>
DSA_CS void sample_accept_any(const SampleView& S, const SampleBlockView* B, long long c, int q, int sweep)
{
    const long long at = sample_at(S, c, q);
    const int mark = S.pmark[at];
    if (mark == kSampleIdle) return;
    const int M = S.nz - 1;
    const long long stride = (long long)S.C * S.ncol;
    int* cnt = S.cnt + at;                      // counter w at cnt[w * stride]
    bool block = false;
    if (Block) block = sample_block_chain(*B, c, sweep);
    if (Block && block) B->cnt[kSampleBlkProposed * stride + at] += 1;
    if (mark == kSampleOutOfBox) {
        cnt[kSampleCntOutOfBox * stride] += 1; cnt[kSampleCntRejected * stride] += 1;
        if (Block && block) B->cnt[kSampleBlkOutOfBox * stride + at] += 1;
    } else {
        bool noroot = false;
        const double phi_new = sample_phi(S, c, q, S.used[c], &noroot);
        bool accepted = false;
        double psi_new = 0.0;
        if (!noroot) {
            psi_new = sample_psi(M, S.lam2, S.v + sample_node(S, c, q, 0), stride);
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
            S.pmark[at] = kSampleAccepted;
            if (Block && block) B->cnt[kSampleBlkAccepted * stride + at] += 1;
        } else {
            if (Block && block) {
                for (int l = 0; l < M; ++l) S.v[sample_node(S, c, q, l)] = B->pold_all[sample_node(S, c, q, l)];
            } else {
                S.v[sample_node(S, c, q, S.pnode[at])] = S.pold[at];
            }
            cnt[kSampleCntRejected * stride] += 1;
            if (noroot) cnt[kSampleCntNoRoot * stride] += 1;
            S.pmark[at] = noroot ? kSampleNoRoot : kSampleRejected;
        }
    }
    if (sweep <= S.burn) return;
    for (int l = 0; l < M; ++l) {
        const long long e = sample_node(S, c, q, l);
        const double d = (double)S.v[e] - (double)S.v0[(long long)l * S.ncol + c];
        S.S1[e] += d;
        S.S2[e] += d * d;
    }
    const double energy = S.phi[at] + S.psi[at];
    S.phisum[at] += S.phi[at];
    if (S.nkept[at] == 0 || energy < S.best_e[at]) {
        S.best_e[at] = energy;
        for (int l = 0; l < M; ++l) S.best_v[sample_node(S, c, q, l)] = S.v[sample_node(S, c, q, l)];
    }
    S.nkept[at] += 1;
}

DSA_CS void sample_accept(const SampleView& S, long long c, int q, int sweep) { sample_accept_any<false>(S, nullptr, c, q, sweep); }
DSA_CS void sample_accept_block(const SampleView& S, const SampleBlockView& B, long long c, int q, int sweep) { sample_accept_any<true>(S, &B, c, q, sweep); }

// The shape of one column (block proposals): column_assemble and column_factor, unchanged, on the column's inputs; where the column has a
// used datum and every pivot is good, the packed triangle goes to tri[e * stride], r_l = sample_rsqrt(d_l) to r[l * stride] -- elsewhere
// both stay as the caller left them.  The model is not stepped.  Returns the flag; every lane returns the same.
template <class Sync>
DSA_CS int sample_shape(const ColumnIn& in, float smooth, float damp, const ColumnWork& w, double* tri, double* r, long long stride, int* nused, int lane,
                        int nlanes, Sync sync)
{
    const double lambda2 = (double)smooth * (double)smooth, mu2 = (double)damp * (double)damp;
    double chi2 = 0.0;
    *nused = column_assemble(in, lambda2, mu2, w, &chi2, lane, nlanes, sync);
    if (*nused == 0) return kColumnNoData;
    const int flag = column_factor(in.M, w, lane, nlanes, sync);
    if (flag != kColumnOk) return flag;
    for (int e = lane; e < column_tri_size(in.M); e += nlanes) tri[e * stride] = w.tri[e];
    for (int l = lane; l < in.M; l += nlanes) r[l * stride] = sample_rsqrt(w.d[l]);
    return kColumnOk;
}

// The finish of (column c, depth l < M), chains ascending, every sum from 0.0; n = nkept (the same for every chain of a column), m_q =
// S1_q / n, w_q = S2_q / n - m_q m_q.  nodes (5, M, ncol): the pooled mean v0 + sum S1 / (n C), the pooled variance sum S2 / (n C) -
// (sum S1 / (n C))^2, W = sum w_q / C, B = sum (m_q - sum m_q / C)^2 / (C - 1) (0 for C = 1), and the node of the best model: the chain with
// the smallest best phi + psi, the first one at a tie.  The thread of l = 0 also writes the column's figures: cols (3, ncol): phi of the
// start, the best phi + psi, the mean kept phi; counts (8, ncol): nused, flag, the four counters summed over the chains, the chains put
// back at the set-up, nkept.  Without a kept sweep (n = 0: the ring, a flagged column, burn >= the sweeps run) every figure of nodes, the
// best phi + psi and the mean kept phi are 0.
DSA_CS void sample_finish(const SampleView& S, long long c, int l, double* nodes, double* cols, int* counts)
{
    const int M = S.nz - 1, C = S.C;
    const int n = S.nkept[sample_at(S, c, 0)];
    const double dn = (double)n, dc = (double)C;
    int best_q = 0;
    for (int q = 1; q < C; ++q)
        if (S.best_e[sample_at(S, c, q)] < S.best_e[sample_at(S, c, best_q)]) best_q = q;
    double out[kSampleNodeFigures] = { 0.0, 0.0, 0.0, 0.0, 0.0 };
    if (n > 0) {
        double s1 = 0.0, s2 = 0.0, sw = 0.0, sm = 0.0;
        for (int q = 0; q < C; ++q) {
            const long long e = sample_node(S, c, q, l);
            const double m = S.S1[e] / dn;
            s1 += S.S1[e];
            s2 += S.S2[e];
            sw += S.S2[e] / dn - m * m;
            sm += m;
        }
        const double pm = s1 / (dn * dc), mbar = sm / dc;
        double sb = 0.0;
        for (int q = 0; q < C; ++q) {
            const double d = S.S1[sample_node(S, c, q, l)] / dn - mbar;
            sb += d * d;
        }
        out[kSampleMean] = (double)S.v0[(long long)l * S.ncol + c] + pm;
        out[kSampleVar] = s2 / (dn * dc) - pm * pm;
        out[kSampleW] = sw / dc;
        out[kSampleB] = C > 1 ? sb / (dc - 1.0) : 0.0;
        out[kSampleBest] = (double)S.best_v[sample_node(S, c, best_q, l)];
    }
    for (int f = 0; f < kSampleNodeFigures; ++f) nodes[((long long)f * M + l) * S.ncol + c] = out[f];
    if (l != 0) return;
    int sums[kSampleCounters] = { 0, 0, 0, 0 }, reseeded = 0;
    double phis = 0.0;
    for (int q = 0; q < C; ++q) {
        const long long at = sample_at(S, c, q);
        for (int w = 0; w < kSampleCounters; ++w) sums[w] += S.cnt[((long long)w * C + q) * S.ncol + c];
        reseeded += S.reseed[at];
        phis += S.phisum[at];
    }
    cols[kSamplePhiStart * S.ncol + c] = S.phi0[c];
    cols[kSampleBestE * S.ncol + c] = n > 0 ? S.best_e[sample_at(S, c, best_q)] : 0.0;
    cols[kSampleMeanPhi * S.ncol + c] = n > 0 ? phis / (dn * dc) : 0.0;
    counts[kSampleNused * S.ncol + c] = S.nused[c];
    counts[kSampleFlag * S.ncol + c] = S.flag[c];
    for (int w = 0; w < kSampleCounters; ++w) counts[(kSampleSumAccepted + w) * S.ncol + c] = sums[w];
    counts[kSampleReseeded * S.ncol + c] = reseeded;
    counts[kSampleNkept * S.ncol + c] = n;
}

// ---- the posterior marginals: observers of the kept sweeps; they write nothing of the above ----

// the bin of value v in the box of (column c, depth l) cut into nbins equal bins: 0 in a box without width, an end bin outside the box
DSA_CS int sample_bin(const SampleView& S, long long c, int l, int nbins, float v)
{
    float lo, hi;
    sample_box(S, c, l, &lo, &hi);
    const double dlo = (double)lo, w = (double)hi - dlo;
    if (!(w > 0.0)) return 0;
    const double t = ((double)v - dlo) / w;
    const double x = t * (double)nbins;
    if (x < 0.0) return 0;
    if (x >= (double)nbins) return nbins - 1;
    return (int)x;
}

// a chain whose state sweep `sweep` added to the moments (sample_accept_any's rule, read after it)
DSA_CS bool sample_marginal_kept(const SampleView& S, long long c, int q, int sweep) { return sweep > S.burn && S.pmark[sample_at(S, c, q)] != kSampleIdle; }

// the sweep's count of (column c, chain q, depth l < M), after the sweep's Metropolis test
DSA_CS void sample_marginal_hist(const SampleView& S, const SampleMarginalView& G, long long c, int q, int l, int sweep)
{
    if (!sample_marginal_kept(S, c, q, sweep)) return;
    const int M = S.nz - 1;
    const int b = sample_bin(S, c, l, G.nbins, S.v[sample_node(S, c, q, l)]);
    G.hist[(((long long)b * M + l) * S.C + q) * S.ncol + c] += 1u;
}

// the sweep's product of (column c, chain q, triangle entry e = column_tri(i, j), j <= i), after the sweep's Metropolis test
DSA_CS void sample_marginal_cov(const SampleView& S, const SampleMarginalView& G, long long c, int q, int e, int sweep)
{
    if (!sample_marginal_kept(S, c, q, sweep)) return;
    const int i = column_tri_row(e), j = e - column_tri(i, 0);
    const double di = (double)S.v[sample_node(S, c, q, i)] - (double)S.v0[(long long)i * S.ncol + c];
    const double dj = (double)S.v[sample_node(S, c, q, j)] - (double)S.v0[(long long)j * S.ncol + c];
    G.P[((long long)e * S.C + q) * S.ncol + c] += di * dj;
}

// The marginal of (column c, depth l < M): pooled (nbins, M, ncol), the counts summed over the chains ascending; figures (1 + nlevels, M,
// ncol), the mode -- the centre of the first fullest pooled bin -- and the quantiles of the levels p (each in (0, 1)): N the pooled total,
// target = p N; at the first bin b, ascending, with h_b > 0 and cum + h_b >= target (cum the total of the bins below), the value
// lo + ((b + (target - cum) / h_b) / nbins) w.  N = 0 (the ring, a flagged column, no kept sweep): zeros, as sample_finish.
DSA_CS void sample_marginal_finish(const SampleView& S, const SampleMarginalView& G, long long c, int l, int nlevels, const double* levels, unsigned* pooled,
                                   double* figures)
{
    const int M = S.nz - 1, C = S.C, nb = G.nbins;
    float lo, hi;
    sample_box(S, c, l, &lo, &hi);
    const double dlo = (double)lo, w = (double)hi - dlo, dnb = (double)nb;
    unsigned long long N = 0ull;
    unsigned top = 0u;
    int bstar = 0;
    for (int b = 0; b < nb; ++b) {
        unsigned h = 0u;
        for (int q = 0; q < C; ++q) h += G.hist[(((long long)b * M + l) * C + q) * S.ncol + c];
        pooled[((long long)b * M + l) * S.ncol + c] = h;
        N += h;
        if (h > top) { top = h; bstar = b; }
    }
    figures[(long long)l * S.ncol + c] = N ? dlo + (((double)bstar + 0.5) / dnb) * w : 0.0;
    for (int k = 0; k < nlevels; ++k) {
        double out = 0.0;
        if (N) {
            const double target = levels[k] * (double)N;
            unsigned long long cum = 0ull;
            for (int b = 0; b < nb; ++b) {
                const unsigned h = pooled[((long long)b * M + l) * S.ncol + c];
                if (h > 0u && (double)(cum + h) >= target) {
                    const double frac = (target - (double)cum) / (double)h;
                    out = dlo + (((double)b + frac) / dnb) * w;
                    break;
                }
                cum += h;
            }
        }
        figures[((long long)(1 + k) * M + l) * S.ncol + c] = out;
    }
}

// The pooled covariance of (column c, triangle entry e = column_tri(i, j)): cov (tri, ncol) = sum_q P_q / (n C) - pm_i pm_j, chains ascending,
// pm sample_finish's pooled mean offset; the diagonal has the bits of sample_finish's variance.  n = 0: 0.
DSA_CS void sample_marginal_cov_finish(const SampleView& S, const SampleMarginalView& G, long long c, int e, double* cov)
{
    const int C = S.C;
    const int n = S.nkept[sample_at(S, c, 0)];
    double out = 0.0;
    if (n > 0) {
        const int i = column_tri_row(e), j = e - column_tri(i, 0);
        const double dn = (double)n, dc = (double)C;
        double si = 0.0, sj = 0.0, sp = 0.0;
        for (int q = 0; q < C; ++q) {
            si += S.S1[sample_node(S, c, q, i)];
            sj += S.S1[sample_node(S, c, q, j)];
            sp += G.P[((long long)e * C + q) * S.ncol + c];
        }
        const double pmi = si / (dn * dc), pmj = sj / (dn * dc);
        out = sp / (dn * dc) - pmi * pmj;
    }
    cov[(long long)e * S.ncol + c] = out;
}

}  // namespace dsa
