// Many LSMR solves on one resident matrix (dsa_lsmr_batch): realisation r solves the row-scaled system diag(s_r) A x = diag(s_r) b,
// the linear step of a bootstrap over the data rows.  Every realisation is bit-identical to dsa_lsmr on its explicitly scaled
// system (entries fl(a * s_r[row]), right-hand side fl(b * s_r)), i.e. to the reference's LSMR on that system.
//
// Why on the device: a lone solve's ordered fp32 reductions are serial chains, and on one wavefront a dependent add costs ~18
// cycles (lsmr.hip); so dsa_lsmr keeps them on the host.  With R realisations there are R independent chains: lane l of group g
// runs the chain of realisation 64 g + l, and a chain costs a lane what it costs one wavefront.  Likewise a matrix entry is read
// once for R products, and its R input operands are one coalesced 256-byte load.
//
// Layout: every batch vector is [group][element][64 realisations] (element i of realisation 64 g + l at (g * len + i) * 64 + l),
// the row scales too.  Realisations past nreal (padding lanes of the last group) have scale 0 and never run.
//
// The order of every sum is the reference's:
//   * products: one wavefront per (output element, group); the entries of the element are read in storage order from a contiguous
//     copy of the resident orderings (SpmvState::Contiguous, built once per loaded matrix) -- value and index wave-uniform, scalar
//     loads -- and each lane adds fl(fl(a * s_r[row]) * in_r[idx]) to its own accumulator;
//   * dnrm2 (lsmrblas.f90:247-277) and dot_product (lsmrModule.f90:744): one workgroup per group stages the terms through LDS and
//     its first wavefront walks them, each lane its own chain (k_b_chain).  dnrm2's running scale is a running maximum of |x|, so
//     wide kernels form it and every element's division ahead of the chain, which is left with the additions;
//   * element-wise updates with per-realisation coefficients and masks.
// The scalar recurrences are dsa::LsmrScalars (lsmr_core.h), the same code dsa_lsmr runs, one per realisation.  A realisation that
// stops is frozen: no kernel writes its lanes again.  Three host synchronisations per iteration (beta, alpha, normx: nreal values each).
//
// Six entry points run that loop.  Each is: the front door (Entry: the argument checks they share), the layout of its pieces of btmp
// (Carve), batch_begin, u and the row scales by k_b_fill under its rule (Fill), batch_solve, then its own measures.  bx keeps the
// solutions for a later call (dsa_forward_steps, SpmvState::bx_valid).
//   * dsa_lsmr_batch: the bootstrap above (FILL_ROWS).
//   * dsa_lsmr_resolution: the right-hand sides of test models, formed on the device: v = unit spikes made in place or host
//     models, row scales 1 and u = 0 (FILL_ONE without b), u = A v by k_b_spmv<true> (fl(a * 1) = a: the chain of dsa_spmv mode 1 from
//     y = 0), then the regularisation rows zeroed.  For spikes, k_b_psf_part / k_b_psf_sum reduce each solution to its PSF measures.
//   * dsa_resolution_blocks (§19): the same spike solves (resolution_solve), the measures taken per parameter block of the unknowns
//     (k_b_psf_blocks_part / k_b_psf_blocks_sum): the joint Vs | gc | gs system of the azimuthal step.
//   * dsa_lsmr_tradeoff (§13): K (weight, damp) pairs.  The products read a coefficient copy of the contiguous values whose regularisation
//     entries hold their integer coefficient c (the resident entry is fl(c * weight0)); with row scales 1 on the data rows and weight_k
//     from ndata up (FILL_WEIGHT) member k multiplies by fl(a * 1) = a and fl(c * weight_k): the system dsa_iteration_system builds with
//     weight_k.  damp_k goes to member k's LsmrScalars.  batch_measures: each solution's misfit, roughness and size.
//   * dsa_lsmr_crossval (§15): the same (weighted_solve) on ncombo pairs x (nfolds hold-outs + the full data): the data rows' scales are 0
//     where the member holds the row out, else 1, and u = fl(b * scale) there (FILL_FOLD); the measures take a hold predicate per lane
//     (HoldFold): kept and held-out misfit apart, and every datum's held-out and full-fit residual stored by the lane that formed it.
//   * dsa_lsmr_voronoi (§14): K random Voronoi projections of the data rows: member k's unknowns are the ncells cells of its tessellation
//     (k_v_assign), its matrix the resident data rows with column j relabelled cell_k(j).  Batch vectors of (ndata, ncells), u = b and row
//     scales 1 (FILL_ONE); Batch::product is the projected one: mode 1 expands v through the cell map and runs k_b_spmv<true> over the data
//     rows, mode 2 walks per (member, cell) the member's CSR positions sorted by cell (k_v_colprod).  k_v_stats: the ensemble statistics.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/dsurftomo_amd.h"
#include "engine.h"
#include "lsmr_core.h"
#include "spmv_state.h"

namespace dsa {

namespace {

// per-realisation parameters, fields of Rp values each: coefficients (float), then flags (int)
enum { C_PRE_U, C_IBETA, C_PRE_V, C_IALPHA, C_C1, C_C2, C_C3, NCOEF };
enum { F_ACT, F_BPOS, F_SLOT, F_LIM, F_APOS, NFLAG };
constexpr int kNParam = NCOEF + NFLAG;

// Element-wise kernels: blockIdx.y is the group, the x dimension strides over its len * 64 elements (lane = realisation % 64).
#define LB_GROUP_LOOP(len)                                                                                            \
    const int g = blockIdx.y;                                                                                         \
    const size_t gbase = (size_t)g * (size_t)(len) * 64;                                                              \
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < (size_t)(len) * 64; t += (size_t)gridDim.x * blockDim.x)

// How k_b_fill scales the rows of member r (par: the rule's values)
enum Fill {
    FILL_ROWS,      // dsa_lsmr_batch: row i by par[r * m + i], the realisation's own row scales
    FILL_ONE,       // dsa_lsmr_resolution, dsa_lsmr_voronoi: every row by 1
    FILL_WEIGHT,    // dsa_lsmr_tradeoff: the data rows by 1, the rows from ndata up by par[r]
    FILL_FOLD,      // dsa_lsmr_crossval, member r = q * stride + f: the data rows by 0 where fold[i] == f, else 1, the rows from ndata up by par[q]
};

// (g, i, l) of the batch layout: scale = the rule's row scale, u = fl(b[i] * scale) on the rows whose right-hand side the rule scales (all
// of FILL_ROWS, the data rows of FILL_FOLD) and b[i] on the others (there the scale is 1, or a weight that multiplies the matrix alone: b is
// stored as it is, not as fl(b * 1)); u = +0 without b.  Both +0 in the padding lanes (r >= nreal), which never run.
__global__ void k_b_fill(Fill rule, int m, int ndata, int nreal, int stride, const float* __restrict__ b, const float* __restrict__ par,
                         const int* __restrict__ fold, float* __restrict__ scale, float* __restrict__ u)
{
    LB_GROUP_LOOP(m) {
        const int r = g * 64 + (int)(t & 63);
        const size_t i = t >> 6;
        float s = 0.0f, uu = 0.0f;
        if (r < nreal) {
            bool mul = false;
            if (rule == FILL_ROWS) { s = par[(size_t)r * (size_t)m + i]; mul = true; }
            else if (rule == FILL_ONE) s = 1.0f;
            else if (i >= (size_t)ndata) s = par[rule == FILL_FOLD ? r / stride : r];
            else if (rule == FILL_FOLD) { s = fold[i] == r % stride ? 0.0f : 1.0f; mul = true; }
            else s = 1.0f;
            if (b) uu = mul ? b[i] * s : b[i];
        }
        scale[gbase + t] = s;
        u[gbase + t] = uu;
    }
}

// (g, i, l) of the batch layout <- realisation-major in[r * len + i] (0 past nreal); T: float (models) or int (cell maps)
template <typename T>
__global__ void k_b_scatter(int len, int nreal, const T* __restrict__ in, T* __restrict__ out)
{
    LB_GROUP_LOOP(len) {
        const int r = g * 64 + (int)(t & 63);
        out[gbase + t] = r < nreal ? in[(size_t)r * (size_t)len + (t >> 6)] : T(0);
    }
}

// The tail of the fp64 block reductions (blocks of four wavefronts): every wavefront leaves its lanes' NS sums in LDS and wavefront 0
// stores, per lane, ((w0 + w1) + w2) + w3 of each to out[0 .. NS)
template <int NS>
__device__ inline void block_sum4(const double (&s)[NS], double* __restrict__ out)
{
    __shared__ double red[NS][4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < NS; ++c) red[c][w][lane] = s[c];
    __syncthreads();
    if (w == 0) {
#pragma unroll
        for (int c = 0; c < NS; ++c) out[c] = ((red[c][0][lane] + red[c][1][lane]) + red[c][2][lane]) + red[c][3][lane];
    }
}

// realisation-major copy of a batch vector of length n: out[r * n + i]; the y dimension strides over the realisations
__global__ void k_b_gather(int n, int nreal, const float* __restrict__ x, float* __restrict__ out)
{
    for (int r = blockIdx.y; r < nreal; r += gridDim.y) {
        const float* __restrict__ xg = x + (size_t)(r >> 6) * (size_t)n * 64 + (r & 63);
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[(size_t)r * n + i] = xg[(size_t)i * 64];
    }
}

// x = c_r * x where flag_r (the reference's dscal: one multiply)
__global__ void k_b_scal(int len, const float* __restrict__ coef, const int* __restrict__ flag, float* __restrict__ x)
{
    LB_GROUP_LOOP(len) {
        const int r = g * 64 + (int)(t & 63);
        if (flag[r]) x[gbase + t] = coef[r] * x[gbase + t];
    }
}

// localVEnqueue (lsmrModule.f90:715-727): queue slot slot_r <- v where slot_r >= 0; the queue is [slot][group][n][64], slots `stride` apart
__global__ void k_b_enqueue(int n, size_t stride, const int* __restrict__ slot, const float* __restrict__ v, float* __restrict__ lv)
{
    LB_GROUP_LOOP(n) {
        const int s = slot[g * 64 + (int)(t & 63)];
        if (s >= 0) lv[(size_t)s * stride + gbase + t] = v[gbase + t];
    }
}

// v = v - d_r * lv where k < lim_r (localVOrtho, lsmrModule.f90:745)
__global__ void k_b_axmy(int n, int k, const float* __restrict__ d, const int* __restrict__ lim, const float* __restrict__ lv, float* __restrict__ v)
{
    LB_GROUP_LOOP(n) {
        const int r = g * 64 + (int)(t & 63);
        if (k < lim[r]) v[gbase + t] = v[gbase + t] - d[r] * lv[gbase + t];
    }
}

// v = v / alpha where apos_r (lsmrModule.f90:508), then where act_r lsmrModule.f90:545-547: hbar = h - c1*hbar; x = x + c2*hbar; h = v - c3*h
__global__ void k_b_update(int n, const float* __restrict__ coef, const int* __restrict__ flag, float* __restrict__ v, float* __restrict__ h,
                           float* __restrict__ hbar, float* __restrict__ x, int Rp)
{
    LB_GROUP_LOOP(n) {
        const int r = g * 64 + (int)(t & 63);
        const size_t e = gbase + t;
        float vv = v[e];
        if (flag[F_APOS * Rp + r]) { vv = coef[C_IALPHA * Rp + r] * vv; v[e] = vv; }
        if (flag[F_ACT * Rp + r]) {
            const float hi = h[e];
            const float hb = hi - coef[C_C1 * Rp + r] * hbar[e];
            hbar[e] = hb;
            x[e] = x[e] + coef[C_C2 * Rp + r] * hb;
            h[e] = vv - coef[C_C3 * Rp + r] * hi;
        }
    }
}

// The ordered reductions.  A lane's chain is cheap: one dependent add (dot_product), or one multiply-add and a select (dnrm2) per
// element.  What would make it expensive is on one side memory -- a wavefront alone keeps too few 256-byte loads in flight -- and
// on the other dnrm2's divisions, a dozen instructions each.  So:
//   * dnrm2's divisions leave the chain.  The running scale of lsmrblas.f90:261-272 is, before element i, exactly the running
//     maximum of |x(1..i-1)| (it is replaced by |x(i)| iff scale < |x(i)|; a NaN never replaces it, as in fmaxf), which does not
//     depend on the sums.  Wide kernels form it (k_pm_blockmax, k_pm_scan, k_pm_terms: block maxima, their running maximum, then
//     within the block) and with it every element's term: +(|x|/scale)**2 where scale >= |x| (the reference's else branch), or
//     -(scale/|x|)**2 with the sign bit set where |x| is a new maximum (its `ssq = 1 + ssq*q**2` branch), +0 for a zero (skipped:
//     ssq + 0 = ssq).  The chain then only adds (or multiplies and adds) in order: the same operations on the same operands.
//   * k_b_chain: a workgroup of kCT threads stages the group's terms chunk by chunk (kCE elements x 64 realisations) into LDS, two
//     chunks of loads ahead in registers, and its first wavefront runs the 64 chains out of LDS while the others stage the next
//     chunk: one barrier per chunk.
constexpr int kCT = 1024;                   // threads of a chain workgroup
constexpr int kCE = 128;                    // elements per chunk: 128 x 64 x 4 B = 32 KB, two buffers
constexpr int kPer = kCE * 64 / kCT;        // floats a thread stages per chunk
constexpr int kPB = 256;                    // elements per block of the running maximum (four wavefronts of 64)

// bm[g][b][lane] = max over the block's elements of |x| (fmaxf: a NaN is passed over, as the reference's scale passes it over)
__global__ __launch_bounds__(256) void k_pm_blockmax(int len, int nblk, const float* __restrict__ x, float* __restrict__ bm)
{
    __shared__ float red[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = blockIdx.y, b = blockIdx.x;
    const float* __restrict__ p = x + (size_t)g * len * 64 + lane;
    const int e0 = b * kPB + w * 64, e1 = min(e0 + 64, len);
    float mx = 0.0f;
    for (int e = e0; e < e1; ++e) mx = fmaxf(mx, fabsf(p[(size_t)e * 64]));
    red[w][lane] = mx;
    __syncthreads();
    if (w == 0) bm[((size_t)g * nblk + b) * 64 + lane] = fmaxf(fmaxf(red[0][lane], red[1][lane]), fmaxf(red[2][lane], red[3][lane]));
}

// per group and lane: bm <- the running maximum before each block (exclusive), tot <- the maximum of the whole vector (dnrm2's final scale)
__global__ __launch_bounds__(64) void k_pm_scan(int nblk, float* __restrict__ bm, float* __restrict__ tot)
{
    const int lane = threadIdx.x;
    float* __restrict__ p = bm + (size_t)blockIdx.x * nblk * 64 + lane;
    float run = 0.0f;
    int b = 0;
    for (; b + 8 <= nblk; b += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(b + u) * 64];
#pragma unroll
        for (int u = 0; u < 8; ++u) { p[(size_t)(b + u) * 64] = run; run = fmaxf(run, v[u]); }
    }
    for (; b < nblk; ++b) { const float v = p[(size_t)b * 64]; p[(size_t)b * 64] = run; run = fmaxf(run, v); }
    tot[(size_t)blockIdx.x * 64 + lane] = run;
}

// T(i) = dnrm2's term of element i (see above) with scale = the lane's running maximum before i
__global__ __launch_bounds__(256) void k_pm_terms(int len, int nblk, const float* __restrict__ x, const float* __restrict__ bm, float* __restrict__ T)
{
    __shared__ float red[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = blockIdx.y, b = blockIdx.x;
    const size_t off = (size_t)g * len * 64 + lane;
    const float* __restrict__ p = x + off;
    float* __restrict__ q = T + off;
    const int e0 = b * kPB + w * 64, e1 = min(e0 + 64, len);
    float mx = 0.0f;
    for (int e = e0; e < e1; ++e) mx = fmaxf(mx, fabsf(p[(size_t)e * 64]));
    red[w][lane] = mx;
    __syncthreads();
    float scale = bm[((size_t)g * nblk + b) * 64 + lane];
    for (int k = 0; k < w; ++k) scale = fmaxf(scale, red[k][lane]);
    for (int e = e0; e < e1; ++e) {
        const float a = fabsf(p[(size_t)e * 64]);
        const bool nm = scale < a;                       // a new maximum (false for a NaN)
        const float qv = nm ? scale / a : a / scale;
        const float t = qv * qv;
        q[(size_t)e * 64] = a == 0.0f ? 0.0f : (nm ? -t : t);
        scale = nm ? a : scale;
    }
}

// out_r = the in-order chain of realisation r's terms: DOT: acc = 0, acc + x(i) * y(i) (dot_product, lsmrModule.f90:744);
// else dnrm2 (lsmrblas.f90:247-277) over the terms T = x of k_pm_terms: ssq = 1, then ssq + T or, where T's sign bit is set,
// 1 + ssq * (-T); the result tot_r * sqrt(ssq).  One workgroup per group.
template <bool DOT>
__global__ __launch_bounds__(kCT) void k_b_chain(int len, const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ tot,
                                                 const float* __restrict__ x1, float* __restrict__ out)
{
    __shared__ float buf[2][kCE * 64];
    const int tid = threadIdx.x, lane = tid & 63;
    const size_t gb = (size_t)blockIdx.x * len * 64, total = (size_t)len * 64;
    const int nchunk = (len + kCE - 1) / kCE;
    float a0[kPer], b0[kPer], a1[kPer], b1[kPer];
    // loads past the vector read its last element (no branches: the loads of a chunk stay in flight across the barriers); stage() zeroes them
    auto load = [&](int c, float* av, float* bv) {
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const size_t f = min((size_t)c * kCE * 64 + (size_t)j * kCT + tid, total - 1);
            av[j] = x[gb + f];
            if (DOT) bv[j] = y[gb + f];
        }
    };
    auto stage = [&](int c, float* s, const float* av, const float* bv) {
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const bool in = (size_t)c * kCE * 64 + (size_t)j * kCT + tid < total;
            s[j * kCT + tid] = in ? (DOT ? av[j] * bv[j] : av[j]) : 0.0f;
        }
    };
    float acc = DOT ? 0.0f : 1.0f;                   // (the chain wavefront's: the dot's sum, or dnrm2's ssq)
    auto chain = [&](int c, const float* s) {
        const int cnt = min(kCE, len - c * kCE);      // elements of this chunk (wave-uniform)
        for (int e = 0; e < cnt; ++e) {
            const float t = s[e * 64 + lane];
            if (DOT) acc = acc + t;
            else {
                const float renew = 1.0f + acc * (-t);
                const float add = acc + t;
                acc = ((__float_as_uint(t) >> 31) && t == t) ? renew : add;     // (a NaN term is never a new maximum)
            }
        }
    };
    load(0, a0, b0);
    load(1, a1, b1);
    for (int c = 0; c < nchunk; c += 2) {            // two chunks per trip: the register sets alternate without copies
        stage(c, buf[0], a0, b0);
        load(c + 2, a0, b0);
        __syncthreads();
        if (tid < 64) chain(c, buf[0]);
        stage(c + 1, buf[1], a1, b1);
        load(c + 3, a1, b1);
        __syncthreads();
        if (tid < 64 && c + 1 < nchunk) chain(c + 1, buf[1]);
    }
    if (tid < 64) {
        float res;
        if (DOT) res = acc;
        else if (len < 1) res = 0.0f;
        else if (len == 1) res = fabsf(x1[gb + lane]);
        else res = tot[(size_t)blockIdx.x * 64 + lane] * sqrtf(acc);
        out[(size_t)blockIdx.x * 64 + lane] = res;
    }
}

// out_r[seg] = pre_r * out_r[seg] + sum over the segment's entries, in storage order, of fl(fl(a * s_r[row]) * in_r[idx]), where
// flag_r.  One wavefront per (segment, group): the entries' values and indices are wave-uniform, the 64 realisations' operands
// of an entry one 256-byte load.  ROW: segments are rows (u += A v), the row scale is the segment's; else segments are columns
// (v += A^T u) and the row scale sits beside the gathered operand.
template <bool ROW>
__global__ __launch_bounds__(256) void k_b_spmv(int nseg, int nin, const long long* __restrict__ ptr, const float* __restrict__ val, const int* __restrict__ idx,
                                                const float* __restrict__ scale, const float* __restrict__ in, float* __restrict__ out,
                                                const float* __restrict__ pre, const int* __restrict__ flag)
{
    const int lane = threadIdx.x & 63, g = blockIdx.y;
    const int seg = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (seg >= nseg) return;
    const int r = g * 64 + lane;
    const bool on = flag[r] != 0;
    if (__ballot(on) == 0) return;
    float* __restrict__ o = out + ((size_t)g * nseg + seg) * 64 + lane;
    const float* __restrict__ x = in + (size_t)g * nin * 64 + lane;
    // [g][m][64]: by rows the output is the row, by columns the input is
    const float* __restrict__ sc = scale + (size_t)g * (ROW ? nseg : nin) * 64 + lane;
    const float srow = ROW ? sc[(size_t)seg * 64] : 0.0f;
    float acc = *o;
    if (pre) acc = pre[r] * acc;
    long long k = ptr[seg];
    const long long k1 = ptr[seg + 1];
    constexpr int U = 8;
    for (; k + U <= k1; k += U) {
        float a[U], xi[U], s[U];
        int ix[U];
#pragma unroll
        for (int u = 0; u < U; ++u) { a[u] = val[k + u]; ix[u] = idx[k + u]; }
#pragma unroll
        for (int u = 0; u < U; ++u) { xi[u] = x[(size_t)ix[u] * 64]; s[u] = ROW ? srow : sc[(size_t)ix[u] * 64]; }
#pragma unroll
        for (int u = 0; u < U; ++u) { const float as = a[u] * s[u]; acc = acc + as * xi[u]; }
    }
    for (; k < k1; ++k) {
        const int i = idx[k];
        const float as = val[k] * (ROW ? srow : sc[(size_t)i * 64]);
        acc = acc + as * x[(size_t)i * 64];
    }
    if (on) *o = acc;
}

// one block of an ordering copied into the contiguous layout: entry k of the segment of (slice j, lane l) goes to start[j*64+l] + k
__global__ void k_contig_fill(int nslots, const long long* __restrict__ off, const int* __restrict__ len, const long long* __restrict__ start,
                              const float* __restrict__ val, const int* __restrict__ idx, const unsigned short* __restrict__ idx16, int base,
                              float* __restrict__ cval, int* __restrict__ cidx)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nslots) return;
    const int n = len[i];
    if (n == 0) return;
    const long long src = off[i >> 6] + (i & 63), dst = start[i];
    for (int k = 0; k < n; ++k) {
        const long long p = src + (long long)k * 64;
        cval[dst + k] = val[p];
        cidx[dst + k] = idx16 ? base + (int)idx16[p] : idx[p];
    }
}

#define LB_TRY(e, call)                                                                        \
    do {                                                                                       \
        hipError_t _r = (call);                                                                \
        if (_r != hipSuccess) { (e)->fail(DSA_ERR_DEVICE, "lsmr_batch: %s failed: %s", #call, hipGetErrorString(_r)); return DSA_ERR_DEVICE; } \
    } while (0)
#define LB_DO(call) do { if (int _rc = (call)) return _rc; } while (0)

// the end of a call's device work: launch errors, then the stream drained
int drain(Engine* e, hipStream_t st)
{
    LB_TRY(e, hipGetLastError());
    LB_TRY(e, hipStreamSynchronize(st));
    return 0;
}

// A segment's entries lie in the blocks of its ordering in storage order: in blocks 0, 1, ... (segments stored in ascending input
// order) or all in the unblocked rest.  So the contiguous copy of segment s is its part of block 0, then of block 1, ...
int build_contiguous(Engine* e, const SpmvState::Ordering& O, int nseg, long long nar, SpmvState::Contiguous& C)
{
    if (e->ensure(C.ptr, (size_t)nseg + 1) || e->ensure(C.val, std::max<size_t>((size_t)nar, 1)) || e->ensure(C.idx, std::max<size_t>((size_t)nar, 1)))
        return e->status;
    const int nb1 = (int)O.blocks.size();
    std::vector<std::vector<int>> seg(nb1), len(nb1);
    for (int b = 0; b < nb1; ++b) {
        const SpmvState::Sliced& L = O.blocks[b];
        if (L.padded <= 0) continue;
        const size_t ns = (size_t)L.nslices * 64;
        seg[b].resize(ns); len[b].resize(ns);
        LB_TRY(e, hipMemcpyAsync(seg[b].data(), L.seg.p, ns * 4, hipMemcpyDeviceToHost, e->stream));
        LB_TRY(e, hipMemcpyAsync(len[b].data(), L.len.p, ns * 4, hipMemcpyDeviceToHost, e->stream));
    }
    LB_TRY(e, hipStreamSynchronize(e->stream));
    std::vector<long long> ptr((size_t)nseg + 1, 0);
    for (int b = 0; b < nb1; ++b)
        for (size_t i = 0; i < len[b].size(); ++i)
            if (len[b][i] > 0) {
                if (seg[b][i] < 0 || seg[b][i] >= nseg) { e->fail(DSA_ERR_INTERNAL, "lsmr_batch: segment %d of an ordering outside 0..%d", seg[b][i], nseg - 1); return DSA_ERR_INTERNAL; }
                ptr[(size_t)seg[b][i] + 1] += len[b][i];
            }
    for (int s = 0; s < nseg; ++s) ptr[(size_t)s + 1] += ptr[s];
    if (ptr[nseg] != nar) { e->fail(DSA_ERR_INTERNAL, "lsmr_batch: an ordering holds %lld entries, the matrix %lld", ptr[nseg], nar); return DSA_ERR_INTERNAL; }
    LB_TRY(e, hipMemcpyAsync(C.ptr.p, ptr.data(), ((size_t)nseg + 1) * 8, hipMemcpyHostToDevice, e->stream));
    std::vector<long long> cur(ptr.begin(), ptr.end() - 1);
    DevBuf<long long> d_start;
    std::vector<long long> start;
    int rc = 0;
    for (int b = 0; b < nb1 && rc == 0; ++b) {
        const SpmvState::Sliced& L = O.blocks[b];
        if (L.padded <= 0) continue;
        const size_t ns = len[b].size();
        start.assign(ns, 0);
        for (size_t i = 0; i < ns; ++i)
            if (len[b][i] > 0) { start[i] = cur[(size_t)seg[b][i]]; cur[(size_t)seg[b][i]] += len[b][i]; }
        if (e->ensure(d_start, ns)) { rc = e->status; break; }
        if (hipMemcpyAsync(d_start.p, start.data(), ns * 8, hipMemcpyHostToDevice, e->stream) != hipSuccess) { e->fail(DSA_ERR_DEVICE, "lsmr_batch: upload failed"); rc = DSA_ERR_DEVICE; break; }
        const bool local = b < O.nblocks;
        hipLaunchKernelGGL(k_contig_fill, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, e->stream, (int)ns, L.off.p, L.len.p, d_start.p, L.val.p,
                           local ? nullptr : L.idx.p, local ? L.idx16.p : nullptr, local ? b * O.block : 0, C.val.p, C.idx.p);
        if (hipStreamSynchronize(e->stream) != hipSuccess || hipGetLastError() != hipSuccess) { e->fail(DSA_ERR_DEVICE, "lsmr_batch: contiguous copy failed"); rc = DSA_ERR_DEVICE; }
    }
    if (d_start.p) (void)hipFree(d_start.p);
    return rc;
}

}  // namespace

int spmv_ensure_contiguous(Engine* e)
{
    SpmvState& S = *e->spmv;
    if (S.contiguous_valid) return 0;
    LB_DO(build_contiguous(e, S.by_row, S.m, S.nar, S.row_csr));
    LB_DO(build_contiguous(e, S.by_col, S.n, S.nar, S.col_csr));
    S.contiguous_valid = true;
    return 0;
}

namespace {

// element-wise launch over every group's len * 64 elements
dim3 grid_of(int len, int G) { return dim3((unsigned)std::min<size_t>(2048, std::max<size_t>(1, ((size_t)len * 64 + 255) / 256)), (unsigned)G); }

// ---- dsa_lsmr_resolution: the test models, and the PSF measures ----

// unit spikes: element i of realisation r is 1 where i == first + r (r < nreal), else 0
__global__ void k_b_spike(int n, int nreal, int first, float* __restrict__ out)
{
    LB_GROUP_LOOP(n) {
        const int r = g * 64 + (int)(t & 63);
        out[gbase + t] = (r < nreal && (long long)(t >> 6) == (long long)first + r) ? 1.0f : 0.0f;
    }
}

// rows [ndata, m) of every group's u <- +0 (the regularisation rows of the right-hand side)
__global__ void k_b_zero_rows(int m, int ndata, float* __restrict__ u)
{
    float* __restrict__ p = u + ((size_t)blockIdx.y * (size_t)m + (size_t)ndata) * 64;
    const size_t len = (size_t)(m - ndata) * 64;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < len; t += (size_t)gridDim.x * blockDim.x) p[t] = 0.0f;
}

// PSF measures of spike realisation r (unknown j = first + r) over its solution x_r: sum x^2, sum x^2 dh^2, sum x^2 dz^2 in fp64, dh the
// great-circle distance (haversine, sphere of kEarthKm) and dz the depth difference from unknown j; coords = (lat deg, lon deg, depth km)
// per unknown.  k_b_psf_part: block (b, g), four wavefronts, wavefront w the elements [b kPsfE + w kPsfE/4, +kPsfE/4) in order, one
// coalesced 256-byte load of bx per element; the four wavefronts' sums added in order.  k_b_psf_sum: the blocks' partials in order.
constexpr int kPsfE = 1024;                 // elements per block
constexpr double kEarthKm = 6371.0;

constexpr double kD2R = 3.14159265358979323846 / 180.0;

// cosl[i] = cos(latitude of unknown i), once per call (psf_dh needs it for both ends of every distance)
__global__ void k_psf_cos(int n, const double* __restrict__ coords, double* __restrict__ cosl)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) cosl[i] = cos(coords[3 * (size_t)i] * kD2R);
}

__device__ inline double psf_dh(double lat_i, double lon_i, double cos_i, double lat_j, double lon_j, double cos_j)
{
    const double sp = sin((lat_i - lat_j) * kD2R * 0.5), sl = sin((lon_i - lon_j) * kD2R * 0.5);
    const double a = sp * sp + cos_i * cos_j * sl * sl;
    return 2.0 * kEarthKm * asin(fmin(1.0, sqrt(a)));
}

__global__ __launch_bounds__(256) void k_b_psf_part(int n, int nb, int first, const double* __restrict__ coords, const double* __restrict__ cosl,
                                                    const float* __restrict__ x, double* __restrict__ part)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = blockIdx.y, b = blockIdx.x;
    const long long jj = (long long)first + g * 64 + lane;
    const int j = jj < n ? (int)jj : n - 1;                           // (padding lanes: any unknown, never read back)
    const double lat_j = coords[3 * (size_t)j], lon_j = coords[3 * (size_t)j + 1], dep_j = coords[3 * (size_t)j + 2], cos_j = cosl[j];
    const float* __restrict__ p = x + (size_t)g * n * 64 + lane;
    const int e0 = b * kPsfE + w * (kPsfE / 4), e1 = min(e0 + kPsfE / 4, n);
    double s[3] = {0.0, 0.0, 0.0};
    for (int e = e0; e < e1; ++e) {
        const double xv = (double)p[(size_t)e * 64];
        if (xv == 0.0) continue;                                          // (its terms are +0)
        const double q = xv * xv;
        const double dh = psf_dh(coords[3 * (size_t)e], coords[3 * (size_t)e + 1], cosl[e], lat_j, lon_j, cos_j);
        const double dz = coords[3 * (size_t)e + 2] - dep_j;
        s[0] = s[0] + q;
        s[1] = s[1] + q * (dh * dh);
        s[2] = s[2] + q * (dz * dz);
    }
    block_sum4(s, part + (((size_t)g * nb + b) * 64 + lane) * 3);
}

// psf[4 r .. 4 r + 3] = {x_r[j], the three sums}; one thread per realisation
__global__ __launch_bounds__(64) void k_b_psf_sum(int n, int nb, int nreal, int first, const float* __restrict__ x, const double* __restrict__ part,
                                                  double* __restrict__ psf)
{
    const int lane = threadIdx.x, g = blockIdx.x, r = g * 64 + lane;
    if (r >= nreal) return;
    double s[3] = {0.0, 0.0, 0.0};
    for (int b = 0; b < nb; ++b) {
        const double* __restrict__ q = part + (((size_t)g * nb + b) * 64 + lane) * 3;
        for (int c = 0; c < 3; ++c) s[c] = s[c] + q[c];
    }
    psf[4 * (size_t)r] = (double)x[((size_t)g * n + (size_t)(first + r)) * 64 + lane];
    for (int c = 0; c < 3; ++c) psf[4 * (size_t)r + 1 + c] = s[c];
}

// The same measures per parameter block (dsa_resolution_blocks): the n unknowns are nblocks blocks of nbc cells on one grid of cells,
// coords and cosl per cell.  Spike r sits at unknown j = first + r, cell cj = j mod nbc; for every block B the three sums run over the
// unknowns B nbc + e of x_r with dh, dz measured from cell cj to cell e.  k_b_psf_blocks_part: block (B nch + c, g), chunk c of block B =
// its cells [c kPsfE, + kPsfE), wavefront w the cells [c kPsfE + w kPsfE/4, + kPsfE/4) in order, the loop body k_b_psf_part's term for
// term; the four wavefronts' sums added in order (block_sum4).  k_b_psf_blocks_sum: block (g, B), the chunks' partials in order.  With
// nblocks = 1 this is k_b_psf_part / k_b_psf_sum's partition and arithmetic: the same bits.
__global__ __launch_bounds__(256) void k_b_psf_blocks_part(int n, int nbc, int nch, int first, const double* __restrict__ coords,
                                                           const double* __restrict__ cosl, const float* __restrict__ x, double* __restrict__ part)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = blockIdx.y, B = blockIdx.x / nch, c = blockIdx.x % nch;
    const long long jj = (long long)first + g * 64 + lane;
    const int j = jj < n ? (int)jj : n - 1;                           // (padding lanes: any unknown, never read back)
    const int cj = j % nbc;
    const double lat_j = coords[3 * (size_t)cj], lon_j = coords[3 * (size_t)cj + 1], dep_j = coords[3 * (size_t)cj + 2], cos_j = cosl[cj];
    const float* __restrict__ p = x + ((size_t)g * n + (size_t)B * nbc) * 64 + lane;
    const int e0 = c * kPsfE + w * (kPsfE / 4), e1 = min(e0 + kPsfE / 4, nbc);
    double s[3] = {0.0, 0.0, 0.0};
    for (int e = e0; e < e1; ++e) {
        const double xv = (double)p[(size_t)e * 64];
        if (xv == 0.0) continue;                                          // (its terms are +0)
        const double q = xv * xv;
        const double dh = psf_dh(coords[3 * (size_t)e], coords[3 * (size_t)e + 1], cosl[e], lat_j, lon_j, cos_j);
        const double dz = coords[3 * (size_t)e + 2] - dep_j;
        s[0] = s[0] + q;
        s[1] = s[1] + q * (dh * dh);
        s[2] = s[2] + q * (dz * dz);
    }
    block_sum4(s, part + (((size_t)g * gridDim.x + blockIdx.x) * 64 + lane) * 3);
}

// psf[(r nblocks + B) 4 .. + 3] = {x_r[B nbc + cj], block B's three sums}; one thread per (realisation, block)
__global__ __launch_bounds__(64) void k_b_psf_blocks_sum(int n, int nbc, int nch, int nreal, int first, const float* __restrict__ x,
                                                         const double* __restrict__ part, double* __restrict__ psf)
{
    const int lane = threadIdx.x, g = blockIdx.x, B = blockIdx.y, nblocks = gridDim.y, r = g * 64 + lane;
    if (r >= nreal) return;
    double s[3] = {0.0, 0.0, 0.0};
    for (int c = 0; c < nch; ++c) {
        const double* __restrict__ q = part + (((size_t)g * nblocks * nch + (size_t)B * nch + c) * 64 + lane) * 3;
        for (int k = 0; k < 3; ++k) s[k] = s[k] + q[k];
    }
    const int cj = (first + r) % nbc;
    double* __restrict__ o = psf + ((size_t)r * nblocks + B) * 4;
    o[0] = (double)x[((size_t)g * n + (size_t)B * nbc + cj) * 64 + lane];
    for (int k = 0; k < 3; ++k) o[1 + k] = s[k];
}

// ---- dsa_lsmr_tradeoff, dsa_lsmr_crossval: the coefficient copy of the contiguous values ----

// c of a regularisation entry a = fl(c * w0): rint(a / w0); `bad` unless c is a non-zero integer of at most 64 whose product gives a's bits back
__device__ inline float coef_of(float a, float w0, bool& bad)
{
    const float c = rintf(a / w0);
    bad = bad || !(fabsf(c) <= 64.0f) || c == 0.0f || __float_as_uint(c * w0) != __float_as_uint(a);
    return c;
}

// row ordering: one thread per row of [ndata, m), its entries val[ptr[row] .. ptr[row + 1]) <- c (the data rows were copied)
__global__ void k_coef_rows(int m, int ndata, float w0, const long long* __restrict__ ptr, float* __restrict__ val, int* __restrict__ flag)
{
    const int row = ndata + blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= m) return;
    bool bad = false;
    for (long long k = ptr[row]; k < ptr[row + 1]; ++k) val[k] = coef_of(val[k], w0, bad);
    if (bad) atomicOr(flag, 1);
}

// column ordering: one thread per entry, those of the rows from ndata up (idx: 0-based row) <- c
__global__ void k_coef_cols(long long nar, int ndata, float w0, const int* __restrict__ idx, float* __restrict__ val, int* __restrict__ flag)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nar || idx[k] < ndata) return;
    bool bad = false;
    val[k] = coef_of(val[k], w0, bad);
    if (bad) atomicOr(flag, 1);
}

// ---- the measures of dsa_lsmr_tradeoff and dsa_lsmr_crossval, and the held-out residuals of the latter ----

// Measures of member r over its solution x_r: sum over the data rows of (b_i - (A x_r)_i)^2 -- for dsa_lsmr_crossval the rows the member
// keeps and those it holds out apart --, sum over the rows from ndata up of ((C x_r)_i)^2 (val: the row ordering's coefficient copy, so
// C = the integer coefficients), sum of x_r^2; fp64.  k_b_meas_rows: block (b, g), four wavefronts, wavefront w the rows
// [b kMeasR + w kMeasR/4, + kMeasR/4) in order, row_product each; the four wavefronts' sums added in order (block_sum4).  k_b_meas_x: the
// same over the elements of x.  k_b_meas_sum: the blocks' partials in order.
constexpr int kMeasR = 64;                  // rows per block
constexpr int kMeasE = 1024;                // elements of x per block

// (A x)_row of the lane's member (p: its x), fp64: the row's entries added in storage order, value and index wave-uniform, one coalesced
// 256-byte load of x per entry, four entries' loads ahead of their additions (the float x float products are exact in fp64)
__device__ inline double row_product(const long long* __restrict__ ptr, const float* __restrict__ val, const int* __restrict__ idx,
                                     const float* __restrict__ p, int row)
{
    double acc = 0.0;
    long long k = ptr[row];
    const long long k1 = ptr[row + 1];
    constexpr int U = 4;
    for (; k + U <= k1; k += U) {
        double a[U], xi[U];
#pragma unroll
        for (int u = 0; u < U; ++u) { a[u] = (double)val[k + u]; xi[u] = (double)p[(size_t)idx[k + u] * 64]; }
#pragma unroll
        for (int u = 0; u < U; ++u) acc = acc + a[u] * xi[u];
    }
    for (; k < k1; ++k) acc = acc + (double)val[k] * (double)p[(size_t)idx[k] * 64];
    return acc;
}

// The hold predicates of k_b_meas_rows: lane() takes the lane's member, row() says whether the member holds data row `row` (residual d) out.
// kSums sums per lane: {kept misfit, roughness} or {kept misfit, held-out misfit, roughness}.
struct KeepAll {                            // dsa_lsmr_tradeoff: every member keeps every row
    static constexpr int kSums = 2;
    __device__ void lane(int) {}
    __device__ bool row(int, double, double*) const { return false; }
};
// dsa_lsmr_crossval: member r = q * stride + f holds out fold f; the full member (f = stride - 1 = nfolds, no datum's fold) keeps every row,
// so its kept sum and its roughness are KeepAll's additions in KeepAll's order.  The lane that holds row i out stores d to
// resid[(2 q) ndata + i], the full member's lane to resid[(2 q + 1) ndata + i]: every (combo, datum) is written once in each half.
struct HoldFold {
    static constexpr int kSums = 3;
    const int* fold;
    int ndata, nreal, stride;
    int r = 0, q = 0, f = 0;                // the lane's member and its (combo, fold)
    __device__ void lane(int r_) { r = r_; q = r / stride; f = r - q * stride; }
    __device__ bool row(int row, double d, double* __restrict__ resid) const
    {
        const bool held = fold[row] == f, full = f == stride - 1;
        if (resid && r < nreal && (held || full)) resid[(2 * (size_t)q + (full ? 1 : 0)) * (size_t)ndata + (size_t)row] = d;
        return held;
    }
};

// part: Hold::kSums sums per (g, block, lane)
template <class Hold>
__global__ __launch_bounds__(256) void k_b_meas_rows(int m, int n, int ndata, int nb, const long long* __restrict__ ptr, const float* __restrict__ val,
                                                     const int* __restrict__ idx, const float* __restrict__ b, const float* __restrict__ x,
                                                     double* __restrict__ part, double* __restrict__ resid, Hold hold)
{
    constexpr int NS = Hold::kSums;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = blockIdx.y, blk = blockIdx.x;
    hold.lane(g * 64 + lane);
    const float* __restrict__ p = x + (size_t)g * n * 64 + lane;
    const int r0 = blk * kMeasR + w * (kMeasR / 4), r1 = min(r0 + kMeasR / 4, m);
    double s[NS] = {};
    for (int row = r0; row < r1; ++row) {
        const double acc = row_product(ptr, val, idx, p, row);
        if (row < ndata) {
            const double d = (double)b[row] - acc;
            if (hold.row(row, d, resid)) s[1] = s[1] + d * d;
            else s[0] = s[0] + d * d;
        }
        else s[NS - 1] = s[NS - 1] + acc * acc;
    }
    block_sum4(s, part + (((size_t)g * nb + blk) * 64 + lane) * NS);
}

__global__ __launch_bounds__(256) void k_b_meas_x(int n, int nb, const float* __restrict__ x, double* __restrict__ part)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = blockIdx.y, blk = blockIdx.x;
    const float* __restrict__ p = x + (size_t)g * n * 64 + lane;
    const int e0 = blk * kMeasE + w * (kMeasE / 4), e1 = min(e0 + kMeasE / 4, n);
    double s[1] = {0.0};
    for (int e = e0; e < e1; ++e) { const double xv = (double)p[(size_t)e * 64]; s[0] = s[0] + xv * xv; }
    block_sum4(s, part + ((size_t)g * nb + blk) * 64 + lane);
}

// meas[(NS + 1) r ..] = the NS row sums of k_b_meas_rows, then sum x^2; one thread per member
template <int NS>
__global__ __launch_bounds__(64) void k_b_meas_sum(int nbr, int nbx, int nreal, const double* __restrict__ rows, const double* __restrict__ xs,
                                                   double* __restrict__ meas)
{
    const int lane = threadIdx.x, g = blockIdx.x, r = g * 64 + lane;
    if (r >= nreal) return;
    double s[NS + 1] = {};
    for (int b = 0; b < nbr; ++b) {
        const double* __restrict__ q = rows + (((size_t)g * nbr + b) * 64 + lane) * NS;
#pragma unroll
        for (int c = 0; c < NS; ++c) s[c] = s[c] + q[c];
    }
    for (int b = 0; b < nbx; ++b) s[NS] = s[NS] + xs[((size_t)g * nbx + b) * 64 + lane];
#pragma unroll
    for (int c = 0; c <= NS; ++c) meas[(NS + 1) * (size_t)r + c] = s[c];
}

// ---- dsa_lsmr_voronoi: the tessellations, every member's list for the transposed product, the projected products, the ensemble statistics ----

constexpr int kVorTile = 1024;              // seed points staged per pass: 1024 x 3 x 8 B = 24 KB of LDS

// cell_mm[r * n + j] = the seed s in [0, ncells) of member r nearest to unknown j: d2 = ((xj-xs)^2 + (yj-ys)^2) + (zj-zs)^2 in fp64 in that
// association (no contraction), the lowest s on ties.  One thread per (member, unknown): blockIdx.x the unknowns, the y dimension strides
// over the members; the member's seed points pass through LDS in tiles of kVorTile, every thread reads the same one (a broadcast).
__global__ __launch_bounds__(256) void k_v_assign(int n, int ncells, int nreal, const double* __restrict__ xyz, const int* __restrict__ seeds,
                                                  int* __restrict__ cell_mm)
{
    __shared__ double sx[kVorTile], sy[kVorTile], sz[kVorTile];
    const int j = blockIdx.x * 256 + threadIdx.x;
    const size_t jj = (size_t)min(j, n - 1);
    const double x = xyz[3 * jj], y = xyz[3 * jj + 1], z = xyz[3 * jj + 2];
    for (int r = blockIdx.y; r < nreal; r += gridDim.y) {
        const int* __restrict__ sd = seeds + (size_t)r * ncells;
        double best = INFINITY;
        int bi = 0;
        for (int s0 = 0; s0 < ncells; s0 += kVorTile) {
            const int cnt = min(kVorTile, ncells - s0);
            __syncthreads();
            for (int t = threadIdx.x; t < cnt; t += 256) {
                const size_t q = 3 * (size_t)sd[s0 + t];
                sx[t] = xyz[q]; sy[t] = xyz[q + 1]; sz[t] = xyz[q + 2];
            }
            __syncthreads();
            for (int t = 0; t < cnt; ++t) {
                const double dx = x - sx[t], dy = y - sy[t], dz = z - sz[t];
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 < best) { best = d2; bi = s0 + t; }
            }
        }
        if (j < n) cell_mm[(size_t)r * n + j] = bi;
    }
}

// rowof[p] = the row whose segment of the CSR copy holds position p < nnz = ptr[ndata] (the last row with ptr[row] <= p)
__global__ void k_v_rowof(int ndata, long long nnz, const long long* __restrict__ ptr, int* __restrict__ rowof)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nnz) return;
    int lo = 0, hi = ndata;                                           // ptr[lo] <= p < ptr[hi]
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (ptr[mid] <= p) lo = mid; else hi = mid;
    }
    rowof[p] = lo;
}

// The sort of one lane group's lists: item i = (member rl = i / nnz of the group, position p = i % nnz) gets the key rl * ncells + cell of
// member rl at the column of p, and the value p.  A stable sort by key leaves member rl's positions at [rl * nnz, (rl + 1) * nnz), by
// cell, ascending within a cell: the listing order of the member's system.
__global__ void k_v_keys(long long items, long long nnz, int n, int ncells, const int* __restrict__ cell_mm, const int* __restrict__ idx,
                         int* __restrict__ keys, int* __restrict__ pos)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= items) return;
    const long long rl = i / nnz, p = i - rl * nnz;
    keys[i] = (int)rl * ncells + cell_mm[(size_t)rl * (size_t)n + (size_t)idx[p]];
    pos[i] = (int)p;
}

// cptr[rl * (ncells + 1) + c] = where cell c begins in member rl's list: the first sorted item with a key >= rl * ncells + c, less rl * nnz
__global__ void k_v_cptr(int members, int ncells, long long nnz, const int* __restrict__ keys, int* __restrict__ cptr)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)members * (ncells + 1)) return;
    const long long rl = t / (ncells + 1);
    const long long key = rl * ncells + (t - rl * (ncells + 1));
    long long lo = 0, hi = (long long)members * nnz;                  // the first item with keys[item] >= key lies in [lo, hi]
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        if ((long long)keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    cptr[t] = (int)(lo - rl * nnz);
}

// mode 1, first half: vfull(g, j, l) = v(g, cell(g, j, l), l), the member's vector on the unknowns; k_b_spmv<true> over the data rows follows
__global__ void k_v_expand(int n, int ncells, const int* __restrict__ cell, const float* __restrict__ v, float* __restrict__ vfull)
{
    LB_GROUP_LOOP(n) vfull[gbase + t] = v[((size_t)g * ncells + (size_t)cell[gbase + t]) * 64 + (t & 63)];
}

// mode 2: v_r[c] = pre_r * v_r[c] + sum over the entries of member r's cell c, in listing order, of fl(a * u_r[row]), where flag_r.  One
// wavefront per (member, cell), four per block, blocks member-major: the 64 lanes load 64 list entries at a time (position, then value,
// row and operand) and form the products in parallel; the additions run in order onto one wave-uniform accumulator, every term
// broadcast from its lane.  ut: u member-major (ut[r * ndata + row]), so a member's operands are one contiguous vector.
__global__ __launch_bounds__(256) void k_v_colprod(int ncells, int ndata, long long nnz, int nblk, const int* __restrict__ list, const int* __restrict__ cptr,
                                                   const float* __restrict__ val, const int* __restrict__ rowof, const float* __restrict__ ut,
                                                   float* __restrict__ v, const float* __restrict__ pre, const int* __restrict__ flag)
{
    const int lane = threadIdx.x & 63;
    const int r = __builtin_amdgcn_readfirstlane((int)(blockIdx.x / (unsigned)nblk));
    const int c = __builtin_amdgcn_readfirstlane((int)(blockIdx.x % (unsigned)nblk) * 4 + (int)(threadIdx.x >> 6));
    if (c >= ncells || flag[r] == 0) return;
    float* __restrict__ o = v + ((size_t)(r >> 6) * ncells + c) * 64 + (r & 63);
    const int* __restrict__ L = list + (size_t)r * (size_t)nnz;
    const float* __restrict__ u = ut + (size_t)r * ndata;
    float acc = *o;
    if (pre) acc = pre[r] * acc;
    const int k1 = cptr[(size_t)r * (ncells + 1) + c + 1];
    for (int k = cptr[(size_t)r * (ncells + 1) + c]; k < k1; k += 64) {
        float t = 0.0f;
        if (k + lane < k1) {
            const int p = L[k + lane];
            t = val[p] * u[rowof[p]];
        }
        const int cnt = min(64, k1 - k);                              // (wave-uniform; a lane past it holds no term and none is added)
        if (cnt == 64) {
#pragma unroll
            for (int i = 0; i < 64; ++i) acc = acc + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t), i));
        } else
            for (int i = 0; i < cnt; ++i) acc = acc + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t), i));
    }
    if (lane == 0) *o = acc;
}

// stats[j] = the mean, stats[n + j] = the sample standard deviation (0 for nreal = 1) over the members k = 0 .. nreal - 1, in that order, of
// xf(k, j) (xf: a batch vector over the unknowns); fp64, one thread per unknown
__global__ void k_v_stats(int n, int nreal, const float* __restrict__ xf, double* __restrict__ stats)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    auto at = [&](int k) { return (double)xf[((size_t)(k >> 6) * n + j) * 64 + (k & 63)]; };
    double s = 0.0;
    for (int k = 0; k < nreal; ++k) s = s + at(k);
    const double mean = s / (double)nreal;
    double ss = 0.0;
    for (int k = 0; k < nreal; ++k) { const double d = at(k) - mean; ss = ss + d * d; }
    stats[j] = mean;
    stats[(size_t)n + j] = nreal > 1 ? sqrt(ss / (double)(nreal - 1)) : 0.0;
}

// ---- the front door and the layouts of the shared buffers ----

constexpr int kMaxReal = 64 * 65535;        // members of one call (gridDim.y lane groups)

// The checks the entry points share, in the order they fire, their texts carrying the entry point's name.  Each returns 0 or the
// error it has reported.
struct Entry {
    const char* name;
    Engine* e = nullptr;
    int m = 0, n = 0;
    // the handle, then `ok`: the caller's own test of its count (1 .. kMaxReal) and of the pointers it requires, `what` its words for them
    int open(dsa_engine* h, bool ok, const char* what)
    {
        if (!h) return DSA_ERR_ARGUMENT;
        e = reinterpret_cast<Engine*>(h);
        if (!ok) { e->fail(DSA_ERR_ARGUMENT, "%s: %s", name, what); return DSA_ERR_ARGUMENT; }
        return 0;
    }
    // a resident matrix (m, n <- its shape) and, where the entry point has data rows (ndata not null), ndata in 1 .. m
    int matrix(const int* ndata)
    {
        if (!e->spmv) { e->fail(DSA_ERR_STATE, "%s: no matrix (call dsa_spmv_load or dsa_iteration_system_device first)", name); return DSA_ERR_STATE; }
        m = e->spmv->m; n = e->spmv->n;
        if (ndata && (*ndata < 1 || *ndata > m)) { e->fail(DSA_ERR_ARGUMENT, "%s: ndata %d outside 1..%d", name, *ndata, m); return DSA_ERR_ARGUMENT; }
        return 0;
    }
    // the entry points that rebuild every row below the data with a member's weight: not on the radial system, whose tie rows lie there too
    int no_tie_rows()
    {
        if (e->spmv && e->spmv->radial) { e->fail(DSA_ERR_STATE, "%s: the resident matrix is the radial system, whose tie rows below the data would be rescaled with the Laplacian rows", name); return DSA_ERR_STATE; }
        return 0;
    }
    // weight0 finite and > 0, then the `count` (weight, damp) pairs of the `noun`s ("member", "combo") finite and >= 0
    int weights(float weight0, int count, const char* noun, const float* weight, const float* damp)
    {
        if (!std::isfinite(weight0) || !(weight0 > 0.0f)) { e->fail(DSA_ERR_ARGUMENT, "%s: weight0 %g is not a finite number > 0", name, (double)weight0); return DSA_ERR_ARGUMENT; }
        for (int r = 0; r < count; ++r)
            if (!std::isfinite(weight[r]) || weight[r] < 0.0f || !std::isfinite(damp[r]) || damp[r] < 0.0f) {
                e->fail(DSA_ERR_ARGUMENT, "%s: %s %d has weight %g, damp %g (both must be finite and >= 0)", name, noun, r, (double)weight[r], (double)damp[r]);
                return DSA_ERR_ARGUMENT;
            }
        return 0;
    }
};

// A bump allocator over one shared device buffer (btmp: floats, ints through at<int>; bpsf: doubles).  An entry point declares its pieces
// once, in order: take() returns a piece's offset and grows `total`, which sizes the buffer; once the buffer stands, at() is the piece's
// pointer.  reuse() starts again at the bottom: what is taken after it lies over pieces that are dead by the time it is written.
template <class T>
struct Carve {
    size_t top = 0, total = 0;
    size_t take(size_t count) { const size_t off = top; top += count; total = std::max(total, top); return off; }
    void reuse() { top = 0; }
    template <class V = T>
    V* at(const DevBuf<T>& buf, size_t off) const { static_assert(sizeof(V) == sizeof(T), "pieces are counted in units of T"); return reinterpret_cast<V*>(buf.p + off); }
};

// ---- the batch of all entry points: set-up (batch_begin), then -- once the caller has filled u and the row scales -- the LSMR loop
// (batch_solve) and, for two of them, the measures (batch_measures) ----
struct Batch {
    Engine* e = nullptr;
    SpmvState* S = nullptr;
    int m = 0, n = 0, G = 0, Rp = 0, localVecs = 0;      // m, n: lengths of the batch vectors (the solved system's)
    int nfull = 0;                                       // columns of the resident matrix: n, but for dsa_lsmr_voronoi (n = ncells)
    size_t vm = 0, vn = 0;
    hipStream_t st = nullptr;
    // host mirror of bparam, then Rp norms.  The host writes the mirror only after a synchronisation that follows the previous upload.
    float* hc = nullptr;
    int* hf = nullptr;
    float* hred = nullptr;
    const float* rval = nullptr;     // values the products read beside row_csr / col_csr (batch_begin: the resident ones; dsa_lsmr_tradeoff: the coefficient copy)
    const float* cval = nullptr;
    bool projected = false;          // dsa_lsmr_voronoi: product() multiplies by the member's projected matrix
    long long pnnz = 0;              // ... entries of the data rows
    int preal = 0;                   // ... members
    float* xout = nullptr;           // the entry point's piece of btmp for the solutions on their way out (batch_solve with x)

    const float* coef(int f) const { return S->bparam.p + (size_t)f * Rp; }
    const int* flag(int f) const { return reinterpret_cast<const int*>(S->bparam.p + (size_t)NCOEF * Rp) + (size_t)f * Rp; }
    int upload() { LB_TRY(e, hipMemcpyAsync(S->bparam.p, S->hbatch, (size_t)kNParam * Rp * 4, hipMemcpyHostToDevice, st)); return 0; }
    // dnrm2 of every realisation's v (len elements): terms and scales by the wide kernels, then the chains
    int norm(int len, const float* v)
    {
        const int nb = (len + kPB - 1) / kPB;
        hipLaunchKernelGGL(k_pm_blockmax, dim3((unsigned)nb, (unsigned)G), dim3(256), 0, st, len, nb, v, S->bpmax.p);
        hipLaunchKernelGGL(k_pm_scan, dim3(G), dim3(64), 0, st, nb, S->bpmax.p, S->bred.p + 2 * (size_t)Rp);
        hipLaunchKernelGGL(k_pm_terms, dim3((unsigned)nb, (unsigned)G), dim3(256), 0, st, len, nb, v, (const float*)S->bpmax.p, S->bterm.p);
        hipLaunchKernelGGL(k_b_chain<false>, dim3(G), dim3(kCT), 0, st, len, (const float*)S->bterm.p, (const float*)nullptr,
                           (const float*)(S->bred.p + 2 * (size_t)Rp), v, S->bred.p);
        LB_TRY(e, hipMemcpyAsync(hred, S->bred.p, (size_t)Rp * 4, hipMemcpyDeviceToHost, st));
        LB_TRY(e, hipStreamSynchronize(st));
        return 0;
    }
    // mode 1: u = pre_r u + A v; mode 2: v = pre_r v + A' u (where the flag is set)
    void product(int mode, const float* pre, const int* fl)
    {
        if (projected) { projected_product(mode, pre, fl); return; }
        if (mode == 1) spmv<true>(m, n, S->row_csr, rval, S->bv.p, S->bu.p, pre, fl);
        else spmv<false>(n, m, S->col_csr, cval, S->bu.p, S->bv.p, pre, fl);
    }
    // k_b_spmv over the nseg segments of a contiguous ordering M with the values val: out = pre_r out + (rows or columns) in, in of nin elements
    template <bool ROW>
    void spmv(int nseg, int nin, const SpmvState::Contiguous& M, const float* val, const float* in, float* out, const float* pre, const int* fl)
    {
        hipLaunchKernelGGL(k_b_spmv<ROW>, dim3((unsigned)((nseg + 3) / 4), (unsigned)G), dim3(256), 0, st, nseg, nin, M.ptr.p, val, M.idx.p,
                           (const float*)S->bscale.p, in, out, pre, fl);
    }
    // u and the row scales of every member under `rule` from the device copies of b (none: u = 0) and of what the rule reads: par, and for
    // FILL_WEIGHT / FILL_FOLD the first regularisation row ndata, for FILL_FOLD the members per combo and the folds
    void fill(Fill rule, int nreal, const float* b, const float* par = nullptr, int ndata = 0, int stride = 1, const int* fold = nullptr)
    {
        hipLaunchKernelGGL(k_b_fill, grid_of(m, G), dim3(256), 0, st, rule, m, ndata, nreal, stride, b, par, fold, S->bscale.p, S->bu.p);
    }
    // The same for member k's M_k (the data rows, column j relabelled cell_k(j); n = ncells).  Mode 1: v expanded to the unknowns, then the
    // resident data rows (row scales 1: fl(a * 1) = a) -- row i adds a * v[cell(col)] in storage order.  Mode 2: u member-major, then
    // every (member, cell) adds its list in order.
    void projected_product(int mode, const float* pre, const int* fl)
    {
        if (mode == 1) {
            hipLaunchKernelGGL(k_v_expand, grid_of(nfull, G), dim3(256), 0, st, nfull, n, (const int*)S->vcell.p, (const float*)S->bv.p, S->vfull.p);
            spmv<true>(m, nfull, S->row_csr, rval, S->vfull.p, S->bu.p, pre, fl);
        } else {
            hipLaunchKernelGGL(k_b_gather, dim3((unsigned)std::min(1024, (m + 255) / 256), (unsigned)std::min(preal, 65535)), dim3(256), 0, st, m, preal,
                               (const float*)S->bu.p, S->vut.p);
            const int nblk = (n + 3) / 4;
            hipLaunchKernelGGL(k_v_colprod, dim3((unsigned)((size_t)nblk * preal)), dim3(256), 0, st, n, m, pnnz, nblk, (const int*)S->vlist.p, (const int*)S->vcptr.p,
                               rval, (const int*)S->vrowof.p, (const float*)S->vut.p, S->bv.p, pre, fl);
        }
    }
};

// contiguous copies, buffers for nreal realisations (btmp: `tmp` floats), the host mirror cleared.  rows / cols > 0: the batch vectors
// have these lengths in place of the resident matrix's (dsa_lsmr_voronoi: ndata, ncells)
int batch_begin(Engine* e, int nreal, int localSize, size_t tmp, Batch& B, int rows = 0, int cols = 0)
{
    SpmvState& S = *e->spmv;
    B.e = e; B.S = &S;
    S.bx_valid = false;                                       // (bx is about to change; batch_solve marks what it leaves)
    const int m = rows > 0 ? rows : S.m, n = cols > 0 ? cols : S.n, G = (nreal + 63) / 64, Rp = 64 * G;
    B.m = m; B.n = n; B.nfull = S.n; B.G = G; B.Rp = Rp;
    B.localVecs = std::max(0, std::min(localSize, std::min(m, n)));                              // :365
    B.vm = (size_t)G * m * 64; B.vn = (size_t)G * n * 64;
    B.st = e->stream;
    const size_t vm = B.vm, vn = B.vn;
    LB_TRY(e, hipSetDevice(e->device));
    LB_DO(spmv_ensure_contiguous(e));
    B.rval = S.row_csr.val.p; B.cval = S.col_csr.val.p;
    if (e->ensure(S.bu, vm) || e->ensure(S.bscale, vm) || e->ensure(S.bv, vn) || e->ensure(S.bh, vn) || e->ensure(S.bhbar, vn) || e->ensure(S.bx, vn) ||
        e->ensure(S.blocalV, std::max<size_t>(vn * (size_t)B.localVecs, 1)) || e->ensure(S.bparam, (size_t)kNParam * Rp) || e->ensure(S.bred, 3 * (size_t)Rp) ||
        e->ensure(S.bterm, std::max(vm, vn)) || e->ensure(S.bpmax, (size_t)G * ((std::max(m, n) + kPB - 1) / kPB) * 64) ||
        e->ensure(S.btmp, std::max<size_t>(tmp, 1))) return e->status;
    const size_t hwords = (size_t)(kNParam + 1) * Rp;
    if (S.hbatch_cap < hwords) {
        if (S.hbatch) (void)hipHostFree(S.hbatch);
        S.hbatch = nullptr; S.hbatch_cap = 0;
        LB_TRY(e, hipHostMalloc(reinterpret_cast<void**>(&S.hbatch), hwords * 4, hipHostMallocDefault));
        S.hbatch_cap = hwords;
    }
    B.hc = S.hbatch;
    B.hf = reinterpret_cast<int*>(S.hbatch + (size_t)NCOEF * Rp);
    B.hred = S.hbatch + (size_t)kNParam * Rp;
    std::memset(S.hbatch, 0, hwords * 4);
    return 0;
}

// The LSMR loop of every realisation from u (bu) and the row scales (bscale) the caller filled: v = x = hbar = 0 (:383-385), ...;
// istop, itn, est per realisation and, where x is not null, the solutions (realisation-major, through B.xout).  bx keeps them.
// Realisation r is damped by damp[r / per] (per = 1: one each; nreal: one for all; nfolds + 1: one per combo).
int batch_solve(Batch& B, int nreal, const float* damp, int per, float atol, float btol, float conlim, int itnlim, float* x, int* istop, int* itn, float* est)
{
    Engine* e = B.e;
    SpmvState& S = *B.S;
    const int m = B.m, n = B.n, G = B.G, Rp = B.Rp, localVecs = B.localVecs;
    const size_t vn = B.vn;
    hipStream_t st = B.st;
    float* hc = B.hc;
    int* hf = B.hf;
    const float* hred = B.hred;
    const float* dc = B.coef(0);
    const int* df = B.flag(0);
    LB_TRY(e, hipMemsetAsync(S.bv.p, 0, vn * 4, st));
    LB_TRY(e, hipMemsetAsync(S.bx.p, 0, vn * 4, st));
    LB_TRY(e, hipMemsetAsync(S.bhbar.p, 0, vn * 4, st));
    std::vector<LsmrScalars> P;
    P.reserve((size_t)nreal);
    for (int r = 0; r < nreal; ++r) P.emplace_back(damp[r / per], atol, btol, conlim, itnlim, localVecs);
    std::vector<char> running((size_t)nreal, 0);
    std::vector<float> alpha0((size_t)nreal, 0.0f), beta0((size_t)nreal, 0.0f);
    LB_DO(B.norm(m, S.bu.p));                                                                      // beta = |u|
    bool any = false;
    for (int r = 0; r < nreal; ++r) {
        beta0[r] = hred[r];
        const bool pos = beta0[r] > 0.0f;
        hf[F_BPOS * Rp + r] = pos;
        hc[C_IBETA * Rp + r] = pos ? 1.0f / beta0[r] : 0.0f;
        any = any || pos;
    }
    if (any) {
        LB_DO(B.upload());
        hipLaunchKernelGGL(k_b_scal, grid_of(m, G), dim3(256), 0, st, m, B.coef(C_IBETA), B.flag(F_BPOS), S.bu.p);      // u = u / beta
        B.product(2,nullptr, B.flag(F_BPOS));                                                                       // v = A'u
        LB_DO(B.norm(n, S.bv.p));                                                                                  // alpha = |v|
        for (int r = 0; r < nreal; ++r) {
            alpha0[r] = hf[F_BPOS * Rp + r] ? hred[r] : 0.0f;
            hf[F_APOS * Rp + r] = alpha0[r] > 0.0f;
            hc[C_IALPHA * Rp + r] = alpha0[r] > 0.0f ? 1.0f / alpha0[r] : 0.0f;
        }
        LB_DO(B.upload());
        hipLaunchKernelGGL(k_b_scal, grid_of(n, G), dim3(256), 0, st, n, B.coef(C_IALPHA), B.flag(F_APOS), S.bv.p);     // v = v / alpha
    }
    int nrun = 0;
    for (int r = 0; r < nreal; ++r) nrun += (running[r] = P[r].start(alpha0[r], beta0[r]));
    const bool localOrtho = localVecs > 0;
    if (nrun > 0) {
        if (localOrtho) LB_TRY(e, hipMemcpyAsync(S.blocalV.p, S.bv.p, vn * 4, hipMemcpyDeviceToDevice, st));                // :408-413
        LB_TRY(e, hipMemcpyAsync(S.bh.p, S.bv.p, vn * 4, hipMemcpyDeviceToDevice, st));
        LB_TRY(e, hipStreamSynchronize(st));                  // (the last upload has landed before the host mirror changes)
    }
    while (nrun > 0) {                                                                           // :480
        for (int r = 0; r < Rp; ++r) {
            const bool on = r < nreal && running[r];
            hf[F_ACT * Rp + r] = on;
            if (on) { P[r].itn += 1; hc[C_PRE_U * Rp + r] = -P[r].alpha; }
        }
        LB_DO(B.upload());
        B.product(1,B.coef(C_PRE_U), B.flag(F_ACT));                                                  // u = A v - alpha u
        LB_DO(B.norm(m, S.bu.p));                                                                  // beta = |u|
        int maxlim = 0;
        any = false;
        for (int r = 0; r < nreal; ++r) {
            hf[F_BPOS * Rp + r] = 0; hf[F_SLOT * Rp + r] = -1; hf[F_LIM * Rp + r] = 0; hf[F_APOS * Rp + r] = 0;
            if (!running[r]) continue;
            LsmrScalars& p = P[r];
            p.beta = hred[r];
            if (!(p.beta > 0.0f)) continue;
            any = true;
            hf[F_BPOS * Rp + r] = 1;
            hc[C_IBETA * Rp + r] = 1.0f / p.beta;
            hc[C_PRE_V * Rp + r] = -p.beta;
            if (p.localOrtho) {                                                                  // localVEnqueue, :715-727
                hf[F_SLOT * Rp + r] = p.enqueue_slot();
                hf[F_LIM * Rp + r] = p.ortho_count();
                maxlim = std::max(maxlim, p.ortho_count());
            }
        }
        if (any) {
            LB_DO(B.upload());
            hipLaunchKernelGGL(k_b_scal, grid_of(m, G), dim3(256), 0, st, m, B.coef(C_IBETA), B.flag(F_BPOS), S.bu.p);  // u = u / beta
            if (localOrtho)
                hipLaunchKernelGGL(k_b_enqueue, grid_of(n, G), dim3(256), 0, st, n, vn, B.flag(F_SLOT), (const float*)S.bv.p, S.blocalV.p);
            B.product(2,B.coef(C_PRE_V), B.flag(F_BPOS));                                             // v = A'u - beta v
            for (int k = 0; k < maxlim; ++k) {                                                   // localVOrtho, :731-748
                const float* lv = S.blocalV.p + (size_t)k * vn;
                hipLaunchKernelGGL(k_b_chain<true>, dim3(G), dim3(kCT), 0, st, n, (const float*)S.bv.p, lv, (const float*)nullptr, (const float*)nullptr,
                                   S.bred.p + Rp);
                hipLaunchKernelGGL(k_b_axmy, grid_of(n, G), dim3(256), 0, st, n, k, (const float*)(S.bred.p + Rp), B.flag(F_LIM), lv, S.bv.p);
            }
            LB_DO(B.norm(n, S.bv.p));                                                              // alpha = |v|
            for (int r = 0; r < nreal; ++r) {
                if (!hf[F_BPOS * Rp + r]) continue;
                LsmrScalars& p = P[r];
                p.alpha = hred[r];
                if (p.alpha > 0.0f) { hf[F_APOS * Rp + r] = 1; hc[C_IALPHA * Rp + r] = 1.0f / p.alpha; }
            }
        }
        for (int r = 0; r < nreal; ++r) {
            if (!running[r]) continue;
            LsmrScalars& p = P[r];
            p.rotate();                                                                          // :516-600
            hc[C_C1 * Rp + r] = p.c1; hc[C_C2 * Rp + r] = p.c2; hc[C_C3 * Rp + r] = p.c3;
        }
        LB_DO(B.upload());
        hipLaunchKernelGGL(k_b_update, grid_of(n, G), dim3(256), 0, st, n, dc, df, S.bv.p, S.bh.p, S.bhbar.p, S.bx.p, Rp);   // :508, :545-547
        LB_DO(B.norm(n, S.bx.p));                                                                  // normx
        for (int r = 0; r < nreal; ++r)
            if (running[r] && P[r].converged(hred[r])) { running[r] = 0; --nrun; }
    }
    for (int r = 0; r < nreal; ++r) {
        LsmrScalars& p = P[r];
        p.finish();
        istop[r] = p.istop; itn[r] = p.itn;
        float* q = est + (size_t)5 * r;
        q[0] = p.normA; q[1] = p.condA; q[2] = p.normr; q[3] = p.normAr; q[4] = p.normx;
    }
    if (x) {
        hipLaunchKernelGGL(k_b_gather, dim3((unsigned)std::min(1024, (n + 255) / 256), (unsigned)std::min(nreal, 65535)), dim3(256), 0, st, n, nreal,
                           (const float*)S.bx.p, B.xout);
        LB_TRY(e, hipMemcpyAsync(x, B.xout, (size_t)nreal * n * 4, hipMemcpyDeviceToHost, st));
    }
    LB_DO(drain(e, st));
    // what bx holds now can be a later call's steps (dsa_forward_steps), unless it is in cell space (dsa_lsmr_voronoi)
    S.bx_valid = !B.projected; S.bx_nreal = nreal; S.bx_n = n;
    return 0;
}

// The coefficient copy of both contiguous value arrays for data rows [0, ndata) and regularisation rows built with weight0: the
// resident values, the entries of the rows from ndata up replaced by c = rint(a / weight0).  Kept until the matrix changes
// (spmv_invalidate_contiguous) or the key (ndata, weight0) does.  DSA_ERR_ARGUMENT when an entry is not fl(c * weight0), 0 < |c| <= 64.
int ensure_coef(Engine* e, int ndata, float weight0)
{
    SpmvState& S = *e->spmv;
    if (S.coef_valid && S.coef_ndata == ndata && std::memcmp(&S.coef_weight0, &weight0, 4) == 0) return 0;
    S.coef_valid = false;
    hipStream_t st = e->stream;
    const size_t nn = std::max<size_t>((size_t)S.nar, 1);
    if (e->ensure(S.row_coef, nn) || e->ensure(S.col_coef, nn) || e->ensure(S.bflag, 1)) return e->status;
    LB_TRY(e, hipMemsetAsync(S.bflag.p, 0, 4, st));
    if (S.nar > 0) {
        LB_TRY(e, hipMemcpyAsync(S.row_coef.p, S.row_csr.val.p, (size_t)S.nar * 4, hipMemcpyDeviceToDevice, st));
        LB_TRY(e, hipMemcpyAsync(S.col_coef.p, S.col_csr.val.p, (size_t)S.nar * 4, hipMemcpyDeviceToDevice, st));
        if (ndata < S.m)
            hipLaunchKernelGGL(k_coef_rows, dim3((unsigned)((S.m - ndata + 255) / 256)), dim3(256), 0, st, S.m, ndata, weight0, (const long long*)S.row_csr.ptr.p,
                               S.row_coef.p, S.bflag.p);
        hipLaunchKernelGGL(k_coef_cols, dim3((unsigned)((S.nar + 255) / 256)), dim3(256), 0, st, S.nar, ndata, weight0, (const int*)S.col_csr.idx.p, S.col_coef.p,
                           S.bflag.p);
    }
    int bad = 0;
    LB_TRY(e, hipMemcpyAsync(&bad, S.bflag.p, 4, hipMemcpyDeviceToHost, st));
    LB_DO(drain(e, st));
    if (bad) {
        e->fail(DSA_ERR_ARGUMENT, "lsmr_tradeoff: a regularisation entry (rows from %d up) is not an integer coefficient of 1..64 times weight0 = %g", ndata, (double)weight0);
        return DSA_ERR_ARGUMENT;
    }
    S.coef_valid = true; S.coef_ndata = ndata; S.coef_weight0 = weight0;
    return 0;
}

// The measures of every solution in bx over the system's b (d_b) and, for HoldFold, every datum's residuals: the layout of bpsf (block
// partials of the rows and of x, the results, the nres residuals), three launches, the copies back.  measures: Hold::kSums + 1 per member,
// or null (then resid is not: the rows' kernel alone)
template <class Hold>
int batch_measures(Batch& B, int nreal, int ndata, const float* d_b, Hold hold, double* measures, double* resid, size_t nres)
{
    constexpr int NS = Hold::kSums;
    Engine* e = B.e;
    SpmvState& S = *B.S;
    const int m = B.m, n = B.n, G = B.G;
    hipStream_t st = B.st;
    const int nbr = (m + kMeasR - 1) / kMeasR, nbx = (n + kMeasE - 1) / kMeasE;
    Carve<double> P;
    const size_t o_rows = P.take((size_t)G * nbr * 64 * NS), o_x = P.take((size_t)G * nbx * 64), o_meas = P.take((NS + 1) * (size_t)B.Rp), o_resid = P.take(nres);
    if (e->ensure(S.bpsf, P.total)) return e->status;
    double *d_rows = P.at(S.bpsf, o_rows), *d_x = P.at(S.bpsf, o_x), *d_meas = P.at(S.bpsf, o_meas), *d_resid = resid ? P.at(S.bpsf, o_resid) : nullptr;
    hipLaunchKernelGGL(k_b_meas_rows<Hold>, dim3((unsigned)nbr, (unsigned)G), dim3(256), 0, st, m, n, ndata, nbr, (const long long*)S.row_csr.ptr.p,
                       (const float*)S.row_coef.p, (const int*)S.row_csr.idx.p, d_b, (const float*)S.bx.p, d_rows, d_resid, hold);
    if (measures) {
        hipLaunchKernelGGL(k_b_meas_x, dim3((unsigned)nbx, (unsigned)G), dim3(256), 0, st, n, nbx, (const float*)S.bx.p, d_x);
        hipLaunchKernelGGL(k_b_meas_sum<NS>, dim3((unsigned)G), dim3(64), 0, st, nbr, nbx, nreal, (const double*)d_rows, (const double*)d_x, d_meas);
        LB_TRY(e, hipMemcpyAsync(measures, d_meas, (NS + 1) * (size_t)nreal * 8, hipMemcpyDeviceToHost, st));
    }
    if (resid) LB_TRY(e, hipMemcpyAsync(resid, d_resid, nres * 8, hipMemcpyDeviceToHost, st));
    return drain(e, st);
}

// dsa_lsmr_tradeoff and dsa_lsmr_crossval from the layout of btmp to the measures: nreal members on the coefficient copy, member r with
// weight[r / per] and damp[r / per]; fold null (per = 1: every member keeps every row) or the fold of every datum (per = nfolds + 1)
int weighted_solve(Entry& in, int nreal, int per, int ndata, const float* b, float weight0, const float* weight, const float* damp, const int* fold, float atol,
                   float btol, float conlim, int itnlim, int localSize, float* x, double* measures, double* resid, size_t nres, int* istop, int* itn, float* est)
{
    Engine* e = in.e;
    const int m = in.m, n = in.n, npar = nreal / per;
    // btmp: the solutions on their way out (member-major), then b, the weights and the fold of every datum (b and fold stay for the measures)
    Carve<float> T;
    const size_t o_x = T.take(x ? (size_t)nreal * n : 0), o_b = T.take((size_t)m), o_w = T.take((size_t)npar), o_fold = T.take(fold ? (size_t)ndata : 0);
    Batch B;
    LB_DO(batch_begin(e, nreal, localSize, T.total, B));
    LB_DO(ensure_coef(e, ndata, weight0));
    SpmvState& S = *e->spmv;
    B.rval = S.row_coef.p; B.cval = S.col_coef.p;
    B.xout = T.at(S.btmp, o_x);
    float *d_b = T.at(S.btmp, o_b), *d_w = T.at(S.btmp, o_w);
    int* d_fold = fold ? T.at<int>(S.btmp, o_fold) : nullptr;
    LB_TRY(e, hipMemcpyAsync(d_b, b, (size_t)m * 4, hipMemcpyHostToDevice, B.st));
    LB_TRY(e, hipMemcpyAsync(d_w, weight, (size_t)npar * 4, hipMemcpyHostToDevice, B.st));
    if (fold) LB_TRY(e, hipMemcpyAsync(d_fold, fold, (size_t)ndata * 4, hipMemcpyHostToDevice, B.st));
    B.fill(fold ? FILL_FOLD : FILL_WEIGHT, nreal, d_b, d_w, ndata, per, d_fold);
    LB_DO(batch_solve(B, nreal, damp, per, atol, btol, conlim, itnlim, x, istop, itn, est));
    if (!measures && !resid) return 0;
    if (fold) return batch_measures(B, nreal, ndata, d_b, HoldFold{d_fold, ndata, nreal, per}, measures, resid, nres);
    return batch_measures(B, nreal, ndata, d_b, KeepAll{}, measures, nullptr, 0);
}

// the spikes spike_first .. spike_first + nreal - 1 lie in [0, n)
int spike_range(Entry& in, int spike_first, int nreal)
{
    if (spike_first >= 0 && (long long)spike_first + nreal <= in.n) return 0;
    in.e->fail(DSA_ERR_ARGUMENT, "%s: spikes %d..%lld outside the %d unknowns", in.name, spike_first, (long long)spike_first + nreal - 1, in.n);
    return DSA_ERR_ARGUMENT;
}

// The solves dsa_lsmr_resolution and dsa_resolution_blocks share, from the layout of btmp to batch_solve: v = the test models (host
// models scattered, or unit spikes made in place), row scales 1 and u = 0, u = A v over every row (k_b_spmv: fl(a * 1) = a, the chain of
// dsa_spmv mode 1 from y = 0), rows [ndata, m) = +0, then the LSMR loop.  B is left for the caller's measures.
int resolution_solve(Entry& in, Batch& B, int nreal, int ndata, const float* models, int spike_first, float damp, float atol, float btol, float conlim,
                     int itnlim, int localSize, float* x, int* istop, int* itn, float* est)
{
    Engine* e = in.e;
    const int m = in.m, n = in.n;
    // btmp: the host models (realisation-major), dead once they are scattered; the solutions on their way out lie over them
    Carve<float> T;
    const size_t o_mod = T.take(models ? (size_t)nreal * n : 0);
    T.reuse();
    const size_t o_x = T.take(x ? (size_t)nreal * n : 0);
    LB_DO(batch_begin(e, nreal, localSize, T.total, B));
    SpmvState& S = *e->spmv;
    const int G = B.G, Rp = B.Rp;
    hipStream_t st = B.st;
    B.xout = T.at(S.btmp, o_x);
    if (models) {
        float* d_mod = T.at(S.btmp, o_mod);
        LB_TRY(e, hipMemcpyAsync(d_mod, models, (size_t)nreal * n * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_b_scatter<float>, grid_of(n, G), dim3(256), 0, st, n, nreal, (const float*)d_mod, S.bv.p);
    } else
        hipLaunchKernelGGL(k_b_spike, grid_of(n, G), dim3(256), 0, st, n, nreal, spike_first, S.bv.p);
    B.fill(FILL_ONE, nreal, nullptr);
    for (int r = 0; r < nreal; ++r) B.hf[F_ACT * Rp + r] = 1;
    LB_DO(B.upload());
    B.product(1, nullptr, B.flag(F_ACT));
    if (ndata < m) hipLaunchKernelGGL(k_b_zero_rows, grid_of(m - ndata, G), dim3(256), 0, st, m, ndata, S.bu.p);
    LB_TRY(e, hipStreamSynchronize(st));                      // (the upload has landed before the host mirror changes)
    for (int r = 0; r < nreal; ++r) B.hf[F_ACT * Rp + r] = 0;
    return batch_solve(B, nreal, &damp, nreal, atol, btol, conlim, itnlim, x, istop, itn, est);
}

}  // namespace

}  // namespace dsa

extern "C" {

int dsa_lsmr_batch(dsa_engine* h_, int nreal, const float* b, const float* row_scale, float damp, float atol, float btol, float conlim, int itnlim,
                   int localSize, float* x, int* istop, int* itn, float* est)
{
    using namespace dsa;
    Entry in{"lsmr_batch"};
    LB_DO(in.open(h_, nreal >= 1 && nreal <= kMaxReal && b && row_scale && x && istop && itn && est, "nreal < 1 or a null argument"));
    LB_DO(in.matrix(nullptr));
    Engine* e = in.e;
    const int m = in.m, n = in.n;
    // btmp: the row scales and b, dead once u is filled; the solutions on their way out lie over them
    Carve<float> T;
    const size_t o_rs = T.take((size_t)nreal * m), o_b = T.take((size_t)m);
    T.reuse();
    const size_t o_x = T.take((size_t)nreal * n);
    Batch B;
    LB_DO(batch_begin(e, nreal, localSize, T.total, B));
    SpmvState& S = *e->spmv;
    float *d_rs = T.at(S.btmp, o_rs), *d_b = T.at(S.btmp, o_b);
    B.xout = T.at(S.btmp, o_x);
    LB_TRY(e, hipMemcpyAsync(d_rs, row_scale, (size_t)nreal * m * 4, hipMemcpyHostToDevice, B.st));
    LB_TRY(e, hipMemcpyAsync(d_b, b, (size_t)m * 4, hipMemcpyHostToDevice, B.st));
    B.fill(FILL_ROWS, nreal, d_b, d_rs);
    return batch_solve(B, nreal, &damp, nreal, atol, btol, conlim, itnlim, x, istop, itn, est);
}

int dsa_lsmr_resolution(dsa_engine* h_, int nreal, int ndata, const float* models, int spike_first, const double* coords, float damp, float atol,
                        float btol, float conlim, int itnlim, int localSize, float* x, double* psf, int* istop, int* itn, float* est)
{
    using namespace dsa;
    Entry in{"lsmr_resolution"};
    LB_DO(in.open(h_, nreal >= 1 && nreal <= kMaxReal && istop && itn && est, "nreal < 1 or a null istop / itn / est"));
    LB_DO(in.matrix(&ndata));
    Engine* e = in.e;
    const int n = in.n;
    if (!models) LB_DO(spike_range(in, spike_first, nreal));
    if (psf && (models || !coords)) { e->fail(DSA_ERR_ARGUMENT, "lsmr_resolution: psf needs spikes (models NULL) and coords"); return DSA_ERR_ARGUMENT; }
    Batch B;
    LB_DO(resolution_solve(in, B, nreal, ndata, models, spike_first, damp, atol, btol, conlim, itnlim, localSize, x, istop, itn, est));
    SpmvState& S = *e->spmv;
    const int G = B.G, Rp = B.Rp;
    hipStream_t st = B.st;
    if (!psf) return 0;
    // bpsf: the blocks' partials, then the results
    const int nb = (n + kPsfE - 1) / kPsfE;
    Carve<double> P;
    const size_t o_part = P.take((size_t)G * nb * 64 * 3), o_psf = P.take(4 * (size_t)Rp);
    if (e->ensure(S.bcoord, 4 * (size_t)n) || e->ensure(S.bpsf, P.total)) return e->status;
    double *d_part = P.at(S.bpsf, o_part), *d_psf = P.at(S.bpsf, o_psf), *d_cos = S.bcoord.p + 3 * (size_t)n;
    LB_TRY(e, hipMemcpyAsync(S.bcoord.p, coords, 3 * (size_t)n * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_psf_cos, dim3((unsigned)std::min(1024, (n + 255) / 256)), dim3(256), 0, st, n, (const double*)S.bcoord.p, d_cos);
    hipLaunchKernelGGL(k_b_psf_part, dim3((unsigned)nb, (unsigned)G), dim3(256), 0, st, n, nb, spike_first, (const double*)S.bcoord.p, (const double*)d_cos,
                       (const float*)S.bx.p, d_part);
    hipLaunchKernelGGL(k_b_psf_sum, dim3((unsigned)G), dim3(64), 0, st, n, nb, nreal, spike_first, (const float*)S.bx.p, (const double*)d_part, d_psf);
    LB_TRY(e, hipMemcpyAsync(psf, d_psf, 4 * (size_t)nreal * 8, hipMemcpyDeviceToHost, st));
    return drain(e, st);
}

int dsa_resolution_blocks(dsa_engine* h_, int nreal, int ndata, int nblocks, int spike_first, const double* coords, float damp, float atol, float btol,
                               float conlim, int itnlim, int localSize, float* x, double* psf, int* istop, int* itn, float* est)
{
    using namespace dsa;
    Entry in{"resolution_blocks"};
    LB_DO(in.open(h_, nreal >= 1 && nreal <= kMaxReal && coords && psf && istop && itn && est, "nreal < 1 or a null coords / psf / istop / itn / est"));
    LB_DO(in.matrix(&ndata));
    Engine* e = in.e;
    const int n = in.n;
    if (nblocks < 1 || n % nblocks != 0) { e->fail(DSA_ERR_ARGUMENT, "resolution_blocks: the %d unknowns are not %d blocks of equal size", n, nblocks); return DSA_ERR_ARGUMENT; }
    LB_DO(spike_range(in, spike_first, nreal));
    Batch B;
    LB_DO(resolution_solve(in, B, nreal, ndata, nullptr, spike_first, damp, atol, btol, conlim, itnlim, localSize, x, istop, itn, est));
    SpmvState& S = *e->spmv;
    const int G = B.G, nbc = n / nblocks, nch = (nbc + kPsfE - 1) / kPsfE;
    hipStream_t st = B.st;
    // bpsf: the chunks' partials, then the results
    Carve<double> P;
    const size_t o_part = P.take((size_t)G * nblocks * nch * 64 * 3), o_psf = P.take(4 * (size_t)nblocks * B.Rp);
    if (e->ensure(S.bcoord, 4 * (size_t)nbc) || e->ensure(S.bpsf, P.total)) return e->status;
    double *d_part = P.at(S.bpsf, o_part), *d_psf = P.at(S.bpsf, o_psf), *d_cos = S.bcoord.p + 3 * (size_t)nbc;
    LB_TRY(e, hipMemcpyAsync(S.bcoord.p, coords, 3 * (size_t)nbc * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_psf_cos, dim3((unsigned)std::min(1024, (nbc + 255) / 256)), dim3(256), 0, st, nbc, (const double*)S.bcoord.p, d_cos);
    hipLaunchKernelGGL(k_b_psf_blocks_part, dim3((unsigned)(nblocks * nch), (unsigned)G), dim3(256), 0, st, n, nbc, nch, spike_first, (const double*)S.bcoord.p,
                       (const double*)d_cos, (const float*)S.bx.p, d_part);
    hipLaunchKernelGGL(k_b_psf_blocks_sum, dim3((unsigned)G, (unsigned)nblocks), dim3(64), 0, st, n, nbc, nch, nreal, spike_first, (const float*)S.bx.p,
                       (const double*)d_part, d_psf);
    LB_TRY(e, hipMemcpyAsync(psf, d_psf, 4 * (size_t)nreal * nblocks * 8, hipMemcpyDeviceToHost, st));
    return drain(e, st);
}

int dsa_lsmr_tradeoff(dsa_engine* h_, int nreal, int ndata, const float* b, float weight0, const float* weight, const float* damp, float atol, float btol,
                      float conlim, int itnlim, int localSize, float* x, double* measures, int* istop, int* itn, float* est)
{
    using namespace dsa;
    Entry in{"lsmr_tradeoff"};
    LB_DO(in.open(h_, nreal >= 1 && nreal <= kMaxReal && b && weight && damp && istop && itn && est, "nreal < 1 or a null b / weight / damp / istop / itn / est"));
    LB_DO(in.matrix(&ndata));
    LB_DO(in.no_tie_rows());
    LB_DO(in.weights(weight0, nreal, "member", weight, damp));
    return weighted_solve(in, nreal, 1, ndata, b, weight0, weight, damp, nullptr, atol, btol, conlim, itnlim, localSize, x, measures, nullptr, 0, istop, itn, est);
}

int dsa_lsmr_crossval(dsa_engine* h_, int ncombo, int nfolds, int ndata, const float* b, float weight0, const float* weight, const float* damp, const int* fold,
                      float atol, float btol, float conlim, int itnlim, int localSize, float* x, double* measures, double* resid, int* istop, int* itn, float* est)
{
    using namespace dsa;
    Entry in{"lsmr_crossval"};
    LB_DO(in.open(h_, ncombo >= 1 && nfolds >= 1 && b && weight && damp && fold && istop && itn && est,
                  "ncombo < 1, nfolds < 1 or a null b / weight / damp / fold / istop / itn / est"));
    Engine* e = in.e;
    const long long members = (long long)ncombo * ((long long)nfolds + 1);
    if (members > kMaxReal) { e->fail(DSA_ERR_ARGUMENT, "lsmr_crossval: %d combos x (%d folds + 1) are more than the %d members one call takes", ncombo, nfolds, kMaxReal); return DSA_ERR_ARGUMENT; }
    LB_DO(in.matrix(&ndata));
    LB_DO(in.no_tie_rows());
    size_t nres = 0;
    if (resid && (__builtin_mul_overflow((size_t)2 * (size_t)ncombo, (size_t)ndata, &nres) || nres > ((size_t)1 << 60) / 8)) {
        e->fail(DSA_ERR_ARGUMENT, "lsmr_crossval: resid of 2 x %d x %d values is more than one call takes", ncombo, ndata);
        return DSA_ERR_ARGUMENT;
    }
    LB_DO(in.weights(weight0, ncombo, "combo", weight, damp));
    for (int i = 0; i < ndata; ++i)
        if (fold[i] < 0 || fold[i] >= nfolds) { e->fail(DSA_ERR_ARGUMENT, "lsmr_crossval: datum %d is in fold %d, outside 0..%d", i, fold[i], nfolds - 1); return DSA_ERR_ARGUMENT; }
    return weighted_solve(in, (int)members, nfolds + 1, ndata, b, weight0, weight, damp, fold, atol, btol, conlim, itnlim, localSize, x, measures, resid, nres, istop, itn, est);
}

int dsa_lsmr_voronoi(dsa_engine* h_, int nreal, int ndata, int ncells, const float* b, const double* xyz, const int* seeds, float damp, float atol, float btol,
                     float conlim, int itnlim, int localSize, float* z, int* cell, double* stats, int* istop, int* itn, float* est)
{
    using namespace dsa;
    Entry in{"lsmr_voronoi"};
    LB_DO(in.open(h_, nreal >= 1 && nreal <= kMaxReal && b && xyz && seeds && istop && itn && est, "nreal < 1 or a null b / xyz / seeds / istop / itn / est"));
    LB_DO(in.matrix(&ndata));
    Engine* e = in.e;
    const int n = in.n;
    if (ncells < 1 || ncells > n) { e->fail(DSA_ERR_ARGUMENT, "lsmr_voronoi: ncells %d outside 1..%d", ncells, n); return DSA_ERR_ARGUMENT; }
    if (ncells > (1 << 24)) { e->fail(DSA_ERR_ARGUMENT, "lsmr_voronoi: ncells %d above %d (the sort keys are 64 ncells)", ncells, 1 << 24); return DSA_ERR_ARGUMENT; }
    if (!std::isfinite(damp)) { e->fail(DSA_ERR_ARGUMENT, "lsmr_voronoi: damp is not finite"); return DSA_ERR_ARGUMENT; }
    for (size_t i = 0; i < 3 * (size_t)n; ++i)
        if (!std::isfinite(xyz[i])) { e->fail(DSA_ERR_ARGUMENT, "lsmr_voronoi: coordinate %d of unknown %zu is not finite", (int)(i % 3), i / 3); return DSA_ERR_ARGUMENT; }
    for (size_t i = 0; i < (size_t)nreal * ncells; ++i)
        if (seeds[i] < 0 || seeds[i] >= n) { e->fail(DSA_ERR_ARGUMENT, "lsmr_voronoi: seed %zu of member %zu is %d, outside 0..%d", i % ncells, i / ncells, seeds[i], n - 1); return DSA_ERR_ARGUMENT; }
    if ((size_t)((ncells + 3) / 4) * (size_t)nreal > 0x7fffffffu) { e->fail(DSA_ERR_ARGUMENT, "lsmr_voronoi: %d members of %d cells are more than one call takes", nreal, ncells); return DSA_ERR_ARGUMENT; }
    // btmp: the solutions on their way out (member-major), then b
    Carve<float> T;
    const size_t o_z = T.take(z ? (size_t)nreal * ncells : 0), o_b = T.take((size_t)ndata);
    Batch B;
    LB_DO(batch_begin(e, nreal, localSize, T.total, B, ndata, ncells));
    SpmvState& S = *e->spmv;
    const int G = B.G, Rp = B.Rp;
    hipStream_t st = B.st;
    long long nnz = 0;                                                // entries of the data rows: the first ndata segments of the CSR copy
    LB_TRY(e, hipMemcpyAsync(&nnz, S.row_csr.ptr.p + ndata, 8, hipMemcpyDeviceToHost, st));
    LB_TRY(e, hipStreamSynchronize(st));
    if (nnz < 0 || nnz > (1ll << 31) / 64 - 1) { e->fail(DSA_ERR_ARGUMENT, "lsmr_voronoi: the data rows hold %lld entries, more than the %lld one lane group's sort takes", nnz, (1ll << 31) / 64 - 1); return DSA_ERR_ARGUMENT; }
    const size_t nz1 = std::max<size_t>((size_t)nnz, 1), vfull = (size_t)G * n * 64;
    if (e->ensure(S.vxyz, 3 * (size_t)n) || e->ensure(S.vseeds, (size_t)nreal * ncells) || e->ensure(S.vcell_mm, (size_t)Rp * n) || e->ensure(S.vcell, vfull) ||
        e->ensure(S.vfull, vfull) || e->ensure(S.vut, (size_t)Rp * ndata) || e->ensure(S.vrowof, nz1) || e->ensure(S.vlist, (size_t)Rp * nz1) ||
        e->ensure(S.vcptr, (size_t)Rp * (ncells + 1)) || e->ensure(S.vkeys, 64 * nz1) || e->ensure(S.vkeys_out, 64 * nz1) || e->ensure(S.vpos, 64 * nz1) ||
        (stats && e->ensure(S.vstats, 2 * (size_t)n))) return e->status;
    // the tessellations
    LB_TRY(e, hipMemcpyAsync(S.vxyz.p, xyz, 3 * (size_t)n * 8, hipMemcpyHostToDevice, st));
    LB_TRY(e, hipMemcpyAsync(S.vseeds.p, seeds, (size_t)nreal * ncells * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_v_assign, dim3((unsigned)((n + 255) / 256), (unsigned)std::min(nreal, 65535)), dim3(256), 0, st, n, ncells, nreal, (const double*)S.vxyz.p,
                       (const int*)S.vseeds.p, S.vcell_mm.p);
    hipLaunchKernelGGL(k_b_scatter<int>, grid_of(n, G), dim3(256), 0, st, n, nreal, (const int*)S.vcell_mm.p, S.vcell.p);      // [group][unknown][64]
    // every member's list: the data rows' CSR positions, stably sorted by cell, one lane group per sort
    LB_TRY(e, hipMemsetAsync(S.vcptr.p, 0, (size_t)Rp * (ncells + 1) * 4, st));
    if (nnz > 0) {
        hipLaunchKernelGGL(k_v_rowof, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, st, ndata, nnz, (const long long*)S.row_csr.ptr.p, S.vrowof.p);
        int bits = 1;
        while ((1ll << bits) < 64ll * ncells) ++bits;
        for (int g = 0; g < G; ++g) {
            const int members = std::min(64, nreal - 64 * g);
            const long long items = (long long)members * nnz;
            int* list = S.vlist.p + (size_t)g * 64 * (size_t)nnz;
            hipLaunchKernelGGL(k_v_keys, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, items, nnz, n, ncells, (const int*)(S.vcell_mm.p + (size_t)g * 64 * n),
                               (const int*)S.row_csr.idx.p, S.vkeys.p, S.vpos.p);
            size_t tmp_bytes = 0;
            LB_TRY(e, hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, (const int*)S.vkeys.p, S.vkeys_out.p, (const int*)S.vpos.p, list, (int)items, 0, bits, st));
            if (e->ensure(S.vsort, std::max<size_t>(tmp_bytes, 1))) return e->status;
            LB_TRY(e, hipcub::DeviceRadixSort::SortPairs(S.vsort.p, tmp_bytes, (const int*)S.vkeys.p, S.vkeys_out.p, (const int*)S.vpos.p, list, (int)items, 0, bits, st));
            const long long np = (long long)members * (ncells + 1);
            hipLaunchKernelGGL(k_v_cptr, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, members, ncells, nnz, (const int*)S.vkeys_out.p,
                               S.vcptr.p + (size_t)g * 64 * (ncells + 1));
        }
    }
    // u = b, row scales 1, then the loop on the projected products
    B.xout = T.at(S.btmp, o_z);
    float* d_b = T.at(S.btmp, o_b);
    LB_TRY(e, hipMemcpyAsync(d_b, b, (size_t)ndata * 4, hipMemcpyHostToDevice, st));
    B.fill(FILL_ONE, nreal, d_b);
    LB_TRY(e, hipGetLastError());
    B.projected = true; B.pnnz = nnz; B.preal = nreal;
    LB_DO(batch_solve(B, nreal, &damp, nreal, atol, btol, conlim, itnlim, z, istop, itn, est));
    if (cell) LB_TRY(e, hipMemcpyAsync(cell, S.vcell_mm.p, (size_t)nreal * n * 4, hipMemcpyDeviceToHost, st));
    if (stats) {
        // x_k[j] = z_k[cell_k(j)] on the unknowns (the expansion of mode 1, of the solutions), then its statistics over k in order
        hipLaunchKernelGGL(k_v_expand, grid_of(n, G), dim3(256), 0, st, n, ncells, (const int*)S.vcell.p, (const float*)S.bx.p, S.vfull.p);
        hipLaunchKernelGGL(k_v_stats, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, nreal, (const float*)S.vfull.p, S.vstats.p);
        LB_TRY(e, hipMemcpyAsync(stats, S.vstats.p, 2 * (size_t)n * 8, hipMemcpyDeviceToHost, st));
    }
    return drain(e, st);
}

}  // extern "C"
