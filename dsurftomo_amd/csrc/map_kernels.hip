// dsa_maps_resolution: the exact resolution matrix and covariance of every period map, from one dense L D L^T
// per map of the resident map system.  The arithmetic of every figure is map_resolution.h's; this file shares the figures out:
//
//   k_map_owner, k_map_columns   one thread per row / column: the owner of every row, the used data, the order of every column's rows
//   k_map_normal                 one thread per entry (i, p) of a map's lower triangle: the ordered sum over column p's rows
//   k_map_panel                  per panel of kMapPanel columns, one workgroup per map: the panel's columns one after the other, v in LDS
//   k_map_trail                  per panel, one workgroup per 64 x 64 tile of every map's trailing matrix: entry (i, j) loses the panel's
//                                64 products L_ip (L_jp d_p), p ascending -- the chain map_factor runs, interrupted between panels
//   k_map_solve                  one lane per used datum: map_solve_datum on T, datum-fastest
//   k_map_rcols                  one thread per entry of R
//   k_map_measures, k_map_leverage, k_map_trace   one thread per unknown / datum / plane
//
// L is stored p slow, i fast: lanes on consecutive rows i read consecutive doubles, L_jp and v_p are broadcasts.  Every output element is
// written by one thread with a vector store; there are no atomics; LDS holds operands only.  No kernel waits for another workgroup.
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/dsurftomo_amd.h"
#include "engine.h"
#include "map_resolution.h"
#include "spmv_state.h"

namespace dsa {

namespace {

constexpr int kPanelThreads = 1024;
constexpr int kTrailTile = 64;              // = kMapPanel: a tile's 64 rows are the lanes of a wavefront
constexpr int kGroupWords = 4;         // per map of a group: map, K, first place in dlist, first double of its T

struct Csr { const long long* ptr; const float* val; const int* idx; };

__global__ __launch_bounds__(256) void k_map_owner(MapShape S, int m, int ndata, Csr row, int* owner, int* used)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= m) return;
    int u;
    owner[r] = map_row_owner(S, ndata, r, row.ptr, row.val, row.idx, &u);
    used[r] = u;
}

__global__ __launch_bounds__(256) void k_map_columns(int n, Csr col, int* bad)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    bad[c] = map_column_check(c, col.ptr, col.idx);
}

__global__ __launch_bounds__(256) void k_map_normal(MapShape S, double damp2, Csr row, Csr col, const long long* G, double* Lbuf)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, p = blockIdx.y, g = blockIdx.z;
    if (i >= S.nm || i < p) return;
    const int map = (int)G[g * kGroupWords];
    Lbuf[(size_t)g * S.nm * S.nm + (size_t)p * S.nm + i] = map_normal_entry(S, map, i, p, damp2, row.ptr, row.val, row.idx, col.ptr, col.val, col.idx);
}

// columns c0 .. c1-1 of every map of the group, whose entries already lost the products of the panels before: column j first forms
// v_p = L_jp d_p for the panel's p < j, every thread then the pivot (the same chain in every thread: all leave together where it fails) and its
// rows of column j
__global__ __launch_bounds__(kPanelThreads) void k_map_panel(int nm, int c0, const long long* G, double* Lbuf, double* dbuf, int* flag)
{
    const int g = blockIdx.x, map = (int)G[g * kGroupWords], tid = threadIdx.x;
    if (flag[map] != kMapOk) return;
    double* L = Lbuf + (size_t)g * nm * nm;
    double* d = dbuf + (size_t)g * nm;
    __shared__ double v[kMapPanel];
    const int c1 = c0 + kMapPanel < nm ? c0 + kMapPanel : nm;
    for (int j = c0; j < c1; ++j) {
        if (tid < j - c0) v[tid] = L[(size_t)(c0 + tid) * nm + j] * d[c0 + tid];
        __syncthreads();
        double dj = L[(size_t)j * nm + j];
        for (int p = c0; p < j; ++p) dj -= L[(size_t)p * nm + j] * v[p - c0];
        if (!(isfinite(dj) && dj > 0.0)) {
            if (tid == 0) flag[map] = kMapNotPositive;
            return;
        }
        if (tid == 0) d[j] = dj;
        for (int i = j + 1 + tid; i < nm; i += kPanelThreads) {
            double s = L[(size_t)j * nm + i];
            for (int p = c0; p < j; ++p) s -= L[(size_t)p * nm + i] * v[p - c0];
            L[(size_t)j * nm + i] = s / dj;
        }
        __syncthreads();
    }
}

// the trailing matrix behind the full panel c0 .. c0+63: tile (bi, bj) of map g, rows i0 + lane, 16 columns per wavefront.  LDS: the
// tile's V_jp = L_jp d_p, p slow; a wavefront reads its 16 of one p as broadcasts.
__global__ __launch_bounds__(256) void k_map_trail(int nm, int c0, const long long* G, double* Lbuf, const double* dbuf, const int* flag)
{
    const int bi = blockIdx.x, bj = blockIdx.y, g = blockIdx.z;
    if (bi < bj || flag[(int)G[g * kGroupWords]] != kMapOk) return;
    double* L = Lbuf + (size_t)g * nm * nm;
    const double* d = dbuf + (size_t)g * nm;
    const int c1 = c0 + kMapPanel, i0 = c1 + bi * kTrailTile, j0 = c1 + bj * kTrailTile, tid = threadIdx.x;
    __shared__ double V[kMapPanel * kTrailTile];
    for (int e = tid; e < kMapPanel * kTrailTile; e += 256) {
        const int jj = e & (kTrailTile - 1), p = e / kTrailTile, j = j0 + jj;
        V[e] = j < nm ? L[(size_t)(c0 + p) * nm + j] * d[c0 + p] : 0.0;
    }
    __syncthreads();
    const int lane = tid & 63, w = tid >> 6, i = i0 + lane, ir = i < nm ? i : nm - 1;
    double acc[16];
    #pragma unroll
    for (int t = 0; t < 16; ++t) {
        const int j = j0 + 16 * w + t;
        acc[t] = (j < nm && i < nm && i >= j) ? L[(size_t)j * nm + i] : 0.0;
    }
    for (int p = 0; p < kMapPanel; ++p) {
        const double lip = L[(size_t)(c0 + p) * nm + ir];
        #pragma unroll
        for (int t = 0; t < 16; ++t) acc[t] -= lip * V[p * kTrailTile + 16 * w + t];
    }
    #pragma unroll
    for (int t = 0; t < 16; ++t) {
        const int j = j0 + 16 * w + t;
        if (j < nm && i < nm && i >= j) L[(size_t)j * nm + i] = acc[t];
    }
}

__global__ __launch_bounds__(64) void k_map_solve(MapShape S, Csr row, const long long* G, const int* dlist, const double* Lbuf, const double* dbuf, double* Tbuf,
                                                  const int* flag)
{
    const int g = blockIdx.y, k = blockIdx.x * 64 + threadIdx.x;
    const long long* e = G + g * kGroupWords;
    const int K = (int)e[1];
    if (k >= K || flag[(int)e[0]] != kMapOk) return;
    map_solve_datum(S, dlist[e[2] + k], row.ptr, row.val, row.idx, Lbuf + (size_t)g * S.nm * S.nm, dbuf + (size_t)g * S.nm, Tbuf + e[3], K, k);
}

__global__ __launch_bounds__(256) void k_map_rcols(MapShape S, int ndata, Csr col, const long long* G, const int* kidx, const double* Tbuf, double* Rbuf,
                                                   const int* flag)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x, l = blockIdx.y, g = blockIdx.z;
    const long long* e = G + g * kGroupWords;
    if (q >= S.nm || flag[(int)e[0]] != kMapOk) return;
    Rbuf[(size_t)g * S.nm * S.nm + (size_t)l * S.nm + q] = map_r_entry(S, (int)e[0], l, q, ndata, col.ptr, col.val, col.idx, kidx, Tbuf + e[3], e[1]);
}

__global__ __launch_bounds__(64) void k_map_measures(MapShape S, const long long* G, const double* Tbuf, const double* Rbuf, double* measures, const int* flag)
{
    const int q = blockIdx.x * 64 + threadIdx.x, g = blockIdx.y;
    const long long* e = G + g * kGroupWords;
    const int map = (int)e[0], K = (int)e[1];
    if (q >= S.nm || flag[map] != kMapOk) return;
    double out[kMapMeasures];
    map_moments(S, q, Rbuf + (size_t)g * S.nm * S.nm, out);
    out[1] = map_covariance(q, q, K, Tbuf + e[3], K);
    out[8] = S.nblocks == 1 ? 0.0 : map_covariance(q, map_next_plane(S, q), K, Tbuf + e[3], K);
    const int c = map_column(S, map, q);
    #pragma unroll
    for (int k = 0; k < kMapMeasures; ++k) measures[(size_t)k * S.n + c] = out[k];
}

__global__ __launch_bounds__(64) void k_map_leverage(MapShape S, Csr row, const long long* G, const int* dlist, const double* Tbuf, double* leverage, const int* flag)
{
    const int g = blockIdx.y, k = blockIdx.x * 64 + threadIdx.x;
    const long long* e = G + g * kGroupWords;
    const int K = (int)e[1];
    if (k >= K || flag[(int)e[0]] != kMapOk) return;
    const int r = dlist[e[2] + k];
    leverage[r] = map_leverage(S, r, row.ptr, row.val, row.idx, Tbuf + e[3], K, k);
}

__global__ __launch_bounds__(64) void k_map_trace(MapShape S, const double* measures, double* trace)
{
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= S.nblocks * S.nmaps) return;
    trace[t] = map_trace(S, t % S.nmaps, t / S.nmaps, measures);
}

#define MR_TRY(e, call)                                                                        \
    do {                                                                                       \
        hipError_t _r = (call);                                                                \
        if (_r != hipSuccess) { (e)->fail(DSA_ERR_DEVICE, "maps_resolution: %s failed: %s", #call, hipGetErrorString(_r)); return DSA_ERR_DEVICE; } \
    } while (0)

int refuse(Engine* e, int code, const char* fmt, long long a = 0, long long b = 0, long long c = 0)
{
    char text[256];
    snprintf(text, sizeof text, fmt, a, b, c);
    e->fail(code, "maps_resolution: %s", text);
    return code;
}

}  // namespace

}  // namespace dsa

extern "C" int dsa_maps_resolution(dsa_engine* h_, int nx, int ny, int nmaps, int nblocks, int ndata, float damp, int r_map, double* measures, double* leverage,
                                   double* trace, int* nused, int* flag, double* R)
{
    using namespace dsa;
    if (!h_) return DSA_ERR_ARGUMENT;
    Engine* e = reinterpret_cast<Engine*>(h_);
    // ---- everything that can be checked without the device ----
    if (!measures) return refuse(e, DSA_ERR_ARGUMENT, "measures is required");
    if (nx < 3 || ny < 3 || nmaps < 1 || (nblocks != 1 && nblocks != 3)) return refuse(e, DSA_ERR_ARGUMENT, "nx and ny must be >= 3, nmaps >= 1, nblocks 1 or 3 (nx %lld, ny %lld)", nx, ny);
    if (!std::isfinite(damp) || damp < 0.0f) return refuse(e, DSA_ERR_ARGUMENT, "damp must be finite and >= 0");
    if (r_map < -1 || r_map >= nmaps) return refuse(e, DSA_ERR_ARGUMENT, "r_map %lld outside -1..%lld", r_map, nmaps - 1);
    if ((R != nullptr) != (r_map >= 0)) return refuse(e, DSA_ERR_ARGUMENT, "R and r_map disagree: R needs r_map >= 0, r_map = -1 a NULL R");
    if (!e->spmv) return refuse(e, DSA_ERR_STATE, "no matrix (call dsa_iteration_system_maps_device or dsa_spmv_load first)");
    SpmvState& M = *e->spmv;
    if (M.radial) return refuse(e, DSA_ERR_STATE, "the resident matrix is the radial system, not a map system");
    const long long nwant = (long long)nblocks * nmaps * (nx - 2) * (ny - 2);
    if (nwant != M.n) return refuse(e, DSA_ERR_ARGUMENT, "the matrix has %lld unknowns, nblocks nmaps (nx-2)(ny-2) is %lld", M.n, nwant);
    if (ndata < 1 || ndata > M.m) return refuse(e, DSA_ERR_ARGUMENT, "ndata %lld outside 1..%lld", ndata, M.m);
    const MapShape S = map_shape(nx, ny, nmaps, nblocks);
    const int m = M.m, n = M.n, nm = S.nm;
    const size_t nm2 = (size_t)nm * nm;
    if (nm > 65535) return refuse(e, DSA_ERR_CAPACITY, "a map of %lld unknowns is beyond the 65535 of a launch", nm);
    if (e->mem_budget && 8 * (2 * nm2 + 2 * (size_t)nm) > e->mem_budget)
        return refuse(e, DSA_ERR_CAPACITY, "one map of %lld unknowns needs more than %lld bytes for its factor and its R, the memory budget is %lld", nm, (long long)(16 * nm2), (long long)e->mem_budget);
    // ---- owners, used data, column order ----
    MR_TRY(e, hipSetDevice(e->device));
    if (int rc = spmv_ensure_contiguous(e)) return rc;
    hipStream_t st = e->stream;
    const Csr row{M.row_csr.ptr.p, M.row_csr.val.p, M.row_csr.idx.p}, col{M.col_csr.ptr.p, M.col_csr.val.p, M.col_csr.idx.p};
    OwnedBuf<int> d_int;                                              // owner (m), used (m), column verdicts (n); later kidx (m), dlist (m), flag (nmaps)
    if (e->ensure(d_int, 2 * (size_t)m + (size_t)std::max(n, nmaps))) return e->status;
    int *d_owner = d_int.p, *d_used = d_int.p + m, *d_bad = d_int.p + 2 * (size_t)m;
    hipLaunchKernelGGL(k_map_owner, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, S, m, ndata, row, d_owner, d_used);
    hipLaunchKernelGGL(k_map_columns, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, col, d_bad);
    std::vector<int> owner((size_t)m), used((size_t)m), bad((size_t)n);
    MR_TRY(e, hipGetLastError());
    MR_TRY(e, hipMemcpyAsync(owner.data(), d_owner, (size_t)m * 4, hipMemcpyDeviceToHost, st));
    MR_TRY(e, hipMemcpyAsync(used.data(), d_used, (size_t)m * 4, hipMemcpyDeviceToHost, st));
    MR_TRY(e, hipMemcpyAsync(bad.data(), d_bad, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    MR_TRY(e, hipStreamSynchronize(st));
    for (int r = 0; r < m; ++r)
        if (owner[r] == kMapRowTwoMaps) return refuse(e, DSA_ERR_ARGUMENT, "row %lld has entries in the unknowns of two maps", r);
    for (int c = 0; c < n; ++c) {
        if (bad[c] == kMapColumnTwice) return refuse(e, DSA_ERR_ARGUMENT, "a row stores column %lld twice", c);
        if (bad[c] == kMapColumnOrder) return refuse(e, DSA_ERR_ARGUMENT, "the rows of column %lld do not ascend: the matrix was not loaded in row order", c);
    }
    // the used data of every map, ascending; the place of every row in its map's list
    std::vector<int> K((size_t)nmaps, 0), kidx((size_t)m, -1), dlist, flags((size_t)nmaps);
    std::vector<long long> koff((size_t)nmaps + 1, 0);
    for (int r = 0; r < ndata; ++r)
        if (used[r]) kidx[r] = K[owner[r]]++;
    for (int k = 0; k < nmaps; ++k) koff[(size_t)k + 1] = koff[k] + K[k];
    dlist.resize((size_t)std::max<long long>(koff[nmaps], 1));
    for (int r = 0; r < ndata; ++r)
        if (used[r]) dlist[(size_t)(koff[owner[r]] + kidx[r])] = r;
    for (int k = 0; k < nmaps; ++k) flags[k] = K[k] > 0 ? kMapOk : kMapNoData;
    // ---- the groups of maps that fit the budget ----
    size_t budget = e->mem_budget;
    if (!budget) {
        size_t free_b = 0, total_b = 0;
        MR_TRY(e, hipMemGetInfo(&free_b, &total_b));
        budget = std::min<size_t>((size_t)(0.5 * (double)free_b), (size_t)16 << 30);
    }
    auto bytes_of = [&](int k) { return 8 * (2 * nm2 + (size_t)K[k] * nm + (size_t)nm); };
    std::vector<std::vector<int>> groups;
    {
        size_t in_group = 0;
        for (int k = 0; k < nmaps; ++k) {
            if (flags[k] != kMapOk) continue;
            const size_t b = bytes_of(k);
            if (b > budget) return refuse(e, DSA_ERR_CAPACITY, "map %lld needs %lld bytes (factor, R and T), the memory budget is %lld", k, (long long)b, (long long)budget);
            if (groups.empty() || in_group + b > budget) { groups.emplace_back(); in_group = 0; }
            groups.back().push_back(k);
            in_group += b;
        }
    }
    size_t gmax = 1, tmax = 1;
    for (const auto& grp : groups) {
        size_t t = 0;
        for (int k : grp) t += (size_t)K[k] * nm;
        gmax = std::max(gmax, grp.size()); tmax = std::max(tmax, t);
    }
    // ---- buffers ----
    OwnedBuf<double> d_L, d_R, d_T, d_d, d_out;
    OwnedBuf<long long> d_G;
    const size_t n_out = (size_t)kMapMeasures * n + (size_t)ndata + (size_t)nblocks * nmaps;
    if (e->ensure(d_L, gmax * nm2) || e->ensure(d_R, gmax * nm2) || e->ensure(d_T, tmax) || e->ensure(d_d, gmax * nm) || e->ensure(d_out, n_out) ||
        e->ensure(d_G, gmax * kGroupWords)) return e->status;
    double *d_meas = d_out.p, *d_lev = d_out.p + (size_t)kMapMeasures * n, *d_trace = d_lev + ndata;
    int *d_kidx = d_int.p, *d_dlist = d_int.p + m, *d_flag = d_int.p + 2 * (size_t)m;     // (owner, used and the verdicts are on the host)
    MR_TRY(e, hipMemsetAsync(d_out.p, 0, n_out * 8, st));
    MR_TRY(e, hipMemcpyAsync(d_kidx, kidx.data(), (size_t)m * 4, hipMemcpyHostToDevice, st));
    MR_TRY(e, hipMemcpyAsync(d_dlist, dlist.data(), (size_t)koff[nmaps] * 4, hipMemcpyHostToDevice, st));
    MR_TRY(e, hipMemcpyAsync(d_flag, flags.data(), (size_t)nmaps * 4, hipMemcpyHostToDevice, st));
    const double damp2 = (double)damp * (double)damp;
    bool have_R = false;
    std::vector<long long> G;
    for (const auto& grp : groups) {
        const int ng = (int)grp.size();
        G.assign((size_t)ng * kGroupWords, 0);
        long long toff = 0;
        int Kmax = 1, gR = -1;
        for (int g = 0; g < ng; ++g) {
            const int k = grp[g];
            G[(size_t)g * kGroupWords] = k; G[(size_t)g * kGroupWords + 1] = K[k]; G[(size_t)g * kGroupWords + 2] = koff[k]; G[(size_t)g * kGroupWords + 3] = toff;
            toff += (long long)K[k] * nm;
            Kmax = std::max(Kmax, K[k]);
            if (k == r_map) gR = g;
        }
        MR_TRY(e, hipMemcpyAsync(d_G.p, G.data(), G.size() * 8, hipMemcpyHostToDevice, st));
        const dim3 per_entry((unsigned)((nm + 255) / 256), (unsigned)nm, (unsigned)ng);
        hipLaunchKernelGGL(k_map_normal, per_entry, dim3(256), 0, st, S, damp2, row, col, (const long long*)d_G.p, d_L.p);
        for (int c0 = 0; c0 < nm; c0 += kMapPanel) {
            hipLaunchKernelGGL(k_map_panel, dim3((unsigned)ng), dim3(kPanelThreads), 0, st, nm, c0, (const long long*)d_G.p, d_L.p, d_d.p, d_flag);
            const int left = nm - (c0 + kMapPanel);
            if (left > 0) {
                const unsigned nb = (unsigned)((left + kTrailTile - 1) / kTrailTile);
                hipLaunchKernelGGL(k_map_trail, dim3(nb, nb, (unsigned)ng), dim3(256), 0, st, nm, c0, (const long long*)d_G.p, d_L.p, (const double*)d_d.p, (const int*)d_flag);
            }
        }
        const dim3 per_datum((unsigned)((Kmax + 63) / 64), (unsigned)ng);
        hipLaunchKernelGGL(k_map_solve, per_datum, dim3(64), 0, st, S, row, (const long long*)d_G.p, (const int*)d_dlist, (const double*)d_L.p, (const double*)d_d.p, d_T.p,
                           (const int*)d_flag);
        hipLaunchKernelGGL(k_map_rcols, per_entry, dim3(256), 0, st, S, ndata, col, (const long long*)d_G.p, (const int*)d_kidx, (const double*)d_T.p, d_R.p, (const int*)d_flag);
        hipLaunchKernelGGL(k_map_measures, dim3((unsigned)((nm + 63) / 64), (unsigned)ng), dim3(64), 0, st, S, (const long long*)d_G.p, (const double*)d_T.p,
                           (const double*)d_R.p, d_meas, (const int*)d_flag);
        hipLaunchKernelGGL(k_map_leverage, per_datum, dim3(64), 0, st, S, row, (const long long*)d_G.p, (const int*)d_dlist, (const double*)d_T.p, d_lev, (const int*)d_flag);
        MR_TRY(e, hipGetLastError());
        MR_TRY(e, hipMemcpyAsync(flags.data(), d_flag, (size_t)nmaps * 4, hipMemcpyDeviceToHost, st));
        MR_TRY(e, hipStreamSynchronize(st));                          // (G and the group's buffers are free again)
        if (gR >= 0 && flags[r_map] == kMapOk) {
            MR_TRY(e, hipMemcpyAsync(R, d_R.p + (size_t)gR * nm2, nm2 * 8, hipMemcpyDeviceToHost, st));
            MR_TRY(e, hipStreamSynchronize(st));
            have_R = true;
        }
    }
    hipLaunchKernelGGL(k_map_trace, dim3((unsigned)((nblocks * nmaps + 63) / 64)), dim3(64), 0, st, S, (const double*)d_meas, d_trace);
    MR_TRY(e, hipGetLastError());
    MR_TRY(e, hipMemcpyAsync(measures, d_meas, (size_t)kMapMeasures * n * 8, hipMemcpyDeviceToHost, st));
    if (leverage) MR_TRY(e, hipMemcpyAsync(leverage, d_lev, (size_t)ndata * 8, hipMemcpyDeviceToHost, st));
    if (trace) MR_TRY(e, hipMemcpyAsync(trace, d_trace, (size_t)nblocks * nmaps * 8, hipMemcpyDeviceToHost, st));
    MR_TRY(e, hipStreamSynchronize(st));
    if (R && !have_R) std::fill(R, R + nm2, 0.0);
    if (nused) std::copy(K.begin(), K.end(), nused);
    if (flag) std::copy(flags.begin(), flags.end(), flag);
    return 0;
}
