// TEST HARNESS (not product): the map resolution of dsurftomo_amd/csrc/map_resolution.h on a CPU behind a C interface, for
// tests/test_hostcheck_map_resolution.py and tests/test_gpu_maps_resolution.py -- every figure by the header's own function, one after the
// other: the arithmetic csrc/map_kernels.hip shares out over the device.  The factor is the header's left-looking map_factor;
// hmr_factor_panelled is this file's own right-looking loop in panels of kMapPanel columns, the order of operations of the device's
// k_map_panel / k_map_trail, which must give the same bits.  With -DHOSTCHECK_MAP_RESOLUTION_MAIN the file is a stand-alone program (for a
// sanitizer build).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../dsurftomo_amd/csrc/map_resolution.h"

using namespace dsa;

namespace {

// a COO matrix (1-based) as the CSR and CSC the engine keeps: every segment's entries in storage order
struct System {
    int m = 0, n = 0;
    std::vector<long long> rptr, cptr;
    std::vector<float> rval, cval;
    std::vector<int> ridx, cidx;
    System(int m_, int n_, long long nar, const float* rw, const int* row, const int* col) : m(m_), n(n_), rptr((size_t)m_ + 1, 0), cptr((size_t)n_ + 1, 0),
        rval((size_t)nar), cval((size_t)nar), ridx((size_t)nar), cidx((size_t)nar)
    {
        for (long long e = 0; e < nar; ++e) { ++rptr[(size_t)row[e]]; ++cptr[(size_t)col[e]]; }
        for (int r = 0; r < m; ++r) rptr[(size_t)r + 1] += rptr[r];
        for (int c = 0; c < n; ++c) cptr[(size_t)c + 1] += cptr[c];
        std::vector<long long> rc(rptr.begin(), rptr.end() - 1), cc(cptr.begin(), cptr.end() - 1);
        for (long long e = 0; e < nar; ++e) {
            const long long a = rc[(size_t)row[e] - 1]++, b = cc[(size_t)col[e] - 1]++;
            rval[(size_t)a] = rw[e]; ridx[(size_t)a] = col[e] - 1;
            cval[(size_t)b] = rw[e]; cidx[(size_t)b] = row[e] - 1;
        }
    }
};

// owners and used data; 0, or 1 a row in two maps, 2 a column stored twice in a row, 3 a column whose rows do not ascend
int structure(const MapShape& S, const System& A, int ndata, std::vector<int>& owner, std::vector<int>& used)
{
    owner.assign((size_t)A.m, kMapRowNone); used.assign((size_t)A.m, 0);
    for (int r = 0; r < A.m; ++r) {
        owner[r] = map_row_owner(S, ndata, r, A.rptr.data(), A.rval.data(), A.ridx.data(), &used[r]);
        if (owner[r] == kMapRowTwoMaps) return 1;
    }
    for (int c = 0; c < A.n; ++c) {
        const int bad = map_column_check(c, A.cptr.data(), A.cidx.data());
        if (bad == kMapColumnTwice) return 2;
        if (bad == kMapColumnOrder) return 3;
    }
    return 0;
}

void normal(const MapShape& S, const System& A, int map, double damp2, std::vector<double>& L)
{
    const int nm = S.nm;
    L.assign((size_t)nm * nm, 0.0);
    for (int p = 0; p < nm; ++p)
        for (int i = p; i < nm; ++i)
            L[(size_t)p * nm + i] = map_normal_entry(S, map, i, p, damp2, A.rptr.data(), A.rval.data(), A.ridx.data(), A.cptr.data(), A.cval.data(), A.cidx.data());
}

// THE TEST'S OWN LOOP: right-looking in panels.  Per panel the panel's columns are finished one after the other from the partial sums the
// earlier panels left, then every entry behind the panel loses the panel's products, p ascending.
int factor_panelled(int nm, double* L, double* d)
{
    std::vector<double> v(kMapPanel);
    for (int c0 = 0; c0 < nm; c0 += kMapPanel) {
        const int c1 = c0 + kMapPanel < nm ? c0 + kMapPanel : nm;
        for (int j = c0; j < c1; ++j) {
            for (int p = c0; p < j; ++p) v[p - c0] = L[(size_t)p * nm + j] * d[p];
            double dj = L[(size_t)j * nm + j];
            for (int p = c0; p < j; ++p) dj -= L[(size_t)p * nm + j] * v[p - c0];
            if (!(std::isfinite(dj) && dj > 0.0)) return kMapNotPositive;
            d[j] = dj;
            for (int i = j + 1; i < nm; ++i) {
                double s = L[(size_t)j * nm + i];
                for (int p = c0; p < j; ++p) s -= L[(size_t)p * nm + i] * v[p - c0];
                L[(size_t)j * nm + i] = s / dj;
            }
        }
        for (int j = c1; j < nm; ++j)
            for (int i = j; i < nm; ++i) {
                double s = L[(size_t)j * nm + i];
                for (int p = c0; p < c1; ++p) s -= L[(size_t)p * nm + i] * (L[(size_t)p * nm + j] * d[p]);
                L[(size_t)j * nm + i] = s;
            }
    }
    return kMapOk;
}

}  // namespace

extern "C" {

// dsa_maps_resolution on the CPU: the matrix as 1-based COO (m x n, nar entries, in row order), the outputs and their layouts the
// library's; any output but measures may be null.  Returns 0, or 1 / 2 / 3 for the three refusals of the structure (nothing is written).
int hmr_resolution(int nx, int ny, int nmaps, int nblocks, int m, int ndata, long long nar, const float* rw, const int* row, const int* col, float damp, int r_map,
                   double* measures, double* leverage, double* trace, int* nused, int* flag, double* R)
{
    const MapShape S = map_shape(nx, ny, nmaps, nblocks);
    const int nm = S.nm;
    const System A(m, S.n, nar, rw, row, col);
    std::vector<int> owner, used;
    if (const int bad = structure(S, A, ndata, owner, used)) return bad;
    const double damp2 = (double)damp * (double)damp;
    for (size_t e = 0; e < (size_t)kMapMeasures * S.n; ++e) measures[e] = 0.0;
    if (leverage) for (int r = 0; r < ndata; ++r) leverage[r] = 0.0;
    if (R) for (size_t e = 0; e < (size_t)nm * nm; ++e) R[e] = 0.0;
    std::vector<int> kidx((size_t)m, -1);
    std::vector<double> L, d((size_t)nm), v((size_t)nm), T, Rm((size_t)nm * nm);
    for (int map = 0; map < nmaps; ++map) {
        std::vector<int> dlist;
        for (int r = 0; r < ndata; ++r)
            if (used[r] && owner[r] == map) { kidx[r] = (int)dlist.size(); dlist.push_back(r); }
        const int K = (int)dlist.size();
        int f = K > 0 ? kMapOk : kMapNoData;
        if (f == kMapOk) {
            normal(S, A, map, damp2, L);
            f = map_factor(nm, L.data(), d.data(), v.data());
        }
        if (nused) nused[map] = K;
        if (flag) flag[map] = f;
        if (f != kMapOk) continue;
        T.assign((size_t)K * nm, 0.0);
        for (int k = 0; k < K; ++k) map_solve_datum(S, dlist[k], A.rptr.data(), A.rval.data(), A.ridx.data(), L.data(), d.data(), T.data(), K, k);
        for (int l = 0; l < nm; ++l)
            for (int q = 0; q < nm; ++q) Rm[(size_t)l * nm + q] = map_r_entry(S, map, l, q, ndata, A.cptr.data(), A.cval.data(), A.cidx.data(), kidx.data(), T.data(), K);
        for (int q = 0; q < nm; ++q) {
            double out[kMapMeasures];
            map_moments(S, q, Rm.data(), out);
            out[1] = map_covariance(q, q, K, T.data(), K);
            out[8] = nblocks == 1 ? 0.0 : map_covariance(q, map_next_plane(S, q), K, T.data(), K);
            for (int k = 0; k < kMapMeasures; ++k) measures[(size_t)k * S.n + map_column(S, map, q)] = out[k];
        }
        if (leverage)
            for (int k = 0; k < K; ++k) leverage[dlist[k]] = map_leverage(S, dlist[k], A.rptr.data(), A.rval.data(), A.ridx.data(), T.data(), K, k);
        if (R && map == r_map) std::memcpy(R, Rm.data(), (size_t)nm * nm * 8);
    }
    if (trace)
        for (int t = 0; t < nblocks * nmaps; ++t) trace[t] = map_trace(S, t % nmaps, t / nmaps, measures);
    return 0;
}

// the factor of one map twice: the header's left-looking map_factor (L1, d1) and this file's panelled right-looking loop (L2, d2), each
// n_m * n_m (entry (i, p) at p n_m + i; the upper triangle 0, the diagonal 1) and n_m doubles.  flags[2].  Returns the structure's verdict.
int hmr_factors(int nx, int ny, int nmaps, int nblocks, int m, int ndata, long long nar, const float* rw, const int* row, const int* col, float damp, int map,
                double* L1, double* d1, double* L2, double* d2, int* flags)
{
    const MapShape S = map_shape(nx, ny, nmaps, nblocks);
    const int nm = S.nm;
    const System A(m, S.n, nar, rw, row, col);
    std::vector<int> owner, used;
    if (const int bad = structure(S, A, ndata, owner, used)) return bad;
    std::vector<double> N, v((size_t)nm);
    normal(S, A, map, (double)damp * (double)damp, N);
    std::memcpy(L1, N.data(), N.size() * 8); std::memcpy(L2, N.data(), N.size() * 8);
    for (int i = 0; i < nm; ++i) d1[i] = d2[i] = 0.0;
    flags[0] = map_factor(nm, L1, d1, v.data());
    flags[1] = factor_panelled(nm, L2, d2);
    for (int i = 0; i < nm; ++i) L1[(size_t)i * nm + i] = L2[(size_t)i * nm + i] = 1.0;       // (the diagonal is work space in both: L's is 1)
    return 0;
}

}  // extern "C"

#ifdef HOSTCHECK_MAP_RESOLUTION_MAIN
namespace {
unsigned long long g_state = 88172645463325252ull;
double uniform()          // xorshift64, in [0, 1)
{
    g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
    return (double)(g_state >> 11) / 9007199254740992.0;
}
}

int main()
{
    int bad = 0;
    const int cases[][4] = { { 3, 3, 1, 1 }, { 7, 6, 2, 1 }, { 7, 6, 3, 3 }, { 11, 9, 2, 3 }, { 10, 10, 2, 1 } };     // nx, ny, nmaps, nblocks
    for (const auto& c : cases) {
        const int nx = c[0], ny = c[1], nmaps = c[2], nblocks = c[3];
        const MapShape S = map_shape(nx, ny, nmaps, nblocks);
        const int ndata = 40 + 3 * S.layer, m = ndata + S.n, per = S.layer < 7 ? S.layer : 7;
        std::vector<float> rw; std::vector<int> row, col;
        for (int dd = 0; dd < ndata; ++dd) {
            const int map = (nmaps > 2 && dd % nmaps == nmaps - 1) ? 0 : dd % nmaps;      // with three maps the last one has no data
            const int i0 = (int)(uniform() * (S.layer - per + 1));
            const float w = dd % 17 == 5 ? 0.0f : 1.0f;                                    // some data without weight
            for (int B = 0; B < nblocks; ++B)
                for (int t = 0; t < per; ++t) { rw.push_back(w * (float)(0.5 + uniform())); row.push_back(dd + 1); col.push_back((B * nmaps + map) * S.layer + i0 + t + 1); }
        }
        for (int u = 0; u < S.n; ++u) { rw.push_back(2.0f); row.push_back(ndata + u + 1); col.push_back(u + 1); }
        std::vector<double> measures((size_t)kMapMeasures * S.n, 9.0), leverage((size_t)ndata, 9.0), trace((size_t)nblocks * nmaps, 9.0), R((size_t)S.nm * S.nm, 9.0);
        std::vector<int> nused(nmaps), flag(nmaps);
        const int rc = hmr_resolution(nx, ny, nmaps, nblocks, m, ndata, (long long)rw.size(), rw.data(), row.data(), col.data(), 0.01f, 0, measures.data(), leverage.data(),
                                      trace.data(), nused.data(), flag.data(), R.data());
        double tsum = 0.0, hsum = 0.0;
        for (double t : trace) tsum += t;
        for (double h : leverage) { hsum += h; if (!(h >= 0.0 && h < 1.0)) ++bad; }
        if (rc != 0 || !(std::fabs(tsum - hsum) <= 1e-10 * (1.0 + tsum))) ++bad;
        for (int u = 0; u < S.n; ++u)
            if (!(measures[u] >= 0.0 && measures[u] <= 1.0) || !(measures[(size_t)S.n + u] >= 0.0)) ++bad;
        if (nmaps > 2 && (flag[nmaps - 1] != kMapNoData || nused[nmaps - 1] != 0)) ++bad;
        if (flag[0] != kMapOk) ++bad;
        std::vector<double> L1((size_t)S.nm * S.nm), L2(L1.size()), d1(S.nm), d2(S.nm);
        int flags[2];
        if (hmr_factors(nx, ny, nmaps, nblocks, m, ndata, (long long)rw.size(), rw.data(), row.data(), col.data(), 0.01f, 0, L1.data(), d1.data(), L2.data(), d2.data(), flags)) ++bad;
        if (flags[0] != kMapOk || flags[1] != kMapOk || std::memcmp(L1.data(), L2.data(), L1.size() * 8) || std::memcmp(d1.data(), d2.data(), d1.size() * 8)) ++bad;
        std::printf("%2d x %2d, %d maps of %d blocks (n_m %3d): rc %d nused %d flag %d trace %.17g sum of leverages %.17g\n", nx, ny, nmaps, nblocks, S.nm, rc, nused[0], flag[0], tsum, hsum);
        // the refusals: a row across two maps, a column twice in a row
        if (nmaps > 1) {
            std::vector<float> rw2(rw); std::vector<int> row2(row), col2(col);
            col2[0] = col2[0] + S.layer;
            if (hmr_resolution(nx, ny, nmaps, nblocks, m, ndata, (long long)rw2.size(), rw2.data(), row2.data(), col2.data(), 0.01f, -1, measures.data(), nullptr, nullptr, nullptr,
                               nullptr, nullptr) != 1) ++bad;
        }
        if (per > 1) {
            std::vector<int> col2(col);
            col2[1] = col2[0];
            if (hmr_resolution(nx, ny, nmaps, nblocks, m, ndata, (long long)rw.size(), rw.data(), row.data(), col2.data(), 0.01f, -1, measures.data(), nullptr, nullptr, nullptr, nullptr,
                               nullptr) != 2) ++bad;
        }
    }
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
#endif
