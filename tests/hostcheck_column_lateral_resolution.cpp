// TEST HARNESS (not product): the resolution of the laterally coupled column step, dsurftomo_amd/csrc/column_lateral_resolution.h, on a CPU
// behind a C interface, for tests/test_hostcheck_column_lateral_resolution.py and tests/test_gpu_column_lateral_resolution.py -- one lane of
// one, the barrier a no-op, the columns and the lane groups one after another where the device runs one block each.  The loops over the
// chunks and the iterations are the engine's: chunks of whole lane groups, the done flags looked at every `poll` iterations.  hlres_anchor is
// section 24's own loop (column_lateral.h) with the right-hand side overwritten, for the bit anchor.  A library of its own so that the other
// harnesses stay as they are.  With -DHOSTCHECK_COLUMN_LATERAL_RESOLUTION_MAIN the file is a stand-alone program over made-up grids of
// every tested size and the special cases (for a sanitizer build).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "../dsurftomo_amd/csrc/column_lateral_resolution.h"

using namespace dsa;

namespace {
struct NoBarrier { void operator()() const {} };

ColumnIn column_in(int nx, int ny, int M, int K, long long c, const float* obs, const float* wt, const double* pv, const double* S)
{
    const long long ncol = (long long)nx * ny;
    ColumnIn in;
    in.M = M; in.K = K;
    in.obs = obs + c; in.obs_stride = ncol;
    in.wt = wt ? wt + c : nullptr; in.wt_stride = ncol;
    in.pv = pv + c; in.pv_stride = ncol;
    in.S = S + c; in.s_lstride = (long long)K * ncol; in.s_kstride = ncol;
    return in;
}
}

extern "C" {

long long hlres_group_bytes(int nx, int ny, int M) { return (long long)(latres_member_bytes(nx - 2, ny - 2, M) * kLatResGroup); }
long long hlres_work_doubles(int M) { return (long long)latres_work_doubles(M); }

// The members kind / index (nmembers) on the interior columns of an (ny, nx) grid of columns that lie the way the engine holds them: obs / wt
// (K, ncol) (wt may be null), pv (K, ncol), S (M, K, ncol), depz (M or more); models: null or (nrows, M, nint).  measures (nmembers, 7), info
// (nmembers, 4), full: null or (nmembers, M, nint); nused / flag (ncol), the ring's left alone.  groups: the lane groups of a chunk (0: all the
// members in one chunk).  poll: the done flags are looked at after every poll-th iteration (0: never).  Returns the iterations started, all
// chunks together.
int hlres_run(int nx, int ny, int M, int K, const float* obs, const float* wt, const double* pv, const double* S, const float* depz, float smooth, float damp,
              float lateral, double tol, int maxit, int poll, int groups, int nmembers, const int* kind, const int* index, const double* models, double* measures,
              double* info, double* full, int* nused, int* flag)
{
    const int nvx = nx - 2, nvy = ny - 2, n = nvx * nvy, T = column_tri_size(M);
    std::vector<double> work(column_work_doubles(M, K)), base(lateral_ws_doubles(nvx, nvy, M), 0.0), H((size_t)n * T, 0.0), lds(latres_work_doubles(M), 0.0);
    const ColumnWork cw = column_work(work.data(), M, K);
    const LateralWs ws = lateral_ws(base.data(), nvx, nvy, M, lateral);
    const NoBarrier sync;
    for (int b = 0; b < n; ++b) {
        const long long c = lateral_model_column(ws, b);
        const ColumnIn in = column_in(nx, ny, M, K, c, obs, wt, pv, S);
        double chi2 = 0.0;
        flag[c] = lateral_setup(in, smooth, damp, cw, ws, b, &nused[c], &chi2, 0, 1, sync);
    }
    for (int b = 0; b < n; ++b) latres_gram(column_in(nx, ny, M, K, lateral_model_column(ws, b), obs, wt, pv, S), cw, ws, b, H.data(), 0, 1, sync);
    const int all = latres_round(nmembers), chunk = groups > 0 ? std::min(all, groups * kLatResGroup) : all;
    const LatResWork w = latres_work(lds.data(), M);
    std::vector<double> batch, meas;
    int started = 0;
    for (int first = 0; first < nmembers; first += chunk) {
        const int count = std::min(chunk, nmembers - first), Sc = latres_round(count), G = Sc / kLatResGroup;
        batch.assign(latres_batch_doubles(nvx, nvy, M, Sc), 0.0);
        meas.assign((size_t)Sc * kLatResMeasures, 0.0);
        const LatResBatch B = latres_batch(ws, H.data(), depz, models, batch.data(), Sc);
        for (int s = 0; s < Sc; ++s) { B.kind[s] = s < count ? kind[first + s] : -1; B.index[s] = s < count ? index[first + s] : 0; }
        for (int g = 0; g < G; ++g) for (int b = 0; b < n; ++b) latres_form(B, b, g, w, 0, 1, sync);
        for (int g = 0; g < G; ++g) for (int b = 0; b < n; ++b) latres_start(B, b, g, w, 0, 1, sync);
        for (int g = 0; g < G; ++g) latres_reduce(B, g, kLatSumRz0, tol, maxit, 0, 1);
        for (int g = 0; g < G; ++g) for (int b = 0; b < n; ++b) latres_residual(B, b, g, w, 0, 1, sync);
        for (int g = 0; g < G; ++g) latres_reduce(B, g, kLatSumFirst, tol, maxit, 0, 1);
        for (int it = 1; ws.edges && it <= maxit; ++it) {
            ++started;
            for (int g = 0; g < G; ++g) for (int b = 0; b < n; ++b) latres_direction(B, b, g, w, 0, 1, sync);
            for (int g = 0; g < G; ++g) latres_reduce(B, g, kLatSumPq, tol, maxit, 0, 1);
            for (int g = 0; g < G; ++g) for (int b = 0; b < n; ++b) latres_update(B, b, g, w, 0, 1, sync);
            for (int g = 0; g < G; ++g) latres_reduce(B, g, kLatSumRz, tol, maxit, 0, 1);
            if (poll > 0 && it % poll == 0 && it < maxit) {
                bool done = true;
                for (int s = 0; s < Sc && done; ++s) done = B.ic[kLatDone * Sc + s] != 0;
                if (done) break;
            }
        }
        for (int g = 0; g < G; ++g) for (int b = 0; b < n; ++b) latres_measure(B, b, g, w, 0, 1, sync);
        for (int g = 0; g < G; ++g) latres_measures(B, g, meas.data(), 0, 1);
        for (int s = 0; s < count; ++s) {
            for (int q = 0; q < kLatResMeasures; ++q) measures[(size_t)(first + s) * kLatResMeasures + q] = meas[(size_t)s * kLatResMeasures + q];
            double* o = info + (size_t)(first + s) * 4;
            o[0] = (double)B.ic[kLatItn * Sc + s]; o[1] = (double)B.ic[kLatStop * Sc + s]; o[2] = B.sc[kLatRz0 * Sc + s]; o[3] = B.sc[kLatRz * Sc + s];
            if (full)
                for (int l = 0; l < M; ++l)
                    for (int b = 0; b < n; ++b) full[((size_t)(first + s) * M + l) * n + b] = B.q[latres_at(B, b, l, s)];
        }
    }
    return started;
}

// section 24's own loop, column_lateral.h as dsa_columns_step_lateral runs it, with b_c overwritten by f (M, nint: depth slowest; 0.0 is
// stored in a column that is not active) on a model without lateral differences: x (M, nint), info (4).
void hlres_anchor(int nx, int ny, int M, int K, const float* obs, const float* wt, const double* pv, const double* S, float smooth, float damp, float lateral,
                  double tol, int maxit, const double* f, double* x, double* info)
{
    const int nvx = nx - 2, nvy = ny - 2, n = nvx * nvy;
    const long long ncol = (long long)nx * ny;
    std::vector<double> work(column_work_doubles(M, K)), base(lateral_ws_doubles(nvx, nvy, M), 0.0), chains(kLateralChains);
    std::vector<float> vels((size_t)M * ncol, 3.5f);
    std::vector<int> nused(ncol, 0);
    const ColumnWork cw = column_work(work.data(), M, K);
    const LateralWs ws = lateral_ws(base.data(), nvx, nvy, M, lateral);
    const NoBarrier sync;
    for (int b = 0; b < n; ++b) {
        const long long c = lateral_model_column(ws, b);
        double chi2 = 0.0;
        (void)lateral_setup(column_in(nx, ny, M, K, c, obs, wt, pv, S), smooth, damp, cw, ws, b, &nused[c], &chi2, 0, 1, sync);
    }
    for (int b = 0; b < n; ++b) {
        if (!ws.active[b]) continue;
        const LateralColumn col = lateral_column(ws, b);
        for (int l = 0; l < M; ++l) col.b[l] = f[(size_t)l * n + b];
    }
    for (int b = 0; b < n; ++b) lateral_start(ws, b, vels.data(), ncol, 0, 1, sync);
    lateral_reduce(ws, kLatSumRz0, tol, maxit, chains.data(), 0, 1, sync);
    for (int b = 0; b < n; ++b) lateral_residual(ws, b, 0, 1, sync);
    lateral_reduce(ws, kLatSumFirst, tol, maxit, chains.data(), 0, 1, sync);
    for (int it = 1; lateral > 0.0f && it <= maxit; ++it) {
        for (int b = 0; b < n; ++b) lateral_direction(ws, b, 0, 1, sync);
        lateral_reduce(ws, kLatSumPq, tol, maxit, chains.data(), 0, 1, sync);
        for (int b = 0; b < n; ++b) lateral_update(ws, b, 0, 1, sync);
        lateral_reduce(ws, kLatSumRz, tol, maxit, chains.data(), 0, 1, sync);
        if (ws.ic[kLatDone]) break;
    }
    for (int b = 0; b < n; ++b) {
        const LateralColumn col = lateral_column(ws, b);
        for (int l = 0; l < M; ++l) x[(size_t)l * n + b] = ws.active[b] ? col.x[l] : 0.0;
    }
    lateral_info(ws, info);
}

// the right-hand side of dsa_columns_step_lateral on the model vels (M or more, ncol): column_lateral.h's bt (M, nint), 0.0 in a column that
// is not active
void hlres_rhs(int nx, int ny, int M, int K, const float* obs, const float* wt, const double* pv, const double* S, float smooth, float damp, float lateral,
               const float* vels, double* bt)
{
    const int nvx = nx - 2, nvy = ny - 2, n = nvx * nvy;
    const long long ncol = (long long)nx * ny;
    std::vector<double> work(column_work_doubles(M, K)), base(lateral_ws_doubles(nvx, nvy, M), 0.0);
    std::vector<int> nused(ncol, 0);
    const ColumnWork cw = column_work(work.data(), M, K);
    const LateralWs ws = lateral_ws(base.data(), nvx, nvy, M, lateral);
    const NoBarrier sync;
    for (int b = 0; b < n; ++b) {
        const long long c = lateral_model_column(ws, b);
        double chi2 = 0.0;
        (void)lateral_setup(column_in(nx, ny, M, K, c, obs, wt, pv, S), smooth, damp, cw, ws, b, &nused[c], &chi2, 0, 1, sync);
    }
    for (int b = 0; b < n; ++b) lateral_start(ws, b, vels, ncol, 0, 1, sync);
    for (int b = 0; b < n; ++b) {
        const LateralColumn col = lateral_column(ws, b);
        for (int l = 0; l < M; ++l) bt[(size_t)l * n + b] = ws.active[b] ? col.b[l] : 0.0;
    }
}

}  // extern "C"

#ifdef HOSTCHECK_COLUMN_LATERAL_RESOLUTION_MAIN
namespace {
unsigned long long g_state = 88172645463325252ull;
double uniform()          // xorshift64, in [0, 1)
{
    g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
    return (double)(g_state >> 11) / 9007199254740992.0;
}

struct Case {
    int nx, ny, M, K, n;
    std::vector<float> obs, wt, depz;
    std::vector<double> pv, S, models;
    std::vector<int> nused, flag, kind, index;
    std::vector<double> measures, info, full;
    Case(int nvx, int nvy, int M_, int K_) : nx(nvx + 2), ny(nvy + 2), M(M_), K(K_), n(nvx * nvy)
    {
        const size_t ncol = (size_t)nx * ny;
        obs.resize(K * ncol); wt.resize(K * ncol); pv.resize(K * ncol); S.resize((size_t)M * K * ncol); nused.assign(ncol, 0); flag.assign(ncol, 0);
        depz.resize(M + 1);
        for (int l = 0; l <= M; ++l) depz[l] = (float)(2.5 * l * (1.0 + 0.1 * l));
        for (auto& v : obs) v = (float)(3.0 + uniform());
        for (auto& v : wt) v = (float)(0.5 + uniform());
        for (auto& v : pv) v = 3.0 + uniform();
        for (auto& v : S) v = uniform() / M;
        models.resize((size_t)2 * M * n);
        for (auto& v : models) v = uniform() - 0.5;
        // every unknown as a spike and as a row (where there are many: the top and the bottom of three columns), one model, one given right-hand side
        for (int j = 0; j < n * M; ++j) {
            const bool few = (j / M == 0 || j / M == n / 2 || j / M == n - 1) && (j % M == 0 || j % M == M - 1);
            if (n * M <= 96 || few) { kind.push_back(0); index.push_back(j); kind.push_back(1); index.push_back(j); }
        }
        kind.push_back(2); index.push_back(0);
        kind.push_back(3); index.push_back(1);
    }
    int run(float lateral, double tol, int maxit, int poll, int groups)
    {
        const size_t m = kind.size();
        measures.assign(m * 7, 0.0); info.assign(m * 4, 0.0); full.assign(m * M * n, 0.0);
        return hlres_run(nx, ny, M, K, obs.data(), wt.data(), pv.data(), S.data(), depz.data(), 0.3f, 0.1f, lateral, tol, maxit, poll, groups, (int)m, kind.data(),
                         index.data(), models.data(), measures.data(), info.data(), full.data(), nused.data(), flag.data());
    }
};
}

int main()
{
    const int grids[][2] = { { 1, 1 }, { 3, 3 }, { 4, 2 }, { 9, 8 } };
    const int sizes[][2] = { { 1, 1 }, { 2, 3 }, { 7, 12 }, { 63, 60 } };
    int bad = 0;
    for (const auto& g : grids)
        for (const auto& mk : sizes) {
            if (mk[0] == 63 && g[0] != 3) continue;
            for (const float lateral : { 0.0f, 0.5f }) {
                Case c(g[0], g[1], mk[0], mk[1]);
                const size_t ncol = (size_t)c.nx * c.ny;
                const int centre = (c.ny / 2) * c.nx + c.nx / 2;
                // the centre column: no datum at all, its S not finite; its left neighbour (where there is one): one datum without a root
                for (int k = 0; k < c.K; ++k) {
                    c.wt[(size_t)k * ncol + centre] = 0.0f;
                    for (int l = 0; l < c.M; ++l) c.S[((size_t)l * c.K + k) * ncol + centre] = NAN;
                }
                if (g[0] > 1 && c.K > 1) {
                    c.pv[centre - 1] = 0.0;
                    for (int l = 0; l < c.M; ++l) c.S[((size_t)l * c.K) * ncol + centre - 1] = NAN;
                }
                const int started = c.run(lateral, 1e-10, 400, 16, mk[0] == 63 ? 1 : 0);
                const std::vector<double> one = c.full, m1 = c.measures;
                c.run(lateral, 1e-10, 400, 1, 1);
                int itmin = 1 << 30, itmax = 0;
                for (size_t s = 0; s < c.kind.size(); ++s) {
                    itmin = std::min(itmin, (int)c.info[4 * s]); itmax = std::max(itmax, (int)c.info[4 * s]);
                    if (c.info[4 * s + 1] != 1.0) ++bad;
                    for (int q = 0; q < 7; ++q) if (!std::isfinite(c.measures[7 * s + q]) || c.measures[7 * s + q] != m1[7 * s + q]) ++bad;
                    if (c.measures[7 * s + 1] < 0.0 || c.measures[7 * s + 5] > c.measures[7 * s + 1] || c.measures[7 * s + 6] < 0.0) ++bad;
                }
                for (size_t q = 0; q < one.size(); ++q) if (!std::isfinite(one[q]) || one[q] != c.full[q]) ++bad;
                if (lateral == 0.0f && (itmax != 0 || started != 0)) ++bad;
                std::printf("%d x %d M %2d K %2d lateral %.1f: %zu members, itn %d .. %d, %d iterations started\n", g[0], g[1], mk[0], mk[1], (double)lateral,
                            c.kind.size(), itmin, itmax, started);
            }
        }
    {   // a column whose kernels are not finite: flag 1, its members zeros; maxit = 1: istop 2
        Case c(3, 3, 4, 6);
        const size_t ncol = 25;
        for (int l = 0; l < c.M; ++l) c.S[((size_t)l * c.K + 2) * ncol + 12] = NAN;
        c.run(0.5f, 1e-10, 1, 1, 0);
        if (c.flag[12] != kColumnNotPositive) ++bad;
        for (size_t s = 0; s < c.kind.size(); ++s) {
            const bool inside = c.kind[s] < 2 && c.index[s] / c.M == 4;
            if (inside) { for (int q = 0; q < 7; ++q) if (c.measures[7 * s + q] != 0.0) ++bad; if (c.info[4 * s] != 0.0) ++bad; }
            else if (c.kind[s] < 2 && (c.info[4 * s + 1] != 2.0 || c.info[4 * s] != 1.0)) ++bad;
        }
        std::printf("not finite: flag %d\n", c.flag[12]);
    }
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
#endif
