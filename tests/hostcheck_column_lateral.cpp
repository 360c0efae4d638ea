// TEST HARNESS (not product): the laterally coupled column step of dsurftomo_amd/csrc/column_lateral.h on a CPU behind a C interface, for
// tests/test_hostcheck_column_lateral.py and tests/test_gpu_column_lateral.py -- one lane of one, the barrier a no-op, the columns one after
// another where the device runs one block each: the arithmetic the kernels share out.  The loop over the iterations is the engine's: bounded
// by maxit, the done flag looked at every `poll` iterations.  A library of its own so that the other harnesses stay as they are.  With
// -DHOSTCHECK_COLUMN_LATERAL_MAIN the file is a stand-alone program that runs the step on made-up grids of every tested size and on the
// special cases (for a sanitizer build).
#include <cstdio>
#include <vector>

#include "../dsurftomo_amd/csrc/column_lateral.h"

using namespace dsa;

namespace {
struct NoBarrier { void operator()() const {} };
}

extern "C" {

long long hlat_ws_doubles(int nx, int ny, int M) { return (long long)lateral_ws_doubles(nx - 2, ny - 2, M); }

// The step of the interior columns of an (ny, nx) grid of columns that lie the way the engine holds them: obs / wt (K, ncol) (wt may be null),
// pv (K, ncol), S (M, K, ncol), vels (M or more, ncol) stepped in place, dv (M, ncol), nused / chi2 / flag (ncol), info (4), delta (null, or
// (M, ncol): the fp64 solution before it is rounded and clipped, 0 where the column was left alone).  The ring's outputs are left alone.
// poll: the done flag is looked at after every poll-th iteration (0: never -- all maxit iterations are started).  Returns the iterations started.
int hlat_step(int nx, int ny, int M, int K, const float* obs, const float* wt, const double* pv, const double* S, float smooth, float damp, float lateral,
              float dvmax, float minvel, float maxvel, double tol, int maxit, int poll, float* vels, float* dv, int* nused, double* chi2, int* flag, double* info,
              double* delta)
{
    const int nvx = nx - 2, nvy = ny - 2, n = nvx * nvy;
    const long long ncol = (long long)nx * ny;
    std::vector<double> work(column_work_doubles(M, K)), base(lateral_ws_doubles(nvx, nvy, M), 0.0), chains(kLateralChains);
    const ColumnWork w = column_work(work.data(), M, K);
    const LateralWs ws = lateral_ws(base.data(), nvx, nvy, M, lateral);
    const NoBarrier sync;
    for (int b = 0; b < n; ++b) {
        const long long c = lateral_model_column(ws, b);
        ColumnIn in;
        in.M = M; in.K = K;
        in.obs = obs + c; in.obs_stride = ncol;
        in.wt = wt ? wt + c : nullptr; in.wt_stride = ncol;
        in.pv = pv + c; in.pv_stride = ncol;
        in.S = S + c; in.s_lstride = (long long)K * ncol; in.s_kstride = ncol;
        flag[c] = lateral_setup(in, smooth, damp, w, ws, b, &nused[c], &chi2[c], 0, 1, sync);
    }
    for (int b = 0; b < n; ++b) lateral_start(ws, b, vels, ncol, 0, 1, sync);
    lateral_reduce(ws, kLatSumRz0, tol, maxit, chains.data(), 0, 1, sync);
    for (int b = 0; b < n; ++b) lateral_residual(ws, b, 0, 1, sync);
    lateral_reduce(ws, kLatSumFirst, tol, maxit, chains.data(), 0, 1, sync);
    int started = 0;
    for (int it = 1; lateral > 0.0f && it <= maxit; ++it) {
        ++started;
        for (int b = 0; b < n; ++b) lateral_direction(ws, b, 0, 1, sync);
        lateral_reduce(ws, kLatSumPq, tol, maxit, chains.data(), 0, 1, sync);
        for (int b = 0; b < n; ++b) lateral_update(ws, b, 0, 1, sync);
        lateral_reduce(ws, kLatSumRz, tol, maxit, chains.data(), 0, 1, sync);
        if (poll > 0 && it % poll == 0 && ws.ic[kLatDone]) break;
    }
    for (int b = 0; b < n; ++b) {
        if (delta) {
            const LateralColumn col = lateral_column(ws, b);
            for (int l = 0; l < M; ++l) delta[(size_t)l * ncol + lateral_model_column(ws, b)] = ws.active[b] ? col.x[l] : 0.0;
        }
        lateral_finish(ws, b, dvmax, minvel, maxvel, vels, ncol, dv, ncol, 0, 1);
    }
    lateral_info(ws, info);
    return started;
}

// the global sum's shape on n given figures (one lane)
double hlat_sum(int n, const double* part)
{
    std::vector<double> base(lateral_ws_doubles(n, 1, 1), 0.0), chains(kLateralChains);
    const LateralWs ws = lateral_ws(base.data(), n, 1, 1, 1.0f);
    for (int b = 0; b < n; ++b) ws.part[b] = part[b];
    return lateral_sum(ws, chains.data(), 0, 1, NoBarrier());
}

}  // extern "C"

#ifdef HOSTCHECK_COLUMN_LATERAL_MAIN
namespace {
unsigned long long g_state = 88172645463325252ull;
double uniform()          // xorshift64, in [0, 1)
{
    g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
    return (double)(g_state >> 11) / 9007199254740992.0;
}

struct Case {
    int nx, ny, M, K;
    std::vector<float> obs, wt, vels, dv;
    std::vector<double> pv, S, chi2;
    std::vector<int> nused, flag;
    double info[4];
    Case(int nvx, int nvy, int M_, int K_) : nx(nvx + 2), ny(nvy + 2), M(M_), K(K_)
    {
        const size_t ncol = (size_t)nx * ny;
        obs.resize(K * ncol); wt.resize(K * ncol); vels.resize((M + 1) * ncol); dv.assign(M * ncol, 0.0f);
        pv.resize(K * ncol); S.resize((size_t)M * K * ncol); chi2.assign(ncol, 0.0); nused.assign(ncol, 0); flag.assign(ncol, 0);
        for (auto& v : obs) v = (float)(3.0 + uniform());
        for (auto& v : wt) v = (float)(0.5 + uniform());
        for (auto& v : pv) v = 3.0 + uniform();
        for (auto& v : S) v = uniform() / M;
        for (auto& v : vels) v = (float)(3.0 + uniform());
    }
    int step(float lateral, double tol, int maxit, int poll)
    {
        return hlat_step(nx, ny, M, K, obs.data(), wt.data(), pv.data(), S.data(), 0.3f, 0.1f, lateral, 0.2f, 3.1f, 3.9f, tol, maxit, poll, vels.data(), dv.data(),
                         nused.data(), chi2.data(), flag.data(), info, nullptr);
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
                const std::vector<float> before = c.vels;
                const int started = c.step(lateral, 1e-10, 400, 16);
                double sum = 0.0;
                for (size_t q = 0; q < c.dv.size(); ++q) {
                    sum += c.dv[q];
                    if (!(c.dv[q] >= -0.2f && c.dv[q] <= 0.2f)) ++bad;
                }
                for (int j = 0; j < c.ny; ++j)
                    for (int i = 0; i < c.nx; ++i) {
                        const size_t col = (size_t)j * c.nx + i;
                        const bool ring = i == 0 || j == 0 || i == c.nx - 1 || j == c.ny - 1;
                        for (int l = 0; l <= c.M; ++l) {
                            const float v = c.vels[(size_t)l * ncol + col];
                            if ((ring || l == c.M || c.flag[col] != 0) && v != before[(size_t)l * ncol + col]) ++bad;
                            if (!ring && l < c.M && c.flag[col] == 0 && !(v >= 3.1f && v <= 3.9f)) ++bad;
                        }
                        if (ring && (c.flag[col] != 0 || c.nused[col] != 0)) ++bad;
                    }
                if (c.flag[centre] != (lateral > 0.0f ? kColumnOk : kColumnNoData) || c.nused[centre] != 0) ++bad;
                if (c.info[1] != 1.0 || (lateral == 0.0f && (c.info[0] != 0.0 || started != 0))) ++bad;
                std::printf("%d x %d M %2d K %2d lateral %.1f: itn %3.0f istop %.0f rz0 %.6g rz %.3g, %d iterations started, sum of dv %.9g\n", g[0], g[1], mk[0], mk[1],
                            (double)lateral, c.info[0], c.info[1], c.info[2], c.info[3], started, sum);
            }
        }
    {   // a column whose kernels are not finite: flag 1, left alone, and its neighbours lose an edge; maxit = 1: istop 2
        Case c(3, 3, 4, 6);
        const size_t ncol = 25;
        for (int l = 0; l < c.M; ++l) c.S[((size_t)l * c.K + 2) * ncol + 12] = NAN;
        const std::vector<float> before = c.vels;
        c.step(0.5f, 1e-10, 1, 1);
        if (c.flag[12] != kColumnNotPositive || c.info[1] != 2.0 || c.info[0] != 1.0) ++bad;
        for (int l = 0; l < c.M; ++l) if (c.vels[(size_t)l * ncol + 12] != before[(size_t)l * ncol + 12] || c.dv[(size_t)l * ncol + 12] != 0.0f) ++bad;
        std::printf("not finite: flag %d itn %.0f istop %.0f\n", c.flag[12], c.info[0], c.info[1]);
    }
    {   // every column without a datum on a model without lateral differences: a defined zero step
        Case c(3, 3, 4, 6);
        for (auto& v : c.wt) v = 0.0f;
        for (size_t q = 0; q < c.vels.size(); ++q) c.vels[q] = 3.5f;
        c.step(0.5f, 1e-10, 10, 1);
        for (const float s : c.dv) if (s != 0.0f) ++bad;
        if (c.info[0] != 0.0 || c.info[1] != 1.0 || c.info[2] != 0.0) ++bad;
        std::printf("no data anywhere: itn %.0f istop %.0f rz0 %g\n", c.info[0], c.info[1], c.info[2]);
    }
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
#endif
