// TEST HARNESS (not product): the laterally coupled radial column step of dsurftomo_amd/csrc/column_radial_lateral.h on a CPU behind a C
// interface, for tests/test_hostcheck_column_radial_lateral.py and tests/test_gpu_column_radial_lateral.py -- one lane of one, the barrier a
// no-op, the columns one after another where the device runs one block each: the arithmetic the kernels share out.  The loop over the
// iterations is the engine's: bounded by maxit, the done flag looked at every `poll` iterations.  A library of its own so that the other
// harnesses stay as they are.  With -DHOSTCHECK_COLUMN_RADIAL_LATERAL_MAIN the file is a stand-alone program that runs the step on made-up
// grids of every tested size and on the special cases (for a sanitizer build).
#include <cstdio>
#include <vector>

#include "../dsurftomo_amd/csrc/column_radial_lateral.h"

using namespace dsa;

namespace {
struct NoBarrier { void operator()() const {} };
}

extern "C" {

long long hrlat_ws_doubles(int nx, int ny, int M) { return (long long)radial_lateral_ws_doubles(nx - 2, ny - 2, M); }

// The step of the interior columns of an (ny, nx) grid of columns that lie the way the engine holds them: obs / wt (K, ncol) (wt may be null),
// pv (K, ncol), Sv / Sh (M, K, ncol), vsv / vsh (M or more, ncol) stepped in place, dv (2, M, ncol), nused / chi2 (2, ncol), flag (ncol),
// info (4), delta (null, or (2M, ncol): the fp64 solution before it is rounded and clipped, 0 where the column was left alone).  love: bit k
// set where slot k is a Love slot.  The ring's outputs are left alone.  poll: the done flag is looked at after every poll-th iteration (0:
// never -- all maxit iterations are started).  Returns the iterations started.
int hrlat_step(int nx, int ny, int M, int K, unsigned long long love, const float* obs, const float* wt, const double* pv, const double* Sv, const double* Sh,
               float smooth, float damp, float aniso, float lateral, float lateral_aniso, float dvmax, float minvel, float maxvel, double tol, int maxit, int poll,
               float* vsv, float* vsh, float* dv, int* nused, double* chi2, int* flag, double* info, double* delta)
{
    const int nvx = nx - 2, nvy = ny - 2, n = nvx * nvy, B = 2 * M;
    const long long ncol = (long long)nx * ny;
    std::vector<double> work(radial_work_doubles(M, K)), base(radial_lateral_ws_doubles(nvx, nvy, M), 0.0), chains(kLateralChains);
    const ColumnWork w = radial_work(work.data(), M, K);
    const RadialLateralWs rl = radial_lateral_ws(base.data(), nvx, nvy, M, lateral, lateral_aniso);
    const LateralWs& ws = rl.ws;
    const NoBarrier sync;
    for (int b = 0; b < n; ++b) {
        const long long c = lateral_model_column(ws, b);
        RadialIn in;
        in.M = M; in.K = K; in.love = love;
        in.obs = obs + c; in.obs_stride = ncol;
        in.wt = wt ? wt + c : nullptr; in.wt_stride = ncol;
        in.pv = pv + c; in.pv_stride = ncol;
        in.Sv = Sv + c; in.Sh = Sh + c; in.s_lstride = (long long)K * ncol; in.s_kstride = ncol;
        int nu[2];
        double x2[2];
        flag[c] = radial_lateral_setup(in, smooth, damp, aniso, vsv + c, vsh + c, ncol, w, rl, b, nu, x2, 0, 1, sync);
        nused[c] = nu[0]; nused[ncol + c] = nu[1];
        chi2[c] = x2[0]; chi2[ncol + c] = x2[1];
    }
    for (int b = 0; b < n; ++b) radial_lateral_start(rl, b, vsv, vsh, ncol, 0, 1, sync);
    lateral_reduce(ws, kLatSumRz0, tol, maxit, chains.data(), 0, 1, sync);
    for (int b = 0; b < n; ++b) radial_lateral_residual(rl, b, 0, 1, sync);
    lateral_reduce(ws, kLatSumFirst, tol, maxit, chains.data(), 0, 1, sync);
    int started = 0;
    for (int it = 1; ws.edges && it <= maxit; ++it) {
        ++started;
        for (int b = 0; b < n; ++b) radial_lateral_direction(rl, b, 0, 1, sync);
        lateral_reduce(ws, kLatSumPq, tol, maxit, chains.data(), 0, 1, sync);
        for (int b = 0; b < n; ++b) lateral_update(ws, b, 0, 1, sync);
        lateral_reduce(ws, kLatSumRz, tol, maxit, chains.data(), 0, 1, sync);
        if (poll > 0 && it % poll == 0 && ws.ic[kLatDone]) break;
    }
    for (int b = 0; b < n; ++b) {
        if (delta) {
            const LateralColumn col = lateral_column(ws, b);
            for (int i = 0; i < B; ++i) delta[(size_t)i * ncol + lateral_model_column(ws, b)] = ws.active[b] ? col.x[i] : 0.0;
        }
        radial_lateral_finish(rl, b, dvmax, minvel, maxvel, vsv, vsh, ncol, dv, dv + (size_t)M * ncol, ncol, 0, 1);
    }
    lateral_info(ws, info);
    return started;
}

}  // extern "C"

#ifdef HOSTCHECK_COLUMN_RADIAL_LATERAL_MAIN
namespace {
unsigned long long g_state = 88172645463325252ull;
double uniform()          // xorshift64, in [0, 1)
{
    g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
    return (double)(g_state >> 11) / 9007199254740992.0;
}

struct Case {
    int nx, ny, M, K;
    unsigned long long love;
    std::vector<float> obs, wt, vsv, vsh, dv;
    std::vector<double> pv, Sv, Sh, chi2;
    std::vector<int> nused, flag;
    double info[4];
    Case(int nvx, int nvy, int M_, int K_) : nx(nvx + 2), ny(nvy + 2), M(M_), K(K_), love(0ull)
    {
        const size_t ncol = (size_t)nx * ny;
        for (int k = 0; k < K; ++k) if (k % 2) love |= 1ull << k;          // odd slots are Love slots
        obs.resize(K * ncol); wt.resize(K * ncol); vsv.resize((M + 1) * ncol); vsh.resize((M + 1) * ncol); dv.assign(2 * M * ncol, 0.0f);
        pv.resize(K * ncol); Sv.resize((size_t)M * K * ncol); Sh.resize((size_t)M * K * ncol); chi2.assign(2 * ncol, 0.0); nused.assign(2 * ncol, 0);
        flag.assign(ncol, 0);
        for (auto& v : obs) v = (float)(3.0 + uniform());
        for (auto& v : wt) v = (float)(0.5 + uniform());
        for (auto& v : pv) v = 3.0 + uniform();
        for (auto& v : Sv) v = uniform() / M;
        for (auto& v : Sh) v = uniform() / M;
        for (auto& v : vsv) v = (float)(3.0 + uniform());
        for (size_t q = 0; q < vsh.size(); ++q) vsh[q] = vsv[q] * (float)(1.0 + 0.06 * uniform());
        // a slot's S on the model it was not run on is never read
        for (int k = 0; k < K; ++k)
            for (int l = 0; l < M; ++l)
                for (size_t c = 0; c < ncol; ++c) (k % 2 ? Sv : Sh)[((size_t)l * K + k) * ncol + c] = NAN;
    }
    int step(float lateral, float lateral_aniso, double tol, int maxit, int poll)
    {
        return hrlat_step(nx, ny, M, K, love, obs.data(), wt.data(), pv.data(), Sv.data(), Sh.data(), 0.3f, 0.1f, 0.2f, lateral, lateral_aniso, 0.2f, 3.1f, 4.2f, tol,
                          maxit, poll, vsv.data(), vsh.data(), dv.data(), nused.data(), chi2.data(), flag.data(), info, nullptr);
    }
};
}

int main()
{
    const int grids[][2] = { { 1, 1 }, { 3, 3 }, { 4, 2 }, { 9, 8 } };
    const int sizes[][2] = { { 1, 2 }, { 2, 4 }, { 7, 12 }, { 63, 60 } };
    const float weights[][2] = { { 0.0f, 0.0f }, { 0.5f, 0.0f }, { 0.5f, 5.0f }, { 0.0f, 0.5f } };
    int bad = 0;
    for (const auto& g : grids)
        for (const auto& mk : sizes) {
            if (mk[0] == 63 && g[0] != 3) continue;
            for (const auto& ww : weights) {
                Case c(g[0], g[1], mk[0], mk[1]);
                const size_t ncol = (size_t)c.nx * c.ny;
                const int centre = (c.ny / 2) * c.nx + c.nx / 2;
                const bool edges = ww[0] > 0.0f || ww[1] > 0.0f;
                // the centre column: no datum at all, its S not finite; its left neighbour (where there is one): one datum without a root
                for (int k = 0; k < c.K; ++k) {
                    c.wt[(size_t)k * ncol + centre] = 0.0f;
                    for (int l = 0; l < c.M; ++l) { c.Sv[((size_t)l * c.K + k) * ncol + centre] = NAN; c.Sh[((size_t)l * c.K + k) * ncol + centre] = NAN; }
                }
                if (g[0] > 1) {
                    c.pv[centre - 1] = 0.0;
                    for (int l = 0; l < c.M; ++l) c.Sv[((size_t)l * c.K) * ncol + centre - 1] = NAN;
                }
                const std::vector<float> before_v = c.vsv, before_h = c.vsh;
                const int started = c.step(ww[0], ww[1], 1e-10, mk[0] == 63 ? 40 : 600, 16);
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
                            const float v = c.vsv[(size_t)l * ncol + col], h = c.vsh[(size_t)l * ncol + col];
                            if ((ring || l == c.M || c.flag[col] != 0) && (v != before_v[(size_t)l * ncol + col] || h != before_h[(size_t)l * ncol + col])) ++bad;
                            if (!ring && l < c.M && c.flag[col] == 0 && !(v >= 3.1f && v <= 4.2f && h >= 3.1f && h <= 4.2f)) ++bad;
                        }
                        if (ring && (c.flag[col] != 0 || c.nused[col] != 0 || c.nused[ncol + col] != 0)) ++bad;
                    }
                if (c.flag[centre] != (edges ? kColumnOk : kColumnNoData) || c.nused[centre] != 0 || c.nused[ncol + centre] != 0) ++bad;
                if (mk[0] != 63 && c.info[1] != 1.0) ++bad;
                if (!edges && (c.info[0] != 0.0 || c.info[1] != 1.0 || started != 0)) ++bad;
                std::printf("%d x %d M %2d K %2d lateral %.1f aniso %.1f: itn %3.0f istop %.0f rz0 %.6g rz %.3g, %d iterations started, sum of dv %.9g\n", g[0], g[1],
                            mk[0], mk[1], (double)ww[0], (double)ww[1], c.info[0], c.info[1], c.info[2], c.info[3], started, sum);
            }
        }
    {   // a column whose used kernels are not finite: flag 1, left alone, and its neighbours lose an edge; maxit = 1: istop 2
        Case c(3, 3, 4, 6);
        const size_t ncol = 25;
        for (int l = 0; l < c.M; ++l) c.Sv[((size_t)l * c.K + 2) * ncol + 12] = NAN;
        const std::vector<float> before_v = c.vsv, before_h = c.vsh;
        c.step(0.5f, 0.5f, 1e-10, 1, 1);
        if (c.flag[12] != kColumnNotPositive || c.info[1] != 2.0 || c.info[0] != 1.0) ++bad;
        for (int l = 0; l < c.M; ++l)
            if (c.vsv[(size_t)l * ncol + 12] != before_v[(size_t)l * ncol + 12] || c.vsh[(size_t)l * ncol + 12] != before_h[(size_t)l * ncol + 12] ||
                c.dv[(size_t)l * ncol + 12] != 0.0f || c.dv[((size_t)c.M + l) * ncol + 12] != 0.0f) ++bad;
        std::printf("not finite: flag %d itn %.0f istop %.0f\n", c.flag[12], c.info[0], c.info[1]);
    }
    {   // every column without a datum on two equal models without lateral differences: a defined zero step
        Case c(3, 3, 4, 6);
        for (auto& v : c.wt) v = 0.0f;
        for (size_t q = 0; q < c.vsv.size(); ++q) { c.vsv[q] = 3.5f; c.vsh[q] = 3.5f; }
        c.step(0.5f, 0.5f, 1e-10, 10, 1);
        for (const float s : c.dv) if (s != 0.0f) ++bad;
        if (c.info[0] != 0.0 || c.info[1] != 1.0 || c.info[2] != 0.0) ++bad;
        std::printf("no data anywhere: itn %.0f istop %.0f rz0 %g\n", c.info[0], c.info[1], c.info[2]);
    }
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
#endif
