// TEST HARNESS (not product): the depth resolution of the radial step, dsurftomo_amd/csrc/column_radial_resolution.h, on a CPU behind a C
// interface, for tests/test_hostcheck_column_radial_resolution.py and tests/test_gpu_column_radial_resolution.py -- one lane of one, the
// barrier a no-op: the arithmetic the kernel shares out over a block.  A library of its own so that the other harnesses stay as they are.
// With -DHOSTCHECK_COLUMN_RADIAL_RESOLUTION_MAIN the file is a stand-alone program that runs the header on made-up columns of every tested
// size and on the special cases (for a sanitizer build).
#include <cmath>
#include <cstdio>
#include <vector>

#include "../dsurftomo_amd/csrc/column_radial_resolution.h"

using namespace dsa;

namespace {
struct NoBarrier { void operator()() const {} };

RadialIn column_of(int M, int K, int ncols, int c, unsigned long long love, const float* obs, const float* wt, const double* pv, const double* Sv, const double* Sh)
{
    RadialIn in;
    in.M = M; in.K = K; in.love = love;
    in.obs = obs + c; in.obs_stride = ncols;
    in.wt = wt ? wt + c : nullptr; in.wt_stride = ncols;
    in.pv = pv + c; in.pv_stride = ncols;
    in.Sv = Sv + c; in.Sh = Sh + c; in.s_lstride = (long long)K * ncols; in.s_kstride = ncols;
    return in;
}
}

extern "C" {

long long hrr_doubles(int M, int K) { return (long long)radial_resolution_doubles(M, K); }

// The resolution of ncols columns that lie side by side the way the engine holds them: obs / wt (K, ncols) (wt may be null), pv (K, ncols),
// Sv / Sh (M, K, ncols), depz (M or more), vsv / vsh (M or more, ncols); measures (6, 2M, ncols), pair (2, M, ncols), leverage (K, ncols),
// trace / nused (2, ncols), flag (ncols), R (null, or (2M, 2M, ncols)), T (null, or (K, 2M, ncols): the generalised inverse, 0 where the
// column is flagged).  love: bit k set where slot k is a Love slot.  only: null, or one flag per column -- 0 leaves the column and its
// outputs alone (the kernel's outer ring).
void hrr_resolution(int M, int K, int ncols, const unsigned char* only, unsigned long long love, const float* obs, const float* wt, const double* pv,
                    const double* Sv, const double* Sh, const float* depz, const float* vsv, const float* vsh, float smooth, float damp, float aniso,
                    double* measures, double* pair, double* leverage, double* trace, double* R, int* nused, int* flag, double* T)
{
    std::vector<double> work(radial_resolution_doubles(M, K));
    const ColumnWork w = radial_work(work.data(), M, K);
    double* t = radial_resolution_t(work.data(), M, K);
    for (int c = 0; c < ncols; ++c) {
        if (only && !only[c]) continue;
        const RadialIn in = column_of(M, K, ncols, c, love, obs, wt, pv, Sv, Sh);
        RadialResOut out;
        out.measures = measures + c; out.m_qstride = 2ll * M * ncols; out.m_jstride = ncols;
        out.pair = pair + c; out.p_qstride = (long long)M * ncols; out.p_lstride = ncols;
        out.leverage = leverage + c; out.h_stride = ncols;
        out.R = R ? R + c : nullptr; out.r_stride = ncols;
        int n[2];
        double tr[2];
        flag[c] = radial_resolution(in, depz, smooth, damp, aniso, vsv + c, vsh + c, ncols, w, t, out, tr, n, 0, 1, NoBarrier());
        nused[c] = n[0]; nused[ncols + c] = n[1];
        trace[c] = tr[0]; trace[ncols + c] = tr[1];
        if (T)
            for (int k = 0; k < K; ++k)
                for (int i = 0; i < 2 * M; ++i) T[((size_t)k * 2 * M + i) * ncols + c] = flag[c] == kColumnOk ? t[i * K + k] : 0.0;
    }
}

// one column: assemble and factor as the resolution does, then column_solve (column_system.h, the step's) on 2M unknowns on every row of
// the expanded G in turn.  vsv / vsh: M values.  T (K, 2M): the solutions, rows of unused data 0.  Returns the flag (T untouched unless 0).
int hrr_rows_by_column_solve(int M, int K, unsigned long long love, const float* obs, const float* wt, const double* pv, const double* Sv, const double* Sh,
                             const float* vsv, const float* vsh, float smooth, float damp, float aniso, double* T)
{
    std::vector<double> work(radial_work_doubles(M, K));
    const ColumnWork w = radial_work(work.data(), M, K);
    const RadialIn in = column_of(M, K, 1, 0, love, obs, wt, pv, Sv, Sh);
    int n[2];
    double chi2[2];
    radial_assemble(in, (double)smooth * (double)smooth, (double)damp * (double)damp, (double)aniso * (double)aniso, vsv, vsh, 1, w, n, chi2, 0, 1, NoBarrier());
    if (n[0] + n[1] == 0) return kColumnNoData;
    const int f = column_factor(2 * M, w, 0, 1, NoBarrier());
    if (f != kColumnOk) return f;
    for (int k = 0; k < K; ++k) {
        const int first = radial_is_love(love, k) ? M : 0;
        for (int i = 0; i < 2 * M; ++i) w.b[i] = 0.0;
        for (int l = 0; l < M; ++l) w.b[first + l] = w.G[k * M + l];
        if (w.a[k] > 0.0) column_solve(2 * M, w, 0, 1, NoBarrier());
        for (int i = 0; i < 2 * M; ++i) T[(size_t)k * 2 * M + i] = w.a[k] > 0.0 ? w.b[i] : 0.0;
    }
    return f;
}

// factor, T and the reductions on a system given as it is: N the packed lower triangle of 2M unknowns (row by row), G (K, M) compact with
// every datum used; measures (6, 2M), pair (2, M), leverage (K), trace (2), R (null or (2M, 2M)).  Returns the flag.
int hrr_finish(int M, int K, unsigned long long love, const double* N, const double* G, const float* depz, double* measures, double* pair, double* leverage,
               double* trace, double* R)
{
    std::vector<double> work(radial_resolution_doubles(M, K), 0.0);
    const ColumnWork w = radial_work(work.data(), M, K);
    for (int e = 0; e < column_tri_size(2 * M); ++e) w.tri[e] = N[e];
    for (int e = 0; e < K * M; ++e) w.G[e] = G[e];
    for (int k = 0; k < K; ++k) w.a[k] = 1.0;
    RadialResOut out;
    out.measures = measures; out.m_qstride = 2 * M; out.m_jstride = 1;
    out.pair = pair; out.p_qstride = M; out.p_lstride = 1;
    out.leverage = leverage; out.h_stride = 1;
    out.R = R; out.r_stride = 1;
    return radial_resolution_finish(M, K, love, depz, w, radial_resolution_t(work.data(), M, K), out, trace, 0, 1, NoBarrier());
}

}  // extern "C"

#ifdef HOSTCHECK_COLUMN_RADIAL_RESOLUTION_MAIN
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
    const int sizes[][2] = { { 1, 2 }, { 2, 4 }, { 7, 12 }, { 63, 60 } };
    const int ncols = 4;
    int bad = 0;
    for (const auto& mk : sizes) {
        const int M = mk[0], K = mk[1], n2 = 2 * M;
        unsigned long long love = 0ull;
        for (int k = 0; k < K; ++k) if (k % 2) love |= 1ull << k;          // odd slots are Love slots
        std::vector<float> obs((size_t)K * ncols), wt((size_t)K * ncols), depz((size_t)M + 1), vsv((size_t)(M + 1) * ncols), vsh((size_t)(M + 1) * ncols);
        std::vector<double> pv((size_t)K * ncols), Sv((size_t)M * K * ncols), Sh((size_t)M * K * ncols), measures((size_t)6 * n2 * ncols, 9.0),
            pair((size_t)2 * M * ncols, 9.0), leverage((size_t)K * ncols, 9.0), trace(2 * ncols, 9.0), R((size_t)n2 * n2 * ncols, 9.0), T((size_t)K * n2 * ncols, 9.0);
        std::vector<int> nused(2 * ncols), flag(ncols);
        for (auto& v : obs) v = (float)(3.0 + uniform());
        for (auto& v : wt) v = (float)(0.5 + uniform());
        for (auto& v : pv) v = 3.0 + uniform();
        for (auto& v : Sv) v = uniform() * 2.0 / M;
        for (auto& v : Sh) v = uniform() * 2.0 / M;
        for (auto& v : vsv) v = (float)(3.0 + uniform());
        for (size_t q = 0; q < vsh.size(); ++q) vsh[q] = vsv[q] * 1.04f;
        for (int l = 0; l <= M; ++l) depz[(size_t)l] = (float)(2.5 * l);
        // a slot's S on the model it was not run on is never read
        for (int k = 0; k < K; ++k)
            for (int l = 0; l < M; ++l)
                for (int c = 0; c < ncols; ++c) (k % 2 ? Sv : Sh)[((size_t)l * K + k) * ncols + c] = NAN;
        // column 1: a datum without a root, one without weight, one without an observation, their S not finite; column 2: no datum at all;
        // column 3: no Love datum
        for (int k = 0; k < K && k < 3; ++k) {
            if (k == 0) pv[(size_t)k * ncols + 1] = 0.0;
            if (k == 1) wt[(size_t)k * ncols + 1] = 0.0f;
            if (k == 2) obs[(size_t)k * ncols + 1] = 0.0f;
            for (int l = 0; l < M; ++l) { Sv[((size_t)l * K + k) * ncols + 1] = NAN; Sh[((size_t)l * K + k) * ncols + 1] = NAN; }
        }
        for (int k = 0; k < K; ++k) wt[(size_t)k * ncols + 2] = 0.0f;
        for (int k = 1; k < K; k += 2) wt[(size_t)k * ncols + 3] = 0.0f;
        hrr_resolution(M, K, ncols, nullptr, love, obs.data(), wt.data(), pv.data(), Sv.data(), Sh.data(), depz.data(), vsv.data(), vsh.data(), 0.3f, 0.1f, 0.2f,
                       measures.data(), pair.data(), leverage.data(), trace.data(), R.data(), nused.data(), flag.data(), T.data());
        for (int c = 0; c < ncols; ++c) {
            double hsum = 0.0;
            for (int k = 0; k < K; ++k) {
                const double h = leverage[(size_t)k * ncols + c];
                hsum += h;
                if (!(h >= 0.0 && h < 1.0)) ++bad;
            }
            for (int j = 0; j < n2; ++j) {
                const double var = measures[((size_t)5 * n2 + j) * ncols + c], m1 = measures[((size_t)1 * n2 + j) * ncols + c], mx = measures[((size_t)3 * n2 + j) * ncols + c];
                const int jt = j < M ? j + M : j - M;
                if (!(var >= 0.0) || !(m1 >= 0.0) || !(mx >= 0.0) || measures[(size_t)j * ncols + c] != R[((size_t)j * n2 + j) * ncols + c] ||
                    measures[((size_t)4 * n2 + j) * ncols + c] != R[((size_t)jt * n2 + j) * ncols + c]) ++bad;
            }
            for (int l = 0; l < M; ++l) {
                const double cov = pair[(size_t)l * ncols + c], vard = pair[((size_t)M + l) * ncols + c];
                const double vv = measures[((size_t)5 * n2 + l) * ncols + c], vh = measures[((size_t)5 * n2 + M + l) * ncols + c];
                if (!(vard >= 0.0) || !(std::fabs(cov) <= std::sqrt(vv * vh) * (1.0 + 1e-12)) || !(std::fabs(vard - (vv + vh - 2.0 * cov)) <= 1e-10 * (vv + vh))) ++bad;
            }
            const double tr = trace[c] + trace[ncols + c];
            if (flag[c] == kColumnOk && !(std::fabs(hsum - tr) <= 1e-10 * (1.0 + std::fabs(tr)))) ++bad;
            if (flag[c] != kColumnOk) {
                if (tr != 0.0 || hsum != 0.0) ++bad;
                for (int e = 0; e < n2 * n2; ++e) if (R[(size_t)e * ncols + c] != 0.0) ++bad;
                for (int e = 0; e < 6 * n2; ++e) if (measures[(size_t)e * ncols + c] != 0.0) ++bad;
                for (int e = 0; e < 2 * M; ++e) if (pair[(size_t)e * ncols + c] != 0.0) ++bad;
            }
            std::printf("M %2d K %2d column %d: nused %2d + %2d flag %d trace %.17g + %.17g sum of leverages %.17g\n", M, K, c, nused[c], nused[ncols + c], flag[c],
                        trace[c], trace[ncols + c], hsum);
        }
        if (flag[0] != kColumnOk || flag[2] != kColumnNoData || nused[2] != 0 || nused[ncols + 2] != 0) ++bad;
        if (flag[3] != kColumnOk || nused[ncols + 3] != 0 || nused[3] != (K + 1) / 2 || trace[ncols + 3] != 0.0) ++bad;
        if (K >= 3 && (nused[1] != (K + 1) / 2 - 2 || nused[ncols + 1] != K / 2 - 1)) ++bad;
        // column_solve on the rows of the expanded G: the same bits
        std::vector<float> o1(K), w1(K), v1(M), h1(M);
        std::vector<double> p1(K), Sv1((size_t)M * K), Sh1((size_t)M * K), T1((size_t)K * n2, 9.0);
        for (int k = 0; k < K; ++k) { o1[k] = obs[(size_t)k * ncols]; w1[k] = wt[(size_t)k * ncols]; p1[k] = pv[(size_t)k * ncols]; }
        for (int e = 0; e < M * K; ++e) { Sv1[(size_t)e] = Sv[(size_t)e * ncols]; Sh1[(size_t)e] = Sh[(size_t)e * ncols]; }
        for (int l = 0; l < M; ++l) { v1[l] = vsv[(size_t)l * ncols]; h1[l] = vsh[(size_t)l * ncols]; }
        if (hrr_rows_by_column_solve(M, K, love, o1.data(), w1.data(), p1.data(), Sv1.data(), Sh1.data(), v1.data(), h1.data(), 0.3f, 0.1f, 0.2f, T1.data()) != kColumnOk) ++bad;
        for (int e = 0; e < K * n2; ++e) if (T1[(size_t)e] != T[(size_t)e * ncols]) ++bad;
    }
    {   // an indefinite matrix of 2M = 2 unknowns: the second pivot is 1 - 4 < 0
        const double N[3] = { 1.0, 2.0, 1.0 }, G[2] = { 1.0, 0.5 };
        const float depz[1] = { 0.0f };
        double measures[12], pair[2], leverage[2], trace[2] = { 9.0, 9.0 }, R[4];
        for (double& v : measures) v = 9.0;
        for (double& v : pair) v = 9.0;
        for (double& v : leverage) v = 9.0;
        for (double& v : R) v = 9.0;
        const int f = hrr_finish(1, 2, 2ull, N, G, depz, measures, pair, leverage, trace, R);
        std::printf("indefinite: flag %d trace %g %g\n", f, trace[0], trace[1]);
        if (f != kColumnNotPositive || trace[0] != 0.0 || trace[1] != 0.0) ++bad;
        for (double v : measures) if (v != 0.0) ++bad;
        for (double v : pair) if (v != 0.0) ++bad;
        for (double v : leverage) if (v != 0.0) ++bad;
        for (double v : R) if (v != 0.0) ++bad;
    }
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
#endif
