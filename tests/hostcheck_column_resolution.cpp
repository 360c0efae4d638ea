// TEST HARNESS (not product): the depth resolution of dsurftomo_amd/csrc/column_resolution.h on a CPU behind a C interface, for
// tests/test_hostcheck_column_resolution.py and tests/test_gpu_column_resolution.py -- one lane of one, the barrier a no-op: the arithmetic
// the kernel shares out over a wavefront.  A library of its own so that the other harnesses stay as they are.  With
// -DHOSTCHECK_COLUMN_RESOLUTION_MAIN the file is a stand-alone program that runs the header on made-up columns of every tested size and on
// the special cases (for a sanitizer build).
#include <cmath>
#include <cstdio>
#include <vector>

#include "../dsurftomo_amd/csrc/column_resolution.h"

using namespace dsa;

namespace {
struct NoBarrier { void operator()() const {} };

ColumnIn column_of(int M, int K, int ncols, int c, const float* obs, const float* wt, const double* pv, const double* S)
{
    ColumnIn in;
    in.M = M; in.K = K;
    in.obs = obs + c; in.obs_stride = ncols;
    in.wt = wt ? wt + c : nullptr; in.wt_stride = ncols;
    in.pv = pv + c; in.pv_stride = ncols;
    in.S = S + c; in.s_lstride = (long long)K * ncols; in.s_kstride = ncols;
    return in;
}
}

extern "C" {

long long hcr_doubles(int M, int K) { return (long long)column_resolution_doubles(M, K); }

// The resolution of ncols columns that lie side by side the way the engine holds them: obs / wt (K, ncols) (wt may be null), pv (K, ncols),
// S (M, K, ncols), depz (M or more); measures (4, M, ncols), leverage (K, ncols), trace / nused / flag (ncols), R (null, or (M, M, ncols)),
// T (null, or (K, M, ncols): the generalised inverse, 0 where the column is flagged).  only: null, or one flag per column -- 0 leaves the
// column and its outputs alone (the kernel's outer ring).
void hcr_resolution(int M, int K, int ncols, const unsigned char* only, const float* obs, const float* wt, const double* pv, const double* S, const float* depz,
                    float smooth, float damp, double* measures, double* leverage, double* trace, double* R, int* nused, int* flag, double* T)
{
    std::vector<double> work(column_resolution_doubles(M, K));
    const ColumnWork w = column_work(work.data(), M, K);
    double* t = column_resolution_t(work.data(), M, K);
    const int Kp = column_resolution_kpad(K);
    for (int c = 0; c < ncols; ++c) {
        if (only && !only[c]) continue;
        const ColumnIn in = column_of(M, K, ncols, c, obs, wt, pv, S);
        ColumnResOut out;
        out.measures = measures + c; out.m_qstride = (long long)M * ncols; out.m_jstride = ncols;
        out.leverage = leverage + c; out.h_stride = ncols;
        out.R = R ? R + c : nullptr; out.r_stride = ncols;
        flag[c] = column_resolution(in, depz, smooth, damp, w, t, out, &trace[c], &nused[c], 0, 1, NoBarrier());
        if (T)
            for (int k = 0; k < K; ++k)
                for (int i = 0; i < M; ++i) T[((size_t)k * M + i) * ncols + c] = flag[c] == kColumnOk ? t[i * Kp + k] : 0.0;
    }
}

// one column: assemble and factor as the resolution does, then column_solve (column_system.h, the step's) on every row of G in turn.
// T (K, M): the solutions, rows of unused data 0.  Returns the flag (T untouched unless 0).
int hcr_rows_by_column_solve(int M, int K, const float* obs, const float* wt, const double* pv, const double* S, float smooth, float damp, double* T)
{
    std::vector<double> work(column_work_doubles(M, K));
    const ColumnWork w = column_work(work.data(), M, K);
    const ColumnIn in = column_of(M, K, 1, 0, obs, wt, pv, S);
    double chi2 = 0.0;
    if (column_assemble(in, (double)smooth * (double)smooth, (double)damp * (double)damp, w, &chi2, 0, 1, NoBarrier()) == 0) return kColumnNoData;
    const int f = column_factor(M, w, 0, 1, NoBarrier());
    if (f != kColumnOk) return f;
    for (int k = 0; k < K; ++k) {
        for (int i = 0; i < M; ++i) w.b[i] = w.G[k * M + i];
        if (w.a[k] > 0.0) column_solve(M, w, 0, 1, NoBarrier());
        for (int i = 0; i < M; ++i) T[(size_t)k * M + i] = w.a[k] > 0.0 ? w.b[i] : 0.0;
    }
    return f;
}

// factor, T and the reductions on a system given as it is: N the packed lower triangle (row by row), G (K, M) with every datum used;
// measures (4, M), leverage (K), trace (1), R (null or (M, M)).  Returns the flag.
int hcr_finish(int M, int K, const double* N, const double* G, const float* depz, double* measures, double* leverage, double* trace, double* R)
{
    std::vector<double> work(column_resolution_doubles(M, K), 0.0);
    const ColumnWork w = column_work(work.data(), M, K);
    for (int e = 0; e < column_tri_size(M); ++e) w.tri[e] = N[e];
    for (int e = 0; e < K * M; ++e) w.G[e] = G[e];
    for (int k = 0; k < K; ++k) w.a[k] = 1.0;
    ColumnResOut out;
    out.measures = measures; out.m_qstride = M; out.m_jstride = 1;
    out.leverage = leverage; out.h_stride = 1;
    out.R = R; out.r_stride = 1;
    return column_resolution_finish(M, K, depz, w, column_resolution_t(work.data(), M, K), out, trace, 0, 1, NoBarrier());
}

}  // extern "C"

#ifdef HOSTCHECK_COLUMN_RESOLUTION_MAIN
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
    const int sizes[][2] = { { 1, 1 }, { 2, 3 }, { 7, 12 }, { 63, 60 } };
    const int ncols = 3;
    int bad = 0;
    for (const auto& mk : sizes) {
        const int M = mk[0], K = mk[1];
        std::vector<float> obs((size_t)K * ncols), wt((size_t)K * ncols), depz((size_t)M + 1);
        std::vector<double> pv((size_t)K * ncols), S((size_t)M * K * ncols), measures((size_t)4 * M * ncols, 9.0), leverage((size_t)K * ncols, 9.0), trace(ncols, 9.0),
            R((size_t)M * M * ncols, 9.0), T((size_t)K * M * ncols, 9.0);
        std::vector<int> nused(ncols), flag(ncols);
        for (auto& v : obs) v = (float)(3.0 + uniform());
        for (auto& v : wt) v = (float)(0.5 + uniform());
        for (auto& v : pv) v = 3.0 + uniform();
        for (auto& v : S) v = uniform() * 2.0 / M;
        for (int l = 0; l <= M; ++l) depz[(size_t)l] = (float)(2.5 * l);
        // column 1: a datum without a root, one without weight, one without an observation, their S not finite; column 2: no datum at all
        for (int k = 0; k < K && k < 3; ++k) {
            if (k == 0) pv[(size_t)k * ncols + 1] = 0.0;
            if (k == 1) wt[(size_t)k * ncols + 1] = 0.0f;
            if (k == 2) obs[(size_t)k * ncols + 1] = 0.0f;
            for (int l = 0; l < M; ++l) S[((size_t)l * K + k) * ncols + 1] = NAN;
        }
        for (int k = 0; k < K; ++k) wt[(size_t)k * ncols + 2] = 0.0f;
        hcr_resolution(M, K, ncols, nullptr, obs.data(), wt.data(), pv.data(), S.data(), depz.data(), 0.3f, 0.1f, measures.data(), leverage.data(), trace.data(),
                       R.data(), nused.data(), flag.data(), T.data());
        for (int c = 0; c < ncols; ++c) {
            double hsum = 0.0;
            for (int k = 0; k < K; ++k) {
                const double h = leverage[(size_t)k * ncols + c];
                hsum += h;
                if (!(h >= 0.0 && h < 1.0)) ++bad;
            }
            for (int j = 0; j < M; ++j) {
                const double var = measures[((size_t)3 * M + j) * ncols + c], m1 = measures[((size_t)1 * M + j) * ncols + c];
                if (!(var >= 0.0) || !(m1 >= 0.0) || measures[(size_t)j * ncols + c] != R[((size_t)j * M + j) * ncols + c]) ++bad;
            }
            if (flag[c] == kColumnOk && !(std::fabs(hsum - trace[c]) <= 1e-10 * (1.0 + std::fabs(trace[c])))) ++bad;
            if (flag[c] != kColumnOk) {
                if (trace[c] != 0.0 || hsum != 0.0) ++bad;
                for (int e = 0; e < M * M; ++e) if (R[(size_t)e * ncols + c] != 0.0) ++bad;
                for (int e = 0; e < 4 * M; ++e) if (measures[(size_t)e * ncols + c] != 0.0) ++bad;
            }
            std::printf("M %2d K %2d column %d: nused %2d flag %d trace %.17g sum of leverages %.17g\n", M, K, c, nused[c], flag[c], trace[c], hsum);
        }
        if (flag[0] != kColumnOk || flag[2] != kColumnNoData || nused[2] != 0 || (K >= 3 && nused[1] != K - 3)) ++bad;
        // column_solve on the rows of G: the same bits
        std::vector<float> o1(K), w1(K);
        std::vector<double> p1(K), S1((size_t)M * K), T1((size_t)K * M, 9.0);
        for (int k = 0; k < K; ++k) { o1[k] = obs[(size_t)k * ncols]; w1[k] = wt[(size_t)k * ncols]; p1[k] = pv[(size_t)k * ncols]; }
        for (int e = 0; e < M * K; ++e) S1[(size_t)e] = S[(size_t)e * ncols];
        if (hcr_rows_by_column_solve(M, K, o1.data(), w1.data(), p1.data(), S1.data(), 0.3f, 0.1f, T1.data()) != kColumnOk) ++bad;
        for (int e = 0; e < K * M; ++e) if (T1[(size_t)e] != T[(size_t)e * ncols]) ++bad;
    }
    {   // an indefinite matrix: the second pivot is 1 - 4 < 0
        const double N[3] = { 1.0, 2.0, 1.0 }, G[4] = { 1.0, 0.5, 0.25, 1.0 };
        const float depz[2] = { 0.0f, 2.0f };
        double measures[8], leverage[2], trace = 9.0, R[4];
        for (double& v : measures) v = 9.0;
        for (double& v : leverage) v = 9.0;
        for (double& v : R) v = 9.0;
        const int f = hcr_finish(2, 2, N, G, depz, measures, leverage, &trace, R);
        std::printf("indefinite: flag %d trace %g\n", f, trace);
        if (f != kColumnNotPositive || trace != 0.0) ++bad;
        for (double v : measures) if (v != 0.0) ++bad;
        for (double v : leverage) if (v != 0.0) ++bad;
        for (double v : R) if (v != 0.0) ++bad;
    }
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
#endif
