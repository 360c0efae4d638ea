// TEST HARNESS (not product): the column step of dsurftomo_amd/csrc/column_system.h on a CPU behind a C interface, for
// tests/test_hostcheck_columns.py and tests/test_gpu_columns.py -- one lane of one, the barrier a no-op: the arithmetic the kernel shares out
// over a wavefront.  A library of its own so that the other harnesses stay as they are.  With -DHOSTCHECK_COLUMNS_MAIN the file is a
// stand-alone program that runs the step on made-up columns of every tested size and on the special cases (for a sanitizer build).
#include <cstdio>
#include <vector>

#include "../dsurftomo_amd/csrc/ray_core.h"
#include "../dsurftomo_amd/csrc/column_system.h"

using namespace dsa;

namespace {
struct NoBarrier { void operator()() const {} };
}

extern "C" {

int hcc_ltl(int M, int l, int lp) { return column_ltl(M, l, lp); }

int hcc_tri_row(int e) { return column_tri_row(e); }

// k_sen_combine's rule on n values: S = (svp a + srho r) + svs with the Brocher chain of the fp32 velocity v
void hcc_combine(long long n, const float* v, int shallow, const double* svs, const double* svp, const double* srho, double* S)
{
    for (long long i = 0; i < n; ++i) {
        float a, r;
        brocher_chain(v[i], shallow != 0, &a, &r);
        S[i] = (svp[i] * (double)a + srho[i] * (double)r) + svs[i];
    }
}

// The step of ncols columns that lie side by side the way the engine holds them: obs / wt (K, ncols) (wt may be null), pv (K, ncols),
// S (M, K, ncols), vels (M or more, ncols) stepped in place, dv (M, ncols), nused / chi2 / flag (ncols), delta (null, or (M, ncols): the
// fp64 solution before it is rounded and clipped, 0 where the column was left alone).  only: null, or one flag per column -- 0 leaves the
// column and its outputs alone (the kernel's outer ring).
void hcc_step(int M, int K, int ncols, const unsigned char* only, const float* obs, const float* wt, const double* pv, const double* S, float smooth, float damp,
              float dvmax, float minvel, float maxvel, float* vels, float* dv, int* nused, double* chi2, int* flag, double* delta)
{
    std::vector<double> work(column_work_doubles(M, K));
    const ColumnWork w = column_work(work.data(), M, K);
    for (int c = 0; c < ncols; ++c) {
        if (only && !only[c]) continue;
        ColumnIn in;
        in.M = M; in.K = K;
        in.obs = obs + c; in.obs_stride = ncols;
        in.wt = wt ? wt + c : nullptr; in.wt_stride = ncols;
        in.pv = pv + c; in.pv_stride = ncols;
        in.S = S + c; in.s_lstride = (long long)K * ncols; in.s_kstride = ncols;
        flag[c] = column_step(in, smooth, damp, dvmax, minvel, maxvel, w, vels + c, ncols, dv + c, ncols, &nused[c], &chi2[c], 0, 1, NoBarrier());
        if (delta) for (int l = 0; l < M; ++l) delta[(size_t)l * ncols + c] = flag[c] == kColumnOk ? w.b[l] : 0.0;
    }
}

// factor, solve and apply on a system given as it is: N the packed lower triangle (row by row), b the right-hand side; vels (M) in place,
// dv (M), d (M) the pivots reached.  Returns the flag.
int hcc_finish(int M, const double* N, const double* b, float dvmax, float minvel, float maxvel, float* vels, float* dv, double* d)
{
    std::vector<double> work(column_work_doubles(M, 1), 0.0);
    const ColumnWork w = column_work(work.data(), M, 1);
    for (int e = 0; e < column_tri_size(M); ++e) w.tri[e] = N[e];
    for (int l = 0; l < M; ++l) { w.b[l] = b[l]; w.d[l] = 0.0; }
    const int f = column_finish(M, w, dvmax, minvel, maxvel, vels, 1, dv, 1, 0, 1, NoBarrier());
    for (int l = 0; l < M; ++l) d[l] = w.d[l];
    return f;
}

}  // extern "C"

#ifdef HOSTCHECK_COLUMNS_MAIN
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
        std::vector<float> obs((size_t)K * ncols), wt((size_t)K * ncols), vels((size_t)(M + 1) * ncols), dv((size_t)M * ncols);
        std::vector<double> pv((size_t)K * ncols), S((size_t)M * K * ncols), chi2(ncols);
        std::vector<int> nused(ncols), flag(ncols);
        for (auto& v : obs) v = (float)(3.0 + uniform());
        for (auto& v : wt) v = (float)(0.5 + uniform());
        for (auto& v : pv) v = 3.0 + uniform();
        for (auto& v : S) v = uniform() / M;
        for (auto& v : vels) v = (float)(3.0 + uniform());
        // column 1: a datum without a root, one without weight, one without an observation, their S not finite; column 2: no datum at all
        for (int k = 0; k < K && k < 3; ++k) {
            if (k == 0) pv[(size_t)k * ncols + 1] = 0.0;
            if (k == 1) wt[(size_t)k * ncols + 1] = 0.0f;
            if (k == 2) obs[(size_t)k * ncols + 1] = 0.0f;
            for (int l = 0; l < M; ++l) S[((size_t)l * K + k) * ncols + 1] = NAN;
        }
        for (int k = 0; k < K; ++k) wt[(size_t)k * ncols + 2] = 0.0f;
        const std::vector<float> before = vels;
        hcc_step(M, K, ncols, nullptr, obs.data(), wt.data(), pv.data(), S.data(), 0.3f, 0.1f, 0.2f, 3.1f, 3.9f, vels.data(), dv.data(), nused.data(), chi2.data(), flag.data(), nullptr);
        for (int c = 0; c < ncols; ++c) {
            double sum = 0.0;
            for (int l = 0; l < M; ++l) {
                const float s = dv[(size_t)l * ncols + c], v = vels[(size_t)l * ncols + c];
                sum += s;
                if (!(s >= -0.2f && s <= 0.2f) || (flag[c] == 0 && !(v >= 3.1f && v <= 3.9f))) ++bad;
                if (flag[c] != 0 && v != before[(size_t)l * ncols + c]) ++bad;
            }
            if (vels[(size_t)M * ncols + c] != before[(size_t)M * ncols + c]) ++bad;
            std::printf("M %2d K %2d column %d: nused %2d flag %d chi2 %.17g sum of dv %.9g\n", M, K, c, nused[c], flag[c], chi2[c], sum);
        }
        if (flag[2] != kColumnNoData || nused[2] != 0 || (K >= 3 && nused[1] != K - 3)) ++bad;
    }
    {   // an indefinite matrix: the second pivot is 1 - 4 < 0
        const double N[3] = { 1.0, 2.0, 1.0 }, b[2] = { 1.0, 1.0 };
        float v[2] = { 3.0f, 3.5f }, dv[2] = { 9.0f, 9.0f };
        double d[2];
        const int f = hcc_finish(2, N, b, 0.5f, 1.0f, 5.0f, v, dv, d);
        std::printf("indefinite: flag %d pivots %g %g\n", f, d[0], d[1]);
        if (f != kColumnNotPositive || v[0] != 3.0f || v[1] != 3.5f || dv[0] != 0.0f || dv[1] != 0.0f) ++bad;
    }
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
#endif
