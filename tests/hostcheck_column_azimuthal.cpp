// TEST HARNESS (not product): the depth inversion of the maps' 2 psi terms of dsurftomo_amd/csrc/column_azimuthal.h on a CPU behind a C
// interface, for tests/test_hostcheck_column_azimuthal.py and tests/test_gpu_column_azimuthal.py -- one lane of one, the barrier a no-op: the
// arithmetic the kernel shares out over a wavefront.  A library of its own so that the other harnesses stay as they are.  With
// -DHOSTCHECK_COLUMN_AZIMUTHAL_MAIN the file is a stand-alone program that runs the header on made-up columns of every tested size and on
// the special cases and checks the laws itself (for a sanitizer build).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../dsurftomo_amd/csrc/column_azimuthal.h"

using namespace dsa;

namespace {
struct NoBarrier { void operator()() const {} };
}

extern "C" {

long long hca_doubles(int M, int K) { return (long long)column_azimuthal_doubles(M, K); }

// ncols columns that lie side by side the way the engine holds them: obs / wt / a1 / a2 (K, ncols) (wt: the effective weights, 0 at a Love
// slot; may be null), pv (K, ncols), Z (M, K, ncols), depz (M or more); g (2, M, ncols), measures (4, M, ncols), leverage (K, ncols), chi2
// (4, ncols), nused / flag (ncols), T (null, or (K, M, ncols): the generalised inverse, 0 where the column is flagged).  only: null, or one
// flag per column -- 0 leaves the column and its outputs alone (the kernel's outer ring).
void hca_azimuthal(int M, int K, int ncols, const unsigned char* only, const float* obs, const float* wt, const double* pv, const double* Z, const float* a1,
                   const float* a2, const float* depz, float smooth, float damp, double* g, double* measures, double* leverage, double* chi2, int* nused, int* flag,
                   double* T)
{
    std::vector<double> work(column_azimuthal_doubles(M, K));
    const ColumnAziWork z = column_azimuthal_work(work.data(), M, K);
    const int Kp = column_resolution_kpad(K);
    for (int c = 0; c < ncols; ++c) {
        if (only && !only[c]) continue;
        ColumnAziIn in;
        in.col.M = M; in.col.K = K;
        in.col.obs = obs + c; in.col.obs_stride = ncols;
        in.col.wt = wt ? wt + c : nullptr; in.col.wt_stride = ncols;
        in.col.pv = pv + c; in.col.pv_stride = ncols;
        in.col.S = Z + c; in.col.s_lstride = (long long)K * ncols; in.col.s_kstride = ncols;
        in.a1 = a1 + c; in.a2 = a2 + c; in.a_stride = ncols;
        ColumnAziOut out;
        out.g = g + c; out.g_qstride = (long long)M * ncols; out.g_lstride = ncols;
        out.chi2 = chi2 + c; out.chi2_stride = ncols;
        out.res.measures = measures + c; out.res.m_qstride = (long long)M * ncols; out.res.m_jstride = ncols;
        out.res.leverage = leverage + c; out.res.h_stride = ncols;
        out.res.R = nullptr; out.res.r_stride = 0;
        flag[c] = column_azimuthal(in, depz, smooth, damp, z, out, &nused[c], 0, 1, NoBarrier());
        if (T)
            for (int k = 0; k < K; ++k)
                for (int i = 0; i < M; ++i) T[((size_t)k * M + i) * ncols + c] = flag[c] == kColumnOk ? z.T[i * Kp + k] : 0.0;
    }
}

// the right-hand sides and the finish on a system given as it is: N the packed lower triangle (row by row), G (K, M) with every datum used
// at weight 1, a1 / a2 (K); g (2, M), measures (4, M), leverage (K), chi2 (4).  Returns the flag.
int hca_finish(int M, int K, const double* N, const double* G, const float* a1, const float* a2, const float* depz, double* g, double* measures, double* leverage,
               double* chi2)
{
    std::vector<double> work(column_azimuthal_doubles(M, K), 0.0);
    const ColumnAziWork z = column_azimuthal_work(work.data(), M, K);
    for (int e = 0; e < column_tri_size(M); ++e) z.w.tri[e] = N[e];
    for (int e = 0; e < K * M; ++e) z.w.G[e] = G[e];
    for (int k = 0; k < K; ++k) z.w.a[k] = 1.0;
    ColumnAziOut out;
    out.g = g; out.g_qstride = M; out.g_lstride = 1;
    out.chi2 = chi2; out.chi2_stride = 1;
    out.res.measures = measures; out.res.m_qstride = M; out.res.m_jstride = 1;
    out.res.leverage = leverage; out.res.h_stride = 1;
    out.res.R = nullptr; out.res.r_stride = 0;
    double before[2];
    column_azimuthal_rhs(M, K, a1, a2, 1, z, before, 0, 1, NoBarrier());
    return column_azimuthal_finish(M, K, depz, z, before, out, 0, 1, NoBarrier());
}

}  // extern "C"

#ifdef HOSTCHECK_COLUMN_AZIMUTHAL_MAIN
namespace {
unsigned long long g_state = 88172645463325252ull;
double uniform()          // xorshift64, in [0, 1)
{
    g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
    return (double)(g_state >> 11) / 9007199254740992.0;
}

struct Case {
    int M, K, ncols;
    std::vector<float> obs, wt, a1, a2, depz;
    std::vector<double> pv, Z;
};

struct Result {
    std::vector<double> g, measures, leverage, chi2, T;
    std::vector<int> nused, flag;
};

Result solve(const Case& q, float smooth = 0.3f, float damp = 0.1f)
{
    Result r;
    const size_t n = (size_t)q.ncols;
    r.g.assign(2 * q.M * n, 9.0); r.measures.assign(4 * q.M * n, 9.0); r.leverage.assign(q.K * n, 9.0); r.chi2.assign(4 * n, 9.0); r.T.assign((size_t)q.K * q.M * n, 9.0);
    r.nused.assign(n, -1); r.flag.assign(n, -1);
    hca_azimuthal(q.M, q.K, q.ncols, nullptr, q.obs.data(), q.wt.data(), q.pv.data(), q.Z.data(), q.a1.data(), q.a2.data(), q.depz.data(), smooth, damp, r.g.data(),
                  r.measures.data(), r.leverage.data(), r.chi2.data(), r.nused.data(), r.flag.data(), r.T.data());
    return r;
}

bool same(const std::vector<double>& a, const std::vector<double>& b) { return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0; }
}

int main()
{
    const int sizes[][2] = { { 1, 1 }, { 2, 3 }, { 7, 12 }, { 63, 60 } };
    const int ncols = 4;
    int bad = 0;
    for (const auto& mk : sizes) {
        Case q;
        q.M = mk[0]; q.K = mk[1]; q.ncols = ncols;
        const int M = q.M, K = q.K;
        q.obs.resize((size_t)K * ncols); q.wt.resize((size_t)K * ncols); q.a1.resize((size_t)K * ncols); q.a2.resize((size_t)K * ncols); q.depz.resize((size_t)M + 1);
        q.pv.resize((size_t)K * ncols); q.Z.resize((size_t)M * K * ncols);
        for (auto& v : q.obs) v = (float)(3.0 + uniform());
        for (auto& v : q.wt) v = (float)(0.5 + uniform());
        for (auto& v : q.pv) v = 3.0 + uniform();
        for (auto& v : q.Z) v = uniform() * 2.0 / M;
        for (auto& v : q.a1) v = (float)(0.06 * (uniform() - 0.5));
        for (auto& v : q.a2) v = (float)(0.06 * (uniform() - 0.5));
        for (int l = 0; l <= M; ++l) q.depz[(size_t)l] = (float)(2.5 * l);
        // column 1: a datum without a root, one without weight (a Love slot is one), one without an observation, their Z and A not finite;
        // column 2: no datum at all; column 3: A2 = 0
        for (int k = 0; k < K && k < 3; ++k) {
            if (k == 0) q.pv[(size_t)k * ncols + 1] = 0.0;
            if (k == 1) q.wt[(size_t)k * ncols + 1] = 0.0f;
            if (k == 2) q.obs[(size_t)k * ncols + 1] = 0.0f;
            for (int l = 0; l < M; ++l) q.Z[((size_t)l * K + k) * ncols + 1] = NAN;
            q.a1[(size_t)k * ncols + 1] = NAN; q.a2[(size_t)k * ncols + 1] = NAN;
        }
        for (int k = 0; k < K; ++k) { q.wt[(size_t)k * ncols + 2] = 0.0f; q.a2[(size_t)k * ncols + 3] = 0.0f; }
        const Result r = solve(q);
        for (int c = 0; c < ncols; ++c) {
            for (int e = 0; e < 2 * M; ++e) if (!std::isfinite(r.g[(size_t)e * ncols + c])) ++bad;
            for (int e = 0; e < 4; ++e) if (!(r.chi2[(size_t)e * ncols + c] >= 0.0)) ++bad;
            if (!(r.chi2[(size_t)2 * ncols + c] <= r.chi2[(size_t)0 * ncols + c]) || !(r.chi2[(size_t)3 * ncols + c] <= r.chi2[(size_t)1 * ncols + c])) ++bad;
            if (r.flag[c] != kColumnOk) {
                for (int e = 0; e < 2 * M; ++e) if (r.g[(size_t)e * ncols + c] != 0.0) ++bad;
                for (int e = 0; e < 4 * M; ++e) if (r.measures[(size_t)e * ncols + c] != 0.0) ++bad;
                for (int e = 0; e < K; ++e) if (r.leverage[(size_t)e * ncols + c] != 0.0) ++bad;
                for (int e = 0; e < 4; ++e) if (r.chi2[(size_t)e * ncols + c] != 0.0) ++bad;
            }
            // gc = sum_k T_kj rhoc_k: the other route through the same linear algebra
            double worst = 0.0, scale = 0.0;
            for (int j = 0; j < M && r.flag[c] == kColumnOk; ++j) {
                double s = 0.0;
                for (int k = 0; k < K; ++k) {
                    const double t = r.T[((size_t)k * M + j) * ncols + c];
                    if (t != 0.0) s += t * ((double)q.wt[(size_t)k * ncols + c] * (double)q.a1[(size_t)k * ncols + c]);
                }
                worst = std::fmax(worst, std::fabs(s - r.g[(size_t)j * ncols + c]));
                scale = std::fmax(scale, std::fabs(s));
            }
            if (!(worst <= 1e-11 * scale)) ++bad;
            std::printf("M %2d K %2d column %d: nused %2d flag %d chi2 %.6g %.6g -> %.6g %.6g, T route differs by %.3g of %.3g\n", M, K, c, r.nused[c], r.flag[c],
                        r.chi2[c], r.chi2[(size_t)ncols + c], r.chi2[(size_t)2 * ncols + c], r.chi2[(size_t)3 * ncols + c], worst, scale);
        }
        if (r.flag[0] != kColumnOk || r.flag[2] != kColumnNoData || r.nused[2] != 0 || (K >= 3 && r.nused[1] != K - 3)) ++bad;
        for (int l = 0; l < M; ++l) if (r.g[((size_t)M + l) * ncols + 3] != 0.0) ++bad;          // A2 = 0: gs = 0.0
        if (r.chi2[(size_t)1 * ncols + 3] != 0.0 || r.chi2[(size_t)3 * ncols + 3] != 0.0) ++bad;
        // swapping A1 and A2 swaps gc and gs; negating A negates g; the measures do not see A
        Case sw = q;
        sw.a1 = q.a2; sw.a2 = q.a1;
        const Result rs = solve(sw);
        Case ng = q;
        for (auto& v : ng.a1) v = -v;
        for (auto& v : ng.a2) v = -v;
        const Result rn = solve(ng);
        for (int c = 0; c < ncols; ++c)
            for (int l = 0; l < M; ++l) {
                const double gc = r.g[(size_t)l * ncols + c], gs = r.g[((size_t)M + l) * ncols + c];
                if (rs.g[(size_t)l * ncols + c] != gs || rs.g[((size_t)M + l) * ncols + c] != gc) ++bad;
                if (rn.g[(size_t)l * ncols + c] != -gc || rn.g[((size_t)M + l) * ncols + c] != -gs) ++bad;
            }
        if (!same(rs.measures, r.measures) || !same(rs.leverage, r.leverage) || !same(rn.measures, r.measures) || !same(rn.leverage, r.leverage) || !same(rn.chi2, r.chi2)) ++bad;
    }
    {   // an indefinite matrix: the second pivot is 1 - 4 < 0
        const double N[3] = { 1.0, 2.0, 1.0 }, G[4] = { 1.0, 0.5, 0.25, 1.0 };
        const float depz[2] = { 0.0f, 2.0f }, a1[2] = { 0.01f, -0.02f }, a2[2] = { 0.03f, 0.01f };
        double g[4], measures[8], leverage[2], chi2[4];
        for (double& v : g) v = 9.0;
        for (double& v : measures) v = 9.0;
        for (double& v : leverage) v = 9.0;
        for (double& v : chi2) v = 9.0;
        const int f = hca_finish(2, 2, N, G, a1, a2, depz, g, measures, leverage, chi2);
        std::printf("indefinite: flag %d\n", f);
        if (f != kColumnNotPositive) ++bad;
        for (double v : g) if (v != 0.0) ++bad;
        for (double v : measures) if (v != 0.0) ++bad;
        for (double v : leverage) if (v != 0.0) ++bad;
        for (double v : chi2) if (v != 0.0) ++bad;
    }
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
#endif
