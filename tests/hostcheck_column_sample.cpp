// TEST HARNESS (not product): the Monte-Carlo depth inversion of dsurftomo_amd/csrc/column_sample.h on a CPU behind a
// C interface, for tests/test_hostcheck_column_sample.py and tests/test_gpu_column_sample.py -- a loop over (chain, column) where the
// device has one thread each.  The caller owns every array and passes the header's SampleView, which tests/column_sample_ref.py mirrors
// field by field.  hcs_forward is a linear stand-in for the dispersion stage: pv = pv0 + A (v - v0), under which the posterior is
// Gaussian.  With -DHOSTCHECK_COLUMN_SAMPLE_MAIN the file is a stand-alone program that runs the sampler on made-up columns of every tested
// size and on the special cases (for a sanitizer build).
#include <cmath>
#include <cstdio>
#include <vector>

#include "../dsurftomo_amd/csrc/column_sample.h"

using namespace dsa;

extern "C" {

int hcs_view_bytes() { return (int)sizeof(SampleView); }

unsigned long long hcs_bits(unsigned long long seed, unsigned long long column, unsigned long long chain, unsigned long long sweep, unsigned long long draw)
{
    return sample_bits(seed, column, chain, sweep, draw);
}

double hcs_unit(unsigned long long k) { return sample_unit(k); }

// w: (n, 5) seed, column, chain, sweep, draw; k, u: (n)
void hcs_draws(long long n, const unsigned long long* w, unsigned long long* k, double* u)
{
    for (long long i = 0; i < n; ++i) {
        k[i] = sample_bits(w[5 * i], w[5 * i + 1], w[5 * i + 2], w[5 * i + 3], w[5 * i + 4]);
        u[i] = sample_unit(k[i]);
    }
}

void hcs_neglog(long long n, const unsigned long long* k, double* out)
{
    for (long long i = 0; i < n; ++i) out[i] = sample_neglog(k[i]);
}

double hcs_psi(int M, double lam2, const float* v) { return sample_psi(M, lam2, v, 1); }

void hcs_setup(const SampleView* S, int phase)
{
    for (int q = 0; q < S->C; ++q)
        for (long long c = 0; c < S->ncol; ++c) {
            if (phase == 0) sample_setup_models(*S, c, q);
            else sample_setup_state(*S, c, q);
        }
}

void hcs_propose(const SampleView* S, int sweep)
{
    for (int q = 0; q < S->C; ++q)
        for (long long c = 0; c < S->ncol; ++c) sample_propose(*S, c, q, sweep);
}

void hcs_accept(const SampleView* S, int sweep)
{
    for (int q = 0; q < S->C; ++q)
        for (long long c = 0; c < S->ncol; ++c) sample_accept(*S, c, q, sweep);
}

void hcs_finish(const SampleView* S, double* nodes, double* cols, int* counts)
{
    for (int l = 0; l < S->nz - 1; ++l)
        for (long long c = 0; c < S->ncol; ++c) sample_finish(*S, c, l, nodes, cols, counts);
}

// the linear forward function on every chain: pv (C, K, ncol) = pv0 (K, ncol) + A (K, M, ncol) (v - v0), the sum over the depths ascending
void hcs_forward(const SampleView* S, const double* pv0, const double* A, double* pv)
{
    const int M = S->nz - 1;
    for (int q = 0; q < S->C; ++q)
        for (int k = 0; k < S->K; ++k)
            for (long long c = 0; c < S->ncol; ++c) {
                double s = pv0[(long long)k * S->ncol + c];
                for (int l = 0; l < M; ++l)
                    s += A[((long long)k * M + l) * S->ncol + c] * ((double)S->v[sample_node(*S, c, q, l)] - (double)S->v0[(long long)l * S->ncol + c]);
                pv[((long long)q * S->K + k) * S->ncol + c] = s;
            }
}

// sweeps first .. first + n - 1 with the linear forward function in place of the dispersion runs; pv is the array S->pv points to
void hcs_linear(const SampleView* S, const double* pv0, const double* A, double* pv, int first, int n)
{
    for (int s = first; s < first + n; ++s) {
        hcs_propose(S, s);
        hcs_forward(S, pv0, A, pv);
        hcs_accept(S, s);
    }
}

}  // extern "C"

#ifdef HOSTCHECK_COLUMN_SAMPLE_MAIN
namespace {

// every array of a stage, and its view
struct Stage {
    std::vector<float> obs, wt, v0, v, best_v, pold;
    std::vector<double> pv, phi, psi, S1, S2, phisum, best_e, phi0, pv0, A, nodes, cols;
    std::vector<int> cnt, nkept, pnode, pmark, reseed, nused, flag, counts;
    std::vector<unsigned long long> used;
    SampleView S{};

    Stage(int nx, int ny, int M, int K, int C, int burn, bool weights)
    {
        const size_t ncol = (size_t)nx * ny, cc = ncol * C, nz = (size_t)M + 1;
        obs.assign(K * ncol, 0.0f); wt.assign(K * ncol, 1.0f); v0.assign(nz * ncol, 0.0f); v.assign(nz * cc, 0.0f); best_v.assign(M * cc, 0.0f); pold.assign(cc, 0.0f);
        pv.assign(K * cc, 0.0); phi.assign(cc, 0.0); psi.assign(cc, 0.0); S1.assign(M * cc, 0.0); S2.assign(M * cc, 0.0); phisum.assign(cc, 0.0); best_e.assign(cc, 0.0);
        phi0.assign(ncol, 0.0); pv0.assign(K * ncol, 0.0); A.assign((size_t)K * M * ncol, 0.0);
        nodes.assign(kSampleNodeFigures * M * ncol, 0.0); cols.assign(kSampleColumnFigures * ncol, 0.0);
        cnt.assign(kSampleCounters * cc, 0); nkept.assign(cc, 0); pnode.assign(cc, 0); pmark.assign(cc, 0); reseed.assign(cc, 0); nused.assign(ncol, 0); flag.assign(ncol, 0);
        counts.assign(kSampleColumnCounts * ncol, 0); used.assign(ncol, 0ull);
        unsigned long long x = 12345u + 977u * (unsigned)M + 31u * (unsigned)K + (unsigned)C;
        auto rnd = [&x]() { x = sample_mix(x + 0x9E3779B97F4A7C15ull); return sample_unit(x >> 11); };
        for (size_t i = 0; i < v0.size(); ++i) v0[i] = (float)(3.0 + rnd());
        for (size_t i = 0; i < pv0.size(); ++i) { pv0[i] = 3.0 + rnd(); obs[i] = (float)(pv0[i] * (1.0 + 0.02 * (2.0 * rnd() - 1.0))); wt[i] = (float)(30.0 + 40.0 * rnd()); }
        for (size_t i = 0; i < A.size(); ++i) A[i] = rnd() * (2.0 / M);
        S.nx = nx; S.ny = ny; S.nz = (int)nz; S.K = K; S.C = C; S.burn = burn; S.ncol = (long long)ncol; S.seed = 0x1234567890ull + (unsigned)M;
        S.lam2 = 4.0; S.step = 0.05; S.spread = 0.05; S.two_t = 2.0; S.width = 0.5f; S.minvel = 2.0f; S.maxvel = 4.5f;
        S.obs = obs.data(); S.wt = weights ? wt.data() : nullptr; S.v0 = v0.data(); S.pv = pv.data(); S.v = v.data(); S.phi = phi.data(); S.psi = psi.data();
        S.cnt = cnt.data(); S.S1 = S1.data(); S.S2 = S2.data(); S.phisum = phisum.data(); S.nkept = nkept.data(); S.best_e = best_e.data(); S.best_v = best_v.data();
        S.pnode = pnode.data(); S.pold = pold.data(); S.pmark = pmark.data(); S.reseed = reseed.data(); S.used = used.data(); S.nused = nused.data(); S.flag = flag.data();
        S.phi0 = phi0.data();
    }

    // the set-up, n sweeps (spoil: every seventh sweep chain 1 of column 5 loses a root and an unused datum of column 6 is NaN), the finish
    double run(int n, bool spoil)
    {
        const size_t ncol = (size_t)S.ncol;
        if (spoil && S.wt) {
            for (int k = 0; k < S.K; ++k) wt[(size_t)k * ncol + 9] = 0.0f;       // column 9: no datum
            wt[6] = 0.0f;                                                         // datum 0 of column 6: unused
        }
        hcs_setup(&S, 0);
        hcs_forward(&S, pv0.data(), A.data(), pv.data());
        if (spoil && S.C > 2) pv[((size_t)2 * S.K) * ncol + 5] = 0.0;                                                // chain 2 of column 5 starts without a root
        hcs_setup(&S, 1);
        for (int s = 1; s <= n; ++s) {
            hcs_propose(&S, s);
            hcs_forward(&S, pv0.data(), A.data(), pv.data());
            if (spoil && S.wt) for (int q = 0; q < S.C; ++q) pv[((size_t)q * S.K) * ncol + 6] = std::nan("");
            if (spoil && s % 7 == 0 && S.C > 1) pv[((size_t)1 * S.K + (S.K - 1)) * ncol + 5] = 0.0;
            hcs_accept(&S, s);
        }
        hcs_finish(&S, nodes.data(), cols.data(), counts.data());
        double sum = 0.0;
        for (double x : nodes) sum += x;
        for (double x : cols) sum += x;
        for (int x : counts) sum += x;
        return sum;
    }
};

}  // namespace

int main()
{
    const int sizes[4][2] = { { 1, 1 }, { 3, 6 }, { 7, 12 }, { 63, 60 } };
    int bad = 0;
    for (const auto& mk : sizes)
        for (int C : { 1, 5 })
            for (int spoil = 0; spoil < 2; ++spoil) {
                Stage st(4, 4, mk[0], mk[1], C, spoil ? 40 : 10, spoil != 0 || C == 5);
                const double sum = st.run(40, spoil != 0);
                std::printf("M %2d K %2d C %d spoil %d: sum %.17g\n", mk[0], mk[1], C, spoil, sum);
                if (!std::isfinite(sum)) ++bad;
            }
    std::vector<unsigned long long> ks = { 1ull, 2ull, (1ull << 52) - 1, (1ull << 52) + 1, (1ull << 53) - 1 };
    for (unsigned long long k : ks) {
        const double want = -std::log((double)k * 1.1102230246251565404e-16), got = sample_neglog(k);
        if (!(std::fabs(got - want) <= 1e-12 * std::fabs(want))) ++bad;
        std::printf("neglog(%llu) = %.17g (libm %.17g)\n", k, got, want);
    }
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
#endif
