// TEST HARNESS (not product): the Monte-Carlo radial depth inversion of dsurftomo_amd/csrc/column_sample_radial.h on a
// CPU behind a C interface, for tests/test_hostcheck_column_sample_radial.py and tests/test_gpu_column_sample_radial.py -- a loop over (chain,
// column) where the device has one thread each.  The caller owns every array and passes the header's SampleRadialView, which
// tests/column_sample_radial_ref.py mirrors field by field.  hcr_forward is a linear stand-in for the dispersion stage: pv = pv0 + A (v -
// v0), v the chain's Vsh and v0 its start at a Love slot, Vsv elsewhere, under which the posterior is Gaussian.  With
// -DHOSTCHECK_COLUMN_SAMPLE_RADIAL_MAIN the file is a stand-alone program that runs the sampler on made-up columns of every tested size and on
// the special cases (for a sanitizer build).
#include <cmath>
#include <cstdio>
#include <vector>

#include "../dsurftomo_amd/csrc/column_sample_radial.h"

using namespace dsa;

extern "C" {

int hcr_view_bytes() { return (int)sizeof(SampleRadialView); }

void hcr_setup(const SampleRadialView* S, int phase)
{
    for (int q = 0; q < S->C; ++q)
        for (long long c = 0; c < S->ncol; ++c) {
            if (phase == 0) sample_radial_setup_models(*S, c, q);
            else sample_radial_setup_state(*S, c, q);
        }
}

void hcr_propose(const SampleRadialView* S, int sweep)
{
    for (int q = 0; q < S->C; ++q)
        for (long long c = 0; c < S->ncol; ++c) sample_radial_propose(*S, c, q, sweep);
}

void hcr_accept(const SampleRadialView* S, int sweep)
{
    for (int q = 0; q < S->C; ++q)
        for (long long c = 0; c < S->ncol; ++c) sample_radial_accept(*S, c, q, sweep);
}

void hcr_finish(const SampleRadialView* S, double* nodes, double* cols, int* counts)
{
    for (int l = 0; l < S->nz - 1; ++l)
        for (long long c = 0; c < S->ncol; ++c) sample_radial_finish(*S, c, l, nodes, cols, counts);
}

// the linear forward function on every chain: pv (C, K, ncol) = pv0 (K, ncol) + A (K, M, ncol) (v - v0), the sum over the depths ascending
void hcr_forward(const SampleRadialView* S, const double* pv0, const double* A, double* pv)
{
    const int M = S->nz - 1;
    for (int q = 0; q < S->C; ++q)
        for (int k = 0; k < S->K; ++k) {
            const bool lv = ((S->love >> k) & 1ull) != 0ull;
            const float* v = lv ? S->vh : S->vv;
            const float* v0 = lv ? S->v0h : S->v0v;
            for (long long c = 0; c < S->ncol; ++c) {
                double s = pv0[(long long)k * S->ncol + c];
                for (int l = 0; l < M; ++l)
                    s += A[((long long)k * M + l) * S->ncol + c] * ((double)v[sample_radial_node(*S, c, q, l)] - (double)v0[(long long)l * S->ncol + c]);
                pv[((long long)q * S->K + k) * S->ncol + c] = s;
            }
        }
}

// sweeps first .. first + n - 1 with the linear forward function in place of the dispersion runs; pv is the array S->pv points to
void hcr_linear(const SampleRadialView* S, const double* pv0, const double* A, double* pv, int first, int n)
{
    for (int s = first; s < first + n; ++s) {
        hcr_propose(S, s);
        hcr_forward(S, pv0, A, pv);
        hcr_accept(S, s);
    }
}

}  // extern "C"

#ifdef HOSTCHECK_COLUMN_SAMPLE_RADIAL_MAIN
namespace {

// every array of a stage, and its view
struct Stage {
    std::vector<float> obs, wt, v0v, v0h, vv, vh, best_vv, best_vh, pold_v, pold_h;
    std::vector<double> pv, phi, psi, S1v, S2v, S1h, S2h, Pvh, X1, X2, phisum, best_e, phi0, pv0, A, nodes, cols;
    std::vector<int> cnt, kcnt, npos, nkept, pnode, pmark, reseed, nused_r, nused_l, flag, counts;
    std::vector<unsigned long long> used;
    SampleRadialView S{};

    Stage(int nx, int ny, int M, int K, int C, int burn, bool weights, int pairs)
    {
        const size_t ncol = (size_t)nx * ny, cc = ncol * C, nz = (size_t)M + 1;
        obs.assign(K * ncol, 0.0f); wt.assign(K * ncol, 1.0f); v0v.assign(nz * ncol, 0.0f); v0h.assign(nz * ncol, 0.0f); vv.assign(nz * cc, 0.0f); vh.assign(nz * cc, 0.0f);
        best_vv.assign(M * cc, 0.0f); best_vh.assign(M * cc, 0.0f); pold_v.assign(cc, 0.0f); pold_h.assign(cc, 0.0f);
        pv.assign(K * cc, 0.0); phi.assign(cc, 0.0); psi.assign(cc, 0.0);
        for (std::vector<double>* a : { &S1v, &S2v, &S1h, &S2h, &Pvh, &X1, &X2 }) a->assign(M * cc, 0.0);
        phisum.assign(cc, 0.0); best_e.assign(cc, 0.0); phi0.assign(ncol, 0.0); pv0.assign(K * ncol, 0.0); A.assign((size_t)K * M * ncol, 0.0);
        nodes.assign(kSrNodeFigures * M * ncol, 0.0); cols.assign(kSampleColumnFigures * ncol, 0.0);
        cnt.assign(kSampleCounters * cc, 0); kcnt.assign(kSampleKindCounters * cc, 0); npos.assign(M * cc, 0); nkept.assign(cc, 0); pnode.assign(cc, 0);
        pmark.assign(cc, 0); reseed.assign(cc, 0); nused_r.assign(ncol, 0); nused_l.assign(ncol, 0); flag.assign(ncol, 0);
        counts.assign(kSrColumnCounts * ncol, 0); used.assign(ncol, 0ull);
        unsigned long long x = 54321u + 977u * (unsigned)M + 31u * (unsigned)K + (unsigned)C;
        auto rnd = [&x]() { x = sample_mix(x + 0x9E3779B97F4A7C15ull); return sample_unit(x >> 11); };
        for (size_t i = 0; i < v0v.size(); ++i) { v0v[i] = (float)(3.0 + rnd()); v0h[i] = v0v[i] * (float)(1.0 + 0.04 * rnd()); }
        for (size_t i = 0; i < pv0.size(); ++i) { pv0[i] = 3.0 + rnd(); obs[i] = (float)(pv0[i] * (1.0 + 0.02 * (2.0 * rnd() - 1.0))); wt[i] = (float)(30.0 + 40.0 * rnd()); }
        for (size_t i = 0; i < A.size(); ++i) A[i] = rnd() * (2.0 / M);
        S.nx = nx; S.ny = ny; S.nz = (int)nz; S.K = K; S.C = C; S.burn = burn; S.pairs = pairs; S.ncol = (long long)ncol; S.seed = 0x1234567890ull + (unsigned)M;
        S.love = 0xAAAAAAAAAAAAAAAAull;                                      // the odd slots are Love slots
        S.lam2 = 4.0; S.gam2 = 9.0; S.step = 0.05; S.spread = 0.05; S.two_t = 2.0; S.width = 0.5f; S.minvel = 2.0f; S.maxvel = 4.5f;
        S.obs = obs.data(); S.wt = weights ? wt.data() : nullptr; S.v0v = v0v.data(); S.v0h = v0h.data(); S.pv = pv.data(); S.vv = vv.data(); S.vh = vh.data();
        S.phi = phi.data(); S.psi = psi.data(); S.cnt = cnt.data(); S.kcnt = kcnt.data(); S.S1v = S1v.data(); S.S2v = S2v.data(); S.S1h = S1h.data(); S.S2h = S2h.data();
        S.Pvh = Pvh.data(); S.X1 = X1.data(); S.X2 = X2.data(); S.npos = npos.data(); S.phisum = phisum.data(); S.nkept = nkept.data(); S.best_e = best_e.data();
        S.best_vv = best_vv.data(); S.best_vh = best_vh.data(); S.pnode = pnode.data(); S.pold_v = pold_v.data(); S.pold_h = pold_h.data(); S.pmark = pmark.data();
        S.reseed = reseed.data(); S.used = used.data(); S.nused_r = nused_r.data(); S.nused_l = nused_l.data(); S.flag = flag.data(); S.phi0 = phi0.data();
    }

    // the set-up, n sweeps (spoil: column 9 without a datum, column 10 without a Rayleigh datum, an unused datum of column 6 is NaN, chain 2 of
    // column 5 starts without a root, every seventh sweep chain 1 of column 5 loses a root), the finish
    double run(int n, bool spoil)
    {
        const size_t ncol = (size_t)S.ncol;
        if (spoil && S.wt) {
            for (int k = 0; k < S.K; ++k) wt[(size_t)k * ncol + 9] = 0.0f;
            for (int k = 0; k < S.K; k += 2) wt[(size_t)k * ncol + 10] = 0.0f;
            wt[6] = 0.0f;
        }
        hcr_setup(&S, 0);
        hcr_forward(&S, pv0.data(), A.data(), pv.data());
        if (spoil && S.C > 2) pv[((size_t)2 * S.K) * ncol + 5] = 0.0;
        hcr_setup(&S, 1);
        for (int s = 1; s <= n; ++s) {
            hcr_propose(&S, s);
            hcr_forward(&S, pv0.data(), A.data(), pv.data());
            if (spoil && S.wt) for (int q = 0; q < S.C; ++q) pv[((size_t)q * S.K) * ncol + 6] = std::nan("");
            if (spoil && s % 7 == 0 && S.C > 1) pv[((size_t)1 * S.K + (S.K - 1)) * ncol + 5] = 0.0;
            hcr_accept(&S, s);
        }
        hcr_finish(&S, nodes.data(), cols.data(), counts.data());
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
                Stage st(4, 4, mk[0], mk[1], C, spoil ? 40 : 10, spoil != 0 || C == 5, C == 5 ? 1 : spoil);
                const double sum = st.run(40, spoil != 0);
                std::printf("M %2d K %2d C %d spoil %d: sum %.17g\n", mk[0], mk[1], C, spoil, sum);
                if (!std::isfinite(sum)) ++bad;
            }
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
#endif
