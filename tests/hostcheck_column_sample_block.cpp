// TEST HARNESS (not product): the block proposals of dsurftomo_amd/csrc/column_sample.h on a CPU behind a C
// interface, for tests/test_hostcheck_column_sample_block.py and tests/test_gpu_column_sample_block.py.  It takes in
// tests/hostcheck_column_sample.cpp as it is -- the set-up, the linear forward function and the finish are that file's hcs_* -- and adds the
// shape of the columns (one lane of one, where the device has a wavefront per column), the proposals and the Metropolis tests with a
// SampleBlockView beside the SampleView, which tests/column_sample_block_ref.py mirrors field by field.  With
// -DHOSTCHECK_COLUMN_SAMPLE_BLOCK_MAIN the file is a stand-alone program that runs block sweeps on made-up columns of every tested size and
// on the special cases (for a sanitizer build).
#include "hostcheck_column_sample.cpp"

namespace {
struct NoSync {
    void operator()() const {}
};
}  // namespace

extern "C" {

int hcb_block_bytes() { return (int)sizeof(SampleBlockView); }

void hcb_rsqrt(long long n, const double* d, double* out)
{
    for (long long i = 0; i < n; ++i) out[i] = sample_rsqrt(d[i]);
}

// the shape of every interior column: obs / wt (K, ncol) fp32 (wt may be null), pv (K, ncol), S (M, K, ncol) -- the device's layouts;
// tri (M (M + 1) / 2, ncol), r (M, ncol), flag and nused (ncol): the ring's and a flagged column's tri and r are zeros
void hcb_shape(int nx, int ny, int M, int K, const float* obs, const float* wt, const double* pv, const double* S, float smooth, float damp, double* tri, double* r,
               int* flag, int* nused)
{
    const long long ncol = (long long)nx * ny;
    std::vector<double> work(column_work_doubles(M, K));
    for (long long e = 0; e < (long long)column_tri_size(M) * ncol; ++e) tri[e] = 0.0;
    for (long long e = 0; e < (long long)M * ncol; ++e) r[e] = 0.0;
    for (long long c = 0; c < ncol; ++c) {
        flag[c] = 0; nused[c] = 0;
        if (!sample_interior(nx, ny, c)) continue;
        ColumnIn in;
        in.M = M; in.K = K;
        in.obs = obs + c; in.obs_stride = ncol;
        in.wt = wt ? wt + c : nullptr; in.wt_stride = ncol;
        in.pv = pv + c; in.pv_stride = ncol;
        in.S = S + c; in.s_lstride = (long long)K * ncol; in.s_kstride = ncol;
        flag[c] = sample_shape(in, smooth, damp, column_work(work.data(), M, K), tri + c, r + c, ncol, &nused[c], 0, 1, NoSync());
    }
}

void hcb_propose(const SampleView* S, const SampleBlockView* B, int sweep)
{
    for (int q = 0; q < S->C; ++q)
        for (long long c = 0; c < S->ncol; ++c) sample_propose_block(*S, *B, c, q, sweep);
}

void hcb_accept(const SampleView* S, const SampleBlockView* B, int sweep)
{
    for (int q = 0; q < S->C; ++q)
        for (long long c = 0; c < S->ncol; ++c) sample_accept_block(*S, *B, c, q, sweep);
}

// sweeps first .. first + n - 1 with hcs_forward in place of the dispersion runs
void hcb_linear(const SampleView* S, const SampleBlockView* B, const double* pv0, const double* A, double* pv, int first, int n)
{
    for (int s = first; s < first + n; ++s) {
        hcb_propose(S, B, s);
        hcs_forward(S, pv0, A, pv);
        hcb_accept(S, B, s);
    }
}

}  // extern "C"

#ifdef HOSTCHECK_COLUMN_SAMPLE_BLOCK_MAIN
namespace {

// every array of a stage with block proposals, and its two views
struct Stage {
    std::vector<float> obs, wt, v0, v, best_v, pold, pold_all;
    std::vector<double> pv, phi, psi, S1, S2, phisum, best_e, phi0, pv0, A, St, nodes, cols, tri, r;
    std::vector<int> cnt, nkept, pnode, pmark, reseed, nused, flag, counts, sflag, snused, bcnt;
    std::vector<unsigned long long> used;
    SampleView S{};
    SampleBlockView B{};

    Stage(int nx, int ny, int M, int K, int C, int burn, int every, float width)
    {
        const size_t ncol = (size_t)nx * ny, cc = ncol * C, nz = (size_t)M + 1;
        obs.assign(K * ncol, 0.0f); wt.assign(K * ncol, 1.0f); v0.assign(nz * ncol, 0.0f); v.assign(nz * cc, 0.0f); best_v.assign(M * cc, 0.0f); pold.assign(cc, 0.0f);
        pold_all.assign(M * cc, 0.0f);
        pv.assign(K * cc, 0.0); phi.assign(cc, 0.0); psi.assign(cc, 0.0); S1.assign(M * cc, 0.0); S2.assign(M * cc, 0.0); phisum.assign(cc, 0.0); best_e.assign(cc, 0.0);
        phi0.assign(ncol, 0.0); pv0.assign(K * ncol, 0.0); A.assign((size_t)K * M * ncol, 0.0); St.assign((size_t)K * M * ncol, 0.0);
        nodes.assign(kSampleNodeFigures * M * ncol, 0.0); cols.assign(kSampleColumnFigures * ncol, 0.0);
        tri.assign((size_t)column_tri_size(M) * ncol, 0.0); r.assign(M * ncol, 0.0);
        cnt.assign(kSampleCounters * cc, 0); nkept.assign(cc, 0); pnode.assign(cc, 0); pmark.assign(cc, 0); reseed.assign(cc, 0); nused.assign(ncol, 0); flag.assign(ncol, 0);
        counts.assign(kSampleColumnCounts * ncol, 0); used.assign(ncol, 0ull); sflag.assign(ncol, 0); snused.assign(ncol, 0); bcnt.assign(kSampleBlockCounters * cc, 0);
        unsigned long long x = 54321u + 977u * (unsigned)M + 31u * (unsigned)K + (unsigned)C;
        auto rnd = [&x]() { x = sample_mix(x + 0x9E3779B97F4A7C15ull); return sample_unit(x >> 11); };
        for (size_t i = 0; i < v0.size(); ++i) v0[i] = (float)(3.0 + rnd());
        for (size_t i = 0; i < pv0.size(); ++i) { pv0[i] = 3.0 + rnd(); obs[i] = (float)(pv0[i] * (1.0 + 0.02 * (2.0 * rnd() - 1.0))); wt[i] = (float)(30.0 + 40.0 * rnd()); }
        for (size_t i = 0; i < A.size(); ++i) A[i] = rnd() * (2.0 / M);
        for (int k = 0; k < K; ++k)                             // A (K, M, ncol) as the shape reads it: (M, K, ncol)
            for (int l = 0; l < M; ++l)
                for (size_t c = 0; c < ncol; ++c) St[((size_t)l * K + k) * ncol + c] = A[((size_t)k * M + l) * ncol + c];
        S.nx = nx; S.ny = ny; S.nz = (int)nz; S.K = K; S.C = C; S.burn = burn; S.ncol = (long long)ncol; S.seed = 0x9876543210ull + (unsigned)M;
        S.lam2 = 4.0; S.step = 0.05; S.spread = 0.05; S.two_t = 2.0; S.width = width; S.minvel = 2.0f; S.maxvel = 4.5f;
        S.obs = obs.data(); S.wt = wt.data(); S.v0 = v0.data(); S.pv = pv.data(); S.v = v.data(); S.phi = phi.data(); S.psi = psi.data();
        S.cnt = cnt.data(); S.S1 = S1.data(); S.S2 = S2.data(); S.phisum = phisum.data(); S.nkept = nkept.data(); S.best_e = best_e.data(); S.best_v = best_v.data();
        S.pnode = pnode.data(); S.pold = pold.data(); S.pmark = pmark.data(); S.reseed = reseed.data(); S.used = used.data(); S.nused = nused.data(); S.flag = flag.data();
        S.phi0 = phi0.data();
        B.tri = tri.data(); B.r = r.data(); B.flag = sflag.data(); B.pold_all = pold_all.data(); B.cnt = bcnt.data(); B.block_every = every;
        B.block_scale = 2.38 * std::sqrt(3.0 / M);
    }

    // the set-up, the shape, n sweeps (spoil: column 9 has no datum, column 10's shape is flagged, every seventh sweep chain 1 of column 5
    // loses a root), the finish
    double run(int n, bool spoil)
    {
        const size_t ncol = (size_t)S.ncol;
        const int M = S.nz - 1;
        if (spoil) for (int k = 0; k < S.K; ++k) wt[(size_t)k * ncol + 9] = 0.0f;
        hcs_setup(&S, 0);
        hcs_forward(&S, pv0.data(), A.data(), pv.data());
        hcs_setup(&S, 1);
        hcb_shape(S.nx, S.ny, M, S.K, obs.data(), wt.data(), pv.data(), St.data(), 2.0f, 0.1f, tri.data(), r.data(), sflag.data(), snused.data());
        if (spoil) sflag[10] = kColumnNotPositive;
        for (int s = 1; s <= n; ++s) {
            hcb_propose(&S, &B, s);
            hcs_forward(&S, pv0.data(), A.data(), pv.data());
            if (spoil && s % 7 == 0 && S.C > 1) pv[((size_t)1 * S.K + (S.K - 1)) * ncol + 5] = 0.0;
            hcb_accept(&S, &B, s);
        }
        hcs_finish(&S, nodes.data(), cols.data(), counts.data());
        double sum = 0.0;
        for (double x : nodes) sum += x;
        for (double x : cols) sum += x;
        for (int x : counts) sum += x;
        for (int x : bcnt) sum += x;
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
            for (int spoil = 0; spoil < 2; ++spoil)
                for (int every : { 1, 3 }) {
                    Stage st(4, 4, mk[0], mk[1], C, spoil ? 40 : 10, every, spoil ? 0.03f : 0.5f);      // (spoil: a box narrow enough to be left)
                    const double sum = st.run(40, spoil != 0);
                    long long proposed = 0, outside = 0;
                    const size_t cc = (size_t)st.S.ncol * C;
                    for (size_t i = 0; i < cc; ++i) { proposed += st.bcnt[kSampleBlkProposed * cc + i]; outside += st.bcnt[kSampleBlkOutOfBox * cc + i]; }
                    std::printf("M %2d K %2d C %d spoil %d every %d: sum %.17g, %lld block proposals, %lld out of the box\n", mk[0], mk[1], C, spoil, every, sum, proposed, outside);
                    if (!std::isfinite(sum) || proposed == 0) ++bad;
                }
    for (double d : { 1.0, 2.0, 4.0, 0.5, 3.0, 1e-300, 1e300, 2.2250738585072014e-308, 1.7976931348623157e308 }) {
        const double want = 1.0 / std::sqrt(d), got = sample_rsqrt(d);
        if (!(std::fabs(got - want) <= 1e-12 * want)) ++bad;
        std::printf("rsqrt(%g) = %.17g (libm %.17g)\n", d, got, want);
    }
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
#endif
