// TEST HARNESS (not product): the posterior marginals of dsurftomo_amd/csrc/column_sample.h on a CPU behind a C
// interface, for tests/test_hostcheck_column_sample_marginals.py and tests/test_gpu_column_sample_marginals.py.  It takes in
// tests/hostcheck_column_sample_block.cpp as it is -- the set-up, the sweeps, the linear forward function and the finish are that file's
// hcs_* and hcb_* -- and adds the bin rule, the counts and products of a kept sweep (a loop over (row, chain, column) where the device has
// one thread each) and the marginals' finish with a SampleMarginalView beside the other two views, which
// tests/column_sample_marginals_ref.py mirrors field by field.  With -DHOSTCHECK_COLUMN_SAMPLE_MARGINALS_MAIN the file is a stand-alone
// program that runs the marginals on made-up columns of the smallest, a middle and the largest size (for a sanitizer build); the stage it
// runs them on is the block file's own, whose main is then compiled under another name and not called.
#ifdef HOSTCHECK_COLUMN_SAMPLE_MARGINALS_MAIN
#define HOSTCHECK_COLUMN_SAMPLE_BLOCK_MAIN
#define main hostcheck_column_sample_block_main
#endif
#include "hostcheck_column_sample_block.cpp"
#ifdef HOSTCHECK_COLUMN_SAMPLE_MARGINALS_MAIN
#undef main
#endif

#include <cstring>

extern "C" {

int hcm_marginal_bytes() { return (int)sizeof(SampleMarginalView); }

// the bins of n values at (column c, depth l)
void hcm_bin(const SampleView* S, long long c, int l, int nbins, long long n, const float* v, int* out)
{
    for (long long i = 0; i < n; ++i) out[i] = sample_bin(*S, c, l, nbins, v[i]);
}

// what the marginals take of sweep `sweep`, after its Metropolis test
void hcm_accumulate(const SampleView* S, const SampleMarginalView* G, int sweep)
{
    const int M = S->nz - 1;
    if (sweep <= S->burn) return;      // (the device launches nothing)
    for (int l = 0; l < M; ++l)
        for (int q = 0; q < S->C; ++q)
            for (long long c = 0; c < S->ncol; ++c) sample_marginal_hist(*S, *G, c, q, l, sweep);
    if (!G->P) return;
    for (int e = 0; e < column_tri_size(M); ++e)
        for (int q = 0; q < S->C; ++q)
            for (long long c = 0; c < S->ncol; ++c) sample_marginal_cov(*S, *G, c, q, e, sweep);
}

// sweeps first .. first + n - 1 with hcs_forward in place of the dispersion runs; G null: the marginals are off
void hcm_linear(const SampleView* S, const SampleBlockView* B, const SampleMarginalView* G, const double* pv0, const double* A, double* pv, int first, int n)
{
    for (int s = first; s < first + n; ++s) {
        hcb_propose(S, B, s);
        hcs_forward(S, pv0, A, pv);
        hcb_accept(S, B, s);
        if (G) hcm_accumulate(S, G, s);
    }
}

// pooled (nbins, M, ncol), figures (1 + nlevels, M, ncol), cov (tri, ncol) or null
void hcm_finish(const SampleView* S, const SampleMarginalView* G, int nlevels, const double* levels, unsigned* pooled, double* figures, double* cov)
{
    const int M = S->nz - 1;
    for (int l = 0; l < M; ++l)
        for (long long c = 0; c < S->ncol; ++c) sample_marginal_finish(*S, *G, c, l, nlevels, levels, pooled, figures);
    if (!cov) return;
    for (int e = 0; e < column_tri_size(M); ++e)
        for (long long c = 0; c < S->ncol; ++c) sample_marginal_cov_finish(*S, *G, c, e, cov);
}

}  // extern "C"

#ifdef HOSTCHECK_COLUMN_SAMPLE_MARGINALS_MAIN
namespace {

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// 40 sweeps of the block file's stage with the marginals beside it; the laws that need no reference.  Returns the number broken.
int run_case(int M, int K, int C, int nbins, bool spoil, double* sum_out)
{
    Stage st(4, 4, M, K, C, 10, 3, spoil ? 0.03f : 0.5f);
    const size_t ncol = (size_t)st.S.ncol, cc = ncol * C, T = (size_t)column_tri_size(M);
    std::vector<unsigned> hist((size_t)nbins * M * cc, 0u), pooled((size_t)nbins * M * ncol, 0u);
    std::vector<double> P(T * cc, 0.0), cov(T * ncol, 0.0);
    const double levels[5] = { 0.025, 0.16, 0.5, 0.84, 0.975 };
    std::vector<double> figures((size_t)6 * M * ncol, 0.0);
    SampleMarginalView G{};
    G.nbins = nbins; G.hist = hist.data(); G.P = P.data();
    if (spoil) for (int k = 0; k < K; ++k) st.wt[(size_t)k * ncol + 9] = 0.0f;      // column 9: no datum
    hcs_setup(&st.S, 0);
    hcs_forward(&st.S, st.pv0.data(), st.A.data(), st.pv.data());
    hcs_setup(&st.S, 1);
    hcb_shape(st.S.nx, st.S.ny, M, K, st.obs.data(), st.wt.data(), st.pv.data(), st.St.data(), 2.0f, 0.1f, st.tri.data(), st.r.data(), st.sflag.data(), st.snused.data());
    hcm_linear(&st.S, &st.B, &G, st.pv0.data(), st.A.data(), st.pv.data(), 1, 40);
    hcs_finish(&st.S, st.nodes.data(), st.cols.data(), st.counts.data());
    hcm_finish(&st.S, &G, 5, levels, pooled.data(), figures.data(), cov.data());
    int bad = 0;
    double sum = 0.0;
    for (size_t c = 0; c < ncol; ++c)
        for (int l = 0; l < M; ++l) {
            const int n = st.nkept[c];
            for (int q = 0; q < C; ++q) {
                unsigned total = 0u;
                for (int b = 0; b < nbins; ++b) total += hist[(((size_t)b * M + l) * C + q) * ncol + c];
                if (total != (unsigned)st.nkept[(size_t)q * ncol + c]) ++bad;
                if (!same_bits(P[((size_t)column_tri(l, l) * C + q) * ncol + c], st.S2[((size_t)l * C + q) * ncol + c])) ++bad;
            }
            if (!same_bits(cov[(size_t)column_tri(l, l) * ncol + c], st.nodes[((size_t)kSampleVar * M + l) * ncol + c])) ++bad;
            float lo, hi;
            sample_box(st.S, (long long)c, l, &lo, &hi);
            double before = n > 0 ? (double)lo : 0.0;
            for (int f = 1; f <= 5; ++f) {
                const double x = figures[((size_t)f * M + l) * ncol + c];
                if (!(x >= before) || (n > 0 && !(x <= (double)hi)) || (n == 0 && x != 0.0)) ++bad;
                before = x;
                sum += x;
            }
            sum += figures[(size_t)l * ncol + c];
        }
    for (double x : cov) { if (!std::isfinite(x)) ++bad; sum += x; }
    *sum_out = sum;
    return bad;
}

}  // namespace

int main()
{
    const int sizes[3][2] = { { 1, 1 }, { 7, 12 }, { 63, 60 } };
    int bad = 0;
    for (const auto& mk : sizes)
        for (int C : { 1, 5 })
            for (int nbins : { 2, 256 })
                for (int spoil = 0; spoil < 2; ++spoil) {
                    double sum = 0.0;
                    const int broken = run_case(mk[0], mk[1], C, nbins, spoil != 0, &sum);
                    std::printf("M %2d K %2d C %d nbins %3d spoil %d: sum %.17g, %d laws broken\n", mk[0], mk[1], C, nbins, spoil, sum, broken);
                    if (broken || !std::isfinite(sum)) ++bad;
                }
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
#endif
