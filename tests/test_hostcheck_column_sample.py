"""The Monte-Carlo depth inversion (dsurftomo_amd/csrc/column_sample.h) on the CPU through
tests/hostcheck_column_sample.cpp: the counter-based generator and sample_neglog against Python, the header against the Python twin
depth.column_sample_twin bit for bit, the sampler's law on a linear forward function -- where the posterior is Gaussian and its mean and
covariance are known -- and the special cases.

The law test's margins come from the run itself: the standard error of the pooled mean (variance) of an unknown is the scatter of the 64
chains' own means (variances) over sqrt(64); the pooled figure must lie within 5 of them of the analytic one.  Lengths used: 64 chains,
4000 sweeps, burn 1000, at (M, K) = (3, 6) and (7, 12).  Worst ratios seen (printed by the test): see DESIGN.md section 29."""
import math

import numpy as np
import pytest

import column_sample_ref as R
from dsurftomo_amd import depth

F = np.float32
WIDE = dict(width=5.0, minvel=0.0, maxvel=10.0)


@pytest.fixture(scope="module")
def h():
    return R.load()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def linear_case(M, K, nx=3, ny=3, seed=5, sigma=0.02):
    """a linear problem on every column: pv = pv0 + A (v - start), kernels of the size of real ones (a datum's kernel sums to about one over
    depth), observations a few sigma off pv0, weights 1 / sigma"""
    rng = np.random.default_rng(seed + 100 * M + K)
    ncol = nx * ny
    start = (3.0 + 0.5 * rng.random((M + 1, ncol))).astype(F)
    A = rng.random((K, M, ncol)) * (2.0 / M)
    pv0 = 3.0 + rng.random((K, ncol))
    obs = (pv0 + 2.0 * sigma * rng.standard_normal((K, ncol))).astype(F)
    wt = np.full((K, ncol), 1.0 / sigma, F)
    return start, obs, wt, pv0, A


def stage(h, start, obs, wt, C, nx=3, ny=3, smooth=10.0, step=0.05, spread=0.05, temperature=1.0, seed=77, burn=0, width=5.0, minvel=0.0, maxvel=10.0):
    return R.Stage(h, nx, ny, start, obs, wt, C, smooth, step, spread, width, temperature, minvel, maxvel, seed, burn)


def begin(st, pv0, A):
    st.setup_models()
    st.forward(pv0, A)
    st.setup_state()


# ---- 1. the generator ----

def test_generator_equals_the_twin(h):
    rng = np.random.default_rng(3)
    w = rng.integers(0, 2 ** 63, (4000, 5), dtype=np.uint64) >> rng.integers(0, 63, (4000, 5)).astype(np.uint64)
    w[:40] = np.array([[a, b, c, d, e] for a in (0, 2 ** 64 - 1) for b in (0, 2 ** 32 + 5) for c in (0, 1) for d in (0, 2 ** 33) for e in (0, 1, 2, 2 ** 40)][:40], np.uint64)
    k, u = R.draws(h, w)
    for i in range(len(w)):
        kk = depth.sample_bits(*[int(x) for x in w[i]])
        assert int(k[i]) == kk and u[i] == depth.sample_unit(kk) and 0.0 <= u[i] < 1.0
    assert (w[:, 1:] > 2 ** 32).any() and len(set(k.tolist())) == len(k)
    assert depth.sample_unit(2 ** 53 - 1) == 1.0 - 2.0 ** -53 and h.hcs_unit(1) == 2.0 ** -53
    assert abs(u.mean() - 0.5) < 5.0 / math.sqrt(12 * len(u))                     # 5 standard errors of a uniform mean


# ---- 2. sample_neglog ----

def test_neglog_against_libm(h):
    rng = np.random.default_rng(4)
    fixed = [1, 2, 2 ** 52 - 1, 2 ** 52 + 1, 2 ** 53 - 1]
    k = np.concatenate([np.array(fixed, np.uint64), rng.integers(1, 2 ** 53, 100000, dtype=np.uint64),
                        rng.integers(1, 2 ** 53, 2000, dtype=np.uint64) >> rng.integers(0, 52, 2000).astype(np.uint64)])
    k = np.maximum(k, np.uint64(1))
    got = R.neglog(h, k)
    want = np.array([-math.log(int(x) * 2.0 ** -53) for x in k])
    rel = np.abs(got - want) / np.abs(want)
    print("sample_neglog: largest relative error against math.log %.3g over %d values" % (rel.max(), k.size))
    assert (got > 0).all() and rel.max() <= 1e-12
    twin =np.array([depth.sample_neglog(int(x)) for x in k[:3000]])
    assert same_bits(twin, got[:3000])


# ---- the header against the twin, bit for bit ----

@pytest.mark.parametrize("M,K,C", [(1, 2, 2), (2, 3, 1), (3, 6, 3), (7, 12, 2)])
def test_header_equals_the_twin(h, M, K, C):
    nx, ny = 4, 3
    start, obs, wt, pv0, A = linear_case(M, K, nx, ny)
    wt[:, 5] *= F(0.5)
    wt[1, 6] = 0.0
    args = dict(smooth=3.0, step=0.08, spread=0.05, temperature=1.5, seed=2 ** 40 + 9, burn=5, width=0.12, minvel=2.9, maxvel=3.6)
    st = stage(h, start, obs, wt, C, nx, ny, **args)
    begin(st, pv0, A)
    fw = stage(h, start, obs, wt, C, nx, ny, **args)

    def forward(models):
        fw.a["models"][...] = models
        fw.forward(pv0, A)
        return fw.pv.copy()

    sweeps = 25
    st.linear(pv0, A, sweeps)
    tw = depth.column_sample_twin(nx, ny, start, obs, wt, forward, C, sweeps, args["burn"], args["smooth"], args["step"], args["spread"], args["width"],
                                  args["temperature"], args["minvel"], args["maxvel"], args["seed"])
    state = st.state()
    for name in R.STATE:
        assert same_bits(state[name], tw[name]), name
    nodes, cols, counts = st.finish()
    for q, name in enumerate(("mean", "var", "W", "B", "best")):
        assert same_bits(nodes[q], tw[name]), name
    assert same_bits(cols[0], tw["phi_start"]) and same_bits(cols[1], tw["best_energy"]) and same_bits(cols[2], tw["mean_phi"])
    assert (counts[0] == tw["nused"]).all() and (counts[1] == tw["flag"]).all() and (counts[7] == tw["nkept"][0]).all()
    assert (state["counters"][2] > 0).any() and (state["counters"][0] > 0).any()           # the narrow box was hit, and moves were made
    if C == 1:
        assert not nodes[3].any()


# ---- 3. the sampler's law ----

@pytest.mark.parametrize("M,K", [(3, 6), (7, 12)])
def test_law_on_a_linear_forward_function(h, M, K):
    C, sweeps, burn, smooth = 64, 4000, 1000, 10.0
    start, obs, wt, pv0, A = linear_case(M, K)
    st = stage(h, start, obs, wt, C, smooth=smooth, burn=burn, **WIDE)
    begin(st, pv0, A)
    st.linear(pv0, A, sweeps)
    nodes, cols, counts = st.finish()
    c = 4                                                                            # the interior column of the 3 x 3 grid
    n = sweeps - burn
    assert counts[7, c] == n and counts[1, c] == 0 and counts[0, c] == K
    # the analytic posterior: precision N = A^T W A + smooth^2 L^T L, mean of v - start = N^-1 (A^T W r - smooth^2 L^T L start)
    a = wt[:, c].astype(np.float64); S = A[:, :, c]
    LtL = depth.column_ltl(M).astype(np.float64)
    N = S.T @ (a[:, None] ** 2 * S) + smooth ** 2 * LtL
    v0 = start[:M, c].astype(np.float64)
    cov = np.linalg.inv(N)
    mean = v0 + cov @ (S.T @ (a ** 2 * (obs[:, c].astype(np.float64) - pv0[:, c])) - smooth ** 2 * (LtL @ v0))
    s = st.state()
    m_q = s["S1"][:, :, c] / n                                                       # (M, C): the chains' own means and variances
    v_q = s["S2"][:, :, c] / n - m_q ** 2
    se_mean = m_q.std(axis=1, ddof=1) / math.sqrt(C)
    se_var = v_q.std(axis=1, ddof=1) / math.sqrt(C)
    r_mean = np.abs(nodes[0][:, c] - mean) / se_mean
    r_var = np.abs(nodes[1][:, c] - np.diag(cov)) / se_var
    rhat = depth.sample_rhat(nodes[2][:, c], nodes[3][:, c], n)
    acc = s["counters"][0, :, c].sum() / (C * sweeps)
    print("M %d K %d: %d chains, %d sweeps, burn %d: worst |mean - analytic| / se %.2f, worst |var - analytic| / se %.2f, worst R-hat %.4f, accepted %.1f %%, sd %.4f .. %.4f"
          % (M, K, C, sweeps, burn, r_mean.max(), r_var.max(), rhat.max(), 100 * acc, np.sqrt(np.diag(cov)).min(), np.sqrt(np.diag(cov)).max()))
    assert (r_mean <= 5.0).all() and (r_var <= 5.0).all()
    assert (rhat < 1.1).all()
    assert np.isfinite(nodes).all() and not nodes[:, :, [0, 1, 2, 3, 5, 6, 7, 8]].any()      # the ring: nothing kept, zeros


# ---- 4. the special cases ----

def test_out_of_box_and_lost_root(h):
    M, K, C = 3, 6, 4
    start, obs, wt, pv0, A = linear_case(M, K)
    st = stage(h, start, obs, wt, C, step=0.3, width=0.05, spread=0.02, minvel=0.0, maxvel=10.0)
    begin(st, pv0, A)
    c = 4
    lo, hi = start[:M, c] - F(0.05), start[:M, c] + F(0.05)
    seen = set()
    for sweep in range(1, 41):
        before = st.state()
        st.propose()
        st.forward(pv0, A)
        lost = sweep % 5 == 0
        if lost:
            st.pv[2, K - 1, c] = 0.0                                                 # chain 2 loses the root of the last datum
        mid = st.a["pmark"][:, c].copy()
        st.accept()
        after = st.state()
        for q in range(C):
            mark = after["pmark"][q, c]
            seen.add(int(mark))
            if mid[q] == R.OUT_OF_BOX:
                assert mark == R.OUT_OF_BOX
            if lost and q == 2 and mid[q] == R.PENDING:
                assert mark == R.NO_ROOT
            if mark in (R.OUT_OF_BOX, R.NO_ROOT, R.REJECTED):                        # a rejection of any kind: the chain is what it was
                assert same_bits(after["models"][:, q, c], before["models"][:, q, c]) and after["phi"][q, c] == before["phi"][q, c] and after["psi"][q, c] == before["psi"][q, c]
            else:
                assert mark == R.ACCEPTED and not same_bits(after["models"][:, q, c], before["models"][:, q, c])
        assert (after["models"][:M, :, c] >= lo[:, None]).all() and (after["models"][:M, :, c] <= hi[:, None]).all()
    assert {R.OUT_OF_BOX, R.NO_ROOT, R.ACCEPTED} <= seen
    cnt = st.state()["counters"][:, :, c]
    assert (cnt[0] + cnt[1] == 40).all() and cnt[2].sum() > 0 and cnt[3, 2] > 0 and not cnt[3, [0, 1, 3]].any()
    assert (st.state()["pmark"][:, [0, 1, 2, 3, 5, 6, 7, 8]] == R.IDLE).all()


def test_unused_datum_with_nan_changes_no_bit(h):
    M, K, C = 3, 6, 3
    start, obs, wt, pv0, A = linear_case(M, K)
    wt[2, 4] = 0.0                                                                   # datum 2 of the interior column is unused
    runs = []
    for poison in (False, True):
        st = stage(h, start, obs, wt, C, burn=3)
        st.setup_models()
        st.forward(pv0, A)
        if poison:
            st.pv[:, 2, 4] = np.nan
        st.setup_state()
        for sweep in range(12):
            st.propose()
            st.forward(pv0, A)
            if poison:
                st.pv[:, 2, 4] = np.nan
            st.accept()
        runs.append((st.state(), st.finish()))
    for name in R.STATE:
        assert same_bits(runs[0][0][name], runs[1][0][name]), name
    for a, b in zip(runs[0][1], runs[1][1]):
        assert same_bits(a, b) and np.isfinite(a).all()
    assert runs[0][1][2][0, 4] == K - 1


def test_column_without_data_is_never_moved(h):
    M, K, C = 3, 6, 3
    start, obs, wt, pv0, A = linear_case(M, K, 4, 3)
    wt[:, 5] = 0.0                                                                   # interior column 5: no datum; interior column 6 samples
    st = stage(h, start, obs, wt, C, 4, 3, burn=2)
    begin(st, pv0, A)
    st.linear(pv0, A, 10)
    s = st.state()
    nodes, cols, counts = st.finish()
    assert counts[1, 5] == 2 and counts[0, 5] == 0 and counts[7, 5] == 0 and counts[1, 6] == 0 and counts[7, 6] == 8
    for q in range(C):
        assert same_bits(s["models"][:, q, 5], start[:, 5])
    assert not s["counters"][:, :, 5].any() and (s["pmark"][:, 5] == R.IDLE).all() and not nodes[:, :, 5].any()
    assert s["counters"][0, :, 6].sum() > 0 and same_bits(s["models"][M], np.broadcast_to(start[M], (C, 12)))      # the bottom depth stays


def test_one_unknown_and_one_chain(h):
    for M, C in ((1, 3), (3, 1), (1, 1)):
        K = 4
        start, obs, wt, pv0, A = linear_case(M, K)
        st = stage(h, start, obs, wt, C, burn=10, smooth=4.0)
        begin(st, pv0, A)
        assert not st.state()["psi"].any() if M == 1 else st.state()["psi"][:, 4].all()
        st.linear(pv0, A, 60)
        nodes, cols, counts = st.finish()
        assert np.isfinite(nodes).all() and counts[7, 4] == 50 and nodes[1][:, 4].min() > 0
        if C == 1:
            assert not nodes[3].any() and same_bits(nodes[1][:, 4], nodes[2][:, 4])              # one chain: B = 0 and the pooled variance is W
        else:
            assert nodes[3][:, 4].min() > 0
        assert counts[2, 4] + counts[3, 4] == 60 * C


def test_reseeded_chain(h):
    M, K, C = 3, 6, 4
    start, obs, wt, pv0, A = linear_case(M, K)
    st = stage(h, start, obs, wt, C, spread=0.1)
    st.setup_models()
    assert not same_bits(st.a["models"][:M, 2, 4], start[:M, 4])
    st.forward(pv0, A)
    st.pv[2, 3, 4] = 0.0                                                             # chain 2 starts where datum 3 has no root
    st.setup_state()
    s = st.state()
    assert (s["reseeded"][:, 4] == [0, 0, 1, 0]).all() and same_bits(s["models"][:, 2, 4], start[:, 4])
    assert s["phi"][2, 4] == s["phi"][0, 4] and s["psi"][2, 4] == s["psi"][0, 4] and s["phi"][1, 4] != s["phi"][0, 4]
    nodes, cols, counts = st.finish()
    assert counts[6, 4] == 1 and counts[0, 4] == K and cols[0, 4] == s["phi"][0, 4]
    st.pv[0, 0, 4] = 0.0                                                             # chain 0 itself without a root: the datum is not used
    st.setup_models(); st.forward(pv0, A); st.pv[0, 0, 4] = 0.0
    st.setup_state()
    assert st.finish()[2][0, 4] == K - 1


def test_nothing_kept_gives_zeros(h):
    M, K, C = 3, 6, 3
    start, obs, wt, pv0, A = linear_case(M, K)
    st = stage(h, start, obs, wt, C, burn=15)
    begin(st, pv0, A)
    st.linear(pv0, A, 15)
    nodes, cols, counts = st.finish()
    assert not nodes.any() and not cols[1:].any() and cols[0, 4] > 0 and counts[7].max() == 0 and counts[2, 4] + counts[3, 4] == 15 * C
    st.linear(pv0, A, 1)
    nodes, cols, counts = st.finish()
    assert counts[7, 4] == 1 and nodes[0][:, 4].all() and not nodes[2][:, 4].any() and np.isfinite(nodes).all()      # one kept sweep: W = 0, not NaN
    assert (depth.sample_rhat(nodes[2], nodes[3], counts[7][None]) == 1.0).all()


def test_standalone_program_runs(h, tmp_path):
    """the same file with its own main (the sizes and the special cases stand-alone: what a sanitizer build runs), here in the plain build"""
    import subprocess
    exe = str(tmp_path / "hostcheck_column_sample")
    subprocess.check_call(["g++"] + R.FLAGS + ["-DHOSTCHECK_COLUMN_SAMPLE_MAIN", "-o", exe, R.SRC, "-lm"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
