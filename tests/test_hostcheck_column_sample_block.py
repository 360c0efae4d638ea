"""The block proposals of the Monte-Carlo depth inversion (dsurftomo_amd/csrc/column_sample.h) on the CPU through
tests/hostcheck_column_sample_block.cpp: sample_rsqrt against math.sqrt and the twin, the header against depth.column_sample_twin bit for
bit with block sweeps on and off, the shape against a plain-Python L D L^T, the sampler's law on section 29's linear forward function,
what the proposals are for (R-hat after 500 sweeps against the single-node chains'), and the special cases.

The law test's margins are section 29's: the standard error of the pooled mean (variance) of an unknown is the scatter of the 64 chains'
own means (variances) over sqrt(64); the pooled figure must lie within 5 of them of the analytic one.  The figures the tests print are in
DESIGN.md section 32."""
import math
import subprocess

import numpy as np
import pytest

import column_sample_block_ref as B
import column_sample_ref as R
import test_hostcheck_column_sample as T29
from dsurftomo_amd import depth

F = np.float32
same_bits = T29.same_bits
linear_case = T29.linear_case
NARROW = dict(smooth=3.0, step=0.08, spread=0.05, temperature=1.5, seed=2 ** 40 + 9, burn=5, width=0.12, minvel=2.9, maxvel=3.6)      # section 29's twin case


@pytest.fixture(scope="module")
def h():
    return B.load()


def block_stage(h, start, obs, wt, C, nx=3, ny=3, smooth=10.0, step=0.05, spread=0.05, temperature=1.0, seed=77, burn=0, width=5.0, minvel=0.0, maxvel=10.0,
                shape=None, block_every=0, block_scale=None):
    M = start.shape[0] - 1
    scale = depth.sample_block_scale(M, float(F(temperature))) if block_scale is None else block_scale
    return B.BlockStage(h, nx, ny, start, obs, wt, C, smooth, step, spread, width, temperature, minvel, maxvel, seed, burn, shape, block_every, scale)


def begin(st, pv0, A):
    st.setup_models()
    st.forward(pv0, A)
    st.setup_state()


def header_shape(h, nx, ny, obs, wt, pv0, A, smooth, damp):
    """the header's shape of the linear problem's columns: the depth kernels are A (K, M, ncol), the curve pv0"""
    return B.shape(h, nx, ny, obs, wt, pv0, np.ascontiguousarray(A.transpose(1, 0, 2)), smooth, damp)


def analytic_shape(M, ncol, c, N):
    """dict(tri, r, flag) with the L D L^T of N at column c, every other column flagged"""
    Lm, d = depth._twin_factor(N)
    sh = dict(tri=np.zeros((B.tri_size(M), ncol)), r=np.zeros((M, ncol)), flag=np.ones(ncol, np.int32))
    for i in range(M):
        for j in range(i):
            sh["tri"][depth.column_tri(i, j), c] = Lm[i, j]
        sh["tri"][depth.column_tri(i, i), c] = N[i, i]
        sh["r"][i, c] = depth.sample_rsqrt(d[i])
    sh["flag"][c] = 0
    return sh


# ---- 1. sample_rsqrt ----

def test_rsqrt_against_libm(h):
    rng = np.random.default_rng(6)
    fixed = [1.0, 2.0, 4.0, 1.0 - 2.0 ** -52, 1.0 + 2.0 ** -52, 1e-300, 1e300, 2.0 ** -1022, float(np.finfo(np.float64).max)]
    fixed += [2.0 ** k for k in range(-1021, 1024, 7)] + [2.0 ** -k for k in range(1, 60)] + [2.0 ** k for k in range(1, 60)]
    d = np.concatenate([np.array(fixed), np.ldexp(1.0 + rng.random(100000), rng.integers(-1022, 1024, 100000))])
    assert np.isfinite(d).all() and (d >= 2.0 ** -1022).all()
    got = B.rsqrt(h, d)
    want = np.array([1.0 / math.sqrt(x) for x in d])
    rel = np.abs(got - want) / want
    print("sample_rsqrt: largest relative error against 1 / math.sqrt %.3g over %d values" % (rel.max(), d.size))
    assert (got > 0).all() and rel.max() <= 1e-12
    twin = np.array([depth.sample_rsqrt(x) for x in d[:4000]])
    assert same_bits(twin, got[:4000])
    assert B.rsqrt(h, [1.0, 4.0, 0.25]).tolist() == [1.0, 0.5, 2.0]


# ---- 2. the header against the twin, bit for bit ----

@pytest.mark.parametrize("every", [1, 2, 3])
@pytest.mark.parametrize("M,K,C", [(1, 2, 2), (2, 3, 1), (3, 6, 3), (7, 12, 2)])
def test_header_equals_the_twin(h, M, K, C, every):
    nx, ny = 4, 3
    start, obs, wt, pv0, A = linear_case(M, K, nx, ny)
    wt[:, 5] *= F(0.5)
    wt[1, 6] = 0.0
    sh = header_shape(h, nx, ny, obs, wt, pv0, A, NARROW["smooth"], 0.1)
    assert sh["flag"][[5, 6]].tolist() == [0, 0]
    st = block_stage(h, start, obs, wt, C, nx, ny, shape=sh, block_every=every, **NARROW)
    begin(st, pv0, A)
    fw = T29.stage(R.load(), start, obs, wt, C, nx, ny, **NARROW)

    def forward(models):
        fw.a["models"][...] = models
        fw.forward(pv0, A)
        return fw.pv.copy()

    sweeps = 25
    st.linear(pv0, A, sweeps)
    a = NARROW
    tw = depth.column_sample_twin(nx, ny, start, obs, wt, forward, C, sweeps, a["burn"], a["smooth"], a["step"], a["spread"], a["width"], a["temperature"], a["minvel"],
                                  a["maxvel"], a["seed"], shape=sh, block_every=every)
    state = st.state()
    for name in R.STATE + B.BLOCK_STATE:
        assert same_bits(state[name], tw[name]), name
    nodes, cols, counts = st.finish()
    for q, name in enumerate(("mean", "var", "W", "B", "best")):
        assert same_bits(nodes[q], tw[name]), name
    assert same_bits(cols[0], tw["phi_start"]) and same_bits(cols[1], tw["best_energy"]) and same_bits(cols[2], tw["mean_phi"])
    bc = state["block_counters"]
    print("M %d K %d C %d every %d: %d block proposals, %d accepted, %d out of the box" % (M, K, C, every, bc[0].sum(), bc[1].sum(), bc[2].sum()))
    assert (bc[0][:, [5, 6]] == sweeps // every).all() and not bc[:, :, [0, 1, 2, 3, 4, 7, 8, 9, 10, 11]].any()
    assert bc[2].sum() > 0 and bc[1].sum() > 0                                     # the narrow box was left, and block moves were made
    assert (bc[1] + bc[2] <= bc[0]).all() and (state["counters"][2] >= bc[2]).all() and (state["counters"][0] >= bc[1]).all()


@pytest.mark.parametrize("M,K,C", [(1, 2, 2), (2, 3, 1), (3, 6, 3), (7, 12, 2)])
def test_block_every_zero_gives_the_single_node_bits(h, M, K, C):
    nx, ny = 4, 3
    start, obs, wt, pv0, A = linear_case(M, K, nx, ny)
    wt[:, 5] *= F(0.5)
    wt[1, 6] = 0.0
    old = T29.stage(R.load(), start, obs, wt, C, nx, ny, **NARROW)                 # section 29's case on section 29's build
    T29.begin(old, pv0, A)
    old.linear(pv0, A, 25)
    want, want_fin = old.state(), old.finish()
    sh = header_shape(h, nx, ny, obs, wt, pv0, A, NARROW["smooth"], 0.1)
    a = NARROW
    for shape in (None, sh):
        st = block_stage(h, start, obs, wt, C, nx, ny, shape=shape, block_every=0, **NARROW)
        begin(st, pv0, A)
        st.linear(pv0, A, 25)
        got = st.state()
        for name in R.STATE:
            assert same_bits(got[name], want[name]), name
        assert not got["block_counters"].any() and not got["pold_all"].any()
        for x, y in zip(st.finish(), want_fin):
            assert same_bits(x, y)

        def forward(models):
            old.a["models"][...] = models
            old.forward(pv0, A)
            return old.pv.copy()
        tw = depth.column_sample_twin(nx, ny, start, obs, wt, forward, C, 25, a["burn"], a["smooth"], a["step"], a["spread"], a["width"], a["temperature"], a["minvel"],
                                      a["maxvel"], a["seed"], shape=shape, block_every=0)
        for name in R.STATE:
            assert same_bits(tw[name], want[name]), name


# ---- 3. the shape ----

@pytest.mark.parametrize("M,K", [(1, 2), (2, 3), (3, 6), (7, 12), (63, 60)])
def test_shape_equals_a_plain_factorisation(h, M, K):
    nx, ny = 4, 3
    start, obs, wt, pv0, A = linear_case(M, K, nx, ny)
    wt[:, 5] = 0.0                                                                 # no datum: flag 2
    wt[1, 6] = 0.0
    smooth, damp = 2.5, 0.3
    sh = header_shape(h, nx, ny, obs, wt, pv0, A, smooth, damp)
    assert sh["flag"].tolist() == [0] * 5 + [2] + [0] * 6 and sh["nused"][5] == 0 and sh["nused"][6] == K - 1
    assert not sh["tri"][:, [0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11]].any() and not sh["r"][:, [0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11]].any()
    c = 6
    used, rho, _, G = depth._twin_data(obs[:, c], wt[:, c], pv0[:, c], A[:, :, c])
    N, _ = depth._twin_normal(G, used, rho, float(F(smooth)) ** 2, float(F(damp)) ** 2)
    Lm = [[0.0] * M for _ in range(M)]; d = [0.0] * M                              # column_factor in plain Python floats
    for j in range(M):
        v = [Lm[j][p] * d[p] for p in range(j)]
        dj = float(N[j, j])
        for p in range(j):
            dj -= Lm[j][p] * v[p]
        assert math.isfinite(dj) and dj > 0
        d[j] = dj
        for i in range(j + 1, M):
            s = float(N[i, j])
            for p in range(j):
                s -= Lm[i][p] * v[p]
            Lm[i][j] = s / dj
    tri = np.array([float(N[i, i]) if i == j else Lm[i][j] for i in range(M) for j in range(i + 1)])
    r = np.array([depth.sample_rsqrt(x) for x in d])
    assert same_bits(sh["tri"][:, c], tri) and same_bits(sh["r"][:, c], r)
    t2, r2, f2 = depth.column_shape_twin(obs[:, c], wt[:, c], pv0[:, c], A[:, :, c], smooth, damp)
    assert f2 == 0 and same_bits(t2, tri) and same_bits(r2, r)
    assert depth.column_shape_twin(obs[:, 5], wt[:, 5], pv0[:, 5], A[:, :, 5], smooth, damp)[2] == 2
    Ln = np.array(Lm) + np.eye(M)
    back = Ln @ np.diag(d) @ Ln.T
    assert np.abs(back - N).max() <= 1e-12 * np.abs(N).max()
    assert np.abs(r * r * np.array(d) - 1.0).max() <= 1e-12


def test_shape_flags_a_bad_pivot(h):
    M, K, nx, ny = 3, 6, 3, 3
    start, obs, wt, pv0, A = linear_case(M, K, nx, ny)
    A[:, :, 4] = np.nan                                                            # every pivot NaN
    sh = header_shape(h, nx, ny, obs, wt, pv0, A, 1.0, 0.1)
    assert sh["flag"][4] == 1 and not sh["tri"].any() and not sh["r"].any()
    assert depth.column_shape_twin(obs[:, 4], wt[:, 4], pv0[:, 4], A[:, :, 4], 1.0, 0.1)[2] == 1


# ---- 4. the law, 5. what the feature is for ----

def analytic(M, K, smooth, start, obs, wt, pv0, A, c=4):
    a = wt[:, c].astype(np.float64); S = A[:, :, c]
    LtL = depth.column_ltl(M).astype(np.float64)
    N = S.T @ (a[:, None] ** 2 * S) + smooth ** 2 * LtL
    v0 = start[:M, c].astype(np.float64)
    cov = np.linalg.inv(N)
    mean = v0 + cov @ (S.T @ (a ** 2 * (obs[:, c].astype(np.float64) - pv0[:, c])) - smooth ** 2 * (LtL @ v0))
    return N, mean, cov


@pytest.mark.parametrize("every", [1, 2])
@pytest.mark.parametrize("M,K", [(3, 6), (7, 12)])
def test_law_on_a_linear_forward_function(h, M, K, every):
    C, sweeps, burn, smooth = 64, 4000, 1000, 10.0
    start, obs, wt, pv0, A = linear_case(M, K)
    c, n = 4, sweeps - burn
    N, mean, cov = analytic(M, K, smooth, start, obs, wt, pv0, A)
    st = block_stage(h, start, obs, wt, C, smooth=smooth, burn=burn, shape=analytic_shape(M, 9, c, N), block_every=every, **T29.WIDE)
    begin(st, pv0, A)
    st.linear(pv0, A, sweeps)
    nodes, cols, counts = st.finish()
    assert counts[7, c] == n and counts[1, c] == 0 and counts[0, c] == K
    s = st.state()
    m_q = s["S1"][:, :, c] / n
    v_q = s["S2"][:, :, c] / n - m_q ** 2
    se_mean = m_q.std(axis=1, ddof=1) / math.sqrt(C)
    se_var = v_q.std(axis=1, ddof=1) / math.sqrt(C)
    r_mean = np.abs(nodes[0][:, c] - mean) / se_mean
    r_var = np.abs(nodes[1][:, c] - np.diag(cov)) / se_var
    rhat = depth.sample_rhat(nodes[2][:, c], nodes[3][:, c], n)
    bc = s["block_counters"][:, :, c].sum(axis=1)
    single = s["counters"][0, :, c].sum() - bc[1], C * sweeps - bc[0]
    print("M %d K %d every %d: worst |mean - analytic| / se %.2f, worst |var - analytic| / se %.2f, worst R-hat %.4f, block sweeps accepted %.1f %%, single-node %s"
          % (M, K, every, r_mean.max(), r_var.max(), rhat.max(), 100.0 * bc[1] / bc[0], "%.1f %%" % (100.0 * single[0] / single[1]) if single[1] else "none"))
    assert bc[0] == C * (sweeps // every) and bc[2] == 0
    assert (r_mean <= 5.0).all() and (r_var <= 5.0).all()
    assert (rhat < 1.1).all()
    assert np.isfinite(nodes).all() and not nodes[:, :, [0, 1, 2, 3, 5, 6, 7, 8]].any()


@pytest.mark.parametrize("M,K", [(3, 6), (7, 12)])
def test_block_sweeps_converge_at_least_twice_as_far(h, M, K):
    C, sweeps, burn, smooth = 64, 500, 100, 10.0
    start, obs, wt, pv0, A = linear_case(M, K)
    c, n = 4, sweeps - burn
    N = analytic(M, K, smooth, start, obs, wt, pv0, A)[0]
    worst = {}
    for every in (0, 1, 2):
        st = block_stage(h, start, obs, wt, C, smooth=smooth, burn=burn, shape=analytic_shape(M, 9, c, N), block_every=every, **T29.WIDE)
        begin(st, pv0, A)
        st.linear(pv0, A, sweeps)
        nodes = st.finish()[0]
        worst[every] = float(depth.sample_rhat(nodes[2][:, c], nodes[3][:, c], n).max()) - 1.0
    print("M %d K %d, %d sweeps, burn %d: worst R-hat - 1 single-node %.4f, every sweep a block %.4f, every second %.4f" % (M, K, sweeps, burn, worst[0], worst[1], worst[2]))
    assert worst[1] <= 0.5 * worst[0] and worst[2] <= 0.5 * worst[0]


# ---- 6. the special cases ----

def test_flagged_shape_falls_back_and_idle_columns_stay(h):
    M, K, C, nx, ny = 3, 6, 3, 4, 3
    start, obs, wt, pv0, A = linear_case(M, K, nx, ny)
    wt[:, 5] = 0.0                                                                 # interior column 5: no datum; column 6 samples
    sh = header_shape(h, nx, ny, obs, wt, pv0, A, 10.0, 0.1)
    assert sh["flag"][5] == 2 and sh["flag"][6] == 0
    sh["flag"][6] = 1                                                              # column 6's shape is flagged: single-node proposals
    args = dict(burn=2, smooth=10.0)
    st = block_stage(h, start, obs, wt, C, nx, ny, shape=sh, block_every=1, **args)
    begin(st, pv0, A)
    st.linear(pv0, A, 10)
    old = T29.stage(R.load(), start, obs, wt, C, nx, ny, **args)
    T29.begin(old, pv0, A)
    old.linear(pv0, A, 10)
    got, want = st.state(), old.state()
    for name in R.STATE:
        assert same_bits(got[name], want[name]), name                              # every sweep a block sweep, and the single-node sampler's bits
    assert not got["block_counters"].any() and (got["pnode"][:, 6] >= 0).all() and got["counters"][0, :, 6].sum() > 0
    for q in range(C):
        assert same_bits(got["models"][:, q, 5], start[:, 5])
    ring = [0, 1, 2, 3, 4, 7, 8, 9, 10, 11]
    assert (got["pmark"][:, ring + [5]] == R.IDLE).all() and same_bits(got["models"][:, :, ring], np.broadcast_to(start[:, None, ring], (M + 1, C, 10)))
    assert same_bits(got["models"][M], np.broadcast_to(start[M], (C, 12)))        # the bottom depth stays


def test_block_out_of_box_and_lost_root(h):
    M, K, C = 3, 6, 4
    start, obs, wt, pv0, A = linear_case(M, K)
    c = 4
    N = analytic(M, K, 10.0, start, obs, wt, pv0, A)[0]
    st = block_stage(h, start, obs, wt, C, width=0.06, spread=0.02, shape=analytic_shape(M, 9, c, N), block_every=1)
    begin(st, pv0, A)
    lo, hi = start[:M, c] - F(0.06), start[:M, c] + F(0.06)
    seen = set()
    for sweep in range(1, 41):
        before = st.state()
        st.propose()
        mid = st.state()
        st.forward(pv0, A)
        lost = sweep % 3 == 0
        if lost:
            st.pv[2, K - 1, c] = 0.0                                                # chain 2 loses the root of the last datum
        st.accept()
        after = st.state()
        for q in range(C):
            mark = after["pmark"][q, c]
            seen.add(int(mark))
            if mid["pmark"][q, c] == R.OUT_OF_BOX:                                  # out of the box: only the mark was written
                assert mark == R.OUT_OF_BOX
                for name in R.STATE + B.BLOCK_STATE:
                    if name != "pmark":
                        assert same_bits(mid[name][..., q, c], before[name][..., q, c]), name
            else:
                assert mid["pmark"][q, c] == R.PENDING and mid["pnode"][q, c] == -1
                assert same_bits(mid["pold_all"][:, q, c], before["models"][:M, q, c]) and (mid["models"][:M, q, c] != before["models"][:M, q, c]).all()
            if lost and q == 2 and mid["pmark"][q, c] == R.PENDING:
                assert mark == R.NO_ROOT
            if mark in (R.OUT_OF_BOX, R.NO_ROOT, R.REJECTED):                        # a rejection of any kind: all M nodes are what they were
                assert same_bits(after["models"][:, q, c], before["models"][:, q, c]) and after["phi"][q, c] == before["phi"][q, c] and after["psi"][q, c] == before["psi"][q, c]
            else:
                assert mark == R.ACCEPTED and same_bits(after["models"][:, q, c], mid["models"][:, q, c])
        assert (after["models"][:M, :, c] >= lo[:, None]).all() and (after["models"][:M, :, c] <= hi[:, None]).all()
    assert {R.OUT_OF_BOX, R.NO_ROOT, R.ACCEPTED} <= seen
    s = st.state()
    cnt, bc = s["counters"][:, :, c], s["block_counters"][:, :, c]
    assert (cnt[0] + cnt[1] == 40).all() and (bc[0] == 40).all() and same_bits(bc[1], cnt[0]) and same_bits(bc[2], cnt[2]) and bc[2].sum() > 0
    assert cnt[3, 2] > 0 and not cnt[3, [0, 1, 3]].any()


def test_one_unknown_and_one_chain(h):
    for M, C in ((1, 3), (3, 1), (1, 1)):
        K = 4
        start, obs, wt, pv0, A = linear_case(M, K)
        N = analytic(M, K, 4.0, start, obs, wt, pv0, A)[0]
        if M == 1:
            assert N.shape == (1, 1)
        st = block_stage(h, start, obs, wt, C, burn=10, smooth=4.0, shape=analytic_shape(M, 9, 4, N), block_every=2)
        begin(st, pv0, A)
        st.linear(pv0, A, 60)
        nodes, cols, counts = st.finish()
        bc = st.state()["block_counters"][:, :, 4]
        assert np.isfinite(nodes).all() and counts[7, 4] == 50 and nodes[1][:, 4].min() > 0
        assert (bc[0] == 30).all() and bc[1].sum() > 0 and counts[2, 4] + counts[3, 4] == 60 * C
        if C == 1:
            assert not nodes[3].any() and same_bits(nodes[1][:, 4], nodes[2][:, 4])
        else:
            assert nodes[3][:, 4].min() > 0


# ---- 7. the stand-alone program ----

def test_standalone_program_runs(h, tmp_path):
    """the same file with its own main (the sizes and the special cases stand-alone: what a sanitizer build runs), here in the plain build"""
    exe = str(tmp_path / "hostcheck_column_sample_block")
    subprocess.check_call(["g++"] + B.FLAGS + ["-DHOSTCHECK_COLUMN_SAMPLE_BLOCK_MAIN", "-o", exe, B.SRC, "-lm"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
