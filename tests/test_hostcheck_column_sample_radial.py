"""The Monte-Carlo radial depth inversion (dsurftomo_amd/csrc/column_sample_radial.h) on the CPU through
tests/hostcheck_column_sample_radial.cpp: the header against the Python twin depth_twins.column_sample_radial_twin bit for bit, the sampler's
law on a linear forward function -- where the posterior of [Vsv ; Vsh] is Gaussian with column_radial_twin's normal matrix at damp 0 as its
precision -- and the special cases.

The law test's margins come from the run itself: the standard error of a pooled figure (mean, variance, cov(Vsv_l, Vsh_l), mean of xi) is the
scatter of the 64 chains' own figures over sqrt(64); the pooled figure must lie within 5 of them of the analytic one.  Lengths used: 64
chains, LAW_SWEEPS sweeps, burn LAW_BURN, at (M, K) = (3, 6) and (5, 12), aniso 0 and strong.  They were chosen on this CPU build (which is
the twin's arithmetic bit for bit) and the worst ratios seen are in DESIGN.md section 37."""
import math
import subprocess

import numpy as np
import pytest

import column_sample_radial_ref as R
from dsurftomo_amd import depth, depth_twins

F = np.float32
WIDE = dict(width=5.0, minvel=0.05, maxvel=10.0)
LAW_SWEEPS, LAW_BURN = 12000, 3000
RING = [0, 1, 2, 3, 5, 6, 7, 8]                                                      # of a 3 x 3 grid; column 4 is the interior one


@pytest.fixture(scope="module")
def h():
    return R.load()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def linear_case(M, K, nx=3, ny=3, seed=5, sigma=0.02, equal=False):
    """a linear problem on every column: pv = pv0 + A (v - start), v the Vsh at a Love slot and the Vsv at a Rayleigh slot, the slots
    interleaved (odd slots Love); kernels of the size of real ones, observations a few sigma off pv0, weights 1 / sigma; Vsh starts up to 4 %
    above Vsv (equal: on it)"""
    rng = np.random.default_rng(seed + 100 * M + K)
    ncol = nx * ny
    start_v = (3.0 + 0.5 * rng.random((M + 1, ncol))).astype(F)
    start_h = start_v.copy() if equal else (start_v * (1.0 + 0.04 * rng.random((M + 1, ncol)))).astype(F)
    A = rng.random((K, M, ncol)) * (2.0 / M)
    pv0 = 3.0 + rng.random((K, ncol))
    obs = (pv0 + 2.0 * sigma * rng.standard_normal((K, ncol))).astype(F)
    wt = np.full((K, ncol), 1.0 / sigma, F)
    love = np.arange(K) % 2 == 1
    return start_v, start_h, obs, wt, love, pv0, A


def stage(h, case, C, nx=3, ny=3, smooth=10.0, aniso=5.0, step=0.05, spread=0.05, temperature=1.0, seed=77, burn=0, width=5.0, minvel=0.05, maxvel=10.0, pairs=True):
    start_v, start_h, obs, wt, love = case[:5]
    return R.Stage(h, nx, ny, start_v, start_h, obs, wt, love, C, smooth, aniso, step, spread, width, temperature, minvel, maxvel, seed, burn, pairs)


def begin(st, pv0, A):
    st.setup_models()
    st.forward(pv0, A)
    st.setup_state()


# ---- 1. the header against the twin, bit for bit ----

@pytest.mark.parametrize("pairs", [True, False])
@pytest.mark.parametrize("M,K,C", [(1, 2, 2), (2, 4, 1), (3, 6, 3), (7, 12, 2)])
def test_header_equals_the_twin(h, M, K, C, pairs):
    nx, ny = 4, 3
    case = linear_case(M, K, nx, ny)
    start_v, start_h, obs, wt, love, pv0, A = case
    wt[:, 5] *= F(0.5)
    wt[1, 6] = 0.0
    args = dict(smooth=3.0, aniso=4.0, step=0.08, spread=0.05, temperature=1.5, seed=2 ** 40 + 9, burn=5, width=0.12, minvel=2.9, maxvel=3.7, pairs=pairs)
    st = stage(h, case, C, nx, ny, **args)
    begin(st, pv0, A)
    fw = stage(h, case, C, nx, ny, **args)

    def forward(vsv, vsh):
        fw.a["vsv"][...] = vsv; fw.a["vsh"][...] = vsh
        fw.forward(pv0, A)
        return fw.pv.copy()

    sweeps = 30
    st.linear(pv0, A, sweeps)
    tw = depth_twins.column_sample_radial_twin(nx, ny, start_v, start_h, obs, wt, love, forward, C, sweeps, args["burn"], args["smooth"], args["aniso"], args["step"],
                                               args["spread"], args["width"], args["temperature"], args["minvel"], args["maxvel"], args["seed"], pairs=pairs)
    state = st.state()
    for name in R.STATE:
        assert same_bits(state[name], tw[name]), name
    fin = st.finish()
    for name in R.NODES + ("best_energy", "mean_phi"):
        assert same_bits(fin[name], tw[name]), name
    assert same_bits(fin["phi_start"], tw["phi_start"])
    assert (fin["nused_r"] == tw["nused_r"]).all() and (fin["nused_l"] == tw["nused_l"]).all() and (fin["flag"] == tw["flag"]).all()
    assert (fin["nkept"] == tw["nkept"][0]).all() and (fin["reseeded"] == tw["reseeded"].sum(axis=0)).all()
    for w, name in enumerate(("accepted", "rejected", "out_of_box", "no_root")):
        assert (fin[name] == tw["counters"][w].sum(axis=0)).all(), name
    for w, name in enumerate(R.COUNTS[7:13]):
        assert (fin[name] == tw["kinds"][w].sum(axis=0)).all(), name
    assert (state["counters"][2] > 0).any() and (state["counters"][0] > 0).any()           # the narrow box was hit, and moves were made
    assert (state["kinds"][2] > 0).any() == pairs and not state["kinds"][:, :, [0, 1, 2, 3, 4, 7, 8, 9, 10, 11]].any()
    if C == 1:
        assert not fin["B_v"].any() and not fin["B_h"].any() and not fin["B_xi"].any()


# ---- 2. the sampler's law ----

def analytic(case, c, smooth, aniso):
    """the Gaussian posterior of [Vsv ; Vsh] of column c: precision N = column_radial_twin's normal matrix at damp 0, mean = start + N^-1 b"""
    start_v, start_h, obs, wt, love, pv0, A = case
    M = start_v.shape[0] - 1
    a = wt[:, c].astype(np.float64)
    G = a[:, None] * A[:, :, c]
    rho = a * (obs[:, c].astype(np.float64) - pv0[:, c])
    v = np.concatenate([start_v[:M, c], start_h[:M, c]]).astype(np.float64)
    d = v[M:] - v[:M]
    used = np.ones(len(a), bool)
    N, b = depth_twins._twin_radial_normal(G, used, love, rho, smooth ** 2, 0.0, aniso ** 2, d)
    LtL = depth.column_ltl(M).astype(np.float64)
    b = b - smooth ** 2 * np.concatenate([LtL @ v[:M], LtL @ v[M:]])                 # the step's b holds the data and the tie; the prior acts on the model itself
    cov = np.linalg.inv(N)
    return v + cov @ b, cov, N


def law_figures(st, case, c, smooth, aniso, sweeps, burn):
    """the worst ratios |pooled - analytic| / se of the means, the variances, cov(Vsv_l, Vsh_l) and the mean of xi, the worst R-hat and the
    acceptance per kind"""
    C, M = st.C, st.M
    n = sweeps - burn
    fin = st.finish()
    s = st.state()
    assert fin["nkept"][c] == n and fin["flag"][c] == 0
    mean, cov, _ = analytic(case, c, smooth, aniso)
    m_v, m_h = s["S1v"][:, :, c] / n, s["S1h"][:, :, c] / n                        # (M, C): the chains' own figures
    v_v, v_h = s["S2v"][:, :, c] / n - m_v ** 2, s["S2h"][:, :, c] / n - m_h ** 2
    c_q = s["Pvh"][:, :, c] / n - m_v * m_h
    x_q = s["X1"][:, :, c] / n
    se = lambda x: x.std(axis=1, ddof=1) / math.sqrt(C)
    r = dict(mean=max((np.abs(fin["mean_v"][:, c] - mean[:M]) / se(m_v)).max(), (np.abs(fin["mean_h"][:, c] - mean[M:]) / se(m_h)).max()),
             var=max((np.abs(fin["var_v"][:, c] - np.diag(cov)[:M]) / se(v_v)).max(), (np.abs(fin["var_h"][:, c] - np.diag(cov)[M:]) / se(v_h)).max()),
             cov=(np.abs(fin["cov_vh"][:, c] - cov[np.arange(M), M + np.arange(M)]) / se(c_q)).max())
    # xi = (h / v)^2 to second order about the Gaussian mean (mv, mh): xi(m) + (1/2) (xi_vv var_v + 2 xi_vh cov + xi_hh var_h)
    mv, mh = mean[:M], mean[M:]
    svv, shh, svh = np.diag(cov)[:M], np.diag(cov)[M:], cov[np.arange(M), M + np.arange(M)]
    xi2 = (mh / mv) ** 2 + 0.5 * (6.0 * mh ** 2 / mv ** 4 * svv - 8.0 * mh / mv ** 3 * svh + 2.0 / mv ** 2 * shh)
    r["xi"] = (np.abs(fin["mean_xi"][:, c] - xi2) / se(x_q)).max()
    rhat = np.concatenate([depth.sample_rhat(fin["W_" + t][:, c], fin["B_" + t][:, c], n) for t in ("v", "h", "xi")])
    kinds = s["kinds"][:, :, c].sum(axis=1)
    acc = [kinds[3 + k] / kinds[k] if kinds[k] else float("nan") for k in range(3)]
    return r, rhat, acc, np.sqrt(np.diag(cov))


def strong_tie(case, c):
    """the aniso at which the tie's precision equals the largest data precision: the largest diagonal entry of G^T G of either block"""
    start_v, start_h, obs, wt, love, pv0, A = case
    G = wt[:, c].astype(np.float64)[:, None] * A[:, :, c]
    return math.sqrt(max((G[~love] ** 2).sum(axis=0).max(), (G[love] ** 2).sum(axis=0).max()))


@pytest.mark.parametrize("strong", [False, True])
@pytest.mark.parametrize("M,K", [(3, 6), (5, 12)])
def test_law_on_a_linear_forward_function(h, M, K, strong):
    C, smooth, c = 64, 10.0, 4
    case = linear_case(M, K)
    aniso = strong_tie(case, c) if strong else 0.0
    st = stage(h, case, C, smooth=smooth, aniso=aniso, burn=LAW_BURN, **WIDE)
    begin(st, case[5], case[6])
    st.linear(case[5], case[6], LAW_SWEEPS)
    r, rhat, acc, sd = law_figures(st, case, c, float(F(smooth)), float(F(aniso)), LAW_SWEEPS, LAW_BURN)
    print("M %d K %d aniso %.3f: %d chains, %d sweeps, burn %d: worst ratio mean %.2f var %.2f cov %.2f xi %.2f, worst R-hat %.4f, accepted Vsv %.1f %% Vsh %.1f %% pair %.1f %%, sd %.4f .. %.4f"
          % (M, K, aniso, C, LAW_SWEEPS, LAW_BURN, r["mean"], r["var"], r["cov"], r["xi"], rhat.max(), 100 * acc[0], 100 * acc[1], 100 * acc[2], sd.min(), sd.max()))
    assert r["mean"] <= 5.0 and r["var"] <= 5.0 and r["cov"] <= 5.0
    assert r["xi"] <= 5.0
    assert (rhat < 1.1).all()
    fin = st.finish()
    assert all(np.isfinite(fin[n]).all() and not fin[n][:, RING].any() for n in R.NODES)      # the ring: nothing kept, zeros
    if strong:                                                                     # recorded, not a condition: the same run without the pair moves
        st2 = stage(h, case, C, smooth=smooth, aniso=aniso, burn=LAW_BURN, pairs=False, **WIDE)
        begin(st2, case[5], case[6])
        st2.linear(case[5], case[6], LAW_SWEEPS)
        rhat2 = law_figures(st2, case, c, float(F(smooth)), float(F(aniso)), LAW_SWEEPS, LAW_BURN)[1]
        print("M %d K %d strong tie: worst R-hat with pairs %.4f, without %.4f" % (M, K, rhat.max(), rhat2.max()))


# ---- 3. the special cases ----

def test_out_of_box_of_every_kind_and_lost_roots(h):
    M, K, C = 3, 6, 6
    case = linear_case(M, K)
    start_v, start_h, obs, wt, love, pv0, A = case
    st = stage(h, case, C, step=0.1, width=0.05, spread=0.02, minvel=0.05, maxvel=10.0, aniso=1.0)
    begin(st, pv0, A)
    c = 4
    box = {0: (start_v[:M, c] - F(0.05), start_v[:M, c] + F(0.05)), 1: (start_h[:M, c] - F(0.05), start_h[:M, c] + F(0.05))}
    inside = lambda b, l, x: box[b][0][l] <= x <= box[b][1][l]
    seen, out_kinds, one_member_out, lost = set(), set(), 0, {0: 0, 1: 0}
    for sweep in range(1, 121):
        before = st.state()
        st.propose()
        st.forward(pv0, A)
        lose = sweep % 5 == 0
        k_lost = 0 if sweep % 10 == 0 else 1                                         # a Rayleigh slot, then a Love slot
        if lose:
            st.pv[2, k_lost, c] = 0.0
        mid = st.state()
        st.accept()
        after = st.state()
        for q in range(C):
            mark = after["pmark"][q, c]
            seen.add(int(mark))
            kind = int(np.flatnonzero(mid["kinds"][:3, q, c] - before["kinds"][:3, q, c])[0])
            if mid["pmark"][q, c] == R.OUT_OF_BOX:
                assert mark == R.OUT_OF_BOX
                out_kinds.add(kind)
                for name in ("vsv", "vsh", "pnode", "pold_v", "pold_h"):                 # nothing but the mark and the kind's count was written
                    assert same_bits(mid[name][..., q, c], before[name][..., q, c]), name
                if kind == 2:                                                        # which of the pair's members left: replay the proposal
                    u0 = depth.sample_unit(depth.sample_bits(77, c, q, sweep, 0)); u1 = depth.sample_unit(depth.sample_bits(77, c, q, sweep, 1))
                    l = min(int(u0 * 3 * M), 3 * M - 1) - 2 * M
                    fd = F(float(F(0.1)) * (2.0 * u1 - 1.0))
                    outs = [not inside(0, l, F(before["vsv"][l, q, c] + fd)), not inside(1, l, F(before["vsh"][l, q, c] + fd))]
                    assert any(outs)
                    one_member_out += outs[0] != outs[1]
            else:
                assert int(mid["pnode"][q, c]) // M == kind
            if lose and q == 2 and mid["pmark"][q, c] == R.PENDING:
                assert mark == R.NO_ROOT
                lost[k_lost] += 1
            if mark in (R.OUT_OF_BOX, R.NO_ROOT, R.REJECTED):                        # a rejection of any kind: the chain is what it was
                assert same_bits(after["vsv"][:, q, c], before["vsv"][:, q, c]) and same_bits(after["vsh"][:, q, c], before["vsh"][:, q, c])
                assert after["phi"][q, c] == before["phi"][q, c] and after["psi"][q, c] == before["psi"][q, c]
            else:
                assert mark == R.ACCEPTED
                moved_v = not same_bits(after["vsv"][:, q, c], before["vsv"][:, q, c]); moved_h = not same_bits(after["vsh"][:, q, c], before["vsh"][:, q, c])
                assert (moved_v, moved_h) == ((True, False), (False, True), (True, True))[kind]
        for b, name in enumerate(("vsv", "vsh")):
            assert (after[name][:M, :, c] >= box[b][0][:, None]).all() and (after[name][:M, :, c] <= box[b][1][:, None]).all()
    assert {R.OUT_OF_BOX, R.NO_ROOT, R.ACCEPTED} <= seen and out_kinds == {0, 1, 2} and one_member_out > 0 and lost[0] > 0 and lost[1] > 0
    s = st.state()
    cnt, kinds = s["counters"][:, :, c], s["kinds"][:, :, c]
    assert (cnt[0] + cnt[1] == 120).all() and (kinds[:3].sum(axis=0) == 120).all() and (kinds[3:].sum(axis=0) == cnt[0]).all()
    assert cnt[3, 2] == lost[0] + lost[1] and not cnt[3, [0, 1, 3, 4, 5]].any()
    assert (s["pmark"][:, RING] == R.IDLE).all()


def test_unused_datum_with_nan_changes_no_bit(h):
    M, K, C = 3, 6, 3
    case = linear_case(M, K)
    case[3][2, 4] = 0.0                                                              # datum 2 of the interior column is unused
    runs = []
    for poison in (False, True):
        st = stage(h, case, C, burn=3)
        st.setup_models()
        st.forward(case[5], case[6])
        if poison:
            st.pv[:, 2, 4] = np.nan
        st.setup_state()
        for sweep in range(12):
            st.propose()
            st.forward(case[5], case[6])
            if poison:
                st.pv[:, 2, 4] = np.nan
            st.accept()
        runs.append((st.state(), st.finish()))
    for name in R.STATE:
        assert same_bits(runs[0][0][name], runs[1][0][name]), name
    for name in runs[0][1]:
        assert same_bits(runs[0][1][name], runs[1][1][name]) and np.isfinite(runs[0][1][name]).all(), name
    assert runs[0][1]["nused_r"][4] == K // 2 - 1 and runs[0][1]["nused_l"][4] == K // 2


def test_no_datum_is_flagged_and_one_type_alone_samples(h):
    M, K, C = 3, 6, 3
    case = linear_case(M, K, 4, 3)
    start_v, start_h, obs, wt, love, pv0, A = case
    wt[:, 5] = 0.0                                                                   # interior column 5: no datum
    wt[~love, 6] = 0.0                                                               # interior column 6: only Love data
    st = stage(h, case, C, 4, 3, burn=2)
    begin(st, pv0, A)
    st.linear(pv0, A, 40)
    s, fin = st.state(), st.finish()
    assert fin["flag"][5] == 2 and fin["nused_r"][5] == 0 and fin["nused_l"][5] == 0 and fin["nkept"][5] == 0
    for q in range(C):
        assert same_bits(s["vsv"][:, q, 5], start_v[:, 5]) and same_bits(s["vsh"][:, q, 5], start_h[:, 5])
    assert not s["counters"][:, :, 5].any() and not s["kinds"][:, :, 5].any() and (s["pmark"][:, 5] == R.IDLE).all()
    assert not any(fin[n][:, 5].any() for n in R.NODES)
    assert fin["flag"][6] == 0 and fin["nused_r"][6] == 0 and fin["nused_l"][6] == K // 2 and fin["nkept"][6] == 38
    assert fin["accepted_v"][6] > 0 and fin["accepted_h"][6] > 0 and fin["var_v"][:, 6].min() > 0          # the prior and the tie hold the Vsv block
    assert same_bits(s["vsv"][M], np.broadcast_to(start_v[M], (C, 12))) and same_bits(s["vsh"][M], np.broadcast_to(start_h[M], (C, 12)))      # the bottom depth stays


def test_one_unknown_and_one_chain(h):
    for M, C in ((1, 3), (3, 1), (1, 1)):
        K = 4
        case = linear_case(M, K)
        st = stage(h, case, C, burn=10, smooth=4.0, aniso=3.0)
        begin(st, case[5], case[6])
        s = st.state()
        if M == 1:                                                                   # only the tie term
            d = float(case[1][0, 4]) - float(case[0][0, 4])
            assert s["psi"][0, 4] == float(F(3.0)) ** 2 * (d * d)
        st.linear(case[5], case[6], 80)
        fin = st.finish()
        assert all(np.isfinite(fin[n]).all() for n in R.NODES) and fin["nkept"][4] == 70 and fin["var_v"][:, 4].min() > 0 and fin["var_h"][:, 4].min() > 0
        for t in ("v", "h", "xi"):
            if C == 1:
                assert not fin["B_" + t].any() and same_bits(fin["var_" + t][:, 4], fin["W_" + t][:, 4])      # one chain: B = 0, the pooled variance is W
            else:
                assert fin["B_" + t][:, 4].min() > 0
        assert fin["accepted"][4] + fin["rejected"][4] == 80 * C
        assert fin["proposed_v"][4] + fin["proposed_h"][4] + fin["proposed_pair"][4] == 80 * C


def test_reseeded_chain(h):
    M, K, C = 3, 6, 4
    case = linear_case(M, K)
    start_v, start_h, obs, wt, love, pv0, A = case
    st = stage(h, case, C, spread=0.1)
    st.setup_models()
    assert not same_bits(st.a["vsv"][:M, 2, 4], start_v[:M, 4]) and not same_bits(st.a["vsh"][:M, 2, 4], start_h[:M, 4])
    st.forward(pv0, A)
    st.pv[2, 3, 4] = 0.0                                                             # chain 2 starts where datum 3 has no root
    st.setup_state()
    s = st.state()
    assert (s["reseeded"][:, 4] == [0, 0, 1, 0]).all() and same_bits(s["vsv"][:, 2, 4], start_v[:, 4]) and same_bits(s["vsh"][:, 2, 4], start_h[:, 4])
    assert s["phi"][2, 4] == s["phi"][0, 4] and s["psi"][2, 4] == s["psi"][0, 4] and s["phi"][1, 4] != s["phi"][0, 4]
    fin = st.finish()
    assert fin["reseeded"][4] == 1 and fin["nused_r"][4] + fin["nused_l"][4] == K and fin["phi_start"][4] == s["phi"][0, 4]
    st.setup_models(); st.forward(pv0, A); st.pv[0, 1, 4] = 0.0                      # chain 0 itself without a root at a Love slot: the datum is not used
    st.setup_state()
    fin = st.finish()
    assert fin["nused_l"][4] == K // 2 - 1 and fin["nused_r"][4] == K // 2


def test_nothing_kept_gives_zeros(h):
    M, K, C = 3, 6, 3
    case = linear_case(M, K)
    st = stage(h, case, C, burn=15)
    begin(st, case[5], case[6])
    st.linear(case[5], case[6], 15)
    fin = st.finish()
    assert not any(fin[n].any() for n in R.NODES) and not fin["best_energy"].any() and not fin["mean_phi"].any()
    assert fin["phi_start"][4] > 0 and fin["nkept"].max() == 0 and fin["accepted"][4] + fin["rejected"][4] == 15 * C
    st.linear(case[5], case[6], 1)
    fin = st.finish()
    assert fin["nkept"][4] == 1 and fin["mean_v"][:, 4].all() and fin["mean_xi"][:, 4].all() and not fin["W_v"][:, 4].any() and not fin["W_xi"][:, 4].any()
    assert all(np.isfinite(fin[n]).all() for n in R.NODES)                           # one kept sweep: W = 0, not NaN
    assert (depth.sample_rhat(fin["W_xi"], fin["B_xi"], fin["nkept"][None]) == 1.0).all()


def test_equal_starts_give_xi_one_and_no_tie(h):
    M, K, C = 3, 6, 2
    case = linear_case(M, K, equal=True)
    # a box so narrow that every proposal leaves it: the chains stay on the start, and the kept sweep sees xi = xi0
    with_tie = stage(h, case, C, aniso=7.0, spread=0.0, burn=0, step=0.3, width=1e-6)
    without = stage(h, case, C, aniso=0.0, spread=0.0, burn=0, step=0.3, width=1e-6)
    for st in (with_tie, without):
        begin(st, case[5], case[6])
    assert same_bits(with_tie.state()["psi"], without.state()["psi"]) and with_tie.state()["psi"][0, 4] > 0      # a zero tie term
    with_tie.linear(case[5], case[6], 3)
    fin = with_tie.finish()
    assert fin["out_of_box"][4] == 3 * C and fin["nkept"][4] == 3
    assert (fin["mean_xi"][:, 4] == 1.0).all() and not fin["var_xi"][:, 4].any() and not fin["p_pos"][:, 4].any() and not fin["cov_vh"][:, 4].any()


# ---- 4. the stand-alone program ----

def test_standalone_program_runs(h, tmp_path):
    """the same file with its own main (the sizes and the special cases stand-alone: what a sanitizer build runs), here in the plain build"""
    exe = str(tmp_path / "hostcheck_column_sample_radial")
    subprocess.check_call(["g++"] + R.FLAGS + ["-DHOSTCHECK_COLUMN_SAMPLE_RADIAL_MAIN", "-o", exe, R.SRC, "-lm"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
