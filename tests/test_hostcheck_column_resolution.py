"""The depth resolution of one column (dsurftomo_amd/csrc/column_resolution.h) on the CPU through
tests/hostcheck_column_resolution.cpp, against the NumPy twin depth.column_resolution_twin: random well-posed columns of the sizes the kernel
meets (one unknown, two, a usual column, the stage's limits), some of their data unused with NaN kernels; the solve against the step's
column_solve bit for bit; the identities of exact arithmetic; the step the resolution predicts; the special cases.

The tolerance is measured, not chosen, the way section 21's is: the twin computes every case a second time from numpy.linalg.pinv of the
stacked [diag(a) S; smooth L; damp I], another algorithm on the same numbers, and the largest difference between its two R, relative to
the largest |R| of the case, is the size of the rounding error (MEASURED below, per size).  The header may differ from the twin by four
times the largest of them -- R, R_jj, the leverages and the trace relative to the largest |R|; m1, m2 and var, which carry other units,
relative to their own largest value.  The figure never comes from the header under test."""
import subprocess

import numpy as np
import pytest

from dsurftomo_amd import depth

import column_resolution_ref as CR
import columns_ref
from column_resolution_ref import SIZES, host_resolution, random_column, same_bits

F = np.float32
SMOOTH, DAMP = 0.3, 0.1
SEED = 11
MEASURED, FACTOR, TOL = CR.MEASURED, CR.FACTOR, CR.TOL        # measured on the twin alone: column_resolution_ref.py


@pytest.fixture(scope="module")
def h():
    return CR.load()


def host_one(h, obs, wt, pv, S, depz, smooth=SMOOTH, damp=DAMP, **kw):
    """the header on one column given as the twin takes it; the outputs without the column axis"""
    out = host_resolution(h, obs[:, None], None if wt is None else wt[:, None], pv[:, None], np.ascontiguousarray(S.T)[:, :, None], depz, smooth, damp, **kw)
    return {k: (v[..., 0] if v.ndim > 1 else v[0]) for k, v in out.items()}


def test_against_the_twin(h):
    """nused and flag equal; measures, leverage, trace and the full R within FACTOR * MEASURED.  The measurement is made again and printed,
    not asserted (it is numpy's pinv that would be tested).  In fact the twin runs the header's operations in its order and the two agree
    to the last bit on this compiler; the tolerance is what the comparison is entitled to."""
    for M, K, unused in SIZES:
        obs, wt, pv, S, depz = random_column(M, K, SEED, unused)
        twin = depth.column_resolution_twin(obs, wt, pv, S, depz, SMOOTH, DAMP)
        rmax = np.abs(twin["other"]["R"]).max()
        rel = np.abs(twin["R"] - twin["other"]["R"]).max() / rmax
        got = host_one(h, obs, wt, pv, S, depz)
        diff = CR.differences(got, twin, rmax)
        print("M %2d K %2d: ldlt against pinv %.3g (MEASURED %.3g; all figures: %s); header against the twin: %s" %
              (M, K, rel, MEASURED[(M, K)], " ".join("%s %.2g" % kv for kv in CR.differences(twin, twin["other"], rmax).items()),
               " ".join("%s %.2g" % kv for kv in diff.items())))
        assert got["nused"] == twin["nused"] == K - unused and got["flag"] == twin["flag"] == 0
        assert max(diff.values()) <= TOL, diff
        assert np.abs(got["T"] - twin["T"]).max() <= TOL * np.abs(twin["T"]).max()
        assert np.array_equal(got["measures"][0], np.diag(got["R"]))              # R_jj is the diagonal of the same R, computed once
        assert rmax > 0.1 and np.isfinite(got["R"]).all()


def test_solve_matches_column_solve(h):
    """row k of T is column_system.h's column_solve applied to g_k, bit for bit; rows of unused data are 0.0"""
    for M, K, unused in SIZES:
        obs, wt, pv, S, depz = random_column(M, K, SEED, unused)
        got = host_one(h, obs, wt, pv, S, depz)
        flag, T = CR.rows_by_column_solve(h, obs, wt, pv, S, SMOOTH, DAMP)
        assert flag == 0 and same_bits(got["T"], T)
        used = (wt > 0) & (obs > 0) & (pv > 0)
        assert not got["T"][~used].any() and np.abs(got["T"][used]).min(axis=1).max() > 0


def test_identities(h):
    """what holds in exact arithmetic, to the tolerance of the comparison: the sum of the leverages is the trace (both are tr(N^-1 G^T G)),
    0 <= h_k < 1, var >= 0, and more damping resolves less.  No bound on R_jj: R is not symmetric and its diagonal may leave [0, 1]."""
    for M, K, unused in SIZES:
        obs, wt, pv, S, depz = random_column(M, K, SEED, unused)
        got = host_one(h, obs, wt, pv, S, depz)
        rmax = np.abs(got["R"]).max()
        used = (wt > 0) & (obs > 0) & (pv > 0)
        assert abs(got["leverage"].sum() - got["trace"]) <= TOL * rmax
        assert not got["leverage"][~used].any()
        assert (got["leverage"][used] >= -TOL * rmax).all() and (got["leverage"] < 1.0).all()
        assert (got["measures"][3] >= 0.0).all() and (got["measures"][1] >= 0.0).all() and (got["measures"][2] >= 0.0).all()
        lo = host_one(h, obs, wt, pv, S, depz, damp=0.05)
        hi = host_one(h, obs, wt, pv, S, depz, damp=0.5)
        assert hi["trace"] < lo["trace"] <= min(M, K - unused) + TOL * rmax
        print("M %2d K %2d: trace %.6f at damp 0.05, %.6f at 0.5; R_jj in [%.3g, %.3g]" % (M, K, lo["trace"], hi["trace"], got["measures"][0].min(), got["measures"][0].max()))


def test_resolution_predicts_the_step(h):
    """obs = fl32(pv + S m) for a random m: the step's unclipped delta is R m + T^T e with e_k = a_k (obs_k - pv_k - (S m)_k), the rounding
    of the observations to fp32, formed in fp64 -- the linear algebra of the resolution is that of the step.  Within the tolerance of the
    comparison, relative to the larger of max |delta| and max |R| max |m| (the size of the terms of R m)."""
    hs = columns_ref.load()
    for M, K, unused in SIZES:
        obs, wt, pv, S, depz = random_column(M, K, SEED, unused)
        used = (wt > 0) & (obs > 0) & (pv > 0)
        rng = np.random.default_rng(100 + M)
        m = 0.2 * (rng.random(M) - 0.5)
        Sm = np.zeros(K)
        Sm[used] = S[used] @ m
        obs2 = np.where(obs > 0, (pv + Sm).astype(F), obs).astype(F)              # (an unused datum stays unused for the same reason)
        got = host_one(h, obs2, wt, pv, S, depz)
        vels = np.full((M + 1, 1), 3.0, F)
        step = columns_ref.host_step(hs, obs2[:, None], wt[:, None], pv[:, None], np.ascontiguousarray(S.T)[:, :, None], vels, SMOOTH, DAMP, 1e6, -1e6, 1e6)
        assert step["flag"][0] == 0 and step["nused"][0] == got["nused"] == K - unused
        e = np.zeros(K)
        e[used] = wt[used].astype(np.float64) * (obs2[used].astype(np.float64) - pv[used] - Sm[used])
        want = got["R"] @ m + got["T"].T @ e
        delta = step["delta"][:, 0]
        scale = max(np.abs(delta).max(), np.abs(got["R"]).max() * np.abs(m).max())
        print("M %2d K %2d: max |delta - (R m + T^T e)| / scale = %.3g (max |delta| %.3g, max |T^T e| %.3g)" %
              (M, K, np.abs(delta - want).max() / scale, np.abs(delta).max(), np.abs(got["T"].T @ e).max()))
        assert np.abs(delta - want).max() <= TOL * scale
        assert np.abs(delta).max() > 1e-3


def test_no_data_is_flag_2_whatever_damp_is(h):
    M, K = 4, 5
    obs, wt, pv, S, depz = random_column(M, K, 6)
    for damp in (0.1, 1e3):
        got = host_one(h, obs, np.zeros(K, F), pv, np.full((K, M), np.nan), depz, damp=damp, fill=9.0)
        assert got["flag"] == 2 and got["nused"] == 0 and got["trace"] == 0.0
        assert not got["measures"].any() and not got["leverage"].any() and not got["R"].any()
        twin = depth.column_resolution_twin(obs, np.zeros(K, F), pv, np.full((K, M), np.nan), depz, SMOOTH, damp)
        assert twin["flag"] == 2 and not twin["R"].any() and twin["other"] is None


def test_not_positive_definite_is_flag_1(h):
    """an N made indefinite by hand (second pivot 1 - 4), one with a zero pivot, one with a pivot that is not finite: flag 1 and every
    output 0.0; the twin agrees.  A definite one next to them is resolved."""
    G = np.array([[1.0, 0.5, 0.0], [0.25, 1.0, 0.5]])
    depz = np.array([0.0, 2.0, 5.0], F)
    for N in ([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]], [[1.0, 1.0, 0.0], [1.0, 1.0, 0.0], [0.0, 0.0, 1.0]],
              [[1.0, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, 1.0]], [[np.nan, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]):
        for full in (True, False):
            flag, out = CR.host_finish(h, N, G, depz, full)
            assert flag == 1 and all(not v.any() for v in out.values())
        twin = depth.column_resolution_twin(np.ones(2, F), None, np.ones(2), G, depz, SMOOTH, DAMP, n_override=N)
        assert twin["flag"] == 1 and not twin["R"].any() and not twin["measures"].any() and not twin["leverage"].any() and twin["trace"] == 0.0
    N = (G.T @ G + np.eye(3)).tolist()
    flag, out = CR.host_finish(h, N, G, depz)
    twin = depth.column_resolution_twin(np.ones(2, F), None, np.ones(2), G, depz, SMOOTH, DAMP, n_override=N)
    assert flag == 0 and twin["flag"] == 0 and np.abs(out["R"] - twin["R"]).max() <= TOL * np.abs(twin["R"]).max()
    assert np.abs(out["R"] - np.linalg.solve(np.array(N), G.T @ G)).max() <= 1e-14


def test_unused_data_change_nothing(h):
    """three more data -- no weight, no observation, no root -- with NaN kernels: every output has the bits of the call without them, their
    leverages and rows of T are 0.0"""
    M, K = 7, 12
    obs, wt, pv, S, depz = random_column(M, K, 5)
    base = host_one(h, obs, wt, pv, S, depz)
    at = [0, 5, 14]                                                                # (positions of the extra data among the 15)
    keep = np.setdiff1d(np.arange(K + 3), at)
    obs2 = np.ones(K + 3, F); wt2 = np.ones(K + 3, F); pv2 = np.full(K + 3, 3.0); S2 = np.full((K + 3, M), np.nan)
    obs2[keep], wt2[keep], pv2[keep], S2[keep] = obs, wt, pv, S
    wt2[at[0]] = 0.0; obs2[at[1]] = 0.0; pv2[at[2]] = 0.0
    got = host_one(h, obs2, wt2, pv2, S2, depz, fill=9.0)
    assert got["nused"] == K and got["flag"] == 0
    for name in ("measures", "R", "trace"):
        assert same_bits(np.asarray(got[name]), np.asarray(base[name])), name
    assert same_bits(got["leverage"][keep], base["leverage"]) and same_bits(got["T"][keep], base["T"])
    assert not got["leverage"][at].any() and not got["T"][at].any()
    twin = depth.column_resolution_twin(obs2, wt2, pv2, S2, depz, SMOOTH, DAMP)
    assert twin["nused"] == K and np.isfinite(twin["R"]).all() and np.isfinite(twin["other"]["R"]).all()
    assert max(CR.differences(got, twin, np.abs(twin["R"]).max()).values()) <= TOL


def test_r_null_changes_no_other_bit(h):
    for M, K, unused in SIZES:
        obs, wt, pv, S, depz = random_column(M, K, SEED, unused)
        a = host_one(h, obs, wt, pv, S, depz)
        b = host_one(h, obs, wt, pv, S, depz, full=False)
        assert "R" not in b
        for name in ("measures", "leverage", "trace", "nused", "flag", "T"):
            assert same_bits(np.asarray(a[name]), np.asarray(b[name])), name


def test_a_column_among_others_and_the_mask(h):
    """columns side by side with the engine's strides: each equals the column alone; a column masked out keeps what it held"""
    M, K, n = 3, 4, 5
    cols = [random_column(M, K, 20 + c) for c in range(n)]
    obs = np.stack([c[0] for c in cols], axis=1); wt = np.stack([c[1] for c in cols], axis=1); pv = np.stack([c[2] for c in cols], axis=1)
    S = np.stack([c[3].T for c in cols], axis=2); depz = cols[0][4]
    only = np.array([1, 0, 1, 1, 0], np.uint8)
    got = host_resolution(h, obs, wt, pv, S, depz, SMOOTH, DAMP, only, fill=9.0)
    for c in range(n):
        if not only[c]:
            assert (got["measures"][:, :, c] == 9.0).all() and (got["R"][:, :, c] == 9.0).all() and got["trace"][c] == 9.0
            continue
        one = host_one(h, cols[c][0], cols[c][1], cols[c][2], cols[c][3], depz)
        assert same_bits(one["R"], got["R"][:, :, c]) and same_bits(one["measures"], got["measures"][:, :, c]) and same_bits(one["leverage"], got["leverage"][:, c])
        assert one["trace"] == got["trace"][c]
    nowt = host_resolution(h, obs, None, pv, S, depz, SMOOTH, DAMP)
    ones = host_resolution(h, obs, np.ones_like(wt), pv, S, depz, SMOOTH, DAMP)
    assert same_bits(nowt["R"], ones["R"]) and same_bits(nowt["leverage"], ones["leverage"])     # no weights: all 1
    assert CR.load().hcr_doubles(63, 60) == 2016 + 3780 + 120 + 189 + 3780


def test_the_stand_alone_program_runs(tmp_path):
    """the same file as a program with its own main (what a sanitizer build runs): it checks the special cases itself"""
    exe = str(tmp_path / "hostcheck_column_resolution")
    subprocess.check_call(["g++"] + [f for f in columns_ref.FLAGS if f != "-fPIC"] + ["-DHOSTCHECK_COLUMN_RESOLUTION_MAIN", "-o", exe, CR.SRC, "-lm"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
