"""The depth step of one column (dsurftomo_amd/csrc/column_system.h) on the CPU through tests/hostcheck_columns.cpp,
against the NumPy twin depth.column_step_twin, which builds the regulariser L explicitly: the closed form of L^T L, the step on random
well-posed columns of the sizes the kernel meets (one unknown, two, a usual column, the stage's limits), and the special cases -- data that
must not be read, a column without data, a matrix that is not positive definite, the clips.

The tolerance of the comparison is measured, not chosen: the twin solves every case a second time with numpy.linalg.lstsq on the stacked
system [diag(a) S; smooth L; damp I], another algorithm on the same numbers, and the largest relative difference between its two answers is
the size of the rounding error of a step (MEASURED below).  The header may differ from the twin by four times that."""
import subprocess

import numpy as np
import pytest

import _libs as L
from dsurftomo_amd import depth

import columns_ref
from columns_ref import FLAGS, SRC, host_step

F = np.float32
SIZES = [(1, 1), (2, 3), (7, 12), (63, 60)]                    # (M, K)
SMOOTH, DAMP, DVMAX, MINVEL, MAXVEL = 0.3, 0.1, 0.25, 2.0, 5.0
# largest relative difference max |delta_ldlt - delta_lstsq| / max |delta_lstsq| over SIZES with seed 11 (the (63, 60) case; printed by
# test_step_against_the_twin), and the factor that covers other seeds
MEASURED = 6.8e-15
FACTOR = 4.0


@pytest.fixture(scope="module")
def h():
    return columns_ref.load()


def random_column(M, K, seed):
    """a well-posed column: positive kernels of the size of real ones (a datum's kernel sums to about one over depth), weights around 1,
    residuals of a few per cent"""
    rng = np.random.default_rng(seed)
    S = rng.random((K, M)) * (2.0 / M)
    pv = 3.0 + rng.random(K)
    obs = (pv * (1.0 + 0.03 * rng.standard_normal(K))).astype(F)
    wt = (0.5 + rng.random(K)).astype(F)
    vels = (3.0 + rng.random(M + 1)).astype(F)
    return obs, wt, pv, S, vels


@pytest.mark.parametrize("M", [1, 2, 3, 4, 9, 63])
def test_ltl_closed_form(h, M):
    want = depth.column_ltl(M)
    got = np.array([[h.hcc_ltl(M, l, lp) for lp in range(M)] for l in range(M)])
    assert (got == want).all()
    assert (got == got.T).all() and h.hcc_ltl(M, M, 0) == 0 and h.hcc_ltl(M, 0, -1) == 0
    if M >= 2:
        assert not got.sum(axis=1).any()                                           # every row of L sums to zero: a constant is not penalised
    assert depth.column_l(M).shape == ((0, 1) if M == 1 else (M, M))


def test_packed_rows(h):
    e = 0
    for i in range(63):
        for j in range(i + 1):
            assert h.hcc_tri_row(e) == i
            e += 1
    assert e == 2016


def test_step_against_the_twin(h):
    """nused and flag equal, delta and chi2 within FACTOR * MEASURED, dv within that and one rounding to fp32; the measurement is made again
    and printed, not asserted (it is numpy's lstsq that would be tested).  In fact the twin runs column_system.h's operations in its order,
    and the two agree to the last bit on this compiler; the tolerance is what the comparison is entitled to."""
    tol = FACTOR * MEASURED
    worst = 0.0
    for M, K in SIZES:
        obs, wt, pv, S, vels = random_column(M, K, 11)
        twin = depth.column_step_twin(obs, wt, pv, S, vels, SMOOTH, DAMP, DVMAX, MINVEL, MAXVEL)
        other = depth.column_step_twin(obs, wt, pv, S, vels, SMOOTH, DAMP, DVMAX, MINVEL, MAXVEL, solver="lstsq")
        scale = np.abs(other["delta"]).max()
        rel = np.abs(twin["delta"] - other["delta"]).max() / scale
        worst = max(worst, rel)
        got = host_step(h, obs[:, None], wt[:, None], pv[:, None], S.T[:, :, None], vels[:, None], SMOOTH, DAMP, DVMAX, MINVEL, MAXVEL)
        d_delta = np.abs(got["delta"][:, 0] - twin["delta"]).max() / scale
        d_chi2 = abs(got["chi2"][0] - twin["chi2"]) / twin["chi2"]
        print("M %2d K %2d: ldlt against lstsq %.3g; header against the twin: delta %.3g chi2 %.3g, dv bits differ at %d of %d" %
              (M, K, rel, d_delta, d_chi2, int((got["dv"][:, 0].view(np.uint32) != twin["dv"].view(np.uint32)).sum()), M))
        assert got["nused"][0] == twin["nused"] == K and got["flag"][0] == twin["flag"] == 0
        assert d_delta <= tol and d_chi2 <= tol
        assert (np.abs(got["dv"][:, 0].astype(np.float64) - twin["dv"]) <= tol * scale + np.spacing(np.abs(twin["dv"]))).all()
        assert (np.abs(got["vels"][:, 0].astype(np.float64) - twin["vels"]) <= tol * scale + np.spacing(twin["vels"])).all()
        assert got["vels"][M, 0] == vels[M]                                       # the bottom depth is kept
        assert np.abs(twin["dv"]).max() > 0
    print("largest ldlt-against-lstsq difference %.3g (MEASURED = %.3g)" % (worst, MEASURED))


def test_unused_data_change_nothing(h):
    """three more data -- no weight, no observation, no root -- with NaN kernels: every output has the bits of the step without them"""
    M, K = 7, 12
    obs, wt, pv, S, vels = random_column(M, K, 5)
    base = host_step(h, obs[:, None], wt[:, None], pv[:, None], S.T[:, :, None], vels[:, None], SMOOTH, DAMP, DVMAX, MINVEL, MAXVEL)
    at = [0, 5, 14]                                                                # (positions of the extra data among the 15)
    keep = np.setdiff1d(np.arange(K + 3), at)
    obs2 = np.ones(K + 3, F); wt2 = np.ones(K + 3, F); pv2 = np.full(K + 3, 3.0); S2 = np.full((K + 3, M), np.nan)
    obs2[keep], wt2[keep], pv2[keep], S2[keep] = obs, wt, pv, S
    wt2[at[0]] = 0.0; obs2[at[1]] = 0.0; pv2[at[2]] = 0.0
    got = host_step(h, obs2[:, None], wt2[:, None], pv2[:, None], S2.T[:, :, None], vels[:, None], SMOOTH, DAMP, DVMAX, MINVEL, MAXVEL)
    assert got["nused"][0] == K and got["flag"][0] == 0
    for name in ("dv", "vels", "chi2", "delta"):
        assert np.array_equal(got[name].view(np.uint8), base[name].view(np.uint8)), name
    twin = depth.column_step_twin(obs2, wt2, pv2, S2, vels, SMOOTH, DAMP, DVMAX, MINVEL, MAXVEL)
    assert twin["nused"] == K and np.isfinite(twin["delta"]).all()
    assert np.abs(got["delta"][:, 0] - twin["delta"]).max() <= FACTOR * MEASURED * np.abs(twin["delta"]).max()
    # a negative observation and a negative curve are not used either
    obs2[at[1]] = -3.0; pv2[at[2]] = -1.0
    again = host_step(h, obs2[:, None], wt2[:, None], pv2[:, None], S2.T[:, :, None], vels[:, None], SMOOTH, DAMP, DVMAX, MINVEL, MAXVEL)
    assert np.array_equal(again["dv"].view(np.uint32), base["dv"].view(np.uint32))


def test_no_data_is_flag_2_whatever_damp_is(h):
    M, K = 4, 5
    obs, wt, pv, S, vels = random_column(M, K, 6)
    for damp in (0.1, 1e3):
        got = host_step(h, obs[:, None], np.zeros((K, 1), F), pv[:, None], np.full((M, K, 1), np.nan), vels[:, None], SMOOTH, damp, DVMAX, MINVEL, MAXVEL)
        assert got["flag"][0] == 2 and got["nused"][0] == 0 and got["chi2"][0] == 0.0
        assert not got["dv"].any() and np.array_equal(got["vels"][:, 0], vels)
        twin = depth.column_step_twin(obs, np.zeros(K, F), pv, np.full((K, M), np.nan), vels, SMOOTH, damp, DVMAX, MINVEL, MAXVEL)
        assert twin["flag"] == 2 and np.array_equal(twin["vels"], vels)


def test_a_column_among_others_and_the_mask(h):
    """columns side by side with the engine's strides: each equals the column alone; a column masked out keeps its zeros"""
    M, K, n = 3, 4, 5
    cols = [random_column(M, K, 20 + c) for c in range(n)]
    obs = np.stack([c[0] for c in cols], axis=1); wt = np.stack([c[1] for c in cols], axis=1); pv = np.stack([c[2] for c in cols], axis=1)
    S = np.stack([c[3].T for c in cols], axis=2); vels = np.stack([c[4] for c in cols], axis=1)
    only = np.array([1, 0, 1, 1, 0], np.uint8)
    got = host_step(h, obs, wt, pv, S, vels, SMOOTH, DAMP, DVMAX, MINVEL, MAXVEL, only)
    for c in range(n):
        if not only[c]:
            assert not got["dv"][:, c].any() and got["nused"][c] == 0 and np.array_equal(got["vels"][:, c], vels[:, c])
            continue
        one = host_step(h, obs[:, c:c + 1], wt[:, c:c + 1], pv[:, c:c + 1], S[:, :, c:c + 1], vels[:, c:c + 1], SMOOTH, DAMP, DVMAX, MINVEL, MAXVEL)
        assert np.array_equal(one["dv"][:, 0].view(np.uint32), got["dv"][:, c].view(np.uint32)) and one["chi2"][0] == got["chi2"][c]
    nowt = host_step(h, obs, None, pv, S, vels, SMOOTH, DAMP, DVMAX, MINVEL, MAXVEL)
    ones = host_step(h, obs, np.ones_like(wt), pv, S, vels, SMOOTH, DAMP, DVMAX, MINVEL, MAXVEL)
    assert np.array_equal(nowt["dv"].view(np.uint32), ones["dv"].view(np.uint32))     # no weights: all 1


def finish(h, N, b, vels, dvmax, minvel, maxvel):
    M = len(b)
    tri = np.array([N[i][j] for i in range(M) for j in range(i + 1)], np.float64)
    v = np.array(vels, F); dv = np.full(M, 9.0, F); d = np.zeros(M)
    flag = h.hcc_finish(M, L.ptr(tri), L.ptr(np.array(b, np.float64)), dvmax, minvel, maxvel, L.ptr(v), L.ptr(dv), L.ptr(d))
    return flag, v, dv, d


def test_not_positive_definite_is_flag_1(h):
    """an N made indefinite by hand (second pivot 1 - 4), one with a zero pivot, one with a pivot that is not finite: flag 1, the column
    unchanged, dv zero; the twin agrees"""
    vels = [3.0, 3.5, 3.7]
    for N in ([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]], [[1.0, 1.0, 0.0], [1.0, 1.0, 0.0], [0.0, 0.0, 1.0]],
              [[1.0, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, 1.0]], [[np.nan, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]):
        flag, v, dv, d = finish(h, N, [1.0, 1.0, 1.0], vels, 0.5, 1.0, 5.0)
        assert flag == 1 and np.array_equal(v, np.array(vels, F)) and not dv.any()
        obs, wt, pv, S, _ = random_column(3, 4, 1)
        twin = depth.column_step_twin(obs, wt, pv, S, np.array(vels, F), SMOOTH, DAMP, 0.5, 1.0, 5.0, n_override=N)
        assert twin["flag"] == 1 and np.array_equal(twin["vels"], np.array(vels, F)) and not twin["dv"].any()
    flag, v, dv, d = finish(h, [[4.0, 2.0], [2.0, 2.0]], [2.0, 1.5], [3.0, 3.5], 0.5, 1.0, 5.0)
    assert flag == 0 and d.tolist() == [4.0, 1.0] and dv.tolist() == [0.25, 0.5] and v.tolist() == [3.25, 4.0]   # L21 = 0.5; y = (2, .5); x = (.25, .5)


def test_clips_are_exact(h):
    """diagonal systems with known solutions: the step is cut at exactly +-dvmax (a step of exactly dvmax stays), the value at the bounds"""
    f = lambda x: float(F(x))
    N = np.eye(6).tolist()
    b = [0.9, -0.9, f(0.25), -f(0.25), 0.1, -0.2]
    vels = [3.0, 3.0, 3.0, 3.0, 4.95, 2.1]
    flag, v, dv, _ = finish(h, N, b, vels, 0.25, 2.0, 5.0)
    assert flag == 0
    assert dv.tolist() == [0.25, -0.25, 0.25, -0.25, f(0.1), f(-0.2)]
    assert v.tolist() == [3.25, 2.75, 3.25, 2.75, 5.0, 2.0]
    obs, wt, pv, S, _ = random_column(6, 3, 2)
    twin = depth.column_step_twin(obs, wt, pv, S, np.array(vels + [9.0], F), 0.0, 1.0, 0.25, 2.0, 5.0)
    assert (np.abs(twin["dv"]) <= F(0.25)).all() and (twin["vels"][:6] <= F(5.0)).all() and twin["vels"][6] == F(9.0)


def test_the_stand_alone_program_runs(tmp_path):
    """the same file as a program with its own main (what a sanitizer build runs): it checks the special cases itself"""
    exe = str(tmp_path / "hostcheck_columns")
    subprocess.check_call(["g++"] + [f for f in FLAGS if f != "-fPIC"] + ["-DHOSTCHECK_COLUMNS_MAIN", "-o", exe, SRC, "-lm"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
