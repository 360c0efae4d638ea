"""The laterally coupled depth step (dsurftomo_amd/csrc/column_lateral.h) on the CPU through
tests/hostcheck_column_lateral.cpp, no GPU: against the NumPy twin depth.column_lateral_twin on random well-posed grids of interior columns;
at lateral = 0 against column_system.h's step, bit for bit; the special cases; and the Gauss-Newton loop on the oracle's curves with noise
and a column without data, next to the independent loop.

The tolerance of the comparison with the twin is measured, not chosen, by the rule of tests/test_hostcheck_columns.py: the twin solves every
case a second time with numpy.linalg.lstsq on the stacked system, and the header may differ from the twin by FACTOR times the largest
relative difference between the twin's two answers (MEASURED below), plus one rounding to fp32 where fp32 is compared."""
import subprocess

import numpy as np
import pytest

import column_lateral_ref as LR
import columns_ref as R
from column_lateral_ref import same_bits
from dsurftomo_amd import depth

F = np.float32
GRIDS = [(1, 1), (3, 3), (4, 2), (9, 8)]                      # interior columns nvx x nvy
SIZES = [(1, 1), (2, 3), (7, 12)]                             # (M, K)
LATERALS = [0.05, 0.5, 5.0]
SMOOTH, DAMP, DVMAX, MINVEL, MAXVEL = 0.3, 0.1, 0.25, 2.0, 5.0
TOL, MAXIT = 1e-12, 2000
# largest relative difference max |delta_pcg - delta_lstsq| / max |delta_lstsq| over GRIDS x SIZES x LATERALS with seed 11 (printed by
# test_step_against_the_twin; 9 x 8, M = 7, lateral 5), and the factor that covers other seeds
MEASURED = 3.6e-12
FACTOR = 4.0


@pytest.fixture(scope="module")
def h():
    return LR.load()


@pytest.fixture(scope="module")
def hs():
    return R.load()


def random_grid(nvx, nvy, M, K, seed, unused=True):
    """well-posed columns as tests/test_hostcheck_columns.py's on an (nvy + 2, nvx + 2) grid, the model a smooth lateral trend with 0.1 km/s
    of scatter; from K = 3 on about a sixth of the data (never datum 0) without weight, their kernels NaN.  Returns (nx, ny, obs, wt, pv, S,
    vels)."""
    rng = np.random.default_rng(seed)
    nx, ny = nvx + 2, nvy + 2
    n = nx * ny
    S = rng.random((M, K, n)) * (2.0 / M)
    pv = 3.0 + rng.random((K, n))
    obs = (pv * (1.0 + 0.03 * rng.standard_normal((K, n)))).astype(F)
    wt = (0.5 + rng.random((K, n))).astype(F)
    i = np.arange(nx)[None, :]; j = np.arange(ny)[:, None]
    base = 3.0 + 0.3 * np.sin(0.8 * i + 0.5 * j)
    vels = (base.ravel()[None, :] + 0.1 * rng.random((M + 1, n)) + 0.2 * np.arange(M + 1)[:, None]).astype(F)
    if unused and K >= 3:
        drop = rng.random((K, n)) < 0.15
        drop[0] = False
        wt[drop] = 0.0
        S[:, drop] = np.nan
    return nx, ny, obs, wt, pv, S, vels


def step(h, grid, lateral, smooth=SMOOTH, damp=DAMP, dvmax=DVMAX, minvel=MINVEL, maxvel=MAXVEL, tol=TOL, maxit=MAXIT, poll=16):
    nx, ny, obs, wt, pv, S, vels = grid
    return LR.host_step(h, nx, ny, obs, wt, pv, S, vels, smooth, damp, lateral, dvmax, minvel, maxvel, tol, maxit, poll)


def interior(grid):
    return R.interior(grid[0], grid[1]) == 1


def test_step_against_the_twin(h):
    """itn, istop, nused and flag equal; delta, chi2, rz0 within FACTOR * MEASURED, dv and the stepped model within that and one rounding to
    fp32.  The measurement is made again and printed, not asserted (it is numpy's lstsq that would be tested)."""
    tol = FACTOR * MEASURED
    worst = 0.0
    for nvx, nvy in GRIDS:
        for M, K in SIZES:
            for lateral in LATERALS:
                grid = random_grid(nvx, nvy, M, K, 11)
                nx, ny, obs, wt, pv, S, vels = grid
                twin = depth.column_lateral_twin(nx, ny, obs, wt, pv, S, vels, SMOOTH, DAMP, lateral, DVMAX, MINVEL, MAXVEL, TOL, MAXIT)
                scale = np.abs(twin["delta_lstsq"]).max()
                rel = np.abs(twin["delta"] - twin["delta_lstsq"]).max() / scale
                worst = max(worst, rel)
                got = step(h, grid, lateral)
                inner = interior(grid)
                d_delta = np.abs(got["delta"] - twin["delta"]).max() / scale
                d_chi2 = np.abs(got["chi2"][inner] - twin["chi2"][inner]).max() / twin["chi2"][inner].max()
                print("%d x %d M %d K %2d lateral %4.2f: itn %3d, pcg against lstsq %.3g; header against the twin: delta %.3g chi2 %.3g" %
                      (nvx, nvy, M, K, lateral, got["itn"], rel, d_delta, d_chi2))
                assert (got["itn"], got["istop"]) == (twin["itn"], twin["istop"]) and got["istop"] == 1
                assert np.array_equal(got["nused"], twin["nused"]) and np.array_equal(got["flag"], twin["flag"]) and not got["flag"].any()
                assert (got["nused"][inner] >= 1).all() and not got["nused"][~inner].any()
                assert d_delta <= tol and d_chi2 <= tol and abs(got["rz0"] - twin["rz0"]) <= tol * twin["rz0"]
                assert (np.abs(got["dv"].astype(np.float64) - twin["dv"]) <= tol * scale + np.spacing(np.abs(twin["dv"]))).all()
                assert (np.abs(got["vels"].astype(np.float64) - twin["vels"]) <= tol * scale + np.spacing(twin["vels"])).all()
                assert same_bits(got["vels"][:, ~inner], vels[:, ~inner]) and same_bits(got["vels"][M], vels[M])       # the ring and the bottom depth
                assert np.isfinite(got["delta"]).all() and np.abs(got["dv"][:, inner]).max() > 0                 # no NaN kernel was read
                if (nvx, nvy) == (1, 1):
                    assert got["itn"] == 0                                                                       # no edge: x0 is the answer
                else:
                    assert got["itn"] >= 2
    print("largest pcg-against-lstsq difference %.3g (MEASURED = %.3g)" % (worst, MEASURED))


def test_degrees_of_the_grids():
    """the twin's edges: 3 x 3 has the degrees 2, 3 and 4; 4 x 2 has no 4 (nvx and nvy mixed up would give another list); 1 x 1 has none"""
    for (nvx, nvy), want in (((1, 1), [0]), ((3, 3), [2, 3, 2, 3, 4, 3, 2, 3, 2]), ((4, 2), [2, 3, 3, 2, 2, 3, 3, 2])):
        nx, ny, obs, wt, pv, S, vels = random_grid(nvx, nvy, 2, 3, 3)
        twin = depth.column_lateral_twin(nx, ny, obs, wt, pv, S, vels, SMOOTH, DAMP, 0.5, DVMAX, MINVEL, MAXVEL)
        assert twin["deg"][R.interior(nx, ny) == 1].tolist() == want
        assert not depth.column_lateral_twin(nx, ny, obs, wt, pv, S, vels, SMOOTH, DAMP, 0.0, DVMAX, MINVEL, MAXVEL)["deg"].any()


@pytest.mark.parametrize("M,K", SIZES + [(63, 60)])
def test_lateral_zero_is_the_plain_step(h, hs, M, K):
    """lateral = 0: delta, dv, chi2, nused, flag and the model are column_step's bit for bit -- flag 2 of a column without data (which is
    then not active) included; no iteration is started"""
    grid = random_grid(3, 3, M, K, 23)
    nx, ny, obs, wt, pv, S, vels = grid
    centre = 2 * nx + 2
    wt[:, centre] = 0.0; S[:, :, centre] = np.nan
    got = step(h, grid, 0.0)
    want = R.host_step(hs, obs, wt, pv, S, vels, SMOOTH, DAMP, DVMAX, MINVEL, MAXVEL, R.interior(nx, ny))
    for name in ("delta", "dv", "chi2", "nused", "flag", "vels"):
        assert same_bits(got[name], want[name]), name
    assert got["flag"][centre] == 2 and (got["itn"], got["istop"], got["started"]) == (0, 1, 0) and np.abs(got["dv"]).max() > 0


def test_a_column_without_data_is_carried(h):
    """lateral > 0: a column without a used datum (its kernels NaN) is flag 0 with nused 0 and chi2 0, and every depth moves towards the
    mean of its four neighbours; the twin agrees"""
    grid = random_grid(3, 3, 7, 12, 5)
    nx, ny, obs, wt, pv, S, vels = grid
    centre = 2 * nx + 2
    wt[:, centre] = 0.0; S[:, :, centre] = np.nan
    vels[:7, centre] += F(0.4)                                                   # well above its neighbours
    got = step(h, grid, 1.0, dvmax=1.0)
    twin = depth.column_lateral_twin(nx, ny, obs, wt, pv, S, vels, SMOOTH, DAMP, 1.0, 1.0, MINVEL, MAXVEL, TOL, MAXIT)
    assert got["flag"][centre] == 0 and got["nused"][centre] == 0 and got["chi2"][centre] == 0.0 and twin["flag"][centre] == 0 and twin["deg"][centre] == 4
    assert np.abs(got["delta"] - twin["delta"]).max() <= FACTOR * MEASURED * np.abs(twin["delta"]).max() and got["itn"] == twin["itn"]
    nb = [centre - 1, centre + 1, centre - nx, centre + nx]
    before = np.abs(vels[:7, centre].astype(np.float64) - vels[:7, nb].astype(np.float64).mean(axis=1))
    after = np.abs(got["vels"][:7, centre].astype(np.float64) - got["vels"][:7, nb].astype(np.float64).mean(axis=1))
    assert (got["dv"][:, centre] < 0).all() and (after < before).all()


def test_a_column_that_is_not_finite_is_left_alone(h):
    """a used kernel of the centre column made NaN by hand: flag 1, the column unchanged, dv 0 -- and its neighbours lose that edge (the
    twin's deg, on the same NaN kernel, drops to 2 all round): itn and delta are the twin's"""
    grid = random_grid(3, 3, 4, 6, 9, unused=False)
    nx, ny, obs, wt, pv, S, vels = grid
    centre = 2 * nx + 2
    S[2, 1, centre] = np.nan
    got = step(h, grid, 0.5)
    twin = depth.column_lateral_twin(nx, ny, obs, wt, pv, S, vels, SMOOTH, DAMP, 0.5, DVMAX, MINVEL, MAXVEL, TOL, MAXIT)
    assert got["flag"][centre] == 1 and twin["flag"][centre] == 1 and got["nused"][centre] == 6
    assert not got["dv"][:, centre].any() and same_bits(got["vels"][:, centre], vels[:, centre])
    assert twin["deg"][R.interior(nx, ny) == 1].tolist() == [2, 2, 2, 2, 0, 2, 2, 2, 2]
    assert got["itn"] == twin["itn"] and np.abs(got["delta"] - twin["delta"]).max() <= FACTOR * MEASURED * np.abs(twin["delta"]).max()
    assert (got["flag"][interior(grid)].sum(), got["istop"]) == (1, 1) and np.isfinite(got["delta"]).all() and np.isfinite([got["rz0"], got["rz"]]).all()


def test_no_data_anywhere_and_all_flagged(h):
    """the defined results: every column without data is a pure smoothing step of the model (flag 0 everywhere; a model without lateral
    differences gets a zero step with rz0 = 0 at itn 0); every column flagged 1 leaves everything alone, itn 0, istop 1, rz0 = rz = 0"""
    nx, ny, obs, wt, pv, S, vels = random_grid(3, 3, 4, 6, 13, unused=False)
    inner = R.interior(nx, ny) == 1
    none = (nx, ny, obs, np.zeros_like(wt), pv, np.full_like(S, np.nan), vels)
    got = step(h, none, 1.0, dvmax=1.0)
    assert not got["flag"].any() and not got["nused"].any() and not got["chi2"].any() and got["istop"] == 1 and got["itn"] >= 2
    assert LR.roughness(got["vels"], nx, ny, 4) < LR.roughness(vels, nx, ny, 4) and np.abs(got["dv"][:, inner]).max() > 0
    flat = np.full_like(vels, F(3.5))
    got = step(h, none[:6] + (flat,), 1.0)
    assert not got["flag"].any() and not got["dv"].any() and same_bits(got["vels"], flat) and (got["itn"], got["istop"], got["rz0"], got["rz"]) == (0, 1, 0.0, 0.0)
    S2 = S.copy(); S2[0, 0, :] = np.nan                                           # datum 0 is used everywhere
    got = step(h, (nx, ny, obs, wt, pv, S2, vels), 1.0)
    assert (got["flag"][inner] == 1).all() and not got["flag"][~inner].any() and not got["dv"].any() and same_bits(got["vels"], vels)
    assert (got["itn"], got["istop"], got["rz0"], got["rz"]) == (0, 1, 0.0, 0.0) and (got["nused"][inner] == 6).all()


def test_clips_are_exact(h):
    """1 x 1, M = 3, one datum per depth through a diagonal kernel and no regulariser but a tiny damping: the steps are known, cut at exactly
    +-dvmax, and the values stop at the bounds.  On 3 x 3 with a strong coupling the clipped steps are exactly +-dvmax and the stepped
    values inside [minvel, maxvel]."""
    f = lambda x: float(F(x))
    M = K = 3
    nx = ny = 3
    n = 9
    S = np.zeros((M, K, n)); pv = np.full((K, n), 3.0); obs = np.full((K, n), 3.0, F); vels = np.full((M + 1, n), 3.0, F)
    for l in range(M):
        S[l, l, 4] = 1.0
    obs[:, 4] = [3.9, 3.1, 2.1]
    vels[:, 4] = [3.0, 4.95, 2.1, 3.0]
    got = LR.host_step(h, nx, ny, obs, None, pv, S, vels, 0.0, 1e-9, 0.0, 0.25, 2.0, 5.0)
    assert got["flag"][4] == 0 and got["dv"][:, 4].tolist() == [0.25, f(got["delta"][1, 4]), -0.25] and abs(got["delta"][1, 4] - (f(3.1) - 3.0)) < 1e-15
    assert got["vels"][:, 4].tolist() == [3.25, 5.0, 2.0, 3.0]
    grid = random_grid(3, 3, 4, 6, 17)
    grid[6][:4, 2 * 5 + 2] += F(1.5)
    got = step(h, grid, 5.0, dvmax=0.1, minvel=3.2, maxvel=3.6)
    inner = interior(grid)
    assert (np.abs(got["dv"]) <= F(0.1)).all() and (np.abs(got["dv"][:, inner]) == F(0.1)).any() and (got["dv"][:, 12] == F(-0.1)).all()
    assert (got["vels"][:4, inner] >= F(3.2)).all() and (got["vels"][:4, inner] <= F(3.6)).all() and (got["vels"][:4, inner] == F(3.2)).any()


def test_a_strong_coupling_smooths_the_stepped_model(h):
    """lateral = 1e3: the summed edge roughness of the stepped model is below the one before the step (far below: the step is free to move)"""
    for nvx, nvy in GRIDS[1:]:
        grid = random_grid(nvx, nvy, 7, 12, 31)
        nx, ny, vels = grid[0], grid[1], grid[6]
        got = step(h, grid, 1e3, dvmax=2.0, tol=1e-8, maxit=20000)
        before, after = LR.roughness(vels, nx, ny, 7), LR.roughness(got["vels"], nx, ny, 7)
        print("%d x %d: itn %d, roughness %.6g -> %.6g" % (nvx, nvy, got["itn"], before, after))
        assert got["istop"] == 1 and not got["flag"].any() and after < before and after < 0.01 * before


def test_maxit_and_the_done_flag(h):
    """maxit = 1 is istop 2 after one iteration.  Looking at the done flag after every iteration, every 16th, every 1000th or never gives the
    same bits, though the loop starts a different number of iterations: x is frozen once the criterion is met"""
    grid = random_grid(9, 8, 2, 3, 41)
    one = step(h, grid, 0.5, maxit=1)
    assert (one["itn"], one["istop"], one["started"]) == (1, 2, 1) and one["rz"] > TOL * TOL * one["rz0"]
    runs = [step(h, grid, 0.5, tol=1e-8, maxit=300, poll=p) for p in (1, 16, 1000, 0)]
    assert [r["started"] for r in runs] == [runs[0]["itn"], -(-runs[0]["itn"] // 16) * 16, 300, 300] and 2 <= runs[0]["itn"] < 284
    for r in runs[1:]:
        for name in ("delta", "dv", "vels", "chi2", "nused", "flag"):
            assert same_bits(r[name], runs[0][name]), name
        assert (r["itn"], r["istop"]) == (runs[0]["itn"], 1) and same_bits(np.array([r["rz0"], r["rz"]]), np.array([runs[0]["rz0"], runs[0]["rz"]]))
    short = step(h, grid, 0.5, tol=1e-8, maxit=runs[0]["itn"] - 1)
    assert short["istop"] == 2 and short["itn"] == runs[0]["itn"] - 1 and not same_bits(short["delta"], runs[0]["delta"])


def test_the_global_sum_has_one_shape(h):
    """64 chains of every 64th figure, added in order: not the plain sequential sum (on 200 figures of mixed size), and the twin's"""
    rng = np.random.default_rng(3)
    part = rng.standard_normal(200) * 10.0 ** rng.integers(-8, 8, 200)
    got = h.hlat_sum(200, part.ctypes.data)
    chains = [sum(part[t::64].tolist(), 0.0) for t in range(64)]
    assert got == sum(chains, 0.0) == depth.lateral_sum(part)
    assert h.hlat_ws_doubles(5, 5, 7) == 9 * (2 * 28 + 8 * 7) + 9 + 8 + (9 + 4 + 1) // 2


def test_loop_on_the_oracles_dispersion(h, hs):
    """5 x 5, nz = 8, columns_ref.WAVES, truth smooth_model, start perturbed(truth), the observations the oracle's curves of the truth times
    (1 + 0.005 N(0, 1)) (column_lateral_ref.noisy: seed 24), the centre column without weights; columns_ref's smooth 0.2, damp 0.05, dvmax
    0.3, four iterations, lateral 0.3 against the independent loop (lateral = 0, which is column_step).  The rms model error over the
    interior nodes above the bottom depth is lower with the coupling; the centre column ends closer to the truth than it started, where
    the independent loop leaves it.  Measured here: start 0.03993; lateral 0.03558, independent 0.04831 km/s; the centre column 0.05117 at
    the start and after the independent loop, 0.03957 km/s with the coupling; 22 to 23 iterations of the conjugate gradients per step.
    (Noise and lateral were chosen here: at 1 % noise the margins of seed 24 shrink to 0.0481 against 0.0743 and 0.0501 against 0.0512.)"""
    nz, nx, ny = 8, R.NX, R.NY
    ncol, centre = nx * ny, 2 * nx + 2
    depz = R.depths(nz)
    truth = R.smooth_model(nx, ny, nz)
    obs = LR.noisy(R.oracle_curves(truth, depz)[0])
    wt = np.ones((R.K, ncol), F); wt[:, centre] = 0.0
    start = R.perturbed(truth)
    curves = lambda m: R.oracle_curves(m, depz)
    make = lambda lateral: lambda model, pv, S: LR.host_step(h, nx, ny, obs, wt, pv, S, model, R.SMOOTH, R.DAMP, lateral, R.DVMAX, R.MINVEL, R.MAXVEL)
    coupled, res = LR.loop(make(LR.LATERAL), start, depz, obs, wt, curves, hs)
    alone, res0 = LR.loop(make(0.0), start, depz, obs, wt, curves, hs)
    col_err = lambda m: float(np.sqrt(((m.reshape(nz, ncol)[:nz - 1, centre].astype(np.float64) - truth.reshape(nz, ncol)[:nz - 1, centre]) ** 2).mean()))
    e = [LR.model_rms(m, truth, nx, ny) for m in (start, coupled, alone)]
    c = [col_err(m) for m in (start, coupled, alone)]
    print("rms model error: start %.5f, lateral %.5f, independent %.5f km/s; centre column: start %.5f, lateral %.5f, independent %.5f km/s; itn %s" %
          (e[0], e[1], e[2], c[0], c[1], c[2], [r["itn"] for r in res]))
    assert all(not r["flag"].any() and r["istop"] == 1 and r["nused"][centre] == 0 for r in res)
    assert all(r["flag"][centre] == 2 and r["flag"].sum() == 2 for r in res0)
    assert e[1] < e[2]
    assert c[1] < c[0] and c[2] == c[0]
    ring = R.interior(nx, ny) == 0
    for model in (coupled, alone):
        assert same_bits(model.reshape(nz, -1)[:, ring], start.reshape(nz, -1)[:, ring]) and same_bits(model[nz - 1], start[nz - 1])


def test_the_stand_alone_program_runs(tmp_path):
    """the same file as a program with its own main (what a sanitizer build runs): it checks the special cases itself"""
    exe = str(tmp_path / "hostcheck_column_lateral")
    subprocess.check_call(["g++"] + [f for f in R.FLAGS if f != "-fPIC"] + ["-DHOSTCHECK_COLUMN_LATERAL_MAIN", "-o", exe, LR.SRC, "-lm"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
