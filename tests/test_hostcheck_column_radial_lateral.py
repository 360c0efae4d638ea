"""The laterally coupled radial depth step (dsurftomo_amd/csrc/column_radial_lateral.h) on the CPU through
tests/hostcheck_column_radial_lateral.cpp, no GPU: against the NumPy twin depth.column_radial_lateral_twin on random well-posed grids of
interior columns; at lateral = lateral_aniso = 0 against column_radial.h's step, bit for bit; the special cases; and the Gauss-Newton loop on
the oracle's curves with noise and a column without data, next to the independent radial loop.

The tolerance of the comparison with the twin is measured, not chosen, by the rule of tests/test_hostcheck_columns.py: the twin solves every
case a second time with numpy.linalg.lstsq on the stacked system, and the header may differ from the twin by FACTOR times the largest
relative difference between the twin's two answers (MEASURED below), plus one rounding to fp32 where fp32 is compared."""
import subprocess

import numpy as np
import pytest

import column_radial_lateral_ref as LR
import column_radial_ref as RR
import columns_ref as R
from column_radial_lateral_ref import same_bits
from dsurftomo_amd import depth

F = np.float32
GRIDS = [(1, 1), (3, 3), (4, 2), (9, 8)]                      # interior columns nvx x nvy
SIZES = [(1, 2), (2, 4), (7, 12)]                             # (M, K)
PAIRS = [(w, wa) for w in (0.05, 0.5, 5.0) for wa in (0.0, 0.5, 5.0)]                          # (lateral, lateral_aniso)
DRAW_SEED, DRAWN = 25, 3                                      # per grid and size: DRAWN of PAIRS by this seed, plus (0, 0.5)
SMOOTH, DAMP, ANISO, DVMAX, MINVEL, MAXVEL = 0.3, 0.1, 0.2, 0.25, 2.0, 5.5
TOL, MAXIT = 1e-12, 4000
# largest relative difference max |delta_pcg - delta_lstsq| / max |delta_lstsq| over cases() with seed 11 (printed by
# test_step_against_the_twin; 3 x 3, M = 7, K = 12, lateral 0.05, lateral_aniso 5), and the factor that covers other seeds
MEASURED = 1.04e-10
FACTOR = 4.0


@pytest.fixture(scope="module")
def h():
    return LR.load()


@pytest.fixture(scope="module")
def hr():
    return RR.load()


@pytest.fixture(scope="module")
def hs():
    return R.load()


def cases():
    """(nvx, nvy, M, K, lateral, lateral_aniso) of the comparison with the twin"""
    rng = np.random.default_rng(DRAW_SEED)
    out = []
    for nvx, nvy in GRIDS:
        for M, K in SIZES:
            picked = [PAIRS[i] for i in sorted(rng.choice(len(PAIRS), DRAWN, replace=False))] + [(0.0, 0.5)]
            out += [(nvx, nvy, M, K, w, wa) for w, wa in picked]
    return out


def love_of(K):
    """Rayleigh and Love slots mixed: the odd slots are Love slots"""
    return np.arange(K) % 2 == 1


def random_grid(nvx, nvy, M, K, seed, unused=True):
    """well-posed columns as tests/test_hostcheck_column_lateral.py's on an (nvy + 2, nvx + 2) grid: Vsv a smooth lateral trend with 0.1 km/s
    of scatter, Vsh up to 6 % above it by a factor that varies from node to node; from K = 3 on about a sixth of the data (never datum 0)
    without weight, their kernels NaN.  Returns dict(nx, ny, love, obs, wt, pv, S (the twin's: slot k on the model it was run on), Sv, Sh (the
    header's: S at the slots each is read at, NaN elsewhere), vsv, vsh)."""
    rng = np.random.default_rng(seed)
    nx, ny = nvx + 2, nvy + 2
    n = nx * ny
    love = love_of(K)
    S = rng.random((M, K, n)) * (2.0 / M)
    pv = 3.0 + rng.random((K, n))
    obs = (pv * (1.0 + 0.03 * rng.standard_normal((K, n)))).astype(F)
    wt = (0.5 + rng.random((K, n))).astype(F)
    i = np.arange(nx)[None, :]; j = np.arange(ny)[:, None]
    base = 3.0 + 0.3 * np.sin(0.8 * i + 0.5 * j)
    vsv = (base.ravel()[None, :] + 0.1 * rng.random((M + 1, n)) + 0.2 * np.arange(M + 1)[:, None]).astype(F)
    vsh = (vsv * (1.0 + 0.06 * rng.random((M + 1, n)))).astype(F)
    if unused and K >= 3:
        drop = rng.random((K, n)) < 0.15
        drop[0] = False
        wt[drop] = 0.0
        S[:, drop] = np.nan
    Sv = S.copy(); Sv[:, love] = np.nan
    Sh = S.copy(); Sh[:, ~love] = np.nan
    return dict(nx=nx, ny=ny, love=love, obs=obs, wt=wt, pv=pv, S=S, Sv=Sv, Sh=Sh, vsv=vsv, vsh=vsh)


def step(h, g, lateral, lateral_aniso, smooth=SMOOTH, damp=DAMP, aniso=ANISO, dvmax=DVMAX, minvel=MINVEL, maxvel=MAXVEL, tol=TOL, maxit=MAXIT, poll=16):
    return LR.host_step(h, g["nx"], g["ny"], g["love"], g["obs"], g["wt"], g["pv"], g["Sv"], g["Sh"], g["vsv"], g["vsh"], smooth, damp, aniso, lateral, lateral_aniso,
                        dvmax, minvel, maxvel, tol, maxit, poll)


def twin_of(g, lateral, lateral_aniso, dvmax=DVMAX, tol=TOL, maxit=MAXIT):
    return depth.column_radial_lateral_twin(g["nx"], g["ny"], g["obs"], g["wt"], g["pv"], g["S"], g["love"], g["vsv"], g["vsh"], SMOOTH, DAMP, ANISO, lateral,
                                            lateral_aniso, dvmax, MINVEL, MAXVEL, tol, maxit)


def interior(g):
    return R.interior(g["nx"], g["ny"]) == 1


def test_step_against_the_twin(h):
    """itn, istop, nused and flag equal; delta, chi2, rz0 within FACTOR * MEASURED, dv and both stepped models within that and one rounding
    to fp32.  The measurement is made again and printed, not asserted (it is numpy's lstsq that would be tested)."""
    tol = FACTOR * MEASURED
    worst = (0.0, None)
    for nvx, nvy, M, K, lateral, lateral_aniso in cases():
        g = random_grid(nvx, nvy, M, K, 11)
        twin = twin_of(g, lateral, lateral_aniso)
        scale = np.abs(twin["delta_lstsq"]).max()
        rel = np.abs(twin["delta"] - twin["delta_lstsq"]).max() / scale
        worst = max(worst, (rel, (nvx, nvy, M, K, lateral, lateral_aniso)))
        got = step(h, g, lateral, lateral_aniso)
        inner = interior(g)
        d_delta = np.abs(got["delta"] - twin["delta"]).max() / scale
        d_chi2 = np.abs(got["chi2"][:, inner] - twin["chi2"][:, inner]).max() / twin["chi2"][:, inner].max()
        print("%d x %d M %d K %2d lateral %4.2f aniso %3.1f: itn %3d, pcg against lstsq %.3g; header against the twin: delta %.3g chi2 %.3g" %
              (nvx, nvy, M, K, lateral, lateral_aniso, got["itn"], rel, d_delta, d_chi2))
        assert (got["itn"], got["istop"]) == (twin["itn"], twin["istop"]) and got["istop"] == 1
        assert np.array_equal(got["nused"], twin["nused"]) and np.array_equal(got["flag"], twin["flag"]) and not got["flag"].any()
        assert (got["nused"][0, inner] >= 1).all() and not got["nused"][:, ~inner].any()
        assert d_delta <= tol and d_chi2 <= tol and abs(got["rz0"] - twin["rz0"]) <= tol * twin["rz0"]
        assert (np.abs(got["dv"].astype(np.float64) - twin["dv"]) <= tol * scale + np.spacing(np.abs(twin["dv"]))).all()
        for name in ("vsv", "vsh"):
            assert (np.abs(got[name].astype(np.float64) - twin[name]) <= tol * scale + np.spacing(twin[name])).all()
            assert same_bits(got[name][:, ~inner], g[name][:, ~inner]) and same_bits(got[name][M], g[name][M])   # the ring and the bottom depth
        assert np.isfinite(got["delta"]).all() and np.abs(got["dv"][:, :, inner]).max() > 0              # no NaN kernel was read
        if (nvx, nvy) == (1, 1):
            assert got["itn"] == 0                                                                       # no edge: x0 is the answer
        else:
            assert got["itn"] >= 2
    print("largest pcg-against-lstsq difference %.3g at %r (MEASURED = %.3g)" % (worst[0], worst[1], MEASURED))


@pytest.mark.parametrize("M,K", SIZES + [(63, 60)])
def test_no_coupling_is_the_radial_step(h, hr, M, K):
    """lateral = lateral_aniso = 0: delta, dv, chi2, nused, flag and both models are radial_step's bit for bit -- flag 2 of a column without
    data (which is then not active) included; no iteration is started, and rz is the residual of the direct solve"""
    for nvx, nvy in GRIDS if M < 63 else [(3, 3)]:
        g = random_grid(nvx, nvy, M, K, 23)
        nx, ny = g["nx"], g["ny"]
        centre = (ny // 2) * nx + nx // 2
        g["wt"][:, centre] = 0.0; g["Sv"][:, :, centre] = np.nan; g["Sh"][:, :, centre] = np.nan
        got = step(h, g, 0.0, 0.0)
        want = RR.host_step(hr, g["love"], g["obs"], g["wt"], g["pv"], g["Sv"], g["Sh"], g["vsv"], g["vsh"], SMOOTH, DAMP, ANISO, DVMAX, MINVEL, MAXVEL, R.interior(nx, ny))
        for name in ("delta", "dv", "chi2", "nused", "flag", "vsv", "vsh"):
            assert same_bits(got[name], want[name]), name
        assert got["flag"][centre] == 2 and (got["itn"], got["istop"], got["started"]) == (0, 1, 0)
        assert 0.0 <= got["rz"] <= 1e-16 * got["rz0"]            # (a backward-stable solve of 126 unknowns: about (126 * 1.1e-16)^2 rz0)
        if (nvx, nvy) != (1, 1):
            assert np.abs(got["dv"]).max() > 0 and got["rz0"] > 0


def test_a_column_without_data_is_carried(h):
    """edges: a column without a used datum of either type (its kernels NaN) is flag 0 with nused 0 0 and chi2 0 0, and every depth of both
    models moves towards the mean of its four neighbours; the twin agrees.  With lateral = 0 and lateral_aniso > 0 it is active too."""
    g = random_grid(3, 3, 7, 12, 5)
    nx = g["nx"]
    centre = 2 * nx + 2
    g["wt"][:, centre] = 0.0
    for name in ("S", "Sv", "Sh"):
        g[name][:, :, centre] = np.nan
    g["vsv"][:7, centre] += F(0.4); g["vsh"][:7, centre] += F(0.4)              # well above its neighbours
    got = step(h, g, 1.0, 0.5, dvmax=1.0)
    twin = twin_of(g, 1.0, 0.5, dvmax=1.0)
    assert got["flag"][centre] == 0 and not got["nused"][:, centre].any() and not got["chi2"][:, centre].any() and twin["flag"][centre] == 0 and twin["deg"][centre] == 4
    assert np.abs(got["delta"] - twin["delta"]).max() <= FACTOR * MEASURED * np.abs(twin["delta"]).max() and got["itn"] == twin["itn"]
    nb = [centre - 1, centre + 1, centre - nx, centre + nx]
    for name, dv in (("vsv", got["dv_sv"]), ("vsh", got["dv_sh"])):
        before = np.abs(g[name][:7, centre].astype(np.float64) - g[name][:7, nb].astype(np.float64).mean(axis=1))
        after = np.abs(got[name][:7, centre].astype(np.float64) - got[name][:7, nb].astype(np.float64).mean(axis=1))
        assert (dv[:, centre] < 0).all() and (after < before).all(), name
    only = step(h, g, 0.0, 0.5)
    assert only["flag"][centre] == 0 and only["itn"] >= 2 and np.abs(only["dv"][:, :, centre]).max() > 0


def test_a_column_that_is_not_finite_is_left_alone(h):
    """a used kernel of the centre column made NaN by hand: flag 1, both models of the column unchanged, dv 0 -- and its neighbours lose that
    edge (the twin's deg, on the same NaN kernel, drops to 2 all round): itn and delta are the twin's"""
    g = random_grid(3, 3, 4, 6, 9, unused=False)
    nx = g["nx"]
    centre = 2 * nx + 2
    g["S"][2, 1, centre] = np.nan; g["Sh"][2, 1, centre] = np.nan                # slot 1 is a Love slot
    got = step(h, g, 0.5, 0.5)
    twin = twin_of(g, 0.5, 0.5)
    assert got["flag"][centre] == 1 and twin["flag"][centre] == 1 and got["nused"][:, centre].tolist() == [3, 3]
    assert not got["dv"][:, :, centre].any() and same_bits(got["vsv"][:, centre], g["vsv"][:, centre]) and same_bits(got["vsh"][:, centre], g["vsh"][:, centre])
    assert twin["deg"][interior(g)].tolist() == [2, 2, 2, 2, 0, 2, 2, 2, 2]
    assert got["itn"] == twin["itn"] and np.abs(got["delta"] - twin["delta"]).max() <= FACTOR * MEASURED * np.abs(twin["delta"]).max()
    assert (got["flag"][interior(g)].sum(), got["istop"]) == (1, 1) and np.isfinite(got["delta"]).all() and np.isfinite([got["rz0"], got["rz"]]).all()


def test_clips_are_exact(h):
    """1 x 1, M = 3, one Rayleigh and one Love datum per depth through diagonal kernels, no regulariser or tie but a tiny damping: the steps
    are known, cut at exactly +-dvmax on both blocks, and the values stop at the bounds.  On 3 x 3 with strong couplings the clipped steps
    are exactly +-dvmax and the stepped values of both models inside [minvel, maxvel]."""
    f = lambda x: float(F(x))
    M, K = 3, 6
    nx = ny = 3
    n = 9
    love = np.arange(K) >= 3
    Sv = np.zeros((M, K, n)); Sh = np.zeros((M, K, n)); pv = np.full((K, n), 3.0); obs = np.full((K, n), 3.0, F)
    vsv = np.full((M + 1, n), 3.0, F); vsh = np.full((M + 1, n), 3.0, F)
    for l in range(M):
        Sv[l, l, 4] = 1.0; Sh[l, 3 + l, 4] = 1.0
    obs[:, 4] = [3.9, 3.1, 2.1, 2.2, 3.05, 3.8]
    vsv[:, 4] = [3.0, 4.95, 2.1, 3.0]
    vsh[:, 4] = [2.2, 3.0, 4.9, 3.0]
    got = LR.host_step(h, nx, ny, love, obs, None, pv, Sv, Sh, vsv, vsh, 0.0, 1e-9, 0.0, 0.0, 0.0, 0.25, 2.0, 5.0)
    assert got["flag"][4] == 0 and got["dv_sv"][:, 4].tolist() == [0.25, f(got["delta"][1, 4]), -0.25] and abs(got["delta"][1, 4] - (f(3.1) - 3.0)) < 1e-15
    assert got["dv_sh"][:, 4].tolist() == [-0.25, f(got["delta"][4, 4]), 0.25] and abs(got["delta"][4, 4] - (f(3.05) - 3.0)) < 1e-15
    assert got["vsv"][:, 4].tolist() == [3.25, 5.0, 2.0, 3.0] and got["vsh"][:, 4].tolist() == [2.0, f(f(3.0) + f(got["delta"][4, 4])), 5.0, 3.0]
    g = random_grid(3, 3, 4, 6, 17)
    g["vsv"][:4, 2 * 5 + 2] += F(1.5); g["vsh"][:4, 2 * 5 + 2] += F(1.5)
    got = step(h, g, 5.0, 5.0, dvmax=0.1, minvel=3.2, maxvel=3.6)
    inner = interior(g)
    assert (np.abs(got["dv"]) <= F(0.1)).all() and (got["dv"][:, :, 12] == F(-0.1)).all()
    for name, dv in (("vsv", got["dv_sv"]), ("vsh", got["dv_sh"])):
        assert (np.abs(dv[:, inner]) == F(0.1)).any() and (got[name][:4, inner] >= F(3.2)).all() and (got[name][:4, inner] <= F(3.6)).all(), name
    assert (got["vsv"][:4, inner] == F(3.2)).any() and (got["vsh"][:4, inner] == F(3.6)).any()


def test_strong_couplings_smooth_what_they_penalise(h):
    """lateral = 1e3: the summed edge roughness of each stepped model falls below a hundredth of its value before the step.  lateral = 0,
    lateral_aniso = 1e3: the same holds for the roughness of Vsh - Vsv (the roughness of Vsv does not have to fall: it is printed)"""
    rough = lambda m, g, M: LR_roughness(m, g["nx"], g["ny"], M)
    for nvx, nvy in GRIDS[1:]:
        g = random_grid(nvx, nvy, 7, 12, 31)
        got = step(h, g, 1e3, 0.0, dvmax=2.0, tol=1e-8, maxit=20000)
        for name in ("vsv", "vsh"):
            before, after = rough(g[name], g, 7), rough(got[name], g, 7)
            print("%d x %d lateral 1e3: itn %d, roughness of %s %.6g -> %.6g" % (nvx, nvy, got["itn"], name, before, after))
            assert got["istop"] == 1 and not got["flag"].any() and after < 0.01 * before
        got = step(h, g, 0.0, 1e3, dvmax=2.0, tol=1e-8, maxit=20000)
        a0 = g["vsh"].astype(np.float64) - g["vsv"].astype(np.float64); a1 = got["vsh"].astype(np.float64) - got["vsv"].astype(np.float64)
        before, after = rough(a0, g, 7), rough(a1, g, 7)
        print("%d x %d lateral_aniso 1e3: itn %d, roughness of Vsh - Vsv %.6g -> %.6g, of Vsv %.6g -> %.6g" %
              (nvx, nvy, got["itn"], before, after, rough(g["vsv"], g, 7), rough(got["vsv"], g, 7)))
        assert got["istop"] == 1 and not got["flag"].any() and after < 0.01 * before


def LR_roughness(vels, nx, ny, M):
    """the sum over the edges between interior columns of the squared differences of the first M rows of vels (>= M, ny * nx), fp64"""
    v = np.asarray(vels, np.float64)[:M].reshape(M, ny, nx)[:, 1:-1, 1:-1]
    return float(((v[:, :, 1:] - v[:, :, :-1]) ** 2).sum() + ((v[:, 1:, :] - v[:, :-1, :]) ** 2).sum())


def test_maxit_and_the_done_flag(h):
    """maxit = 1 is istop 2 after one iteration.  Looking at the done flag after every iteration, every 16th, every 1000th or never gives the
    same bits, though the loop starts a different number of iterations: x is frozen once the criterion is met"""
    g = random_grid(9, 8, 2, 4, 41)
    one = step(h, g, 0.5, 0.5, maxit=1)
    assert (one["itn"], one["istop"], one["started"]) == (1, 2, 1) and one["rz"] > TOL * TOL * one["rz0"]
    runs = [step(h, g, 0.5, 0.5, tol=1e-8, maxit=300, poll=p) for p in (1, 16, 1000, 0)]
    assert [r["started"] for r in runs] == [runs[0]["itn"], -(-runs[0]["itn"] // 16) * 16, 300, 300] and 2 <= runs[0]["itn"] < 284
    for r in runs[1:]:
        for name in ("delta", "dv", "vsv", "vsh", "chi2", "nused", "flag"):
            assert same_bits(r[name], runs[0][name]), name
        assert (r["itn"], r["istop"]) == (runs[0]["itn"], 1) and same_bits(np.array([r["rz0"], r["rz"]]), np.array([runs[0]["rz0"], runs[0]["rz"]]))
    short = step(h, g, 0.5, 0.5, tol=1e-8, maxit=runs[0]["itn"] - 1)
    assert short["istop"] == 2 and short["itn"] == runs[0]["itn"] - 1 and not same_bits(short["delta"], runs[0]["delta"])


def test_the_workspace_is_the_lateral_one_at_twice_the_size(h):
    assert h.hrlat_ws_doubles(5, 5, 7) == 9 * (2 * 105 + 8 * 14) + 9 + 8 + (9 + 4 + 1) // 2


def loop_setting(nz=8):
    """the loop tests' case: (depz, truth_v, truth_h, start, wt, centre)"""
    nx, ny = R.NX, R.NY
    depz = R.depths(nz)
    truth_v = R.smooth_model(nx, ny, nz)
    truth_h = RR.truth_vsh(truth_v)
    wt = np.ones((R.K, nx * ny), F); wt[:, 2 * nx + 2] = 0.0
    return depz, truth_v, truth_h, R.perturbed(truth_v), wt, 2 * nx + 2


def test_loop_on_the_oracles_dispersion(h, hs):
    """5 x 5, nz = 8, columns_ref.WAVES, truth column_radial_ref.truth_vsh over smooth_model, both models started at perturbed(truth Vsv), the
    observations the oracle's curves of the truth times (1 + 0.005 N(0, 1)) (seed 24), the centre column without weights; smooth 0.2, damp
    0.05, aniso 0.2, dvmax 0.3, four iterations, lateral 0.3 and lateral_aniso 0.6 against the independent radial loop (both 0, which is
    radial_step).  The rms error of xi over the interior nodes above the bottom depth is lower with the coupling, and the centre column's xi
    ends closer to the truth than xi = 1 is.  Measured here: 0.08701 at the start; coupled 0.01901, independent 0.03546; the centre column
    0.01980 with the coupling against 0.08701 for xi = 1, where the independent loop leaves it; 45 to 48 iterations of the conjugate
    gradients per step.  (The setting was chosen here; the alternatives tried are in DESIGN.md section 25.)"""
    nz, nx, ny = 8, R.NX, R.NY
    depz, truth_v, truth_h, start, wt, centre = loop_setting(nz)
    obs = LR.noisy(RR.oracle_curves_radial(truth_v, truth_h, depz)[0])
    curves = lambda v, w: RR.oracle_curves_radial(v, w, depz)
    make = lambda lateral, la: lambda v, w, pv, Sv, Sh: LR.host_step(h, nx, ny, RR.LOVE, obs, wt, pv, Sv, Sh, v, w, R.SMOOTH, R.DAMP, RR.ANISO, lateral, la, R.DVMAX,
                                                                     R.MINVEL, R.MAXVEL)
    cv, ch, res = LR.loop(make(LR.LATERAL, LR.LATERAL_ANISO), start, start, depz, curves, hs)
    av, ah, res0 = LR.loop(make(0.0, 0.0), start, start, depz, curves, hs)
    e = [LR.xi_rms(v, w, truth_v, truth_h, nx, ny) for v, w in ((start, start), (cv, ch), (av, ah))]
    c = [LR.xi_column_rms(v, w, truth_v, truth_h, centre) for v, w in ((None, None), (cv, ch), (av, ah))]
    print("rms error of xi: start %.5f, coupled %.5f, independent %.5f; centre column: xi = 1 %.5f, coupled %.5f, independent %.5f; itn %s" %
          (e[0], e[1], e[2], c[0], c[1], c[2], [r["itn"] for r in res]))
    assert all(not r["flag"].any() and r["istop"] == 1 and not r["nused"][:, centre].any() for r in res)
    assert all(r["flag"][centre] == 2 and r["flag"].sum() == 2 for r in res0)
    assert e[1] < e[2]
    assert c[1] < c[0] and c[2] == c[0]
    ring = R.interior(nx, ny) == 0
    for model in (cv, ch, av, ah):
        assert same_bits(model.reshape(nz, -1)[:, ring], start.reshape(nz, -1)[:, ring]) and same_bits(model[nz - 1], start[nz - 1])


def test_the_stand_alone_program_runs(tmp_path):
    """the same file as a program with its own main (what a sanitizer build runs): it checks the special cases itself"""
    exe = str(tmp_path / "hostcheck_column_radial_lateral")
    subprocess.check_call(["g++"] + [f for f in R.FLAGS if f != "-fPIC"] + ["-DHOSTCHECK_COLUMN_RADIAL_LATERAL_MAIN", "-o", exe, LR.SRC, "-lm"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
