"""The radially anisotropic depth step of one column (dsurftomo_amd/csrc/column_radial.h) on the CPU through
tests/hostcheck_column_radial.cpp, no GPU: against the NumPy twin depth.column_radial_twin on random well-posed columns of the sizes the
kernel meets; at aniso = 0 against column_system.h's step on each block, bit for bit; the special cases; the Gauss-Newton loop on the
oracle's curves of a truth with Vsh 6 % above Vsv at mid depth, next to the isotropic loop on the same observations; and the host side of
`python -m dsurftomo_amd.depth --radial`: flags, refusals, files, symbols.

The tolerance of the comparison with the twin is measured, not chosen, by the rule of tests/test_hostcheck_columns.py: the twin solves every
case a second time with numpy.linalg.lstsq on the stacked system, and the header may differ from the twin by FACTOR times the largest
relative difference between the twin's two answers (MEASURED below), plus one rounding to fp32 where fp32 is compared."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _libs as L
import column_radial_ref as RR
import columns_ref as R
from column_radial_ref import same_bits
from dsurftomo_amd import depth, io, maps

F = np.float32
SIZES = [(1, 2), (2, 4), (7, 12), (63, 60)]                    # (M, K)
SMOOTH, DAMP, ANISO, DVMAX, MINVEL, MAXVEL = 0.3, 0.1, 0.2, 0.25, 2.0, 5.0
# largest relative difference max |delta_ldlt - delta_lstsq| / max |delta_lstsq| over SIZES with seed 11 (printed by
# test_step_against_the_twin), and the factor that covers other seeds
MEASURED = 8.8e-15
FACTOR = 4.0
NEW = ("dsa_dispersion_begin_radial", "dsa_columns_step_radial", "dsa_dispersion_get_model_radial")


@pytest.fixture(scope="module")
def h():
    return RR.load()


@pytest.fixture(scope="module")
def hs():
    return R.load()


def random_column(M, K, seed, unused=True):
    """a well-posed column as tests/test_hostcheck_columns.py's, with Rayleigh and Love slots mixed, Vsh 2 to 6 % off Vsv, and -- from K = 4
    on -- a Rayleigh and a Love datum that are not used (no weight, no root) whose kernels are NaN.  Returns (love, obs, wt, pv, S (K, M):
    each slot's kernel on its own model, vsv, vsh)."""
    rng = np.random.default_rng(seed)
    love = rng.random(K) < 0.5
    love[0], love[1] = False, True
    if K >= 4:
        love[2], love[3] = False, True
    S = rng.random((K, M)) * (2.0 / M)
    pv = 3.0 + rng.random(K)
    obs = (pv * (1.0 + 0.03 * rng.standard_normal(K))).astype(F)
    wt = (0.5 + rng.random(K)).astype(F)
    vsv = (3.0 + rng.random(M + 1)).astype(F)
    vsh = (vsv * (1.0 + 0.02 + 0.04 * rng.random(M + 1))).astype(F)
    if unused and K >= 4:
        wt[2] = 0.0; pv[3] = 0.0
        S[2:4] = np.nan
    return love, obs, wt, pv, S, vsv, vsh


def split(love, S):
    """the two arrays the header reads, (M, K, 1): a slot's kernel on the model it was not run on is NaN -- it must never be read"""
    Sv = np.where(love[:, None], np.nan, S).T[:, :, None]
    Sh = np.where(love[:, None], S, np.nan).T[:, :, None]
    return Sv, Sh


def step(h, col, aniso=ANISO, smooth=SMOOTH, damp=DAMP, dvmax=DVMAX, minvel=MINVEL, maxvel=MAXVEL):
    love, obs, wt, pv, S, vsv, vsh = col
    Sv, Sh = split(love, S)
    return RR.host_step(h, love, obs[:, None], wt[:, None], pv[:, None], Sv, Sh, vsv[:, None], vsh[:, None], smooth, damp, aniso, dvmax, minvel, maxvel)


def test_step_against_the_twin(h):
    """nused and flag equal; delta and chi2 within FACTOR * MEASURED, dv and the stepped models within that and one rounding to fp32.  The
    measurement is made again and printed, not asserted (it is numpy's lstsq that would be tested)."""
    tol = FACTOR * MEASURED
    worst = 0.0
    for M, K in SIZES:
        col = random_column(M, K, 11)
        love, obs, wt, pv, S, vsv, vsh = col
        args = (obs, wt, pv, S, love, vsv, vsh, SMOOTH, DAMP, ANISO, DVMAX, MINVEL, MAXVEL)
        twin = depth.column_radial_twin(*args)
        other = depth.column_radial_twin(*args, solver="lstsq")
        scale = np.abs(other["delta"]).max()
        rel = np.abs(twin["delta"] - other["delta"]).max() / scale
        worst = max(worst, rel)
        got = step(h, col)
        d_delta = np.abs(got["delta"][:, 0] - twin["delta"]).max() / scale
        d_chi2 = max(abs(got["chi2"][q, 0] - twin["chi2"][q]) / twin["chi2"][q] for q in range(2))
        print("M %2d K %2d (%d Love slots): ldlt against lstsq %.3g; header against the twin: delta %.3g chi2 %.3g" % (M, K, int(love.sum()), rel, d_delta, d_chi2))
        nunused = 2 if K >= 4 else 0
        assert got["nused"][:, 0].tolist() == twin["nused"] and sum(twin["nused"]) == K - nunused and min(twin["nused"]) >= 1
        assert got["flag"][0] == twin["flag"] == 0
        assert d_delta <= tol and d_chi2 <= tol
        for name, tw in (("dv_sv", twin["dv_sv"]), ("dv_sh", twin["dv_sh"])):
            assert (np.abs(got[name][:, 0].astype(np.float64) - tw) <= tol * scale + np.spacing(np.abs(tw))).all(), name
        for name in ("vsv", "vsh"):
            assert (np.abs(got[name][:, 0].astype(np.float64) - twin[name]) <= tol * scale + np.spacing(twin[name])).all(), name
            assert got[name][M, 0] == col[5 if name == "vsv" else 6][M]              # the bottom depth is kept
        assert np.abs(twin["dv_sv"]).max() > 0 and np.abs(twin["dv_sh"]).max() > 0
        assert np.isfinite(got["delta"]).all()                                       # no NaN kernel was read
    print("largest ldlt-against-lstsq difference %.3g (MEASURED = %.3g)" % (worst, MEASURED))


@pytest.mark.parametrize("M,K", SIZES)
def test_aniso_zero_is_the_plain_step_on_each_block(h, hs, M, K):
    """aniso = 0: the Vsv block is column_step with the Love weights zeroed, the Vsh block column_step on the Vsh model with the Rayleigh
    weights zeroed -- dv and the stepped models bit for bit, chi2 and nused per wave type too"""
    col = random_column(M, K, 23)
    love, obs, wt, pv, S, vsv, vsh = col
    got = step(h, col, aniso=0.0)
    assert got["flag"][0] == 0
    Sv, Sh = split(love, S)
    for q, (mine, vel, Sq) in enumerate(((~love, vsv, Sv), (love, vsh, Sh))):
        w = np.where(mine, wt, F(0.0))
        want = R.host_step(hs, obs[:, None], w[:, None], pv[:, None], Sq, vel[:, None], SMOOTH, DAMP, DVMAX, MINVEL, MAXVEL)
        assert want["flag"][0] == 0 and want["nused"][0] == got["nused"][q, 0] >= 1
        assert same_bits(got["dv"][q], want["dv"]) and same_bits(got["vsh" if q else "vsv"], want["vels"])
        assert same_bits(got["chi2"][q], want["chi2"]) and same_bits(got["delta"][q * M:(q + 1) * M], want["delta"])
        assert np.abs(want["dv"]).max() > 0


def test_one_wave_type_without_data_still_steps(h):
    """no Love datum used: flag 0; the Vsh block is moved by the tie alone, towards the stepped Vsv; at aniso = 0 it does not move"""
    M, K = 7, 12
    love, obs, wt, pv, S, vsv, vsh = random_column(M, K, 5)
    wt = np.where(love, F(0.0), wt)
    col = (love, obs, wt, pv, np.where(love[:, None], np.nan, S), vsv, vsh)
    got = step(h, col, aniso=0.5)
    assert got["flag"][0] == 0 and got["nused"][1, 0] == 0 and got["nused"][0, 0] >= 1 and got["chi2"][1, 0] == 0.0
    assert np.abs(got["dv_sv"]).max() > 0 and np.abs(got["dv_sh"]).max() > 0
    twin = depth.column_radial_twin(obs, wt, pv, col[4], love, vsv, vsh, SMOOTH, DAMP, 0.5, DVMAX, MINVEL, MAXVEL)
    assert twin["flag"] == 0 and np.abs(got["delta"][:, 0] - twin["delta"]).max() <= FACTOR * MEASURED * np.abs(twin["delta"]).max()
    alone = step(h, col, aniso=0.0)
    assert alone["flag"][0] == 0 and not alone["dv_sh"].any() and same_bits(alone["vsh"][:, 0], vsh)


def test_no_data_is_flag_2_whatever_damp_and_aniso_are(h):
    M, K = 4, 6
    love, obs, wt, pv, S, vsv, vsh = random_column(M, K, 6)
    nan = np.full((K, M), np.nan)
    for damp, aniso in ((0.1, 0.0), (1e3, 0.2), (0.1, 1e3)):
        got = step(h, (love, obs, np.zeros(K, F), pv, nan, vsv, vsh), aniso=aniso, damp=damp)
        assert got["flag"][0] == 2 and not got["nused"].any() and not got["chi2"].any() and not got["dv"].any()
        assert same_bits(got["vsv"][:, 0], vsv) and same_bits(got["vsh"][:, 0], vsh)
        twin = depth.column_radial_twin(obs, np.zeros(K, F), pv, nan, love, vsv, vsh, SMOOTH, damp, aniso, DVMAX, MINVEL, MAXVEL)
        assert twin["flag"] == 2 and np.array_equal(twin["vsv"], vsv) and np.array_equal(twin["vsh"], vsh)


def test_not_positive_definite_is_flag_1(h):
    """a 4 x 4 matrix (M = 2) made indefinite by hand in the coupling (fourth pivot 1 - 4), one with a zero pivot, two with a pivot that is
    not finite: flag 1, both models unchanged, dv zero; the twin agrees.  A definite one with a known solution steps both models."""
    vsv, vsh = [3.0, 3.5], [3.2, 3.6]
    eye = np.eye(4)
    bad = []
    n = eye.copy(); n[3, 1] = n[1, 3] = 2.0; bad.append(n)
    n = eye.copy(); n[2, 0] = n[0, 2] = 1.0; bad.append(n)
    n = eye.copy(); n[2, 2] = np.inf; bad.append(n)
    n = eye.copy(); n[0, 0] = np.nan; bad.append(n)
    love, obs, wt, pv, S, _, _ = random_column(2, 4, 1, unused=False)
    for N in bad:
        flag, v, w, dv, d = RR.host_finish(h, N, [1.0] * 4, vsv, vsh, 0.5, 1.0, 5.0)
        assert flag == 1 and np.array_equal(v, np.array(vsv, F)) and np.array_equal(w, np.array(vsh, F)) and not dv.any()
        twin = depth.column_radial_twin(obs, wt, pv, S, love, np.array(vsv, F), np.array(vsh, F), SMOOTH, DAMP, ANISO, 0.5, 1.0, 5.0, n_override=N)
        assert twin["flag"] == 1 and np.array_equal(twin["vsv"], np.array(vsv, F)) and not twin["dv_sv"].any() and not twin["dv_sh"].any()
    # [[4, 2], [2, 2]] on (Vsv_0, Vsh_0), identity on the others: L = 0.5, d = (4, 1, 1, 1), x = (.25, .125, .5, -.25)
    N = np.diag([4.0, 1.0, 2.0, 1.0]); N[2, 0] = N[0, 2] = 2.0
    flag, v, w, dv, d = RR.host_finish(h, N, [2.0, 0.125, 1.5, -0.25], vsv, vsh, 0.5, 1.0, 5.0)
    assert flag == 0 and d.tolist() == [4.0, 1.0, 1.0, 1.0] and dv.tolist() == [0.25, 0.125, 0.5, -0.25]
    assert v.tolist() == [3.25, 3.625] and w.tolist() == [F(3.2) + F(0.5), F(3.6) - F(0.25)]


def test_clips_are_exact(h):
    """a diagonal system with known solutions: both blocks' steps are cut at exactly +-dvmax (a step of exactly dvmax stays), the values at
    the bounds"""
    f = lambda x: float(F(x))
    N = np.eye(6)
    b = [0.9, f(0.25), 0.1, -0.9, -f(0.25), -0.2]
    vsv, vsh = [3.0, 3.0, 4.95], [3.0, 3.0, 2.1]
    flag, v, w, dv, _ = RR.host_finish(h, N, b, vsv, vsh, 0.25, 2.0, 5.0)
    assert flag == 0
    assert dv.tolist() == [0.25, 0.25, f(0.1), -0.25, -0.25, f(-0.2)]
    assert v.tolist() == [3.25, 3.25, 5.0] and w.tolist() == [2.75, 2.75, 2.0]


def test_a_strong_tie_pulls_the_models_together(h):
    """aniso = 1e3: |vsh - vsv| after the step is below the one before it at every depth above the bottom"""
    for M, K in SIZES:
        col = random_column(M, K, 31)
        vsv, vsh = col[5], col[6]
        got = step(h, col, aniso=1e3, dvmax=1.0)
        assert got["flag"][0] == 0
        before = np.abs(vsh[:M].astype(np.float64) - vsv[:M])
        after = np.abs(got["vsh"][:M, 0].astype(np.float64) - got["vsv"][:M, 0])
        assert (after < before).all() and after.max() < 0.05 * before.min()


def test_columns_side_by_side_and_the_mask(h):
    """columns with the engine's strides: each equals the column alone; a column masked out keeps its zeros; no weights means all 1"""
    M, K, n = 3, 6, 4
    cols = [random_column(M, K, 40 + c, unused=False) for c in range(n)]
    love = cols[0][0]
    obs = np.stack([c[1] for c in cols], axis=1); wt = np.stack([c[2] for c in cols], axis=1); pv = np.stack([c[3] for c in cols], axis=1)
    S = np.stack([c[4].T for c in cols], axis=2); vsv = np.stack([c[5] for c in cols], axis=1); vsh = np.stack([c[6] for c in cols], axis=1)
    only = np.array([1, 0, 1, 1], np.uint8)
    args = (SMOOTH, DAMP, ANISO, DVMAX, MINVEL, MAXVEL)
    got = RR.host_step(h, love, obs, wt, pv, S, S, vsv, vsh, *args, only)
    for c in range(n):
        if not only[c]:
            assert not got["dv"][:, :, c].any() and not got["nused"][:, c].any() and same_bits(got["vsv"][:, c], vsv[:, c]) and same_bits(got["vsh"][:, c], vsh[:, c])
            continue
        s = slice(c, c + 1)
        one = RR.host_step(h, love, obs[:, s], wt[:, s], pv[:, s], S[:, :, s], S[:, :, s], vsv[:, s], vsh[:, s], *args)
        assert same_bits(one["dv"][:, :, 0], got["dv"][:, :, c]) and same_bits(one["chi2"][:, 0], got["chi2"][:, c])
    nowt = RR.host_step(h, love, obs, None, pv, S, S, vsv, vsh, *args)
    ones = RR.host_step(h, love, obs, np.ones_like(wt), pv, S, S, vsv, vsh, *args)
    assert same_bits(nowt["dv"], ones["dv"]) and same_bits(nowt["chi2"], ones["chi2"])
    assert h.hrad_doubles(63, 60) * 8 == 98232 and h.hrad_doubles(7, 12) == 14 * 15 // 2 + 84 + 24 + 42


@pytest.mark.parametrize("nz", [3, 8])
def test_loop_on_the_oracles_dispersion(h, hs, nz):
    """5 x 5, columns_ref.WAVES, truth Vsv = smooth_model and Vsh 6 % above it at mid depth, the observations the oracle's curves in fp32 (the
    Love ones on Vsh), both models started at perturbed(truth Vsv); smooth 0.2, damp 0.05, aniso 0.2, dvmax 0.3, four iterations.  The sum
    of chi2 before the last radial step is below the one before the first, and below half of what the isotropic loop (column_step on the
    same observations) has before its last step.  A NumPy double-precision loop gave 9.8e-3 against 0.675 (nz 8) and 8.5e-2 against 0.294
    (nz 3) there."""
    depz = R.depths(nz)
    truth_v = R.smooth_model(R.NX, R.NY, nz)
    truth_h = RR.truth_vsh(truth_v)
    assert same_bits(truth_h[nz - 1], truth_v[nz - 1]) and 1.03 < (truth_h / truth_v).max() <= 1.0601
    obs = RR.oracle_curves_radial(truth_v, truth_h, depz)[0].astype(F)
    start = R.perturbed(truth_v)
    seen = []
    vsv, vsh, chi2, rms = RR.loop(h, hs, start, start, depz, obs, lambda v, w: RR.oracle_curves_radial(v, w, depz),
                                  after=lambda it, m, inputs, out: seen.append((out["flag"].copy(), np.abs(out["dv"]).max())))
    _, iso, _ = R.loop(hs, start, depz, obs, lambda m: R.oracle_curves(m, depz))
    print("nz %d: sum of chi2 before each radial step %s; before each isotropic step %s" % (nz, " ".join("%.4g" % x for x in chi2), " ".join("%.4g" % x for x in iso)))
    print("nz %d: rms (Rayleigh, Love) before each radial step %s" % (nz, " ".join("(%.5f, %.5f)" % r for r in rms)))
    inner = R.interior(R.NX, R.NY) == 1
    xi = (vsh.reshape(nz, -1)[:nz - 1, inner].astype(np.float64) / vsv.reshape(nz, -1)[:nz - 1, inner]) ** 2
    print("nz %d: xi after the loop median %.4f, range %.4f to %.4f (truth up to %.4f)" % (nz, np.median(xi), xi.min(), xi.max(), float((truth_h / truth_v).max()) ** 2))
    assert len(chi2) == len(iso) == R.ITERATIONS
    assert chi2[-1] < chi2[0]
    assert chi2[-1] < 0.5 * iso[-1]
    assert all(not f.any() and d > 0 for f, d in seen)
    ring = ~inner
    for model in (vsv, vsh):
        assert same_bits(model.reshape(nz, -1)[:, ring], start.reshape(nz, -1)[:, ring]) and same_bits(model[nz - 1], start[nz - 1])


def test_the_stand_alone_program_runs(tmp_path):
    """the same file as a program with its own main (what a sanitizer build runs): it checks the special cases itself"""
    exe = str(tmp_path / "hostcheck_column_radial")
    subprocess.check_call(["g++"] + [f for f in R.FLAGS if f != "-fPIC"] + ["-DHOSTCHECK_COLUMN_RADIAL_MAIN", "-o", exe, RR.SRC, "-lm"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr


# ---- the host side of the driver ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def taipei():
    return io.load()


def small_case(taipei):
    return dict(taipei, nx=6, ny=5, nz=3, depz=np.array([0.0, 2.0, 5.0], F), tRc=np.array([4.0, 6.5]), tRg=np.array([5.0]), tLc=np.zeros(0), tLg=np.array([8.0]), kmax=4)


def test_parser_defaults_and_old_attributes():
    a = depth.parser().parse_args(["dir"])
    assert (a.radial, a.aniso) == (False, 0.2) and depth.DEFAULT_ANISO == 0.2
    assert (a.maps, a.iterations, a.smooth, a.damp, a.dvmax, a.min_dws, a.out, a.resolution, a.sigma) == (None, 4, 0.5, 0.1, 0.5, 0.0, ".", False, None)      # as they were
    a = depth.parser().parse_args(["dir", "--radial", "--aniso", "0.7", "--damp", "0.3"])
    assert (a.radial, a.aniso, a.damp, a.smooth) == (True, 0.7, 0.3, 0.5)


@pytest.mark.parametrize("argv", [["--radial", "--aniso", "-0.1"], ["--radial", "--aniso", "nan"], ["--radial", "--aniso", "inf"], ["--radial", "--resolution"],
                                  ["--radial", "--resolution", "--sigma", "0.05"]])
def test_cli_refuses_before_the_library(monkeypatch, tmp_path, argv):
    import dsurftomo_amd.engine as E

    def refuse(*_):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(E, "load_library", refuse)
    monkeypatch.setattr(io, "load", refuse)
    with pytest.raises(SystemExit) as exc:
        depth.main([str(tmp_path)] + argv)
    assert exc.value.code == 2


def test_run_refuses_before_the_engine_exists(monkeypatch, tmp_path, taipei):
    """a bad aniso and --radial with --resolution before the input is read; an input without Love periods (the Taipei example's) or without
    Rayleigh periods before the library is loaded"""
    import dsurftomo_amd.engine as E

    def refuse(*_):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(E, "load_library", refuse)
    real_load = io.load
    monkeypatch.setattr(io, "load", refuse)
    for aniso in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="--aniso"):
            depth.run(str(tmp_path), radial=True, aniso=aniso)
    with pytest.raises(ValueError, match="exclude"):
        depth.run(str(tmp_path), radial=True, resolution=True)
    depth.check(aniso=0.0)
    monkeypatch.setattr(io, "load", real_load)
    assert len(taipei["tLc"]) + len(taipei["tLg"]) == 0
    with pytest.raises(ValueError, match="Rayleigh and Love"):
        depth.run(io.HERE, radial=True, out_dir=str(tmp_path))
    with pytest.raises(ValueError, match="the input lists 0 and 1"):
        depth.check_radial(dict(small_case(taipei), tRc=np.zeros(0), tRg=np.zeros(0)))
    depth.check_radial(small_case(taipei))


def test_radial_files_round_trip(tmp_path, taipei):
    c = small_case(taipei)
    nx, ny, nz = 6, 5, 3
    rng = np.random.default_rng(12)
    vsv = (2.0 + 2.0 * rng.random((nz, ny, nx))).astype(F)
    vsh = (vsv * (1.0 + 0.05 * rng.standard_normal((nz, ny, nx)))).astype(F)
    path = str(tmp_path / "DepthRadial.dat")
    depth.write_radial(path, c, vsv, vsh)
    rows = depth.read_radial(path)
    assert len(rows) == nx * ny * nz
    v = vsv.ravel().astype(np.float64); w = vsh.ravel().astype(np.float64)
    assert [r["vsv"] for r in rows] == v.tolist() and [r["vsh"] for r in rows] == w.tolist()
    assert [r["voigt"] for r in rows] == np.sqrt((2.0 * v * v + w * w) / 3.0).tolist() and [r["xi"] for r in rows] == ((w / v) * (w / v)).tolist()
    assert [r["depth"] for r in rows[::nx * ny]] == [0.0, 2.0, 5.0]
    lon, lat = maps._lonlat(c, 0, 0)
    k = 1 * nx + 1
    assert rows[k]["lon"] == float(lon) and rows[k]["lat"] == float(lat)           # node order: Depth.dat's
    with open(path) as fh:
        assert re.search(r"\d\.\d{15,16}(e[-+]\d+)?\b", fh.read())               # 17 significant digits
    step = lambda seed: dict(nused=np.random.default_rng(seed).integers(0, 5, (2, nx * ny)).astype(np.int32), chi2=np.random.default_rng(seed).random((2, nx * ny)),
                             flag=np.random.default_rng(seed).integers(0, 3, nx * ny).astype(np.int32))
    first, last = step(1), step(2)
    fit = str(tmp_path / "DepthRadialFit.dat")
    depth.write_radial_fit(fit, c, first, last)
    rows = depth.read_radial_fit(fit)
    assert len(rows) == nx * ny
    assert [r["nused_r"] for r in rows] == last["nused"][0].tolist() and [r["nused_l"] for r in rows] == last["nused"][1].tolist()
    assert [r["flag"] for r in rows] == last["flag"].tolist()
    rms = lambda s, q, i: float(np.sqrt(s["chi2"][q][i] / s["nused"][q][i])) if s["nused"][q][i] else 0.0
    for i, r in enumerate(rows):
        assert (r["rms_first_r"], r["rms_last_r"], r["rms_first_l"], r["rms_last_l"]) == (rms(first, 0, i), rms(last, 0, i), rms(first, 1, i), rms(last, 1, i))
    # the log's xi: the unflagged interior columns above the bottom depth
    flag = np.zeros(nx * ny, np.int32); flag[1 * nx + 1] = 2
    ok = (R.interior(nx, ny) == 1) & (flag == 0)
    xi = ((vsh.reshape(nz, -1)[:nz - 1, ok].astype(np.float64) / vsv.reshape(nz, -1)[:nz - 1, ok]) ** 2)
    got = depth.xi_summary(c, vsv, vsh, flag)
    assert np.allclose(got, (np.median(xi), xi.min(), xi.max()), rtol=1e-15, atol=0)
    assert depth.xi_summary(c, vsv, vsh, np.full(nx * ny, 1)) is None


def test_new_symbols_declared_bound_and_exported():
    """declared in the public header, argtypes set by engine.py on both kinds of handle (load_library's and a bare CDLL through
    declare_solvers), Engine methods, exported by the built library; the new header is in the build's list"""
    from dsurftomo_amd import build
    from dsurftomo_amd import engine as E
    build.build()
    with open(os.path.join(L.ROOT, "include", "dsurftomo_amd.h")) as fh:
        header = fh.read()
    assert re.search(r"^int dsa_dispersion_begin_radial\(dsa_engine\* e, int nx, int ny, int nz, const float\* vsv, const float\* vsh, const float\* depz, float minthk,\s*"
                     r"int kmax_total, int nmaps_total\);", header, re.M)
    assert re.search(r"^int dsa_columns_step_radial\(dsa_engine\* e, int nmaps, const float\* obs, const float\* wt, float smooth, float damp, float aniso, float dvmax,\s*"
                     r"float minvel, float maxvel, float\* dv, int\* nused, double\* chi2, int\* flag\);", header, re.M)
    assert re.search(r"^int dsa_dispersion_get_model_radial\(dsa_engine\* e, float\* vsv, float\* vsh\);", header, re.M)
    lib = E.load_library()
    bare = E.declare_solvers(C.CDLL(build.LIB))
    for handle in (lib, bare):
        assert [len(getattr(handle, n).argtypes) for n in NEW] == [10, 14, 3]
    for method in ("dispersion_begin_radial", "columns_step_radial", "dispersion_get_model_radial"):
        assert callable(getattr(E.Engine, method))
    assert "column_radial.h" in build.HEADERS and "column_system.h" in build.HEADERS and "column_kernels.hip" in build.SOURCES
    assert os.path.exists(os.path.join(L.ROOT, "dsurftomo_amd", "csrc", "column_radial.h"))
    assert len(lib.dsa_columns_step.argtypes) == 13 and len(lib.dsa_columns_resolution.argtypes) == 12      # the old entry points are as they were
