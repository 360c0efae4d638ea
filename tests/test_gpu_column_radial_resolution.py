"""dsa_columns_resolution_radial (csrc/column_kernels.hip: k_column_resolution_radial) on the device against the CPU
build of the same header (tests/hostcheck_column_radial_resolution.cpp through column_radial_resolution_ref), bit for bit: the kernel shares
column_radial_resolution.h's loops out over a block of two wavefronts -- one lane per datum in the solves, one per unknown in the
reductions -- every figure is one sequential fp64 chain under -ffp-contract=off, so neither the lane mapping nor the number of lanes
can show.

tests/test_gpu_column_radial.py's grid and cases: 5 x 5 (9 interior columns), three periods of each of the four wave types (K = 12: slots 0-5
Rayleigh, 6-11 Love), nz = 2, 3, 8, smooth_model and edge_model, Vsh 3 % above Vsv; and once the stage's limits, nz = 64 with K = 60.  The
inputs of the host are the curves and kernels fetched from the device after the runs, so the dispersion stage's own arithmetic is not under
test."""
import os
import time

import numpy as np
import pytest

import column_radial_ref as RR
import column_radial_resolution_ref as RS
import columns_ref as R
from column_radial_ref import same_bits
from dsurftomo_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

F = np.float32
NX, NY, K = R.NX, R.NY, R.K
NCOL = NX * NY
RING = R.interior(NX, NY) == 0
CENTRE = 2 * NX + 2
DSA_ERR_ARGUMENT, DSA_ERR_STATE = -2, -5                      # include/dsurftomo_amd.h
ARGS = (R.SMOOTH, R.DAMP, RR.ANISO)
STEP = (R.SMOOTH, R.DAMP, RR.ANISO, R.DVMAX, R.MINVEL, R.MAXVEL)
FIGURES = ("measures", "pair", "leverage", "trace", "nused", "flag")


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def h():
    return RS.load()


@pytest.fixture(scope="module")
def hs():
    return R.load()


def runs(e, waves=R.WAVES):
    first = 0
    for wave, kind, t in waves:
        e.dispersion_run(wave, kind, t, True, first, first)
        first += len(t)


def above(vsv, factor=1.03):
    """Vsh = Vsv * factor above the bottom depth, equal at it (test_gpu_column_radial.py's)"""
    vsh = np.array(vsv, F, copy=True)
    vsh[:-1] = (vsh[:-1] * F(factor)).astype(F)
    return vsh


def case(model_name, nz):
    """test_gpu_column_radial.py's: weights around 1, a tenth of them 0, the centre column without any"""
    depz = R.depths(nz)
    vel = (R.smooth_model if model_name == "smooth" else R.edge_model)(NX, NY, nz)
    rng = np.random.default_rng(7 + nz)
    wt = (0.5 + rng.random((K, NCOL))).astype(F)
    wt[rng.random((K, NCOL)) < 0.1] = 0.0
    wt[:, CENTRE] = 0.0
    return depz, vel, rng, wt


def fetched(e, hs, vsv, vsh, depz, nmaps=K):
    """the curves and the combined sensitivities on both models that the resident runs left, as the host takes them"""
    nz = vsv.shape[0]
    pv, svs, svp, srho = e.dispersion_fetch(0, nmaps, True, 0)
    return pv, R.host_combine(hs, vsv.reshape(nz, -1), depz, svs, svp, srho), R.host_combine(hs, vsh.reshape(nz, -1), depz, svs, svp, srho)


def against_host(h, e, love, obs, wt, pv, Sv, Sh, depz, vsv, vsh, args=ARGS):
    """the device's figures, with and without the full R, and the host's on the fetched values: bit for bit.  Returns (device, host)."""
    nz = vsv.shape[0]
    want = RS.host_resolution(h, love, obs, wt, pv, Sv, Sh, depz, vsv.reshape(nz, NCOL), vsh.reshape(nz, NCOL), *args, R.interior(NX, NY))
    got = e.columns_resolution_radial(obs, wt, *args, full=True)
    for name in FIGURES + ("R",):
        assert same_bits(got[name], want[name]), "%s differs from the host's (%d of %d)" % (name, int((got[name] != want[name]).sum()), got[name].size)
    lean = e.columns_resolution_radial(obs, wt, *args)
    assert "R" not in lean
    for name in FIGURES:
        assert same_bits(lean[name], got[name]), "%s changes when R is not asked for" % name
    return got, want


@pytest.mark.parametrize("nz", [2, 3, 8])
@pytest.mark.parametrize("model_name", ["smooth", "edge"])
def test_resolution_equals_the_host_bit_for_bit(eng, h, hs, model_name, nz):
    """(a) and (b): every output equals the CPU build of the header, with the full R and without it; the ring is zeros, the column without
    weights is flag 2 and zeros, nothing is NaN; both models are as they were."""
    depz, vsv, rng, wt = case(model_name, nz)
    vsh = above(vsv)
    eng.dispersion_begin_radial(vsv, vsh, depz, R.MINTHK, K, K)
    runs(eng)
    pv, Sv, Sh = fetched(eng, hs, vsv, vsh, depz)
    obs = (2.5 + 1.5 * rng.random((K, NCOL))).astype(F)
    if model_name == "edge":
        assert (pv[:, ~RING] == 0).any() and (pv[:, ~RING] > 0).any(), "the edge model should lose some roots inside the ring at these periods"
    got, _ = against_host(h, eng, RR.LOVE, obs, wt, pv, Sv, Sh, depz, vsv, vsh)
    for name in FIGURES + ("R",):
        assert not got[name][..., RING].any(), name
        assert not got[name][..., CENTRE].any() or name == "flag", name
        assert np.isfinite(got[name]).all(), name
    assert got["flag"][CENTRE] == 2
    used = (wt > 0) & (obs > 0) & (pv > 0)
    assert (got["nused"][0][~RING] == used[~RR.LOVE].sum(axis=0)[~RING]).all() and (got["nused"][1][~RING] == used[RR.LOVE].sum(axis=0)[~RING]).all()
    ok = (got["flag"] == 0) & ~RING
    assert ok.any() and (got["trace"].sum(axis=0)[ok] > 0).all() and (got["measures"][5][:, ok] > 0).all() and (got["pair"][1][:, ok] > 0).all()
    assert np.abs(got["measures"][3][:, ok]).max() > 0                                   # (the tie leaks)
    models = eng.dispersion_get_model_radial()
    assert same_bits(models[0], vsv) and same_bits(models[1], vsh)
    against_host(h, eng, RR.LOVE, obs, None, pv, Sv, Sh, depz, vsv, vsh)            # without weights: all 1


def test_the_call_is_read_only(eng):
    """(c): runs, columns_resolution_radial, columns_step_radial give the bits of runs, columns_step_radial in every output and in both
    models; after the step the call is DSA_ERR_STATE until the runs are repeated"""
    nz = 8
    depz, vsv, rng, wt = case("smooth", nz)
    vsh = above(vsv)
    obs = (2.5 + 1.5 * rng.random((K, NCOL))).astype(F)
    eng.dispersion_begin_radial(vsv, vsh, depz, R.MINTHK, K, K)
    runs(eng)
    plain = eng.columns_step_radial(obs, wt, *STEP)
    plain_models = eng.dispersion_get_model_radial()
    eng.dispersion_begin_radial(vsv, vsh, depz, R.MINTHK, K, K)
    runs(eng)
    first = eng.columns_resolution_radial(obs, wt, *ARGS, full=True)
    models = eng.dispersion_get_model_radial()
    assert same_bits(models[0], vsv) and same_bits(models[1], vsh)
    again = eng.columns_resolution_radial(obs, wt, *ARGS, full=True)                  # (the marks stay: a second call needs no new runs)
    for name in first:
        assert same_bits(first[name], again[name]), name
    step = eng.columns_step_radial(obs, wt, *STEP)
    for name in ("dv_sv", "dv_sh", "chi2", "nused", "flag"):
        assert same_bits(step[name], plain[name]), name
    after = eng.dispersion_get_model_radial()
    assert same_bits(after[0], plain_models[0]) and same_bits(after[1], plain_models[1]) and np.abs(step["dv_sv"]).max() > 0
    with pytest.raises(EngineError, match="has not been run") as exc:
        eng.columns_resolution_radial(obs, wt, *ARGS)
    assert exc.value.code == DSA_ERR_STATE
    runs(eng)
    assert (eng.columns_resolution_radial(obs, wt, *ARGS)["flag"][~RING & (wt > 0).any(axis=0)] == 0).all()


@pytest.mark.parametrize("nz", [2, 3, 8])
def test_aniso_zero_is_columns_resolution_on_each_model(eng, nz):
    """(d): aniso = 0: R_jj, m1_own, m2_own, var and the own block of R of the Vsv block, and the Rayleigh leverages, are
    dsa_columns_resolution's on a plain stage holding vsv with the Love weights zeroed, those of the Vsh block and the Love leverages its
    figures on a plain stage holding vsh with the Rayleigh weights zeroed -- bit for bit; m1_cross, R_cross and cov are zeros"""
    depz, vsv, rng, wt = case("smooth", nz)
    vsh = above(vsv)
    M = nz - 1
    love = RR.LOVE
    obs = (2.5 + 1.5 * rng.random((K, NCOL))).astype(F)
    want = []
    for vel, mine in ((vsv, ~love), (vsh, love)):
        eng.dispersion_begin(vel, depz, R.MINTHK, K, K)
        runs(eng)
        want.append(eng.columns_resolution(obs, np.where(mine[:, None], wt, F(0.0)), R.SMOOTH, R.DAMP, full=True))
    eng.dispersion_begin_radial(vsv, vsh, depz, R.MINTHK, K, K)
    runs(eng)
    got = eng.columns_resolution_radial(obs, wt, R.SMOOTH, R.DAMP, 0.0, full=True)
    both = (got["nused"][0] > 0) & (got["nused"][1] > 0) & (got["flag"] == 0)
    assert both[~RING].sum() >= 8
    for q, mine in enumerate((~love, love)):
        out = want[q]
        blk = slice(q * M, (q + 1) * M)
        assert same_bits(got["nused"][q], out["nused"]) and same_bits(got["flag"][both], out["flag"][both])
        for mine_q, theirs in ((0, 0), (1, 1), (2, 2), (5, 3)):
            assert same_bits(got["measures"][mine_q][blk][:, both], out["measures"][theirs][:, both]), (q, mine_q)
        assert same_bits(got["leverage"][mine][:, both], out["leverage"][mine][:, both]) and same_bits(got["trace"][q][both], out["trace"][both])
        assert same_bits(got["R"][blk, blk][:, :, both], out["R"][:, :, both]) and np.abs(out["R"][:, :, both]).max() > 0
    assert not got["measures"][3].any() and not got["measures"][4].any() and not got["pair"][0].any()
    assert not got["R"][:M, M:].any() and not got["R"][M:, :M].any()
    var = got["measures"][5]
    assert (np.abs(got["pair"][1] - (var[:M] + var[M:])) <= RS.TOL * got["pair"][1].max()).all()


@pytest.mark.parametrize("nz", [3, 8])
def test_resolution_predicts_the_devices_step(eng, h, hs, nz):
    """(e): equal starting models and obs = fl32(pv + S^ m) for a random m of a few per cent: the device's radial step, dvmax large, is
    R m + T^T e rounded to fp32, with e_k = a_k (obs_k - pv_k - (S^ m)_k) in fp64, R the device's and T the host's (the device does not
    return it; its figures equal the host's bit for bit).  Within the measured tolerance of the comparison plus one rounding to fp32."""
    depz, vsv, rng, wt = case("smooth", nz)
    M = nz - 1
    love = RR.LOVE
    eng.dispersion_begin_radial(vsv, vsv, depz, R.MINTHK, K, K)
    runs(eng)
    pv, Sv, Sh = fetched(eng, hs, vsv, vsv, depz)
    assert (pv[:, ~RING] > 0).all()
    m = 0.1 * (rng.random((2 * M, NCOL)) - 0.5)
    Sm = np.where(love[:, None], np.einsum("lkc,lc->kc", Sh, m[M:]), np.einsum("lkc,lc->kc", Sv, m[:M]))
    obs = (pv + Sm).astype(F)
    got, want = against_host(h, eng, love, obs, wt, pv, Sv, Sh, depz, vsv, vsv)
    step = eng.columns_step_radial(obs, wt, R.SMOOTH, R.DAMP, RR.ANISO, 1e3, -1e3, 1e3)
    dv = np.concatenate([step["dv_sv"], step["dv_sh"]]).astype(np.float64)
    used = (wt > 0) & (obs > 0) & (pv > 0)
    e = np.where(used, wt.astype(np.float64) * (obs.astype(np.float64) - pv - Sm), 0.0)
    worst = 0.0
    for c in np.flatnonzero(~RING):
        if c == CENTRE:
            assert step["flag"][c] == 2 and not dv[:, c].any()
            continue
        assert step["flag"][c] == 0 and got["flag"][c] == 0
        pred = got["R"][:, :, c] @ m[:, c] + want["T"][:, :, c].T @ e[:, c]
        scale = max(np.abs(pred).max(), np.abs(got["R"][:, :, c]).max() * np.abs(m[:, c]).max())
        err = np.abs(dv[:, c] - pred)
        worst = max(worst, float((err / scale).max()))
        assert (err <= RS.TOL * scale + np.spacing(np.abs(pred).astype(F)).astype(np.float64)).all()
    print("nz %d: largest |dv - (R m + T^T e)| / scale %.3g (one fp32 rounding is 6e-8)" % (nz, worst))
    assert np.abs(dv).max() > 1e-3


def test_the_limits_once(eng, h, hs):
    """(f): nz = 64 (2M = 126 unknowns), K = 60 -- test_gpu_column_resolution.py's period lists -- smooth_model on the 5 x 5 grid, Vsh 3 %
    above Vsv: the one launch that asks for 158 712 bytes of LDS.  Equal to the host bit for bit, all nine interior columns resolved."""
    nz, nmaps = 64, 60
    waves = [(2, 0, np.linspace(3.0, 45.0, 15)), (2, 1, np.linspace(4.0, 46.0, 15)), (1, 0, np.linspace(3.0, 45.0, 15)), (1, 1, np.linspace(4.0, 46.0, 15))]
    love = np.concatenate([np.full(len(t), wave == 1) for wave, _, t in waves])
    depz = R.depths(nz)
    vsv = R.smooth_model(NX, NY, nz)
    vsh = above(vsv)
    assert h.hrr_doubles(nz - 1, nmaps) * 8 == 158712 <= 163840
    eng.dispersion_begin_radial(vsv, vsh, depz, R.MINTHK, nmaps, nmaps)
    t0 = time.perf_counter()
    runs(eng, waves)
    t1 = time.perf_counter()
    pv, Sv, Sh = fetched(eng, hs, vsv, vsh, depz, nmaps)
    obs = np.where(pv > 0, pv * 1.01, 3.0).astype(F)
    t2 = time.perf_counter()
    got, _ = against_host(h, eng, love, obs, None, pv, Sv, Sh, depz, vsv, vsh)
    t3 = time.perf_counter()
    print("nz 64, K 60: the four dispersion runs %.3f s, two resolution calls and the host's %.3f s; roots %d of %d, traces %.4f to %.4f (Vsv) and %.4f to %.4f (Vsh)" %
          (t1 - t0, t3 - t2, int((pv[:, ~RING] > 0).sum()), 9 * nmaps, got["trace"][0][~RING].min(), got["trace"][0][~RING].max(), got["trace"][1][~RING].min(),
           got["trace"][1][~RING].max()))
    assert (got["flag"][~RING] == 0).all() and not got["flag"][RING].any()
    assert np.isfinite(got["R"]).all() and (got["trace"][:, ~RING] > 0).all() and (got["trace"][:, ~RING] < nz - 1).all()


def test_refusals(eng):
    """(g): a plain stage, a bad aniso, each NULL output, stale marks -- the code of each, found before the device is touched: the runs stay
    fresh and the models unchanged, so the good call after each succeeds without new runs"""
    nz = 3
    depz, vsv, rng, wt = case("smooth", nz)
    vsh = above(vsv)
    obs = np.full((K, NCOL), 3.0, F)

    def refused(call, match, code):
        with pytest.raises(EngineError, match=match) as exc:
            call()
        assert exc.value.code == code

    def usable():
        assert (eng.columns_resolution_radial(obs, wt, *ARGS)["flag"][~RING & (wt > 0).any(axis=0)] == 0).all()

    eng.dispersion_begin(vsv, depz, R.MINTHK, K, K)
    runs(eng)
    refused(lambda: eng.columns_resolution_radial(obs, None, *ARGS), "not radial", DSA_ERR_STATE)
    assert (eng.columns_resolution(obs, None, R.SMOOTH, R.DAMP)["flag"][~RING] == 0).all()      # the plain stage is as usable as before
    eng.dispersion_begin_radial(vsv, vsh, depz, R.MINTHK, K, K)
    refused(lambda: eng.columns_resolution_radial(obs, None, *ARGS), "has not been run", DSA_ERR_STATE)      # no runs since begin
    runs(eng)
    usable()
    refused(lambda: eng.columns_resolution(obs, None, R.SMOOTH, R.DAMP), "is radial", DSA_ERR_STATE)          # stays refused as it is
    usable()
    for bad in (-0.1, np.nan, np.inf):
        refused(lambda: eng.columns_resolution_radial(obs, None, R.SMOOTH, R.DAMP, bad), "aniso", DSA_ERR_ARGUMENT)
    refused(lambda: eng.columns_resolution_radial(obs, None, R.SMOOTH, 0.0, RR.ANISO), "damp", DSA_ERR_ARGUMENT)
    refused(lambda: eng.columns_resolution_radial(obs, None, -0.5, R.DAMP, RR.ANISO), "smooth", DSA_ERR_ARGUMENT)
    refused(lambda: eng.columns_resolution_radial(obs[:K - 1], None, *ARGS), "maps given", DSA_ERR_ARGUMENT)
    w = wt.copy(); w[5, 7] = -1.0
    refused(lambda: eng.columns_resolution_radial(obs, w, *ARGS), "wt", DSA_ERR_ARGUMENT)
    usable()
    # the required outputs, through the library itself: the binding always passes them
    import ctypes as C
    lib = eng._L
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    M = nz - 1
    meas = np.zeros((6, 2 * M, NCOL)); pair = np.zeros((2, M, NCOL)); lev = np.zeros((K, NCOL)); tr = np.zeros((2, NCOL))
    nu = np.zeros((2, NCOL), np.int32); fl = np.zeros(NCOL, np.int32)
    outs = [p(meas), p(pair), p(lev), p(tr), p(nu), p(fl), None]
    for missing in range(6):
        args = list(outs); args[missing] = None
        assert lib.dsa_columns_resolution_radial(eng._h, K, p(obs), None, *ARGS, *args) == DSA_ERR_ARGUMENT
        assert b"required" in lib.dsa_error_string(eng._h)
    assert lib.dsa_columns_resolution_radial(eng._h, K, p(obs), None, *ARGS, *outs) == 0 and tr[:, ~RING].all()
    assert lib.dsa_columns_resolution_radial(eng._h, K, None, None, *ARGS, *outs) == DSA_ERR_ARGUMENT
    usable()
    # stale marks
    eng.dispersion_run(1, 0, R.WAVES[2][2], False, 0, 6)                           # the Love maps again without kernels: no slot answers for them
    refused(lambda: eng.columns_resolution_radial(obs, None, *ARGS), "slot 6 has not been run", DSA_ERR_STATE)
    runs(eng)
    eng.dispersion_run(2, 0, R.WAVES[0][2], True, 3, 0)                            # the first wave type's kernels into the second's slots
    refused(lambda: eng.columns_resolution_radial(obs, None, *ARGS), "hold different curves", DSA_ERR_STATE)
    runs(eng)
    usable()
    eng.columns_step_radial(obs, wt, *STEP)
    refused(lambda: eng.columns_resolution_radial(obs, wt, *ARGS), "has not been run", DSA_ERR_STATE)         # after a step, until the runs are repeated
    runs(eng)
    usable()


def test_the_driver_end_to_end(eng, tmp_path):
    """depth.run_radial and then depth.resolve_radial (what --radial --radial-resolution runs) on the Taipei example's grid and model
    (18 x 18 x 9) with its 26 periods dealt out over the four wave types, test_gpu_column_radial.py's observations: the two files hold the
    call's figures, the log its summary, and the models are the loop's"""
    from dsurftomo_amd import depth, io
    c = io.load()
    t = np.asarray(c["tRc"], np.float64)
    c = dict(c, tRc=t[:7], tRg=t[7:14], tLc=t[14:20], tLg=t[20:])
    plan = depth.slot_plan(c)
    kmax, nx, ny, nz = c["kmax"], c["nx"], c["ny"], c["nz"]
    M = nz - 1
    start = np.ascontiguousarray(np.asarray(c["vels"], F).transpose(2, 1, 0))
    eng.dispersion_begin_radial(start, RR.truth_vsh(start, 0.05), c["depz"], c["minthk"], kmax, kmax)
    for wave, kind, tt, first in plan:
        eng.dispersion_run(wave, kind, tt, False, 0, first)
    obs = eng.dispersion_fetch(0, kmax).astype(F)
    lines = []
    out, _, _ = depth.run_radial(eng, c, plan, obs, None, 2, 0.2, 0.05, depth.DEFAULT_ANISO, 0.3, str(tmp_path), lines.append)
    sigma = 0.02
    res = depth.resolve_radial(eng, c, plan, obs, None, 0.2, 0.05, depth.DEFAULT_ANISO, sigma, str(tmp_path), lines.append)
    print("\n".join(lines))
    r = res["resolution"]
    inner = R.interior(nx, ny) == 1
    assert not r["flag"].any() and (r["nused"][:, inner] > 0).all() and res["summary"]["columns"] == int(inner.sum())
    models = eng.dispersion_get_model_radial()
    assert same_bits(models[0], out["vsv"]) and same_bits(models[1], out["vsh"])            # the call left the loop's models
    rows = depth.read_radial_resolution(res["resolution_path"])
    assert len(rows) == M * nx * ny
    cols = depth.radial_resolution_columns(r, out["vsv"].reshape(nz, -1), out["vsh"].reshape(nz, -1), sigma)
    for name in depth.RADIAL_RESOLUTION_NAMES:
        assert [row[name] for row in rows] == cols[name].ravel().tolist(), name
    assert (cols["leak_h"][:, inner] > 0).all() and (cols["leak_v"][:, inner] < 1).all() and (cols["sd_xi"][:, inner] > 0).all()
    lev = depth.read_radial_leverage(res["leverage_path"])
    assert [row["leverage"] for row in lev] == r["leverage"].T.ravel().tolist()
    assert any("Vsv block" in ln and "median leak share" in ln for ln in lines) and any("|xi - 1| > 2 sd_xi" in ln for ln in lines)
    assert os.path.basename(res["resolution_path"]) == "DSurfTomo.inDepthRadialResolution.dat"
    assert os.path.basename(res["leverage_path"]) == "DSurfTomo.inDepthRadialLeverage.dat"
