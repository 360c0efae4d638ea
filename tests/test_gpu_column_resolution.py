"""dsa_columns_resolution (csrc/column_kernels.hip: k_column_resolution) on the device against the CPU build of the same
header (tests/hostcheck_column_resolution.cpp through column_resolution_ref), bit for bit: the kernel shares column_resolution.h's loops out
over a wavefront -- one lane per datum in the solves, one per unknown in the reductions -- every figure is one sequential fp64 chain under
-ffp-contract=off, there is no square root and the division is IEEE, so the lane mapping cannot show.

tests/test_gpu_columns.py's cases: grid 5 x 5 (9 interior columns), three periods of each of the four wave types (K = 12), nz = 2, 3, 8,
smooth_model and edge_model (columns without a Love root at these periods); and once the stage's limits, nz = 64 with K = 60.  The inputs
of the host are the curves and kernels fetched from the device after the runs, so the dispersion stage's own arithmetic is not under test."""
import time

import numpy as np
import pytest

import column_resolution_ref as CR
import columns_ref as R
from column_resolution_ref import same_bits
from dsurftomo_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

F = np.float32
NX, NY, K = R.NX, R.NY, R.K
NCOL = NX * NY
RING = R.interior(NX, NY) == 0
CENTRE = 2 * NX + 2
DSA_ERR_ARGUMENT, DSA_ERR_STATE = -2, -5                      # include/dsurftomo_amd.h
STEP = (R.SMOOTH, R.DAMP, R.DVMAX, R.MINVEL, R.MAXVEL)
FIGURES = ("measures", "leverage", "trace", "nused", "flag")


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def h():
    return CR.load()


@pytest.fixture(scope="module")
def hs():
    return R.load()


def runs(e, waves=R.WAVES):
    first = 0
    for wave, kind, t in waves:
        e.dispersion_run(wave, kind, t, True, first, first)
        first += len(t)


def case(model_name, nz):
    """test_gpu_columns.py's: weights around 1, a tenth of them 0, the centre column without any"""
    depz = R.depths(nz)
    vel = (R.smooth_model if model_name == "smooth" else R.edge_model)(NX, NY, nz)
    rng = np.random.default_rng(7 + nz)
    wt = (0.5 + rng.random((K, NCOL))).astype(F)
    wt[rng.random((K, NCOL)) < 0.1] = 0.0
    wt[:, CENTRE] = 0.0
    return depz, vel, rng, wt


def fetched(e, hs, model, depz, nmaps=K):
    """the curves and the combined sensitivities the resident runs left, as the host takes them"""
    nz = model.shape[0]
    pv, svs, svp, srho = e.dispersion_fetch(0, nmaps, True, 0)
    return pv, R.host_combine(hs, model.reshape(nz, -1), depz, svs, svp, srho)


def against_host(h, e, obs, wt, pv, S, depz, smooth=R.SMOOTH, damp=R.DAMP):
    """the device's figures, with and without the full R, and the host's on the fetched values: bit for bit.  Returns (device, host)."""
    nx_ny = pv.shape[1]
    side = int(round(np.sqrt(nx_ny)))
    want = CR.host_resolution(h, obs, wt, pv, S, depz, smooth, damp, R.interior(side, side))
    got = e.columns_resolution(obs, wt, smooth, damp, full=True)
    for name in FIGURES + ("R",):
        assert same_bits(got[name], want[name]), "%s differs from the host's (%d of %d)" % (name, int((got[name] != want[name]).sum()), got[name].size)
    lean = e.columns_resolution(obs, wt, smooth, damp)
    assert "R" not in lean
    for name in FIGURES:
        assert same_bits(lean[name], got[name]), "%s changes when R is not asked for" % name
    return got, want


@pytest.mark.parametrize("nz", [2, 3, 8])
@pytest.mark.parametrize("model_name", ["smooth", "edge"])
def test_resolution_equals_the_host_bit_for_bit(eng, h, hs, model_name, nz):
    """(a) and (b): every output equals the CPU build of the header, with the full R and without it; the ring is zeros, a column without
    weights is flag 2 and zeros, a datum without a root is dropped, nothing is NaN; the model is as it was."""
    depz, vel, rng, wt = case(model_name, nz)
    eng.dispersion_begin(vel, depz, R.MINTHK, K, K)
    runs(eng)
    pv, S = fetched(eng, hs, vel, depz)
    obs = (2.5 + 1.5 * rng.random((K, NCOL))).astype(F)
    if model_name == "edge":
        assert (pv[:, ~RING] == 0).any() and (pv[:, ~RING] > 0).any(), "the edge model should lose some roots inside the ring at these periods"
    got, _ = against_host(h, eng, obs, wt, pv, S, depz)
    for name in FIGURES + ("R",):
        assert not got[name][..., RING].any(), name
        assert not got[name][..., CENTRE].any() or name == "flag", name
        assert np.isfinite(got[name]).all(), name
    assert got["flag"][CENTRE] == 2
    used = ((wt > 0) & (obs > 0) & (pv > 0)).sum(axis=0)
    assert (got["nused"][~RING] == used[~RING]).all()
    ok = (got["flag"] == 0) & ~RING
    assert ok.any() and (got["trace"][ok] > 0).all() and (got["measures"][3][:, ok] > 0).all()
    assert same_bits(eng.dispersion_get_model(), vel)
    against_host(h, eng, obs, None, pv, S, depz)                                   # without weights: all 1


def test_the_call_is_read_only(eng):
    """(c): runs, columns_resolution, columns_step give the bits of runs, columns_step in dv, chi2, nused, flag and the model; after the
    step the call is DSA_ERR_STATE until the runs are repeated"""
    nz = 8
    depz, vel, rng, wt = case("smooth", nz)
    obs = (2.5 + 1.5 * rng.random((K, NCOL))).astype(F)
    eng.dispersion_begin(vel, depz, R.MINTHK, K, K)
    runs(eng)
    plain = eng.columns_step(obs, wt, *STEP)
    plain_model = eng.dispersion_get_model()
    eng.dispersion_begin(vel, depz, R.MINTHK, K, K)
    runs(eng)
    first = eng.columns_resolution(obs, wt, R.SMOOTH, R.DAMP, full=True)
    assert same_bits(eng.dispersion_get_model(), vel)
    again = eng.columns_resolution(obs, wt, R.SMOOTH, R.DAMP, full=True)           # (the marks stay: a second call needs no new runs)
    for name in first:
        assert same_bits(first[name], again[name]), name
    step = eng.columns_step(obs, wt, *STEP)
    for name in ("dv", "chi2", "nused", "flag"):
        assert same_bits(step[name], plain[name]), name
    assert same_bits(eng.dispersion_get_model(), plain_model) and np.abs(step["dv"]).max() > 0
    with pytest.raises(EngineError, match="has not been run") as exc:
        eng.columns_resolution(obs, wt, R.SMOOTH, R.DAMP)
    assert exc.value.code == DSA_ERR_STATE
    runs(eng)
    assert (eng.columns_resolution(obs, wt, R.SMOOTH, R.DAMP)["flag"][~RING & (wt > 0).any(axis=0)] == 0).all()


@pytest.mark.parametrize("nz", [3, 8])
def test_resolution_predicts_the_devices_step(eng, h, hs, nz):
    """(d): obs = fl32(pv + S m) for a random m of a few per cent: the device's step, dvmax large, is R m + T^T e rounded to fp32, with
    e_k = a_k (obs_k - pv_k - (S m)_k) in fp64, R the device's and T the host's (the device does not return it; its figures equal the
    host's bit for bit).  Within the measured tolerance of the comparison plus one rounding to fp32."""
    depz, vel, rng, wt = case("smooth", nz)
    M = nz - 1
    eng.dispersion_begin(vel, depz, R.MINTHK, K, K)
    runs(eng)
    pv, S = fetched(eng, hs, vel, depz)
    assert (pv[:, ~RING] > 0).all()
    m = 0.1 * (rng.random((M, NCOL)) - 0.5)
    Sm = np.einsum("lkc,lc->kc", S, m)
    obs = (pv + Sm).astype(F)
    got, want = against_host(h, eng, obs, wt, pv, S, depz)
    step = eng.columns_step(obs, wt, R.SMOOTH, R.DAMP, 1e3, -1e3, 1e3)
    used = (wt > 0) & (obs > 0) & (pv > 0)
    e = np.where(used, wt.astype(np.float64) * (obs.astype(np.float64) - pv - Sm), 0.0)
    worst = 0.0
    for c in np.flatnonzero(~RING):
        if c == CENTRE:
            assert step["flag"][c] == 2 and not step["dv"][:, c].any()
            continue
        assert step["flag"][c] == 0 and got["flag"][c] == 0
        pred = got["R"][:, :, c] @ m[:, c] + want["T"][:, :, c].T @ e[:, c]
        scale = max(np.abs(pred).max(), np.abs(got["R"][:, :, c]).max() * np.abs(m[:, c]).max())
        err = np.abs(step["dv"][:, c].astype(np.float64) - pred)
        worst = max(worst, float((err / scale).max()))
        assert (err <= CR.TOL * scale + np.spacing(np.abs(pred).astype(F)).astype(np.float64)).all()
    print("nz %d: largest |dv - (R m + T^T e)| / scale %.3g (one fp32 rounding is 6e-8)" % (nz, worst))
    assert np.abs(step["dv"]).max() > 1e-3


def test_the_limits_once(eng, h, hs):
    """(e): nz = 64 (M = 63), K = 60 -- 15 phase periods linspace(3, 45, 15) and 15 group periods linspace(4, 46, 15) of each wave type --
    smooth_model on the 5 x 5 grid: the one launch that asks for more than 64 KB of LDS (79 080 bytes).  Equal to the host bit for bit,
    and at least one interior column is resolved."""
    nz, nmaps = 64, 60
    waves = [(2, 0, np.linspace(3.0, 45.0, 15)), (2, 1, np.linspace(4.0, 46.0, 15)), (1, 0, np.linspace(3.0, 45.0, 15)), (1, 1, np.linspace(4.0, 46.0, 15))]
    depz = R.depths(nz)
    vel = R.smooth_model(NX, NY, nz)
    eng.dispersion_begin(vel, depz, R.MINTHK, nmaps, nmaps)
    t0 = time.perf_counter()
    runs(eng, waves)
    t1 = time.perf_counter()
    pv, S = fetched(eng, hs, vel, depz, nmaps)
    obs = np.where(pv > 0, pv, 3.0).astype(F)
    assert CR.load().hcr_doubles(nz - 1, nmaps) * 8 == 79080 > 64 * 1024
    t2 = time.perf_counter()
    got, _ = against_host(h, eng, obs, None, pv, S, depz)
    t3 = time.perf_counter()
    ok = (got["flag"] == 0) & ~RING
    print("nz 64, K 60: the four dispersion runs %.3f s, two resolution calls and the host's %.3f s; %d of 9 interior columns resolved, roots %d of %d, trace %.4f to %.4f" %
          (t1 - t0, t3 - t2, int(ok.sum()), int((pv[:, ~RING] > 0).sum()), 9 * nmaps, got["trace"][ok].min() if ok.any() else 0.0, got["trace"][ok].max() if ok.any() else 0.0))
    assert ok.any()
    assert np.isfinite(got["R"]).all() and (got["trace"][ok] > 0).all() and (got["trace"][ok] < nz - 1).all()


def test_refusals(eng):
    """(f): every bad argument is DSA_ERR_ARGUMENT and every bad state DSA_ERR_STATE, found before the device is touched -- the runs stay
    fresh and the model unchanged, so the good call after each succeeds without new runs"""
    nz = 3
    depz, vel, rng, wt = case("smooth", nz)
    obs = np.full((K, NCOL), 3.0, F)
    codes = []

    def refused(match, o=obs, w=None, smooth=R.SMOOTH, damp=R.DAMP):
        with pytest.raises(EngineError, match=match) as exc:
            eng.columns_resolution(o, w, smooth, damp)
        codes.append(exc.value.code)

    def usable():
        assert (eng.columns_resolution(obs, wt, R.SMOOTH, R.DAMP)["flag"][~RING & (wt > 0).any(axis=0)] == 0).all()

    eng.dispersion_begin(vel, depz, R.MINTHK, K, K)
    refused("has not been run")                                                    # no runs since begin
    assert codes == [DSA_ERR_STATE]
    runs(eng)
    usable()
    del codes[:]
    for bad in (-1.0, np.nan, np.inf):
        w = wt.copy(); w[5, 7] = bad
        refused("wt", w=w)
    refused("damp", damp=0.0)
    refused("damp", damp=-0.1)
    refused("damp", damp=np.nan)
    refused("smooth", smooth=-0.5)
    refused("smooth", smooth=np.inf)
    refused("maps given", o=obs[:K - 1])
    o = obs.copy(); o[0, 0] = np.nan
    refused("obs", o=o)
    assert set(codes) == {DSA_ERR_ARGUMENT} and len(codes) == 10
    usable()
    # the required outputs, through the library itself: the binding always passes them
    import ctypes as C
    lib = eng._L
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    meas = np.zeros((4, nz - 1, NCOL)); lev = np.zeros((K, NCOL)); tr = np.zeros(NCOL); nu = np.zeros(NCOL, np.int32); fl = np.zeros(NCOL, np.int32)
    outs = [p(meas), p(lev), p(tr), None, p(nu), p(fl)]
    for missing in (0, 1, 2, 4, 5):
        args = list(outs); args[missing] = None
        assert lib.dsa_columns_resolution(eng._h, K, p(obs), None, R.SMOOTH, R.DAMP, *args) == DSA_ERR_ARGUMENT
        assert b"required" in lib.dsa_error_string(eng._h)
    assert lib.dsa_columns_resolution(eng._h, K, p(obs), None, R.SMOOTH, R.DAMP, *outs) == 0 and tr[~RING].all()
    assert lib.dsa_columns_resolution(eng._h, K, None, None, R.SMOOTH, R.DAMP, *outs) == DSA_ERR_ARGUMENT
    usable()
    # states
    del codes[:]
    eng.dispersion_run(1, 0, R.WAVES[2][2], False, 0, 6)                           # the Love maps again without kernels: no slot answers for them
    refused("slot 6 has not been run")
    runs(eng)
    eng.dispersion_run(2, 0, R.WAVES[0][2], True, 3, 0)                            # the first wave type's kernels into the second's slots
    refused("hold different curves")
    runs(eng)
    usable()
    eng.dispersion_begin_models(np.stack([vel, vel]), depz, R.MINTHK, K)
    eng.dispersion_run(*R.WAVES[0], False, 0, 0)
    refused("2 models")
    assert set(codes) == {DSA_ERR_STATE} and len(codes) == 3
    eng.dispersion_begin(vel, depz, R.MINTHK, K, K)
    runs(eng)
    usable()
    assert same_bits(eng.dispersion_get_model(), vel)
