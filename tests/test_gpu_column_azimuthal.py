"""dsa_columns_azimuthal (csrc/column_kernels.hip: k_column_azimuthal) on the device against the CPU build of the same
header (tests/hostcheck_column_azimuthal.cpp through column_azimuthal_ref), bit for bit: the kernel shares column_azimuthal.h's loops out over
a wavefront -- one lane per datum and one per right-hand side in the solves, one per unknown in the reductions -- every figure is one
sequential fp64 chain under -ffp-contract=off, there is no square root and the division is IEEE, so the lane mapping cannot show.

tests/test_gpu_columns.py's cases: grid 5 x 5 (9 interior columns), three periods of each of the four wave types (K = 12: 6 Rayleigh data, 6
Love slots that must be dropped), nz = 2, 3, 8, smooth_model and edge_model, weights with zeros and the centre column all zero; and once the
stage's limits, nz = 64 with K = 60.  The inputs of the host are the curves and the Vs kernels fetched from the device after the runs, with
Z made by depth.azimuthal_factor from the fetched model, so the dispersion stage's own arithmetic is not under test."""
import ctypes as C

import numpy as np
import pytest

import column_azimuthal_ref as CA
import column_resolution_ref as CR
import columns_ref as R
from column_azimuthal_ref import same_bits
from dsurftomo_amd import depth
from dsurftomo_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

F = np.float32
NX, NY, K = R.NX, R.NY, R.K
NCOL = NX * NY
INNER = R.interior(NX, NY)
RING = INNER == 0
CENTRE = 2 * NX + 2
LOVE = np.array([wave == 1 for wave, _, t in R.WAVES for _ in t])
DSA_ERR_ARGUMENT, DSA_ERR_STATE = -2, -5                      # include/dsurftomo_amd.h
STEP = (R.SMOOTH, R.DAMP, R.DVMAX, R.MINVEL, R.MAXVEL)
FIGURES = ("gc", "gs", "measures", "leverage", "chi2", "nused", "flag")
LIMIT_WAVES = [(2, 0, np.linspace(3.0, 45.0, 15)), (2, 1, np.linspace(4.0, 46.0, 15)), (1, 0, np.linspace(3.0, 45.0, 15)), (1, 1, np.linspace(4.0, 46.0, 15))]


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def h():
    return CA.load()


def runs(e, waves=R.WAVES):
    first = 0
    for wave, kind, t in waves:
        e.dispersion_run(wave, kind, t, True, first, first)
        first += len(t)


def case(model_name, nz):
    """test_gpu_columns.py's: weights around 1, a tenth of them 0, the centre column without any; A1, A2 of a few per cent of c0, both signs"""
    depz = R.depths(nz)
    vel = (R.smooth_model if model_name == "smooth" else R.edge_model)(NX, NY, nz)
    rng = np.random.default_rng(7 + nz)
    wt = (0.5 + rng.random((K, NCOL))).astype(F)
    wt[rng.random((K, NCOL)) < 0.1] = 0.0
    wt[:, CENTRE] = 0.0
    obs = (2.5 + 1.5 * rng.random((K, NCOL))).astype(F)
    a1 = (0.03 * obs * rng.standard_normal((K, NCOL))).astype(F)
    a2 = (0.03 * obs * rng.standard_normal((K, NCOL))).astype(F)
    return depz, vel, wt, obs, a1, a2


def fetched(e, nmaps=K):
    """the curves and the depth factor Z of the resident runs and model, as the host takes them; and everything fetched, for the bits"""
    model = e.dispersion_get_model()
    got = e.dispersion_fetch(0, nmaps, True, 0)
    return got[0], depth.azimuthal_factor(got[1], model), (model,) + tuple(got)


def against_host(h, e, obs, a1, a2, wt, pv, Z, love, depz, smooth=R.SMOOTH, damp=R.DAMP):
    """the device's figures and the host's on the fetched values: bit for bit.  Returns (device, host)."""
    want = CA.host_azimuthal(h, obs, a1, a2, wt, pv, Z, love, depz, smooth, damp, INNER)
    got = e.columns_azimuthal(obs, a1, a2, wt, smooth, damp)
    for name in FIGURES:
        assert same_bits(got[name], want[name]), "%s differs from the host's (%d of %d)" % (name, int((got[name] != want[name]).sum()), got[name].size)
    return got, want


@pytest.mark.parametrize("nz", [2, 3, 8])
@pytest.mark.parametrize("model_name", ["smooth", "edge"])
def test_azimuthal_equals_the_host_bit_for_bit(eng, h, model_name, nz):
    """(a) and (c): every output equals the CPU build of the header, with and without weights; the ring is zeros, the centre column is flag
    2 and zeros, the leverage is 0 at Love and unused slots, nothing is NaN, nused is the count of the rule"""
    depz, vel, wt, obs, a1, a2 = case(model_name, nz)
    eng.dispersion_begin(vel, depz, R.MINTHK, K, K)
    runs(eng)
    pv, Z, _ = fetched(eng)
    if model_name == "edge":
        assert (pv[:, ~RING] == 0).any() and (pv[:6, ~RING] > 0).any(), "the edge model should lose some roots inside the ring at these periods"
        print("edge model, nz %d: %d of %d Rayleigh curves inside the ring have no root" % (nz, int((pv[:6, ~RING] == 0).sum()), 6 * 9))
    got, _ = against_host(h, eng, obs, a1, a2, wt, pv, Z, LOVE, depz)
    for name in FIGURES:
        assert not got[name][..., RING].any(), name
        assert not got[name][..., CENTRE].any() or name == "flag", name
        assert np.isfinite(got[name]).all(), name
    assert got["flag"][CENTRE] == 2
    used = (wt > 0) & (obs > 0) & (pv > 0) & ~LOVE[:, None]
    assert (got["nused"][~RING] == used.sum(axis=0)[~RING]).all() and got["nused"].max() <= 6
    assert not got["leverage"][~used].any()
    ok = (got["flag"] == 0) & ~RING
    assert ok.any() and (got["leverage"][:, ok][used[:, ok]] > 0).all() and (got["measures"][3][:, ok] > 0).all()
    assert (got["chi2"][2:, ok] <= got["chi2"][:2, ok]).all() and (got["chi2"][:2, ok] > 0).all()
    assert np.abs(got["gc"][:, ok]).max() > 1e-3 and np.abs(got["gs"][:, ok]).max() > 1e-3
    assert same_bits(eng.dispersion_get_model(), vel)
    nowt, _ = against_host(h, eng, obs, a1, a2, None, pv, Z, LOVE, depz)             # without weights: all 1, the Love slots still dropped
    assert not nowt["leverage"][LOVE].any() and nowt["flag"][CENTRE] == 0


def test_the_call_is_read_only(eng):
    """(b): after the call the model and everything dispersion_fetch returns have their bits; a columns_resolution and a columns_step after it
    give the bits of a fresh engine that never made the call; a second call without new runs repeats its bits"""
    nz = 8
    depz, vel, wt, obs, a1, a2 = case("smooth", nz)
    fresh = Engine(0)
    try:
        fresh.dispersion_begin(vel, depz, R.MINTHK, K, K)
        runs(fresh)
        plain_res = fresh.columns_resolution(obs, wt, R.SMOOTH, R.DAMP, full=True)
        plain = fresh.columns_step(obs, wt, *STEP)
        plain_model = fresh.dispersion_get_model()
    finally:
        fresh.close()
    eng.dispersion_begin(vel, depz, R.MINTHK, K, K)
    runs(eng)
    before = fetched(eng)[2]
    first = eng.columns_azimuthal(obs, a1, a2, wt, R.SMOOTH, R.DAMP)
    for a, b in zip(before, fetched(eng)[2]):
        assert same_bits(a, b)
    again = eng.columns_azimuthal(obs, a1, a2, wt, R.SMOOTH, R.DAMP)                 # (the marks stay: a second call needs no new runs)
    for name in first:
        assert same_bits(first[name], again[name]), name
    res = eng.columns_resolution(obs, wt, R.SMOOTH, R.DAMP, full=True)
    for name in plain_res:
        assert same_bits(res[name], plain_res[name]), name
    step = eng.columns_step(obs, wt, *STEP)
    for name in ("dv", "chi2", "nused", "flag"):
        assert same_bits(step[name], plain[name]), name
    assert same_bits(eng.dispersion_get_model(), plain_model) and np.abs(step["dv"]).max() > 0
    with pytest.raises(EngineError, match="has not been run") as exc:
        eng.columns_azimuthal(obs, a1, a2, wt, R.SMOOTH, R.DAMP)
    assert exc.value.code == DSA_ERR_STATE


def test_synthetic_recovery(eng, h):
    """(d): a layered truth at nz = 8 -- 2 % at N30E in the upper half, 1 % at N100E below -- A = fl32(Z g_true) through the device's own
    kernels, small smooth and damp.  In exact arithmetic the answer is R g_true; the device's g equals it, with the host's full R (S = Z, the
    effective weights), within the measured tolerance of the comparison plus the fp32 rounding of A carried through T: sum_k |T_kj| a_k
    2^-24 |A_k|.  The device's figures equal the twin's lstsq route within the same tolerance.  The axis error and the amplitude ratio per depth
    are printed, not asserted: how well depth separates is what R_jj says."""
    nz, smooth, damp = 8, 0.05, R.DAMP
    M = nz - 1
    depz, vel, wt, _, _, _ = case("smooth", nz)
    eng.dispersion_begin(vel, depz, R.MINTHK, K, K)
    runs(eng)
    pv, Z, _ = fetched(eng)
    assert (pv[:, ~RING] > 0).all()
    amp = np.where(np.arange(M) < (M + 1) // 2, 2.0, 1.0) / 50.0
    axis = np.radians(np.where(np.arange(M) < (M + 1) // 2, 30.0, 100.0))
    truth = np.stack([amp * np.cos(2 * axis), amp * np.sin(2 * axis)])               # (2, M): gc, gs
    A = np.einsum("lkc,ql->qkc", np.where(LOVE[None, :, None], 0.0, Z), truth)
    a1, a2 = A[0].astype(F), A[1].astype(F)
    obs = pv.astype(F)
    got, _ = against_host(h, eng, obs, a1, a2, wt, pv, Z, LOVE, depz, smooth, damp)
    weff = CA.effective_weights(wt, LOVE, (K, NCOL))
    res = CR.host_resolution(CR.load(), obs, weff, pv, np.where(LOVE[None, :, None], 0.0, Z), depz, smooth, damp, INNER)
    worst = worst_twin = 0.0
    for c in np.flatnonzero(~RING):
        if c == CENTRE:
            assert got["flag"][c] == 2 and not got["gc"][:, c].any()
            continue
        assert got["flag"][c] == 0 and res["flag"][c] == 0
        Rm, T = res["R"][:, :, c], res["T"][:, :, c]
        twin = depth.column_azimuthal_twin(obs[:, c], a1[:, c], a2[:, c], wt[:, c], pv[:, c], Z[:, :, c].T, LOVE, depz, smooth, damp)
        one = {name: got[name][..., c] for name in ("gc", "gs", "measures", "leverage", "chi2")}
        d = CA.differences(one, twin["other"], np.abs(Rm).max())
        worst_twin = max(worst_twin, max(d.values()))
        assert max(d.values()) <= CA.TOL, (c, d)
        for q, (name, a) in enumerate((("gc", a1), ("gs", a2))):
            pred = Rm @ truth[q]
            scale = max(np.abs(pred).max(), np.abs(Rm).max() * np.abs(truth[q]).max())
            carried = 2.0 ** -24 * (np.abs(T).T @ (weff[:, c].astype(np.float64) * np.abs(a[:, c]).astype(np.float64)))
            err = np.abs(got[name][:, c] - pred)
            worst = max(worst, float((err / scale).max()))
            assert (err <= CA.TOL * scale + carried).all(), (c, name, err, carried)
    ok = (got["flag"] == 0) & ~RING
    gc, gs = got["gc"][:, ok], got["gs"][:, ok]
    found = np.degrees(0.5 * np.arctan2(gs, gc))
    miss = (found - np.degrees(axis)[:, None] + 90.0) % 180.0 - 90.0
    ratio = np.hypot(gc, gs) / amp[:, None]
    print("largest |g - R g_true| / scale %.3g (the fp32 rounding of A is 6e-8 of it); device against the twin's lstsq route %.3g (TOL %.3g)" % (worst, worst_twin, CA.TOL))
    for l in range(M):
        print("depth %5.1f km: truth %.0f %% at N%.0fE; median axis error %+6.1f deg, median amplitude ratio %.3f, median R_jj %.3f" %
              (depz[l], 50.0 * amp[l], np.degrees(axis[l]), np.median(miss[l]), np.median(ratio[l]), np.median(got["measures"][0][l, ok])))


def test_the_limits_once(eng, h):
    """(e): nz = 64 (M = 63), K = 60 in test_gpu_column_resolution.py::test_the_limits_once's configuration: the one launch that asks for
    more than 64 KB of LDS (81 048 bytes).  Equal to the host bit for bit, and at least one interior column is solved."""
    nz, nmaps = 64, 60
    depz = R.depths(nz)
    vel = R.smooth_model(NX, NY, nz)
    love = np.arange(nmaps) >= 30
    eng.dispersion_begin(vel, depz, R.MINTHK, nmaps, nmaps)
    runs(eng, LIMIT_WAVES)
    pv, Z, _ = fetched(eng, nmaps)
    obs = np.where(pv > 0, pv, 3.0).astype(F)
    rng = np.random.default_rng(64)
    a1 = (0.03 * obs * rng.standard_normal(obs.shape)).astype(F)
    a2 = (0.03 * obs * rng.standard_normal(obs.shape)).astype(F)
    assert CA.load().hca_doubles(nz - 1, nmaps) * 8 == 81048 > 64 * 1024
    got, _ = against_host(h, eng, obs, a1, a2, None, pv, Z, love, depz)
    ok = (got["flag"] == 0) & ~RING
    print("nz 64, K 60: %d of 9 interior columns solved, Rayleigh roots %d of %d, largest |g| %.4g" %
          (int(ok.sum()), int((pv[:30, ~RING] > 0).sum()), 9 * 30, max(np.abs(got["gc"]).max(), np.abs(got["gs"]).max())))
    assert ok.any() and all(np.isfinite(got[name]).all() for name in FIGURES) and not got["leverage"][love].any()


def test_refusals(eng):
    """(f): every bad argument is DSA_ERR_ARGUMENT and every bad state DSA_ERR_STATE, found before the device is touched -- the runs stay
    fresh and the model unchanged, so the good call after each succeeds without new runs"""
    nz = 3
    depz, vel, wt, _, a1, a2 = case("smooth", nz)
    obs = np.full((K, NCOL), 3.0, F)
    codes = []

    def refused(match, o=obs, x1=a1, x2=a2, w=None, smooth=R.SMOOTH, damp=R.DAMP):
        with pytest.raises(EngineError, match=match) as exc:
            eng.columns_azimuthal(o, x1, x2, w, smooth, damp)
        codes.append(exc.value.code)

    def usable():
        assert (eng.columns_azimuthal(obs, a1, a2, wt, R.SMOOTH, R.DAMP)["flag"][~RING & (wt[:6] > 0).any(axis=0)] == 0).all()

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
    refused("damp", damp=np.nan)
    refused("smooth", smooth=-0.5)
    refused("smooth", smooth=np.inf)
    refused("maps given", o=obs[:K - 1], x1=a1[:K - 1], x2=a2[:K - 1])
    o = obs.copy(); o[0, 0] = np.nan
    refused("obs", o=o)
    for bad in (np.nan, np.inf):
        x = a1.copy(); x[7, 3] = bad                                                # (at a Love slot of a ring column: checked all the same)
        refused("a1", x1=x)
        refused("a2", x2=x)
    assert set(codes) == {DSA_ERR_ARGUMENT} and len(codes) == 13
    usable()
    with pytest.raises(ValueError, match="a1 holds"):
        eng.columns_azimuthal(obs, a1[:3], a2, None, R.SMOOTH, R.DAMP)
    # the required and the optional pointers, through the library itself: the binding always passes them all
    lib = eng._L
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    g = np.zeros((2, nz - 1, NCOL)); meas = np.zeros((4, nz - 1, NCOL)); lev = np.zeros((K, NCOL)); chi2 = np.zeros((4, NCOL))
    nu = np.zeros(NCOL, np.int32); fl = np.zeros(NCOL, np.int32)
    ins = [p(obs), p(a1), p(a2), None]
    outs = [p(g), p(meas), p(lev), p(chi2), p(nu), p(fl)]
    for missing in (0, 4, 5):
        args = list(outs); args[missing] = None
        assert lib.dsa_columns_azimuthal(eng._h, K, *ins, R.SMOOTH, R.DAMP, *args) == DSA_ERR_ARGUMENT
        assert b"required" in lib.dsa_error_string(eng._h)
    for missing in (0, 1, 2):
        args = list(ins); args[missing] = None
        assert lib.dsa_columns_azimuthal(eng._h, K, *args, R.SMOOTH, R.DAMP, *outs) == DSA_ERR_ARGUMENT
    assert lib.dsa_columns_azimuthal(eng._h, K, *ins, R.SMOOTH, R.DAMP, *outs) == 0 and g[:, :, ~RING].any()
    lean = np.zeros_like(g)
    assert lib.dsa_columns_azimuthal(eng._h, K, *ins, R.SMOOTH, R.DAMP, p(lean), None, None, None, p(nu), p(fl)) == 0 and same_bits(lean, g)
    usable()
    # states
    del codes[:]
    eng.dispersion_run(2, 0, R.WAVES[0][2], False, 0, 0)                           # the first maps again without kernels: no slot answers for them
    refused("slot 0 has not been run")
    runs(eng)
    eng.dispersion_run(2, 0, R.WAVES[0][2], True, 3, 0)                            # the first wave type's kernels into the second's slots
    refused("hold different curves")
    runs(eng)
    usable()
    eng.dispersion_begin(vel, depz, R.MINTHK, 6, 6)                                # a stage of Love slots only
    runs(eng, R.WAVES[2:])
    refused("Rayleigh", o=obs[:6], x1=a1[:6], x2=a2[:6])
    eng.dispersion_begin_models(np.stack([vel, vel]), depz, R.MINTHK, K)
    eng.dispersion_run(*R.WAVES[0], False, 0, 0)
    refused("2 models")
    eng.dispersion_begin_radial(vel, vel, depz, R.MINTHK, K, K)
    runs(eng)
    refused("is radial")
    eng.columns_sample_begin(vel, depz, R.MINTHK, list(R.WAVES), obs, wt, 2, 3.0, 0.05, 0.05, 0.4, 1.0, R.MINVEL, R.MAXVEL, 1, 0)
    refused("sample stage")
    eng.columns_sample_run(1)                                                      # the sample stage is usable after the refusal
    assert set(codes) == {DSA_ERR_STATE} and len(codes) == 6
    eng.dispersion_begin(vel, depz, R.MINTHK, K, K)
    runs(eng)
    usable()
    assert same_bits(eng.dispersion_get_model(), vel)
