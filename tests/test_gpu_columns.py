"""dsa_columns_step (csrc/column_kernels.hip: k_column_step) on the device against the CPU build of the same header
(tests/hostcheck_columns.cpp through columns_ref), bit for bit: the kernel shares column_system.h's loops out over a wavefront, every figure
is one sequential fp64 chain under -ffp-contract=off, there is no square root and the division is IEEE, so the lane mapping cannot show.

Grid 5 x 5 (9 interior columns), three periods of each of the four wave types (K = 12), nz = 2, 3, 8 (M = 1: no regulariser row; M = 2: the
two closing rows only; M = 7), test_gpu_dispersion.py's smooth_model and edge_model -- the latter has columns without a Love root at these
periods, whose data must be dropped and whose kernels must not be read.  The inputs of the host step are the curves and kernels fetched
from the device after the runs, so the dispersion stage's own arithmetic is not under test here."""
import numpy as np
import pytest

import columns_ref as R
from dsurftomo_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

F = np.float32
NX, NY, K = R.NX, R.NY, R.K
NCOL = NX * NY
RING = R.interior(NX, NY) == 0
DSA_ERR_ARGUMENT, DSA_ERR_STATE = -2, -5                      # include/dsurftomo_amd.h
ARGS = (R.SMOOTH, R.DAMP, R.DVMAX, R.MINVEL, R.MAXVEL)


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def h():
    return R.load()


def runs(e, skip=None):
    first = 0
    for n, (wave, kind, t) in enumerate(R.WAVES):
        if n != skip:
            e.dispersion_run(wave, kind, t, True, first, first)
        first += len(t)


def begin(e, vel, depz):
    e.dispersion_begin(vel, depz, R.MINTHK, K, K)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def against_host(h, e, model, depz, obs, wt, args=ARGS):
    """the device's step and the host's on the values fetched before it: every output and the stepped model, bit for bit.  Returns (the
    device's result, the stepped model, the fetched pv)."""
    nz = model.shape[0]
    pv, svs, svp, srho = e.dispersion_fetch(0, K, True, 0)
    S = R.host_combine(h, model.reshape(nz, NCOL), depz, svs, svp, srho)
    want = R.host_step(h, obs, wt, pv, S, model.reshape(nz, NCOL), *args, R.interior(NX, NY))
    got = e.columns_step(obs, wt, *args)
    after = e.dispersion_get_model()
    for name in ("nused", "flag", "chi2", "dv"):
        assert same_bits(got[name], want[name]), "%s differs from the host's (%d of %d)" % (name, int((got[name] != want[name]).sum()), got[name].size)
    assert same_bits(after.reshape(nz, NCOL), want["vels"]), "the stepped model differs from the host's"
    return got, after, pv


def case(model_name, nz):
    depz = R.depths(nz)
    vel = (R.smooth_model if model_name == "smooth" else R.edge_model)(NX, NY, nz)
    rng = np.random.default_rng(7 + nz)
    wt = (0.5 + rng.random((K, NCOL))).astype(F)
    wt[rng.random((K, NCOL)) < 0.1] = 0.0
    wt[:, 2 * NX + 2] = 0.0                                                      # the centre column: no datum
    return depz, vel, rng, wt


@pytest.mark.parametrize("nz", [2, 3, 8])
@pytest.mark.parametrize("model_name", ["smooth", "edge"])
def test_step_equals_the_host_bit_for_bit(eng, h, model_name, nz):
    """(a) and (b): smooth_model with observations 2 % off its own curves (small steps), edge_model with observations far from its curves
    (steps clipped at dvmax, values at the bounds) and curves without a root.  What stays: the ring, the bottom depth, a column whose
    weights are all 0; nothing is NaN."""
    depz, vel, rng, wt = case(model_name, nz)
    begin(eng, vel, depz)
    runs(eng)
    pv0 = eng.dispersion_fetch(0, K, False, 0)
    if model_name == "smooth":
        obs = (pv0 * (1.0 + 0.02 * rng.standard_normal((K, NCOL)))).astype(F)
        args = ARGS
    else:
        obs = (2.5 + 1.5 * rng.random((K, NCOL))).astype(F)
        args = (R.SMOOTH, R.DAMP, 0.1, 2.0, 4.5)
        inner_pv = pv0[:, ~RING]
        assert (inner_pv == 0).any() and (inner_pv > 0).any(), "the edge model should lose some roots inside the ring at these periods"
    got, after, pv = against_host(h, eng, vel, depz, obs, wt, args)
    assert same_bits(pv, pv0)
    model = after.reshape(nz, NCOL); before = vel.reshape(nz, NCOL)
    assert same_bits(model[:, RING], before[:, RING]) and same_bits(model[nz - 1], before[nz - 1])
    assert not got["dv"][:, RING].any() and not got["nused"][RING].any() and not got["chi2"][RING].any() and not got["flag"][RING].any()
    centre = 2 * NX + 2
    assert got["flag"][centre] == 2 and got["nused"][centre] == 0 and not got["dv"][:, centre].any() and same_bits(model[:, centre], before[:, centre])
    assert np.isfinite(model).all() and np.isfinite(got["dv"]).all() and np.isfinite(got["chi2"]).all()
    used = ((wt > 0) & (obs > 0) & (pv > 0)).sum(axis=0)
    assert (got["nused"][~RING] == used[~RING]).all()                          # a datum without a root is dropped, not propagated
    stepped = (got["flag"] == 0) & ~RING
    assert stepped.any() and np.abs(got["dv"][:, stepped]).max() > 0
    assert (np.abs(got["dv"]) <= F(args[2])).all() and (model[:nz - 1][:, stepped] >= F(args[3])).all() and (model[:nz - 1][:, stepped] <= F(args[4])).all()
    if model_name == "edge":
        assert (np.abs(got["dv"]) == F(args[2])).any()                           # clipped at exactly dvmax somewhere
    # without weights: all 1
    begin(eng, vel, depz)
    runs(eng)
    against_host(h, eng, vel, depz, obs, None, args)


@pytest.mark.parametrize("nz", [2, 3, 8])
def test_loop_reduces_the_misfit(eng, h, nz):
    """(c): the observations are the device's own curves of a smooth truth in fp32, the start is the truth with a smooth 3 % perturbation;
    four iterations, each step equal to the host's from that iteration's fetched values; the sum of chi2 before the last step is below the
    one before the first (the same loop on the oracle's curves: test_depth_patterns.py).  The rms values are printed, not asserted."""
    depz = R.depths(nz)
    truth = R.smooth_model(NX, NY, nz)
    begin(eng, truth, depz)
    runs(eng)
    obs = eng.dispersion_fetch(0, K, False, 0).astype(F)
    assert (obs[:, ~RING] > 0).all()
    start = R.perturbed(truth)
    begin(eng, start, depz)
    model = start
    chi2, rms = [], []
    for it in range(R.ITERATIONS):
        runs(eng)
        got, model, _ = against_host(h, eng, model, depz, obs, None)
        assert not got["flag"].any()
        chi2.append(float(got["chi2"].sum()))
        rms.append(float(np.sqrt(got["chi2"].sum() / got["nused"].sum())))
    print("nz %d: rms before each step %s km/s" % (nz, " ".join("%.6f" % r for r in rms)))
    assert chi2[-1] < chi2[0]


def test_state_is_checked(eng):
    """(d): a step without runs, a second step without new runs, a step with one slot not rerun, a step on two models: DSA_ERR_STATE;
    the engine stays usable after each"""
    nz = 3
    depz, vel, rng, wt = case("smooth", nz)
    obs = np.full((K, NCOL), 3.0, F)

    def refused(match):
        with pytest.raises(EngineError, match=match) as exc:
            eng.columns_step(obs, None, *ARGS)
        return exc.value.code

    begin(eng, vel, depz)
    state = DSA_ERR_STATE
    assert refused("has not been run") == state                                  # no runs since begin
    runs(eng)
    ok = eng.columns_step(obs, None, *ARGS)
    assert (ok["flag"][~RING] == 0).all()
    assert refused("has not been run") == state                                  # a second step without new runs
    runs(eng, skip=2)
    assert refused("slot 6 has not been run") == state                           # the third wave type (slots 6 .. 8) not rerun
    runs(eng)
    eng.dispersion_run(1, 0, R.WAVES[2][2], False, 0, 6)                         # the Love maps again without kernels: no slot answers for them
    assert refused("slot 6 has not been run") == state
    runs(eng)
    eng.dispersion_run(2, 0, R.WAVES[0][2], True, 3, 0)                          # the first wave type's kernels into the second's slots
    assert refused("hold different curves") == state
    runs(eng)
    assert (eng.columns_step(obs, None, *ARGS)["flag"][~RING] == 0).all()      # usable after the refusals
    eng.dispersion_begin_models(np.stack([vel, vel]), depz, R.MINTHK, K)
    for wave, kind, t in R.WAVES[:1]:
        eng.dispersion_run(wave, kind, t, False, 0, 0)
    assert refused("2 models") == state
    with pytest.raises(EngineError, match="2 models"):
        eng.dispersion_get_model()
    begin(eng, vel, depz)
    runs(eng)
    assert (eng.columns_step(obs, None, *ARGS)["flag"][~RING] == 0).all()


def test_arguments_are_checked(eng):
    """(d): every bad argument is DSA_ERR_ARGUMENT, found before the device is touched -- the runs stay fresh and the model unchanged, so
    the good call at the end succeeds without new runs"""
    nz = 3
    depz, vel, rng, wt = case("smooth", nz)
    obs = np.full((K, NCOL), 3.0, F)
    begin(eng, vel, depz)
    runs(eng)
    codes = set()

    def refused(match, o=obs, w=None, args=ARGS):
        with pytest.raises(EngineError, match=match) as exc:
            eng.columns_step(o, w, *args)
        codes.add(exc.value.code)

    smooth, damp, dvmax, lo, hi = ARGS
    for bad in (-1.0, np.nan, np.inf):
        w = wt.copy(); w[5, 7] = bad
        refused("wt", w=w)
    refused("damp", args=(smooth, 0.0, dvmax, lo, hi))
    refused("damp", args=(smooth, -0.1, dvmax, lo, hi))
    refused("damp", args=(smooth, np.nan, dvmax, lo, hi))
    refused("smooth", args=(-0.5, damp, dvmax, lo, hi))
    refused("dvmax", args=(smooth, damp, 0.0, lo, hi))
    refused("dvmax", args=(smooth, damp, -1.0, lo, hi))
    refused("minvel", args=(smooth, damp, dvmax, 4.0, 3.0))
    refused("maps given", o=obs[:K - 1])
    o = obs.copy(); o[0, 0] = np.nan
    refused("obs", o=o)
    assert codes == {DSA_ERR_ARGUMENT}
    assert same_bits(eng.dispersion_get_model(), vel)
    assert (eng.columns_step(obs, wt, *ARGS)["flag"][~RING & (wt > 0).any(axis=0)] == 0).all()
