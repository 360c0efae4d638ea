"""dsa_columns_step_lateral (csrc/column_kernels.hip: k_lateral_*) on the device against the CPU build of the same
header (tests/hostcheck_column_lateral.cpp through column_lateral_ref), bit for bit: the kernels share column_lateral.h's loops out over a
wavefront per column, every figure is one sequential fp64 chain under -ffp-contract=off, the global sums have one shape (64 chains), and the
scalars of the conjugate-gradient loop are computed once, so neither the lane mapping nor the number of launches can show.

tests/test_gpu_columns.py's cases: grid 5 x 5 (9 interior columns), three periods of each of the four wave types (K = 12), nz = 2, 3, 8,
smooth_model and edge_model, the centre column without weights; once 6 x 4 and once 11 x 10 (72 interior columns: more than one term in the
chains of the global sums).  The inputs of the host step are the curves and kernels fetched from the device after the runs, so the
dispersion stage's own arithmetic is not under test here."""
import numpy as np
import pytest

import column_lateral_ref as LR
import columns_ref as R
from column_lateral_ref import same_bits
from dsurftomo_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

F = np.float32
NX, NY, K = R.NX, R.NY, R.K
DSA_ERR_ARGUMENT, DSA_ERR_STATE, DSA_ERR_CAPACITY = -2, -5, -6                      # include/dsurftomo_amd.h
BASE = (R.SMOOTH, R.DAMP)
CLIP = (R.DVMAX, R.MINVEL, R.MAXVEL)


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def h():
    return LR.load()


@pytest.fixture(scope="module")
def hs():
    return R.load()


def runs(e, waves=R.WAVES):
    first = 0
    for wave, kind, t in waves:
        e.dispersion_run(wave, kind, t, True, first, first)
        first += len(t)


def against_host(h, hs, e, model, depz, obs, wt, lateral, clip=CLIP, nmaps=K, tol=LR.TOL, maxit=LR.MAXIT):
    """the device's step and the host's on the values fetched before it: every output, info and the stepped model, bit for bit.  Returns
    (the device's result, the stepped model)."""
    nz, ny, nx = model.shape
    ncol = nx * ny
    pv, svs, svp, srho = e.dispersion_fetch(0, nmaps, True, 0)
    S = R.host_combine(hs, model.reshape(nz, ncol), depz, svs, svp, srho)
    want = LR.host_step(h, nx, ny, obs, wt, pv, S, model.reshape(nz, ncol), *BASE, lateral, *clip, tol, maxit)
    got = e.columns_step_lateral(obs, wt, *BASE, lateral, *clip, tol, maxit)
    after = e.dispersion_get_model()
    print("%d x %d nz %d lateral %g: itn %d istop %d rz0 %.6g rz %.3g (host: itn %d istop %d)" % (nx, ny, nz, lateral, got["itn"], got["istop"], got["rz0"], got["rz"],
                                                                                             want["itn"], want["istop"]))
    assert (got["itn"], got["istop"]) == (want["itn"], want["istop"])
    assert same_bits(np.array([got["rz0"], got["rz"]]), np.array([want["rz0"], want["rz"]])), "rz0 / rz differ from the host's"
    for name in ("nused", "flag", "chi2", "dv"):
        assert same_bits(got[name], want[name]), "%s differs from the host's (%d of %d)" % (name, int((got[name] != want[name]).sum()), got[name].size)
    assert same_bits(after.reshape(nz, ncol), want["vels"]), "the stepped model differs from the host's"
    return got, after


def case(model_name, nz, nx=NX, ny=NY):
    """test_gpu_columns.py's: weights around 1, a tenth of them 0, the centre column without any"""
    depz = R.depths(nz)
    vel = (R.smooth_model if model_name == "smooth" else R.edge_model)(nx, ny, nz)
    rng = np.random.default_rng(7 + nz)
    wt = (0.5 + rng.random((K, nx * ny))).astype(F)
    wt[rng.random((K, nx * ny)) < 0.1] = 0.0
    wt[:, (ny // 2) * nx + nx // 2] = 0.0
    return depz, vel, rng, wt


def observations(e, model_name, rng, ncol):
    pv0 = e.dispersion_fetch(0, K, False, 0)
    if model_name == "smooth":
        return (pv0 * (1.0 + 0.02 * rng.standard_normal((K, ncol)))).astype(F), CLIP
    return (2.5 + 1.5 * rng.random((K, ncol))).astype(F), (0.1, 2.0, 4.5)


@pytest.mark.parametrize("lateral", [0.2, 2.0])
@pytest.mark.parametrize("nz", [2, 3, 8])
@pytest.mark.parametrize("model_name", ["smooth", "edge"])
def test_step_equals_the_host_bit_for_bit(eng, h, hs, model_name, nz, lateral):
    """(a) and (d): with weights and without.  What stays: the ring and the bottom depth; the centre column, which has no weights, is flag 0
    with nused 0 and moves; nothing is NaN."""
    depz, vel, rng, wt = case(model_name, nz)
    ncol = NX * NY
    ring = R.interior(NX, NY) == 0
    centre = 2 * NX + 2
    eng.dispersion_begin(vel, depz, R.MINTHK, K, K)
    runs(eng)
    obs, clip = observations(eng, model_name, rng, ncol)
    got, after = against_host(h, hs, eng, vel, depz, obs, wt, lateral, clip)
    model = after.reshape(nz, ncol); before = vel.reshape(nz, ncol)
    assert same_bits(model[:, ring], before[:, ring]) and same_bits(model[nz - 1], before[nz - 1])
    assert not got["dv"][:, ring].any() and not got["nused"][ring].any() and not got["chi2"][ring].any() and not got["flag"][ring].any()
    assert got["flag"][centre] == 0 and got["nused"][centre] == 0 and got["chi2"][centre] == 0.0
    assert np.abs(got["dv"][:, centre]).max() > 0 and not same_bits(model[:, centre], before[:, centre])
    assert np.isfinite(model).all() and np.isfinite(got["dv"]).all() and np.isfinite(got["chi2"]).all() and np.isfinite([got["rz0"], got["rz"]]).all()
    assert got["istop"] == 1 and got["itn"] >= 1
    assert (np.abs(got["dv"]) <= F(clip[0])).all() and (model[:nz - 1][:, ~ring] >= F(clip[1])).all() and (model[:nz - 1][:, ~ring] <= F(clip[2])).all()
    eng.dispersion_begin(vel, depz, R.MINTHK, K, K)
    runs(eng)
    against_host(h, hs, eng, vel, depz, obs, None, lateral, clip)


@pytest.mark.parametrize("nx,ny", [(6, 4), (11, 10)])
def test_other_grids(eng, h, hs, nx, ny):
    """(b): 4 x 2 interior columns (no column has four neighbours; nvx and nvy differ) and 9 x 8 = 72 (the chains of the global sums hold
    more than one term), nz = 3"""
    nz = 3
    depz, vel, rng, wt = case("smooth", nz, nx, ny)
    eng.dispersion_begin(vel, depz, R.MINTHK, K, K)
    runs(eng)
    obs, clip = observations(eng, "smooth", rng, nx * ny)
    got, _ = against_host(h, hs, eng, vel, depz, obs, wt, 0.5, clip)
    assert got["istop"] == 1 and got["itn"] >= 2 and not got["flag"].any()


def test_lateral_zero_is_columns_step(eng):
    """(c): lateral = 0 on one stage against dsa_columns_step on a second one: every output and the stepped model bit for bit, flag 2 of the
    centre column included; no iteration"""
    for model_name, nz in (("smooth", 8), ("edge", 3)):
        depz, vel, rng, wt = case(model_name, nz)
        eng.dispersion_begin(vel, depz, R.MINTHK, K, K)
        runs(eng)
        obs, clip = observations(eng, model_name, rng, NX * NY)
        got = eng.columns_step_lateral(obs, wt, *BASE, 0.0, *clip)
        model = eng.dispersion_get_model()
        eng.dispersion_begin(vel, depz, R.MINTHK, K, K)
        runs(eng)
        want = eng.columns_step(obs, wt, *BASE, *clip)
        for name in ("nused", "flag", "chi2", "dv"):
            assert same_bits(got[name], want[name]), name
        assert same_bits(model, eng.dispersion_get_model())
        assert (got["itn"], got["istop"]) == (0, 1) and got["flag"][2 * NX + 2] == 2 and np.abs(got["dv"]).max() > 0


def test_loop_with_a_column_without_data(eng, h, hs):
    """(e): tests/test_hostcheck_column_lateral.py's loop on the device's own curves: the truth smooth_model at nz = 8, the observations its
    curves with column_lateral_ref's noise, the centre column without weights, the start perturbed(truth), four iterations with the lateral
    step (each equal to the host's from that iteration's fetched values) and with dsa_columns_step.  The rms model error over the interior
    nodes above the bottom depth is lower with the coupling, and the centre column ends closer to the truth than it started, where the
    independent loop leaves it."""
    nz = 8
    ncol = NX * NY
    centre = 2 * NX + 2
    depz = R.depths(nz)
    truth = R.smooth_model(NX, NY, nz)
    eng.dispersion_begin(truth, depz, R.MINTHK, K, K)
    runs(eng)
    obs = LR.noisy(eng.dispersion_fetch(0, K, False, 0))
    wt = np.ones((K, ncol), F); wt[:, centre] = 0.0
    start = R.perturbed(truth)
    eng.dispersion_begin(start, depz, R.MINTHK, K, K)
    model = start
    itns = []
    for it in range(R.ITERATIONS):
        runs(eng)
        got, model = against_host(h, hs, eng, model, depz, obs, wt, LR.LATERAL)
        assert not got["flag"].any()
        itns.append(got["itn"])
    eng.dispersion_begin(start, depz, R.MINTHK, K, K)
    for it in range(R.ITERATIONS):
        runs(eng)
        alone = eng.columns_step(obs, wt, *BASE, *CLIP)
        assert alone["flag"][centre] == 2
    independent = eng.dispersion_get_model()
    col_err = lambda m: float(np.sqrt(((m.reshape(nz, ncol)[:nz - 1, centre].astype(np.float64) - truth.reshape(nz, ncol)[:nz - 1, centre]) ** 2).mean()))
    e_lat, e_ind, e_start = LR.model_rms(model, truth, NX, NY), LR.model_rms(independent, truth, NX, NY), LR.model_rms(start, truth, NX, NY)
    print("rms model error: start %.5f, lateral %.5f, independent %.5f km/s; centre column: start %.5f, lateral %.5f, independent %.5f km/s; itn %s" %
          (e_start, e_lat, e_ind, col_err(start), col_err(model), col_err(independent), itns))
    assert e_lat < e_ind
    assert col_err(model) < col_err(start) and col_err(independent) == col_err(start)


def test_the_limits_once(eng, h, hs):
    """(f): nz = 64 (M = 63), K = 60 -- test_gpu_column_resolution.py's period lists -- smooth_model on the 5 x 5 grid, maxit = 5: equal to
    the host bit for bit"""
    nz, nmaps = 64, 60
    waves = [(2, 0, np.linspace(3.0, 45.0, 15)), (2, 1, np.linspace(4.0, 46.0, 15)), (1, 0, np.linspace(3.0, 45.0, 15)), (1, 1, np.linspace(4.0, 46.0, 15))]
    depz = R.depths(nz)
    vel = R.smooth_model(NX, NY, nz)
    eng.dispersion_begin(vel, depz, R.MINTHK, nmaps, nmaps)
    runs(eng, waves)
    pv = eng.dispersion_fetch(0, nmaps, False, 0)
    obs = (np.where(pv > 0, pv, 3.0) * 1.01).astype(F)
    got, _ = against_host(h, hs, eng, vel, depz, obs, None, 0.5, nmaps=nmaps, maxit=5)
    assert got["itn"] == 5 and got["istop"] == 2 and np.abs(got["dv"]).max() > 0 and np.isfinite(got["dv"]).all()


def test_refusals(eng):
    """(g): a radial stage and a second step without new runs are DSA_ERR_STATE, a bad lateral, tol or maxit DSA_ERR_ARGUMENT -- found
    before the device is touched: the runs stay fresh and the model unchanged, so the good call at the end succeeds without new runs"""
    nz = 3
    depz, vel, rng, wt = case("smooth", nz)
    obs = np.full((K, NX * NY), 3.0, F)
    good = dict(lateral=0.2, tol=1e-8, maxit=50)

    def refused(match, **kw):
        a = dict(good, **kw)
        with pytest.raises(EngineError, match=match) as exc:
            eng.columns_step_lateral(obs, None, *BASE, a["lateral"], *CLIP, a["tol"], a["maxit"])
        return exc.value.code

    eng.dispersion_begin_radial(vel, vel, depz, R.MINTHK, K, K)
    runs(eng)
    assert refused("radial") == DSA_ERR_STATE
    eng.dispersion_begin(vel, depz, R.MINTHK, K, K)
    runs(eng)
    for bad in (-0.1, np.nan, np.inf):
        assert refused("lateral", lateral=bad) == DSA_ERR_ARGUMENT
    for bad in (0.0, -1e-8, np.nan, np.inf):
        assert refused("tol", tol=bad) == DSA_ERR_ARGUMENT
    for bad in (0, -3):
        assert refused("maxit", maxit=bad) == DSA_ERR_ARGUMENT
    assert same_bits(eng.dispersion_get_model(), vel)
    ok = eng.columns_step_lateral(obs, None, *BASE, good["lateral"], *CLIP, good["tol"], good["maxit"])
    assert not ok["flag"].any() and ok["istop"] == 1
    assert refused("has not been run") == DSA_ERR_STATE                          # a second step without new runs
    runs(eng)
    assert eng.columns_step_lateral(obs, None, *BASE, good["lateral"], *CLIP)["istop"] == 1


def test_workspace_beyond_the_memory_budget(eng, h):
    """a memory budget below the loop's workspace is DSA_ERR_CAPACITY with both sizes in the message, found before the device is touched:
    the runs stay fresh and the model unchanged, and with the budget lifted the same call succeeds without new runs"""
    nz = 3
    depz, vel, rng, wt = case("smooth", nz)
    obs = np.full((K, NX * NY), 3.0, F)
    need = h.hlat_ws_doubles(NX, NY, nz - 1) * 8
    eng.dispersion_begin(vel, depz, R.MINTHK, K, K)
    runs(eng)
    try:
        eng.set_memory_budget(need - 1)
        with pytest.raises(EngineError, match="needs %d bytes, the memory budget is %d" % (need, need - 1)) as exc:
            eng.columns_step_lateral(obs, None, *BASE, 0.2, *CLIP)
        assert exc.value.code == DSA_ERR_CAPACITY
        assert same_bits(eng.dispersion_get_model(), vel)
        eng.set_memory_budget(need)                                              # the workspace alone is held against the budget
        assert eng.columns_step_lateral(obs, None, *BASE, 0.2, *CLIP)["istop"] == 1
    finally:
        eng.set_memory_budget(0)
    runs(eng)
    assert eng.columns_step_lateral(obs, None, *BASE, 0.2, *CLIP)["istop"] == 1
