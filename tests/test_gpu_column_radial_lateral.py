"""dsa_columns_step_radial_lateral (csrc/column_kernels.hip: k_radial_lateral_setup and k_radial_lateral_start, then the k_lateral_*
kernels every coupled system runs, k_lateral_residual and k_lateral_direction on RadialLateralWs) on the device against the CPU build of the same header (tests/hostcheck_column_radial_lateral.cpp through
column_radial_lateral_ref), bit for bit: the kernels share column_radial_lateral.h's loops out over a wavefront per column, every figure is
one sequential fp64 chain under -ffp-contract=off, the global sums have one shape (64 chains), and the scalars of the conjugate-gradient
loop are computed once, so neither the lane mapping nor the number of launches can show.

tests/test_gpu_columns.py's cases: grid 5 x 5 (9 interior columns), three periods of each of the four wave types (K = 12), nz = 2, 3, 8,
smooth_model and edge_model with Vsh 3 % above Vsv above the bottom depth, the centre column without weights; once 6 x 4 and once 11 x 10
(72 interior columns: more than one term in the chains of the global sums).  The inputs of the host step are the curves and kernels fetched
from the device after the runs, so the dispersion stage's own arithmetic is not under test here."""
import numpy as np
import pytest

import column_lateral_ref as IR
import column_radial_lateral_ref as LR
import column_radial_ref as RR
import columns_ref as R
from column_radial_lateral_ref import same_bits
from dsurftomo_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

F = np.float32
NX, NY, K = R.NX, R.NY, R.K
DSA_ERR_ARGUMENT, DSA_ERR_STATE, DSA_ERR_CAPACITY = -2, -5, -6                      # include/dsurftomo_amd.h
BASE = (R.SMOOTH, R.DAMP, RR.ANISO)
CLIP = (R.DVMAX, R.MINVEL, R.MAXVEL)
PAIRS = [(0.2, 0.0), (0.2, 0.5), (0.0, 2.0)]                                         # (lateral, lateral_aniso)


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


def above(vsv, factor=1.03):
    """Vsh = Vsv * factor above the bottom depth, equal at it"""
    vsh = np.array(vsv, F, copy=True)
    vsh[:-1] = (vsh[:-1] * F(factor)).astype(F)
    return vsh


def against_host(h, hs, e, vsv, vsh, depz, obs, wt, lateral, lateral_aniso, clip=CLIP, love=RR.LOVE, nmaps=K, tol=LR.TOL, maxit=LR.MAXIT):
    """the device's step and the host's on the values fetched before it: every output, info and both stepped models, bit for bit.  Returns
    (the device's result, the stepped (vsv, vsh))."""
    nz, ny, nx = vsv.shape
    ncol = nx * ny
    pv, svs, svp, srho = e.dispersion_fetch(0, nmaps, True, 0)
    Sv = R.host_combine(hs, vsv.reshape(nz, ncol), depz, svs, svp, srho)
    Sh = R.host_combine(hs, vsh.reshape(nz, ncol), depz, svs, svp, srho)
    want = LR.host_step(h, nx, ny, love, obs, wt, pv, Sv, Sh, vsv.reshape(nz, ncol), vsh.reshape(nz, ncol), *BASE, lateral, lateral_aniso, *clip, tol, maxit)
    got = e.columns_step_radial_lateral(obs, wt, *BASE, lateral, lateral_aniso, *clip, tol, maxit)
    after = e.dispersion_get_model_radial()
    print("%d x %d nz %d lateral %g aniso %g: itn %d istop %d rz0 %.6g rz %.3g (host: itn %d istop %d)" %
          (nx, ny, nz, lateral, lateral_aniso, got["itn"], got["istop"], got["rz0"], got["rz"], want["itn"], want["istop"]))
    assert (got["itn"], got["istop"]) == (want["itn"], want["istop"])
    assert same_bits(np.array([got["rz0"], got["rz"]]), np.array([want["rz0"], want["rz"]])), "rz0 / rz differ from the host's"
    for name in ("nused", "flag", "chi2", "dv_sv", "dv_sh"):
        assert same_bits(got[name], want[name]), "%s differs from the host's (%d of %d)" % (name, int((got[name] != want[name]).sum()), got[name].size)
    assert same_bits(after[0].reshape(nz, ncol), want["vsv"]), "the stepped Vsv differs from the host's"
    assert same_bits(after[1].reshape(nz, ncol), want["vsh"]), "the stepped Vsh differs from the host's"
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


@pytest.mark.parametrize("lateral,lateral_aniso", PAIRS)
@pytest.mark.parametrize("nz", [2, 3, 8])
@pytest.mark.parametrize("model_name", ["smooth", "edge"])
def test_step_equals_the_host_bit_for_bit(eng, h, hs, model_name, nz, lateral, lateral_aniso):
    """(7): with weights and without.  What stays: the ring and the bottom depth of both models; the centre column, which has no weights, is
    flag 0 with nused 0 0 and moves; nothing is NaN."""
    depz, vsv, rng, wt = case(model_name, nz)
    vsh = above(vsv)
    ncol = NX * NY
    ring = R.interior(NX, NY) == 0
    centre = 2 * NX + 2
    eng.dispersion_begin_radial(vsv, vsh, depz, R.MINTHK, K, K)
    runs(eng)
    obs, clip = observations(eng, model_name, rng, ncol)
    got, after = against_host(h, hs, eng, vsv, vsh, depz, obs, wt, lateral, lateral_aniso, clip)
    assert not got["nused"][:, ring].any() and not got["chi2"][:, ring].any() and not got["flag"][ring].any()
    assert got["flag"][centre] == 0 and not got["nused"][:, centre].any() and not got["chi2"][:, centre].any()
    moved = False
    for model, start, dv in ((after[0], vsv, got["dv_sv"]), (after[1], vsh, got["dv_sh"])):
        model = model.reshape(nz, ncol); before = start.reshape(nz, ncol)
        assert same_bits(model[:, ring], before[:, ring]) and same_bits(model[nz - 1], before[nz - 1]) and not dv[:, ring].any()
        assert np.isfinite(model).all() and np.isfinite(dv).all()
        assert (np.abs(dv) <= F(clip[0])).all() and (model[:nz - 1][:, ~ring] >= F(clip[1])).all() and (model[:nz - 1][:, ~ring] <= F(clip[2])).all()
        moved = moved or (np.abs(dv[:, centre]).max() > 0 and not same_bits(model[:, centre], before[:, centre]))
    assert moved
    assert np.isfinite(got["chi2"]).all() and np.isfinite([got["rz0"], got["rz"]]).all() and got["itn"] >= 1
    eng.dispersion_begin_radial(vsv, vsh, depz, R.MINTHK, K, K)
    runs(eng)
    against_host(h, hs, eng, vsv, vsh, depz, obs, None, lateral, lateral_aniso, clip)


@pytest.mark.parametrize("nx,ny", [(6, 4), (11, 10)])
def test_other_grids(eng, h, hs, nx, ny):
    """(8): 4 x 2 interior columns (no column has four neighbours; nvx and nvy differ) and 9 x 8 = 72 (the chains of the global sums hold
    more than one term), nz = 3"""
    nz = 3
    depz, vsv, rng, wt = case("smooth", nz, nx, ny)
    vsh = above(vsv)
    eng.dispersion_begin_radial(vsv, vsh, depz, R.MINTHK, K, K)
    runs(eng)
    obs, clip = observations(eng, "smooth", rng, nx * ny)
    got, _ = against_host(h, hs, eng, vsv, vsh, depz, obs, wt, 0.5, 0.5, clip)
    assert got["itn"] >= 2 and not got["flag"].any()


def test_no_coupling_is_columns_step_radial(eng):
    """(9): lateral = lateral_aniso = 0 on one stage against dsa_columns_step_radial on a second one: every output and both stepped models
    bit for bit, flag 2 of the centre column included; no iteration"""
    for model_name, nz in (("smooth", 8), ("edge", 3)):
        depz, vsv, rng, wt = case(model_name, nz)
        vsh = above(vsv)
        eng.dispersion_begin_radial(vsv, vsh, depz, R.MINTHK, K, K)
        runs(eng)
        obs, clip = observations(eng, model_name, rng, NX * NY)
        got = eng.columns_step_radial_lateral(obs, wt, *BASE, 0.0, 0.0, *clip)
        models = eng.dispersion_get_model_radial()
        eng.dispersion_begin_radial(vsv, vsh, depz, R.MINTHK, K, K)
        runs(eng)
        want = eng.columns_step_radial(obs, wt, *BASE, *clip)
        for name in ("nused", "flag", "chi2", "dv_sv", "dv_sh"):
            assert same_bits(got[name], want[name]), name
        for a, b in zip(models, eng.dispersion_get_model_radial()):
            assert same_bits(a, b)
        assert (got["itn"], got["istop"]) == (0, 1) and got["flag"][2 * NX + 2] == 2 and np.abs(got["dv_sv"]).max() > 0 and np.abs(got["dv_sh"]).max() > 0


def test_loop_with_a_column_without_data(eng, h, hs):
    """(10): tests/test_hostcheck_column_radial_lateral.py's loop on the device's own curves: the truth column_radial_ref.truth_vsh over
    smooth_model at nz = 8, the observations its curves with column_radial_lateral_ref's noise, the centre column without weights, both
    models started at perturbed(truth Vsv), four iterations with the coupled step (each equal to the host's from that iteration's fetched
    values) and with dsa_columns_step_radial.  The rms error of xi over the interior nodes above the bottom depth is lower with the
    coupling, and the centre column's xi ends closer to the truth than xi = 1 is."""
    nz = 8
    ncol = NX * NY
    centre = 2 * NX + 2
    depz = R.depths(nz)
    truth_v = R.smooth_model(NX, NY, nz)
    truth_h = RR.truth_vsh(truth_v)
    eng.dispersion_begin_radial(truth_v, truth_h, depz, R.MINTHK, K, K)
    runs(eng)
    obs = LR.noisy(eng.dispersion_fetch(0, K, False, 0))
    wt = np.ones((K, ncol), F); wt[:, centre] = 0.0
    start = R.perturbed(truth_v)
    eng.dispersion_begin_radial(start, start, depz, R.MINTHK, K, K)
    vsv, vsh = start, start
    itns = []
    for it in range(R.ITERATIONS):
        runs(eng)
        got, (vsv, vsh) = against_host(h, hs, eng, vsv, vsh, depz, obs, wt, LR.LATERAL, LR.LATERAL_ANISO)
        assert not got["flag"].any() and got["istop"] == 1
        itns.append(got["itn"])
    eng.dispersion_begin_radial(start, start, depz, R.MINTHK, K, K)
    for it in range(R.ITERATIONS):
        runs(eng)
        alone = eng.columns_step_radial(obs, wt, *BASE, *CLIP)
        assert alone["flag"][centre] == 2
    av, ah = eng.dispersion_get_model_radial()
    e = [LR.xi_rms(v, w, truth_v, truth_h, NX, NY) for v, w in ((start, start), (vsv, vsh), (av, ah))]
    c = [LR.xi_column_rms(v, w, truth_v, truth_h, centre) for v, w in ((None, None), (vsv, vsh), (av, ah))]
    print("rms error of xi: start %.5f, coupled %.5f, independent %.5f; centre column: xi = 1 %.5f, coupled %.5f, independent %.5f; itn %s" %
          (e[0], e[1], e[2], c[0], c[1], c[2], itns))
    assert e[1] < e[2]
    assert c[1] < c[0]


def test_the_limits_once(eng, h, hs):
    """(11): nz = 64 (M = 63), K = 60 -- test_gpu_column_resolution.py's period lists -- smooth_model on the 5 x 5 grid with Vsh 3 % above,
    maxit = 5: the one launch above 64 KB of LDS, equal to the host bit for bit"""
    nz, nmaps = 64, 60
    waves = [(2, 0, np.linspace(3.0, 45.0, 15)), (2, 1, np.linspace(4.0, 46.0, 15)), (1, 0, np.linspace(3.0, 45.0, 15)), (1, 1, np.linspace(4.0, 46.0, 15))]
    love = np.concatenate([np.full(len(t), wave == 1) for wave, _, t in waves])
    depz = R.depths(nz)
    vsv = R.smooth_model(NX, NY, nz)
    vsh = above(vsv)
    eng.dispersion_begin_radial(vsv, vsh, depz, R.MINTHK, nmaps, nmaps)
    runs(eng, waves)
    pv = eng.dispersion_fetch(0, nmaps, False, 0)
    obs = (np.where(pv > 0, pv, 3.0) * 1.01).astype(F)
    got, _ = against_host(h, hs, eng, vsv, vsh, depz, obs, None, 0.5, 0.5, love=love, nmaps=nmaps, maxit=5)
    assert got["itn"] == 5 and got["istop"] == 2 and np.abs(got["dv_sv"]).max() > 0 and np.isfinite(got["dv_sv"]).all() and np.isfinite(got["dv_sh"]).all()


def test_refusals(eng):
    """(12): a plain stage and a second step without new runs are DSA_ERR_STATE, a bad lateral, lateral_aniso, tol or maxit
    DSA_ERR_ARGUMENT -- found before the device is touched: the runs stay fresh and the models unchanged, so the good call at the end
    succeeds without new runs"""
    nz = 3
    depz, vsv, rng, wt = case("smooth", nz)
    vsh = above(vsv)
    obs = np.full((K, NX * NY), 3.0, F)
    good = dict(lateral=0.2, lateral_aniso=0.4, tol=1e-8, maxit=50)

    def refused(match, **kw):
        a = dict(good, **kw)
        with pytest.raises(EngineError, match=match) as exc:
            eng.columns_step_radial_lateral(obs, None, *BASE, a["lateral"], a["lateral_aniso"], *CLIP, a["tol"], a["maxit"])
        return exc.value.code

    eng.dispersion_begin(vsv, depz, R.MINTHK, K, K)
    runs(eng)
    assert refused("not radial") == DSA_ERR_STATE
    eng.dispersion_begin_radial(vsv, vsh, depz, R.MINTHK, K, K)
    runs(eng)
    for bad in (-0.1, np.nan, np.inf):
        assert refused("lateral .* must be finite", lateral=bad) == DSA_ERR_ARGUMENT
        assert refused("lateral_aniso .* must be finite", lateral_aniso=bad) == DSA_ERR_ARGUMENT
    for bad in (0.0, -1e-8, np.nan, np.inf):
        assert refused("tol", tol=bad) == DSA_ERR_ARGUMENT
    for bad in (0, -3):
        assert refused("maxit", maxit=bad) == DSA_ERR_ARGUMENT
    for a, b in zip(eng.dispersion_get_model_radial(), (vsv, vsh)):
        assert same_bits(a, b)
    ok = eng.columns_step_radial_lateral(obs, None, *BASE, good["lateral"], good["lateral_aniso"], *CLIP, good["tol"], good["maxit"])
    assert not ok["flag"].any() and ok["istop"] in (1, 2) and ok["carried"] == 0
    assert refused("has not been run") == DSA_ERR_STATE                          # a second step without new runs
    runs(eng)
    assert not eng.columns_step_radial_lateral(obs, None, *BASE, good["lateral"], good["lateral_aniso"], *CLIP)["flag"].any()


def test_workspace_beyond_the_memory_budget(eng, h):
    """(12): a memory budget below the loop's workspace is DSA_ERR_CAPACITY with both sizes in the message, found before the device is
    touched: the runs stay fresh and the models unchanged, and with the budget lifted the same call succeeds without new runs"""
    nz = 3
    depz, vsv, rng, wt = case("smooth", nz)
    vsh = above(vsv)
    obs = np.full((K, NX * NY), 3.0, F)
    need = h.hrlat_ws_doubles(NX, NY, nz - 1) * 8
    eng.dispersion_begin_radial(vsv, vsh, depz, R.MINTHK, K, K)
    runs(eng)
    try:
        eng.set_memory_budget(need - 1)
        with pytest.raises(EngineError, match="needs %d bytes, the memory budget is %d" % (need, need - 1)) as exc:
            eng.columns_step_radial_lateral(obs, None, *BASE, 0.2, 0.4, *CLIP)
        assert exc.value.code == DSA_ERR_CAPACITY
        for a, b in zip(eng.dispersion_get_model_radial(), (vsv, vsh)):
            assert same_bits(a, b)
        eng.set_memory_budget(need)                                              # the workspace alone is held against the budget
        assert not eng.columns_step_radial_lateral(obs, None, *BASE, 0.2, 0.4, *CLIP)["flag"].any()
    finally:
        eng.set_memory_budget(0)
    runs(eng)
    assert not eng.columns_step_radial_lateral(obs, None, *BASE, 0.2, 0.4, *CLIP)["flag"].any()


def test_both_coupled_steps_share_one_engine(eng, h, hs):
    """(13): dsa_columns_step_lateral on a 6 x 4 grid (nz = 3, lateral 0.3), then dsa_columns_step_radial_lateral on 11 x 10 (nz = 8, at
    0.3, 0.6), then the first call again on a fresh dispersion_begin with the same inputs, all on one engine, whose two steps share their
    workspace: each result equals its host harness bit for bit, and the third equals the first bit for bit -- what a call that read what
    an earlier one left in the workspace would break."""
    hi = IR.load()

    def lateral_call():
        nz, nx, ny = 3, 6, 4
        depz, vel, rng, wt = case("smooth", nz, nx, ny)
        eng.dispersion_begin(vel, depz, R.MINTHK, K, K)
        runs(eng)
        pv, svs, svp, srho = eng.dispersion_fetch(0, K, True, 0)
        obs = (pv * (1.0 + 0.02 * rng.standard_normal((K, nx * ny)))).astype(F)
        S = R.host_combine(hs, vel.reshape(nz, nx * ny), depz, svs, svp, srho)
        want = IR.host_step(hi, nx, ny, obs, wt, pv, S, vel.reshape(nz, nx * ny), R.SMOOTH, R.DAMP, 0.3, *CLIP)
        got = eng.columns_step_lateral(obs, wt, R.SMOOTH, R.DAMP, 0.3, *CLIP, IR.TOL, IR.MAXIT)
        got["vels"] = eng.dispersion_get_model().reshape(nz, nx * ny)
        assert (got["itn"], got["istop"]) == (want["itn"], want["istop"]) and got["itn"] >= 1
        assert same_bits(np.array([got["rz0"], got["rz"]]), np.array([want["rz0"], want["rz"]]))
        for name in ("nused", "flag", "chi2", "dv", "vels"):
            assert same_bits(got[name], want[name]), "%s differs from the host's" % name
        return got

    first = lateral_call()
    nz, nx, ny = 8, 11, 10
    depz, vsv, rng, wt = case("smooth", nz, nx, ny)
    vsh = above(vsv)
    eng.dispersion_begin_radial(vsv, vsh, depz, R.MINTHK, K, K)
    runs(eng)
    obs, clip = observations(eng, "smooth", rng, nx * ny)
    got, _ = against_host(h, hs, eng, vsv, vsh, depz, obs, wt, 0.3, 0.6, clip)
    assert got["itn"] >= 2
    again = lateral_call()
    assert (first["itn"], first["istop"], first["carried"]) == (again["itn"], again["istop"], again["carried"])
    for name in ("nused", "flag", "chi2", "dv", "vels", "rz0", "rz"):
        assert same_bits(np.asarray(first[name]), np.asarray(again[name])), "%s of the repeated call differs from the first" % name
