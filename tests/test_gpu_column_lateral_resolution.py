"""dsa_columns_resolution_lateral (csrc/column_kernels.hip: k_latres_*) on the device against the CPU build of the same
header (tests/hostcheck_column_lateral_resolution.cpp through column_lateral_resolution_ref), bit for bit: a member's arithmetic is one
sequential fp64 chain under -ffp-contract=off whichever lane runs it, the global sums have section 24's shape, and a member's scalars are
its own, so neither the lane mapping, the chunking nor the number of launches can show.

tests/test_gpu_columns.py's cases: grid 5 x 5 (9 interior columns), three periods of each of the four wave types (K = 12), nz = 2, 3, 8,
smooth_model and edge_model, the centre column without weights; once 11 x 10 (72 interior columns: two terms in eight chains of the global
sums) and once the limits.  The inputs of the host run are the curves and kernels fetched from the device after the dispersion runs, so the
dispersion stage's own arithmetic is not under test here."""
import numpy as np
import pytest

import column_lateral_resolution_ref as RR
import columns_ref as R
from column_lateral_resolution_ref import same_bits
from dsurftomo_amd.engine import Engine, EngineError
from test_gpu_column_lateral import BASE, CLIP, K, NX, NY, case, observations, runs

pytestmark = pytest.mark.gpu

F = np.float32
DSA_ERR_ARGUMENT, DSA_ERR_STATE, DSA_ERR_CAPACITY = -2, -5, -6                      # include/dsurftomo_amd.h
TOL, MAXIT = 1e-8, 500
NAMES = ("measures", "full", "itn", "istop", "rz0", "rz", "nused", "flag")


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def h():
    return RR.load()


@pytest.fixture(scope="module")
def hs():
    return R.load()


def members(nint, M, every=1, rows=2):
    """every `every`-th unknown as kinds 0 and 1, then one member of kind 2 and one of kind 3; the models: rows of standard normals"""
    kind, index = RR.every_unknown(nint, M)
    keep = (index % every) == 0
    models = np.random.default_rng(7).standard_normal((rows, M, nint))
    return np.r_[kind[keep], 2, 3].astype(np.int32), np.r_[index[keep], 0, rows - 1].astype(np.int32), models


def host_inputs(hs, e, model, depz, nmaps=K):
    nz, ny, nx = model.shape
    pv, svs, svp, srho = e.dispersion_fetch(0, nmaps, True, 0)
    return pv, R.host_combine(hs, model.reshape(nz, nx * ny), depz, svs, svp, srho)


def against_host(h, hs, e, model, depz, obs, wt, lateral, kind, index, models, nmaps=K, tol=TOL, maxit=MAXIT, full=True):
    """the device's members and the host's on the values fetched from the device: measures, info, full, nused and flag, bit for bit"""
    nz, ny, nx = model.shape
    pv, S = host_inputs(hs, e, model, depz, nmaps)
    want = RR.host_run(h, nx, ny, obs, wt, pv, S, depz, *BASE, lateral, kind, index, models, tol, maxit)
    got = e.columns_resolution_lateral(obs, wt, *BASE, lateral, kind, index, models, tol, maxit, full=full)
    print("%d x %d nz %d lateral %g: %d members, itn %d .. %d (host %d .. %d), istop %s" % (nx, ny, nz, lateral, len(kind), got["itn"].min(), got["itn"].max(),
                                                                                         want["itn"].min(), want["itn"].max(), sorted(set(got["istop"].tolist()))))
    for name in NAMES:
        if name == "full" and not full:
            assert "full" not in got
            continue
        assert same_bits(got[name], want[name]), "%s differs from the host's (%d of %d)" % (name, int((got[name] != want[name]).sum()), got[name].size)
    return got


@pytest.mark.parametrize("lateral", [0.2, 2.0])
@pytest.mark.parametrize("nz", [2, 3, 8])
@pytest.mark.parametrize("model_name", ["smooth", "edge"])
def test_members_equal_the_host_bit_for_bit(eng, h, hs, model_name, nz, lateral):
    """(a): every unknown as a spike and as a row, a test model and a given right-hand side (at nz = 8 128 members, two lane groups), with
    the weightless centre column, with full and without; then without weights.  The stage is read only: the same runs serve every call."""
    depz, vel, rng, wt = case(model_name, nz)
    M, centre = nz - 1, 2 * NX + 2
    eng.dispersion_begin(vel, depz, R.MINTHK, K, K)
    runs(eng)
    obs, _ = observations(eng, model_name, rng, NX * NY)
    kind, index, models = members(9, M)
    got = against_host(h, hs, eng, vel, depz, obs, wt, lateral, kind, index, models)
    assert got["flag"][centre] == 0 and got["nused"][centre] == 0
    assert np.isfinite(got["full"]).all() and np.isfinite(got["measures"]).all() and not got["measures"][kind >= 2].any()
    spike = np.flatnonzero((kind == 0) & (index // M == 4))
    assert not got["full"][spike].any() and not got["itn"][spike].any()                              # a spike in the column without data
    if model_name == "smooth":
        assert (got["istop"] == 1).all() and not got["flag"].any() and got["itn"][kind == 1].min() >= 1
        assert (np.abs(got["full"][(kind == 1) & (index // M == 4)]).max(axis=(1, 2)) > 0).all()  # its rows are carried
    m = got["measures"][kind < 2]
    assert (m[:, 6] >= 0).all() and (m[:, 5] >= 0).all() and (m[:, 5] <= m[:, 1]).all()
    against_host(h, hs, eng, vel, depz, obs, wt, lateral, kind, index, models, full=False)
    against_host(h, hs, eng, vel, depz, obs, None, lateral, kind, index, models)
    assert same_bits(eng.dispersion_get_model(), vel)


def test_another_grid(eng, h, hs):
    """(b): 11 x 10 (72 interior columns), nz = 3, every fifth unknown"""
    nx, ny, nz = 11, 10, 3
    depz, vel, rng, wt = case("smooth", nz, nx, ny)
    eng.dispersion_begin(vel, depz, R.MINTHK, K, K)
    runs(eng)
    obs, _ = observations(eng, "smooth", rng, nx * ny)
    kind, index, models = members(72, nz - 1, every=5)
    got = against_host(h, hs, eng, vel, depz, obs, wt, 0.5, kind, index, models)
    assert (got["istop"] == 1).all() and got["itn"][kind == 1].min() >= 2 and not got["flag"].any() and len(np.unique(got["itn"][kind == 1])) >= 2
    assert not got["itn"][(kind == 0) & (index // 2 == 40)].any()                 # (unknown 80 is a spike in the centre column, which has no data)


def test_the_limits_once(eng, h, hs):
    """(b): nz = 64 (M = 63), K = 60 -- test_gpu_column_resolution.py's period lists -- smooth_model on the 5 x 5 grid, maxit = 5 (istop 2),
    70 members: two lane groups, the last partial, 97 272 bytes of LDS a block"""
    nz, nmaps = 64, 60
    waves = [(2, 0, np.linspace(3.0, 45.0, 15)), (2, 1, np.linspace(4.0, 46.0, 15)), (1, 0, np.linspace(3.0, 45.0, 15)), (1, 1, np.linspace(4.0, 46.0, 15))]
    depz = R.depths(nz)
    vel = R.smooth_model(NX, NY, nz)
    eng.dispersion_begin(vel, depz, R.MINTHK, nmaps, nmaps)
    runs(eng, waves)
    pv = eng.dispersion_fetch(0, nmaps, False, 0)
    obs = (np.where(pv > 0, pv, 3.0) * 1.01).astype(F)
    kind, index, models = members(9, nz - 1, every=17)
    assert len(kind) == 70
    got = against_host(h, hs, eng, vel, depz, obs, None, 0.5, kind, index, models, nmaps=nmaps, maxit=5)
    assert (got["itn"] == 5).all() and (got["istop"] == 2).all() and np.isfinite(got["full"]).all() and np.abs(got["full"]).max() > 0


def test_a_given_right_hand_side_is_the_step(eng, h, hs):
    """(c): the member of kind 3 whose f is the host's right-hand side of the coupled step on the present state gives x with (float)x = dv of
    dsa_columns_step_lateral, bit for bit, and the same itn -- that step run afterwards on the same runs with a large dvmax, the same tol and
    maxit.  The step's bits are those of a stage that never ran the resolution.  A resolution call after the step is DSA_ERR_STATE."""
    nz, lateral = 8, 0.5
    depz, vel, rng, wt = case("smooth", nz)
    M, ncol = nz - 1, NX * NY
    inner = R.interior(NX, NY) == 1
    eng.dispersion_begin(vel, depz, R.MINTHK, K, K)
    runs(eng)
    obs, _ = observations(eng, "smooth", rng, ncol)
    pv, S = host_inputs(hs, eng, vel, depz)
    bt = RR.host_rhs(h, NX, NY, obs, wt, pv, S, vel.reshape(nz, ncol), *BASE, lateral)
    kind = np.array([3], np.int32); index = np.zeros(1, np.int32)
    res = eng.columns_resolution_lateral(obs, wt, *BASE, lateral, kind, index, bt[None], TOL, MAXIT, full=True)
    step = eng.columns_step_lateral(obs, wt, *BASE, lateral, 100.0, 0.0, 100.0, TOL, MAXIT)
    after = eng.dispersion_get_model()
    assert same_bits(res["full"][0].astype(F), step["dv"][:, inner]) and np.abs(step["dv"]).max() > 0
    assert (res["itn"][0], res["istop"][0]) == (step["itn"], step["istop"]) == (step["itn"], 1) and step["itn"] >= 2
    assert same_bits(np.array([res["rz0"][0], res["rz"][0]]), np.array([step["rz0"], step["rz"]]))
    with pytest.raises(EngineError, match="has not been run") as exc:
        eng.columns_resolution_lateral(obs, wt, *BASE, lateral, kind, index, bt[None], TOL, MAXIT)
    assert exc.value.code == DSA_ERR_STATE
    eng.dispersion_begin(vel, depz, R.MINTHK, K, K)
    runs(eng)
    fresh = eng.columns_step_lateral(obs, wt, *BASE, lateral, 100.0, 0.0, 100.0, TOL, MAXIT)
    for name in ("dv", "nused", "chi2", "flag"):
        assert same_bits(step[name], fresh[name]), name
    assert (step["itn"], step["rz"]) == (fresh["itn"], fresh["rz"]) and same_bits(after, eng.dispersion_get_model())


def test_chunks_and_the_memory_budget(eng, h):
    """(d): nz = 8, 128 members.  With the memory budget at one lane group's bytes the members are solved in two chunks: the bits of the
    single-chunk run.  A budget below one group is DSA_ERR_CAPACITY with the sizes in the message, found before the device is touched: the
    runs stay fresh, and with the budget lifted the same call succeeds without new runs."""
    nz = 8
    depz, vel, rng, wt = case("smooth", nz)
    eng.dispersion_begin(vel, depz, R.MINTHK, K, K)
    runs(eng)
    obs, _ = observations(eng, "smooth", rng, NX * NY)
    kind, index, models = members(9, nz - 1)
    assert len(kind) == 128
    call = lambda: eng.columns_resolution_lateral(obs, wt, *BASE, 2.0, kind, index, models, TOL, MAXIT, full=True)
    one = call()
    group = h.hlres_group_bytes(NX, NY, nz - 1)
    try:
        eng.set_memory_budget(group)
        two = call()
        eng.set_memory_budget(group - 1)
        with pytest.raises(EngineError, match="needs %d bytes, %d are allowed" % (group, group - 1)) as exc:
            call()
        assert exc.value.code == DSA_ERR_CAPACITY
    finally:
        eng.set_memory_budget(0)
    for name in NAMES:
        assert same_bits(one[name], two[name]), name
    assert len(np.unique(one["itn"])) >= 2
    again = call()
    for name in NAMES:
        assert same_bits(one[name], again[name]), name


def test_refusals(eng):
    """(e): a radial stage is DSA_ERR_STATE; a bad lateral, tol or maxit, no member, a kind or an index out of range, models missing or not
    finite are DSA_ERR_ARGUMENT -- found before the device is touched: the runs stay fresh, so the good call at the end succeeds"""
    nz = 3
    depz, vel, rng, wt = case("smooth", nz)
    obs = np.full((K, NX * NY), 3.0, F)
    models = np.ones((2, nz - 1, 9))
    good = dict(lateral=0.2, tol=1e-8, maxit=50, kind=[0, 1, 2, 3], index=[17, 0, 1, 0], models=models)

    def refused(match, **kw):
        a = dict(good, **kw)
        with pytest.raises(EngineError, match=match) as exc:
            eng.columns_resolution_lateral(obs, None, *BASE, a["lateral"], a["kind"], a["index"], a["models"], a["tol"], a["maxit"])
        return exc.value.code

    eng.dispersion_begin_radial(vel, vel, depz, R.MINTHK, K, K)
    runs(eng)
    assert refused("radial") == DSA_ERR_STATE
    eng.dispersion_begin(vel, depz, R.MINTHK, K, K)
    runs(eng)
    for bad in (-0.1, np.nan):
        assert refused("lateral", lateral=bad) == DSA_ERR_ARGUMENT
    for bad in (0.0, np.inf):
        assert refused("tol", tol=bad) == DSA_ERR_ARGUMENT
    assert refused("maxit", maxit=0) == DSA_ERR_ARGUMENT
    assert refused("nmembers", kind=[], index=[]) == DSA_ERR_ARGUMENT
    for bad in (-1, 4):
        assert refused("kind", kind=[0, bad, 2, 3]) == DSA_ERR_ARGUMENT
    for bad in ([18, 0, 1, 0], [0, -1, 1, 0], [0, 0, 2, 0], [0, 0, 0, -1]):
        assert refused("index", index=bad) == DSA_ERR_ARGUMENT
    assert refused("models is required", models=None) == DSA_ERR_ARGUMENT
    nan = models.copy(); nan[1, 0, 3] = np.nan
    assert refused("not finite", models=nan) == DSA_ERR_ARGUMENT
    with pytest.raises(ValueError):
        eng.columns_resolution_lateral(obs, None, *BASE, 0.2, [0, 1], [0], None)
    with pytest.raises(ValueError):
        eng.columns_resolution_lateral(obs, None, *BASE, 0.2, [2], [0], np.ones((1, nz, 9)))
    ok = eng.columns_resolution_lateral(obs, None, *BASE, good["lateral"], good["kind"], good["index"], models, good["tol"], good["maxit"])
    assert (ok["istop"] == 1).all() and not ok["flag"].any()
    only = eng.columns_resolution_lateral(obs, None, *BASE, good["lateral"], [0, 1], [17, 0], None, good["tol"], good["maxit"])           # no models needed
    assert same_bits(only["measures"], ok["measures"][:2])
