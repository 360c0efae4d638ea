"""The block proposals of the sample stage (dsa_columns_sample_shape, dsa_columns_sample_blocks, dsa_columns_sample_block_state;
csrc/column_kernels.hip: k_sample_shape, k_sample_propose_block, k_sample_accept_block) on the device against the CPU
build of the same header (tests/hostcheck_column_sample_block.cpp through column_sample_block_ref), bit for bit.  The set-up is
tests/test_gpu_column_sample.py's: grid 5 x 5, columns_ref.WAVES (K = 12), nz = 2, 3, 8, smooth_model and edge_model, weights with some zeros
and the centre column all zero.  The host replays every sweep from the curves fetched from the device and with the device's shape, so the
dispersion stage's own arithmetic is not under test here.

(f), measured on the MI355X: see DESIGN.md section 32."""
import numpy as np
import pytest

import column_sample_block_ref as B
import column_sample_ref as S
import columns_ref as R
import test_gpu_column_sample as G
from dsurftomo_amd import depth
from dsurftomo_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

F = np.float32
NX, NY, K, NCOL, RING, CENTRE, SIGMA = G.NX, G.NY, G.K, G.NCOL, G.RING, G.CENTRE, G.SIGMA
DSA_ERR_ARGUMENT, DSA_ERR_STATE = G.DSA_ERR_ARGUMENT, G.DSA_ERR_STATE
same_bits = G.same_bits
DAMP = R.DAMP / SIGMA                                          # the step's damp scaled as the sampler's weights are


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def hb():
    return B.load()


@pytest.fixture(scope="module")
def hc():
    return R.load()


def with_kernels(e, vel, depz):
    """a single-model stage on vel whose maps and slots were all run with kernels"""
    e.dispersion_begin(vel, depz, R.MINTHK, K, K)
    first = 0
    for wave, kind, t in R.WAVES:
        e.dispersion_run(wave, kind, t, True, first, first)
        first += len(t)


def device_shape(e, vel, depz, obs, wt, smooth):
    with_kernels(e, vel, depz)
    return e.columns_sample_shape(obs, wt, smooth, DAMP)


def host(hb, vel, obs, wt, C, par, seed, burn, shape, every, scale):
    nz = vel.shape[0]
    return B.BlockStage(hb, NX, NY, vel.reshape(nz, NCOL), obs, wt, C, par["smooth"], par["step"], par["spread"], par["width"], par["temperature"], par["minvel"],
                        par["maxvel"], seed, burn, shape, every, scale)


def device_state(e):
    return dict(e.columns_sample_state(), **e.columns_sample_block_state())


def assert_state(dev, hs, what):
    want = hs.state()
    for name in S.STATE + B.BLOCK_STATE:
        assert same_bits(dev[name], want[name]), "%s: %s differs from the host's (%d of %d)" % (what, name, int((dev[name] != want[name]).sum()), want[name].size)


@pytest.mark.parametrize("nz", [2, 3, 8])
@pytest.mark.parametrize("model_name", ["smooth", "edge"])
def test_shape_bit_for_bit_and_the_stage_stays(eng, hb, hc, model_name, nz):
    """(a): tri, r and flag against the host build on the curve and kernels dispersion_fetch returns; a step after the shape call gives the
    bits of a step without it"""
    depz, vel, obs, wt, par = G.case(eng, model_name, nz)
    with_kernels(eng, vel, depz)
    pv, svs, svp, srho = eng.dispersion_fetch(0, K, True, 0)
    Sk = R.host_combine(hc, vel.reshape(nz, NCOL), depz, svs, svp, srho)
    want = B.shape(hb, NX, NY, obs, wt, pv, Sk, par["smooth"], DAMP)
    got = eng.columns_sample_shape(obs, wt, par["smooth"], DAMP)
    for name in ("tri", "r", "flag"):
        assert same_bits(got[name], want[name]), "%s differs from the host's (%d of %d)" % (name, int((got[name] != want[name]).sum()), got[name].size)
    inner = ~RING
    assert got["flag"][CENTRE] == 2 and not got["flag"][RING].any() and (got["flag"][inner] == 0).sum() >= 4
    ok = inner & (got["flag"] == 0)
    assert (got["r"][:, ok] > 0).all() and not got["r"][:, ~ok].any() and not got["tri"][:, ~ok].any() and np.isfinite(got["tri"]).all()
    assert eng._L.dsa_columns_sample_shape(eng._h, K, obs.ctypes.data, wt.ctypes.data, par["smooth"], DAMP, None, None, None) == 0      # every output may be NULL
    after_shape = eng.columns_step(obs, wt, *G.R_ARGS), eng.dispersion_get_model()
    with_kernels(eng, vel, depz)
    plain = eng.columns_step(obs, wt, *G.R_ARGS), eng.dispersion_get_model()
    for name in plain[0]:
        assert same_bits(after_shape[0][name], plain[0][name]), name
    assert same_bits(after_shape[1], plain[1])


@pytest.mark.parametrize("every", [1, 2])
@pytest.mark.parametrize("model_name,nz,C", [("smooth", 2, 3), ("smooth", 2, 27), ("smooth", 3, 3), ("smooth", 3, 27), ("smooth", 8, 3), ("smooth", 8, 27), ("edge", 8, 3)])
def test_replay_bit_for_bit(eng, hb, model_name, nz, C, every):
    """(b): the set-up and six sweeps of run(1), burn 2; after each the host proposes from the previous state with the device's shape and
    accepts from the device's fetched curves; every array of the state, the block state and the final fetch is the device's"""
    depz, vel, obs, wt, par = G.case(eng, model_name, nz)
    shape = device_shape(eng, vel, depz, obs, wt, par["smooth"])
    scale = depth.sample_block_scale(nz - 1, par["temperature"])
    seed, burn = 2 ** 36 + 13 * nz + C, 2
    G.begin(eng, vel, depz, obs, wt, C, par, seed, burn)
    eng.columns_sample_blocks(every, scale)
    hs = host(hb, vel, obs, wt, C, par, seed, burn, shape, every, scale)
    hs.setup_models()
    hs.setup_state(G.maps_of(eng, C))
    assert_state(device_state(eng), hs, "set-up")
    for sweep in range(1, 7):
        hs.propose()
        proposed = hs.a["pmark"].copy()
        eng.columns_sample_run(1)
        dev = device_state(eng)
        assert ((dev["pmark"] == S.OUT_OF_BOX) == (proposed == S.OUT_OF_BOX)).all() and ((dev["pmark"] == S.IDLE) == (proposed == S.IDLE)).all()
        hs.accept(G.maps_of(eng, C))
        assert_state(dev, hs, "sweep %d" % sweep)
    bc = dev["block_counters"]
    moving = ~RING & (dev["pmark"][0] != S.IDLE)
    blocked = moving & (shape["flag"] == 0)
    assert blocked.sum() >= 4 and (bc[0][:, blocked] == 6 // every).all() and not bc[:, :, ~blocked].any()
    G.assert_fetch(eng.columns_sample_fetch(), hs)


def test_one_call_equals_seven(eng):
    """(c): run(7) against seven run(1), every second sweep a block sweep, burn 3 inside the run"""
    depz, vel, obs, wt, par = G.case(eng, "smooth", 8)
    device_shape(eng, vel, depz, obs, wt, par["smooth"])
    out = []
    for calls in ((7,), (1,) * 7):
        G.begin(eng, vel, depz, obs, wt, 5, par, 99, 3)
        eng.columns_sample_blocks(2, depth.sample_block_scale(7, par["temperature"]))
        for n in calls:
            eng.columns_sample_run(n)
        out.append((device_state(eng), eng.columns_sample_fetch()))
    for part in (0, 1):
        for name in out[0][part]:
            assert same_bits(out[0][part][name], out[1][part][name]), name
    bc = out[0][0]["block_counters"]
    assert bc[0].max() == 3 and bc[1].sum() > 0 and (out[0][1]["nkept"][~RING & (out[0][1]["flag"] == 0)] == 4).all()


def test_off_means_the_single_node_bits(eng):
    """(d): a stage opened after a shape call without dsa_columns_sample_blocks, and one with block_every = 0, against a stage on a fresh
    engine"""
    depz, vel, obs, wt, par = G.case(eng, "smooth", 8)
    fresh = Engine(0)
    try:
        G.begin(fresh, vel, depz, obs, wt, 4, par, 17, 2)
        fresh.columns_sample_run(6)
        want = fresh.columns_sample_state(), fresh.columns_sample_fetch()
    finally:
        fresh.close()
    device_shape(eng, vel, depz, obs, wt, par["smooth"])
    for off in (False, True):
        G.begin(eng, vel, depz, obs, wt, 4, par, 17, 2)
        if off:
            eng.columns_sample_blocks(2, 1.0)
            eng.columns_sample_blocks(0, 1.0)                                      # on, and off again
        eng.columns_sample_run(6)
        got = eng.columns_sample_state(), eng.columns_sample_fetch()
        for part in (0, 1):
            for name in want[part]:
                assert same_bits(got[part][name], want[part][name]), name
        blk = eng.columns_sample_block_state()
        assert not blk["block_counters"].any() and not blk["pold_all"].any()


def test_what_stays(eng):
    """(e): a narrow box that block proposals of scale 0.3 leave: accepted + rejected = sweeps, the block counters agree with the others, every node is
    inside its box, nothing is NaN, the ring, the bottom depth and the all-zero column are untouched"""
    nz, sweeps = 8, 20
    depz, vel, obs, wt, par = G.case(eng, "smooth", nz)
    par = dict(par, width=0.08)
    shape = device_shape(eng, vel, depz, obs, wt, par["smooth"])
    before = vel.reshape(nz, NCOL)
    for C, every in ((4, 1), (1, 3)):
        G.begin(eng, vel, depz, obs, wt, C, par, 3, 5)
        eng.columns_sample_blocks(every, 0.3)
        eng.columns_sample_run(sweeps)
        st, res = device_state(eng), eng.columns_sample_fetch()
        m = st["models"]
        for q in range(C):
            assert same_bits(m[:, q][:, RING], before[:, RING]) and same_bits(m[nz - 1, q], before[nz - 1]) and same_bits(m[:, q, CENTRE], before[:, CENTRE])
        lo = np.maximum(F(par["minvel"]), before[:nz - 1] - F(par["width"])); hi = np.minimum(F(par["maxvel"]), before[:nz - 1] + F(par["width"]))
        assert (m[:nz - 1] >= lo[:, None]).all() and (m[:nz - 1] <= hi[:, None]).all()
        assert all(np.isfinite(a).all() for a in st.values()) and all(np.isfinite(a).all() for a in res.values())
        moving = ~RING & (res["flag"] == 0)
        assert res["flag"][CENTRE] == 2 and moving.sum() == 8 and (shape["flag"][moving] == 0).all()
        cnt, bc = st["counters"], st["block_counters"]
        total = cnt[0] + cnt[1]
        assert (total[:, moving] == sweeps).all() and not total[:, ~moving].any()
        assert (bc[0][:, moving] == sweeps // every).all() and not bc[:, :, ~moving].any()
        assert (bc[1] + bc[2] <= bc[0]).all() and (bc[1] <= cnt[0]).all() and (bc[2] <= cnt[2]).all()
        print("C %d every %d: %d block proposals, %d accepted, %d out of the box" % (C, every, bc[0].sum(), bc[1].sum(), bc[2].sum()))
        if C == 4:
            assert bc[2].sum() > 0 and bc[1].sum() > 0
        if every == 1:
            assert same_bits(bc[1], cnt[0]) and same_bits(bc[2], cnt[2])
        assert (res["accepted"] + res["rejected"] == sweeps * C * moving).all() and (res["nkept"] == (sweeps - 5) * moving).all()


def test_block_sweeps_converge_further(eng):
    """(f): section 29's convergence run -- nz = 8, 16 chains, 400 sweeps, burn 200, sigma 0.02, smooth 10, a wide box, start perturbed --
    once single-node and once with every second sweep a block sweep at the default scale: the median R-hat - 1 over the unknowns of the block
    run is smaller, and its mean kept phi is still below a quarter of phi at the start.  The twin on the oracle's dispersion, and the
    device: see DESIGN.md section 32."""
    nz, C, sweeps, burn = 8, 16, 400, 200
    depz = R.depths(nz)
    truth = R.smooth_model(NX, NY, nz)
    obs = G.curves_of(eng, truth, depz).astype(F)
    start = R.perturbed(truth)
    wt = np.full((K, NCOL), 1.0 / SIGMA, F)
    inner = ~RING
    shape = device_shape(eng, start, depz, obs, wt, 10.0)
    assert (shape["flag"][inner] == 0).all()
    median = {}
    for every in (0, 2):
        eng.columns_sample_begin(start, depz, R.MINTHK, G.PLAN, obs, wt, C, 10.0, 0.05, 0.05, 5.0, 1.0, R.MINVEL, R.MAXVEL, 20261020, burn)
        if every:
            eng.columns_sample_blocks(every, depth.sample_block_scale(nz - 1, 1.0))
        eng.columns_sample_run(sweeps)
        res = eng.columns_sample_fetch()
        bc = eng.columns_sample_block_state()["block_counters"]
        assert (res["flag"][inner] == 0).all() and (res["nkept"][inner] == sweeps - burn).all()
        phi0, phi1 = float(res["phi_start"][inner].mean()), float(res["mean_phi"][inner].mean())
        rhat = depth.sample_rhat(res["W"], res["B"], res["nkept"][None])[:, inner]
        median[every] = float(np.median(rhat)) - 1.0
        print("block_every %d: phi per column %.2f at the start, %.2f over the kept sweeps (%.1f %%); accepted %.1f %% (block proposals: %d of %d); R-hat median %.4f, worst %.4f"
              % (every, phi0, phi1, 100 * phi1 / phi0, 100.0 * res["accepted"].sum() / (res["accepted"].sum() + res["rejected"].sum()), bc[1].sum(), bc[0].sum(),
                 float(np.median(rhat)), float(rhat.max())))
        assert phi1 < 0.25 * phi0
    assert median[2] < median[0]


def test_refusals(eng):
    """(g): blocks without a stage, after a sweep, without a shape or with one of other dimensions, bad arguments; the shape call on a
    multi-model or unmarked stage; the engine usable after each, an open stage as it was"""
    nz = 3
    depz, vel, obs, wt, par = G.case(eng, "smooth", nz)

    def refused(call, code, match=None):
        with pytest.raises(EngineError, match=match) as exc:
            call()
        assert exc.value.code == code

    fresh = Engine(0)
    try:
        G.begin(fresh, vel, depz, obs, wt, 2, par, 1, 0)
        refused(lambda: fresh.columns_sample_blocks(1, 1.0), DSA_ERR_STATE, "no shape")                  # no shape was ever built here
        fresh.columns_sample_run(1)
    finally:
        fresh.close()
    eng.dispersion_begin(vel, depz, R.MINTHK, K, K)                              # a plain stage, nothing run with kernels
    refused(lambda: eng.columns_sample_shape(obs, wt, par["smooth"], DAMP), DSA_ERR_STATE, "has not been run")
    refused(lambda: eng.columns_sample_blocks(1, 1.0), DSA_ERR_STATE, "dsa_columns_sample_begin")     # no sample stage
    refused(eng.columns_sample_block_state, DSA_ERR_STATE)
    eng.dispersion_begin_models(np.stack([vel, vel]), depz, R.MINTHK, K)
    refused(lambda: eng.columns_sample_shape(obs, wt, par["smooth"], DAMP), DSA_ERR_STATE, "2 models")
    with_kernels(eng, vel, depz)
    refused(lambda: eng.columns_sample_shape(obs, wt, par["smooth"], 0.0), DSA_ERR_ARGUMENT, "damp")
    refused(lambda: eng.columns_sample_shape(obs[:5], wt[:5], par["smooth"], DAMP), DSA_ERR_ARGUMENT, "maps")
    eng.columns_sample_shape(obs, wt, par["smooth"], DAMP)
    depz8, vel8, obs8, wt8, par8 = G.case(eng, "smooth", 8)
    G.begin(eng, vel8, depz8, obs8, wt8, 2, par8, 1, 0)
    refused(lambda: eng.columns_sample_blocks(1, 1.0), DSA_ERR_STATE, "held shape")                    # a shape of nz = 3, a stage of nz = 8
    eng.columns_sample_run(1)
    G.begin(eng, vel, depz, obs, wt, 2, par, 1, 0)
    for every, scale in ((-1, 1.0), (1, 0.0), (1, -2.0), (1, np.nan), (1, np.inf)):
        refused(lambda: eng.columns_sample_blocks(every, scale), DSA_ERR_ARGUMENT, "block_every" if every < 0 else "block_scale")
    eng.columns_sample_blocks(2, 0.5)
    eng.columns_sample_run(2)
    kept = device_state(eng)
    refused(lambda: eng.columns_sample_blocks(1, 1.0), DSA_ERR_STATE, "sweeps have been run")
    refused(lambda: eng.columns_sample_shape(obs, wt, par["smooth"], DAMP), DSA_ERR_STATE, "sample stage")
    now = device_state(eng)
    for name in kept:
        assert same_bits(kept[name], now[name]), name                              # the open stage is as it was
    eng.columns_sample_run(2)                                                      # and goes on: sweep 4 is a block sweep
    assert eng.columns_sample_block_state()["block_counters"][0].max() == 2
