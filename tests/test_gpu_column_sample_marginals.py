"""The posterior marginals of the sample stage (dsa_columns_sample_marginals, _marginals_fetch, _marginals_state; csrc/column_kernels.hip:
k_sample_hist, k_sample_cov, k_sample_marginal_finish) on the device against the CPU build of the same header
(tests/hostcheck_column_sample_marginals.cpp through column_sample_marginals_ref), bit for bit, and against the NumPy twin.  The set-up is
tests/test_gpu_column_sample.py's: grid 5 x 5, columns_ref.WAVES (K = 12), nz = 2, 3, 8, smooth_model and edge_model, weights with some zeros
and the centre column all zero.  The host accumulates every sweep from the state fetched from the device, so neither the dispersion stage
nor the sampler's own arithmetic is under test here.

Measured on the MI355X: see DESIGN.md section 33."""
import numpy as np
import pytest

import column_sample_marginals_ref as M33
import column_sample_ref as S
import columns_ref as R
import test_gpu_column_sample as G
import test_gpu_column_sample_block as GB
from dsurftomo_amd import depth
from dsurftomo_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

F = np.float32
NX, NY, K, NCOL, RING, CENTRE = G.NX, G.NY, G.K, G.NCOL, G.RING, G.CENTRE
DSA_ERR_ARGUMENT, DSA_ERR_STATE = G.DSA_ERR_ARGUMENT, G.DSA_ERR_STATE
same_bits = G.same_bits
LEVELS = M33.LEVELS


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def hm():
    return M33.load()


def host(hm, vel, obs, wt, C, par, seed, burn, nbins, with_cov=True):
    nz = vel.shape[0]
    return M33.MarginalStage(hm, NX, NY, vel.reshape(nz, NCOL), obs, wt, C, par["smooth"], par["step"], par["spread"], par["width"], par["temperature"], par["minvel"],
                             par["maxvel"], seed, burn, nbins=nbins, with_cov=with_cov)


def assert_marginal_state(eng, hs, what):
    dev, want = eng.columns_sample_marginals_state(), hs.marginal_state()
    assert sorted(dev) == sorted(want)
    for name in want:
        assert same_bits(dev[name], want[name]), "%s: %s differs from the host's (%d of %d)" % (what, name, int((dev[name] != want[name]).sum()), want[name].size)
    return dev


def assert_marginal_fetch(got, want):
    assert sorted(got) == sorted(want)
    for name in want:
        assert same_bits(np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])), name


def laws(st, ms, res, mg, vel, par, nkept):
    """CPU check 3's laws on the device's arrays"""
    nz = vel.shape[0]
    M = nz - 1
    moving = ~RING & (res["flag"] == 0)
    assert moving.sum() == 8 and res["flag"][CENTRE] == 2
    total = ms["hist"].sum(axis=0, dtype=np.int64)                                   # (M, C, ncol)
    assert (total[:, :, moving] == nkept).all() and not ms["hist"][:, :, :, ~moving].any()
    assert (res["nkept"] == nkept * moving).all()
    lo, hi = depth.sample_box(vel.reshape(nz, NCOL)[:M], par["width"], par["minvel"], par["maxvel"])
    q = mg["quantiles"]
    if nkept:
        assert (np.diff(q, axis=0) >= 0).all() and (q[:, :, moving] >= lo[:, moving]).all() and (q[:, :, moving] <= hi[:, moving]).all()
        assert (mg["mode"][:, moving] > lo[:, moving]).all() and (mg["mode"][:, moving] < hi[:, moving]).all()
    else:
        assert not q.any() and not mg["mode"].any()
    assert not q[:, :, ~moving].any() and not mg["mode"][:, ~moving].any() and not mg["hist"][:, :, ~moving].any()
    assert same_bits(mg["hist"], ms["hist"].sum(axis=2, dtype=np.uint32))
    assert all(np.isfinite(a).all() for a in mg.values()) and all(np.isfinite(a).all() for a in ms.values())
    if "P" in ms:
        for i in range(M):
            assert same_bits(ms["P"][depth.column_tri(i, i)], st["S2"][i])          # the diagonal of P is S2
            assert same_bits(mg["cov"][depth.column_tri(i, i)], res["var"][i])      # the diagonal of cov is the fetched variance
        assert not ms["P"][:, :, ~moving].any() and not mg["cov"][:, ~moving].any()


REPLAY = [("smooth", 2, 3, 2, 0), ("smooth", 2, 27, 7, 0), ("smooth", 3, 3, 64, 0), ("smooth", 3, 27, 2, 0), ("smooth", 8, 3, 7, 0), ("smooth", 8, 27, 64, 0),
          ("smooth", 8, 3, 64, 2), ("smooth", 8, 27, 7, 2), ("edge", 8, 3, 7, 0), ("edge", 8, 27, 2, 2)]


@pytest.mark.parametrize("model_name,nz,C,nbins,every", REPLAY)
def test_replay_bit_for_bit(eng, hm, model_name, nz, C, nbins, every):
    """(a): the set-up and six sweeps of run(1), burn 2, the covariance on; after each the host build takes the device's fetched state and
    accumulates from it: hist and P are the device's after every sweep, the final fetch (five levels) is the host's finish; the NumPy twin
    reproduces the pooled counts from the models fetched after each sweep"""
    depz, vel, obs, wt, par = G.case(eng, model_name, nz)
    if every:
        GB.device_shape(eng, vel, depz, obs, wt, par["smooth"])
    seed, burn = 2 ** 37 + 17 * nz + C, 2
    G.begin(eng, vel, depz, obs, wt, C, par, seed, burn)
    if every:
        eng.columns_sample_blocks(every, depth.sample_block_scale(nz - 1, par["temperature"]))
    eng.columns_sample_marginals(nbins, True)
    hs = host(hm, vel, obs, wt, C, par, seed, burn, nbins)
    assert_marginal_state(eng, hs, "set-up")
    pooled = np.zeros((nbins, nz - 1, NCOL), np.int64)
    for sweep in range(1, 7):
        eng.columns_sample_run(1)
        dev = eng.columns_sample_state()
        hs.take(dev, sweep)
        hs.accumulate()
        assert_marginal_state(eng, hs, "sweep %d" % sweep)
        if sweep > burn:
            moving = dev["pmark"][0] != S.IDLE
            pooled[:, :, moving] += depth.sample_marginal_counts(dev["models"], vel.reshape(nz, NCOL), par["width"], par["minvel"], par["maxvel"], nbins)[:, :, moving]
    got, want = eng.columns_sample_marginals_fetch(LEVELS), hs.marginal_finish(LEVELS)
    assert_marginal_fetch(got, want)
    assert same_bits(got["hist"], pooled.astype(np.uint32))
    mode, quant = depth.sample_marginal_twin(got["hist"], vel.reshape(nz, NCOL), par["width"], par["minvel"], par["maxvel"], LEVELS)
    assert same_bits(got["mode"], mode) and same_bits(np.ascontiguousarray(got["quantiles"]), quant)
    assert got["hist"].sum() == 4 * C * (nz - 1) * int((~RING & (dev["pmark"][0] != S.IDLE)).sum()) > 0
    if every:
        assert eng.columns_sample_block_state()["block_counters"][0].max() == 6 // every


def test_one_call_equals_seven(eng):
    """(b): run(7) against seven run(1), every second sweep a block sweep, burn 3 inside the run: all new arrays are equal"""
    depz, vel, obs, wt, par = G.case(eng, "smooth", 8)
    GB.device_shape(eng, vel, depz, obs, wt, par["smooth"])
    out = []
    for calls in ((7,), (1,) * 7):
        G.begin(eng, vel, depz, obs, wt, 5, par, 99, 3)
        eng.columns_sample_marginals(7, True)                                       # before the blocks: either order
        eng.columns_sample_blocks(2, depth.sample_block_scale(7, par["temperature"]))
        for n in calls:
            eng.columns_sample_run(n)
        out.append((eng.columns_sample_marginals_state(), eng.columns_sample_marginals_fetch(LEVELS), eng.columns_sample_state()))
    for part in (0, 1, 2):
        for name in out[0][part]:
            assert same_bits(np.ascontiguousarray(out[0][part][name]), np.ascontiguousarray(out[1][part][name])), name
    assert out[0][1]["hist"].sum() == 4 * 5 * 7 * 8 and out[0][0]["P"].any()


def test_only_observes(eng):
    """(c): with the marginals on, state, block state and fetch have the bits of a fresh engine's run without them; on and then nbins = 0
    is off; a begin after a stage that had them on starts with them off"""
    depz, vel, obs, wt, par = G.case(eng, "smooth", 8)
    scale = depth.sample_block_scale(7, par["temperature"])
    fresh = Engine(0)
    try:
        GB.device_shape(fresh, vel, depz, obs, wt, par["smooth"])
        G.begin(fresh, vel, depz, obs, wt, 4, par, 17, 2)
        fresh.columns_sample_blocks(2, scale)
        fresh.columns_sample_run(6)
        want = fresh.columns_sample_state(), fresh.columns_sample_block_state(), fresh.columns_sample_fetch()
    finally:
        fresh.close()
    GB.device_shape(eng, vel, depz, obs, wt, par["smooth"])

    def run(mode):
        G.begin(eng, vel, depz, obs, wt, 4, par, 17, 2)
        eng.columns_sample_blocks(2, scale)
        if mode in ("on", "on-off"):                                               # ("after": a begin after a stage that had them on, and no call)
            eng.columns_sample_marginals(64, True)
        if mode == "on-off":
            eng.columns_sample_marginals(0, 0)
        eng.columns_sample_run(6)
        return eng.columns_sample_state(), eng.columns_sample_block_state(), eng.columns_sample_fetch()

    for mode in ("on", "after", "on-off"):
        got = run(mode)
        for part in (0, 1, 2):
            for name in want[part]:
                assert same_bits(got[part][name], want[part][name]), (mode, name)
        if mode == "on":
            assert eng.columns_sample_marginals_state()["hist"].sum() == 4 * 4 * 7 * 8
        else:
            for call in (eng.columns_sample_marginals_state, lambda: eng.columns_sample_marginals_fetch(LEVELS)):
                with pytest.raises(EngineError, match="marginals are off") as exc:
                    call()
                assert exc.value.code == DSA_ERR_STATE


def test_laws_and_what_stays(eng):
    """(d): the laws of the counts and the finish; the ring, the flag-2 column and the bottom depth are zero or untouched; nothing is NaN;
    one chain works; burn = sweeps gives zeros; with_cov = 0 leaves hist as it is bit for bit and refuses a cov fetch"""
    nz, sweeps = 8, 20
    depz, vel, obs, wt, par = G.case(eng, "smooth", nz)
    par = dict(par, width=0.08, step=0.1)                                          # a narrow box that the proposals often leave
    before = vel.reshape(nz, NCOL)
    hist_with_cov = None
    for C, burn, with_cov in ((4, 5, True), (4, 5, False), (1, 5, True), (3, 20, True)):
        G.begin(eng, vel, depz, obs, wt, C, par, 3, burn)
        eng.columns_sample_marginals(16, with_cov)
        eng.columns_sample_run(sweeps)
        st, ms, res = eng.columns_sample_state(), eng.columns_sample_marginals_state(), eng.columns_sample_fetch()
        mg = eng.columns_sample_marginals_fetch(LEVELS)
        assert ("P" in ms) == with_cov and ("cov" in mg) == with_cov
        laws(st, ms, res, mg, vel, par, sweeps - burn)
        m = st["models"]
        for q in range(C):
            assert same_bits(m[:, q][:, RING], before[:, RING]) and same_bits(m[nz - 1, q], before[nz - 1]) and same_bits(m[:, q, CENTRE], before[:, CENTRE])
        assert mg["hist"].shape == (16, nz - 1, NCOL) and ms["hist"].shape == (16, nz - 1, C, NCOL)      # no bottom depth in the new arrays
        if burn == sweeps:
            assert not ms["hist"].any() and not ms["P"].any() and not mg["cov"].any()
        elif C == 4:
            ends = (mg["hist"][0] + mg["hist"][-1]).sum() / mg["hist"].sum()
            print("with_cov %d: %.1f %% of the kept states in an end bin of a box of half width %.2f km/s" % (with_cov, 100.0 * ends, par["width"]))
            if with_cov:
                hist_with_cov = ms["hist"]
            else:
                assert same_bits(ms["hist"], hist_with_cov)                        # the covariance does not show in the counts
                with pytest.raises(EngineError, match="with_cov") as exc:
                    eng.columns_sample_marginals_fetch(LEVELS, cov=True)
                assert exc.value.code == DSA_ERR_STATE
                assert eng._L.dsa_columns_sample_marginals_state(eng._h, None, ms["hist"].ctypes.data) == DSA_ERR_STATE
                no_hist = eng.columns_sample_marginals_fetch((0.5,), hist=False)       # hist may be NULL
                assert "hist" not in no_hist and same_bits(no_hist["quantiles"][0], mg["quantiles"][2])


def test_refusals(eng):
    """(e): marginals without a stage or after a sweep, bad nbins and with_cov; the fetch while they are off, with bad levels, without
    figures; the engine usable after each, an open stage as it was"""
    nz = 3
    depz, vel, obs, wt, par = G.case(eng, "smooth", nz)

    def refused(call, code, match=None):
        with pytest.raises(EngineError, match=match) as exc:
            call()
        assert exc.value.code == code

    eng.dispersion_begin(vel, depz, R.MINTHK, K, K)                              # a plain stage: no sample stage is open
    refused(lambda: eng.columns_sample_marginals(8, True), DSA_ERR_STATE, "dsa_columns_sample_begin")
    refused(lambda: eng.columns_sample_marginals_fetch(LEVELS), DSA_ERR_STATE, "dsa_columns_sample_begin")
    refused(eng.columns_sample_marginals_state, DSA_ERR_STATE)
    G.begin(eng, vel, depz, obs, wt, 2, par, 1, 0)
    refused(lambda: eng.columns_sample_marginals_fetch(LEVELS), DSA_ERR_STATE, "marginals are off")
    for nbins, cov in ((-1, 0), (1, 0), (257, 1), (2 ** 20, 0)):
        refused(lambda: eng.columns_sample_marginals(nbins, cov), DSA_ERR_ARGUMENT, "nbins")
    for cov in (2, -1):
        refused(lambda: eng.columns_sample_marginals(8, cov), DSA_ERR_ARGUMENT, "with_cov")
    refused(lambda: eng.columns_sample_marginals_fetch(LEVELS), DSA_ERR_STATE, "marginals are off")      # a refusal switched nothing on
    eng.columns_sample_marginals(8, True)
    eng.columns_sample_marginals(256, False)                                         # again, before the first sweep: the last call holds
    eng.columns_sample_marginals(8, True)
    eng.columns_sample_run(2)
    kept = dict(eng.columns_sample_state(), **eng.columns_sample_marginals_state())
    mg = eng.columns_sample_marginals_fetch(LEVELS)
    refused(lambda: eng.columns_sample_marginals(8, True), DSA_ERR_STATE, "sweeps have been run")
    refused(lambda: eng.columns_sample_marginals(0, 0), DSA_ERR_STATE, "sweeps have been run")
    for levels in ((0.0,), (1.0,), (0.5, -0.1), (np.nan,), (np.inf,), (0.5, 1.5), tuple([0.5] * 17)):
        refused(lambda: eng.columns_sample_marginals_fetch(levels), DSA_ERR_ARGUMENT, "level")
    lv = np.array(LEVELS)
    assert eng._L.dsa_columns_sample_marginals_fetch(eng._h, -1, lv.ctypes.data, None, mg["mode"].ctypes.data, None) == DSA_ERR_ARGUMENT
    assert eng._L.dsa_columns_sample_marginals_fetch(eng._h, 5, lv.ctypes.data, None, None, None) == DSA_ERR_ARGUMENT      # figures is required
    assert eng._L.dsa_columns_sample_marginals_fetch(eng._h, 5, None, None, mg["mode"].ctypes.data, None) == DSA_ERR_ARGUMENT
    assert eng._L.dsa_columns_sample_marginals_state(eng._h, None, None) == 0      # each pointer may be NULL
    now = dict(eng.columns_sample_state(), **eng.columns_sample_marginals_state())
    for name in kept:
        assert same_bits(kept[name], now[name]), name                              # the open stage is as it was
    assert_marginal_fetch(eng.columns_sample_marginals_fetch(LEVELS), mg)
    none = eng.columns_sample_marginals_fetch(())                                    # no level: the mode alone
    assert none["quantiles"].shape == (0, nz - 1, NCOL) and same_bits(none["mode"], mg["mode"])
    eng.columns_sample_run(2)                                                        # and goes on
    assert eng.columns_sample_marginals_state()["hist"].sum() == 4 * 2 * (nz - 1) * 8
