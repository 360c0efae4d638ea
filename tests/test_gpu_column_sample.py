"""dsa_columns_sample_* (csrc/column_kernels.hip: k_sample_*) on the device against the CPU build of the same header
(tests/hostcheck_column_sample.cpp through column_sample_ref), bit for bit: one thread per (column, chain) runs column_sample.h's sequential
fp64 chains under -ffp-contract=off, without libm, a square root or an atomic, so the mapping cannot show.  The host replays every sweep
from the curves fetched from the device, so the dispersion stage's own arithmetic is not under test here -- except in (c), which checks
that a chain's maps are those of its model alone.

Grid 5 x 5 (9 interior columns), columns_ref.WAVES (K = 12), nz = 2, 3, 8, test_gpu_dispersion.py's smooth_model and edge_model (the latter
has columns that lose Love roots), weights with some zeros and the centre column all zero.

(e), measured on the MI355X: see DESIGN.md section 29."""
import numpy as np
import pytest

import column_sample_ref as S
import columns_ref as R
from dsurftomo_amd import depth
from dsurftomo_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

F = np.float32
NX, NY, K = R.NX, R.NY, R.K
NCOL = NX * NY
RING = R.interior(NX, NY) == 0
CENTRE = 2 * NX + 2
DSA_ERR_ARGUMENT, DSA_ERR_STATE = -2, -5                      # include/dsurftomo_amd.h
PLAN = [(wave, kind, t) for wave, kind, t in R.WAVES]
SIGMA = 0.02
# smooth, step, spread, width, temperature, minvel, maxvel
PAR = dict(smooth=3.0, step=0.05, spread=0.05, width=0.4, temperature=1.0, minvel=R.MINVEL, maxvel=R.MAXVEL)


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def h():
    return S.load()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def curves_of(e, vel, depz):
    """the device's own curves of one model, (K, ncol)"""
    e.dispersion_begin(vel, depz, R.MINTHK, K, K)
    first = 0
    for wave, kind, t in R.WAVES:
        e.dispersion_run(wave, kind, t, False, 0, first)
        first += len(t)
    return e.dispersion_fetch(0, K, False, 0)


def case(e, model_name, nz):
    """test_gpu_columns.py's case with weights of the size of 1 / sigma: (depz, model, obs, wt, parameters)"""
    depz = R.depths(nz)
    vel = (R.smooth_model if model_name == "smooth" else R.edge_model)(NX, NY, nz)
    rng = np.random.default_rng(7 + nz)
    wt = ((0.5 + rng.random((K, NCOL))) / SIGMA).astype(F)
    wt[rng.random((K, NCOL)) < 0.1] = 0.0
    wt[:, CENTRE] = 0.0                                                          # the centre column: no datum
    pv0 = curves_of(e, vel, depz)
    par = dict(PAR)
    if model_name == "smooth":
        obs = (pv0 * (1.0 + 0.02 * rng.standard_normal((K, NCOL)))).astype(F)
    else:
        obs = (2.5 + 1.5 * rng.random((K, NCOL))).astype(F)
        par.update(temperature=2000.0, spread=0.2, step=0.2)                    # far from the data: a hot chain still accepts and rejects
        inner = pv0[:, ~RING]
        assert (inner == 0).any() and (inner > 0).any(), "the edge model should lose some roots inside the ring at these periods"
    return depz, vel, obs, wt, par


def begin(e, vel, depz, obs, wt, C, par, seed, burn):
    e.columns_sample_begin(vel, depz, R.MINTHK, PLAN, obs, wt, C, par["smooth"], par["step"], par["spread"], par["width"], par["temperature"], par["minvel"],
                           par["maxvel"], seed, burn)


def host(h, vel, obs, wt, C, par, seed, burn):
    nz = vel.shape[0]
    return S.Stage(h, NX, NY, vel.reshape(nz, NCOL), obs, wt, C, par["smooth"], par["step"], par["spread"], par["width"], par["temperature"], par["minvel"],
                   par["maxvel"], seed, burn)


def maps_of(e, C):
    return e.dispersion_fetch(0, C * K, False, 0).reshape(C, K, NCOL)


def assert_state(dev, hs, what):
    want = hs.state()
    for name in S.STATE:
        assert same_bits(dev[name], want[name]), "%s: %s differs from the host's (%d of %d)" % (what, name, int((dev[name] != want[name]).sum()), want[name].size)


def assert_fetch(res, hs):
    nodes, cols, counts = hs.finish()
    for q, name in enumerate(("mean", "var", "W", "B", "best")):
        assert same_bits(res[name], nodes[q]), name
    for q, name in enumerate(("phi_start", "best_energy", "mean_phi")):
        assert same_bits(res[name], cols[q]), name
    for q, name in enumerate(("nused", "flag", "accepted", "rejected", "out_of_box", "no_root", "reseeded", "nkept")):
        assert same_bits(res[name], counts[q]), name


@pytest.mark.parametrize("C", [3, 27])
@pytest.mark.parametrize("nz", [2, 3, 8])
@pytest.mark.parametrize("model_name", ["smooth", "edge"])
def test_replay_bit_for_bit(eng, h, model_name, nz, C):
    """(a): the set-up and six sweeps of run(1), burn 2; after each the host proposes from the previous state and accepts from the device's
    fetched curves, and every array of the state is the device's; the final fetch is the host's finish.  25 * 27 threads fill no whole
    wavefront."""
    depz, vel, obs, wt, par = case(eng, model_name, nz)
    seed, burn = 2 ** 35 + 11 * nz + C, 2
    begin(eng, vel, depz, obs, wt, C, par, seed, burn)
    hs = host(h, vel, obs, wt, C, par, seed, burn)
    hs.setup_models()
    hs.setup_state(maps_of(eng, C))
    assert_state(eng.columns_sample_state(), hs, "set-up")
    marks = set()
    for sweep in range(1, 7):
        hs.propose()
        proposed = (hs.a["pnode"].copy(), hs.a["pold"].copy(), hs.a["pmark"].copy())
        eng.columns_sample_run(1)
        dev = eng.columns_sample_state()
        assert same_bits(dev["pnode"], proposed[0]) and same_bits(dev["pold"], proposed[1]), "sweep %d: the proposal differs from the host's" % sweep
        assert ((dev["pmark"] == S.OUT_OF_BOX) == (proposed[2] == S.OUT_OF_BOX)).all() and ((dev["pmark"] == S.IDLE) == (proposed[2] == S.IDLE)).all()
        hs.accept(maps_of(eng, C))
        assert_state(dev, hs, "sweep %d" % sweep)
        marks |= set(np.unique(dev["pmark"]).tolist())
    assert {S.IDLE, S.ACCEPTED} <= marks and (S.REJECTED in marks or S.NO_ROOT in marks or S.OUT_OF_BOX in marks)
    res = eng.columns_sample_fetch()
    assert_fetch(res, hs)
    assert (res["nkept"][~RING & (res["flag"] == 0)] == 4).all() and res["flag"][CENTRE] == 2


def test_one_call_equals_seven(eng):
    """(b): run(7) against seven run(1), burn 3 inside the run: state and fetch bit for bit"""
    depz, vel, obs, wt, par = case(eng, "smooth", 8)
    out = []
    for calls in ((7,), (1,) * 7):
        begin(eng, vel, depz, obs, wt, 5, par, 99, 3)
        for n in calls:
            eng.columns_sample_run(n)
        out.append((eng.columns_sample_state(), eng.columns_sample_fetch()))
    for part in (0, 1):
        for name in out[0][part]:
            assert same_bits(out[0][part][name], out[1][part][name]), name
    assert (out[0][1]["nkept"][~RING & (out[0][1]["flag"] == 0)] == 4).all() and out[0][0]["counters"][0].sum() > 0


def test_a_chain_sees_its_own_model(eng, h):
    """(c): the maps of chain q after a sweep are those of the chain's proposed model run alone through dsa_dispersion_begin -- the model
    store (depth, chain, column) and the map store (chain, map, column) are the ones the kernels and the stage agree on.  The proposed
    models are the host's, whose proposal the device's equals (node and old value here, everything in (a))."""
    nz, C = 8, 3
    depz, vel, obs, wt, par = case(eng, "smooth", nz)
    begin(eng, vel, depz, obs, wt, C, par, 5, 0)
    hs = host(h, vel, obs, wt, C, par, 5, 0)
    hs.setup_models()
    start_models = hs.a["models"].copy()
    hs.setup_state(maps_of(eng, C))
    hs.propose()
    proposed = hs.a["models"].copy()
    eng.columns_sample_run(1)
    dev = eng.columns_sample_state()
    assert same_bits(dev["pnode"], hs.a["pnode"]) and same_bits(dev["pold"], hs.a["pold"])
    accepted = dev["pmark"] == S.ACCEPTED
    assert accepted.any() and same_bits(dev["models"].transpose(1, 2, 0)[accepted], proposed.transpose(1, 2, 0)[accepted])
    got = maps_of(eng, C)
    assert not same_bits(proposed[:, 1], proposed[:, 2]) and not same_bits(proposed, start_models)
    for q in (1, 2):
        alone = curves_of(eng, proposed[:, q].reshape(nz, NY, NX), depz)
        assert same_bits(alone, got[q]), "chain %d" % q


def test_what_stays(eng):
    """(d): the ring in every chain, the bottom depth, the column whose weights are all 0 (flag 2); nothing is NaN, every node stays inside
    its box, accepted + rejected = sweeps; one chain works"""
    nz = 8
    depz, vel, obs, wt, par = case(eng, "smooth", nz)
    par = dict(par, width=0.08, step=0.1)                                        # a narrow box that the proposals often leave
    before = vel.reshape(nz, NCOL)
    for C in (4, 1):
        begin(eng, vel, depz, obs, wt, C, par, 3, 5)
        eng.columns_sample_run(20)
        st, res = eng.columns_sample_state(), eng.columns_sample_fetch()
        m = st["models"]
        for q in range(C):
            assert same_bits(m[:, q][:, RING], before[:, RING]) and same_bits(m[nz - 1, q], before[nz - 1]) and same_bits(m[:, q, CENTRE], before[:, CENTRE])
        lo = np.maximum(F(par["minvel"]), before[:nz - 1] - F(par["width"])); hi = np.minimum(F(par["maxvel"]), before[:nz - 1] + F(par["width"]))
        assert (m[:nz - 1] >= lo[:, None]).all() and (m[:nz - 1] <= hi[:, None]).all()
        assert all(np.isfinite(a).all() for a in st.values()) and all(np.isfinite(a).all() for a in res.values())
        moving = ~RING & (res["flag"] == 0)
        assert res["flag"][CENTRE] == 2 and res["nused"][CENTRE] == 0 and moving.sum() == 8 and not res["flag"][RING].any()
        total = st["counters"][0] + st["counters"][1]
        assert (total[:, moving] == 20).all() and not total[:, ~moving].any() and (st["counters"][2] + st["counters"][3] <= st["counters"][1]).all()
        assert st["counters"][2].sum() > 0 and st["counters"][0].sum() > 0
        assert (res["accepted"] + res["rejected"] == 20 * C * moving).all() and (res["nkept"] == 15 * moving).all()
        assert (res["var"][:, moving] >= 0).all() and not res["mean"][:, ~moving].any()
        used = ((wt > 0) & (obs > 0)).sum(axis=0)
        assert (res["nused"][~RING] == used[~RING]).all()
        if C == 1:
            assert not res["B"].any()
        assert same_bits(eng.dispersion_fetch(K * (C - 1), K, False, 0), maps_of(eng, C)[C - 1])      # dsa_dispersion_fetch works, global maps


def test_the_chains_fit_the_data(eng):
    """(e): nz = 8, 16 chains, 400 sweeps, burn 200, step 0.05, spread 0.05, sigma 0.02, smooth 10, a wide box; the observations are the
    device's own curves of smooth_model in fp32, the start is perturbed.  Over the interior columns the mean kept phi is below a quarter of
    phi at the start (the CPU prototype on the oracle's dispersion: 7 %).  No recovery of the truth in model space is asserted: the
    prototype's posterior mean is no nearer the truth than the start, which is the feature's point."""
    nz, C, sweeps, burn = 8, 16, 400, 200
    depz = R.depths(nz)
    truth = R.smooth_model(NX, NY, nz)
    obs = curves_of(eng, truth, depz).astype(F)
    assert (obs[:, ~RING] > 0).all()
    start = R.perturbed(truth)
    wt = np.full((K, NCOL), 1.0 / SIGMA, F)
    eng.columns_sample_begin(start, depz, R.MINTHK, PLAN, obs, wt, C, 10.0, 0.05, 0.05, 5.0, 1.0, R.MINVEL, R.MAXVEL, 20261020, burn)
    eng.columns_sample_run(sweeps)
    res = eng.columns_sample_fetch()
    inner = ~RING
    assert (res["flag"][inner] == 0).all() and (res["nkept"][inner] == sweeps - burn).all() and (res["nused"][inner] == K).all()
    phi0, phi1 = float(res["phi_start"][inner].mean()), float(res["mean_phi"][inner].mean())
    rms = lambda m: float(np.sqrt(((m[:, inner] - truth.reshape(nz, NCOL)[:nz - 1][:, inner]) ** 2).mean()))
    rhat = depth.sample_rhat(res["W"], res["B"], res["nkept"][None])[:, inner]
    print("phi per column: %.2f at the start, %.2f on average over the kept sweeps (%.1f %%); accepted %.1f %%; rms to the truth: start %.4f, posterior mean %.4f km/s; "
          "posterior sd median %.4f km/s; R-hat median %.3f, worst %.3f" %
          (phi0, phi1, 100 * phi1 / phi0, 100.0 * res["accepted"].sum() / (res["accepted"].sum() + res["rejected"].sum()), rms(start.reshape(nz, NCOL)[:nz - 1]),
           rms(res["mean"]), float(np.median(depth.sample_sd(res["var"])[:, inner])), float(np.median(rhat)), float(rhat.max())))
    assert phi1 < 0.25 * phi0


def test_refusals(eng):
    """(f): every refusal of begin is DSA_ERR_ARGUMENT, found before the device is touched -- an open stage stays as it was; run, fetch and
    state without a stage, and the column steps, the resolution and dsa_dispersion_get_model on an open one (one chain too), are
    DSA_ERR_STATE; the engine is usable after each"""
    nz = 3
    depz, vel, obs, wt, par = case(eng, "smooth", nz)
    eng.dispersion_begin(vel, depz, R.MINTHK, K, K)                              # a plain stage: no sample stage is open
    for call in (lambda: eng.columns_sample_run(1), eng.columns_sample_fetch, eng.columns_sample_state):
        with pytest.raises(EngineError) as exc:
            call()
        assert exc.value.code == DSA_ERR_STATE
    begin(eng, vel, depz, obs, wt, 2, par, 1, 0)
    eng.columns_sample_run(2)
    kept = eng.columns_sample_state()
    codes = set()

    def refused(match, vel=vel, obs=obs, wt=wt, C=2, plan=PLAN, burn=0, **over):
        p = dict(par, **over)
        with pytest.raises(EngineError, match=match) as exc:
            eng.columns_sample_begin(vel, depz, R.MINTHK, plan, obs, wt, C, p["smooth"], p["step"], p["spread"], p["width"], p["temperature"], p["minvel"], p["maxvel"], 1, burn)
        codes.add(exc.value.code)

    refused("nchains", C=0)
    refused("index range", C=2 ** 31 // NCOL + 1)
    refused("no interior", vel=vel[:, :2], obs=obs.reshape(K, NY, NX)[:, :2].reshape(K, -1), wt=None)
    for bad in (np.nan, np.inf):
        o = obs.copy(); o[3, 7] = bad
        refused("obs", obs=o)
    for bad in (-1.0, np.nan, np.inf):
        w = wt.copy(); w[5, 7] = bad
        refused("wt", wt=w)
    for name, bads in (("step", (0.0, -1.0, np.nan)), ("spread", (-0.1, np.inf)), ("width", (0.0, np.nan)), ("temperature", (0.0, -2.0)), ("smooth", (-0.5, np.nan))):
        for bad in bads:
            refused(name, **{name: bad})
    refused("minvel", minvel=4.0, maxvel=3.0)
    refused("burn", burn=-1)
    refused("add up", plan=PLAN[:3])
    refused("add up", plan=PLAN + PLAN[:1])
    refused("plan", plan=[(3, 0, PLAN[0][2])] + PLAN[1:])
    assert codes == {DSA_ERR_ARGUMENT}
    now = eng.columns_sample_state()
    for name in kept:
        assert same_bits(kept[name], now[name]), name                              # the open stage is as it was
    for C in (2, 1):
        begin(eng, vel, depz, obs, wt, C, par, 1, 0)
        for call in (lambda: eng.columns_step(obs, wt, *R_ARGS), lambda: eng.columns_resolution(obs, wt, R.SMOOTH, R.DAMP),
                     lambda: eng.columns_step_lateral(obs, wt, R.SMOOTH, R.DAMP, 0.5, R.DVMAX, R.MINVEL, R.MAXVEL), eng.dispersion_get_model):
            with pytest.raises(EngineError, match="sample stage") as exc:
                call()
            assert exc.value.code == DSA_ERR_STATE
        eng.columns_sample_run(1)                                                  # usable after the refusals
        assert eng._L.dsa_dispersion_failure(eng._h, 0, None, None, None, None) == DSA_ERR_STATE
        assert eng.dispersion_model_failures(C).shape == (C,)
    eng.dispersion_begin(vel, depz, R.MINTHK, K, K)                              # a new begin ends the sample stage
    with pytest.raises(EngineError) as exc:
        eng.columns_sample_run(1)
    assert exc.value.code == DSA_ERR_STATE
    assert same_bits(eng.dispersion_get_model(), vel)
    first = 0
    for wave, kind, t in R.WAVES:
        eng.dispersion_run(wave, kind, t, True, first, first)
        first += len(t)
    assert (eng.columns_step(obs, wt, *R_ARGS)["flag"][~RING & (wt > 0).any(axis=0)] == 0).all()


R_ARGS = (R.SMOOTH, R.DAMP, R.DVMAX, R.MINVEL, R.MAXVEL)
