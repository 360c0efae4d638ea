"""dsa_columns_sample_radial_* (csrc/column_kernels.hip: k_sample_radial_*) on the device against the CPU build of the
same header (tests/hostcheck_column_sample_radial.cpp through column_sample_radial_ref), bit for bit: one thread per (column, chain) runs
column_sample_radial.h's sequential fp64 chains under -ffp-contract=off, without libm, a square root or an atomic, so the mapping cannot
show.  The host replays every sweep from the curves fetched from the device, so the dispersion stage's own arithmetic is not under test
here -- except in (c), which checks that a chain's Rayleigh maps are those of its Vsv and its Love maps those of its Vsh.

Grid 5 x 5 (9 interior columns), columns_ref.WAVES (K = 12: Rayleigh and Love, phase and group), nz = 2, 3, 8, test_gpu_dispersion.py's
smooth_model and edge_model as Vsv with Vsh = 1.03 Vsv at the odd depths, weights with some zeros and the centre column all zero.

(e), measured on the MI355X and on the CPU twin: see DESIGN.md section 37."""
import ctypes
import re

import numpy as np
import pytest

import column_sample_radial_ref as S
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
LOVE = np.concatenate([[wave == 1] * len(t) for wave, _, t in R.WAVES])
SIGMA = 0.02
PAR = dict(smooth=3.0, aniso=2.0, step=0.05, spread=0.05, width=0.4, temperature=1.0, minvel=R.MINVEL, maxvel=R.MAXVEL)
R_ARGS = (R.SMOOTH, R.DAMP, R.DVMAX, R.MINVEL, R.MAXVEL)


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


def vsh_of(vsv):
    """Vsv scaled by 1.03 at the odd depths"""
    vsh = vsv.copy()
    vsh[1::2] = (vsh[1::2] * F(1.03)).astype(F)
    return vsh


def curves_of(e, vsv, vsh, depz):
    """the device's own curves of one pair of models through dsa_dispersion_begin_radial, (K, ncol)"""
    e.dispersion_begin_radial(vsv, vsh, depz, R.MINTHK, K, K)
    first = 0
    for wave, kind, t in R.WAVES:
        e.dispersion_run(wave, kind, t, False, 0, first)
        first += len(t)
    return e.dispersion_fetch(0, K, False, 0)


_CASES = {}


def case(e, model_name, nz):
    """(depz, vsv, vsh, obs, wt, parameters), computed once per (model, nz) and left unchanged"""
    if (model_name, nz) in _CASES:
        return _CASES[model_name, nz]
    depz = R.depths(nz)
    vsv = (R.smooth_model if model_name == "smooth" else R.edge_model)(NX, NY, nz)
    vsh = vsh_of(vsv)
    rng = np.random.default_rng(7 + nz)
    wt = ((0.5 + rng.random((K, NCOL))) / SIGMA).astype(F)
    wt[rng.random((K, NCOL)) < 0.1] = 0.0
    wt[:, CENTRE] = 0.0                                                          # the centre column: no datum
    pv0 = curves_of(e, vsv, vsh, depz)
    par = dict(PAR)
    if model_name == "smooth":
        obs = (pv0 * (1.0 + 0.02 * rng.standard_normal((K, NCOL)))).astype(F)
    else:
        obs = (2.5 + 1.5 * rng.random((K, NCOL))).astype(F)
        par.update(temperature=2000.0, spread=0.2, step=0.2)                    # far from the data: a hot chain still accepts and rejects
        inner = pv0[:, ~RING]
        assert (inner > 0).any()
    for a in (depz, vsv, vsh, obs, wt):
        a.setflags(write=False)
    _CASES[model_name, nz] = (depz, vsv, vsh, obs, wt, par)
    return _CASES[model_name, nz]


def begin(e, vsv, vsh, depz, obs, wt, C, par, seed, burn, pairs=True):
    e.columns_sample_radial_begin(vsv, vsh, depz, R.MINTHK, PLAN, obs, wt, C, par["smooth"], par["aniso"], par["step"], par["spread"], par["width"],
                                  par["temperature"], par["minvel"], par["maxvel"], seed, burn, pairs)


def host(h, vsv, vsh, obs, wt, C, par, seed, burn, pairs=True):
    nz = vsv.shape[0]
    return S.Stage(h, NX, NY, vsv.reshape(nz, NCOL), vsh.reshape(nz, NCOL), obs, wt, LOVE, C, par["smooth"], par["aniso"], par["step"], par["spread"], par["width"],
                   par["temperature"], par["minvel"], par["maxvel"], seed, burn, pairs)


def maps_of(e, C):
    return e.dispersion_fetch(0, C * K, False, 0).reshape(C, K, NCOL)


def assert_state(dev, hs, what):
    want = hs.state()
    for name in S.STATE:
        assert same_bits(dev[name], want[name]), "%s: %s differs from the host's (%d of %d)" % (what, name, int((dev[name] != want[name]).sum()), want[name].size)


def assert_fetch(res, hs):
    want = hs.finish()
    assert set(res) == set(want)
    for name in want:
        assert same_bits(res[name], want[name]), name


@pytest.mark.parametrize("nz,C,pairs", [(2, 3, True), (2, 27, True), (3, 3, True), (3, 27, True), (8, 3, True), (8, 27, True), (3, 3, False)])
@pytest.mark.parametrize("model_name", ["smooth", "edge"])
def test_replay_bit_for_bit(eng, h, model_name, nz, C, pairs):
    """(a): the set-up and six sweeps of run(1), burn 2; after each the host proposes from the previous state and accepts from the device's
    fetched curves, and every array of the state is the device's; the final fetch is the host's finish.  25 * 27 threads fill no whole
    wavefront."""
    depz, vsv, vsh, obs, wt, par = case(eng, model_name, nz)
    seed, burn = 2 ** 35 + 11 * nz + C, 2
    begin(eng, vsv, vsh, depz, obs, wt, C, par, seed, burn, pairs)
    hs = host(h, vsv, vsh, obs, wt, C, par, seed, burn, pairs)
    hs.setup_models()
    hs.setup_state(maps_of(eng, C))
    assert_state(eng.columns_sample_radial_state(), hs, "set-up")
    marks = set()
    for sweep in range(1, 7):
        hs.propose()
        proposed = {n: hs.a[n].copy() for n in ("pnode", "pold_v", "pold_h", "pmark", "kinds")}
        eng.columns_sample_radial_run(1)
        dev = eng.columns_sample_radial_state()
        for n in ("pnode", "pold_v", "pold_h"):
            assert same_bits(dev[n], proposed[n]), "sweep %d: the proposal differs from the host's (%s)" % (sweep, n)
        assert same_bits(dev["kinds"][:3], proposed["kinds"][:3])
        assert ((dev["pmark"] == S.OUT_OF_BOX) == (proposed["pmark"] == S.OUT_OF_BOX)).all() and ((dev["pmark"] == S.IDLE) == (proposed["pmark"] == S.IDLE)).all()
        hs.accept(maps_of(eng, C))
        assert_state(dev, hs, "sweep %d" % sweep)
        marks |= set(np.unique(dev["pmark"]).tolist())
    assert {S.IDLE, S.ACCEPTED} <= marks and (S.REJECTED in marks or S.NO_ROOT in marks or S.OUT_OF_BOX in marks)
    res = eng.columns_sample_radial_fetch()
    assert_fetch(res, hs)
    assert (res["nkept"][~RING & (res["flag"] == 0)] == 4).all() and res["flag"][CENTRE] == 2
    assert (res["proposed_pair"].sum() > 0) == pairs


def test_one_call_equals_seven(eng):
    """(b): run(7) against seven run(1), burn 3 inside the run: state and fetch bit for bit"""
    depz, vsv, vsh, obs, wt, par = case(eng, "smooth", 8)
    out = []
    for calls in ((7,), (1,) * 7):
        begin(eng, vsv, vsh, depz, obs, wt, 5, par, 99, 3)
        for n in calls:
            eng.columns_sample_radial_run(n)
        out.append((eng.columns_sample_radial_state(), eng.columns_sample_radial_fetch()))
    for part in (0, 1):
        for name in out[0][part]:
            assert same_bits(out[0][part][name], out[1][part][name]), name
    assert (out[0][1]["nkept"][~RING & (out[0][1]["flag"] == 0)] == 4).all() and out[0][0]["counters"][0].sum() > 0


def test_a_chain_sees_its_own_two_models(eng, h):
    """(c): after a sweep the Rayleigh maps of chain q are those of the chain's proposed Vsv and its Love maps those of its proposed Vsh, the
    pair run alone through dsa_dispersion_begin_radial.  The chains used differ between Vsv and Vsh at every depth of every interior column
    and the swapped pair gives other curves, so a swapped store cannot pass.  The proposed models are the host's, whose proposal the device's
    equals (here node and old values, everything in (a))."""
    nz, C = 8, 3
    depz, vsv, vsh, obs, wt, par = case(eng, "smooth", nz)
    begin(eng, vsv, vsh, depz, obs, wt, C, par, 5, 0)
    hs = host(h, vsv, vsh, obs, wt, C, par, 5, 0)
    hs.setup_models()
    hs.setup_state(maps_of(eng, C))
    hs.propose()
    prop_v, prop_h = hs.a["vsv"].copy(), hs.a["vsh"].copy()
    eng.columns_sample_radial_run(1)
    dev = eng.columns_sample_radial_state()
    assert same_bits(dev["pnode"], hs.a["pnode"]) and same_bits(dev["pold_v"], hs.a["pold_v"]) and same_bits(dev["pold_h"], hs.a["pold_h"])
    accepted = dev["pmark"] == S.ACCEPTED
    assert accepted.any()
    assert same_bits(dev["vsv"].transpose(1, 2, 0)[accepted], prop_v.transpose(1, 2, 0)[accepted]) and same_bits(dev["vsh"].transpose(1, 2, 0)[accepted], prop_h.transpose(1, 2, 0)[accepted])
    got = maps_of(eng, C)
    moving = ~RING & (np.arange(NCOL) != CENTRE)
    for q in (1, 2):
        assert (prop_v[:, q][:, moving] != prop_h[:, q][:, moving]).all() and (prop_v[1::2, q] != prop_h[1::2, q]).all()
        pv, ph = prop_v[:, q].reshape(nz, NY, NX), prop_h[:, q].reshape(nz, NY, NX)
        alone = curves_of(eng, pv, ph, depz)
        assert same_bits(alone, got[q]), "chain %d" % q
        swapped = curves_of(eng, ph, pv, depz)
        assert (swapped[~LOVE][:, ~RING] != got[q][~LOVE][:, ~RING]).any() and (swapped[LOVE][:, ~RING] != got[q][LOVE][:, ~RING]).any()


def test_what_stays(eng):
    """(d): the ring in every chain, the bottom depth of both models, the column whose weights are all 0 (flag 2); nothing is NaN, every node
    stays inside its box, accepted + rejected = sweeps, the kinds' proposals add up to the sweeps of a moving chain; one chain works"""
    nz = 8
    depz, vsv, vsh, obs, wt, par = case(eng, "smooth", nz)
    par = dict(par, width=0.08, step=0.1)                                        # a narrow box that the proposals often leave
    starts = dict(vsv=vsv.reshape(nz, NCOL), vsh=vsh.reshape(nz, NCOL))
    for C in (4, 1):
        begin(eng, vsv, vsh, depz, obs, wt, C, par, 3, 5)
        eng.columns_sample_radial_run(20)
        st, res = eng.columns_sample_radial_state(), eng.columns_sample_radial_fetch()
        for name, before in starts.items():
            m = st[name]
            for q in range(C):
                assert same_bits(m[:, q][:, RING], before[:, RING]) and same_bits(m[nz - 1, q], before[nz - 1]) and same_bits(m[:, q, CENTRE], before[:, CENTRE]), name
            lo = np.maximum(F(par["minvel"]), before[:nz - 1] - F(par["width"])); hi = np.minimum(F(par["maxvel"]), before[:nz - 1] + F(par["width"]))
            assert (m[:nz - 1] >= lo[:, None]).all() and (m[:nz - 1] <= hi[:, None]).all(), name
        assert all(np.isfinite(a).all() for a in st.values()) and all(np.isfinite(a).all() for a in res.values())
        moving = ~RING & (res["flag"] == 0)
        assert res["flag"][CENTRE] == 2 and res["nused_r"][CENTRE] == 0 and res["nused_l"][CENTRE] == 0 and moving.sum() == 8 and not res["flag"][RING].any()
        total = st["counters"][0] + st["counters"][1]
        assert (total[:, moving] == 20).all() and not total[:, ~moving].any() and (st["counters"][2] + st["counters"][3] <= st["counters"][1]).all()
        assert (st["kinds"][:3].sum(axis=0)[:, moving] == 20).all() and not st["kinds"][:, :, ~moving].any()
        assert (st["kinds"][3:].sum(axis=0) == st["counters"][0]).all() and (st["kinds"][3:] <= st["kinds"][:3]).all()
        assert st["counters"][2].sum() > 0 and st["counters"][0].sum() > 0
        assert (res["accepted"] + res["rejected"] == 20 * C * moving).all() and (res["nkept"] == 15 * moving).all()
        assert (res["proposed_v"] + res["proposed_h"] + res["proposed_pair"] == 20 * C * moving).all()
        for t in ("v", "h", "xi"):
            # a node that never moved has the variance s2 / n - (s1 / n)^2 of 15 equal values below 1: 0 up to the rounding of the two terms,
            # each within 15 ulp(1) = 3.4e-15 -- which sample_sd takes as 0
            assert (res["var_" + t][:, moving] >= -1e-14).all() and (res["var_" + t][:, moving] > 0).any() and not res["mean_" + t][:, ~moving].any()
        assert ((res["p_pos"] >= 0) & (res["p_pos"] <= 1)).all()
        used = (wt > 0) & (obs > 0)
        assert (res["nused_r"][~RING] == used[~LOVE].sum(axis=0)[~RING]).all() and (res["nused_l"][~RING] == used[LOVE].sum(axis=0)[~RING]).all()
        if C == 1:
            assert not res["B_v"].any() and not res["B_h"].any() and not res["B_xi"].any()
        assert same_bits(eng.dispersion_fetch(K * (C - 1), K, False, 0), maps_of(eng, C)[C - 1])      # dsa_dispersion_fetch works, global maps


def test_the_chains_fit_the_data(eng):
    """(e): nz = 8, 16 chains, 400 sweeps, burn 200, step 0.05, spread 0.05, sigma 0.02, smooth 10, aniso 10, a wide box, pairs on; the
    observations are the device's own curves of the true pair (smooth_model and its Vsh) in fp32, the start is perturbed on both.  Over the
    interior columns the mean kept phi is below a quarter of phi at the start (the CPU twin on the oracle's dispersion, same seed: see
    DESIGN.md section 37)."""
    nz, C, sweeps, burn = 8, 16, 400, 200
    depz = R.depths(nz)
    truth_v = R.smooth_model(NX, NY, nz)
    truth_h = vsh_of(truth_v)
    obs = curves_of(eng, truth_v, truth_h, depz).astype(F)
    assert (obs[:, ~RING] > 0).all()
    start_v, start_h = R.perturbed(truth_v), R.perturbed(truth_h)
    wt = np.full((K, NCOL), 1.0 / SIGMA, F)
    eng.columns_sample_radial_begin(start_v, start_h, depz, R.MINTHK, PLAN, obs, wt, C, 10.0, 10.0, 0.05, 0.05, 5.0, 1.0, R.MINVEL, R.MAXVEL, 20261021, burn, True)
    eng.columns_sample_radial_run(sweeps)
    res = eng.columns_sample_radial_fetch()
    inner = ~RING
    assert (res["flag"][inner] == 0).all() and (res["nkept"][inner] == sweeps - burn).all() and (res["nused_r"][inner] + res["nused_l"][inner] == K).all()
    phi0, phi1 = float(res["phi_start"][inner].mean()), float(res["mean_phi"][inner].mean())
    rhat = {t: depth.sample_rhat(res["W_" + t], res["B_" + t], res["nkept"][None])[:, inner] for t in ("v", "h", "xi")}
    acc = [res["accepted_" + k].sum() / max(res["proposed_" + k].sum(), 1) for k in ("v", "h", "pair")]
    print("phi per column: %.2f at the start, %.2f on average over the kept sweeps (%.1f %%); accepted Vsv %.1f %% Vsh %.1f %% pair %.1f %%; R-hat median / worst: "
          "Vsv %.3f / %.3f, Vsh %.3f / %.3f, xi %.3f / %.3f; sd of xi median %.4f" %
          (phi0, phi1, 100 * phi1 / phi0, 100 * acc[0], 100 * acc[1], 100 * acc[2], np.median(rhat["v"]), rhat["v"].max(), np.median(rhat["h"]), rhat["h"].max(),
           np.median(rhat["xi"]), rhat["xi"].max(), float(np.median(depth.sample_sd(res["var_xi"])[:, inner]))))
    assert phi1 < 0.25 * phi0


def test_refusals_and_stage_rules(eng):
    """(f): every refusal of begin is DSA_ERR_ARGUMENT, found before the device is touched -- an open stage stays as it was; the isotropic
    sample entries on a radial stage, the radial entries on an isotropic stage or without one, and what a sample stage refuses are
    DSA_ERR_STATE; the engine is usable after each; after the stage a dsa_dispersion_begin and an isotropic sample stage give a fresh
    engine's bits"""
    nz = 3
    depz, vsv, vsh, obs, wt, par = case(eng, "smooth", nz)
    iso = lambda e, C=2: e.columns_sample_begin(vsv, depz, R.MINTHK, PLAN, obs, wt, C, par["smooth"], par["step"], par["spread"], par["width"], par["temperature"],
                                                par["minvel"], par["maxvel"], 1, 0)
    radial_calls = (lambda: eng.columns_sample_radial_run(1), eng.columns_sample_radial_fetch, eng.columns_sample_radial_state)

    def state_error(call, match=None):
        with pytest.raises(EngineError, match=match) as exc:
            call()
        assert exc.value.code == DSA_ERR_STATE

    eng.dispersion_begin(vsv, depz, R.MINTHK, K, K)                              # a plain stage: no sample stage is open
    for call in radial_calls:
        state_error(call)
    iso(eng)                                                                     # an isotropic sample stage is no radial one
    for call in radial_calls:
        state_error(call)
    eng.columns_sample_run(1)                                                    # ... and is usable after the refusals
    begin(eng, vsv, vsh, depz, obs, wt, 2, par, 1, 0)
    eng.columns_sample_radial_run(2)
    kept = eng.columns_sample_radial_state()
    codes = set()

    def refused(match, vsv=vsv, vsh=vsh, obs=obs, wt=wt, C=2, plan=PLAN, burn=0, pairs=1, **over):
        p = dict(par, **over)
        with pytest.raises(EngineError, match=match) as exc:
            eng.columns_sample_radial_begin(vsv, vsh, depz, R.MINTHK, plan, obs, wt, C, p["smooth"], p["aniso"], p["step"], p["spread"], p["width"], p["temperature"],
                                            p["minvel"], p["maxvel"], 1, burn, pairs)
        codes.add(exc.value.code)

    refused("nchains", C=0)
    refused("index range", C=2 ** 31 // NCOL + 1)
    refused("no interior", vsv=vsv[:, :2], vsh=vsh[:, :2], obs=obs.reshape(K, NY, NX)[:, :2].reshape(K, -1), wt=None)
    refused("null model", vsh=None)
    for bad in (np.nan, np.inf):
        o = obs.copy(); o[3, 7] = bad
        refused("obs", obs=o)
        m = vsh.copy(); m[1, 2, 2] = bad
        refused("not finite", vsh=m)
        m = vsv.copy(); m[1, 2, 2] = bad
        refused("not finite", vsv=m)
    for bad in (-1.0, np.nan, np.inf):
        w = wt.copy(); w[5, 7] = bad
        refused("wt", wt=w)
    for name, bads in (("step", (0.0, -1.0, np.nan)), ("spread", (-0.1, np.inf)), ("width", (0.0, np.nan)), ("temperature", (0.0, -2.0)), ("smooth", (-0.5, np.nan)),
                       ("aniso", (-0.5, np.nan, np.inf)), ("minvel", (0.0, -1.0, np.nan))):
        for bad in bads:
            refused(name, **{name: bad})
    refused("minvel", minvel=4.0, maxvel=3.0)
    refused("burn", burn=-1)
    refused("pairs", pairs=2)
    refused("pairs", pairs=-1)
    refused("add up", plan=PLAN[:3])
    refused("add up", plan=PLAN + PLAN[:1])
    refused("plan", plan=[(3, 0, PLAN[0][2])] + PLAN[1:])
    assert codes == {DSA_ERR_ARGUMENT}
    # the library's entry itself, for what the binding cannot pass: null pointers, and an nz, nmaps or nper that the arrays do not have (each is
    # refused before any array is read)
    plan_arrays = dict(iwave=np.array([r[0] for r in PLAN], np.int32), igr=np.array([r[1] for r in PLAN], np.int32), nper=np.array([len(r[2]) for r in PLAN], np.int32),
                       t=np.concatenate([r[2] for r in PLAN]).astype(np.float64))

    def raw(match, **over):
        a = dict(plan_arrays, nz=nz, vsv=vsv, depz=depz, minthk=R.MINTHK, nruns=len(PLAN), nmaps=K)
        a.update(over)
        ptr = lambda x: None if x is None else np.ascontiguousarray(x).ctypes.data_as(ctypes.c_void_p)
        rc = eng._L.dsa_columns_sample_radial_begin(eng._h, NX, NY, a["nz"], 2, ptr(a["vsv"]), ptr(vsh), ptr(a["depz"]), a["minthk"], a["nruns"], ptr(a["iwave"]), ptr(a["igr"]),
                                                    ptr(a["nper"]), ptr(a["t"]), a["nmaps"], ptr(obs), ptr(wt), par["smooth"], par["aniso"], par["step"], par["spread"],
                                                    par["width"], par["temperature"], par["minvel"], par["maxvel"], 1, 0, 1)
        assert rc == DSA_ERR_ARGUMENT and re.search(match, eng._L.dsa_error_string(eng._h).decode()), (match, rc)

    for bad in (1, 65):
        raw("nz=%d" % bad, nz=bad)
    raw("null model", vsv=None)
    raw("null model or depths", depz=None)
    for bad in (0.0, -1.0, float("nan")):
        raw("minthk", minthk=bad)
    for bad in (0, 61):
        raw("%d maps" % bad, nmaps=bad)
    raw("plan of the runs is missing", nruns=0)
    for name in ("iwave", "igr", "nper", "t"):
        raw("plan of the runs is missing", **{name: None})
    for bad in (0, 61):
        n = plan_arrays["nper"].copy(); n[1] = bad
        raw("run 1 of the plan", nper=n)
    for bad in (np.nan, np.inf):
        t = plan_arrays["t"].copy(); t[4] = bad
        raw("period 4 of the plan is not finite", t=t)
    now = eng.columns_sample_radial_state()
    for name in kept:
        assert same_bits(kept[name], now[name]), name                              # the open stage is as it was
    for C in (2, 1):
        begin(eng, vsv, vsh, depz, obs, wt, C, par, 1, 0)
        for call in (lambda: eng.columns_step(obs, wt, *R_ARGS), lambda: eng.columns_resolution(obs, wt, R.SMOOTH, R.DAMP),
                     lambda: eng.columns_step_radial(obs, wt, R.SMOOTH, R.DAMP, 0.2, R.DVMAX, R.MINVEL, R.MAXVEL),
                     lambda: eng.columns_resolution_radial(obs, wt, R.SMOOTH, R.DAMP, 0.2),
                     lambda: eng.columns_step_lateral(obs, wt, R.SMOOTH, R.DAMP, 0.5, R.DVMAX, R.MINVEL, R.MAXVEL), eng.dispersion_get_model,
                     eng.dispersion_get_model_radial, eng.kernels_from_dispersion_radial,
                     lambda: eng.update_radial(np.zeros(2 * (NX - 2) * (NY - 2) * (nz - 1), F), 0.1, R.MINVEL, R.MAXVEL)):
            state_error(call, "sample stage")
        # the isotropic sample entries, begin among them
        for call in (lambda: eng.columns_sample_run(1), eng.columns_sample_fetch, lambda: eng._check(eng._L.dsa_columns_sample_state(eng._h, *([None] * 14))),
                     lambda: eng.columns_sample_blocks(2, 1.0), lambda: eng._check(eng._L.dsa_columns_sample_block_state(eng._h, None, None)),
                     lambda: eng.columns_sample_marginals(8), lambda: eng._check(eng._L.dsa_columns_sample_marginals_fetch(eng._h, 0, None, None, None, None)),
                     lambda: eng._check(eng._L.dsa_columns_sample_marginals_state(eng._h, None, None)), lambda: eng.columns_sample_shape(obs, wt, R.SMOOTH, R.DAMP),
                     lambda: iso(eng)):
            state_error(call, "radial sample stage")
        eng.columns_sample_radial_run(1)                                           # usable after the refusals
        assert eng._L.dsa_dispersion_failure(eng._h, 0, None, None, None, None) == DSA_ERR_STATE
        assert eng.dispersion_model_failures(C).shape == (C,)
    # after the stage: a plain begin ends it, and an isotropic sample stage then has a fresh engine's bits
    eng.dispersion_begin(vsv, depz, R.MINTHK, K, K)
    for call in radial_calls:
        state_error(call)
    assert same_bits(eng.dispersion_get_model(), vsv)
    outs = []
    fresh = Engine(0)
    try:
        for e in (eng, fresh):
            iso(e, 3)
            e.columns_sample_run(4)
            outs.append((e.columns_sample_state(), e.columns_sample_fetch()))
    finally:
        fresh.close()
    for part in (0, 1):
        for name in outs[0][part]:
            assert same_bits(outs[0][part][name], outs[1][part][name]), name
    assert outs[0][0]["counters"][0].sum() > 0
    eng.dispersion_begin_radial(vsv, vsh, depz, R.MINTHK, K, K)                  # the radial step works again
    first = 0
    for wave, kind, t in R.WAVES:
        eng.dispersion_run(wave, kind, t, True, first, first)
        first += len(t)
    assert (eng.columns_step_radial(obs, wt, R.SMOOTH, R.DAMP, 0.2, R.DVMAX, R.MINVEL, R.MAXVEL)["flag"][~RING & (wt > 0).any(axis=0)] == 0).all()
