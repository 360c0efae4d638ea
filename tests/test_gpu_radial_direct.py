"""Radial anisotropy through the direct 3-D inversion on the device: dsa_kernels_from_dispersion_radial,
dsa_solve_rows_radial, dsa_iteration_system_radial_device, dsa_update_radial and the driver dsurftomo_amd.radial.

Everything is held against what the tree already had, bit for bit: the depth factors against dsa_set_depth_kernels with the fetched kernels
on either model (on a second engine given the same maps: dsa_set_depth_kernels replaces the resident Vsv model of a radial stage), the rows
against dsa_solve_rows with the Love units' columns moved, the system against the NumPy twin plus dsa_spmv_load on the host rows, the update
against dsa_dispersion_begin_radial on the twin's stepped models and against dsa_model_update, the block PSFs against dsa_lsmr_resolution.
The recoveries are conditions against SciPy's fp64 LSMR and against the isotropic loop.

Shapes: synth.boundary_case() at its defaults (12 x 11 x 5, periods of all four wave types); the rows over three launches need more than
128 traced rays (a launch takes at least 64), so that test has six sources per period; the system tests use section 19's
boundary_case(nx=10, ny=9, nz=4, ...) with kLg = 1 added."""
import ctypes as C
import os

import numpy as np
import pytest

import synth
from dsurftomo_amd import depth, io
from dsurftomo_amd import radial as RD
from dsurftomo_amd.analyses.common import LSMR_ARGS, _p, unknown_coords
from dsurftomo_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu
F = np.float32
ERR_ARGUMENT, ERR_STATE, ERR_CAPACITY = -2, -5, -6                      # include/dsurftomo_amd.h


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def model_of(c):
    """the case's model as the engine takes it: (nz, ny, nx) fp32"""
    return np.ascontiguousarray(np.asarray(c["vels"], F).transpose(2, 1, 0))


def above(vsv, factor=1.03):
    """Vsh = Vsv * factor above the bottom depth, equal at it"""
    vsh = np.array(vsv, F, copy=True)
    vsh[:-1] = (vsh[:-1] * F(factor)).astype(F)
    return vsh


def no_failures(e):
    """every curve has a root (dsa_dispersion_diagnostics count 0): no case below is a case about missing roots"""
    cnt = C.c_longlong(0); first = (C.c_int * 5)(); per = C.c_double(0.0)
    fn = e._L.dsa_dispersion_diagnostics
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert fn(e._h, C.byref(cnt), first, C.byref(per)) == 0
    assert cnt.value == 0, "dispersion curves without a root: %d, first %s" % (cnt.value, list(first))


def staged(c, vsv, vsh):
    """a fresh engine with a radial stage on (vsv, vsh), the runs, the maps, the radial depth factors and the plan.  Returns (engine, plan)."""
    e = Engine(0)
    u = RD.radial_plan(c)
    RD.begin(e, c, u, vsv, vsh)
    RD.stage(e, c, u)
    no_failures(e)
    return e, u


def plain_staged(c, vs):
    """the same on a plain stage holding one model, with dsa_kernels_from_dispersion"""
    e = Engine(0)
    u = RD.radial_plan(c)
    e.dispersion_begin(vs, c["depz"], c["minthk"], c["kmax"], u["nmaps"])
    plain_stage(e, c, u)
    return e, u


def plain_stage(e, c, u):
    for wave, kind, t, first in depth.slot_plan(c):
        e.dispersion_run(wave, kind, t, True, first, first)
    for wave, t, first in u["copies"]:
        e.dispersion_run(wave, 0, t, False, 0, first)
    e.maps_from_dispersion(c["goxd"], c["gozd"], c["dvxd"], c["dvzd"], 8)
    e.kernels_from_dispersion()
    e.plan(u["map_index"], u["scx"], u["scz"], u["nrec"], u["rcx"], u["rcz"], mode=u["mode"], sen_slot=u["sen_slot"], data_first=u["data_first"])


def capacity(c):
    return c["ndata"] * c["nparpi"] + 1


def same_rows(a, b):
    """(times, rw, iw, col) twice: bit for bit"""
    assert a[1].size == b[1].size > 0
    assert (bits(a[0]) == bits(b[0])).all() and (bits(a[1]) == bits(b[1])).all() and (a[2] == b[2]).all() and (a[3] == b[3]).all()


# ---- 1. depth factors ----

def test_depth_factors_are_each_slots_models():
    """Vsh = 1.03 Vsv: after kernels_from_dispersion_radial plain dsa_solve_rows gives, for the data of Rayleigh units, the entries of
    dsa_set_depth_kernels with the fetched kernels and vels = Vsv, and for the data of Love units those with vels = Vsh -- on a second
    engine given the same maps, since dsa_set_depth_kernels would replace the radial stage's resident Vsv"""
    c = synth.boundary_case()
    vsv = model_of(c); vsh = above(vsv)
    e, u = staged(c, vsv, vsh)
    try:
        cap = capacity(c)
        got = e.solve_rows(cap)
        pv = e.dispersion_fetch(0, u["nmaps"])
        _, svs, svp, srho = e.dispersion_fetch(0, c["kmax"], True, 0)
    finally:
        e.close()
    wave = u["wave"]
    assert (wave == 1).any() and (wave == 2).any() and got[1].size > 0
    e2 = Engine(0)
    try:
        e2.set_maps(c["nx"], c["ny"], c["goxd"], c["gozd"], c["dvxd"], c["dvzd"], pv, dicing=8)
        e2.plan(u["map_index"], u["scx"], u["scz"], u["nrec"], u["rcx"], u["rcz"], mode=u["mode"], sen_slot=u["sen_slot"], data_first=u["data_first"])
        for model, w in ((vsv, 2), (vsh, 1)):
            e2.set_depth_kernels(model, c["depz"], svs, svp, srho)
            want = e2.solve_rows(cap)
            assert (bits(want[0]) == bits(got[0])).all()
            a, b = wave[got[2] - 1] == w, wave[want[2] - 1] == w
            assert a.sum() == b.sum() > 0
            assert (bits(got[1][a]) == bits(want[1][b])).all() and (got[2][a] == want[2][b]).all() and (got[3][a] == want[3][b]).all()
            # ... and on the data of the other wave type this model's factors give other values: the test tells the models apart
            o, p = wave[got[2] - 1] != w, wave[want[2] - 1] != w
            assert o.sum() != p.sum() or not (bits(got[1][o]) == bits(want[1][p])).all()
    finally:
        e2.close()


def test_equal_models_give_the_plain_stages_rows():
    """Vsh = Vsv: the rows are those of a plain stage with dsa_kernels_from_dispersion, bit for bit"""
    c = synth.boundary_case()
    vs = model_of(c)
    e, u = staged(c, vs, vs)
    try:
        got = e.solve_rows(capacity(c))
    finally:
        e.close()
    p, _ = plain_staged(c, vs)
    try:
        no_failures(p)
        same_rows(got, p.solve_rows(capacity(c)))
    finally:
        p.close()


# ---- 2. rows ----

@pytest.mark.parametrize("lanes", [1, 4])
def test_radial_rows_are_the_plain_rows_with_love_columns_moved(lanes):
    """over three launches: solve_rows_radial == dsa_solve_rows on the same engine with + maxvp on the columns of Love units, in rw, iw,
    order, nar, times and statistics; with null arrays the same nar; the exact capacity, and one entry short of it"""
    c = synth.boundary_case(nsrc=6, nrcf=7)
    vsv = model_of(c)
    e, u = staged(c, vsv, above(vsv))
    try:
        cap, maxvp = capacity(c), c["nparpi"]
        e.set_option("ray_lanes", lanes)
        plain = e.solve_rows(cap)
        nrays = int(e.stats()["rays"])
        assert nrays > 128
        per_ray = (c["nx"] * c["ny"] + (c["nx"] - 2) * (c["ny"] - 2)) * 4 + 32
        e.set_option("ray_budget", -(-nrays // 3) * per_ray)
        plain = e.solve_rows(cap)
        st0 = e.stats()
        got = e.solve_rows_radial(cap)
        st1 = e.stats()
        assert st1["ray_launches"] == 3 and st1["rays"] == nrays
        love = u["wave"][plain[2] - 1] == 1
        assert 0 < love.sum() < love.size
        same_rows(got, (plain[0], plain[1], plain[2], plain[3] + maxvp * love))
        assert got[3].max() <= 2 * maxvp and got[3][love].min() > maxvp >= got[3][~love].max()
        t2, nar2 = e.solve_rows_radial_device()
        st2 = e.stats()
        assert nar2 == got[1].size and (bits(t2) == bits(got[0])).all()
        for k in ("nar", "rays", "ray_launches", "ray_steps", "rays_clamped"):
            assert st2[k] == st1[k] == st0[k], k
        e.solve_rows_radial_device(nar2)
        with pytest.raises(EngineError) as exc:
            e.solve_rows_radial_device(nar2 - 1)
        assert exc.value.code == ERR_CAPACITY
        with pytest.raises(EngineError) as exc:
            e.solve_rows_radial(nar2 - 1)
        assert exc.value.code == ERR_CAPACITY
        # the plain call afterwards is unchanged, and the option rows_on_device is off as it was found
        same_rows(e.solve_rows(cap), plain)
        nar = C.c_longlong(0)
        assert e._L.dsa_solve_rows(e._h, _p(np.zeros(e.ndata, F)), None, None, None, C.c_longlong(cap), C.byref(nar)) == ERR_ARGUMENT
    finally:
        e.close()


# ---- 3. the system ----

def system_case():
    c = synth.boundary_case(nx=10, ny=9, nz=4, kRc=3, kRg=1, kLc=1, kLg=1, nsrc=8, nrcf=8, ragged=False)
    c.update(threshold0=F(1.2), weight0=F(2.0), damp=F(0.5), minvel=F(1.5), maxvel=F(5.5))
    assert c["nparpi"] == 168
    return c


def solves_on(e, b, damp, n, m, seed):
    """dsa_spmv both ways on seeded vectors and dsa_lsmr, on whatever is resident on e"""
    rng = np.random.default_rng(seed)
    Ax = e.spmv(1, rng.standard_normal(n).astype(F), np.zeros(m, F))
    Aty = e.spmv(2, np.zeros(n, F), rng.standard_normal(m).astype(F))
    return dict(Ax=Ax, Aty=Aty, **e.lsmr(b, damp, *LSMR_ARGS))


def same_solves(a, b):
    for k in ("Ax", "Aty", "x", "normA", "condA", "normr", "normAr", "normx"):
        assert (bits(a[k]) == bits(b[k])).all(), k
    assert a["istop"] == b["istop"] and a["itn"] == b["itn"]


@pytest.fixture(scope="module")
def system_engine():
    """the system case on one engine with Vsh 3 % above Vsv, its host rows, and data with about a fifth of the weights at zero"""
    c = system_case()
    vsv = model_of(c); vsh = above(vsv)
    e, u = staged(c, vsv, vsh)
    rows = e.solve_rows_radial(capacity(c))
    r = synth.LCG(91)
    obst = (rows[0] * (1.0 + 0.04 * (r.uniform(c["ndata"]) - 0.5))).astype(F)
    yield dict(e=e, u=u, c=c, vsv=vsv, vsh=vsh, rows=rows, obst=obst)
    e.close()


def build(Q, weight_h, aniso):
    e, c = Q["e"], Q["c"]
    _, nnz = e.solve_rows_radial_device()
    assert nnz == Q["rows"][1].size
    return e.iteration_system_radial_device(c["nx"], c["ny"], c["nz"], Q["obst"], Q["rows"][0], c["threshold0"], c["weight0"], weight_h, aniso)


@pytest.mark.parametrize("weight_h,aniso", [(2.0, 0.0), (1.0, 0.3), (2.0, 0.3)])
def test_system_equals_the_twin_on_the_host_rows(system_engine, weight_h, aniso):
    from dsurftomo_amd.analyses.azimuthal import azimuthal_weights
    Q = system_engine
    e, c = Q["e"], Q["c"]
    dsyn, rw, iw, col = Q["rows"]
    dall, maxvp, damp = c["ndata"], c["nparpi"], float(c["damp"])
    D = build(Q, weight_h, aniso)
    dev = solves_on(e, D["cbst"], damp, D["n"], D["m"], 17)
    res = (Q["obst"] - dsyn).astype(F)
    dw = azimuthal_weights(res, c["threshold0"])
    assert 0 < int((dw == 0).sum()) < dall
    S = RD.radial_system(c["nx"], c["ny"], c["nz"], rw, iw, col, res, dw, c["weight0"], weight_h, aniso, Q["vsv"], Q["vsh"])
    assert D["m"] == S["m"] == dall + 3 * maxvp and D["n"] == S["n"] == 2 * maxvp and D["nar"] == S["rw"].size
    assert (bits(D["datweight"]) == bits(dw)).all() and (bits(D["cbst"]) == bits(S["b"])).all()
    tie_b = D["cbst"][dall + 2 * maxvp:]
    assert (tie_b != 0).all() if aniso > 0 else not tie_b.any()
    # norm: per column the sequential fp32 sum of |entry| over the scaled data entries in storage order
    want_norm = np.zeros(2 * maxvp, F)
    scaled = np.abs(S["rw"][:rw.size])
    for k in range(rw.size):
        want_norm[col[k] - 1] = want_norm[col[k] - 1] + scaled[k]
    assert (bits(D["norm"]) == bits(want_norm)).all() and want_norm[maxvp:].max() > 0 and want_norm[:maxvp].max() > 0
    for B in (0, 1):
        nb = D["norm"][B * maxvp:(B + 1) * maxvp]
        tot = F(0)
        for v in nb:
            tot = F(tot + v)
        assert (bits(D["dws"][B]) == bits(np.array([nb.max(), tot / F(maxvp)], F))).all()
    # the host route on the same engine
    e.spmv_load(S["m"], S["n"], S["rw"], S["row"], S["col"])
    same_solves(dev, solves_on(e, S["b"], damp, S["n"], S["m"], 17))
    assert dev["itn"] > 3 and dev["x"][maxvp:].any() and dev["x"][:maxvp].any()


# ---- 4. the update ----

def test_update_equals_begin_on_the_twins_models():
    """update_radial with a step that is clipped and driven to both bounds somewhere: the models through dispersion_get_model_radial and
    the next runs' maps are those of dispersion_begin_radial on the twin's stepped models; the ring and the bottom depth are untouched; at
    dvmax = 0.5 each block is dsa_model_update's"""
    c = synth.boundary_case()
    nx, ny, nz, maxvp = c["nx"], c["ny"], c["nz"], c["nparpi"]
    vsv = model_of(c); vsh = above(vsv)
    rng = np.random.default_rng(3)
    dv = (0.08 * rng.standard_normal(2 * maxvp)).astype(F)
    dv[[0, 1, maxvp, maxvp + 1]] = [0.9, -0.9, 0.2, -0.2]
    minvel, maxvel = F(2.55), F(3.6)
    e, u = staged(c, vsv, vsh)
    try:
        e.update_radial(dv, 0.2, minvel, maxvel)
        got = e.dispersion_get_model_radial()
        want = RD.update_radial_twin(vsv, vsh, dv, 0.2, minvel, maxvel)
        ring = np.ones((ny, nx), bool); ring[1:-1, 1:-1] = False
        for B, before in enumerate((vsv, vsh)):
            assert (bits(got[B]) == bits(want[B])).all(), B
            assert (bits(got[B][:, ring]) == bits(before[:, ring])).all() and (bits(got[B][-1]) == bits(before[-1])).all()
            inner = got[B][:-1, 1:-1, 1:-1]
            assert inner.min() == minvel and inner.max() == maxvel and (got[B] != before).any()
        # the next runs work on the stepped models
        RD.stage(e, c, u)
        no_failures(e)
        maps_got = e.dispersion_fetch(0, u["nmaps"])
        rows_got = e.solve_rows_radial(capacity(c))
        # dvmax = 0.5 on the stepped models: each block against the host's dsa_model_update
        e.update_radial(dv * F(4.0), 0.5, minvel, maxvel)
        half = e.dispersion_get_model_radial()
    finally:
        e.close()
    for B in (0, 1):
        host = np.array(want[B], F, copy=True); step = (dv * F(4.0))[B * maxvp:(B + 1) * maxvp].copy()
        assert e._L.dsa_model_update(nx, ny, nz, _p(step), _p(host), minvel, maxvel) == 0
        assert (bits(half[B]) == bits(host)).all(), B
    e2, _ = staged(c, want[0], want[1])
    try:
        assert (bits64(e2.dispersion_fetch(0, u["nmaps"])) == bits64(maps_got)).all()
        same_rows(e2.solve_rows_radial(capacity(c)), rows_got)
    finally:
        e2.close()


# ---- 5. refusals ----

def test_refusals_leave_the_engine_usable(system_engine):
    Q = system_engine
    e, c, u = Q["e"], Q["c"], Q["u"]
    nx, ny, nz, dall, maxvp = c["nx"], c["ny"], c["nz"], c["ndata"], c["nparpi"]
    cap = capacity(c)
    dsyn = Q["rows"][0]
    f = np.float32
    cbst = np.zeros(dall + 3 * maxvp, f); dw = np.zeros(dall, f); norm = np.zeros(2 * maxvp, f); dws = np.zeros(4, f)
    m, nar = C.c_int(0), C.c_longlong(0)
    lib = e._L

    def radial_system(h, w0=2.0, wh=1.0, an=0.3, obs=Q["obst"], nx_=nx):
        return lib.dsa_iteration_system_radial_device(h, nx_, ny, nz, dall, _p(obs), _p(dsyn), c["threshold0"], w0, wh, an, _p(cbst), _p(dw), _p(norm), C.byref(m),
                                                      C.byref(nar), _p(dws))

    def iso_system(h):
        return lib.dsa_iteration_system_device(h, nx, ny, nz, dall, _p(Q["obst"]), _p(dsyn), c["threshold0"], c["weight0"], _p(cbst), _p(dw), _p(norm), C.byref(m),
                                               C.byref(nar), _p(dws))

    def code(fn, *args):
        with pytest.raises(EngineError) as exc:
            fn(*args)
        return exc.value.code

    # the new calls on a plain stage, the engine usable after each
    p, _ = plain_staged(c, Q["vsv"])
    try:
        assert code(p.kernels_from_dispersion_radial) == ERR_STATE and "not radial" in lib.dsa_error_string(p._h).decode()
        assert code(p.solve_rows_radial, cap) == ERR_STATE
        assert code(p.solve_rows_radial_device) == ERR_STATE
        assert code(p.update_radial, np.zeros(2 * maxvp, f), 0.5, 1.5, 5.5) == ERR_STATE
        assert radial_system(p._h) == ERR_STATE                                                    # the builder without rows
        plain_rows = p.solve_rows(cap)
        assert plain_rows[1].size > 0
        # plain rows left on the device are not radial rows
        p.set_option("rows_on_device", 1)
        p.solve_rows_device()
        assert radial_system(p._h) == ERR_STATE and "not radial rows" in lib.dsa_error_string(p._h).decode()
        assert iso_system(p._h) == 0
    finally:
        p.close()
    # a slot without a fresh mark: before any run, and with one wave type's runs missing
    q = Engine(0)
    try:
        RD.begin(q, c, u, Q["vsv"], Q["vsh"])
        assert code(q.kernels_from_dispersion_radial) == ERR_STATE
        plan = depth.slot_plan(c)
        for wave, kind, t, first in plan[:-1]:
            q.dispersion_run(wave, kind, t, True, first, first)
        assert code(q.kernels_from_dispersion_radial) == ERR_STATE and "slot %d" % plan[-1][3] in lib.dsa_error_string(q._h).decode()
        wave, kind, t, first = plan[-1]
        q.dispersion_run(wave, kind, t, False, first, first)                                    # a run without kernels leaves the slot unmarked
        assert code(q.kernels_from_dispersion_radial) == ERR_STATE
        assert code(q.kernels_from_dispersion) == ERR_STATE                                       # ... and the plain call keeps refusing a radial stage
        RD.stage(q, c, u)
        same_rows(q.solve_rows_radial(cap), Q["rows"])
        # rows after an update without new kernels; stale slots
        q.update_radial(np.zeros(2 * maxvp, f), 0.5, 1.5, 5.5)
        assert code(q.solve_rows_radial, cap) == ERR_STATE and code(q.solve_rows_radial_device) == ERR_STATE
        assert code(q.kernels_from_dispersion_radial) == ERR_STATE
        for bad in ((np.zeros(2 * maxvp, f), 0.0, 1.5, 5.5), (np.zeros(2 * maxvp, f), float("nan"), 1.5, 5.5), (np.zeros(2 * maxvp, f), 0.5, 5.5, 1.5)):
            assert code(q.update_radial, *bad) == ERR_ARGUMENT
        assert lib.dsa_update_radial(q._h, nx, ny, nz, None, 0.5, 1.5, 5.5) == ERR_ARGUMENT and lib.dsa_update_radial(q._h, nx + 1, ny, nz, _p(norm), 0.5, 1.5, 5.5) == ERR_ARGUMENT
        RD.stage(q, c, u)
        same_rows(q.solve_rows_radial(cap), Q["rows"])                                            # a zero step: the same models, the same rows
    finally:
        q.close()
    # only some of the three arrays
    out = np.zeros(e.ndata, f); rw = np.zeros(cap, f); iw = np.zeros(cap, np.int32)
    n = C.c_longlong(0)
    for arrays in ((_p(rw), None, None), (_p(rw), _p(iw), None), (None, _p(iw), _p(iw))):
        assert lib.dsa_solve_rows_radial(e._h, _p(out), *arrays, C.c_longlong(cap), C.byref(n)) == ERR_ARGUMENT
    # radial rows: the isotropic builder refuses them, whatever the option rows_on_device says; bad weights and a bad aniso leave them alone; the builder twice
    e.solve_rows_radial_device()
    assert iso_system(e._h) == ERR_STATE and "radial" in lib.dsa_error_string(e._h).decode()
    for w0, wh, an in ((-1.0, 1.0, 0.3), (2.0, -1.0, 0.3), (2.0, 1.0, -0.3), (float("nan"), 1.0, 0.3), (2.0, float("inf"), 0.3), (2.0, 1.0, float("nan"))):
        assert radial_system(e._h, w0, wh, an) == ERR_ARGUMENT
    assert radial_system(e._h, obs=None) == ERR_ARGUMENT and radial_system(e._h, nx_=2) == ERR_ARGUMENT and radial_system(e._h, nx_=nx + 1) == ERR_ARGUMENT
    assert radial_system(e._h) == 0 and m.value == dall + 3 * maxvp
    b = cbst.copy()
    assert radial_system(e._h) == ERR_STATE and "already" in lib.dsa_error_string(e._h).decode() and iso_system(e._h) == ERR_STATE
    # the sweeps that rescale every row below the data refuse the radial system; the plain solve runs
    K = 2
    w = np.array([2.0, 1.0], f); d = np.array([0.5, 0.5], f)
    x = np.zeros((K, 2 * maxvp), f); meas = np.zeros((K, 4)); istop = np.zeros(2 * K + 2, np.int32); itn = np.zeros(2 * K + 2, np.int32); est = np.zeros((2 * K + 2, 5), f)
    assert lib.dsa_lsmr_tradeoff(e._h, K, dall, _p(b), 2.0, _p(w), _p(d), *LSMR_ARGS, _p(x), _p(meas), _p(istop), _p(itn), _p(est)) == ERR_STATE
    assert "tie rows" in lib.dsa_error_string(e._h).decode()
    fold = (np.arange(dall) % 2).astype(np.int32)
    assert lib.dsa_lsmr_crossval(e._h, 1, 2, dall, _p(b), 2.0, _p(w), _p(d), _p(fold), *LSMR_ARGS, None, _p(meas), None, _p(istop), _p(itn), _p(est)) == ERR_STATE
    e._mn = (m.value, 2 * maxvp)
    sol = e.lsmr(b, 0.5, *LSMR_ARGS)
    assert sol["itn"] > 3
    # ... and a matrix loaded afterwards is no radial system: the sweep takes it
    S = RD.radial_system(nx, ny, nz, Q["rows"][1], Q["rows"][2], Q["rows"][3], (Q["obst"] - dsyn).astype(f), dw, 2.0, 1.0, 0.3, Q["vsv"], Q["vsh"])
    e.spmv_load(S["m"], S["n"], S["rw"], S["row"], S["col"])
    rc = lib.dsa_lsmr_tradeoff(e._h, K, dall, _p(b), 2.0, _p(w), _p(d), *LSMR_ARGS, _p(x), _p(meas), _p(istop), _p(itn), _p(est))
    assert rc == 0 or "tie rows" not in lib.dsa_error_string(e._h).decode()


# ---- 6. block PSFs ----

def test_block_psfs_on_the_radial_system(system_engine):
    """dsa_resolution_blocks(nblocks = 2) on the radial system, spikes across the boundary between the blocks: the solves are
    dsa_lsmr_resolution's bits, the co-located values exact, the fp64 sums NumPy's to 1e-9"""
    from test_gpu_azimuthal_device import check_blocks
    Q = system_engine
    e, c = Q["e"], Q["c"]
    maxvp = c["nparpi"]
    D = build(Q, 1.0, 0.3)
    coords = unknown_coords(c)
    first, Rn = maxvp - 40, 80
    plain, P = check_blocks(e, c["ndata"], 2 * maxvp, 2, first, Rn, coords, float(c["damp"]), 400)
    assert P["itn"].max() > 3
    for r in (0, 39, 40, 79):
        j = first + r
        assert P["psf"][r, j // maxvp, 0] == P["x"][r, j]
        assert P["psf"][r, 1 - j // maxvp, 0] == P["x"][r, (j + maxvp) % (2 * maxvp)]
    # the tie rows couple the blocks: a spike's image has energy in the other block
    assert (P["psf"][:40, 1, 1] > 0).any() and (P["psf"][40:, 0, 1] > 0).any()


# ---- 7. linear recovery ----

# What fp32 LSMR on the device showed against SciPy's fp64 LSMR on the same assembled system in the first run on an MI355X (DESIGN.md
# section 28): (device figure, SciPy figure) of the rms error of dVsh in km/s; the test allows the device to exceed SciPy by twice the
# observed excess.
RECOVERY_WEIGHT, RECOVERY_DAMP, RECOVERY_ANISO, RECOVERY_THRESHOLD = 0.2, 0.01, 0.05, 1000.0
# 0.007088497 km/s against 0.007088510 (the anomaly's rms over those 180 cells: 0.034308), itn 35: no excess, so no margin.
OBSERVED = {"vsh_rms": (0.007088497, 0.007088510)}


def allowed(key, err_ref):
    dev, ref = OBSERVED[key]
    return err_ref + 2.0 * max(dev - ref, 0.0)


def gaussian_vsh(c, vsv, percent=3.0, sigma=2.5, sigma_z=0.8):
    """(2 maxvp,) float64: dVsv = 0, dVsh a Gaussian of `percent` of the local velocity around the middle of the grid at mid depth, sigma in
    cells"""
    nvx, nvz, nl = c["nx"] - 2, c["ny"] - 2, c["nz"] - 1
    k, j, i = np.meshgrid(np.arange(nl), np.arange(nvz), np.arange(nvx), indexing="ij")
    g = np.exp(-0.5 * (((i - (nvx - 1) / 2.0) ** 2 + (j - (nvz - 1) / 2.0) ** 2) / sigma ** 2 + (k - (nl - 1) / 2.0) ** 2 / sigma_z ** 2)).ravel()
    out = np.zeros(2 * nvx * nvz * nl)
    out[nvx * nvz * nl:] = 0.01 * percent * vsv.astype(np.float64).ravel()[RD.unknown_nodes(c["nx"], c["ny"], c["nz"])] * g
    return out


def test_linear_recovery_against_scipy():
    """obst = dsyn + G0 delta with dVsh a +3 % Gaussian at mid depth and dVsv = 0, both models the case's: one step on the device against
    SciPy's fp64 lsmr on the twin's assembled system, over the cells of the Vsh block with above-median DWS"""
    import scipy.sparse as sp
    from scipy.sparse.linalg import lsmr
    c = synth.boundary_case()
    vs = model_of(c)
    maxvp = c["nparpi"]
    e, u = staged(c, vs, vs)
    try:
        dsyn, rw, iw, col = e.solve_rows_radial(capacity(c))
        dall = dsyn.size
        G = sp.csr_matrix((rw.astype(np.float64), (iw - 1, col - 1)), shape=(dall, 2 * maxvp))
        truth = gaussian_vsh(c, vs)
        obst = (dsyn.astype(np.float64) + G @ truth).astype(F)
        e.solve_rows_radial_device()
        D = e.iteration_system_radial_device(c["nx"], c["ny"], c["nz"], obst, dsyn, RECOVERY_THRESHOLD, RECOVERY_WEIGHT, RECOVERY_WEIGHT, RECOVERY_ANISO)
        dev = e.lsmr(D["cbst"], RECOVERY_DAMP, *LSMR_ARGS)
    finally:
        e.close()
    assert D["datweight"].mean() > 0.9
    S = RD.radial_system(c["nx"], c["ny"], c["nz"], rw, iw, col, (obst - dsyn).astype(F), D["datweight"], RECOVERY_WEIGHT, RECOVERY_WEIGHT, RECOVERY_ANISO, vs, vs)
    A = sp.csr_matrix((S["rw"].astype(np.float64), (S["row"] - 1, S["col"] - 1)), shape=(S["m"], S["n"]))
    atol, btol, conlim, itnlim, _ = LSMR_ARGS
    x = lsmr(A, S["b"].astype(np.float64), damp=RECOVERY_DAMP, atol=atol, btol=btol, conlim=conlim, maxiter=itnlim)[0]
    dws = D["norm"][maxvp:]
    cells = dws > np.median(dws)
    rms = lambda v: float(np.sqrt(np.mean(np.square(v))))
    err_ref, err_dev, size = rms((x - truth)[maxvp:][cells]), rms((dev["x"].astype(np.float64) - truth)[maxvp:][cells]), rms(truth[maxvp:][cells])
    print("radial recovery (vsh_rms): rms error of dVsh over %d cells: scipy fp64 %.9f km/s, device fp32 %.9f km/s, rms of the anomaly %.6f km/s; device itn %d istop %d; "
          "rms of the recovered dVsv %.6f km/s" % (int(cells.sum()), err_ref, err_dev, size, dev["itn"], dev["istop"], rms(dev["x"][:maxvp].astype(np.float64))))
    assert err_ref < 0.5 * size, "the yardstick itself must recover the anomaly"
    assert err_dev <= allowed("vsh_rms", err_ref)


# ---- 8. the nonlinear loop ----

# chosen on the CPU with the reference's forward path and SciPy's fp64 LSMR on the twin's system (there: 0.21362 0.04309 0.01502 0.01288 s, final
# Love 0.02211 s against the isotropic loop's 0.19508 s, median xi 1.07278), not on the device
LOOP = dict(weight=0.5, damp=0.05, aniso=0.05, dvmax=0.5, threshold0=1000.0)


def isotropic_loop(c, u, start, obst, iterations):
    """the existing route on one model: per iteration the stage, the rows left on the device, dsa_iteration_system_device, dsa_lsmr,
    dsa_model_update; then the times of the final model.  Returns the residuals of the final model."""
    nx, ny, nz, dall, maxvp = c["nx"], c["ny"], c["nz"], c["ndata"], c["nparpi"]
    vs = np.array(start, F, copy=True)
    e = Engine(0)
    try:
        e.set_option("rows_on_device", 1)
        for it in range(iterations + 1):
            e.dispersion_begin(vs, c["depz"], c["minthk"], c["kmax"], u["nmaps"])
            plain_stage(e, c, u)
            if it == iterations:
                return (obst - e.solve()).astype(F)
            dsyn, _ = e.solve_rows_device()
            cbst = np.zeros(dall + maxvp, F); dw = np.zeros(dall, F); norm = np.zeros(maxvp, F); dws = np.zeros(2, F)
            m, nar = C.c_int(0), C.c_longlong(0)
            assert e._L.dsa_iteration_system_device(e._h, nx, ny, nz, dall, _p(obst), _p(dsyn), LOOP["threshold0"], LOOP["weight"], _p(cbst), _p(dw), _p(norm),
                                                    C.byref(m), C.byref(nar), _p(dws)) == 0
            e._mn = (m.value, maxvp)
            x = e.lsmr(cbst, LOOP["damp"], *LSMR_ARGS)["x"].copy()
            assert e._L.dsa_model_update(nx, ny, nz, _p(x), _p(vs), c["minvel"], c["maxvel"]) == 0
    finally:
        e.close()


def test_nonlinear_loop_recovers_radial_anisotropy():
    """truth: Vsv the case's model, Vsh = Vsv (1 + 0.06 sin(pi (k + 0.5) / (nz - 1))) above the bottom; obst the times of the truth's radial
    stage; both models start from Vsv; three iterations.  Conditions: (i) the weighted rms residual falls strictly from iteration to
    iteration, (ii) the final Love rms is below that of the isotropic loop on the same data and settings, (iii) the median xi over the cells
    with above-median DWS (both blocks' added) is > 1.  Conditions, not measurements; what the first run showed:
    weighted rms residual 0.21576 -> 0.04214 -> 0.02440 -> 0.02290 s, final Love rms 0.02290 s against the isotropic loop's 0.19530 s, median
    xi 1.07875 over 180 cells (truth 1.11394), itn 35, 34, 33.  The reference's quartile rule kept all 113 data in the three systems and 16
    of the final residuals -- nearly all of them have one sign by then, so the rule drops the small ones: the final figures are over the
    largest residuals, of the radial and of the isotropic loop alike."""
    from dsurftomo_amd.analyses.azimuthal import azimuthal_weights
    c = synth.boundary_case()
    c.update(threshold0=F(LOOP["threshold0"]), minvel=F(1.5), maxvel=F(5.5))
    nz, maxvp = c["nz"], c["nparpi"]
    vsv = model_of(c)
    vsh = np.array(vsv, F, copy=True)
    for k in range(nz - 1):
        vsh[k] = (vsv[k] * F(1.0 + 0.06 * np.sin(np.pi * (k + 0.5) / (nz - 1)))).astype(F)
    t, u = staged(c, vsv, vsh)
    try:
        obst = t.solve()
    finally:
        t.close()
    e = Engine(0)
    log = []
    try:
        RD.begin(e, c, u, vsv, vsv)
        out = RD.iterate(e, c, u, obst, 3, LOOP["weight"], LOOP["weight"], LOOP["damp"], LOOP["aniso"], LOOP["dvmax"], log=log.append)
        RD.stage(e, c, u)
        no_failures(e)
        res = (obst - e.solve()).astype(F)
        got_v, got_h = e.dispersion_get_model_radial()
    finally:
        e.close()
    w = azimuthal_weights(res, LOOP["threshold0"])
    final = RD.wave_rms(res, w, u["wave"])
    rms = [h["rms"] for h in out["history"]] + [final[None][1]]
    res_iso = isotropic_loop(c, u, vsv, obst, 3)
    iso = RD.wave_rms(res_iso, azimuthal_weights(res_iso, LOOP["threshold0"]), u["wave"])
    norm = out["system"]["norm"]
    cells = (norm[:maxvp] + norm[maxvp:]) > np.median(norm[:maxvp] + norm[maxvp:])
    node = RD.unknown_nodes(c["nx"], c["ny"], c["nz"])
    xi = (got_h.ravel()[node].astype(np.float64) / got_v.ravel()[node]) ** 2
    xi_true = (vsh.ravel()[node].astype(np.float64) / vsv.ravel()[node]) ** 2
    print("radial loop: weighted rms residual %s s; final Rayleigh %.5f s Love %.5f s; isotropic loop's final Rayleigh %.5f s Love %.5f s; "
          "median xi over %d cells %.5f (truth %.5f); itn %s; data kept %s then %d" % (" ".join("%.5f" % r for r in rms), final[2][1], final[1][1], iso[2][1], iso[1][1], int(cells.sum()),
                                                                 float(np.median(xi[cells])), float(np.median(xi_true[cells])), [h["itn"] for h in out["history"]],
                                                                 [h["kept"] for h in out["history"]], final[None][0]))
    assert len(log) == 3 and all(h["itn"] > 0 for h in out["history"])
    assert all(b < a for a, b in zip(rms, rms[1:])), rms
    assert final[1][1] < iso[1][1]
    assert float(np.median(xi[cells])) > 1.0


# ---- 9. the driver ----

DEAL = (8, 5, 7, 6)                      # the Taipei example's 26 periods as Rayleigh phase, Rayleigh group, Love phase, Love group periods


def deal_taipei(path, vel_obs=None):
    """the Taipei example's directory with its periods dealt out over the four wave types (DEAL), the way dsurftomo_amd.io.load reads it:
    the input file's period lists and the data file's source lines say so; the stations, the grid, the model and every other setting are
    the example's.  vel_obs: the velocities of the receiver lines in file order (None: the example's)."""
    import shutil
    with open(os.path.join(io.HERE, "DSurfTomo.in")) as fh:
        lines = fh.read().splitlines()
    t = lines[14].split()
    assert lines[13].split()[0] == "26" and len(t) == 26 == sum(DEAL)
    per, first = [], 0
    for n in DEAL:
        per += ["%d" % n, " ".join(t[first:first + n])]
        first += n
    (path / "DSurfTomo.in").write_text("\n".join(lines[:13] + per + lines[18:21]) + "\n")
    shutil.copy(os.path.join(io.HERE, "MOD"), str(path / "MOD"))
    bounds = np.cumsum((0,) + DEAL)
    out, q = [], 0
    with open(os.path.join(io.HERE, lines[3].split()[0])) as fh:
        for line in fh:
            if not line.strip():
                continue
            if line[0] == "#":
                w = line[1:].split()
                slot = int(w[2]) - 1
                kind = int(np.searchsorted(bounds, slot, side="right")) - 1
                out.append("# %s %s %d %d %d" % (w[0], w[1], slot - bounds[kind] + 1, 2 if kind < 2 else 1, kind % 2))
            else:
                w = line.split()
                out.append("%s %s %s" % (w[0], w[1], w[2] if vel_obs is None else "%.7f" % vel_obs[q]))
                q += 1
    (path / lines[3].split()[0]).write_text("\n".join(out) + "\n")


def test_driver_on_the_taipei_grid(tmp_path):
    """radial.run end to end on the Taipei example's grid and stations, its 26 periods dealt out over the four wave types; the observations
    are the times of a truth with Vsh 5 % above the model at mid depth: both files' shapes, xi finite, every node inside [minvel, maxvel]"""
    src = tmp_path / "case"; out_dir = tmp_path / "out"
    src.mkdir(); out_dir.mkdir()
    deal_taipei(src)
    c = io.load(str(src))
    assert (c["kRc"], c["kRg"], c["kLc"], c["kLg"]) == DEAL and c["ndata"] == io.load()["ndata"]
    nx, ny, nz = c["nx"], c["ny"], c["nz"]
    vsv = model_of(c)
    vsh = np.array(vsv, F, copy=True)
    mid = (nz - 1) // 2
    vsh[mid] = (vsv[mid] * F(1.05)).astype(F)
    truth = Engine(0)
    try:
        u = RD.radial_plan(c)
        RD.begin(truth, c, u, vsv, vsh)
        RD.stage(truth, c, u)
        obst = truth.solve()
    finally:
        truth.close()
    assert (obst > 0).all()
    deal_taipei(src, np.asarray(c["dist"], np.float64) / obst)
    cl = io.load(str(src))
    assert cl["ndata"] == c["ndata"] and np.abs(cl["obst"] - obst).max() < 1e-5 * obst.max()
    log = []
    out, path = RD.run(str(src), iterations=2, aniso=0.1, resolution=True, out_dir=str(out_dir), log=log.append)
    rows = depth.read_radial(path)
    assert path.endswith("DSurfTomo.inRadial.dat") and len(rows) == nx * ny * nz
    assert [r["vsv"] for r in rows] == out["vsv"].ravel().astype(np.float64).tolist() and [r["vsh"] for r in rows] == out["vsh"].ravel().astype(np.float64).tolist()
    assert all(np.isfinite(r["xi"]) and r["xi"] > 0 for r in rows)
    for model in (out["vsv"], out["vsh"]):
        assert np.isfinite(model).all() and model.min() >= cl["minvel"] and model.max() <= cl["maxvel"]
    assert (out["vsh"] != out["vsv"]).any()
    res = RD.read_radial_resolution(str(out_dir / "DSurfTomo.inRadialResolution.dat"))
    maxvp = cl["nparpi"]
    assert len(res) == 2 * maxvp and [r["block"] for r in res] == [0] * maxvp + [1] * maxvp
    assert all(np.isfinite(r["rjj"]) and 0.0 <= r["share"] <= 1.0 for r in res) and max(r["rjj"] for r in res) > 0
    h = out["history"]
    assert len(h) == 2 and all(q["itn"] > 0 for q in h) and h[1]["rms"] < h[0]["rms"]
    assert len(log) == 2 + 2 + 1 and "Rayleigh" in log[0] and "Vsv -> Vsh" in log[3]
