"""dsa_step_models / dsa_forward_steps: K models built on the device from a base model and K steps (host steps, or the solutions a batch
solve left on the drop-in engine), forward-modelled in one call and judged by misfit sums reduced on the device; and
python -m dsurftomo_amd.invert --tradeoff-nonlinear / --crossval-nonlinear on top.

* the models are bit-identical to K host dsa_model_update calls on copies (a NaN step: a NaN node);
* under exact_ties = 2 dsurf is bit-identical to dsa_forward_models on those models, for either unit order and any pass size, and so
  are the sums; each sum is within relative (N + 4) 2^-52 of numpy on the returned times -- the bound of two fp64 summation orders of
  N non-negative terms, N the group's data count;
* steps == NULL after dsa_lsmr_tradeoff (6 and 70 members) and dsa_lsmr_crossval gives the bits of the same steps from the host, and
  DSA_ERR_STATE where no fitting batch is resident;
* default mode with bundles across models: every time within 1e-4 s of the oracle's CalSurfG on the host-built model;
* the Taipei example.

The five steps, for unknown (i, jj, l) and p = sin(2 i/(nx-2) + 0.5 l) cos(1.3 jj/(ny-2)): 0, 0.30 p, 0.90 p, +0.5 everywhere, -0.7
everywhere, in float32, with minvel 2.2 and maxvel 4.0: each of the three clips of the update bites.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _libs as L
import parity_log
import synth
from dsurftomo_amd import invert
from dsurftomo_amd import io as taipei
from dsurftomo_amd.engine import Engine, EngineError
from test_gpu_forward_models import BIG, GROUPS, bits32, bits64, dropin, exact2, forward_models     # noqa: F401 (dropin, exact2: fixtures)
from test_gpu_lsmr import system
from test_gpu_tradeoff import MEMBERS

pytestmark = pytest.mark.gpu
TOL = 1e-4
ERR_ARGUMENT, ERR_STATE = -2, -5
MINVEL, MAXVEL = 2.2, 4.0
ALPHA = [0.0, 0.5, 1.0, 2.0, 1.0]


def five_steps(c):
    """(5, n) float32 in the order of dsa_model_update's dv: layer, then jj, then i"""
    nx, ny, nz = c["nx"], c["ny"], c["nz"]
    l = np.arange(nz - 1, dtype=np.float64)[:, None, None]
    jj = np.arange(ny - 2, dtype=np.float64)[None, :, None]
    i = np.arange(nx - 2, dtype=np.float64)[None, None, :]
    p = np.sin(2.0 * i / (nx - 2) + 0.5 * l) * np.cos(1.3 * jj / (ny - 2))
    one = np.ones_like(p)
    return np.stack([0.0 * p, 0.30 * p, 0.90 * p, 0.5 * one, -0.7 * one]).reshape(5, -1).astype(np.float32)


def host_models(lib, c, steps, alpha=None):
    """the host loop: dsa_model_update on a copy of the model and a copy of the (scaled) step, per member.  List of (nx, ny, nz) Fortran arrays."""
    f = np.float32
    invert.bind(lib)
    out = []
    for k, s in enumerate(steps):
        step = np.array(s if alpha is None else f(alpha[k]) * np.asarray(s, f), f, copy=True)      # (a copy: dsa_model_update clips it in place)
        m = np.asfortranarray(np.array(c["vels"], f, copy=True))
        assert lib.dsa_model_update(c["nx"], c["ny"], c["nz"], L.ptr(step), L.ptr(m), MINVEL, MAXVEL) == 0
        out.append(m)
    return out


def bite(c, steps, alpha, models):
    """(steps clipped, nodes at minvel, nodes at maxvel) over all members"""
    f = np.float32
    s = np.asarray(steps, f) if alpha is None else (np.asarray(alpha, f)[:, None] * np.asarray(steps, f)).astype(f)
    m = np.stack(models)
    return int((np.abs(s) > 0.5).sum()), int((m == f(MINVEL)).sum()), int((m == f(MAXVEL)).sum())


def same_models(got, want):
    """NaN where the host has NaN, the same bits elsewhere"""
    got, want = np.asarray(got, np.float32), np.stack(want)
    assert got.shape == want.shape
    nan = np.isnan(want)
    return bool(np.isnan(got[nan]).all() and (bits32(got[~nan]) == bits32(want[~nan])).all())


def test_step_models_equal_the_host_loop(engine):
    lib = engine._L
    c = synth.boundary_case()
    assert (c["nx"], c["ny"], c["nz"], c["nparpi"], c["ndata"]) == (12, 11, 5, 360, 113)
    steps = five_steps(c)
    for alpha in (None, ALPHA):
        want = host_models(lib, c, steps, alpha)
        got = engine.step_models(c["vels"], steps, MINVEL, MAXVEL, alpha)
        assert same_models(got, want) and not np.isnan(got).any()
        clips, lo, hi = bite(c, steps, alpha, want)
        print("alpha", alpha, "steps clipped", clips, "nodes at minvel", lo, "at maxvel", hi)
        assert clips > 0 and lo > 0 and hi > 0
        # the outer ring in x and the bottom layer keep the base value
        assert (bits32(got[:, 0]) == bits32(c["vels"][0])).all() and (bits32(got[:, :, -1]) == bits32(c["vels"][:, -1])).all()
        assert (bits32(got[..., -1]) == bits32(c["vels"][..., -1])).all()
    assert len(set(m.tobytes() for m in want)) == 5
    # a member with a NaN, a +inf, a -inf and steps of exactly +-0.5
    odd = (0.2 * steps[2]).astype(np.float32)
    odd[[3, 50, 97, 200, 301]] = [np.nan, np.inf, -np.inf, 0.5, -0.5]
    both = np.stack([odd, steps[1]])
    want = host_models(lib, c, both)
    got = engine.step_models(c["vels"], both, MINVEL, MAXVEL)
    assert int(np.isnan(want[0]).sum()) == 1 and not np.isnan(want[1]).any()
    assert same_models(got, want)
    got = engine.step_models(c["vels"], both, MINVEL, MAXVEL, [1.0, 0.5])
    assert same_models(got, host_models(lib, c, both, [1.0, 0.5]))


# ---- the drop-in entry -----------------------------------------------------------------------------------------------------------

def forward_steps(lib, c, steps, alpha=None, dicing=8, ldd=None, fill=0.0, obst=None, w=None, group=None, ngroups=1, dsurf=True, models=True, measures=True,
                  nmodels=None, expect=0):
    """dsa_forward_steps; steps None: the resident batch, nmodels members.  Returns dict(models (K, nx, ny, nz), dsurf (K, ldd), measures
    (K, ngroups, 2), fails (K,)), None where not asked for"""
    f = np.float32
    nx, ny, nz, nd = c["nx"], c["ny"], c["nz"], c["ndata"]
    if steps is not None:
        steps = np.ascontiguousarray(steps, f)
        K = steps.shape[0]
    else:
        K = int(nmodels)
    ldd = nd if ldd is None else ldd
    base = np.ascontiguousarray(c["vels"].transpose(2, 1, 0), f)
    out_m = np.zeros((K, nz, ny, nx), f) if models else None
    out_d = np.full((K, ldd), fill, f) if dsurf else None
    out_s = np.full((K, ngroups, 2), -1.0) if measures and obst is not None else None
    fails = np.full(K, -1, np.int64)
    i32 = lambda v: C.byref(C.c_int(int(v)))
    f32 = lambda v: C.byref(C.c_float(float(v)))
    p = lambda a: None if a is None else L.ptr(np.ascontiguousarray(a))
    keep = [np.ascontiguousarray(a) if a is not None else None for a in (alpha if alpha is None else np.asarray(alpha, f), obst, w, group)]
    _, tail = taipei._args(c)
    rc = lib.dsa_forward_steps(i32(nx), i32(ny), i32(nz), i32(K), L.ptr(base), p(steps), p(keep[0]), f32(MINVEL), f32(MAXVEL), p(out_m), p(out_d), i32(ldd), i32(dicing),
                               L.ptr(fails), p(keep[1]), p(keep[2]), p(keep[3]), i32(ngroups), p(out_s), *tail)
    assert rc == expect, (rc, lib.dsa_dropin_error())
    return dict(models=None if out_m is None else out_m.transpose(0, 3, 2, 1), dsurf=out_d, measures=out_s, fails=fails)


def data_of(c, times):
    """observed times, weights (some 0) and the group i mod 3 for the measures of a case"""
    nd = c["ndata"]
    r = synth.LCG(4242)
    obst = (times * (1.0 + 0.04 * (r.uniform(nd) - 0.5))).astype(np.float32)
    u = r.uniform(nd)
    w = np.where(u < 0.15, 0.0, 0.5 + u).astype(np.float32)
    return obst, w, (np.arange(nd) % 3).astype(np.int32)


def assert_measures(got, dsurf, obst, w, group, ngroups):
    """each sum within relative (N + 4) 2^-52 of numpy on the times the same call returned, N the group's data count"""
    want = invert.nonlinear_measures(obst, dsurf, w, group, ngroups)
    counts = np.bincount(np.zeros(obst.size, np.int64) if group is None else group, minlength=ngroups)
    worst = 0.0
    for g in range(ngroups):
        tol = (counts[g] + 4) * 2.0 ** -52
        d = np.abs(got[:, g] - want[:, g])
        assert (d <= tol * want[:, g]).all(), (g, got[:, g], want[:, g])
        if counts[g]:
            assert (want[:, g] > 0).all()
            worst = max(worst, float((d / want[:, g]).max() / tol))
    return worst


@pytest.mark.parametrize("name,kw", [("default", {}), ("groups", GROUPS)])
def test_forward_steps_equal_forward_models_on_the_host_built_models(exact2, name, kw):
    lib, h = exact2
    c = synth.boundary_case(**kw)
    nd = c["ndata"]
    steps = five_steps(c)
    want_m = host_models(lib, c, steps)
    clips, lo, hi = bite(c, steps, None, want_m)
    assert clips > 0 and lo > 0 and hi > 0
    for dicing in (8, 5):
        want_t, f0 = forward_models(lib, c, want_m, dicing)
        assert (f0 == 0).all() and np.isfinite(want_t).all() and (want_t > 0).all() and want_t.max() < 64.0
        obst, w, group = data_of(c, want_t[0])
        r = forward_steps(lib, c, steps, dicing=dicing, obst=obst, w=w, group=group, ngroups=4)
        assert (r["fails"] == 0).all()
        assert same_models(r["models"], want_m)
        assert (bits32(r["dsurf"]) == bits32(want_t)).all(), (name, dicing, float(np.abs(r["dsurf"] - want_t).max()))
        worst = assert_measures(r["measures"], r["dsurf"], obst, w, group, 4)
        assert (r["measures"][:, 3] == 0).all() and not np.signbit(r["measures"][:, 3]).any()       # the empty group: +0
        assert (r["measures"][2:, :3] > 0).all()
        one = forward_steps(lib, c, steps, dicing=dicing, obst=obst, w=w)                           # group NULL: one group
        worst = max(worst, assert_measures(one["measures"], one["dsurf"], obst, w, None, 1))
        assert (bits32(one["dsurf"]) == bits32(want_t)).all()
        plain = forward_steps(lib, c, steps, dicing=dicing, obst=obst, models=False)                # no weights: both sums are the plain one
        assert (bits64(plain["measures"][..., 0]) == bits64(plain["measures"][..., 1])).all()
        assert (bits64(plain["measures"][..., 1]) == bits64(one["measures"][..., 1])).all()
        # the same call again, passes of 3 + 2, the other unit order, no dsurf: the same bits
        again = forward_steps(lib, c, steps, dicing=dicing, obst=obst, w=w, group=group, ngroups=4)
        assert lib.dsa_set_option(h, b"forward_models_chunk", C.c_double(3)) == 0
        split = forward_steps(lib, c, steps, dicing=dicing, obst=obst, w=w, group=group, ngroups=4)
        assert lib.dsa_set_option(h, b"forward_models_chunk", C.c_double(0)) == 0
        assert lib.dsa_set_option(h, b"forward_models_order", C.c_double(1)) == 0
        other = forward_steps(lib, c, steps, dicing=dicing, obst=obst, w=w, group=group, ngroups=4)
        split_other = None
        if dicing == 8:
            assert lib.dsa_set_option(h, b"forward_models_chunk", C.c_double(3)) == 0
            split_other = forward_steps(lib, c, steps, dicing=dicing, obst=obst, w=w, group=group, ngroups=4, dsurf=False)
            assert lib.dsa_set_option(h, b"forward_models_chunk", C.c_double(0)) == 0
        assert lib.dsa_set_option(h, b"forward_models_order", C.c_double(0)) == 0
        blind = forward_steps(lib, c, steps, dicing=dicing, obst=obst, w=w, group=group, ngroups=4, dsurf=False, models=False)
        assert blind["dsurf"] is None and blind["models"] is None
        for tag, v in (("again", again), ("passes", split), ("order", other), ("order + passes, no dsurf", split_other), ("no dsurf", blind)):
            if v is None:
                continue
            assert (v["fails"] == 0).all()
            assert (bits64(v["measures"]) == bits64(r["measures"])).all(), (name, dicing, tag)
            if v["dsurf"] is not None:
                assert (bits32(v["dsurf"]) == bits32(want_t)).all(), (name, dicing, tag)
            if v["models"] is not None:
                assert same_models(v["models"], want_m), (name, dicing, tag)
        # ldd above the number of data: the rows beyond stay as they were
        pad = forward_steps(lib, c, steps, dicing=dicing, ldd=nd + 5, fill=-7.0, obst=obst, w=w, group=group, ngroups=4)
        assert (bits32(pad["dsurf"][:, :nd]) == bits32(want_t)).all() and (pad["dsurf"][:, nd:] == -7.0).all()
        assert (bits64(pad["measures"]) == bits64(r["measures"])).all()
        # alpha: the models of the scaled steps
        al = forward_steps(lib, c, steps, alpha=ALPHA, dicing=dicing, dsurf=False)
        assert same_models(al["models"], host_models(lib, c, steps, ALPHA)) and al["measures"] is None
        parity_log.add(f"dsa_forward_steps, case {name}, dicing {dicing}, exact_ties 2: 5 models x {nd} data = dsa_forward_models on the host-built models, bit for bit; "
                       f"misfit sums vs numpy: worst {worst:.3f} of the bound (N + 4) 2^-52")


# ---- the resident source ---------------------------------------------------------------------------------------------------------

def borrowed(lib, h):
    """an Engine object on the drop-in engine's handle (never closed: the handle is the library's)"""
    e = Engine.__new__(Engine)
    e._L, e._h = lib, h
    e.nnx = e.nnz = e._nrays = e._ndata = 0
    e._disp = (0, 0, 0)
    return e


def same_results(a, b):
    return (same_models(a["models"], list(np.asarray(b["models"]))) and (bits32(a["dsurf"]) == bits32(b["dsurf"])).all()
            and (bits64(a["measures"]) == bits64(b["measures"])).all() and (a["fails"] == b["fails"]).all())


def test_resident_steps_equal_host_steps(exact2):
    lib, h = exact2
    c = synth.boundary_case()
    nd, n = c["ndata"], c["nparpi"]
    fwd = L.call_boundary(lib.dsa_calsurfg, c)
    S = system(c, weight0=2.0, fwd=fwd)
    assert S["n"] == n and S["m"] == nd + n
    obst, w, group = data_of(c, fwd["dsurf"])
    kw = dict(obst=obst, w=w, group=group, ngroups=3)
    e = borrowed(lib, h)
    try:
        nar = S["nar"]
        load = lambda: e.spmv_load(S["m"], S["n"], S["rw"], S["iw"][1:nar + 1], S["iw"][nar + 1:])
        # no batch solved: a fresh engine, and the drop-in engine right after a load
        fresh = Engine(0)
        try:
            with pytest.raises(EngineError) as ei:
                fresh.step_models(c["vels"], None, MINVEL, MAXVEL, nmodels=6)
            assert ei.value.code == ERR_STATE and "resident" in str(ei.value)
        finally:
            fresh.close()
        load()
        forward_steps(lib, c, None, nmodels=6, expect=ERR_STATE, **kw)
        assert b"resident" in lib.dsa_dropin_error()
        first = None
        for K in (6, 70):
            if K == 6:
                wk, dk = [m[0] for m in MEMBERS], [m[1] for m in MEMBERS]
            else:
                wk, dk = invert.tradeoff_grid(np.geomspace(0.25, 64.0, 14), [0.0, 0.3, 1.0, 2.5, 4.0])
            T = e.lsmr_tradeoff(S["b"], nd, 2.0, wk, dk)
            assert T["x"].shape == (K, n) and np.abs(T["x"]).max() > 1e-3
            res = forward_steps(lib, c, None, nmodels=K, **kw)
            res2 = forward_steps(lib, c, None, nmodels=K, **kw)                 # the forward call leaves the batch where it is
            host = forward_steps(lib, c, T["x"], **kw)
            assert same_results(res, host) and same_results(res2, host), K
            assert same_models(e.step_models(c["vels"], None, MINVEL, MAXVEL, nmodels=K), list(np.asarray(host["models"])))
            assert len(set(m.tobytes() for m in np.asarray(host["models"]))) > K // 2        # (the members differ: the comparison is not between equal things)
            if K == 6:
                first = host
                # wrong member count; a grid whose unknowns are not the matrix's columns
                forward_steps(lib, c, None, nmodels=5, expect=ERR_STATE, **kw)
                assert b"6 solutions" in lib.dsa_dropin_error()
                c4 = synth.boundary_case(nz=4)
                assert c4["nparpi"] == 270
                forward_steps(lib, c4, None, nmodels=6, expect=ERR_STATE)
                assert b"360 columns" in lib.dsa_dropin_error()
                back = forward_steps(lib, c, None, nmodels=6, **kw)                # a valid call afterwards: the earlier bits
                assert same_results(back, host)
        # cross-validation, x kept on the device, against a second run that returned it
        fold = (np.arange(nd) % 2).astype(np.int32)
        V0 = e.lsmr_crossval(S["b"], nd, 2.0, [2.0], [1.0], fold, 2, want_x=False, want_resid=False)
        assert V0["x"] is None
        res = forward_steps(lib, c, None, nmodels=3, obst=obst, w=w, group=fold, ngroups=2)
        V1 = e.lsmr_crossval(S["b"], nd, 2.0, [2.0], [1.0], fold, 2)
        host = forward_steps(lib, c, V1["x"], obst=obst, w=w, group=fold, ngroups=2)
        assert same_results(res, host)
        # the full member of (weight0, damp 1) is trade-off member 0
        assert (bits32(host["dsurf"][2]) == bits32(first["dsurf"][0])).all()
        # a Voronoi batch leaves solutions in cell space; a load or a new matrix leaves none
        xyz = np.stack(np.meshgrid(np.arange(c["nz"] - 1.0), np.arange(c["ny"] - 2.0), np.arange(c["nx"] - 2.0), indexing="ij"), -1).reshape(-1, 3)
        seeds = invert.voronoi_seeds(n, 20, 3, 1)
        e.lsmr_voronoi(S["b"][:nd], nd, 20, xyz, seeds, 1.0, want_cell=False, want_stats=False)
        forward_steps(lib, c, None, nmodels=3, expect=ERR_STATE, **kw)
        assert b"voronoi" in lib.dsa_dropin_error()
        T = e.lsmr_tradeoff(S["b"], nd, 2.0, [m[0] for m in MEMBERS], [m[1] for m in MEMBERS], want_x=False)
        assert same_results(forward_steps(lib, c, None, nmodels=6, **kw), first)
        load()
        forward_steps(lib, c, None, nmodels=6, expect=ERR_STATE, **kw)
        # host steps need no batch
        assert (forward_steps(lib, c, five_steps(c), **kw)["fails"] == 0).all()
    finally:
        e._h = None
    parity_log.add("dsa_forward_steps, steps = NULL after dsa_lsmr_tradeoff (6 and 70 members) and dsa_lsmr_crossval (x = NULL): models, times, sums, failures = the same steps from the host, bit for bit")


# ---- default mode, bundles across models -----------------------------------------------------------------------------------------

def test_default_mode_with_bundles_against_the_oracle():
    code = r'''
import sys, numpy as np, ctypes as C
sys.path.insert(0, %r); sys.path.insert(0, %r)
import _libs as L, synth
import test_gpu_forward_steps as T
from test_gpu_forward_models import with_model
from dsurftomo_amd import engine
lib = engine.load_library()
lib.dsa_dropin_engine.restype = C.c_void_p
lib.dsa_dropin_error.restype = C.c_char_p
c = synth.boundary_case(**T.BIG)
steps = T.five_steps(c)
def stats():
    st = np.zeros(64)
    assert lib.dsa_get_stats(C.c_void_p(lib.dsa_dropin_engine()), st.ctypes.data_as(C.c_void_p)) == 0
    return st
T.forward_steps(lib, c, steps[:1])
units1 = stats()[5]
models = T.host_models(lib, c, steps)
clips, lo, hi = T.bite(c, steps, None, models)
assert clips > 0 and lo > 0 and hi > 0, (clips, lo, hi)
ref = [L.call_boundary(L.oracle().dso_calsurfg, with_model(c, m))["dsurf"] for m in models]
obst, w, group = T.data_of(c, ref[0])
r = T.forward_steps(lib, c, steps, obst=obst, w=w, group=group, ngroups=4)
st = stats()
assert (r["fails"] == 0).all()
assert T.same_models(r["models"], models)
assert units1 > 0 and st[5] == 5 * units1, (units1, st[5])          # DSA_STAT_UNITS
assert st[26] == 4 and st[28] > 0, st[:30]                           # DSA_STAT_BUNDLE_SIZE, DSA_STAT_BUNDLED_UNITS
worst = 0.0
for k, o in enumerate(ref):
    assert np.isfinite(o).all() and (o > 0).all() and o.max() < 64.0
    d = float(np.abs(r["dsurf"][k] - o).max())
    print("model", k, "worst |dt|", d, "largest time", float(o.max()))
    worst = max(worst, d)
    assert d <= T.TOL, (k, d)
share = T.assert_measures(r["measures"], r["dsurf"], obst, w, group, 4)
blind = T.forward_steps(lib, c, steps, obst=obst, w=w, group=group, ngroups=4, dsurf=False, models=False)
assert (T.bits64(blind["measures"]) == T.bits64(r["measures"])).all()
print("bundled", int(st[28]), "of", int(st[5]), "units; worst", worst, "s; sums at", round(share, 3), "of their bound")
print("steps ok")
''' % (L.ROOT, os.path.join(L.ROOT, "tests"))
    env = dict(os.environ, DSA_BUNDLE="4")
    env.pop("DSA_EXACT_TIES", None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "steps ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    parity_log.add("dsa_forward_steps, 20 x 18 x 6 with stations, 5 step models, DSA_BUNDLE=4: " + "; ".join(l for l in r.stdout.splitlines() if l.startswith("bundled")) +
                   " against the oracle's CalSurfG per host-built model")


# ---- the Taipei example ----------------------------------------------------------------------------------------------------------

def test_nonlinear_members_on_taipei(tmp_path):
    code = r'''
import sys, os, numpy as np
sys.path.insert(0, %r)
from dsurftomo_amd import invert, io
out = %r
seen, args = [], []
inner = invert.iteration_device
def spy(*a, **kw):
    st = inner(*a, **kw)
    seen.append(st); args.append(np.array(a[3], copy=True))
    return st
invert.iteration_device = spy
c = io.load(io.HERE)
W0, nd = float(c["weight0"]), c["ndata"]
runs = {}
for tag, kw in (("plain", {}), ("trade", dict(tradeoff_weights=[W0, 2 * W0])), ("trade_nl", dict(tradeoff_weights=[W0, 2 * W0], tradeoff_nonlinear=True)),
                ("cv", dict(crossval=2, crossval_weights=[W0])), ("cv_nl", dict(crossval=2, crossval_weights=[W0], crossval_nonlinear=True))):
    d = os.path.join(out, tag)
    os.makedirs(d)
    del seen[:]; del args[:]
    log = []
    _, hist = invert.run(io.HERE, maxiter=2, out_dir=d, log=log.append, **kw)
    runs[tag] = (hist, list(seen), log, list(args))
name = "DSurfTomo.in"
def same_files(a, b, only=None):
    names = sorted(os.listdir(os.path.join(out, a))) if only is None else only
    assert len(names) >= 1
    for f in names:
        x = open(os.path.join(out, a, f), "rb").read()
        y = open(os.path.join(out, b, f), "rb").read()
        assert x == y and len(x) > 0, (a, b, f)
    return names
plain = same_files("plain", "trade_nl")
same_files("plain", "cv_nl")
assert len(plain) >= 5
same_files("trade", "trade_nl")
same_files("cv", "cv_nl")
assert sorted(set(os.listdir(os.path.join(out, "trade_nl"))) - set(os.listdir(os.path.join(out, "trade")))) == [name + "TradeoffNonlinear.dat"]
assert sorted(set(os.listdir(os.path.join(out, "cv_nl"))) - set(os.listdir(os.path.join(out, "cv")))) == [name + "CrossvalNonlinear.dat"]
for tag in ("plain", "trade", "cv"):
    assert not any("nonlinear" in l for l in runs[tag][2])
def rel(a, b):
    return abs(a - b) / b
tol = (nd + 8) * 2.0 ** -52          # the sum within (N + 4) 2^-52, then a division and a square root: half of it and two roundings
# trade-off: member (W0, damp) is the step the run takes, its model the model of iteration 2
hist, sts, log, obs = runs["trade_nl"]
nl = hist[0]["tradeoff_nonlinear"]
rows = io.read_tradeoff_nonlinear(os.path.join(out, "trade_nl", name + "TradeoffNonlinear.dat"))
assert rows == nl["members"] and len(rows) == 2 and [r["weight"] for r in rows] == [W0, 2 * W0]
a = np.ascontiguousarray(nl["dsyn"][0]).view(np.uint32)
b = np.ascontiguousarray(sts[1]["dsyn"]).view(np.uint32)
assert a.size == b.size == nd and (a == b).all(), int((a != b).sum())
assert (np.ascontiguousarray(nl["dsyn"][1]).view(np.uint32) != b).any()
want = invert.nonlinear_measures(obs[0], sts[1]["dsyn"], sts[0]["datweight"])[0, 0]
assert rel(rows[0]["weighted_rms"], np.sqrt(want[0] / nd)) <= tol and rel(rows[0]["rms"], np.sqrt(want[1] / nd)) <= tol
assert all(r["disp_failures"] == 0 for r in rows)
assert rel(rows[0]["predicted_rms"], hist[0]["tradeoff"]["members"][0]["misfit"] / np.sqrt(nd)) <= 1e-15
assert "tradeoff_nonlinear" not in hist[1] and sum("tradeoff nonlinear" in l for l in log) == 2
print("tradeoff", [(r["weight"], r["predicted_rms"], r["weighted_rms"], r["rms"]) for r in rows])
# cross-validation: the full member of (W0, damp)
hist, sts, log, obs = runs["cv_nl"]
nl = hist[0]["crossval_nonlinear"]
rows = io.read_crossval_nonlinear(os.path.join(out, "cv_nl", name + "CrossvalNonlinear.dat"))
assert rows == nl["members"] and len(rows) == 1 and rows[0]["weight"] == W0 and nl["resident"] and nl["calls"] == 1
assert nl["dsyn"].shape == (3, nd)
a = np.ascontiguousarray(nl["dsyn"][2]).view(np.uint32)
b = np.ascontiguousarray(sts[1]["dsyn"]).view(np.uint32)
assert (a == b).all(), int((a != b).sum())
want = invert.nonlinear_measures(obs[0], sts[1]["dsyn"], sts[0]["datweight"])[0, 0]
assert rel(rows[0]["full_rms"], np.sqrt(want[0] / nd)) <= tol
fold = invert.crossval_folds(c, 2, "datum", 1)
held = invert.nonlinear_measures(obs[0], nl["dsyn"][:2], sts[0]["datweight"], fold, 2)
assert rel(rows[0]["heldout_rms"], np.sqrt((held[0, 0, 0] + held[1, 1, 0]) / nd)) <= tol
assert rows[0]["cv_rms"] == hist[0]["crossval"]["members"][0]["cv_rms"] and rows[0]["disp_failures"] == 0
assert sum("crossval nonlinear" in l for l in log) == 2
print("crossval", [(r["weight"], r["heldout_rms"], r["full_rms"], r["cv_rms"]) for r in rows])
print("nonlinear ok")
''' % (L.ROOT, str(tmp_path))
    env = dict(os.environ, DSA_EXACT_TIES="2")
    env.pop("DSA_BUNDLE", None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "nonlinear ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    parity_log.add("nonlinear members on Taipei (exact_ties 2): " + "; ".join(l for l in r.stdout.splitlines() if l.startswith(("tradeoff", "crossval"))))
