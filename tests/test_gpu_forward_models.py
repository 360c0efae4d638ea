"""K Vs models forward-modelled in one call (dsa_dispersion_begin_models, dsa_forward_models) and the step-length line search on top.

* dispersion stage with a model dimension: model k's maps of the batched launch are bit-identical to a single-model begin / run /
  fetch, also when the batch runs at another group width than the single model (32 x 132 = 4 224 curves: 4 lanes per curve where
  the single model's 132 curves run 8 lanes each);
* dsa_forward_models under exact_ties = 2: column k is bit-identical to dsa_calsurfg's dsurf (dicing 8) / dsa_synthetic's times
  (dicing 5) on model k alone, whatever the pass size; padding rows of dsurf stay untouched;
* default mode with bundles across models: every time within 1e-4 s of the oracle's CalSurfG on its model;
* argument errors leave the engine usable;
* python -m dsurftomo_amd.invert --line-search on the Taipei example.

The four models are synth.boundary_case()'s scaled by 1, 0.94, 1.06 and 1 + 0.05 sin(3.1 i/nx) cos(2.3 j/ny).
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

pytestmark = pytest.mark.gpu
TOL = 1e-4
ERR_ARGUMENT, ERR_STATE = -2, -5
GROUPS = dict(kRc=0, kRg=2, kLc=0, kLg=1)
BIG = dict(nx=20, ny=18, nz=6, nsrc=8, nrcf=7, kRc=3, kRg=1, kLc=1, kLg=1, stations=True)


def models_of(c):
    """the four test models of a boundary case, each (nx, ny, nz) float32 in Fortran order"""
    nx, ny = c["nx"], c["ny"]
    i = np.arange(nx, dtype=np.float64)[:, None, None]
    j = np.arange(ny, dtype=np.float64)[None, :, None]
    factors = (1.0, 0.94, 1.06, 1.0 + 0.05 * np.sin(3.1 * i / nx) * np.cos(2.3 * j / ny))
    return [np.asfortranarray((c["vels"].astype(np.float64) * f).astype(np.float32)) for f in factors]


def stacked(models):
    """(K, nz, ny, nx): the C order of Fortran vels(nx, ny, nz, K)"""
    return np.ascontiguousarray(np.stack([m.transpose(2, 1, 0) for m in models]), np.float32)


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- 1. dispersion stage, engine level -----------------------------------------------------------------------------------------

def _runs(c):
    """(iwave, igr, periods, first map): the four wave types into distinct maps"""
    out, m = [], 0
    for iwave, igr, t in ((2, 0, c["tRc"]), (2, 1, c["tRg"]), (1, 0, c["tLc"]), (1, 1, c["tLg"])):
        out.append((iwave, igr, t, m))
        m += len(t)
    return out, m


@pytest.fixture(scope="module")
def single_maps(engine):
    """maps of each of the four models computed alone: (4, nmaps, ncol) float64; computed once, never changed"""
    c = synth.boundary_case()
    runs, nmaps = _runs(c)
    out = []
    for m in models_of(c):
        engine.dispersion_begin(m.transpose(2, 1, 0), c["depz"], c["minthk"], nmaps, nmaps)
        for iwave, igr, t, first in runs:
            engine.dispersion_run(iwave, igr, t, False, 0, first)
        assert engine.stats()["curves"] == c["nx"] * c["ny"] * len(runs)
        out.append(engine.dispersion_fetch(0, nmaps))
    out = np.stack(out)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("K", [4, 32])
def test_dispersion_of_k_models_equals_one_model_at_a_time(engine, single_maps, K):
    c = synth.boundary_case()
    runs, nmaps = _runs(c)
    ncol = c["nx"] * c["ny"]
    assert ncol == 132
    four = models_of(c)
    engine.dispersion_begin_models(stacked([four[k % 4] for k in range(K)]), c["depz"], c["minthk"], nmaps)
    for iwave, igr, t, first in runs:
        engine.dispersion_run(iwave, igr, t, False, 0, first)
    # one launch per run over all models: K * ncol curves each
    assert engine.stats()["curves"] == K * ncol * len(runs)
    if K == 32:
        assert ncol <= 4096 < K * ncol <= 32768          # 8 lanes per curve alone, 4 in the batch (Engine::dispersion_run)
    assert (engine.dispersion_model_failures(K) == 0).all()
    assert np.isfinite(single_maps).all() and (single_maps > 0).all()
    for k in range(K):
        pv = engine.dispersion_fetch(k * nmaps, nmaps)
        assert (bits64(pv) == bits64(single_maps[k % 4])).all(), (K, k)
    # models differ: the comparison above is not between equal things
    assert np.abs(single_maps[1] - single_maps[0]).min() > 1e-3
    parity_log.add(f"dispersion of {K} models in one launch per wave type ({K * ncol} curves): all {K * nmaps} maps = the single-model runs, bit for bit")


def test_forced_group_widths_give_the_same_bits(engine, single_maps):
    c = synth.boundary_case()
    runs, nmaps = _runs(c)
    four = models_of(c)
    try:
        for shift in (0, 1, 2, 3):
            engine.set_option("disp_group_shift", shift)
            engine.dispersion_begin_models(stacked(four), c["depz"], c["minthk"], nmaps)
            for iwave, igr, t, first in runs:
                engine.dispersion_run(iwave, igr, t, False, 0, first)
            pv = engine.dispersion_fetch(0, 4 * nmaps).reshape(4, nmaps, -1)
            assert (bits64(pv) == bits64(single_maps)).all(), shift
    finally:
        engine.set_option("disp_group_shift", -1)


def test_one_model_is_dispersion_begin_and_kernels_need_one_model(engine):
    from dsurftomo_amd.engine import EngineError
    c = synth.boundary_case()
    four = models_of(c)
    t, n = c["tRc"], len(c["tRc"])
    engine.dispersion_begin(four[3].transpose(2, 1, 0), c["depz"], c["minthk"], n, n)
    engine.dispersion_run(2, 0, t, True, 0, 0)
    want = engine.dispersion_fetch(0, n, kernels=True)
    engine.dispersion_begin_models(stacked(four[3:]), c["depz"], c["minthk"], n)
    engine.dispersion_run(2, 0, t, True, 0, 0)
    got = engine.dispersion_fetch(0, n, kernels=True)
    for a, b in zip(want, got):
        assert (bits64(a) == bits64(b)).all()
    assert np.abs(want[1]).max() > 0
    engine.kernels_from_dispersion()
    # more than one model: no depth kernels
    engine.dispersion_begin_models(stacked(four), c["depz"], c["minthk"], n)
    with pytest.raises(EngineError) as ei:
        engine.dispersion_run(2, 0, t, True, 0, 0)
    assert ei.value.code == ERR_ARGUMENT
    engine.dispersion_run(2, 0, t, False, 0, 0)
    with pytest.raises(EngineError) as ei:
        engine.kernels_from_dispersion()
    assert ei.value.code == ERR_STATE
    assert (engine.dispersion_model_failures(4) == 0).all()
    with pytest.raises(EngineError) as ei:
        engine.dispersion_begin_models(np.zeros((0, c["nz"], c["ny"], c["nx"]), np.float32), c["depz"], c["minthk"], n)
    assert ei.value.code == ERR_ARGUMENT


def test_diagnostics_count_over_all_models(engine):
    """dsa_dispersion_diagnostics counts over all models and agrees with the per-model counts: every curve of these models has a root"""
    c = synth.boundary_case()
    four = models_of(c)
    runs, nmaps = _runs(c)
    engine.dispersion_begin_models(stacked(four), c["depz"], c["minthk"], nmaps)
    for iwave, igr, t, first in runs:
        engine.dispersion_run(iwave, igr, t, False, 0, first)
    cnt = C.c_longlong(-1)
    first = (C.c_int * 5)()
    per = C.c_double(0)
    lib = engine._L
    lib.dsa_dispersion_diagnostics.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.dsa_dispersion_diagnostics(engine._h, C.byref(cnt), first, C.byref(per)) == 0
    assert cnt.value == int(engine.dispersion_model_failures(4).sum()) == 0


# ---- 2. drop-in entry under exact_ties = 2 -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dropin():
    from dsurftomo_amd import build, engine as E
    build.build()
    lib = E.load_library()
    lib.dsa_dropin_engine.restype = C.c_void_p
    lib.dsa_dropin_error.restype = C.c_char_p
    h = lib.dsa_dropin_engine()
    assert h, lib.dsa_dropin_error()
    return lib, C.c_void_p(h)


@pytest.fixture()
def exact2(dropin):
    """the drop-in engine with exact_ties = 2 (every unit by the reference's march), put back afterwards"""
    lib, h = dropin
    assert lib.dsa_set_option(h, b"exact_ties", C.c_double(2)) == 0
    yield lib, h
    assert lib.dsa_set_option(h, b"exact_ties", C.c_double(1)) == 0
    assert lib.dsa_set_option(h, b"forward_models_chunk", C.c_double(0)) == 0
    assert lib.dsa_set_option(h, b"forward_models_order", C.c_double(0)) == 0


def forward_models(lib, c, models, dicing, ldd=None, fill=0.0, expect=0):
    from dsurftomo_amd import io
    K = len(models)
    ldd = c["ndata"] if ldd is None else ldd
    vels = stacked(models) if K else np.zeros(1, np.float32)
    dsurf = np.full((max(K, 1), max(ldd, 1)), fill, np.float32)
    fails = np.full(max(K, 1), -1, np.int64)
    i32 = lambda v: C.byref(C.c_int(int(v)))
    _, tail = io._args(c)
    rc = lib.dsa_forward_models(i32(c["nx"]), i32(c["ny"]), i32(c["nz"]), i32(K), L.ptr(vels), L.ptr(dsurf), i32(ldd), i32(dicing), L.ptr(fails), *tail)
    assert rc == expect, (rc, lib.dsa_dropin_error())
    return dsurf, fails


def with_model(c, m):
    cc = dict(c)
    cc["vels"] = m
    return cc


_SINGLE = {}


def single_model_times(lib, name, kw):
    """per model: dsa_calsurfg's dsurf and dsa_synthetic's times (noise 0) under exact_ties = 2; computed once per case"""
    if name not in _SINGLE:
        c = synth.boundary_case(**kw)
        cal, syn = [], []
        for m in models_of(c):
            cal.append(L.call_boundary(lib.dsa_calsurfg, with_model(c, m))["dsurf"])
            syn.append(L.call_boundary(lib.dsa_synthetic, with_model(c, m), synthetic=True))
        cal, syn = np.stack(cal), np.stack(syn)
        cal.setflags(write=False); syn.setflags(write=False)
        _SINGLE[name] = (cal, syn)
    return _SINGLE[name]


@pytest.mark.parametrize("name,kw", [("default", {}), ("groups", GROUPS)])
def test_forward_models_columns_equal_the_single_model_calls(exact2, name, kw):
    lib, h = exact2
    c = synth.boundary_case(**kw)
    four = models_of(c)
    nd = c["ndata"]
    cal, syn = single_model_times(lib, name, kw)
    assert np.isfinite(cal).all() and (cal > 0).all() and np.abs(cal[1] - cal[0]).max() > 0.01
    for dicing, want in ((8, cal), (5, syn)):
        got, fails = forward_models(lib, c, four, dicing)
        assert (fails == 0).all()
        assert (bits32(got) == bits32(want)).all(), (name, dicing, float(np.abs(got - want).max()))
        # one model
        for k in (0, 3):
            one, f1 = forward_models(lib, c, four[k:k + 1], dicing)
            assert f1[0] == 0 and (bits32(one[0]) == bits32(want[k])).all(), (name, dicing, k)
        # passes of 3 + 1 models
        assert lib.dsa_set_option(h, b"forward_models_chunk", C.c_double(3)) == 0
        split, fs = forward_models(lib, c, four, dicing)
        assert lib.dsa_set_option(h, b"forward_models_chunk", C.c_double(0)) == 0
        assert (fs == 0).all() and (bits32(split) == bits32(got)).all(), (name, dicing)
        # the other unit order gives the same bits (every unit is marched on its own)
        assert lib.dsa_set_option(h, b"forward_models_order", C.c_double(1)) == 0
        other, _ = forward_models(lib, c, four, dicing)
        assert lib.dsa_set_option(h, b"forward_models_order", C.c_double(0)) == 0
        assert (bits32(other) == bits32(got)).all(), (name, dicing)
        # ldd above the number of data: the rows beyond stay as they were
        pad, _ = forward_models(lib, c, four, dicing, ldd=nd + 5, fill=-7.0)
        assert (bits32(pad[:, :nd]) == bits32(want)).all() and (pad[:, nd:] == -7.0).all()
    # model 0's maps are the ones served afterwards, also after passes (the pass holding model 0 runs last)
    which = 1 if name == "groups" else 0
    n = c["kRg"] if name == "groups" else c["kRc"]
    ncol = c["nx"] * c["ny"]
    forward_models(lib, with_model(c, four[0]), four[:1], 5)
    pv0 = np.zeros((n, ncol))
    assert lib.dsa_dropin_velocity_maps(C.byref(C.c_int(which)), L.ptr(pv0)) == 0
    assert lib.dsa_set_option(h, b"forward_models_chunk", C.c_double(3)) == 0
    forward_models(lib, c, four, 5)
    assert lib.dsa_set_option(h, b"forward_models_chunk", C.c_double(0)) == 0
    pv = np.zeros((n, ncol))
    assert lib.dsa_dropin_velocity_maps(C.byref(C.c_int(which)), L.ptr(pv)) == 0
    assert (bits64(pv) == bits64(pv0)).all() and (pv0 > 0).all()
    parity_log.add(f"dsa_forward_models, case {name}, exact_ties 2: 4 models x {nd} data = dsa_calsurfg / dsa_synthetic per model, bit for bit (one call, one model, passes of 3 + 1, both unit orders)")


# ---- 4. errors ------------------------------------------------------------------------------------------------------------------

def test_argument_errors_leave_the_engine_usable(exact2):
    lib, h = exact2
    c = synth.boundary_case()
    four = models_of(c)
    cal, _ = single_model_times(lib, "default", {})
    forward_models(lib, c, [], 8, expect=ERR_ARGUMENT)                          # nmodels < 1
    forward_models(lib, c, four, 8, ldd=c["ndata"] - 1, expect=ERR_ARGUMENT)    # ldd below the number of data
    for dicing in (0, 4, 6, 16):
        forward_models(lib, c, four, dicing, expect=ERR_ARGUMENT)
    assert b"dicing" in lib.dsa_dropin_error()
    from dsurftomo_amd import io
    i32 = lambda v: C.byref(C.c_int(int(v)))
    _, tail = io._args(c)
    vels = stacked(four)
    dsurf = np.zeros((4, c["ndata"]), np.float32)
    head = [i32(c["nx"]), i32(c["ny"]), i32(c["nz"]), i32(4), L.ptr(vels), L.ptr(dsurf), i32(c["ndata"]), i32(8), None]
    for pos in (4, 5, 6, 7):                                                    # vels, dsurf, ldd, dicing
        bad = list(head)
        bad[pos] = None
        assert lib.dsa_forward_models(*bad, *tail) == ERR_ARGUMENT
    bad_tail = list(tail)
    bad_tail[15] = None                                                         # depz
    assert lib.dsa_forward_models(*head, *bad_tail) == ERR_ARGUMENT
    assert (dsurf == 0).all()
    # disp_failures may be null; a valid call afterwards gives the bits of the single-model calls
    assert lib.dsa_forward_models(*head, *tail) == 0, lib.dsa_dropin_error()
    assert (bits32(dsurf) == bits32(cal)).all()


# ---- 3. default mode, bundles across models ------------------------------------------------------------------------------------

def test_default_mode_with_bundles_against_the_oracle():
    code = r'''
import sys, numpy as np, ctypes as C
sys.path.insert(0, %r); sys.path.insert(0, %r)
import _libs as L, synth
import test_gpu_forward_models as T
from dsurftomo_amd import engine
lib = engine.load_library()
lib.dsa_dropin_engine.restype = C.c_void_p
lib.dsa_dropin_error.restype = C.c_char_p
c = synth.boundary_case(**T.BIG)
four = T.models_of(c)
def stats():
    st = np.zeros(64)
    assert lib.dsa_get_stats(C.c_void_p(lib.dsa_dropin_engine()), st.ctypes.data_as(C.c_void_p)) == 0
    return st
one, _ = T.forward_models(lib, c, four[:1], 8)
units1 = stats()[5]
got, fails = T.forward_models(lib, c, four, 8)
st = stats()
assert (fails == 0).all()
assert units1 > 0 and st[5] == 4 * units1, (units1, st[5])          # DSA_STAT_UNITS
assert st[26] == 4 and st[28] > 0, st[:30]                           # DSA_STAT_BUNDLE_SIZE, DSA_STAT_BUNDLED_UNITS
worst = 0.0
for k, m in enumerate(four):
    o = L.call_boundary(L.oracle().dso_calsurfg, T.with_model(c, m))["dsurf"]
    assert np.isfinite(o).all() and o.max() < 64.0
    d = float(np.abs(got[k] - o).max())
    print("model", k, "worst |dt|", d, "largest time", float(o.max()))
    worst = max(worst, d)
    assert d <= T.TOL, (k, d)
print("bundled", int(st[28]), "of", int(st[5]), "units; worst", worst)
print("models ok")
''' % (L.ROOT, os.path.join(L.ROOT, "tests"))
    env = dict(os.environ, DSA_BUNDLE="4")
    env.pop("DSA_EXACT_TIES", None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "models ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    parity_log.add("dsa_forward_models, 20 x 18 x 6 with stations, 4 models, DSA_BUNDLE=4: " + "; ".join(l for l in r.stdout.splitlines() if l.startswith("bundled")) + " s against the oracle's CalSurfG per model")


# ---- 5. line search on the Taipei example --------------------------------------------------------------------------------------

def test_line_search_on_taipei(tmp_path):
    code = r'''
import sys, os, numpy as np
sys.path.insert(0, %r)
from dsurftomo_amd import invert, io
out = %r
seen = []
inner = invert.iteration_device
def spy(*a, **kw):
    st = inner(*a, **kw)
    seen.append(st)
    return st
invert.iteration_device = spy
runs = {}
for tag, ls in (("plain", None), ("one", [1.0]), ("three", [0.0, 0.5, 1.0])):
    d = os.path.join(out, tag)
    os.makedirs(d)
    del seen[:]
    log = []
    _, hist = invert.run(io.HERE, maxiter=2, out_dir=d, log=log.append, line_search=ls)
    runs[tag] = (hist, list(seen), log)
name = "DSurfTomo.in"
for f in ("Measure.dat.iter001", "Measure.dat.iter002", "Measure.dat"):
    a = open(os.path.join(out, "plain", name + f), "rb").read()
    b = open(os.path.join(out, "one", name + f), "rb").read()
    assert a == b and len(a) > 1000, f
assert not os.path.exists(os.path.join(out, "plain", name + "LineSearch.dat"))
assert "line_search" not in runs["plain"][0][0] and not any("line search" in l for l in runs["plain"][2])
hist, sts, log = runs["three"]
rows = io.read_line_search(os.path.join(out, "three", name + "LineSearch.dat"))
assert len(rows) == 6 and [r["iteration"] for r in rows] == [1, 1, 1, 2, 2, 2] and [r["alpha"] for r in rows] == [0.0, 0.5, 1.0] * 2
for it in (1, 2):
    rr = [r for r in rows if r["iteration"] == it]
    assert sum(r["chosen"] for r in rr) == 1 and all(r["disp_failures"] == 0 for r in rr)
    chosen = [r for r in rr if r["chosen"]][0]
    assert chosen["weighted_rms"] == min(r["weighted_rms"] for r in rr)
    assert hist[it - 1]["line_search"]["alpha"] == chosen["alpha"]
    print("iteration", it, "scores", [r["weighted_rms"] for r in rr], "chosen", chosen["alpha"])
assert rows[0]["weighted_rms"] == hist[0]["rms"], (rows[0]["weighted_rms"], hist[0]["rms"])
assert ("%%8.3f" %% rows[0]["weighted_rms"]) in [l for l in log if "rms of residual" in l][0]
ls1 = sts[0]["line_search"]
a = np.ascontiguousarray(ls1["dsyn"][ls1["chosen"]]).view(np.uint32)
b = np.ascontiguousarray(sts[1]["dsyn"]).view(np.uint32)
assert a.size == b.size == 2061 and (a == b).all(), int((a != b).sum())
assert sum("line search" in l for l in log) == 2
print("line search ok")
''' % (L.ROOT, str(tmp_path))
    env = dict(os.environ, DSA_EXACT_TIES="2")
    env.pop("DSA_BUNDLE", None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "line search ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    parity_log.add("line search on Taipei (exact_ties 2): " + "; ".join(l for l in r.stdout.splitlines() if l.startswith("iteration")))
