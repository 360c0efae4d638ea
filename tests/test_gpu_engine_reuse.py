"""Engine reuse: whatever an engine did before, a workload that states all its own inputs and settings returns, bit
for bit, what a fresh engine returns.  The engine keeps some fifty state flags and dozens of buffers that only ever grow; this file runs the
families of entry points (tests/reuse_workloads.py) after one another on one engine -- stale data behind a shrunken shape, a mark, flag or
pool that survives a stage change, an error path that leaves half a result behind all show as a changed bit.

  * expected bits: every (workload, shape) on a fresh engine of its own, twice, the two identical (the workload is reproducible at all);
    the engine under test never supplies them;
  * test_pairs[A-B], for every B behind A in the list: A.big, B.small, A.big on one fresh engine -- every unordered pair in both
    directions.  One item per pair, not per A: an item per A took up to 3.7 s, five times the suite's yardstick;
  * test_same_kind[A]: big, big, small, big, small, small;
  * test_long_walk: one engine, a seeded walk of 150 steps, every (workload, shape) at least three times, in fifteen items of 10 steps that
    continue each other on that engine;
  * the drop-in's process-wide engine through its own entries, big, small, big, against its first answers and against an engine of the
    test's own running the calls those entries make;
  * the schedules themselves, on the CPU.

An unexpected EngineError fails the item where it is raised: nothing more is started on that engine."""
import collections

import numpy as np
import pytest

import _libs as L
import reuse_workloads as W
from dsurftomo_amd import io
from dsurftomo_amd.engine import Engine, declare_solvers, load_library

SEGMENTS = list(range(0, W.WALK_STEPS, W.WALK_SEGMENT))          # first steps of the long walk's items


def fresh(name, shape):
    e = Engine(0)
    try:
        return W.run(name, shape, e)
    finally:
        e.close()


class Expected:
    """the expected bits of a (workload, shape): its arrays on a fresh engine of its own, computed when first asked for -- twice, and the two
    must not differ in a bit (the workload is reproducible at all) -- and kept unchanged for the module"""

    def __init__(self):
        self.kept = {}

    def __getitem__(self, key):
        if key not in self.kept:
            first = fresh(*key)
            d = W.difference(fresh(*key), first)
            assert d is None, "%s.%s is not reproducible on fresh engines: %s differs in %d of %d elements" % (key + d)
            self.kept[key] = first
        return self.kept[key]


@pytest.fixture(scope="module")
def expected():
    return Expected()


def walk(e, steps, expected, first=0, last=None):
    """steps[first:last] of (workload, shape) on the engine e, each against the expected bits; a failure names the step, the five before
    it, the first field that differs and how many of its elements do"""
    for k in range(first, len(steps) if last is None else last):
        name, shape = steps[k]
        want = expected[name, shape]
        d = W.difference(W.run(name, shape, e), want)
        if d is not None:
            before = " -> ".join("%s.%s" % s for s in steps[max(k - 5, 0):k]) or "a fresh engine"
            pytest.fail("step %d, %s.%s after %s: %s differs from a fresh engine's in %d of %d elements" % ((k, name, shape, before) + d))


def walk_fresh(steps, expected):
    e = Engine(0)
    try:
        walk(e, steps, expected)
    finally:
        e.close()


# ---- the schedules, on the CPU ---------------------------------------------------------------------------------------------------------------

def test_schedules_cover_what_they_claim():
    """the pair schedules together hold every ordered pair of different workloads as two consecutive steps -- A.big -> B.small and
    B.small -> A.big for A before B in the list --; the walk visits every (workload, shape) at least three times, it is the same walk every
    time, and its segments are the whole of it"""
    n = len(W.NAMES)
    assert n == len(set(W.NAMES)) >= 16 and set(W.RUN) == set(W.NAMES) and len(W.PAIRS) == len(set(W.PAIRS)) == n * (n - 1) // 2
    seen = set()
    for a, b in W.PAIRS:
        steps = W.pair_schedule(a, b)
        assert steps == [(a, "big"), (b, "small"), (a, "big")] and a != b
        seen |= set(zip(steps, steps[1:]))
    assert {(p[0], q[0]) for p, q in seen} == {(a, b) for a in W.NAMES for b in W.NAMES if a != b}
    steps = W.walk_schedule()
    count = collections.Counter(steps)
    assert len(steps) == W.WALK_STEPS == 150 and set(count) == {(n, s) for n in W.NAMES for s in W.SHAPES} and min(count.values()) >= 3
    assert steps == W.walk_schedule()
    assert len({(a, b) for a, b in zip(steps, steps[1:])}) > 120                 # (a walk, not a cycle: nearly every transition is another one)
    assert [k for first in SEGMENTS for k in range(first, min(first + W.WALK_SEGMENT, len(steps)))] == list(range(len(steps)))
    assert W.SAME_KIND == ("big", "big", "small", "big", "small", "small")


def test_difference_names_the_field_and_the_count():
    a = dict(x=np.arange(6, dtype=np.float32), y=np.zeros((2, 3)))
    b = dict(x=a["x"].copy(), y=a["y"].copy())
    assert W.difference(a, b) is None
    b["y"][1, 1:] = -0.0                                                         # equal as numbers, not as bytes
    assert W.difference(a, b) == ("y", 2, 6)
    b["x"] = b["x"].astype(np.float64)
    assert W.difference(a, b)[0].startswith("x (float32")
    assert W.difference(dict(x=a["x"][:5]), dict(x=a["x"]))[0].startswith("x (")
    assert W.difference(dict(x=a["x"]), dict(z=a["x"]))[0].startswith("the fields")


# ---- on the device -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("a,b", W.PAIRS, ids=["%s-%s" % p for p in W.PAIRS])
def test_pairs(expected, a, b):
    """one item per unordered pair (per workload A the items A-B of every B behind it): A.big, B.small, A.big on one fresh engine"""
    walk_fresh(W.pair_schedule(a, b), expected)


@pytest.mark.gpu
@pytest.mark.parametrize("a", W.NAMES)
def test_same_kind(expected, a):
    """the same call twice, shrink, grow"""
    walk_fresh([(a, shape) for shape in W.SAME_KIND], expected)


@pytest.fixture(scope="module")
def walker():
    """the one engine of the long walk and how far it has come; `dead`: why nothing more is started on it"""
    w = dict(engine=None, done=0, dead=None)
    yield w
    if w["engine"] is not None:
        w["engine"].close()


@pytest.mark.gpu
@pytest.mark.parametrize("first", SEGMENTS)
def test_long_walk(expected, walker, first):
    """one engine, 150 seeded steps, in items of 10 steps that continue each other (an item run alone walks the steps before it first):
    histories of three and more stages, such as radial stage -> sampler -> plain stage"""
    steps = W.walk_schedule()
    if walker["dead"]:
        pytest.fail("nothing more is started on the walk's engine after %s" % walker["dead"])
    if walker["engine"] is None or walker["done"] > first:
        if walker["engine"] is not None:
            walker["engine"].close()
        walker.update(engine=Engine(0), done=0)
    last = min(first + W.WALK_SEGMENT, len(steps))
    try:
        walk(walker["engine"], steps, expected, walker["done"], last)
    except BaseException as exc:
        walker["dead"] = "the item of step %d failed (%s)" % (first, type(exc).__name__)
        raise
    walker["done"] = last


def same_call(got, want, what):
    for k in ("dsurf", "rw", "iw", "col"):
        d = W.difference({k: np.ascontiguousarray(got[k])}, {k: np.ascontiguousarray(want[k])})
        assert d is None, "%s: %s differs in %d of %d elements" % ((what,) + d)
    assert got["nar"] == want["nar"] > 0


@pytest.mark.gpu
def test_dropin_boundary(expected):
    """dropin.hip's process-wide engine, reachable through its entries only, and in whatever state the tests before this one left it:
    dsa_calsurfg big, small, big, the same with dsa_calsurfg_azimuthal, dsa_forward_models and dsa_forward_steps, every answer the first
    one of its shape -- and the answer of an engine of the test's own that makes the calls the entry makes (workloads `rows`,
    `forward_models`; for the azimuthal entry the isotropic calls with dsa_solve_rows_azimuthal under the Rayleigh mask)"""
    import ctypes as C
    lib = declare_solvers(load_library())
    eng = lib.dsa_dropin_engine()
    assert eng
    for k, v in W.DEFAULTS.items():                                              # (options are sticky and not under test)
        assert lib.dsa_set_option(eng, k.encode(), C.c_double(v)) == 0, k
    case = {s: W.boundary(s) for s in W.SHAPES}
    order = ("big", "small", "big")

    def azimuthal(c):
        nd, npar = c["ndata"], c["nparpi"]
        cap = 3 * nd * npar + 1
        iw = np.zeros(cap + 1, np.int32); rw = np.zeros(cap, np.float32); col = np.zeros(cap, np.int32); dsurf = np.zeros(nd, np.float32)
        nar = C.c_int(0)
        head, tail = io._args(c)
        lib.dsa_dropin_set_capacity(cap)
        try:
            rc = lib.dsa_calsurfg_azimuthal(*head, L.ptr(iw), L.ptr(rw), L.ptr(col), L.ptr(dsurf), *tail, C.byref(nar))
        finally:
            lib.dsa_dropin_set_capacity(0)
        assert rc == 0, lib.dsa_dropin_error().decode()
        n = nar.value
        return dict(dsurf=dsurf, nar=n, rw=rw[:n].copy(), iw=iw[1:n + 1].copy(), col=col[:n].copy())

    first = {}
    for entry, call in (("dsa_calsurfg", lambda c: L.call_boundary(lib.dsa_calsurfg, c)), ("dsa_calsurfg_azimuthal", azimuthal)):
        for shape in order:
            got = call(case[shape])
            same_call(got, first.setdefault((entry, shape), got), "%s %s again" % (entry, shape))
    # the engine-level calls of the same cases
    for shape in W.SHAPES:
        c, d = case[shape], first["dsa_calsurfg", shape]
        want = expected["rows", shape]
        same_call(d, dict(dsurf=want["times"], rw=want["rw"], iw=want["iw"], col=want["col"], nar=want["rw"].size), "dsa_calsurfg %s against an engine's own calls" % shape)
        e = Engine(0)
        try:
            W.stage_rows(e, c)
            on = np.ones(c["kmax"], np.int32); on[c["layout"]["sLc"]:] = 0
            e.set_azimuthal_slots(on)
            t, rw, iw, col = e.solve_rows_azimuthal(W.capacity(c, 3))
        finally:
            e.close()
        same_call(first["dsa_calsurfg_azimuthal", shape], dict(dsurf=t, rw=rw, iw=iw, col=col, nar=rw.size), "dsa_calsurfg_azimuthal %s against an engine's own calls" % shape)
    # the forward entries: K models given, and K models stepped on the device from given steps
    models = {s: [np.asfortranarray((np.asarray(case[s]["vels"], np.float32) * np.float32(1.0 + 0.015 * k)).astype(np.float32)) for k in range(3 if s == "big" else 1)]
              for s in W.SHAPES}
    steps = {s: (0.05 * (W.SM.mix(np.arange((3 if s == "big" else 1) * case[s]["nparpi"]), 17) - 0.5)).astype(np.float32).reshape(-1, case[s]["nparpi"]) for s in W.SHAPES}
    for shape in order:
        c = case[shape]
        t, fails = io.call_forward_models(c, models[shape], lib=lib)
        got = dict(times=np.ascontiguousarray(t), failures=fails)
        d = W.difference(got, first.setdefault(("dsa_forward_models", shape), got))
        assert d is None, "dsa_forward_models %s again: %s differs in %d of %d elements" % ((shape,) + d)
        d = W.difference(dict(times=got["times"]), dict(times=expected["forward_models", shape]["times"]))
        assert d is None, "dsa_forward_models %s against an engine's own calls: %s differs in %d of %d elements" % ((shape,) + d)
        r = io.call_forward_steps(c, c["vels"], steps[shape], obst=(t[0] * W.factors(c["ndata"], 96)).astype(np.float32), want_models=True, lib=lib)
        got = {k: np.ascontiguousarray(v) for k, v in r.items() if v is not None}
        assert got["dsurf"].size > 0 and (got["dsurf"] > 0).all() and got["measures"].any()
        d = W.difference(got, first.setdefault(("dsa_forward_steps", shape), got))
        assert d is None, "dsa_forward_steps %s again: %s differs in %d of %d elements" % ((shape,) + d)
