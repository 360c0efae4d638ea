"""Every launch shape of the unit-by-unit fixed-point solve (csrc/fim_kernel.hip) on small grids, bit for bit against the oracle.

Engine::launch_shape picks the workgroup size from the grid alone (128 threads up to 700 nodes per side ... 1024 beyond 3000), so without the
option fim_threads the 256-, 512- and 1024-thread kernels only ever run on grids too large to compare in every bit.  Here each of them solves
the units of tests/golden/solve_units.json -- units without exact ties, whose fixed point IS the oracle's Fast Marching field whatever the
schedule (tests/solve_units.py, checked on the CPU by tests/test_solve_units.py) -- on 121^2, 161^2, 257^2 and 121 x 257 nodes, with
bundle = 0 (stats()["bundles"] == 0: the unit-by-unit kernels are what runs) and, unless stated, exact_ties = 0 (nothing is marched: the
fixed-point kernels' own output is what is compared).  Every comparison on the listed units is bitwise; the only other bar of this file is the
project's 1e-4 s in test_default_mode_across_sizes, whose units include ties.

Instantiations and the cases that run them (the option fim_threads sets both launches of a unit: the refined box and the coarse grid):

  k_fim_sorted<NT, COMPACT = true,  TIE = true >   coarse grid   test_sorted_shapes_equal_the_oracle[tie1-NT-*], test_window[*-NT-*] (NT 128, 1024)
  k_fim_sorted<NT, COMPACT = true,  TIE = false>   coarse grid   test_sorted_shapes_equal_the_oracle[tie0-NT-*]
  k_fim_sorted<NT, COMPACT = false, TIE = true >   refined box   test_sorted_shapes_equal_the_oracle[tie1-NT-*]
  k_fim_sorted<NT, COMPACT = false, TIE = false>   refined box   test_sorted_shapes_equal_the_oracle[tie0-NT-*]
  k_fim<NT>                                        refined box   test_list_variant_all_sizes[NT-*]; k_fim<128> with overflowing lists
                                                                 (list_cap 512, ready_cap 256: 2 to 26 rescans a call):
                                                                 test_list_variant_overflowing_lists
  for NT in 128, 256, 512, 1024: sixteen k_fim_sorted and four k_fim.  k_fim_sorted<1024, true, true> with recycled field slots:
  test_slot_recycling_at_1024_threads; <256 | 512 | 1024, *, true> followed by the march of the flagged units: test_default_mode_across_sizes.

Not covered: option tie_frozen_bundles (it needs a bundle that froze a cycle; none is constructed here).

The engine of this module is its own (conftest's PRODUCT_DEFAULTS do not reset fim_threads, window_cells, list_cap, ready_cap or fim_sorted):
every test sets every option it depends on through `configure`.
"""
import numpy as np
import pytest

import _libs as L
import parity_log
import solve_units as SU
import synth
import test_gpu_parity as P

pytestmark = pytest.mark.gpu
TOL = 1e-4          # (test_default_mode_across_sizes only)
THREADS = (128, 256, 512, 1024)
GRID_NAMES = tuple(SU.GRIDS)

# the options this module changes, at the product's defaults but for bundle = 0 and exact_ties = 0
BASE = dict(bundle=0, exact_ties=0, tie_detect=1, fim_threads=0, fim_sorted=1, window_cells=1.25, list_cap=0, ready_cap=0, field_pool=0,
            tie_threshold=2e-5, tie_sum_threshold=0, tie_count_threshold=0, tie_map_strict=1)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def configure(e, **over):
    for k, v in {**BASE, **over}.items():
        e.set_option(k, v)


@pytest.fixture(scope="module")
def eng():
    from dsurftomo_amd import build
    from dsurftomo_amd.engine import Engine
    build.build()
    e = Engine(0)
    yield e
    e.close()


class Call:
    """the listed units of one grid as one engine call -- two receivers per unit, one far and one 0.3 cells from the source -- and the
    oracle's answer to it, computed once"""

    def __init__(self, name):
        rows = SU.load()[name]
        self.name = name
        self.nx, self.ny, self.gd = SU.GRIDS[name]
        self.kinds = sorted({k for k, _, _ in rows})
        cases = {k: SU.Case(name, k) for k in self.kinds}
        self.g = g = cases[self.kinds[0]].g
        self.pv = np.stack([cases[k].pv for k in self.kinds])
        self.veln = [cases[k].veln for k in self.kinds]
        self.map_index = np.array([self.kinds.index(k) for k, _, _ in rows], np.int32)
        self.src, self.sols = [], []
        for k, fx, fz in rows:
            sx, sz, o = cases[k].solve(fx, fz)
            self.src.append((sx, sz)); self.sols.append(o)
        self.rcx, self.rcz, self.ref = receivers(g, self.src, self.sols, [self.veln[m] for m in self.map_index])

    def set_maps(self, e):
        e.set_maps(self.nx, self.ny, synth.GOXD, synth.GOZD, synth.DVD, synth.DVD, self.pv, dicing=self.gd)
        assert (e.nnx, e.nnz) == (self.g.nnx, self.g.nnz)

    def args(self):
        n = len(self.src)
        return dict(map_index=self.map_index, scx=[s[0] for s in self.src], scz=[s[1] for s in self.src], nrec=np.full(n, 2, np.int32),
                    rcx=self.rcx.reshape(-1), rcz=self.rcz.reshape(-1))


def receivers(g, src, sols, veln):
    """per source: another source's place and a point 0.3 cells away (as tests/test_gpu_parity.py); the oracle's times there"""
    f = np.float32
    n = len(src)
    rcx = np.array([[src[(i + 3) % n][0], f(s[0] + f(0.3) * g.dnx)] for i, s in enumerate(src)], f)
    rcz = np.array([[src[(i + 3) % n][1], f(s[1] + f(0.2) * g.dnz)] for i, s in enumerate(src)], f)
    rcx = np.clip(rcx, g.gox, f(g.gox + f(g.nnx - 1.01) * g.dnx)).astype(f)
    rcz = np.clip(rcz, g.goz, f(g.goz + f(g.nnz - 1.01) * g.dnz)).astype(f)
    ref = np.array([[L.o_srtimes(g, veln[u], sols[u]["T"], src[u][0], src[u][1], rcx[u, k], rcz[u, k]) for k in range(2)] for u in range(n)], f)
    return rcx, rcz, ref


_calls = {}


def call_of(name):
    if name not in _calls:
        _calls[name] = Call(name)
    return _calls[name]


class Result:
    def __init__(self, e, call, fields=True):
        call.set_maps(e)
        self.times = e.traveltimes(**call.args())
        n = len(call.src)
        self.stats = e.stats()
        assert self.stats["bundles"] == 0 and self.stats["bundled_units"] == 0
        self.rounds = e.unit_rounds()
        self.flags, self.influence = e.unit_ties()
        self.count, self.sum, _ = e.unit_tie_sums()
        self.fields = [e.field(u) for u in range(n)] if fields else None
        self.refined = [e.refined(u) for u in range(n)] if fields else None


def assert_is_the_oracle(res, call, what):
    for u, o in enumerate(call.sols):
        assert (bits(res.fields[u]) != bits(o["T"])).sum() == 0, (what, call.name, u, "coarse field")
        Tr, Sr = res.refined[u]
        assert Tr.shape == o["Tr"].shape, (what, call.name, u)
        assert (np.sign(o["Sr"]).clip(-1, 1) != Sr).sum() == 0, (what, call.name, u, "refined status classes")
        known = o["Sr"] >= 0             # alive nodes and the narrow band's trial values
        assert (bits(Tr[known]) != bits(o["Tr"][known])).sum() == 0, (what, call.name, u, "refined times")
    assert (bits(res.times.reshape(-1, 2)) != bits(call.ref)).sum() == 0, (what, call.name, "receiver times")


def assert_same_bits(a, b, what):
    assert (bits(a.times) != bits(b.times)).sum() == 0, (what, "receiver times")
    for u in range(len(a.fields)):
        assert (bits(a.fields[u]) != bits(b.fields[u])).sum() == 0, (what, u, "coarse field")
        assert (bits(a.refined[u][0]) != bits(b.refined[u][0])).sum() == 0, (what, u, "refined times")
        assert (a.refined[u][1] != b.refined[u][1]).sum() == 0, (what, u, "refined statuses")


_sorted = {}


def sorted_run(eng, name):
    """the run every variant is compared with: the ordered kernels at the product's launch shape"""
    if name not in _sorted:
        configure(eng)
        _sorted[name] = Result(eng, call_of(name))
    return _sorted[name]


@pytest.mark.parametrize("name", GRID_NAMES)
@pytest.mark.parametrize("nt", THREADS)
@pytest.mark.parametrize("tie", [1, 0], ids=["tie1", "tie0"])
def test_sorted_shapes_equal_the_oracle(eng, name, nt, tie):
    """k_fim_sorted<nt, *, tie> on the refined box and on the coarse grid: coarse field, refined snapshot, status classes and receiver times of
    every listed unit are the oracle's; the census (tie = 1) finds no tie on these units and flags none"""
    call = call_of(name)
    configure(eng, fim_threads=nt, tie_detect=tie)
    res = Result(eng, call)
    assert_is_the_oracle(res, call, "%d threads, tie_detect %d" % (nt, tie))
    if tie:
        assert (res.count != 0).sum() == 0 and (res.flags != 0).sum() == 0, (res.count, res.flags)
    assert res.stats["tie_units"] == 0
    assert res.stats["rescans"] == 0


@pytest.mark.parametrize("name", GRID_NAMES)
@pytest.mark.parametrize("nt", [128, 1024])
def test_window(eng, name, nt):
    """the causal window (option window_cells: 0.5, 1.25, 6 cells) changes the schedule, not the field: the oracle's bits at each.

    The deferral path (more ready nodes of one colour than rhalf = 4 nt, the rest stay in their masks) runs at 257^2 with 128 threads and 6 cells:
    a front 80 cells from the source is about 2 pi 80 = 500 nodes long, a 6-cell window holds about six layers of it, 3000 nodes, 1500 of
    each colour -- three times rhalf = 512 (with 1024 threads, rhalf = 4096, all of them fit).  unit_rounds() differs between the 0.5- and the
    6-cell run: the option reached the kernel."""
    call = call_of(name)
    rounds = {}
    for wc in SU.WINDOWS:
        configure(eng, fim_threads=nt, window_cells=wc)
        res = Result(eng, call)
        assert_is_the_oracle(res, call, "%d threads, window %g" % (nt, wc))
        rounds[wc] = res.rounds
    assert (rounds[0.5] != rounds[6.0]).any(), rounds


@pytest.mark.parametrize("name", GRID_NAMES)
@pytest.mark.parametrize("nt", THREADS)
def test_list_variant_all_sizes(eng, name, nt):
    """k_fim<nt> (option fim_sorted = 0: the refined boxes through the list kernel) leaves the refined snapshot, and everything downstream of
    it, as the ordered kernels do -- and both are the oracle's"""
    call = call_of(name)
    ref = sorted_run(eng, name)
    configure(eng, fim_sorted=0, fim_threads=nt)
    res = Result(eng, call)
    assert_same_bits(res, ref, "list variant, %d threads" % nt)
    assert_is_the_oracle(res, call, "list variant, %d threads" % nt)
    assert res.stats["rescans"] == 0


OVERFLOW_CAPS = (512, 256)     # list_cap, ready_cap: the shortest lists dsa_set_option accepts (csrc/engine.h: kMinListCap, kMinReadyCap)


@pytest.mark.parametrize("name", GRID_NAMES)
def test_list_variant_overflowing_lists(eng, name):
    """k_fim<128> with lists too short for the 129^2 box's front (list_cap = 512, ready_cap = 256 against the default 16 * 258 + 4096 and
    8 * 258 + 2048): entries that do not fit are dropped (SC_OVERFLOW), the nodes keep their queued bit and a rescan of the field collects
    them.  stats()["rescans"] > 0, and the same bits as the ordered kernels.

    Measured on these four calls of twelve units (rescans per call, grids in the order of GRID_NAMES): list_cap = 256, ready_cap = 128 -- where
    the search for an overflowing size started -- "fixed-point solve did not converge (rounds 20609)" on every grid: each rescan reopens the
    causal window, and the box runs out of its 64 (rnx + rnz) + 4096 rounds; 384 / 192: 278, 330, 649, 475 rescans, the right bits, twenty
    times the time; 512 / 256: 5, 3, 11, 7 (2 to 26 in later runs: the count depends on the schedule); 1024 / 512 and more: none.  So dsa_set_option now refuses lists below 512 / 256
    (test_short_lists_are_refused), and this case runs at that floor."""
    call = call_of(name)
    ref = sorted_run(eng, name)
    configure(eng, fim_sorted=0, fim_threads=128, list_cap=OVERFLOW_CAPS[0], ready_cap=OVERFLOW_CAPS[1])
    res = Result(eng, call)
    parity_log.add("list variant, grid %s, list_cap %d ready_cap %d: %d rescans over %d units" % (name, *OVERFLOW_CAPS, res.stats["rescans"], len(call.src)))
    assert res.stats["rescans"] > 0
    assert_same_bits(res, ref, "overflowing lists")
    assert_is_the_oracle(res, call, "overflowing lists")


def test_short_lists_are_refused(eng):
    """lists the list kernel cannot finish a refined box with (see test_list_variant_overflowing_lists) are an argument error of dsa_set_option, not a
    solve that fails; 0 (from the grid) and the floor itself are accepted, and a refused value leaves the option as it was"""
    from dsurftomo_amd.engine import EngineError
    call = call_of("121")
    configure(eng, fim_sorted=0)
    for option, floor in (("list_cap", OVERFLOW_CAPS[0]), ("ready_cap", OVERFLOW_CAPS[1])):
        for bad in (1, floor // 2, floor - 1, -1):
            with pytest.raises(EngineError) as x:
                eng.set_option(option, bad)
            assert x.value.code != 0 and option in str(x.value)
        eng.set_option(option, floor)
        eng.set_option(option, 0)
    res = Result(eng, call)                       # the refused values changed nothing: the default lists, no rescan
    assert res.stats["rescans"] == 0
    assert_is_the_oracle(res, call, "after refused options")


def test_slot_recycling_at_1024_threads(eng):
    """twelve units through two field slots (option field_pool = 2: a workgroup claims a slot, resets it, and hands it on) with 1024 threads:
    the receiver times of a slot per unit (field_pool = -1), which are the oracle's"""
    call = call_of("257")
    assert len(call.src) == 12
    configure(eng, fim_threads=1024, field_pool=-1)
    own = Result(eng, call, fields=False)
    configure(eng, fim_threads=1024, field_pool=2)
    two = Result(eng, call, fields=False)
    assert two.stats["field_slots"] == 2 and own.stats["field_slots"] >= 12
    assert (bits(two.times) != bits(own.times)).sum() == 0
    assert (bits(two.times.reshape(-1, 2)) != bits(call.ref)).sum() == 0


# ---- units with ties: the default mode and the flag rule --------------------------------------------------------------------------------

class CheckerCall:
    """sources (tests/test_gpu_parity.py: positions) on the (35, "checker4", 8) case of tests/test_gpu_parity.py, ties included: 257^2 nodes"""

    def __init__(self, frac):
        self.name = "257 checker4"
        self.nx = self.ny = 35
        self.gd = 8
        self.src = P.positions(35, 8, frac)
        self.g, pv, veln, self.sols = P.oracle_case(35, "checker4", 8, self.src)
        self.pv = pv[None, :]
        self.map_index = np.zeros(len(self.src), np.int32)
        self.rcx, self.rcz, self.ref = receivers(self.g, self.src, self.sols, [veln] * len(self.src))

    set_maps = Call.set_maps
    args = Call.args


_checker = {}


def checker_call(frac):
    key = tuple(frac)
    if key not in _checker:
        _checker[key] = CheckerCall(frac)
    return _checker[key]


def test_default_mode_across_sizes(eng):
    """exact_ties = 1 (fixed point, census, flagged units marched) with 256, 512 and 1024 threads on units with ties: every field within
    1e-4 s of the oracle, every marched unit the oracle's bit for bit, and the same units marched at every size -- the census reads the
    converged field, not the schedule"""
    call = checker_call(P.FRAC[:12])
    marched = {}
    for nt in (256, 512, 1024):
        configure(eng, exact_ties=1, fim_threads=nt)
        res = Result(eng, call)
        m = (res.flags & 2) != 0
        marched[nt] = m
        for u, o in enumerate(call.sols):
            d = float(np.abs(res.fields[u] - o["T"]).max())
            assert d <= TOL, (nt, u, d)
            if m[u]:
                assert (bits(res.fields[u]) != bits(o["T"])).sum() == 0, (nt, u, "a marched unit")
                assert (bits(res.times[2 * u:2 * u + 2]) != bits(call.ref[u])).sum() == 0, (nt, u, "a marched unit's receiver times")
        assert np.abs(res.times.reshape(-1, 2).astype(np.float64) - call.ref).max() <= TOL
        parity_log.add("default mode, 257^2 checker4, %d threads: units marched %s" % (nt, np.flatnonzero(m).tolist()))
    assert m.any()
    assert (marched[256] == marched[512]).all() and (marched[256] == marched[1024]).all(), marched


# sources on nodes of the checkerboard: (5, 7) and (16, 24) of tests/test_gpu_parity.py, and ten of 75 drawn nodes at which the CPU's tie study
# (tests/hostcheck.cpp: hc_tie_study) finds a tie with an influence in the converged field -- so that most units of the call hold ties
FLAG_NODES = [(5.0, 7.0), (16.0, 24.0), (129.0, 215.0), (215.0, 90.0), (27.0, 230.0), (56.0, 184.0), (176.0, 71.0), (10.0, 87.0), (163.0, 233.0),
              (46.0, 241.0), (69.0, 161.0), (223.0, 146.0)]


@pytest.mark.parametrize("option,column", [("tie_sum_threshold", "sum"), ("tie_count_threshold", "count")])
def test_flag_rule_thresholds(eng, option, column):
    """the flag rule's summed-influence and tie-count thresholds (Engine::tie_verdict) in mode 0 on a call with ties: with tie_threshold out of
    reach and tie_map_strict = 0 (a flag depends on the unit alone) the flagged units are exactly those whose sum / count exceeds the
    threshold -- the median of the call's -- and fields and receiver times do not change in any bit: the options only flag.
    (The sums are multiples of 2^-30 s below 2^-6 s, exact in fp32: the engine's comparison in fp64 is the one made here.)

    The census counts the evaluations of the iteration that end on a tie, transient ones among them, so a unit's count and sum depend on the
    schedule and differ from run to run (measured over 24 runs of this call: unit 8 counts 1 or 3, unit 10 counts 1 or 2, the fields and times
    the same bits in all): the threshold is the median of a first run, the flags of the second run are held against that run's own sums and
    counts, and the two runs' census figures are not compared."""
    call = checker_call(FLAG_NODES)
    configure(eng, tie_map_strict=0)
    base = Result(eng, call)
    values = getattr(base, column)
    thr = float(np.median(values.astype(np.float64)))
    thr = float(int(thr)) if column == "count" else float(np.float32(thr))       # (as the engine stores it)
    assert thr > 0, values
    configure(eng, tie_map_strict=0, tie_threshold=1.0, **{option: thr})
    res = Result(eng, call)
    want = getattr(res, column).astype(np.float64) > thr
    assert 0 < want.sum() < len(want), (values, thr)
    assert ((res.flags & 1) != 0).tolist() == want.tolist(), (res.flags, getattr(res, column), thr)
    assert res.stats["tie_units"] == want.sum()
    assert_same_bits(res, base, option)
