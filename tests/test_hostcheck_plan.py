"""How a launch is bundled (dsurftomo_amd/csrc/bundle_plan.h), on the CPU through tests/hostcheck_plan.cpp: which units share a bundle,
the launch order, the second group of a large launch, the choice of the bundle size and the field slots.  What is expected here is written
down from the rules as the header's comments state them, not taken from the code."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import _libs as L
import synth

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libhostcheck_plan.so")
I64 = C.c_longlong
AMPLE = 1 << 60


@pytest.fixture(scope="module")
def h():
    src = os.path.join(HERE, "hostcheck_plan.cpp")
    hdr = [os.path.join(L.ROOT, "dsurftomo_amd", "csrc", n) for n in ("eikonal_core.h", "source_stage.h", "bundle_plan.h")]
    if L._stale(SO, [src] + hdr):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-msse2",
                               "-mfpmath=sse", "-shared", "-o", SO, src, "-lm"])
    lib = C.CDLL(SO)
    f32, i32, vp = L.f32, L.i32, L.vp
    lib.hcp_slot_bytes.restype = I64
    lib.hcp_slot_bytes.argtypes = [i32, I64, i32, I64, i32]
    lib.hcp_source_before.argtypes = [f32] * 4
    lib.hcp_farness.restype = f32
    lib.hcp_farness.argtypes = [i32, i32] + [f32] * 6
    lib.hcp_census.argtypes = [vp, i32, i32, vp]
    lib.hcp_layout.argtypes = [i32, i32, f32, f32, f32, f32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    lib.hcp_choose.argtypes = [vp, i32, vp, I64, I64, I64, vp, vp]
    lib.hcp_slots.argtypes = [vp, I64, i32, I64, i32, i32, I64, vp, vp]
    return lib


def options(bundle=1, mpl=0, tail=1, order=0, threads=256, threads_auto=1):
    return np.array([bundle, mpl, tail, order, threads, threads_auto], np.int32)


# a grid on which node coordinates are exact in fp32 (origin 0, spacings 1 and 2), and a rectangular one as the engine derives it
EXACT = (129, 257, 0.0, 0.0, 1.0, 2.0)


def rect_grid():
    gox, goz, dn, _ = synth.grid_origin(19)
    return (129, 257, float(gox), float(goz), float(dn), float(np.float32(1.3) * dn))


def farness(grid, scx, scz):
    """minus the squared node distance to the farthest corner, fp32, in the operand order of the engine"""
    nnx, nnz, gox, goz, dnx, dnz = grid
    f = np.float32
    fx = (np.asarray(scx, f) - f(gox)) / f(dnx); fz = (np.asarray(scz, f) - f(goz)) / f(dnz)
    dx = np.maximum(fx, f(nnx - 1) - fx); dz = np.maximum(fz, f(nnz - 1) - fz)
    return -(dx * dx + dz * dz)


def keys(scx, scz):
    """the source of a unit: its coordinates bit for bit, ordered as the pair (bits of scx, bits of scz)"""
    a = np.ascontiguousarray(scx, np.float32).view(np.uint32).astype(np.uint64)
    b = np.ascontiguousarray(scz, np.float32).view(np.uint32).astype(np.uint64)
    return (a << np.uint64(32)) | b


def census(h, counts, G):
    c = np.ascontiguousarray(counts, np.int32)
    out = np.zeros(2, np.int64)
    h.hcp_census(L.ptr(c), c.size, G, L.ptr(out))
    return int(out[0]), int(out[1])


def layout(h, grid, scx, scz, G, opt):
    scx = np.ascontiguousarray(scx, np.float32); scz = np.ascontiguousarray(scz, np.float32)
    n = scx.size
    flag, rank, bundle, place = (np.zeros(n, np.int32) for _ in range(4))
    scal = np.zeros(7, np.int32)
    h.hcp_layout(grid[0], grid[1], grid[2], grid[3], grid[4], grid[5], n, L.ptr(scx), L.ptr(scz), G, L.ptr(opt),
                 L.ptr(flag), L.ptr(rank), L.ptr(bundle), L.ptr(place), L.ptr(scal))
    d = dict(zip(("a", "b", "Gb", "mpl_now", "mpl_b", "threads_b", "nsolo"), (int(v) for v in scal)))
    d.update(flag=flag, rank=rank, bundle=bundle, place=place, n=n)
    d["sizes"] = np.bincount(bundle[bundle >= 0], minlength=max(d["a"], 0) + d["b"])
    return d


def units_of(counts, order="source"):
    """unit -> source for sources with counts[s] units: source by source, or period outer and source inner (the reference's order)"""
    counts = np.asarray(counts)
    if order == "source":
        return np.repeat(np.arange(counts.size), counts)
    return np.concatenate([np.nonzero(counts > p)[0] for p in range(int(counts.max()))])


def line_sources(nsrc):
    """sources on the line z = 2000 of a 4001^2 grid with exact node coordinates, source i at x = i + 1 (left of the middle): the lower i,
    the longer its front"""
    assert nsrc < 2000
    grid = (4001, 4001, 0.0, 0.0, 1.0, 1.0)
    return grid, np.arange(1, nsrc + 1, dtype=np.float32), np.full(nsrc, 2000.0, np.float32)


def expected_ranks(grid, scx, scz, G):
    """launch ranks of a launch without a second group, by the rules: a source's units in their own order in pieces of G, a remainder of
    one solo; solo units first, farthest first, the lower unit first on equal farness; then the bundles, farthest first, in source order
    and then piece order on equal farness"""
    far = farness(grid, scx, scz); key = keys(scx, scz)
    n = len(scx)
    bundles, solo = [], []
    for k in np.unique(key):
        v = np.nonzero(key == k)[0]
        for q, i in enumerate(range(0, v.size, G) if G else []):
            m = v[i:i + G]
            if m.size >= 2: bundles.append((far[m[0]], int(k), q, list(m)))
            else: solo.append(int(m[0]))
        if not G: solo += list(v)
    solo.sort(key=lambda u: (far[u], u))
    bundles.sort(key=lambda b: b[:3])
    rank = np.zeros(n, np.int32)
    order = solo + [u for b in bundles for u in b[3]]
    rank[order] = np.arange(n)
    return rank, len(solo), [b[3] for b in bundles]


# ---- small shared rules ---------------------------------------------------------------------------------------------------------------
def test_source_key_orders_as_the_pair_of_bit_patterns(h):
    assert h.hcp_source_before(1.0, 5.0, 2.0, 0.0) == 1 and h.hcp_source_before(2.0, 0.0, 1.0, 5.0) == 0
    assert h.hcp_source_before(1.0, 2.0, 1.0, 3.0) == 1 and h.hcp_source_before(1.0, 2.0, 1.0, 2.0) == 0
    assert h.hcp_source_before(0.0, 0.0, -0.0, 0.0) == 1          # bit for bit: -0 is another source than 0, and its pattern is the larger


def test_farness_and_slot_bytes(h):
    g = rect_grid()
    sx, sz = synth.sources(19, 50, seed=synth.SEED + 3)
    got = np.array([h.hcp_farness(g[0], g[1], g[2], g[3], g[4], g[5], float(x), float(z)) for x, z in zip(sx, sz)], np.float32)
    assert (got.view(np.uint32) == farness(g, sx, sz).view(np.uint32)).all()
    assert h.hcp_farness(*EXACT, 10.0, 20.0) == -float(118 ** 2 + 246 ** 2)       # x = 10 of 0..128, z = 20 / 2 = 10 of 0..256
    assert [h.hcp_bundle_log2(G) for G in (4, 8, 16)] == [2, 3, 4]
    # a slot: G members and the shared record per node (4 B), 2^(exc_log2cap + log2 G) exception entries of 8 B, the tile records
    assert h.hcp_slot_bytes(16, 1000, 10, 77, 1) == 17 * 1000 * 4 + (8 << 14) + 77 * 4
    assert h.hcp_slot_bytes(8, 1000, 10, 77, 2) == 17 * 1000 * 4 + (8 << 13) + 77 * 4
    assert h.hcp_slot_bytes(4, 64, 12, 10, 1) == 5 * 64 * 4 + (8 << 14) + 40


# ---- census and pieces ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["source", "period"])
def test_pieces_of_16_17_and_18_units(h, order):
    counts = np.array([16, 17, 18])
    assert census(h, counts, 16) == (4, 50)
    assert census(h, counts, 8) == (7, 50)
    src = units_of(counts, order)
    sx = np.array([30.0, 20.0, 10.0], np.float32)[src]; sz = np.full(src.size, 40.0, np.float32)
    for G, want in ((16, [[16], [16], [16, 2]]), (8, [[8, 8], [8, 8], [8, 8, 2]])):
        d = layout(h, EXACT, sx, sz, G, options(bundle=G))
        assert d["a"] == sum(len(w) for w in want) and d["b"] == 0 and d["nsolo"] == 1
        assert int((d["flag"] == 0).sum()) == 1 and src[d["flag"] == 0][0] == 1          # the seventeenth unit of the second source
        for s in range(3):
            mine = np.nonzero(src == s)[0]
            b = d["bundle"][mine]
            assert [int((b == k).sum()) for k in dict.fromkeys(b[b >= 0])] == want[s]
            # a source's members are consecutive in its own unit order, bundle after bundle
            inb = mine[b >= 0]
            assert (np.diff(d["rank"][inb]) == 1).all() and (d["place"][inb] == np.concatenate([np.arange(w) for w in want[s]])).all()


def test_a_single_unit_is_always_solo(h):
    for G in (4, 8, 16):
        assert census(h, [1, 1, 1], G) == (0, 0)
        d = layout(h, EXACT, [1.0, 2.0, 3.0], [2.0, 2.0, 2.0], G, options())
        assert d["nsolo"] == 3 and d["a"] == 0 and d["b"] == 0 and (d["flag"] == 0).all()
        assert census(h, [G + 1], G) == (1, G)


# ---- launch ranks ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [0, 4, 16])
def test_launch_ranks_on_a_rectangular_grid(h, G):
    g = rect_grid()
    sx, sz = synth.sources(19, 37, seed=synth.SEED + 11)
    counts = np.array([(1, 2, 5, 16, 9, 33)[s % 6] for s in range(37)])
    src = units_of(counts, "period")
    d = layout(h, g, sx[src], sz[src], G, options(bundle=G if G else 1))
    want, nsolo, bundles = expected_ranks(g, sx[src], sz[src], G)
    assert sorted(d["rank"]) == list(range(src.size))
    assert d["nsolo"] == nsolo and d["a"] == len(bundles) and d["b"] == 0
    assert (d["rank"] == want).all()
    assert (d["rank"][d["flag"] == 0] < nsolo).all() and (d["rank"][d["flag"] != 0] >= nsolo).all()
    # the two spacings differ: with dx and dz exchanged the order would be another one
    gx = (g[0], g[1], g[2], g[3], g[5], g[4])
    assert (expected_ranks(gx, sx[src], sz[src], G)[0] != want).any()


def test_equal_farness_keeps_unit_order_and_source_order(h):
    # x = 10 and x = 118 are equally far from their farthest corner on 0..128; so are the bundles of one source
    sx = np.array([118.0, 10.0, 118.0, 10.0, 64.0] + [118.0] * 8 + [10.0] * 7, np.float32)
    sz = np.array([40.0, 40.0, 40.0, 40.0, 2.0] + [40.0] * 15, np.float32)
    d = layout(h, EXACT, sx, sz, 0, options())
    assert d["nsolo"] == sx.size and (d["rank"][:4] == [0, 1, 2, 3]).all() and d["rank"][4] == sx.size - 1          # as far as each other: the lower unit first
    d = layout(h, EXACT, sx, sz, 4, options(bundle=4))
    ten = np.nonzero(sx == 10.0)[0]; other = np.nonzero(sx == 118.0)[0]
    # source x = 10 (9 units: 4 + 4 and a solo one) before source x = 118 (the larger bit pattern; 4 + 4 + 2), each one's pieces in their order
    assert d["nsolo"] == 2 and d["a"] == 5 and d["b"] == 0
    assert (d["bundle"][ten] == [0, 0, 0, 0, 1, 1, 1, 1, -1]).all() and (d["bundle"][other] == [2, 2, 2, 2, 3, 3, 3, 3, 4, 4]).all()
    assert d["rank"][ten[8]] == 0 and d["rank"][4] == 1          # the solo units: the ninth of x = 10 is farther than (64, 2)
    assert (d["rank"][ten[:8]] == 2 + np.arange(8)).all() and (d["rank"][other] == 10 + np.arange(10)).all()


# ---- the second group of a large launch -------------------------------------------------------------------------------------------------
def big_launch(h, nsrc, per=16, G=16, short=(), **opt):
    grid, sx, sz = line_sources(nsrc)
    counts = np.full(nsrc, per)
    for s, c in short: counts[s] = c
    src = units_of(counts, "period")
    return src, counts, layout(h, grid, sx[src], sz[src], G, options(**opt))


def test_wide_tail_behind_the_first_generation(h):
    src, _, d = big_launch(h, 1000, tail=1)
    assert (d["a"], d["b"], d["Gb"], d["threads_b"], d["mpl_b"], d["mpl_now"]) == (768, 232, 16, 768, 4, 4)
    assert (d["flag"][src >= 768] == 2).all() and (d["flag"][src < 768] == 1).all()          # the first 768 are the longest
    assert (d["bundle"] == src).all() and (d["sizes"] == 16).all()
    assert sorted(d["rank"]) == list(range(16000)) and (d["rank"] == 16 * d["bundle"] + d["place"]).all()


def test_halves_behind_the_first_generation(h):
    src, _, d = big_launch(h, 1000, tail=0)
    assert (d["a"], d["b"], d["Gb"], d["threads_b"], d["mpl_b"]) == (768, 464, 8, 256, 2)
    assert d["a"] + d["b"] == 1232 and (d["flag"] == 1).all()
    assert (d["sizes"][:768] == 16).all() and (d["sizes"][768:] == 8).all()
    tail = src >= 768
    assert (d["bundle"][~tail] == src[~tail]).all()
    assert (d["bundle"][tail] == 768 + 2 * (src[tail] - 768) + (np.arange(16000) // 1000)[tail] // 8).all()          # first and second half, in order
    assert sorted(d["rank"]) == list(range(16000))
    # more than 256 beyond the first generation: halves whatever bundle_tail says
    _, _, d = big_launch(h, 1100, tail=1)
    assert (d["a"], d["b"], d["Gb"], d["threads_b"], d["mpl_b"]) == (768, 664, 8, 256, 2) and (d["flag"] == 1).all()


def test_short_pieces_beyond_the_first_generation_are_not_cut(h):
    # the ten shortest fronts have 9 units (fewer than G / 2 + 2): whole, in the first group; one of 10 units is cut into 8 + 2
    short = [(s, 9) for s in range(990, 1000)] + [(980, 10)]
    src, counts, d = big_launch(h, 1000, tail=0, short=short)
    assert (d["a"], d["b"], d["Gb"]) == (768 + 10, 2 * (232 - 10), 8)
    for s in range(990, 1000):
        b = np.unique(d["bundle"][src == s])
        assert b.size == 1 and 768 <= b[0] < 778 and d["sizes"][b[0]] == 9
    b = d["bundle"][src == 980]
    assert (b >= 778).all() and (np.bincount(b - b.min()) == [8, 2]).all()


@pytest.mark.parametrize("case", [dict(nsrc=768), dict(nsrc=1500), dict(nsrc=1000, per=4, G=4), dict(nsrc=1000, bundle=16), dict(nsrc=1000, mpl=2),
                                  dict(nsrc=1000, mpl=4), dict(nsrc=1000, threads=768), dict(nsrc=1000, threads=512)],
                         ids=lambda c: "-".join("%s%s" % kv for kv in c.items()))
@pytest.mark.parametrize("tail", [0, 1])
def test_no_second_group(h, case, tail):
    src, _, d = big_launch(h, tail=tail, **case)
    G = case.get("G", 16)
    assert (d["a"], d["b"], d["Gb"]) == (case["nsrc"], 0, 0) and (d["flag"] == 1).all()
    assert (d["bundle"] == src).all() and (d["rank"] == G * d["bundle"] + d["place"]).all()
    assert d["threads_b"] == case.get("threads", 256)
    # members per lane: the option; 16 members or another workgroup size four; 8 and 4 members two from 513 bundles on
    assert d["mpl_now"] == (case.get("mpl") or (2 if G == 4 else 4))


def test_bundle_order_1_groups_the_first_generation_by_cu(h):
    src, _, d = big_launch(h, 1000, tail=1, order=1)
    assert (d["a"], d["b"], d["threads_b"]) == (768, 232, 768)
    first = np.zeros(1000, np.int64); first[d["bundle"][:1000]] = src[:1000]          # bundle -> its source = its place in "longest first"
    p = np.arange(768)
    assert (first[:768] == 3 * (p % 256) + p // 256).all() and (first[768:] == np.arange(768, 1000)).all()
    # only with a wide tail: with halves, and with the values 2 and 3, the order is that of bundle_order = 0
    for kw in (dict(tail=0, order=1), dict(tail=1, order=2), dict(tail=1, order=3)):
        _, _, d1 = big_launch(h, 1000, **kw)
        _, _, d0 = big_launch(h, 1000, tail=kw["tail"], order=0)
        assert (d1["rank"] == d0["rank"]).all() and (d1["bundle"] == d0["bundle"]).all() and (d1["flag"] == d0["flag"]).all()


# ---- the choice of size ------------------------------------------------------------------------------------------------------------------
def choose(h, counts, nn=1025, nnz=None, nmaps=16, step=1 << 30, room=AMPLE, failed=0, nrec_c=None, exc_log2cap=12, lists=None, bstride=1, **opt):
    nnz = nnz or nn
    nbx, nbz = (nn + 7) // 8, (nnz + 7) // 8
    nrec_c = nbx * nbz * 64 if nrec_c is None else nrec_c
    lists = 4 * nbx * nbz + 2 if lists is None else lists
    c = np.ascontiguousarray(counts, np.int32)
    dims = np.array([nn, nnz, nmaps, exc_log2cap, step, bstride, failed], np.int32)
    out = np.zeros(3, np.int64)
    h.hcp_choose(L.ptr(c), c.size, L.ptr(dims), nrec_c, lists, room, L.ptr(options(**opt)), L.ptr(out))
    return int(out[0]), bool(out[1]), int(out[2])


def test_no_bundles(h):
    full = [16] * 1000
    assert choose(h, full, bundle=0) == (0, False, 16000)
    assert choose(h, full, failed=1) == (0, False, 16000)
    assert choose(h, full, failed=1, bundle=16)[0] == 16          # (a forced size stays)
    assert choose(h, [1] * 5000) == (0, False, 5000)
    assert choose(h, [1] * 5000, bundle=4) == (0, False, 5000)
    assert choose(h, full, nn=113) == (0, False, 16000)            # below 120 nodes per side ...
    assert choose(h, full, nn=129, nnz=113) == (0, False, 16000)
    assert choose(h, full, nn=113, bundle=8) == (8, False, 0)      # ... where a forced size is still honoured
    assert choose(h, full, nn=121)[0] == 16


def test_small_grids_need_384_bundles_of_8(h):
    assert choose(h, [16] * 100, nn=257) == (0, False, 1600)       # 100 of 16, 200 of 8; 400 of 4 do not count
    assert choose(h, [16] * 191, nn=385) == (0, False, 16 * 191)   # 382 of 8
    G, wide, solo = choose(h, [16] * 200, nn=257)                   # 200 of 16 are too few, 400 of 8 may do
    assert G in (0, 8) and not wide
    assert choose(h, [16] * 400, nn=257) == (16, False, 0)
    G, wide, _ = choose(h, [16] * 100, nn=401)                     # from 400 nodes per side a small launch runs wide
    assert G > 0 and wide
    for n in (50, 100, 250):
        assert not choose(h, [16] * n, nn=385)[1] and not choose(h, [16] * n, nn=257, nnz=1025)[1]


def test_limits_of_the_bundle_fields(h):
    one = dict(counts=[16] * 10, nmaps=1)
    # 32-bit byte offsets inside a bundle field: records x members x 4 B x stride below 2^32 (which keeps records x members below 2^30 too)
    assert choose(h, nrec_c=1 << 25, bundle=16, **one)[0] == 16
    assert choose(h, nrec_c=1 << 25, bundle=16, bstride=2, **one)[0] == 0
    assert choose(h, nrec_c=1 << 26, bundle=16, **one)[0] == 0 and choose(h, nrec_c=1 << 26, bundle=8, **one)[0] == 8
    # record indices below 2^27
    assert choose(h, nrec_c=(1 << 27) - 64, bundle=4, **one)[0] == 4 and choose(h, nrec_c=1 << 27, bundle=4, **one)[0] == 0
    # 32-bit byte offsets inside the member-minor slowness: records x maps x 4 B
    assert choose(h, [16] * 10, nrec_c=1 << 20, nmaps=1023, bundle=16)[0] == 16 and choose(h, [16] * 10, nrec_c=1 << 20, nmaps=1024, bundle=16)[0] == 0
    # automatic: the sizes that fit are still there
    assert choose(h, [16] * 1000, nrec_c=1 << 26, nmaps=1)[0] == 8


def test_room_for_one_generation_of_slots(h):
    nrec_c, lists, xl, nmaps = 129 * 129 * 64, 4 * 129 * 129 + 2, 12, 16
    slot = h.hcp_slot_bytes(16, nrec_c, xl, lists, 1)
    # 1 000 bundles of 16, three workgroups of 256 threads per CU: 768 resident and an eighth more; beside them the member-minor slowness; within 70 % of the room
    need = (768 + 96) * slot + nmaps * nrec_c * 4
    assert choose(h, [16] * 1000, bundle=16, room=int(need / 0.7) + (1 << 20))[0] == 16
    assert choose(h, [16] * 1000, bundle=16, room=int(need / 0.7) - (1 << 20))[0] == 0
    # a launch takes no more than `step` units, so no more bundles either: 100 bundles need 100 slots
    need = 100 * slot + nmaps * nrec_c * 4
    assert choose(h, [16] * 1000, bundle=16, step=100, room=int(need / 0.7) + (1 << 20))[0] == 16
    assert choose(h, [16] * 1000, bundle=16, step=100, room=int(need / 0.7) - (1 << 20))[0] == 0


def test_solo_units_are_units_minus_covered(h):
    counts = [16, 17, 18, 1, 2]
    assert choose(h, counts, bundle=16) == (16, False, 54 - 52)
    assert choose(h, counts, bundle=4) == (4, False, 54 - (16 + 16 + 18 + 2))
    assert choose(h, [5, 9, 1], bundle=8) == (8, False, 15 - (5 + 8))
    for n in (250, 1000):
        G, _, solo = choose(h, [16, 17, 1] * n)
        assert G == 16 and solo == 2 * n


# The calls of profiles/r17_bundle_plan_refactor_ab.log with ample room: bundle_size / bundle_threads as the parent commit reported them on
# the GPU (a call without bundles reports no threads)
RAGGED = [(1, 2, 5, 16)[s % 4] for s in range(40)]
AB_PICKS = [("a-129-ragged-auto", dict(counts=RAGGED, nn=129, step=240), 0, 0),
            ("a-129-ragged-4", dict(counts=RAGGED, nn=129, step=240, bundle=4), 4, 256),
            ("a-129-ragged-8", dict(counts=RAGGED, nn=129, step=240, bundle=8), 8, 256),
            ("a-129-ragged-16", dict(counts=RAGGED, nn=129, step=240, bundle=16), 16, 256),
            ("b-257-200x16", dict(counts=[16] * 200, nn=257, step=3200), 8, 256),
            ("c-1025-250x16", dict(counts=[16] * 250, step=4000), 16, 768),
            ("d-1025-1000x16-tail1", dict(counts=[16] * 1000, step=16000, tail=1), 16, 256),
            ("d-1025-1000x16-tail0", dict(counts=[16] * 1000, step=16000, tail=0), 16, 256),
            ("e-1025-1000x16-chunk4096-tail1", dict(counts=[16] * 1000, step=4096, tail=1), 16, 256),
            ("e-1025-1000x16-chunk4096-tail0", dict(counts=[16] * 1000, step=4096, tail=0), 16, 256),
            ("f-129x257-40x8-auto", dict(counts=[8] * 40, nn=129, nnz=257, nmaps=8, step=320), 0, 0),
            ("f-129x257-40x8-8", dict(counts=[8] * 40, nn=129, nnz=257, nmaps=8, step=320, bundle=8), 8, 256),
            ("g-1025-64x16", dict(counts=[16] * 64, step=1024), 4, 768)]


@pytest.mark.parametrize("case", AB_PICKS, ids=lambda c: c[0])
def test_picks_of_the_ab_calls(h, case):
    _, kw, G, threads = case
    got, wide, _ = choose(h, **kw)
    assert got == G and (not G or (768 if wide else 256) == threads)


# ---- invariants on random ragged unit sets -----------------------------------------------------------------------------------------------
COMBOS = list(itertools.product((1, 0), (0, 2, 4), (0, 1), (0, 1), (256, 768)))          # automatic / forced, members per lane, tail, order, threads


def random_sets():
    """about 200 ragged sets, 1 to 40 units per source; every eighth large enough for a second group (600 to 1600 bundles)"""
    rng = np.random.default_rng(20251017)
    for k in range(200):
        G = (4, 8, 16)[k % 3]
        auto, mpl, tail, order, threads = COMBOS[(k // 3) % len(COMBOS)]
        if k % 8 == 0:          # (the large ones with the options under which a second group forms)
            G, auto, mpl, tail, order, threads = (8, 16)[(k // 8) % 2], 1, 0, (k // 16) % 2, (k // 32) % 2, 256
        per_source = {4: 5.6, 8: 3.0, 16: 1.75}[G]
        nsrc = int(rng.integers(600, 1600) / per_source) if k % 8 == 0 else int(rng.integers(1, 60))
        counts = rng.integers(1, 41, nsrc)
        src = units_of(counts, "period" if k % 2 else "source")
        sx, sz = synth.sources(19, nsrc, seed=int(rng.integers(1, 1 << 30)))
        yield G, options(bundle=1 if auto else G, mpl=mpl, tail=tail, order=order, threads=threads), counts, src, sx, sz


def check_invariants(h, grid, G, opt, counts, src, sx, sz):
    d = layout(h, grid, sx[src], sz[src], G, opt)
    n, a, b = src.size, d["a"], d["b"]
    assert a >= 0 and set(np.unique(d["flag"])) <= {0, 1, 2}
    member = d["bundle"] >= 0
    assert ((d["flag"] == 0) == ~member).all() and d["nsolo"] == int((~member).sum())
    # every unit solo or in exactly one bundle: the places of a bundle are 0 .. size - 1, each once
    assert d["sizes"].size == a + b and d["sizes"].sum() == member.sum()
    pairs = d["bundle"][member].astype(np.int64) * 64 + d["place"][member]
    assert np.unique(pairs).size == pairs.size and (d["place"][member] < d["sizes"][d["bundle"][member]]).all()
    # one source per bundle
    if a + b: assert np.unique(np.stack([d["bundle"][member], src[member]]), axis=1).shape[1] == a + b
    halves = b > 0 and d["Gb"] == G // 2
    assert (d["sizes"][:a] >= 2).all() and (d["sizes"][:a] <= G).all()
    if b: assert (d["sizes"][a:] >= 2).all() and (d["sizes"][a:] <= d["Gb"]).all() and d["Gb"] in (G, G // 2)
    assert ((d["flag"] == 2) == (member & (d["bundle"] >= a) if b and d["threads_b"] == 768 else np.zeros(n, bool))).all()          # the wide tail's members
    nb, covered = census(h, counts, G)
    assert member.sum() == covered and a + b - (b // 2 if halves else 0) == nb
    # ranks: a permutation, solo units first, then the members bundle by bundle
    assert (np.sort(d["rank"]) == np.arange(n)).all() and (d["rank"][~member] < d["nsolo"]).all()
    start = d["nsolo"] + np.concatenate([[0], np.cumsum(d["sizes"])[:-1]]) if a + b else np.zeros(0, np.int64)
    assert (d["rank"][member] == start[d["bundle"][member]] + d["place"][member]).all()
    return b > 0


def test_invariants_on_random_unit_sets(h):
    g = rect_grid()
    second = sum(check_invariants(h, g, *s) for s in random_sets())
    assert second >= 10         # (the sets reach the second group, wide and in halves)


# ---- field slots ---------------------------------------------------------------------------------------------------------------------------
def slots(h, a, b=0, G=16, Gb=0, mpl_now=4, mpl_b=2, threads_a=256, threads_b=256, nrec_c=1 << 14, xl=10, lists=100, bstride=1, pool=0, room=AMPLE):
    lay = np.array([a, b, G, Gb, mpl_now, mpl_b, threads_a, threads_b], np.int32)
    gr = np.zeros(16, np.int64); tot = np.zeros(4, np.int64)
    h.hcp_slots(L.ptr(lay), nrec_c, xl, lists, bstride, pool, room, L.ptr(gr), L.ptr(tot))
    names = ("G", "count", "slots", "xlog", "b_stride", "b_off", "exc_off", "slot0")
    return [dict(zip(names, (int(v) for v in gr[q * 8:q * 8 + 8]))) for q in range(2)], dict(zip(("b", "exc", "slots", "no_room_for"), (int(v) for v in tot)))


def test_slots_are_the_bundles_the_resident_ones_the_option_or_the_room(h):
    # resident: 256 CUs x one workgroup of 512 threads or more, three of 256 with two members per lane or 16 members, else two; and an eighth more
    for kw, resident in ((dict(G=16), 768), (dict(G=8, mpl_now=4), 512), (dict(G=8, mpl_now=2), 768), (dict(G=4, mpl_now=4, threads_a=768), 256), (dict(G=16, threads_a=512), 256)):
        for count in (1, resident, resident + resident // 8, 5000):
            g, t = slots(h, count, **kw)
            assert g[0]["slots"] == min(count, resident + resident // 8) and t["slots"] == g[0]["slots"] and t["no_room_for"] == 0
    assert slots(h, 5000, pool=10)[0][0]["slots"] == 10 and slots(h, 7, pool=10)[0][0]["slots"] == 7 and slots(h, 5000, pool=2000)[0][0]["slots"] == 2000
    slot = h.hcp_slot_bytes(16, 1 << 14, 10, 100, 1)
    for fit in (1, 5, 863):
        assert slots(h, 5000, room=int((fit + 0.5) * slot / 0.7))[0][0]["slots"] == fit
        assert slots(h, 5000, pool=2000, room=int((fit + 0.5) * slot / 0.7))[0][0]["slots"] == fit
    g, t = slots(h, 5000, room=int(0.9 * slot / 0.7))
    assert t["no_room_for"] == slot


def test_two_groups_share_the_room_and_do_not_overlap(h):
    nrec_c, xl, lists = 1 << 14, 10, 100
    s16, s8 = h.hcp_slot_bytes(16, nrec_c, xl, lists, 1), h.hcp_slot_bytes(8, nrec_c, xl, lists, 1)
    for Gb, tb, mb, res_b in ((8, 256, 2, 768), (16, 768, 4, 256)):
        g, t = slots(h, 768, 464, Gb=Gb, mpl_b=mb, threads_b=tb)
        assert [r["slots"] for r in g] == [768, min(464, res_b + res_b // 8)]
        assert [r["xlog"] for r in g] == [xl + 4, xl + (3 if Gb == 8 else 4)] and [r["b_stride"] for r in g] == [17 * nrec_c, (Gb + 1) * nrec_c]
        # cumulative, the second group behind the first
        assert (g[0]["b_off"], g[0]["exc_off"], g[0]["slot0"]) == (0, 0, 0)
        assert (g[1]["b_off"], g[1]["exc_off"], g[1]["slot0"]) == (768 * 17 * nrec_c, 768 << (xl + 4), 768)
        assert t["b"] == g[1]["b_off"] + g[1]["slots"] * g[1]["b_stride"] and t["exc"] == g[1]["exc_off"] + (g[1]["slots"] << g[1]["xlog"]) and t["slots"] == 768 + g[1]["slots"]
    # each group gets half of the room's share
    room = int(200.5 * s16 / 0.7)
    g, t = slots(h, 768, 464, Gb=8, room=room)
    assert g[0]["slots"] == 100 and g[1]["slots"] == min(464, int(0.7 * room) // s8 // 2)
    assert slots(h, 768, 0, room=room)[0][0]["slots"] == 200
    assert slots(h, 768, 464, Gb=8, room=int(1.9 * s16 / 0.7))[1]["no_room_for"] == s16
