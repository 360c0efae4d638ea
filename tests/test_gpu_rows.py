"""Rays and Frechet rows at scale and in every solve mode, against the oracle.

The core check takes every unit's inputs from the engine after dsa_solve_rows -- its coarse field, refined snapshot and diced
velocity -- traces each ray with the oracle's rpaths (dso_rpaths) and assembles its row with the oracle's row loop
(dso_assemble_row).  The engine's COO rows must equal the concatenation bit for bit, and so must the ray-step count, the number of
clamped rays and the first clamped unit (dsa_ray_diagnostics against the oracle's rbint).  This isolates the tracer and the row
kernels (k_rays, k_row_list, k_row_emit, k_scan) from tie differences of the eikonal solve, so it holds on any medium and in any
mode: default, marched (exact_ties = 1 flagged units, exact_ties = 2), bundled, refined boxes in bundles, the hand-off replay.
Where the engine's fields are the oracle's own (exact_ties = 2; units without ties), the whole chain runs on the oracle as well.

Every case asserts from stats() that the path it is about was taken.  Each test uses an engine of its own.
"""
import concurrent.futures as cf
import ctypes as C
import hashlib
import os
import sys
import time

import numpy as np
import pytest

import _libs as L
import parity_log
import synth
import synth_matrix as SM

NX = 131                    # the headline grid: 1025^2 nodes (bench.py)
WORKERS = 16


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture
def eng():
    """a private engine: the options these tests set (ray_budget, ray_lanes, rows_on_device, keep_fields, ...) die with it"""
    from dsurftomo_amd import build
    from dsurftomo_amd.engine import Engine
    build.build()
    e = Engine(0)
    yield e
    e.close()


def depth_model(nx, ny, nz=9, kmax=1, shallow=False, seed=5):
    """vels (nz, ny, nx) fp32 that vary laterally (so the Brocher coefficients differ from vertex to vertex), depz, and synthetic
    depth kernels sen_* (nz, kmax, ny*nx) fp64 like bench.py's rays leg.  depz(nz-1) < 35 km picks the shallow coefficient set."""
    i = np.arange(nx)[None, None, :]
    j = np.arange(ny)[None, :, None]
    k = np.arange(nz)[:, None, None]
    vels = (2.5 + 0.2 * k + 0.15 * np.sin(2 * np.pi * i / nx + 0.4 * k) * np.cos(3 * np.pi * j / ny)).astype(np.float32)
    depz = (np.arange(nz) * (3.0 if shallow else 36.0 / (nz - 2))).astype(np.float32)
    n = nz * kmax * nx * ny
    sen = [(0.02 + 0.05 * SM.mix(np.arange(n), seed + q)).reshape(nz, kmax, nx * ny) for q in range(3)]
    assert (depz[nz - 2] < 35.0) == shallow
    return vels, depz, sen[0], sen[1], sen[2]


def capacity(u, per_ray=8000):
    return int(np.sum(u["nrec"])) * per_ray


def solve_rows(e, u, dm, sen_slot=None, keep=True):
    """dsa_solve_rows on the plan u with the depth model dm; returns (times, rw, iw, col, stats, (clamped, first clamped unit))"""
    e.keep_fields(keep)
    e.set_depth_kernels(*dm)
    e.plan(u["map_index"], u["scx"], u["scz"], u["nrec"], u["rcx"], u["rcz"], sen_slot=sen_slot)
    t, rw, iw, col = e.solve_rows(capacity(u))
    return t, rw, iw, col, e.stats(), e.ray_diagnostics()


def _trace_unit(g, vn, sol, sx, sz, rcx, rcz, dm, slot, row0):
    A = L.RowAssembler(*dm)
    out = []
    for q in range(rcx.size):
        fdm, rb, ns = L.o_rpaths(g, sol, vn, sx, sz, rcx[q], rcz[q])
        out.append((*A(fdm, slot, row0 + q + 1), rb, ns))
    return out


def oracle_rows(g, u, dm, fields, slots=None, units=None):
    """rows of the plan's rays traced by the oracle on the given fields: fields(k) -> (veln, T, Tr, Sr) of unit k, indexed [ix, iz].
    Returns dict(rw, iw, col, and per ray: steps, rbint, ray_unit) in data order."""
    n = len(u["map_index"])
    units = range(n) if units is None else units
    first = np.concatenate([[0], np.cumsum(u["nrec"])]).astype(np.int64)
    slots = np.zeros(n, np.int32) if slots is None else np.asarray(slots)
    res = {}
    with cf.ThreadPoolExecutor(WORKERS) as pool:
        futs = {}
        for k in units:
            vn, T, Tr, Sr = fields(k)
            b = L.Box()
            assert L.oracle().dso_source_box(C.byref(g), u["scx"][k], u["scz"][k], C.byref(b)) == 0
            assert Tr.shape == (b.nnx, b.nnz), (k, Tr.shape, b.nnx, b.nnz)
            sol = dict(box=b, T=T, Tr=np.ascontiguousarray(Tr), Sr=np.ascontiguousarray(Sr, np.int32))
            a, z = first[k], first[k + 1]
            futs[k] = pool.submit(_trace_unit, g, vn, sol, u["scx"][k], u["scz"][k], u["rcx"][a:z], u["rcz"][a:z], dm, int(slots[k]), int(a))
            if len(futs) >= 4 * WORKERS:           # (bounded memory: a 1025^2 field is 4 MB)
                for kk in list(futs)[:2 * WORKERS]:
                    res[kk] = futs.pop(kk).result()
        for kk in list(futs):
            res[kk] = futs.pop(kk).result()
    rays = [r for k in units for r in res[k]]
    cat = lambda i, t: np.concatenate([r[i] for r in rays]).astype(t) if rays else np.zeros(0, t)
    ray_unit = np.concatenate([np.full(int(u["nrec"][k]), k) for k in units]) if rays else np.zeros(0, int)
    return dict(rw=cat(0, np.float32), iw=cat(1, np.int32), col=cat(2, np.int32), rbint=np.array([r[3] for r in rays]),
                steps=np.array([r[4] for r in rays], np.int64), ray_unit=ray_unit)


def engine_fields(e, u):
    """fields(k) of the engine's resident units (keep_fields)"""
    vel = {}

    def fields(k):
        m = int(u["map_index"][k])
        if m not in vel:
            vel[m] = e.velocity(m)
        T = e.field(k)
        Tr, Sr = e.refined(k)
        return vel[m], T, Tr, Sr.astype(np.int32)
    return fields


def oracle_fields(g, pv):
    """fields(k) solved by the oracle itself (dso_gridder, dso_solve_source)"""
    vel = {}

    def fields(k, u):
        m = int(u["map_index"][k])
        if m not in vel:
            vel[m] = L.o_gridder(g, pv[m])
        s = L.o_solve(g, pv[m], vel[m], u["scx"][k], u["scz"][k])
        return vel[m], s["T"], s["Tr"], s["Sr"]
    return fields


def first_difference(got, want):
    n = min(got["rw"].size, want["rw"].size)
    d = np.flatnonzero((bits(got["rw"][:n]) != bits(want["rw"][:n])) | (got["iw"][:n] != want["iw"][:n]) | (got["col"][:n] != want["col"][:n]))
    if d.size == 0:
        return "first %d entries equal, then one list ends" % n
    i = d[0]
    return "entry %d: row %d col %d value %r, oracle row %d col %d value %r" % (i, got["iw"][i], got["col"][i], got["rw"][i], want["iw"][i],
                                                                            want["col"][i], want["rw"][i])


def assert_rows(got, want, what):
    """COO rows (rw, iw, col) bit for bit"""
    assert got["rw"].size == want["rw"].size and (bits(got["rw"]) == bits(want["rw"])).all() and (got["iw"] == want["iw"]).all() and \
        (got["col"] == want["col"]).all(), "%s: %d entries vs the oracle's %d; %s" % (what, got["rw"].size, want["rw"].size, first_difference(got, want))


def assert_against(run, o, what):
    """an engine run (solve_rows) against oracle_rows: rows, ray steps, clamped rays and the first clamped unit"""
    t, rw, iw, col, st, (clamped, first_unit) = run
    assert_rows(dict(rw=rw, iw=iw, col=col), o, what)
    assert st["nar"] == rw.size and st["rays"] == o["steps"].size
    assert st["ray_steps"] == o["steps"].sum(), (what, st["ray_steps"], int(o["steps"].sum()))
    want_first = int(o["ray_unit"][o["rbint"] == 1].min()) if (o["rbint"] == 1).any() else -1
    assert (clamped, first_unit) == (int((o["rbint"] == 1).sum()), want_first), (what, clamped, first_unit)
    assert st["rays_clamped"] == clamped


def timed(label, t0):
    parity_log.add("%s: %.1f s" % (label, time.perf_counter() - t0))


def headline_plan(nsrc=256, nper=1, nrec=32):
    return synth.units(NX, nsrc, nper, nrec)


# ---- 1, 2: the headline grid -----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_headline_rows_with_one_and_four_lanes_per_ray(eng):
    """bench.py's rays leg (256 sources x 32 receivers at 1025^2, smooth map, nz = 9) with one lane per ray -- the path of launches
    above 81 920 rays, whose B-spline quotients go through shared reciprocals (ray_core.h) -- and with four: both equal the oracle on
    the engine's fields, and each other; then once more with the rows kept on the device and copied to host arrays"""
    t0 = time.perf_counter()
    u = headline_plan()
    pv = synth.medium(NX, "smooth", 0)
    dm = depth_model(NX, NX)
    e = eng
    e.set_maps(NX, NX, synth.GOXD, synth.GOZD, synth.DVD, synth.DVD, pv)
    g = L.grid(NX, NX, synth.GOXD, synth.GOZD, synth.DVD, synth.DVD)
    e.set_option("ray_lanes", 1)
    r1 = solve_rows(e, u, dm)
    o = oracle_rows(g, u, dm, engine_fields(e, u))
    digest = [hashlib.sha256(e.field(k).tobytes()).digest() for k in range(len(u["nrec"]))]
    assert_against(r1, o, "one lane per ray")
    assert r1[1].size > 1_000_000 and r1[4]["ray_steps"] > 100 * r1[4]["rays"]
    e.set_option("ray_lanes", 4)
    r4 = solve_rows(e, u, dm)
    assert [hashlib.sha256(e.field(k).tobytes()).digest() for k in range(len(u["nrec"]))] == digest     # the same fields as the first run
    assert_against(r4, o, "four lanes per ray")
    e.set_option("ray_lanes", 0)
    e.set_option("rows_on_device", 1)
    rd = solve_rows(e, u, dm)
    assert_against(rd, o, "rows on the device, copied out")
    assert bits(rd[0]).tolist() == bits(r1[0]).tolist() == bits(r4[0]).tolist()
    parity_log.add("rows at 1025^2 smooth: %d rays, %d entries, %d steps, %d clamped: one lane, four lanes and device-resident rows equal the "
                   "oracle on the engine's fields bit for bit" % (o["steps"].size, o["rw"].size, o["steps"].sum(), (o["rbint"] == 1).sum()))
    timed("rows at 1025^2, three runs and the oracle", t0)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,lanes", [("rough", 1), ("checker", 0)])
def test_headline_rows_on_rough_and_checker_media(eng, kind, lanes):
    """the same workload on a rough and on the checkerboard medium in the default mode: on the checkerboard the tie census marches
    units (exact_ties = 1), so rays run on marched fields as well as on fixed-point ones"""
    t0 = time.perf_counter()
    u = headline_plan()
    pv = synth.medium(NX, kind, 0)
    dm = depth_model(NX, NX, shallow=True)
    e = eng
    e.set_maps(NX, NX, synth.GOXD, synth.GOZD, synth.DVD, synth.DVD, pv)
    g = L.grid(NX, NX, synth.GOXD, synth.GOZD, synth.DVD, synth.DVD)
    e.set_option("ray_lanes", lanes)
    r = solve_rows(e, u, dm)
    st = r[4]
    if kind == "checker":
        assert st["exact_units"] > 0
    o = oracle_rows(g, u, dm, engine_fields(e, u))
    assert_against(r, o, kind)
    parity_log.add("rows at 1025^2 %s (%d units marched): %d rays, %d entries equal the oracle on the engine's fields" %
                   (kind, st["exact_units"], o["steps"].size, o["rw"].size))
    timed("rows at 1025^2 %s" % kind, t0)


# ---- 3: bundles --------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_rows_on_bundled_fields(eng):
    """48 sources x 8 periods at 1025^2 in bundles of 8 with their refined boxes in the bundles too (bundle_refined = 2): rows equal
    the oracle on the bundled fields, and equal a bundle = 0 run ray by ray wherever a unit's fields are bit-identical in both"""
    from dsurftomo_amd.engine import Engine
    t0 = time.perf_counter()
    nsrc, nper, nrec = 48, 8, 16
    u = synth.units(NX, nsrc, nper, nrec)
    pv = np.stack([synth.medium(NX, "smooth", p) for p in range(nper)])
    dm = depth_model(NX, NX, kmax=nper, seed=9)
    slots = u["map_index"]
    g = L.grid(NX, NX, synth.GOXD, synth.GOZD, synth.DVD, synth.DVD)
    e = eng
    e.set_maps(NX, NX, synth.GOXD, synth.GOZD, synth.DVD, synth.DVD, pv)
    e.set_option("bundle", 8)
    e.set_option("bundle_refined", 2)
    rb = solve_rows(e, u, dm, sen_slot=slots)
    assert rb[4]["bundle_size"] == 8 and rb[4]["bundled_units"] > 0
    o = oracle_rows(g, u, dm, engine_fields(e, u), slots=slots)
    assert_against(rb, o, "bundles of 8")
    e0 = Engine(0)
    try:
        e0.set_maps(NX, NX, synth.GOXD, synth.GOZD, synth.DVD, synth.DVD, pv)
        e0.set_option("bundle", 0)
        r0 = solve_rows(e0, u, dm, sen_slot=slots)
        assert r0[4]["bundle_size"] == 0
        n = nsrc * nper
        same = np.zeros(n, bool)
        for k in range(n):
            tb, sb = e.refined(k)
            t0_, s0 = e0.refined(k)
            same[k] = (bits(e.field(k)) == bits(e0.field(k))).all() and ((sb == 0) == (s0 == 0)).all() and (bits(tb[sb == 0]) == bits(t0_[sb == 0])).all()
    finally:
        e0.close()
    assert same.sum() >= n // 2
    rows_b = np.searchsorted(rb[2], np.arange(n * nrec + 1) + 1)      # entries of datum d: [rows[d], rows[d + 1])
    rows_0 = np.searchsorted(r0[2], np.arange(n * nrec + 1) + 1)
    for k in np.flatnonzero(same):
        a, z = k * nrec, (k + 1) * nrec
        gb = slice(rows_b[a], rows_b[z]); g0 = slice(rows_0[a], rows_0[z])
        assert_rows(dict(rw=r0[1][g0], iw=r0[2][g0], col=r0[3][g0]), dict(rw=rb[1][gb], iw=rb[2][gb], col=rb[3][gb]), "unit %d, bundle 0 vs 8" % k)
    parity_log.add("rows on bundled fields at 1025^2 (%d units in bundles of 8, refined boxes bundled): equal the oracle on the fields; "
                   "%d of %d units have bit-identical fields without bundles and the same rows" % (n, same.sum(), n))
    timed("rows on bundled fields", t0)


# ---- 4: the march's fields end to end ---------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_rows_under_exact_ties_2_against_the_full_oracle(eng):
    """exact_ties = 2 marches every unit like the reference: 16 units at 1025^2 -- T, the refined snapshot and its alive set equal the
    oracle's dso_solve_source, unit by unit, and the rows equal dso_solve_source -> dso_rpaths -> dso_assemble_row"""
    t0 = time.perf_counter()
    u = synth.units(NX, 16, 1, 32)
    pv = synth.medium(NX, "smooth", 1)[None]
    dm = depth_model(NX, NX)
    g = L.grid(NX, NX, synth.GOXD, synth.GOZD, synth.DVD, synth.DVD)
    e = eng
    e.set_maps(NX, NX, synth.GOXD, synth.GOZD, synth.DVD, synth.DVD, pv)
    e.set_option("exact_ties", 2)
    r = solve_rows(e, u, dm)
    assert r[4]["exact_units"] == 16
    of = oracle_fields(g, pv)
    with cf.ThreadPoolExecutor(WORKERS) as pool:
        sols = list(pool.map(lambda k: of(k, u), range(16)))
    assert (bits(e.velocity(0)) == bits(sols[0][0])).all(), "diced velocity"
    for k, (vn, T, Tr, Sr) in enumerate(sols):
        assert (bits(e.field(k)) == bits(T)).all(), "unit %d: coarse field" % k
        tr, sr = e.refined(k)
        assert ((sr == 0) == (Sr == 0)).all(), "unit %d: alive set of the refined snapshot" % k
        # (the tracer reads the snapshot's alive nodes only; the others hold what each solve left there: infinity here, zero in the oracle)
        assert tr.shape == Tr.shape and (bits(tr[Sr == 0]) == bits(Tr[Sr == 0])).all(), "unit %d: refined snapshot" % k
    o = oracle_rows(g, u, dm, lambda k: sols[k])
    assert_against(r, o, "exact_ties = 2, full oracle")
    parity_log.add("rows at 1025^2 under exact_ties = 2: 16 units' fields and %d rays' rows (%d entries) equal the oracle end to end" % (o["steps"].size, o["rw"].size))
    timed("rows under exact_ties = 2", t0)


# ---- 5: geometry edges ---------------------------------------------------------------------------------------------------------

def edge_medium(nx, ny, kind):
    """pv (nx*ny,) on a rectangular grid (latitude index fastest), faster towards all four edges so that rays there leave the grid
    and are clamped"""
    i = np.arange(nx, dtype=np.float64)[None, :]
    j = np.arange(ny, dtype=np.float64)[:, None]
    if kind == "smooth":
        v = 2.9 * (1.0 + 0.10 * np.sin(4 * np.pi * i / nx) * np.cos(3 * np.pi * j / ny))
    else:
        v = 3.0 * (1.0 + 0.13 * np.where(((i // 4) + (j // 4)) % 2 == 0, 1.0, -1.0))
    d = np.minimum(np.minimum(i, nx - 1 - i), np.minimum(j, ny - 1 - j))
    v = v * (1.0 + 0.25 * np.exp(-d / 2.0))
    return np.ascontiguousarray(v.reshape(-1), np.float64)


def edge_plan(g, nmaps):
    """sources and receivers where rays go wrong, in node coordinates (fx along x = colatitude, fz along z = longitude)"""
    f = np.float32
    X, Z = g.nnx - 1, g.nnz - 1                      # last node index
    vx = g.gdx                                       # nodes per vertex cell
    at = lambda fx, fz: (f(g.gox + f(fx) * g.dnx), f(g.goz + f(fz) * g.dnz))
    units = []
    sx, sz = 0.43 * X + 0.3, 0.57 * Z + 0.3
    units.append(((sx, sz), [(sx + 0.2, sz + 0.3),                                 # the source's own cell
                             (sx + 2.5, sz - 3.25), (sx - 6.6, sz + 5.1),          # inside the refined box
                             (sx, sz),                                             # the source itself: no step
                             (float(round(0.2 * X)), 0.35 * Z + 0.4), (0.8 * X + 0.3, float(round(0.15 * Z))),   # node lines
                             (float(round(0.7 * X)), float(round(0.8 * Z))),       # a node
                             (vx * 3.0, 0.3 * Z + 0.7), (0.6 * X + 0.45, vx * 5.0),                # vertex lines: weights exactly 0
                             (vx * 4.0, vx * 7.0), (vx * 2.0 + 0.5, vx * 2.0)]))
    sx, sz = float(round(0.3 * X)), float(round(0.6 * Z))                          # a source on a node
    units.append(((sx, sz), [(sx + 3.0, sz), (sx, sz - 4.0), (sx + vx, sz + vx), (0.9 * X, 0.1 * Z + 0.2)]))
    # the outermost cells: pairs hugging every edge (clamped rays) and the corners
    e1, e2 = 0.004, 0.996
    units.append(((e1, 0.1 * Z), [(e1, 0.9 * Z), (0.3, 0.5 * Z), (0.5, Z - 0.4), (X - 0.3, 0.2)]))
    units.append(((X - 0.9, 0.15 * Z), [(X - e1 - 0.001, 0.85 * Z), (X - 0.6, 0.5 * Z + 0.1), (0.4, 0.3)]))
    units.append(((0.2 * X, e1), [(0.8 * X, e1), (0.5 * X, 0.4), (X - 0.5, Z - 0.5)]))
    units.append(((0.15 * X, Z - 0.9), [(0.9 * X, Z - e1 - 0.001), (0.5 * X + 0.2, Z - 0.6), (0.3, 0.2)]))
    # sources in the last cell before each edge: refined boxes cut by the edge (open on that side)
    for s in ((X - 0.9, 0.5 * Z + 0.25), (0.5, 0.45 * Z), (0.55 * X, Z - 0.9), (0.35 * X, 0.5), (X - 0.9, Z - 0.9), (0.6, 0.7)):
        units.append((s, [(max(s[0] - 1.3, 0.2), min(s[1] + 0.6, Z - 0.1)), (0.5 * X + 0.1, 0.5 * Z + 0.3), (X - s[0] + 0.1, Z - s[1] + 0.2), (e2, s[1])]))
    # nearer to a high edge: the reference's own start-up march ends with nothing alive and its field stays zero (the engine's reads
    # infinite); every ray from there has NaN gradients, is clamped and runs nnx * nnz steps
    ndeg = len(units)
    for s in ((X - 0.3, 0.3 * Z), (0.4 * X, Z - 0.3), (X - 0.2, Z - 0.2), (X - e1 - 0.001, 0.15 * Z), (0.15 * X, Z - e1 - 0.001)):
        units.append((s, [(0.5 * X + 0.3, 0.6 * Z + 0.1), (s[0] - 2.6, s[1] - 1.7)]))
    u = dict(map_index=[], scx=[], scz=[], nrec=[], rcx=[], rcz=[])
    for m in range(nmaps):
        for (s, recs) in units:
            for (fx, fz) in [s] + recs:
                assert 0 <= fx < X and 0 <= fz < Z
            x, z = at(*s)
            u["map_index"].append(m); u["scx"].append(x); u["scz"].append(z); u["nrec"].append(len(recs))
            for r in recs:
                x, z = at(*r)
                u["rcx"].append(x); u["rcz"].append(z)
    u = {k: np.asarray(v, np.int32 if k in ("map_index", "nrec") else np.float32) for k, v in u.items()}
    u["degenerate"] = np.concatenate([m * len(units) + np.arange(ndeg, len(units)) for m in range(nmaps)])
    return u


def check_full_oracle_where_fields_agree(e, g, u, pv, dm, r, label):
    """units that hold no tie and whose fields equal the oracle's: their rows from the oracle alone, start to finish"""
    flags, _ = e.unit_ties()
    of = oracle_fields(g, pv)
    n = len(u["nrec"])
    agree = []
    for k in range(n):
        if flags[k] != 0:
            continue
        vn, T, Tr, Sr = of(k, u)
        tr, sr = e.refined(k)
        if (bits(e.field(k)) == bits(T)).all() and ((sr == 0) == (Sr == 0)).all() and (bits(tr[Sr == 0]) == bits(Tr[Sr == 0])).all():
            assert (bits(e.velocity(int(u["map_index"][k]))) == bits(vn)).all()
            agree.append(k)
    assert len(agree) >= 1, (label, n)
    o = oracle_rows(g, u, dm, lambda k: of(k, u), slots=u["map_index"], units=agree)
    first = np.concatenate([[0], np.cumsum(u["nrec"])])
    lo = np.searchsorted(r[2], first + 1)
    sel = np.concatenate([np.arange(lo[k], lo[k + 1]) for k in agree])
    assert_rows(dict(rw=r[1][sel], iw=r[2][sel], col=r[3][sel]), o, label + ", full oracle")
    return len(agree)


@pytest.mark.gpu
@pytest.mark.parametrize("nx,ny,lanes", [(35, 35, 1), (41, 29, 4)])
def test_rows_at_geometry_edges(eng, nx, ny, lanes):
    """receivers in the source's cell and refined box, on node lines and on vertex lines (B-spline weights exactly 0), sources and
    receivers in the outermost cells (clamped rays: rbint, dsa_ray_diagnostics), sources in the last cell before an edge; a square and
    a non-square grid, one and four lanes per ray, two media, the shallow Brocher set on one grid"""
    t0 = time.perf_counter()
    g = L.grid(nx, ny, synth.GOXD, synth.GOZD, synth.DVD, synth.DVD)
    pv = np.stack([edge_medium(nx, ny, "smooth"), edge_medium(nx, ny, "checker")])
    u = edge_plan(g, 2)
    dm = depth_model(nx, ny, kmax=2, shallow=nx == ny, seed=nx)
    slots = u["map_index"]
    e = eng
    e.set_maps(nx, ny, synth.GOXD, synth.GOZD, synth.DVD, synth.DVD, pv)
    assert (e.nnx, e.nnz) == (g.nnx, g.nnz)
    e.set_option("ray_lanes", lanes)
    r = solve_rows(e, u, dm, sen_slot=slots)
    st = r[4]
    assert st["rays_clamped"] >= 1
    o = oracle_rows(g, u, dm, engine_fields(e, u), slots=slots)
    assert_against(r, o, "geometry edges %dx%d" % (nx, ny))
    assert (o["steps"] == 0).sum() >= 2                 # (the receiver on the source, for both maps)
    # the degenerate units: the reference's field is zero, the engine's has no finite node, and their rays are the reference's all the same
    of = oracle_fields(g, pv)
    for k in u["degenerate"]:
        assert of(k, u)[1].max() == 0 and not np.isfinite(e.field(k)).any(), k
    deg = np.isin(o["ray_unit"], u["degenerate"])
    assert (o["rbint"][deg] == 1).all() and (o["steps"][deg] == g.nnx * g.nnz).all()
    od = oracle_rows(g, u, dm, lambda k: of(k, u), slots=slots, units=u["degenerate"])
    sel = np.isin(r[2], np.flatnonzero(np.isin(np.repeat(np.arange(len(u["nrec"])), u["nrec"]), u["degenerate"])) + 1)
    assert_rows(dict(rw=r[1][sel], iw=r[2][sel], col=r[3][sel]), od, "geometry edges %dx%d, degenerate sources, full oracle" % (nx, ny))
    agree = check_full_oracle_where_fields_agree(e, g, u, pv, dm, r, "geometry edges %dx%d" % (nx, ny))
    parity_log.add("rows at geometry edges %dx%d nodes: %d rays (%d clamped, first in unit %d), %d entries equal the oracle on the engine's "
                   "fields; %d of %d units also equal the oracle end to end" % (g.nnx, g.nnz, o["steps"].size, r[5][0], r[5][1], o["rw"].size,
                                                                                  agree, len(u["nrec"])))
    timed("rows at geometry edges %dx%d" % (nx, ny), t0)


@pytest.mark.gpu
def test_rows_on_fields_after_the_hand_off_replay(eng):
    """a slice of test_gpu_exact.py's hand-off generator (161^2, dicing 5, sources on node lines and up to the edge): the units that
    the replay resolves, found by a times-only call without the replay, traced with the replay on"""
    sys.path.insert(0, os.path.join(L.ROOT, "tools"))
    import fuzz_sources
    t0 = time.perf_counter()
    keep, env = synth.sources, {k: os.environ.get(k) for k in ("DSA_FUZZ_SNAP", "DSA_FUZZ_INNER")}
    os.environ["DSA_FUZZ_SNAP"] = "1"; os.environ["DSA_FUZZ_INNER"] = "1.0"
    try:
        fuzz_sources.install()
        nx, nsrc, nper, nrec, gd = 35, 1000, 16, 32, 5
        full = synth.units(nx, nsrc, nper, nrec, gd=gd, seed=synth.SEED + 2253)
    finally:
        synth.sources = keep
        for k, v in env.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v
    e = eng
    pv = np.stack([synth.medium(nx, "smooth", p) for p in range(nper)])
    e.set_maps(nx, nx, synth.GOXD, synth.GOZD, synth.DVD, synth.DVD, pv, dicing=gd)
    g = L.grid(nx, nx, synth.GOXD, synth.GOZD, synth.DVD, synth.DVD, gd)
    e.set_option("handoff_replay", 0)
    e.plan(**full); e.solve()
    flags, _ = e.unit_ties()
    # rays need every receiver strictly inside the grid
    fx = lambda x: (x - np.float32(g.gox)) / np.float32(g.dnx)
    fz = lambda z: (z - np.float32(g.goz)) / np.float32(g.dnz)
    inside = lambda x, z: (fx(x) > 0.01) & (fx(x) < g.nnx - 1.01) & (fz(z) > 0.01) & (fz(z) < g.nnz - 1.01)
    ok = inside(full["rcx"], full["rcz"]).reshape(-1, nrec).all(axis=1) & inside(full["scx"], full["scz"])
    marched = np.flatnonzero(((flags & 2) != 0) & ok)
    others = np.flatnonzero(((flags & 2) == 0) & ok)[::500]
    pick = np.sort(np.concatenate([marched[:48], others]))
    assert marched.size >= 1
    ray = (pick[:, None] * nrec + np.arange(nrec)[None, :]).reshape(-1)
    u = dict(map_index=full["map_index"][pick], scx=full["scx"][pick], scz=full["scz"][pick], nrec=full["nrec"][pick], rcx=full["rcx"][ray],
             rcz=full["rcz"][ray])
    dm = depth_model(nx, nx, kmax=nper, seed=3)
    slots = u["map_index"]
    e.set_option("handoff_replay", 1)
    r = solve_rows(e, u, dm, sen_slot=slots)
    assert r[4]["handoffs_replayed"] >= 1
    o = oracle_rows(g, u, dm, engine_fields(e, u), slots=slots)
    assert_against(r, o, "hand-off replay")
    parity_log.add("rows after the hand-off replay (N=%d, dicing 5): %d units (%d refined boxes replayed, %d marched), %d rays, %d entries equal "
                   "the oracle on the engine's fields" % (g.nnx, pick.size, r[4]["handoffs_replayed"], r[4]["exact_units"], o["steps"].size, o["rw"].size))
    timed("rows after the hand-off replay", t0)


# ---- 6: device-resident rows across ray launches and chunks ---------------------------------------------------------------------

@pytest.mark.gpu
def test_device_resident_rows_across_launches_and_chunks(eng):
    """rows_on_device with 64 rays per launch (ray_budget = 40 000) and two units per chunk: the resident rows grow launch after launch
    (Engine::trace_chunk, ensure_keep), and dsa_iteration_system_device + dsa_lsmr on them equal dsa_iteration_system + dsa_lsmr on the
    host rows of the same plan, every output bit for bit"""
    t0 = time.perf_counter()
    nx, nz, nsrc, nper, nrec = 35, 6, 6, 2, 48
    u = synth.units(nx, nsrc, nper, nrec, seed=synth.SEED + 5)
    pv = np.stack([synth.medium(nx, "smooth", p) for p in range(nper)])
    dm = depth_model(nx, nx, nz=nz, kmax=nper, seed=21)
    slots = u["map_index"]
    e = eng
    L_ = e._L
    e.set_maps(nx, nx, synth.GOXD, synth.GOZD, synth.DVD, synth.DVD, pv)
    e.set_option("ray_budget", 40000)
    e.set_option("max_chunk", 2)
    dall = nsrc * nper * nrec
    maxvp = (nx - 2) * (nx - 2) * (nz - 1)
    # host rows
    dsyn, rw, iw, col, st, diag = solve_rows(e, u, dm, sen_slot=slots, keep=False)
    assert st["chunk"] == 2 and diag[0] == st["rays_clamped"]
    nar = rw.size
    obst = (dsyn * (1.0 + 0.04 * (SM.mix(np.arange(dall), 3) - 0.5))).astype(np.float32)
    cap = nar + 7 * maxvp
    hrw = np.zeros(cap, np.float32); hrw[:nar] = rw
    hcol = np.zeros(cap, np.int32); hcol[:nar] = col
    hiw = np.zeros(2 * cap + 1, np.int32); hiw[1:nar + 1] = iw
    f = np.float32
    out = {}
    for side in ("host", "device"):
        out[side] = dict(cbst=np.zeros(dall + maxvp, f), datweight=np.zeros(dall, f), norm=np.zeros(maxvp, f), dws=np.zeros(2, f))
    m, nar2 = C.c_int(0), C.c_longlong(0)
    L_.dsa_iteration_system.argtypes = [C.c_int] * 4 + [C.c_longlong] * 2 + [C.c_void_p] * 5 + [C.c_float] * 2 + [C.c_void_p] * 6
    h = out["host"]
    assert L_.dsa_iteration_system(nx, nx, nz, dall, nar, cap, L.ptr(hrw), L.ptr(hiw), L.ptr(hcol), L.ptr(obst), L.ptr(dsyn), 3.0, 2.0,
                                   L.ptr(h["cbst"]), L.ptr(h["datweight"]), L.ptr(h["norm"]), C.byref(m), C.byref(nar2), L.ptr(h["dws"])) == 0
    h["m"], n2 = m.value, nar2.value
    e.spmv_load(h["m"], maxvp, hrw[:n2], hiw[1:n2 + 1], hiw[n2 + 1:2 * n2 + 1])
    h.update(e.lsmr(h["cbst"][:h["m"]], 0.5))
    # device rows
    e.set_option("rows_on_device", 1)
    e.set_depth_kernels(*dm)
    e.plan(u["map_index"], u["scx"], u["scz"], u["nrec"], u["rcx"], u["rcz"], sen_slot=slots)
    t_dev, nar_dev = e.solve_rows_device()
    st = e.stats()
    # (no counter reports launches: ray_budget = 40 000 bytes holds fewer than 64 rays' slabs at this grid, and a launch takes at least 64
    # rays -- Engine::trace_chunk -- so the 96 rays of a 2-unit chunk take two launches, and the second grows the resident rows)
    per_ray = (nx * nx + (nx - 2) ** 2) * 4 + 32          # slab and vertex list of a ray (Engine::trace_chunk)
    assert 40000 / per_ray < 64
    launches = np.ceil(np.asarray(u["nrec"]).reshape(-1, 2).sum(axis=1) / 64)
    assert st["chunk"] == 2 and launches.min() >= 2 and nar_dev == nar and (bits(t_dev) == bits(dsyn)).all()
    d = out["device"]
    L_.dsa_iteration_system_device.argtypes = [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 2 + [C.c_float] * 2 + [C.c_void_p] * 6
    assert L_.dsa_iteration_system_device(e._h, nx, nx, nz, dall, L.ptr(obst), L.ptr(t_dev), 3.0, 2.0, L.ptr(d["cbst"]), L.ptr(d["datweight"]),
                                          L.ptr(d["norm"]), C.byref(m), C.byref(nar2), L.ptr(d["dws"])) == 0, e._L.dsa_error_string(e._h)
    d["m"] = m.value
    assert nar2.value == n2 and d["m"] == h["m"]
    x = np.zeros(maxvp, f)
    ii = [C.c_int(-1), C.c_int(-1)]
    ff = [C.c_float(0.0) for _ in range(5)]
    assert L_.dsa_lsmr(e._h, L.ptr(d["cbst"]), 0.5, 1e-6, 1e-6, 100.0, 400, 10, L.ptr(x), *[C.byref(v) for v in ii], *[C.byref(v) for v in ff]) == 0
    d.update(x=x, istop=ii[0].value, itn=ii[1].value, **{k: f(v.value) for k, v in zip(("normA", "condA", "normr", "normAr", "normx"), ff)})
    assert h["itn"] > 3 and h["istop"] == d["istop"] and h["itn"] == d["itn"]
    for k in ("cbst", "datweight", "norm", "dws", "x", "normA", "condA", "normr", "normAr", "normx"):
        assert (bits(np.asarray(h[k], f)) == bits(np.asarray(d[k], f))).all(), k
    parity_log.add("device-resident rows over %d chunks of 2 units, 64 rays per launch: %d entries; system and LSMR (%d iterations) equal the host "
                   "path's bit for bit" % (len(u["nrec"]) // 2, nar, h["itn"]))
    timed("device-resident rows across launches and chunks", t0)


# ---- the quotients of the one-lane tracer's fast branch --------------------------------------------------------------------------

@pytest.mark.gpu
def test_the_fast_branch_divisions_are_the_compilers_division():
    """ray_core.h: with one lane per ray the 32 B-spline weight products of a sub-segment (each zero or at least 2^-100: weights_plain)
    are divided by v^2 through shared reciprocals (divf_by).  Over those operands -- fp32 numerators 2^-100 .. 2^1, denominators
    2^-7 .. 2^14 (v from 0.1 to 100 km/s) -- and the fp64 ranges of the in-contract check, no quotient differs from the compiler's
    division.  Below 2^-102 some do (measured: 15 of 2e8 numerators in [2^-104, 2^-103)), which is why weights_plain stops at 2^-50
    per weight rather than 2^-52: reported, not asserted."""
    from dsurftomo_amd.engine import selfcheck_divisions
    n64, bad64, n32, bad32 = selfcheck_divisions(20261016, 200, [-200, 200, -200, 200, -100, 1, -7, 14])
    parity_log.add("shared-reciprocal divisions, the fast branch's operands (fp32 numerators 2^-100..2^1, denominators 2^-7..2^14): "
                   "fp64 %d pairs, %d differ; fp32 %d pairs, %d differ" % (n64, bad64, n32, bad32))
    m64, w64, m32, w32 = selfcheck_divisions(20261017, 200, [-200, 200, -200, 200, -102, -100, -7, 14])
    parity_log.add("shared-reciprocal divisions, fp32 numerators 2^-102..2^-100, denominators 2^-7..2^14: %d of %d differ" % (w32, m32))
    assert n32 >= 200_000_000 and m32 >= 200_000_000
    assert bad64 == 0 and bad32 == 0 and w64 == 0 and w32 == 0
    _, _, k32, x32 = selfcheck_divisions(20261018, 100, [-200, 200, -200, 200, -104, -103, -7, 14])
    parity_log.add("shared-reciprocal divisions, fp32 numerators 2^-104..2^-103 (products of weights down to 2^-52, no longer divided this way): "
                   "%d of %d differ" % (x32, k32))


# ---- the oracle's pieces compose to its whole ------------------------------------------------------------------------------------

def test_oracle_rays_and_rows_compose_to_dso_calsurfg():
    """no GPU: dso_solve_source -> dso_rpaths -> dso_assemble_row, ray by ray, is dso_calsurfg's matrix (what the GPU tests above
    rely on when they trace the engine's fields with the oracle)"""
    c = synth.boundary_case(kRc=3, kRg=0, kLc=0, kLg=0)
    vel = np.ascontiguousarray(c["vels"].T)
    pv, svs, svp, srho = L.depthkernel("oracle", vel, c["depz"], float(c["minthk"]), 2, 0, c["tRc"])
    whole = L.call_boundary(L.oracle().dso_calsurfg, c)
    g = L.grid(c["nx"], c["ny"], c["goxd"], c["gozd"], c["dvxd"], c["dvzd"])
    A = L.RowAssembler(vel, c["depz"], svs, svp, srho)
    rw, iw, col = [], [], []
    row = 0
    for k in range(c["kmax"]):
        veln = L.o_gridder(g, pv[c["periods"][0, k] - 1])
        for s in range(c["nsrcsurf1"][k]):
            p = c["periods"][s, k] - 1
            sol = L.o_solve(g, pv[p], veln, c["scxf"][s, k], c["sczf"][s, k])
            for q in range(c["nrc1"][s, k]):
                row += 1
                fdm, _, _ = L.o_rpaths(g, sol, veln, c["scxf"][s, k], c["sczf"][s, k], c["rcxf"][q, s, k], c["rczf"][q, s, k])
                a, b, cc = A(fdm, k, row)
                rw.append(a); iw.append(b); col.append(cc)
    got = dict(rw=np.concatenate(rw), iw=np.concatenate(iw), col=np.concatenate(col))
    assert row == c["ndata"] and got["rw"].size == whole["nar"] > 0
    assert_rows(got, whole, "dso_calsurfg")
