"""The CPU oracle against the reference's own Fortran, bit-exact.  Wider sweep than the golden files.

The reference's side of every comparison is recorded in tests/golden/ref_digests.json (refrecord.py); where
the reference build (oracle/_ref) is present it also runs live and must match the record."""
import json

import numpy as np
import pytest

import _libs as L
import dispersion_cases as D
import geometry_cases as G
import refrecord
import synth


def f32(v):
    return np.asarray(v, np.float32)


FIELDS_RAYS = [(18, "smooth", 8), (35, "checker4", 8), (35, "rough", 8), (35, "smooth", 5)]


def fields_rays(side, nx, kind, gd):
    wb = side.grid(nx, nx, synth.GOXD, synth.GOZD, synth.DVD, synth.DVD, gd)
    try:
        out = {"grid": f32([wb.gox, wb.goz, wb.dnx, wb.dnz])}
        pv = synth.medium(nx, kind)
        out["veln"] = wb.gridder(pv)
        N = wb.nnx
        rng = synth.LCG(99 + nx)
        u = rng.uniform(12)
        frac = [(0.43 * N + 0.3, 0.61 * N + 0.6), (1.4, N / 2 + 0.2), (N - 2.5, N - 3.3), (5.0, 7.0)]
        frac += [(u[2 * i] * (N - 1), u[2 * i + 1] * (N - 1)) for i in range(3)]
        for s, (fx, fz) in enumerate(frac):
            sx = np.float32(wb.gox + np.float32(fx) * wb.dnx)
            sz = np.float32(wb.goz + np.float32(fz) * wb.dnz)
            for k, v in refrecord.canonical_solve(wb.solve(sx, sz)).items():
                out["%s%d" % (k, s)] = v
            v = rng.uniform(8)
            for i in range(4):
                rx = np.float32(wb.gox + np.float32(0.2 + v[2 * i] * (N - 1.4)) * wb.dnx)
                rz = np.float32(wb.goz + np.float32(0.2 + v[2 * i + 1] * (N - 1.4)) * wb.dnz)
                out["t%d_%d" % (s, i)] = f32(wb.srtimes(sx, sz, rx, rz))
                out["fdm%d_%d" % (s, i)] = wb.rpaths(sx, sz, rx, rz)
        return out
    finally:
        wb.close()


@pytest.mark.parametrize("nx,kind,gd", FIELDS_RAYS)
def test_fields_rays_bitwise(nx, kind, gd):
    refrecord.check("fields_rays[%d-%s-%d]" % (nx, kind, gd), lambda side: fields_rays(side, nx, kind, gd))


HEADLINE = [(131, "smooth", 3), (131, "rough", 0), (131, "checker", 0)]


def fields_headline(side, nx, kind, period):
    wb = side.grid(nx, nx, synth.GOXD, synth.GOZD, synth.DVD, synth.DVD, 8)
    try:
        out = {"grid": f32([wb.gox, wb.goz, wb.dnx, wb.dnz])}
        pv = synth.medium(nx, kind, period)
        out["veln"] = wb.gridder(pv)
        N = wb.nnx
        rng = synth.LCG(7 + nx)
        for s, (fx, fz) in enumerate(((0.37 * (N - 1) + 0.3, 0.58 * (N - 1) + 0.6), (N - 9.25, 300.5))):
            sx = np.float32(wb.gox + np.float32(fx) * wb.dnx)
            sz = np.float32(wb.goz + np.float32(fz) * wb.dnz)
            sol = refrecord.canonical_solve(wb.solve(sx, sz))
            out["T%d" % s], out["Tr%d" % s] = sol["T"], sol["Tr"]
            v = rng.uniform(16)
            for i in range(8):
                rx = np.float32(wb.gox + np.float32(0.2 + v[2 * i] * (N - 1.4)) * wb.dnx)
                rz = np.float32(wb.goz + np.float32(0.2 + v[2 * i + 1] * (N - 1.4)) * wb.dnz)
                out["t%d_%d" % (s, i)] = f32(wb.srtimes(sx, sz, rx, rz))
        return out
    finally:
        wb.close()


@pytest.mark.parametrize("nx,kind,period", HEADLINE)
def test_fields_bitwise_at_headline_size(nx, kind, period):
    """1025^2 (BASELINE.json configs[2] size): the oracle's field, refined snapshot and receiver times against
    the reference's travel / srtimes (CalSurfG.f90:288-487, :1636-1759), every bit -- the GPU parity tests at
    this size compare with an oracle that is pinned at this size"""
    refrecord.check("fields_headline[%d-%s-%d]" % (nx, kind, period), lambda side: fields_headline(side, nx, kind, period))


def surfdisp96_sweep(side):
    out = {}
    for m, (thk, vpv, vs, rho, t) in enumerate(L.layered_models(40)):
        for iwave in (1, 2):
            for igr in (0, 1):
                out["c%d_%d%d" % (m, iwave, igr)] = L.surfdisp96(side.name, thk, vpv, vs, rho, 1, iwave, 1, igr, t)
    thk, vpv, vs, rho, t = L.layered_models(1, seed=9)[0]       # flat-earth branch
    for iwave in (1, 2):
        out["flat_%d" % iwave] = L.surfdisp96(side.name, thk, vpv, vs, rho, 0, iwave, 1, 0, t)
    return out


def test_surfdisp96_bitwise():
    """surfdisp96.f:52-350 on 40 random layered models x (Love, Rayleigh) x (phase, group), spherical"""
    refrecord.check("surfdisp96", surfdisp96_sweep)


DEPTH = [(2, 0), (2, 1), (1, 0), (1, 1)]


def depth_kernels(side, iwave, igr):
    c = synth.boundary_case(nx=6, ny=5, nz=7)
    vel = np.ascontiguousarray(c["vels"].T)
    t = np.array([1.0, 2.0, 4.0, 7.0, 11.0, 16.0])
    out = {"pv_only": L.depthkernel(side.name, vel, c["depz"], 1.0, iwave, igr, t, kernels=False)}
    for k, a in zip(("pv", "sen_vs", "sen_vp", "sen_rho"), L.depthkernel(side.name, vel, c["depz"], 1.0, iwave, igr, t)):
        out[k] = a
    return out


@pytest.mark.parametrize("iwave,igr", DEPTH)
def test_depth_kernels_bitwise(iwave, igr):
    """caldespersion (CalSurfG.f90:2320-2368) and depthkernel (:1461-1597) on a 6x5x7 model"""
    refrecord.check("depth_kernels[%d-%d]" % (iwave, igr), lambda side: depth_kernels(side, iwave, igr))


BOUNDARY = [dict(), dict(deep=True, nz=7, nx=10, ny=13, seed=5), dict(kRc=0, kRg=2, kLc=0, kLg=1)]


def boundary(side, kw):
    c = synth.boundary_case(**kw)
    a = L.call_boundary(side.calsurfg, c)
    return {"nar": np.int32(a["nar"]), "dsurf": a["dsurf"], "rw": a["rw"], "iw": a["iw"], "col": a["col"],
            "obst": L.call_boundary(side.synthetic, c, synthetic=True)}


@pytest.mark.parametrize("kw", BOUNDARY)
def test_boundary_bitwise(kw):
    """The whole boundary: CalSurfG (:939-1459) -> dsurf + CSR-ish rows (rw, iw, col, nar) and
    synthetic (:2412-2865, noiselevel 0) -> obst; all four wave types, ragged source/receiver
    counts, the pvRc overwrite by the group-velocity periods"""
    out = refrecord.check("boundary%s" % json.dumps(kw, sort_keys=True), lambda side: boundary(side, kw))
    assert out["nar"] > 0

def fields_rays_geometry(side, name, kind):
    """the body of fields_rays on a row of geometry_cases.CASES: any nx x ny, origin, spacings and dicing"""
    nx, ny, goxd, gozd, dvxd, dvzd, gd = G.geometry(name)
    wb = side.grid(nx, ny, goxd, gozd, dvxd, dvzd, gd)
    try:
        assert (wb.nnx, wb.nnz) == G.nodes(name)
        out = {"grid": f32([wb.gox, wb.goz, wb.dnx, wb.dnz])}
        out["veln"] = wb.gridder(G.medium(nx, ny, kind))
        src, rec = G.plan(name)
        for s in range(G.NSRC):
            sx, sz = G.radians(wb.gox, wb.goz, wb.dnx, wb.dnz, src[s])
            for k, v in refrecord.canonical_solve(wb.solve(sx, sz)).items():
                out["%s%d" % (k, s)] = v
            rx, rz = G.radians(wb.gox, wb.goz, wb.dnx, wb.dnz, rec[s])
            for i in range(G.NREC):
                out["t%d_%d" % (s, i)] = f32(wb.srtimes(sx, sz, rx[i], rz[i]))
                out["fdm%d_%d" % (s, i)] = wb.rpaths(sx, sz, rx[i], rz[i])
        return out
    finally:
        wb.close()


@pytest.mark.parametrize("name,kind", G.PAIRS)
def test_fields_rays_geometry(name, kind):
    """rectangles, unequal spacings, high latitudes north and south, negative longitudes, the equator, dicing 3 (geometry_cases.py): grid
    constants, diced velocity, coarse field, status classes and live times of the refined box, receiver times and the vertex sums of
    every ray (CalSurfG.f90:288-487, :1636-1759, :1771-2318) -- every branch that tells nnx from nnz or dnx from dnz shows here"""
    out = refrecord.check("fields_rays_geometry[%s-%s]" % (name, kind), lambda side: fields_rays_geometry(side, name, kind))
    NX, NZ = G.nodes(name)
    nx, ny = G.geometry(name)[:2]
    assert out["veln"].shape == (NX, NZ) and out["fdm0_0"].shape == (nx, ny)
    # what the case is there for: finite fields everywhere, every refined box with live nodes, every ray leaving vertex sums behind
    for s in range(G.NSRC):
        assert np.isfinite(out["T%d" % s]).all() and out["T%d" % s].max() > 0 and (out["Sr%d" % s] == 0).any(), (name, s)
        for i in range(G.NREC):
            assert np.isfinite(out["fdm%d_%d" % (s, i)]).all() and np.abs(out["fdm%d_%d" % (s, i)]).max() > 0 and out["t%d_%d" % (s, i)] > 0
    if (nx, ny) == (18, 35) or (nx, ny) == (35, 18):
        assert NX != NZ
    if name in ("unequal", "taipei", "north65", "north80", "south50", "dice3"):
        assert out["grid"][2] != out["grid"][3]


# ---- the dispersion inputs of tests/test_gpu_dispersion.py ------------------------------------------------------------------------------------

def dispersion_envelope_cases():
    """name -> (nx, ny, nz, minthk, model, periods, kernels, iwave, igr, rmax, failed roots expected): the model of
    test_every_variant_gives_the_same_bits with kernels and of test_failure_count_and_first_failure without, all four wave kinds, and the
    natural sizes whose models are there for the arithmetic (curves_34400 and curves_8600 are smooth models sized for the lane rule)"""
    out = {}
    for iwave, igr in DEPTH:
        # Love: the columns without any contrast have no root at long periods; Rayleigh: the slow half space has none
        out["variants-%d-%d" % (iwave, igr)] = (6, 4, 12, 3.0, D.edge_model, D.EDGE_T, True, iwave, igr, 45, True)
        out["failures-%d-%d" % (iwave, igr)] = (6, 4, 12, 3.0, D.edge_model, D.EDGE_T[:10], False, iwave, igr, 45, True)
    for name, (nx, ny, nz, minthk, model, t, kernels, iwave, igr, rmax, _) in D.NATURAL.items():
        if name not in ("curves_34400", "curves_8600"):
            out["%s-%d-%d" % (name, iwave, igr)] = (nx, ny, nz, minthk, model, t, kernels, iwave, igr, rmax, NATURAL_FAIL[name])
    return out


# whether a natural size holds failed roots (pv = 0): periods of 90 s and more on edge_model's columns without contrast / with a slow half
# space; nz64 (there for rmax 127, the layer tables in global scratch) reaches 250 km depth and keeps every root up to its 200 s
NATURAL_FAIL = {"rmax64": True, "rmax65": True, "curves_3870": True, "nz64": False, "nper60": True}


def dispersion_envelope(side, case):
    nx, ny, nz, minthk, model, t, kernels, iwave, igr = case[:9]
    vel, depz = model(nx, ny, nz), D.depths(nz)
    r = L.depthkernel(side.name, vel, depz, minthk, iwave, igr, t, kernels)
    return dict(zip(("pv", "sen_vs", "sen_vp", "sen_rho"), r)) if kernels else {"pv": r}


ENVELOPE = dispersion_envelope_cases()


@pytest.mark.parametrize("name", list(ENVELOPE))
def test_dispersion_envelope(name):
    """depthkernel / caldespersion (CalSurfG.f90:1461-1597, :2320-2368) on the inputs the device dispersion tests trust the oracle on:
    low-velocity zones, no contrast, a slow half space, a 1 km/s surface layer, a fast lid; periods from 0.02 s to 1000 s; failed roots;
    rmax 45, 64, 65 and 127; 60 periods in one call"""
    case = ENVELOPE[name]
    nx, ny, nz, minthk = case[:4]
    assert D.layer_count(D.depths(nz), minthk) == case[9]
    out = refrecord.check("dispersion_envelope[%s]" % name, lambda side: dispersion_envelope(side, case))
    failed = out["pv"] == 0
    assert failed.any() == case[10] and not failed.all(axis=0).any(), "%s: %d of %d roots failed" % (name, failed.sum(), failed.size)
    assert all(np.isfinite(a).all() for a in out.values())


def aprod(side):
    import ctypes as C
    r = synth.LCG(2)
    m, n, nar = 50, 40, 900
    row = (1 + (r.uniform(nar) * m).astype(np.int32)).clip(1, m).astype(np.int32)
    col = (1 + (r.uniform(nar) * n).astype(np.int32)).clip(1, n).astype(np.int32)
    rw = (r.uniform(nar) - 0.5).astype(np.float32)
    iw = np.concatenate([[nar], row, col]).astype(np.int32)
    ib = lambda v: C.byref(C.c_int(int(v)))
    out = {}
    for mode in (1, 2):
        x = np.linspace(-1, 1, n).astype(np.float32)
        y = np.linspace(2, -2, m).astype(np.float32)
        side.aprod(ib(mode), ib(m), ib(n), L.ptr(x), L.ptr(y), ib(iw.size), ib(nar), L.ptr(iw), L.ptr(rw))
        out["x%d" % mode], out["y%d" % mode] = x, y
    return out


def test_aprod_bitwise():
    refrecord.check("aprod", aprod)


def recorded_cases():
    """(name, body) of every check above, for tests/golden/make_golden.py"""
    for nx, kind, gd in FIELDS_RAYS:
        yield "fields_rays[%d-%s-%d]" % (nx, kind, gd), lambda side, a=(nx, kind, gd): fields_rays(side, *a)
    for nx, kind, period in HEADLINE:
        yield "fields_headline[%d-%s-%d]" % (nx, kind, period), lambda side, a=(nx, kind, period): fields_headline(side, *a)
    yield "surfdisp96", surfdisp96_sweep
    for iwave, igr in DEPTH:
        yield "depth_kernels[%d-%d]" % (iwave, igr), lambda side, a=(iwave, igr): depth_kernels(side, *a)
    for kw in BOUNDARY:
        yield "boundary%s" % json.dumps(kw, sort_keys=True), lambda side, kw=kw: boundary(side, kw)
    yield "aprod", aprod
    for name, kind in G.PAIRS:
        yield "fields_rays_geometry[%s-%s]" % (name, kind), lambda side, a=(name, kind): fields_rays_geometry(side, *a)
    for name, case in ENVELOPE.items():
        yield "dispersion_envelope[%s]" % name, lambda side, case=case: dispersion_envelope(side, case)
