"""Geometries the parity tests visit besides the squares at colatitude 60 degrees of tests/synth.py: rectangles both ways, unequal
spacings in latitude and longitude, high northern and southern latitudes (the three reduction branches of ray_core.h's sinf_libm),
negative longitudes, a grid that straddles the equator with its first longitude at 0, and a third dicing.  Shared by the pin of the
oracle to the reference (tests/test_oracle_vs_ref.py: test_fields_rays_geometry) and the device tests (tests/test_gpu_geometry.py).

Data only: this module imports neither the engine nor pytest.

Sources are given in nodes of the propagation grid (node 0 .. N - 1 on each axis).  None lies nearer than EDGE nodes to the node
count of either axis, f <= N - EDGE: in the last cells before a high edge the reference's start-up march is not reproducible (it
leaves NaN at thousands of nodes, a count that changes with the geometry; NOTEBOOK.md, tests/test_gpu_rows.py edge_plan), so such
inputs pin nothing.  `plan` asserts the bound.
"""
import numpy as np

import synth
from solve_units import medium          # noqa: F401  (synth.medium's formulas on nx x ny vertices)

EDGE = 2.3

# name: (nx, ny, goxd, gozd, dvxd, dvzd, dicing, media)
CASES = {
    "tall": (18, 35, 30.0, 100.0, 0.01, 0.01, 8, ("smooth", "homog")),
    "wide5": (35, 18, 30.0, 100.0, 0.01, 0.01, 5, ("rough",)),
    "unequal": (18, 18, 30.0, 100.0, 0.01, 0.013, 8, ("smooth",)),
    "taipei": (18, 18, 25.2, 121.35, 0.015, 0.017, 8, ("rough", "homog")),
    "north65": (20, 14, 65.0, 170.0, 0.02, 0.05, 8, ("rough", "homog")),
    "north80": (14, 20, 80.0, -120.0, 0.02, 0.1, 8, ("smooth",)),
    "south50": (12, 23, -50.0, -70.0, 0.03, 0.02, 8, ("rough", "homog")),
    "equator": (16, 16, 0.05, 0.0, 0.01, 0.01, 8, ("smooth", "rough")),
    "dice3": (30, 22, 40.0, 5.0, 0.02, 0.03, 3, ("rough",)),
}
PAIRS = [(name, kind) for name, row in CASES.items() for kind in row[7]]
NSRC, NREC = 6, 4


def geometry(name):
    """(nx, ny, goxd, gozd, dvxd, dvzd, dicing) of a case: the arguments of L.grid / Engine.set_maps"""
    return CASES[name][:7]


def nodes(name):
    """(NX, NZ) of the propagation grid"""
    nx, ny, gd = CASES[name][0], CASES[name][1], CASES[name][6]
    return (nx - 3) * gd + 1, (ny - 3) * gd + 1


def plan(name):
    """(sources (NSRC, 2), receivers (NSRC, NREC, 2)) in nodes of the propagation grid, float64: an interior source off the nodes, one
    1.4 cells from the low-x edge, one near the high corner, one on a node, two drawn by synth.LCG in [1.5, N - 3.5]; per source four
    receivers drawn the way test_oracle_vs_ref.fields_rays draws them, in [0.2, N - 1.2]"""
    nx, ny = CASES[name][:2]
    NX, NZ = nodes(name)
    rng = synth.LCG(99 + 64 * nx + ny)
    u = rng.uniform(4)
    src = [(0.43 * NX + 0.3, 0.61 * NZ + 0.6), (1.4, NZ / 2 + 0.2), (NX - 2.5, NZ - 3.3), (5.0, 7.0)]
    src += [(1.5 + u[2 * i] * (NX - 5.0), 1.5 + u[2 * i + 1] * (NZ - 5.0)) for i in range(2)]
    rec = []
    for _ in src:
        v = rng.uniform(2 * NREC)
        rec.append([(0.2 + v[2 * i] * (NX - 1.4), 0.2 + v[2 * i + 1] * (NZ - 1.4)) for i in range(NREC)])
    src, rec = np.array(src), np.array(rec)
    assert src.shape == (NSRC, 2) and rec.shape == (NSRC, NREC, 2)
    assert (src >= 0).all() and (src[:, 0] <= NX - EDGE).all() and (src[:, 1] <= NZ - EDGE).all(), "%s: a source in the last cells before a high edge" % name
    assert (rec >= 0).all() and (rec[:, :, 0] < NX - 1).all() and (rec[:, :, 1] < NZ - 1).all()
    return src, rec


def radians(gox, goz, dnx, dnz, p):
    """node coordinates (..., 2) -> (x, z) fp32 radians the way every test here places a point: gox + fp32(f) * dnx, in fp32"""
    f = np.float32
    p = np.asarray(p)
    return (f(gox) + p[..., 0].astype(f) * f(dnx)).astype(f), (f(goz) + p[..., 1].astype(f) * f(dnz)).astype(f)


def colatitudes(name):
    """colatitude in radians (float64) of the first and the last node line of the propagation grid"""
    nx, ny, goxd, gozd, dvxd, dvzd, gd = geometry(name)
    return np.radians(90.0 - goxd), np.radians(90.0 - goxd + (nx - 3) * dvxd)
