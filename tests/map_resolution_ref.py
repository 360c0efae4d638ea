"""Test infrastructure for the resolution of the period maps: the CPU build of dsurftomo_amd/csrc/map_resolution.h
(tests/hostcheck_map_resolution.cpp) behind NumPy, built with columns_ref's flags, the synthetic map systems of the tests, and the
comparison of two sets of figures, each quantity on its own scale.  Nothing under dsurftomo_amd/ imports this module."""
import ctypes as C
import os
import subprocess

import numpy as np

import _libs as L
from columns_ref import FLAGS
from dsurftomo_amd import maps as M

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libhostcheck_map_resolution.so")
SRC = os.path.join(HERE, "hostcheck_map_resolution.cpp")
HDR = [os.path.join(L.ROOT, "dsurftomo_amd", "csrc", "map_resolution.h")]
F = np.float32
_lib = None

WEIGHT, WEIGHT_AZI, DAMP = 2.0, 4.0, 0.01
# (nx, ny, nmaps, nblocks, rays, vertices per ray): n_m = 20, 60, 63, 64, 189, 192 -- below, at and across the panel width of 64 and no
# multiples of it; the rays of a map are more than one wavefront and no multiple of one; with three maps the last has no datum
SYSTEMS = [(7, 6, 2, 1, 150, 6), (7, 6, 3, 3, 200, 6), (11, 9, 2, 1, 170, 9), (10, 10, 2, 1, 190, 8), (11, 9, 2, 3, 200, 9), (10, 10, 3, 3, 200, 7)]
# The tolerance of every comparison with the twin, measured on the twin alone (the convention of sections 21 and 22): the largest difference
# between maps.map_resolution_twin's two routes (normal equations, pinv of the stacked matrix) per system with seed 11, every quantity on
# its own scale as differences() takes it (test_hostcheck_map_resolution.py prints it again), and the factor that covers other seeds.
MEASURED = {20: 6.1e-15, 60: 5.4e-15, 63: 1.4e-14, 64: 7.2e-15, 189: 1.4e-14, 192: 6.8e-15}
FACTOR = 4.0
TOL = FACTOR * max(MEASURED.values())


def load():
    global _lib
    if _lib is not None:
        return _lib
    if L._stale(SO, [SRC] + HDR):
        subprocess.check_call(["g++"] + FLAGS + ["-shared", "-o", SO, SRC, "-lm"])
    lib = C.CDLL(SO)
    lib.hmr_resolution.argtypes = [L.i32] * 6 + [C.c_longlong] + [L.vp] * 3 + [L.f32, L.i32] + [L.vp] * 6
    lib.hmr_factors.argtypes = [L.i32] * 6 + [C.c_longlong] + [L.vp] * 3 + [L.f32, L.i32] + [L.vp] * 5
    _lib = lib
    return lib


def system(nx, ny, nmaps, nblocks, rays, per, seed, weight=WEIGHT, weight_azi=WEIGHT_AZI, unweighted=3, avoid=None):
    """A synthetic map system through maps.map_system: `rays` data rows of `per` vertices each (ascending columns, the same vertices in
    every block, entries of the size of path lengths over c^2 in block 0 and signed in the others), datum d on map d mod nmaps -- with
    three maps the last map's go to map 0 instead, so that it has no datum; `unweighted` data of weight 0; avoid: a vertex no ray touches.
    Returns the dict of map_system with nx, ny, nmaps, nblocks, ndata added."""
    rng = np.random.default_rng(seed)
    layer = (nx - 2) * (ny - 2)
    pool = np.array([i for i in range(layer) if i != avoid])
    rw, row, col = [], [], []
    for d in range(rays):
        k = d % nmaps
        if nmaps > 2 and k == nmaps - 1:
            k = 0
        i0 = np.sort(rng.choice(pool, min(per, pool.size), replace=False))
        for B in range(nblocks):
            f = (0.5 + rng.random(i0.size)) * (1.0 if B == 0 else rng.uniform(-1, 1, i0.size))
            rw.extend(f); row.extend([d + 1] * i0.size); col.extend((B * nmaps + k) * layer + i0 + 1)
    res = (rng.standard_normal(rays) * 0.1).astype(F)
    dw = np.ones(rays, F)
    dw[rng.choice(rays, unweighted, replace=False)] = 0
    S = M.map_system(nx, ny, nmaps, nblocks, np.array(rw, F), np.array(row), np.array(col), res, dw, weight, weight_azi)
    S.update(nx=nx, ny=ny, nmaps=nmaps, nblocks=nblocks, ndata=rays, datweight=dw)
    return S


def _outputs(S, fill):
    nx, ny, nmaps, nblocks = S["nx"], S["ny"], S["nmaps"], S["nblocks"]
    layer = (nx - 2) * (ny - 2)
    return dict(measures=np.full((9, nblocks, nmaps, layer), fill), leverage=np.full(S["ndata"], fill), trace=np.full((nblocks, nmaps), fill),
                nused=np.zeros(nmaps, np.int32), flag=np.zeros(nmaps, np.int32))


def _coo(S, rw=None, row=None, col=None):
    return (np.ascontiguousarray(S["rw"] if rw is None else rw, F), np.ascontiguousarray(S["row"] if row is None else row, np.int32),
            np.ascontiguousarray(S["col"] if col is None else col, np.int32))


def host_resolution(h, S, damp=DAMP, r_map=-1, fill=9.0, **coo):
    """hmr_resolution on a system().  Returns (verdict, dict as Engine.maps_resolution's); verdict 1 a row in two maps, 2 a column twice
    in a row, 3 a column whose rows do not ascend (the outputs are then untouched)."""
    rw, row, col = _coo(S, **coo)
    out = _outputs(S, fill)
    nm = S["nblocks"] * (S["nx"] - 2) * (S["ny"] - 2)
    if r_map >= 0:
        out["R"] = np.full((nm, nm), fill)
    rc = h.hmr_resolution(S["nx"], S["ny"], S["nmaps"], S["nblocks"], S["m"], S["ndata"], rw.size, L.ptr(rw), L.ptr(row), L.ptr(col), damp, r_map,
                          L.ptr(out["measures"]), L.ptr(out["leverage"]), L.ptr(out["trace"]), L.ptr(out["nused"]), L.ptr(out["flag"]),
                          L.ptr(out["R"]) if r_map >= 0 else None)
    return rc, out


def host_all(h, S, damp=DAMP):
    """host_resolution with the R of every map: the dict with R a list, as the twin's"""
    Rs = []
    for k in range(S["nmaps"]):
        rc, out = host_resolution(h, S, damp, k)
        assert rc == 0
        Rs.append(out["R"])
    out["R"] = Rs
    return out


def host_factors(h, S, k, damp=DAMP):
    """(flags, L1, d1, L2, d2): map k's factor by the header's left-looking loop and by the harness's own panelled right-looking one"""
    rw, row, col = _coo(S)
    nm = S["nblocks"] * (S["nx"] - 2) * (S["ny"] - 2)
    L1, L2, d1, d2 = np.zeros((nm, nm)), np.zeros((nm, nm)), np.zeros(nm), np.zeros(nm)
    flags = np.zeros(2, np.int32)
    rc = h.hmr_factors(S["nx"], S["ny"], S["nmaps"], S["nblocks"], S["m"], S["ndata"], rw.size, L.ptr(rw), L.ptr(row), L.ptr(col), damp, k, L.ptr(L1), L.ptr(d1),
                       L.ptr(L2), L.ptr(d2), L.ptr(flags))
    assert rc == 0
    return flags, L1, d1, L2, d2


def differences(a, b):
    """The largest differences between two sets of figures of one system (dicts as the twin's, R a list per map), each on its scale: R,
    R_qq, the R of the co-located unknowns, the leverages and the traces relative to the largest |R| of b (all are sums of products of that
    size); var and the covariance relative to the largest var; the four sums of R^2, which carry other units, relative to their own largest
    value.  Returns {name: relative difference}."""
    rmax = max(np.abs(R).max() for R in b["R"])
    ma, mb = a["measures"], b["measures"]
    vmax = np.abs(mb[1]).max()
    d = dict(R=max(np.abs(x - y).max() for x, y in zip(a["R"], b["R"])) / rmax, rqq=np.abs(ma[0] - mb[0]).max() / rmax,
             leak=np.abs(ma[6:8] - mb[6:8]).max() / rmax, leverage=np.abs(a["leverage"] - b["leverage"]).max() / rmax,
             trace=np.abs(a["trace"] - b["trace"]).max() / rmax, var=np.abs(ma[1] - mb[1]).max() / vmax, cov=np.abs(ma[8] - mb[8]).max() / vmax)
    for q, name in ((2, "own"), (3, "mx"), (4, "my"), (5, "all")):
        d[name] = np.abs(ma[q] - mb[q]).max() / np.abs(mb[q]).max()
    return d


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
