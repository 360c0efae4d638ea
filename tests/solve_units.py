"""Units (grid, medium, source) whose fixed point is the oracle's Fast Marching field in every bit, whatever the schedule -- the inputs of
tests/test_gpu_solve_shapes.py, chosen on the CPU and checked on the CPU (tests/test_solve_units.py).

A field with exact ties has two self-consistent states, so bit-equality with the oracle and across schedules is only asked
of units without them.  `tie_free` is the property: the emulated device schedule (tests/hostcheck.cpp) at windows of 0.5, 1.25 and 6 cells, and
the whole unit through the worklist solve, give the oracle's coarse field, refined snapshot and status classes bit for bit, and no
evaluation of any of these solves ends on an exact tie with an influence (what the device's census counts).  The list itself is data:
tests/golden/solve_units.json, written once by `python tests/solve_units.py` from the candidates below.

Test infrastructure only: nothing under dsurftomo_amd/ imports this module.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np

import _libs as L
import synth

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libhostcheck.so")
LIST = os.path.join(HERE, "golden", "solve_units.json")

# name -> (nx, ny, dicing): propagation grids of 121^2, 161^2, 257^2 nodes and the rectangle 121 x 257 (nbx != nbz)
GRIDS = {"121": (18, 18, 8), "161": (35, 35, 5), "257": (35, 35, 8), "121x257": (18, 35, 8)}
MEDIA = ("smooth", "rough", "wild", "homog")
WINDOWS = (0.5, 1.25, 6.0)
NCAND = 64          # candidates per (grid, medium): 62 drawn by synth.sources, two within three cells of a grid edge
PER_GRID = 12       # units listed per grid, shared evenly among the media that are not dropped there


def medium(nx, ny, kind):
    """synth.medium, and its formulas on nx x ny vertices for the rectangle: (ny*nx,) float64, latitude index fastest"""
    if nx == ny:
        return synth.medium(nx, kind)
    i = np.arange(nx, dtype=np.float64)[None, :]
    j = np.arange(ny, dtype=np.float64)[:, None]
    if kind == "homog":
        v = np.full((ny, nx), 3.0)
    elif kind == "smooth":
        v = 2.8 * (1.0 + 0.10 * np.sin(4 * np.pi * i / nx) * np.cos(4 * np.pi * j / ny))
    elif kind in ("rough", "wild"):
        r = synth.LCG(synth.SEED + (7 if kind == "rough" else 13)).uniform(nx * ny).reshape(ny, nx)
        v = 3.0 * (1.0 + (0.10 if kind == "rough" else 0.45) * (2 * r - 1))
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(v.reshape(-1), np.float64)


def grid_of(name):
    nx, ny, gd = GRIDS[name]
    return L.grid(nx, ny, synth.GOXD, synth.GOZD, synth.DVD, synth.DVD, gd)


def position(g, fx, fz):
    """a source given as fractions of the grid -> (x, z) fp32 radians"""
    f = np.float32
    return (f(g.gox + f(fx * (g.nnx - 1)) * g.dnx), f(g.goz + f(fz * (g.nnz - 1)) * g.dnz))


def candidates(name):
    """NCAND sources as fractions of the grid (5 decimals): synth.sources' draws, then two within three cells of an edge"""
    nx, ny, gd = GRIDS[name]
    g = grid_of(name)
    sx, _ = synth.sources(nx, NCAND - 2, gd)
    _, sz = synth.sources(ny, NCAND - 2, gd)
    fx = (sx.astype(np.float64) - g.gox) / g.dnx / (g.nnx - 1)
    fz = (sz.astype(np.float64) - g.goz) / g.dnz / (g.nnz - 1)
    out = [(round(float(a), 5), round(float(b), 5)) for a, b in zip(fx, fz)]
    out.append((round(1.4 / (g.nnx - 1), 5), 0.52))                       # 1.4 cells from the low-x edge
    out.append((0.37, round((g.nnz - 1 - 2.3) / (g.nnz - 1), 5)))         # 2.3 cells from the high-z edge
    return out


def hostcheck():
    src = os.path.join(HERE, "hostcheck.cpp")
    hdr = [os.path.join(L.ROOT, "dsurftomo_amd", "csrc", n) for n in ("eikonal_core.h", "source_stage.h", "host_geometry.h", "exact_march.h",
                                                                     "dispersion_core.h", "ray_core.h")]
    hdr.append(os.path.join(HERE, "solve_node_walk_ref.h"))
    if L._stale(SO, [src] + hdr):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-msse2",
                               "-mfpmath=sse", "-shared", "-o", SO, src, "-lm"])
    h = C.CDLL(SO)
    h.hc_solve_source.argtypes = [L.i32, L.i32, L.f32, L.f32, L.f32, L.f32, L.i32, L.vp, L.f32, L.f32] + [L.vp] * 7
    h.hc_coarse_problem.argtypes = [L.i32, L.i32, L.f32, L.f32, L.f32, L.f32, L.i32, L.vp, L.f32, L.f32] + [L.vp] * 5
    h.hc_device_schedule.argtypes = [L.i32, L.i32, L.vp, L.vp, L.vp, L.vp, L.f32, L.f32, L.f32, L.f32, L.i32, L.i32, L.vp, L.vp, L.i32]
    h.hc_device_schedule.restype = C.c_long
    h.hc_tie_study.argtypes = [L.i32, L.i32, L.vp, L.vp, L.vp, L.vp, L.f32, L.f32, L.f32, L.f32, L.f32, L.vp]
    h.hc_unit_ties.restype = C.POINTER(C.c_long)
    return h


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Case:
    """one (grid, medium): the oracle's grid, velocity field and solves"""

    def __init__(self, name, kind):
        self.name, self.kind = name, kind
        self.nx, self.ny, self.gd = GRIDS[name]
        self.g = grid_of(name)
        self.pv = medium(self.nx, self.ny, kind)
        self.veln = L.o_gridder(self.g, self.pv)

    def solve(self, fx, fz):
        sx, sz = position(self.g, fx, fz)
        return sx, sz, L.o_solve(self.g, self.pv, self.veln, sx, sz)


def tie_free(H, case, fx, fz):
    """(the property holds, why not) for one source of a Case"""
    g, pv = case.g, case.pv
    nx, ny, gd = case.nx, case.ny, case.gd
    NX, NZ = g.nnx, g.nnz
    sx, sz, o = case.solve(fx, fz)
    geo = (nx, ny, synth.GOXD, synth.GOZD, synth.DVD, synth.DVD, gd, L.ptr(pv), sx, sz)
    # the whole unit through the worklist solve: refined snapshot, status classes, coarse field; ties of both stages
    T = np.zeros((NX, NZ), np.float32); Tr = np.zeros(129 * 129, np.float32); Sr = np.zeros(129 * 129, np.int32)
    it = np.zeros((NX, NZ), np.float32); is_ = np.zeros((NX, NZ), np.int32); box = np.zeros(6, np.int32); st = np.zeros(4, np.int64)
    ties = H.hc_unit_ties()
    ties[0] = ties[1] = 0
    if H.hc_solve_source(*geo, L.ptr(T), L.ptr(Tr), L.ptr(Sr), L.ptr(it), L.ptr(is_), L.ptr(box), L.ptr(st)) != 0:
        return False, "outside"
    if st[1] != 0:
        return False, "serial march guard"
    if ties[0] != 0:
        return False, "%d evaluations of the worklist solve end on a tie" % ties[0]
    if ties[1] != 0:
        return False, "%d outputs of the hand-off depend on a node that ties in rank with the one that ends the refined stage" % ties[1]
    n = box[4] * box[5]
    if (box[4], box[5]) != o["Sr"].shape:
        return False, "refined box"
    Trh = Tr[:n].reshape(box[4], box[5]); Srh = Sr[:n].reshape(box[4], box[5])
    if (np.sign(o["Sr"]).clip(-1, 1) != np.sign(Srh).clip(-1, 1)).any():
        return False, "refined status classes"
    known = o["Sr"] >= 0
    if (bits(Trh[known]) != bits(o["Tr"][known])).any():
        return False, "refined times"
    if (bits(T) != bits(o["T"])).any():
        return False, "coarse field (worklist)"
    # the device schedule at three windows: the same bits, no tie met on the way
    for wc in WINDOWS:
        for study in (False, True):
            T = np.zeros((NX, NZ), np.float32); tau = np.zeros((NX, NZ), np.float32); slow = np.zeros((NX, NZ), np.float32)
            ris = np.zeros(NX, np.float32); geom = np.zeros(4, np.float32)
            if H.hc_coarse_problem(*geo, L.ptr(T), L.ptr(tau), L.ptr(slow), L.ptr(ris), L.ptr(geom)) != 0:
                return False, "outside"
            w = np.float32(wc * geom[3])
            if study:
                out = np.zeros(4)
                if H.hc_tie_study(NX, NZ, L.ptr(T), L.ptr(tau), L.ptr(slow), L.ptr(ris), geom[0], geom[1], geom[2], w, 0.0, L.ptr(out)) != 0:
                    return False, "no convergence"
                if out[2] != 0:
                    return False, "%d evaluations of the device schedule end on a tie (window %g)" % (out[2], wc)
            else:
                out = np.zeros(4, np.int64); cyc = np.zeros(4, np.int32)
                if H.hc_device_schedule(NX, NZ, L.ptr(T), L.ptr(tau), L.ptr(slow), L.ptr(ris), geom[0], geom[1], geom[2], w, 1, 20000,
                                        L.ptr(out), L.ptr(cyc), 4) != 0:
                    return False, "no convergence"
                if out[3] != 0:
                    return False, "a cycle was frozen"
                if (bits(np.abs(T)) != bits(o["T"])).any():
                    return False, "coarse field (device schedule, window %g)" % wc
    return True, ""


def load():
    """the committed list: {grid name: [(medium, fx, fz), ...]}"""
    with open(LIST) as f:
        d = json.load(f)
    return {name: [(k, float(a), float(b)) for k, a, b in rows] for name, rows in d["units"].items()}


def select(log=print):
    """the choice (a minute of CPU per grid).  Per grid and medium: the candidates that hold the property; a medium with fewer than four of
    them among its NCAND is dropped on that grid; of each medium left, the edge candidates that hold and then the first of synth.sources'
    draws, PER_GRID // (media left) in all.  Returns (units as load() gives them, candidates that hold per grid / medium)."""
    H = hostcheck()
    units, held = {}, {}
    for name in GRIDS:
        cand = candidates(name)
        per = {}
        for kind in MEDIA:
            case = Case(name, kind)
            per[kind] = []
            for c in cand[-2:] + cand[:-2]:
                good, why = tie_free(H, case, *c)
                if good:
                    per[kind].append(c)
                else:
                    log("%s %s (%g, %g): %s" % (name, kind, c[0], c[1], why))
            held["%s/%s" % (name, kind)] = len(per[kind])
        kinds = [k for k in MEDIA if len(per[k]) >= 4]
        units[name] = [(k, fx, fz) for k in kinds for fx, fz in per[k][:PER_GRID // len(kinds)]]
    return units, held


if __name__ == "__main__":
    import sys
    units, held = select(log=lambda s: sys.stderr.write(s + "\n"))
    with open(LIST, "w") as f:
        f.write('{"candidates_that_hold_of_%d": %s,\n "units": {\n' % (NCAND, json.dumps(held)))
        f.write(",\n".join('  "%s": [%s]' % (n, ", ".join(json.dumps(list(u)) for u in rows)) for n, rows in units.items()))
        f.write("\n }\n}\n")
