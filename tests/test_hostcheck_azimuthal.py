"""The azimuthal back-trace (ray_core.h: trace_ray<., true>) on the CPU, through tests/hostcheck_azimuthal.cpp, on
the oracle's fields: the isotropic slab stays the oracle's bit for bit, one and four lanes agree, and the 2psi weights are checked against
a geometry that never looks at a gradient -- the oracle's own path points."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _libs as L
import synth

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libhostcheck_azimuthal.so")

# Bound of the mean cos 2psi / sin 2psi of a ray against the path-point model: four times the worst deviation measured over this file's 96
# rays (worst 3.82e-3).  The path points are fp32 radians -- an ulp is 1.2e-7 rad against steps of 1.1e-5 to 1.7e-5 rad, a
# per-step direction noise of up to 1e-2 that averages out over a ray's steps.  A swapped component or sign is an error of order 1.
DELTA = 1.53e-2
assert DELTA <= 0.02

CASES = [(18, "smooth", 8), (18, "rough", 5), (35, "homog", 8), (35, "checker4", 8)]


def load():
    src = os.path.join(HERE, "hostcheck_azimuthal.cpp")
    hdr = [os.path.join(L.ROOT, "dsurftomo_amd", "csrc", n) for n in ("eikonal_core.h", "source_stage.h", "host_geometry.h", "ray_core.h")]
    if L._stale(SO, [src] + hdr):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-msse2",
                               "-mfpmath=sse", "-shared", "-o", SO, src, "-lm"])
    h = C.CDLL(SO)
    h.hca_trace_ray.argtypes = [L.i32, L.i32, L.f32, L.f32, L.f32, L.f32, L.i32, L.vp, L.vp, L.vp, L.vp, L.f32, L.f32, L.f32, L.f32,
                                L.vp, L.vp, L.vp, L.vp, L.i32]
    return h


def twin(h, nx, gd, g, veln, sol, sx, sz, rx, rz, lanes):
    """(fdm3 (3, nvx+2, nvz+2) [iso | c | s] in the oracle's layout, clamp flag, steps, sums (2,))"""
    fdm3 = np.zeros((3, g.nvx + 2, g.nvz + 2), np.float32)
    fl, st = L.i32(0), L.i32(0)
    sums = np.zeros(2, np.float32)
    rc = h.hca_trace_ray(nx, nx, synth.GOXD, synth.GOZD, synth.DVD, synth.DVD, gd, L.ptr(veln), L.ptr(sol["T"]),
                         L.ptr(np.ascontiguousarray(sol["Tr"])), L.ptr(np.ascontiguousarray(sol["Sr"])), sx, sz, rx, rz,
                         L.ptr(fdm3), C.byref(fl), C.byref(st), L.ptr(sums), lanes)
    assert rc == 0, rc
    return fdm3, fl.value, st.value, sums


def oracle_path_radians(g, sol, veln, sx, sz, rx, rz, cap=1 << 14):
    """the oracle's ray points (colatitude, longitude) in radians, fp32 as it keeps them: the receiver, the end point of every step, the source"""
    O = L.oracle()
    O.dso_rpaths_path.argtypes = [C.POINTER(L.Grid), C.POINTER(L.Box), L.vp, L.vp, L.vp, L.vp, L.f32, L.f32, L.f32, L.f32, L.vp,
                                  C.POINTER(L.i32), C.POINTER(L.i32), L.vp, L.i32, C.POINTER(L.i32)]
    fdm = np.zeros((g.nvx + 2, g.nvz + 2), np.float32)
    rb, ns, n = L.i32(0), L.i32(0), L.i32(0)
    path = np.zeros((cap, 2), np.float32)
    rc = O.dso_rpaths_path(C.byref(g), C.byref(sol["box"]), L.ptr(veln), L.ptr(sol["T"]), L.ptr(np.ascontiguousarray(sol["Tr"])),
                           L.ptr(np.ascontiguousarray(sol["Sr"])), sx, sz, rx, rz, L.ptr(fdm), C.byref(rb), C.byref(ns), L.ptr(path), cap, C.byref(n))
    assert rc == 0 and n.value <= cap
    return path[:n.value].astype(np.float64), rb.value, ns.value, fdm


def model_2psi(g, pts, steps):
    """cos 2psi and sin 2psi of every step from the path points alone: south = dx R, east = dz R sin x_j, north = -south, psi clockwise
    from north; the final (source) point is ignored"""
    x, z = pts[:steps + 1, 0], pts[:steps + 1, 1]
    south = np.diff(x) * float(g.earth)
    east = np.diff(z) * float(g.earth) * np.sin(x[:-1])
    north = -south
    q = north * north + east * east
    assert (q > 0).all()
    return (north * north - east * east) / q, 2.0 * north * east / q


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def rays():
    """every ray of this file once: per case 3 sources x 8 receivers, all at least three node cells inside the grid and at least a quarter
    of the grid apart.  Entries: dict(case, ref (oracle fdm), rb, ns, pts, one (twin with 1 lane), four (with 4 lanes))"""
    h = load()
    out = []
    for nx, kind, gd in CASES:
        g = L.grid(nx, nx, synth.GOXD, synth.GOZD, synth.DVD, synth.DVD, gd)
        pv = synth.medium(nx, kind)
        veln = L.o_gridder(g, pv)
        N = g.nnx
        r = synth.LCG(23 + nx + gd)
        for fx, fz in [(0.43 * N + 0.3, 0.61 * N + 0.6), (4.4, N / 2 + 0.2), (N - 5.5, N - 6.3)]:
            sx = np.float32(g.gox + np.float32(fx) * g.dnx)
            sz = np.float32(g.goz + np.float32(fz) * g.dnz)
            sol = L.o_solve(g, pv, veln, sx, sz)
            k = 0
            while k < 8:
                u = r.uniform(2)
                px, pz = 3.3 + u[0] * (N - 7.6), 3.3 + u[1] * (N - 7.6)
                if np.hypot(px - fx, pz - fz) < 0.25 * N:
                    continue
                k += 1
                rx = np.float32(g.gox + np.float32(px) * g.dnx)
                rz = np.float32(g.goz + np.float32(pz) * g.dnz)
                pts, rb, ns, ref = oracle_path_radians(g, sol, veln, sx, sz, rx, rz)
                out.append(dict(case=(nx, kind, gd), g=g, ref=ref, rb=rb, ns=ns, pts=pts,
                                one=twin(h, nx, gd, g, veln, sol, sx, sz, rx, rz, 1), four=twin(h, nx, gd, g, veln, sol, sx, sz, rx, rz, 4)))
    assert len(out) == 24 * len(CASES)
    return out


def test_no_ray_is_clamped(rays):
    """the oracle's rbint: the geometry checks below hold for unclamped steps (a clamped step keeps its gradient's direction, its end point not)"""
    for q in rays:
        assert q["rb"] & 1 == 0 and q["one"][1] == 0 and q["four"][1] == 0, q["case"]
        assert len(q["pts"]) == q["ns"] + 2, "receiver, one point per step, the source"


def test_isotropic_slab_flag_and_steps_are_the_oracles(rays):
    """with the accumulation on, the isotropic slab, the clamp flag and the steps equal o_rpaths' bit for bit"""
    for q in rays:
        fdm3, fl, st, _ = q["one"]
        assert (bits(fdm3[0]) != bits(q["ref"])).sum() == 0, q["case"]
        assert fl == (q["rb"] & 1) and st == q["ns"], q["case"]
        assert q["ns"] > 20


def test_one_and_four_lanes_agree(rays):
    """the three slabs and the sums, bit for bit"""
    for q in rays:
        a, b = q["one"], q["four"]
        assert (bits(a[0]) != bits(b[0])).sum() == 0, q["case"]
        assert a[1:3] == b[1:3] and (bits(a[3]) == bits(b[3])).all(), q["case"]
        assert np.abs(a[0][1]).max() > 0 and np.abs(a[0][2]).max() > 0


def test_ray_means_against_the_path_points(rays):
    """sum c2 / steps and sum s2 / steps against the model from the oracle's path points"""
    worst = 0.0
    for q in rays:
        c2, s2 = model_2psi(q["g"], q["pts"], q["ns"])
        sums, n = q["one"][3].astype(np.float64), q["ns"]
        d = max(abs(sums[0] / n - c2.mean()), abs(sums[1] / n - s2.mean()))
        worst = max(worst, d)
    print("worst deviation of a ray's mean cos 2psi / sin 2psi from the path-point model: %.3g (bound %.3g)" % (worst, DELTA))
    assert worst <= DELTA


def test_vertex_ratios_lie_in_the_rays_range(rays):
    """per vertex with |fdm| >= 1e-4: fdm_c / fdm within the ray's [min c2 - delta, max c2 + delta], fdm_s / fdm likewise, and
    fdm_c^2 + fdm_s^2 <= fdm^2 (1 + 1e-5).  The homogeneous medium is the sharp case: its rays turn little (the last steps before the
    source apart, where the gradient of the refined field wobbles), the intervals are narrow, and where the two do not meet the check pairs c
    with the c slab and s with the s slab"""
    sharp = 0
    for q in rays:
        c2, s2 = model_2psi(q["g"], q["pts"], q["ns"])
        f, fc, fs = (q["one"][0][b].astype(np.float64) for b in range(3))
        m = np.abs(f) >= 1e-4
        assert m.sum() > 0
        rc, rs = fc[m] / f[m], fs[m] / f[m]
        assert rc.min() >= c2.min() - DELTA and rc.max() <= c2.max() + DELTA, (q["case"], rc.min(), rc.max(), c2.min(), c2.max())
        assert rs.min() >= s2.min() - DELTA and rs.max() <= s2.max() + DELTA, (q["case"], rs.min(), rs.max(), s2.min(), s2.max())
        assert (fc * fc + fs * fs <= f * f * (1.0 + 1e-5)).all(), q["case"]
        # a ray whose two intervals do not meet tells the slabs apart: swapped, every ratio would fall outside
        if q["case"][1] == "homog" and (c2.min() - DELTA > s2.max() + DELTA or s2.min() - DELTA > c2.max() + DELTA):
            sharp += 1
    print("homogeneous rays whose cos 2psi and sin 2psi intervals are disjoint: %d of 24" % sharp)
    assert sharp >= 12
