"""Test infrastructure for the laterally coupled radial depth step: the CPU build of
dsurftomo_amd/csrc/column_radial_lateral.h (tests/hostcheck_column_radial_lateral.cpp) behind NumPy, the errors of xi the loop tests compare,
and the Gauss-Newton loop written over any source of curves and depth kernels -- the device's fetched ones in
tests/test_gpu_column_radial_lateral.py, the oracle's in tests/test_hostcheck_column_radial_lateral.py.  Nothing under dsurftomo_amd/ imports
this module."""
import ctypes as C
import os
import subprocess

import numpy as np

import _libs as L
import column_radial_ref as RR
import columns_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libhostcheck_column_radial_lateral.so")
SRC = os.path.join(HERE, "hostcheck_column_radial_lateral.cpp")
HDR = [os.path.join(L.ROOT, "dsurftomo_amd", "csrc", n) for n in ("column_radial_lateral.h", "column_lateral.h", "column_radial.h", "column_system.h")]
F = np.float32
TOL, MAXIT = 1e-8, 500
# the loop tests' setting (chosen on the oracle's curves, tests/test_hostcheck_column_radial_lateral.py: test_loop_on_the_oracles_dispersion)
LATERAL, LATERAL_ANISO, NOISE, NOISE_SEED = 0.3, 0.6, 0.005, 24
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if L._stale(SO, [SRC] + HDR):
        subprocess.check_call(["g++"] + R.FLAGS + ["-shared", "-o", SO, SRC, "-lm"])
    lib = C.CDLL(SO)
    lib.hrlat_ws_doubles.argtypes = [L.i32] * 3
    lib.hrlat_ws_doubles.restype = C.c_longlong
    lib.hrlat_step.argtypes = [L.i32] * 4 + [C.c_ulonglong] + [L.vp] * 5 + [L.f32] * 8 + [C.c_double, L.i32, L.i32] + [L.vp] * 8
    lib.hrlat_step.restype = L.i32
    _lib = lib
    return lib


same_bits = RR.same_bits


def host_step(h, nx, ny, love, obs, wt, pv, Sv, Sh, vsv, vsh, smooth, damp, aniso, lateral, lateral_aniso, dvmax, minvel, maxvel, tol=TOL, maxit=MAXIT, poll=16):
    """hrlat_step on an (ny, nx) grid of columns: obs / wt (K, ny * nx) fp32, pv (K, ny * nx), Sv / Sh (M, K, ny * nx), vsv / vsh (>= M, ny * nx)
    fp32.  Returns dict(vsv, vsh (the stepped copies), dv (2, M, n), dv_sv, dv_sh (its halves), nused (2, n), chi2 (2, n), flag (n), delta
    (2M, n), itn, istop, rz0, rz, started (iterations the loop started))."""
    M, K, n = Sv.shape
    obs = np.ascontiguousarray(obs, F); pv = np.ascontiguousarray(pv, np.float64)
    Sv = np.ascontiguousarray(Sv, np.float64); Sh = np.ascontiguousarray(Sh, np.float64)
    wt = None if wt is None else np.ascontiguousarray(wt, F)
    assert n == nx * ny and nx >= 3 and ny >= 3 and obs.shape == (K, n) and pv.shape == (K, n) and Sh.shape == Sv.shape and len(love) == K
    assert vsv.shape == vsh.shape and vsv.shape[0] >= M and vsv.shape[1] == n and (wt is None or wt.shape == (K, n))
    v = np.array(vsv, F, copy=True, order="C"); w = np.array(vsh, F, copy=True, order="C")
    info = np.zeros(4)
    out = dict(vsv=v, vsh=w, dv=np.zeros((2, M, n), F), nused=np.zeros((2, n), np.int32), chi2=np.zeros((2, n)), flag=np.zeros(n, np.int32), delta=np.zeros((2 * M, n)))
    out["started"] = h.hrlat_step(nx, ny, M, K, RR.mask(love), L.ptr(obs), L.ptr(wt), L.ptr(pv), L.ptr(Sv), L.ptr(Sh), smooth, damp, aniso, lateral, lateral_aniso,
                                  dvmax, minvel, maxvel, tol, maxit, poll, L.ptr(v), L.ptr(w), L.ptr(out["dv"]), L.ptr(out["nused"]), L.ptr(out["chi2"]),
                                  L.ptr(out["flag"]), L.ptr(info), L.ptr(out["delta"]))
    out.update(itn=int(info[0]), istop=int(info[1]), rz0=float(info[2]), rz=float(info[3]), dv_sv=out["dv"][0], dv_sh=out["dv"][1])
    return out


def xi_of(vsv, vsh):
    """(Vsh / Vsv)^2, fp64"""
    r = np.asarray(vsh, np.float64) / np.asarray(vsv, np.float64)
    return r * r


def xi_rms(vsv, vsh, truth_v, truth_h, nx, ny):
    """the rms difference of xi from the truth's over the interior nodes above the bottom depth, fp64"""
    nz = truth_v.shape[0]
    inner = R.interior(nx, ny) == 1
    pick = lambda m: np.asarray(m, np.float64).reshape(nz, -1)[:nz - 1, inner]
    d = xi_of(pick(vsv), pick(vsh)) - xi_of(pick(truth_v), pick(truth_h))
    return float(np.sqrt((d * d).mean()))


def xi_column_rms(vsv, vsh, truth_v, truth_h, column):
    """the same over one column's nodes above the bottom depth; vsv = vsh = None: the error of xi = 1"""
    nz = truth_v.shape[0]
    pick = lambda m: np.asarray(m, np.float64).reshape(nz, -1)[:nz - 1, column]
    got = np.ones(nz - 1) if vsv is None else xi_of(pick(vsv), pick(vsh))
    d = got - xi_of(pick(truth_v), pick(truth_h))
    return float(np.sqrt((d * d).mean()))


def noisy(obs, level=NOISE, seed=NOISE_SEED):
    """obs (fp64 or fp32 curves) times (1 + level * standard normal) of a fixed seed, fp32"""
    return (np.asarray(obs, np.float64) * (1.0 + level * np.random.default_rng(seed).standard_normal(obs.shape))).astype(F)


def loop(step, start_v, start_h, depz, curves, hs, iterations=R.ITERATIONS, after=None):
    """column_radial_ref.loop over a step of one's own: per iteration curves(vsv, vsh) -> (pv, svs, svp, srho) in slot order, host_combine on
    both models, step(vsv (nz, ncol), vsh (nz, ncol), pv, Sv, Sh) -> a result with "vsv" and "vsh".  after(iteration, (vsv, vsh) before, (pv,
    Sv, Sh), result): a hook.  Returns (vsv, vsh, [the results])."""
    nz, ny, nx = start_v.shape
    n = ny * nx
    vsv = np.array(start_v, F, copy=True); vsh = np.array(start_h, F, copy=True)
    results = []
    for it in range(iterations):
        pv, svs, svp, srho = curves(vsv, vsh)
        Sv = R.host_combine(hs, vsv.reshape(nz, n), depz, svs, svp, srho)
        Sh = R.host_combine(hs, vsh.reshape(nz, n), depz, svs, svp, srho)
        out = step(vsv.reshape(nz, n), vsh.reshape(nz, n), pv, Sv, Sh)
        if after is not None:
            after(it, (vsv, vsh), (pv, Sv, Sh), out)
        results.append(out)
        vsv, vsh = out["vsv"].reshape(nz, ny, nx), out["vsh"].reshape(nz, ny, nx)
    return vsv, vsh, results
