"""Test infrastructure for the radially anisotropic depth step: the CPU build of dsurftomo_amd/csrc/column_radial.h
(tests/hostcheck_column_radial.cpp) behind NumPy, the truth model of the loop tests and the Gauss-Newton loop written over any source of
curves and depth kernels -- the device's fetched ones in tests/test_gpu_column_radial.py, the oracle's in
tests/test_hostcheck_column_radial.py.  Nothing under dsurftomo_amd/ imports this module."""
import ctypes as C
import os
import subprocess

import numpy as np

import _libs as L
import columns_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libhostcheck_column_radial.so")
SRC = os.path.join(HERE, "hostcheck_column_radial.cpp")
HDR = [os.path.join(L.ROOT, "dsurftomo_amd", "csrc", n) for n in ("column_radial.h", "column_system.h")]
F = np.float32
ANISO = 0.2
LOVE = np.concatenate([np.full(len(t), wave == 1) for wave, _, t in R.WAVES])          # per slot of columns_ref.WAVES
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if L._stale(SO, [SRC] + HDR):
        subprocess.check_call(["g++"] + R.FLAGS + ["-shared", "-o", SO, SRC, "-lm"])
    lib = C.CDLL(SO)
    lib.hrad_doubles.argtypes = [L.i32] * 2
    lib.hrad_doubles.restype = C.c_longlong
    lib.hrad_step.argtypes = [L.i32] * 3 + [L.vp, C.c_ulonglong] + [L.vp] * 5 + [L.f32] * 6 + [L.vp] * 7
    lib.hrad_step.restype = None
    lib.hrad_finish.argtypes = [L.i32, L.vp, L.vp] + [L.f32] * 3 + [L.vp] * 4
    _lib = lib
    return lib


def mask(love):
    """the kernel's 64-bit argument: bit k set where slot k is a Love slot"""
    return sum(1 << k for k, on in enumerate(np.asarray(love, bool)) if on)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def host_step(h, love, obs, wt, pv, Sv, Sh, vsv, vsh, smooth, damp, aniso, dvmax, minvel, maxvel, only=None):
    """hrad_step on columns side by side: obs / wt (K, n) fp32, pv (K, n), Sv / Sh (M, K, n), vsv / vsh (>= M, n) fp32.  Returns dict(vsv, vsh
    (the stepped copies), dv (2, M, n), dv_sv, dv_sh (its halves), nused (2, n), chi2 (2, n), flag (n), delta (2M, n))."""
    M, K, n = Sv.shape
    obs = np.ascontiguousarray(obs, F); pv = np.ascontiguousarray(pv, np.float64)
    Sv = np.ascontiguousarray(Sv, np.float64); Sh = np.ascontiguousarray(Sh, np.float64)
    wt = None if wt is None else np.ascontiguousarray(wt, F)
    only = None if only is None else np.ascontiguousarray(only, np.uint8)
    assert obs.shape == (K, n) and pv.shape == (K, n) and Sh.shape == Sv.shape and vsv.shape == vsh.shape and vsv.shape[0] >= M and vsv.shape[1] == n
    assert (wt is None or wt.shape == (K, n)) and (only is None or only.shape == (n,)) and len(love) == K
    v = np.array(vsv, F, copy=True, order="C"); w = np.array(vsh, F, copy=True, order="C")
    out = dict(vsv=v, vsh=w, dv=np.zeros((2, M, n), F), nused=np.zeros((2, n), np.int32), chi2=np.zeros((2, n)), flag=np.zeros(n, np.int32), delta=np.zeros((2 * M, n)))
    h.hrad_step(M, K, n, L.ptr(only), mask(love), L.ptr(obs), L.ptr(wt), L.ptr(pv), L.ptr(Sv), L.ptr(Sh), smooth, damp, aniso, dvmax, minvel, maxvel, L.ptr(v), L.ptr(w),
                L.ptr(out["dv"]), L.ptr(out["nused"]), L.ptr(out["chi2"]), L.ptr(out["flag"]), L.ptr(out["delta"]))
    out["dv_sv"], out["dv_sh"] = out["dv"][0], out["dv"][1]
    return out


def host_finish(h, N, b, vsv, vsh, dvmax, minvel, maxvel):
    """hrad_finish on a (2M, 2M) matrix given in full (its lower triangle is used).  Returns (flag, vsv, vsh, dv (2M), pivots)."""
    n2 = len(b)
    tri = np.array([N[i][j] for i in range(n2) for j in range(i + 1)], np.float64)
    v = np.array(vsv, F); w = np.array(vsh, F); dv = np.full(n2, 9.0, F); d = np.zeros(n2)
    flag = h.hrad_finish(n2 // 2, L.ptr(tri), L.ptr(np.array(b, np.float64)), dvmax, minvel, maxvel, L.ptr(v), L.ptr(w), L.ptr(dv), L.ptr(d))
    return flag, v, w, dv, d


def truth_vsh(vsv, amplitude=0.06):
    """the loop tests' truth: Vsh = Vsv (1 + amplitude sin(pi (k + 0.5) / (nz - 1))) above the bottom depth, equal at it"""
    nz = vsv.shape[0]
    k = np.arange(nz - 1)
    out = np.array(vsv, np.float64)
    out[:nz - 1] *= (1.0 + amplitude * np.sin(np.pi * (k + 0.5) / (nz - 1)))[:, None, None]
    return np.ascontiguousarray(out, F)


def oracle_curves_radial(vsv, vsh, depz):
    """columns_ref.oracle_curves with the Love entries of WAVES computed on vsh and the Rayleigh entries on vsv"""
    parts = [L.depthkernel("oracle", vsh if wave == 1 else vsv, depz, R.MINTHK, wave, kind, t) for wave, kind, t in R.WAVES]
    return tuple(np.concatenate([p[q] for p in parts], axis=0 if q == 0 else 1) for q in range(4))


def loop(h, hs, start_v, start_h, depz, obs, curves, iterations=R.ITERATIONS, wt=None, aniso=ANISO, after=None):
    """columns_ref.loop with the radial step: per iteration curves(vsv, vsh) -> (pv, svs, svp, srho) in slot order, host_combine on both
    models, host_step on the interior columns.  after(iteration, (vsv, vsh) before, (pv, Sv, Sh), host result): a hook.  Returns (vsv, vsh,
    [sum of chi2 over both wave types before each step], [(rms Rayleigh, rms Love) before each step])."""
    nz, ny, nx = start_v.shape
    n = ny * nx
    vsv = np.array(start_v, F, copy=True); vsh = np.array(start_h, F, copy=True)
    chi2, rms = [], []
    for it in range(iterations):
        pv, svs, svp, srho = curves(vsv, vsh)
        Sv = R.host_combine(hs, vsv.reshape(nz, n), depz, svs, svp, srho)
        Sh = R.host_combine(hs, vsh.reshape(nz, n), depz, svs, svp, srho)
        out = host_step(h, LOVE, obs, wt, pv, Sv, Sh, vsv.reshape(nz, n), vsh.reshape(nz, n), R.SMOOTH, R.DAMP, aniso, R.DVMAX, R.MINVEL, R.MAXVEL, R.interior(nx, ny))
        chi2.append(float(out["chi2"].sum()))
        rms.append(tuple(float(np.sqrt(out["chi2"][q].sum() / max(int(out["nused"][q].sum()), 1))) for q in range(2)))
        if after is not None:
            after(it, (vsv, vsh), (pv, Sv, Sh), out)
        vsv, vsh = out["vsv"].reshape(nz, ny, nx), out["vsh"].reshape(nz, ny, nx)
    return vsv, vsh, chi2, rms
