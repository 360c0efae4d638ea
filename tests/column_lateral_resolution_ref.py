"""Test infrastructure for the resolution of the laterally coupled depth step: the CPU build of
dsurftomo_amd/csrc/column_lateral_resolution.h (tests/hostcheck_column_lateral_resolution.cpp) behind NumPy, for
tests/test_hostcheck_column_lateral_resolution.py and tests/test_gpu_column_lateral_resolution.py.  Nothing under dsurftomo_amd/ imports
this module."""
import ctypes as C
import os
import subprocess

import numpy as np

import _libs as L
import columns_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libhostcheck_column_lateral_resolution.so")
SRC = os.path.join(HERE, "hostcheck_column_lateral_resolution.cpp")
HDR = [os.path.join(L.ROOT, "dsurftomo_amd", "csrc", n) for n in ("column_lateral_resolution.h", "column_lateral.h", "column_system.h")]
F = np.float32
NAMES = ("val", "m1", "mz", "mx", "my", "own", "var")
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if L._stale(SO, [SRC] + HDR):
        subprocess.check_call(["g++"] + R.FLAGS + ["-shared", "-o", SO, SRC, "-lm"])
    lib = C.CDLL(SO)
    lib.hlres_group_bytes.argtypes = [L.i32] * 3
    lib.hlres_group_bytes.restype = C.c_longlong
    lib.hlres_work_doubles.argtypes = [L.i32]
    lib.hlres_work_doubles.restype = C.c_longlong
    lib.hlres_run.argtypes = [L.i32] * 4 + [L.vp] * 5 + [L.f32] * 3 + [C.c_double] + [L.i32] * 4 + [L.vp] * 8
    lib.hlres_run.restype = L.i32
    lib.hlres_anchor.argtypes = [L.i32] * 4 + [L.vp] * 4 + [L.f32] * 3 + [C.c_double, L.i32] + [L.vp] * 3
    lib.hlres_anchor.restype = None
    lib.hlres_rhs.argtypes = [L.i32] * 4 + [L.vp] * 4 + [L.f32] * 3 + [L.vp] * 2
    lib.hlres_rhs.restype = None
    _lib = lib
    return lib


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def every_unknown(nint, M, kinds=(0, 1)):
    """kind, index of every unknown as each of kinds, the kinds of one unknown side by side"""
    kind = np.tile(np.array(kinds, np.int32), nint * M)
    index = np.repeat(np.arange(nint * M, dtype=np.int32), len(kinds))
    return kind, index


def _inputs(nx, ny, obs, wt, pv, S):
    M, K, n = S.shape
    obs = np.ascontiguousarray(obs, F); pv = np.ascontiguousarray(pv, np.float64); S = np.ascontiguousarray(S, np.float64)
    wt = None if wt is None else np.ascontiguousarray(wt, F)
    assert n == nx * ny and nx >= 3 and ny >= 3 and obs.shape == (K, n) and pv.shape == (K, n) and (wt is None or wt.shape == (K, n))
    return M, K, obs, wt, pv, S


def host_run(h, nx, ny, obs, wt, pv, S, depz, smooth, damp, lateral, kind, index, models=None, tol=1e-8, maxit=500, poll=16, groups=0):
    """hlres_run on an (ny, nx) grid of columns: obs / wt (K, ny * nx) fp32, pv (K, ny * nx), S (M, K, ny * nx), depz (M or more) fp32; models
    None or (rows, M, interior columns).  Returns dict(measures (nmembers, 7), itn, istop (nmembers) int32, rz0, rz (nmembers), full (nmembers,
    M, interior columns), nused, flag (ny * nx), started (the iterations the loops started))."""
    M, K, obs, wt, pv, S = _inputs(nx, ny, obs, wt, pv, S)
    nint = (nx - 2) * (ny - 2)
    kind = np.ascontiguousarray(kind, np.int32); index = np.ascontiguousarray(index, np.int32)
    depz = np.ascontiguousarray(depz, F)
    assert kind.shape == index.shape and kind.ndim == 1 and depz.size >= M
    if models is not None:
        models = np.ascontiguousarray(models, np.float64)
        assert models.ndim == 3 and models.shape[1:] == (M, nint)
    n = kind.size
    info = np.zeros((n, 4))
    out = dict(measures=np.zeros((n, 7)), full=np.zeros((n, M, nint)), nused=np.zeros(nx * ny, np.int32), flag=np.zeros(nx * ny, np.int32))
    out["started"] = h.hlres_run(nx, ny, M, K, L.ptr(obs), L.ptr(wt), L.ptr(pv), L.ptr(S), L.ptr(depz), smooth, damp, lateral, tol, maxit, poll, groups, n, L.ptr(kind),
                                 L.ptr(index), L.ptr(models), L.ptr(out["measures"]), L.ptr(info), L.ptr(out["full"]), L.ptr(out["nused"]), L.ptr(out["flag"]))
    out.update(itn=info[:, 0].astype(np.int32), istop=info[:, 1].astype(np.int32), rz0=info[:, 2].copy(), rz=info[:, 3].copy())
    return out


def host_anchor(h, nx, ny, obs, wt, pv, S, smooth, damp, lateral, f, tol=1e-8, maxit=500):
    """hlres_anchor: section 24's own loop with the right-hand side f (M, interior columns) on a model without lateral differences.  Returns
    dict(x (M, interior columns), itn, istop, rz0, rz)."""
    M, K, obs, wt, pv, S = _inputs(nx, ny, obs, wt, pv, S)
    f = np.ascontiguousarray(f, np.float64)
    assert f.shape == (M, (nx - 2) * (ny - 2))
    x = np.zeros_like(f); info = np.zeros(4)
    h.hlres_anchor(nx, ny, M, K, L.ptr(obs), L.ptr(wt), L.ptr(pv), L.ptr(S), smooth, damp, lateral, tol, maxit, L.ptr(f), L.ptr(x), L.ptr(info))
    return dict(x=x, itn=int(info[0]), istop=int(info[1]), rz0=float(info[2]), rz=float(info[3]))


def host_rhs(h, nx, ny, obs, wt, pv, S, vels, smooth, damp, lateral):
    """hlres_rhs: the right-hand side of the laterally coupled step on the model vels (M or more, ny * nx) fp32: (M, interior columns)"""
    M, K, obs, wt, pv, S = _inputs(nx, ny, obs, wt, pv, S)
    v = np.ascontiguousarray(vels, F)
    assert v.shape[0] >= M and v.shape[1] == nx * ny
    bt = np.zeros((M, (nx - 2) * (ny - 2)))
    h.hlres_rhs(nx, ny, M, K, L.ptr(obs), L.ptr(wt), L.ptr(pv), L.ptr(S), smooth, damp, lateral, L.ptr(v), L.ptr(bt))
    return bt
