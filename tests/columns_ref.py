"""Test infrastructure for the depth step of the columns: the CPU build of dsurftomo_amd/csrc/column_system.h
(tests/hostcheck_columns.cpp) behind NumPy, the small cases of tests/test_gpu_columns.py, and the Gauss-Newton loop of its test (c) written
over any source of curves and depth kernels -- the device's fetched ones there, the oracle's in tests/test_depth_patterns.py.  Nothing under
dsurftomo_amd/ imports this module."""
import ctypes as C
import os
import subprocess

import numpy as np

import _libs as L

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libhostcheck_columns.so")
SRC = os.path.join(HERE, "hostcheck_columns.cpp")
HDR = [os.path.join(L.ROOT, "dsurftomo_amd", "csrc", n) for n in ("column_system.h", "ray_core.h", "source_stage.h")]
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-msse2", "-mfpmath=sse"]
F = np.float32
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if L._stale(SO, [SRC] + HDR):
        subprocess.check_call(["g++"] + FLAGS + ["-shared", "-o", SO, SRC, "-lm"])
    lib = C.CDLL(SO)
    lib.hcc_ltl.argtypes = [L.i32] * 3
    lib.hcc_tri_row.argtypes = [L.i32]
    lib.hcc_combine.argtypes = [C.c_longlong, L.vp, L.i32, L.vp, L.vp, L.vp, L.vp]
    lib.hcc_combine.restype = None
    lib.hcc_step.argtypes = [L.i32] * 3 + [L.vp] * 5 + [L.f32] * 5 + [L.vp] * 6
    lib.hcc_step.restype = None
    lib.hcc_finish.argtypes = [L.i32, L.vp, L.vp] + [L.f32] * 3 + [L.vp] * 3
    _lib = lib
    return lib


def host_step(h, obs, wt, pv, S, vels, smooth, damp, dvmax, minvel, maxvel, only=None):
    """hcc_step on columns side by side: obs / wt (K, n) fp32, pv (K, n), S (M, K, n), vels (>= M, n) fp32.  Returns dict(vels (the stepped
    copy), dv, nused, chi2, flag, delta)."""
    M, K, n = S.shape
    obs = np.ascontiguousarray(obs, F); pv = np.ascontiguousarray(pv, np.float64); S = np.ascontiguousarray(S, np.float64)
    wt = None if wt is None else np.ascontiguousarray(wt, F)
    only = None if only is None else np.ascontiguousarray(only, np.uint8)
    assert obs.shape == (K, n) and pv.shape == (K, n) and vels.shape[0] >= M and vels.shape[1] == n
    assert (wt is None or wt.shape == (K, n)) and (only is None or only.shape == (n,))
    v = np.array(vels, F, copy=True, order="C")
    out = dict(vels=v, dv=np.zeros((M, n), F), nused=np.zeros(n, np.int32), chi2=np.zeros(n), flag=np.zeros(n, np.int32), delta=np.zeros((M, n)))
    h.hcc_step(M, K, n, L.ptr(only), L.ptr(obs), L.ptr(wt), L.ptr(pv), L.ptr(S), smooth, damp, dvmax, minvel, maxvel, L.ptr(v), L.ptr(out["dv"]),
               L.ptr(out["nused"]), L.ptr(out["chi2"]), L.ptr(out["flag"]), L.ptr(out["delta"]))
    return out


def host_combine(h, vels, depz, svs, svp, srho):
    """k_sen_combine on the host: vels (nz, ncol) fp32, the three kernels (nz, K, ncol) as dispersion_fetch returns them.  Returns S
    (nz - 1, K, ncol); the engine's rule for the coefficient set: depz[nz - 2] < 35 km"""
    nz, K, ncol = svs.shape
    M = nz - 1
    v = np.ascontiguousarray(np.broadcast_to(np.asarray(vels, F).reshape(nz, 1, ncol)[:M], (M, K, ncol)))
    a = [np.ascontiguousarray(x[:M], np.float64) for x in (svs, svp, srho)]
    S = np.zeros((M, K, ncol))
    h.hcc_combine(S.size, L.ptr(v), 1 if F(depz[nz - 2]) < F(35.0) else 0, L.ptr(a[0]), L.ptr(a[1]), L.ptr(a[2]), L.ptr(S))
    return S


def interior(nx, ny):
    """one flag per column of an (ny, nx) grid: 1 inside the outer ring"""
    m = np.zeros((ny, nx), np.uint8)
    m[1:-1, 1:-1] = 1
    return m.ravel()


# ---- the cases of the GPU test, shared with the CPU loop --------------------------------------------------------------------------------

NX = NY = 5
WAVES = [(2, 0, np.array([4.0, 9.0, 20.0])), (2, 1, np.array([5.0, 11.0, 24.0])), (1, 0, np.array([4.0, 9.0, 20.0])), (1, 1, np.array([5.0, 11.0, 24.0]))]
K = sum(len(t) for _, _, t in WAVES)
MINTHK = 2.0
SMOOTH, DAMP, DVMAX, MINVEL, MAXVEL = 0.2, 0.05, 0.3, 0.5, 6.0
ITERATIONS = 4


def depths(nz):
    """test_gpu_dispersion.py's: nz depth nodes with spacings growing from 2 to ~6 km"""
    return np.concatenate([[0.0], np.cumsum(np.round(2.0 + 4.0 * np.arange(nz - 1) / max(nz - 2, 1)))]).astype(F)


def smooth_model(nx, ny, nz):
    """test_gpu_dispersion.py's smooth_model, (nz, ny, nx)"""
    i = np.arange(nx)[None, None, :]; j = np.arange(ny)[None, :, None]; k = np.arange(nz)[:, None, None]
    v = (2.6 + 1.9 * k / max(nz - 1, 1)) * (1.0 + 0.05 * np.sin(0.7 * i + 0.3 * k) * np.cos(0.5 * j))
    return np.ascontiguousarray(v, F)


def edge_model(nx, ny, nz):
    """test_gpu_dispersion.py's edge_model, (nz, ny, nx): columns cycling through six kinds, among them no contrast at all (no Love root at
    long periods) and a half space slower than the layers above (no Rayleigh root at long periods)"""
    base = np.linspace(2.4, 4.6, nz)
    cols = []
    for c in range(nx * ny):
        v = base.copy()
        kind = c % 6
        if kind == 1:
            v[nz // 4:nz // 2 + 1] = 2.0
        elif kind == 2:
            v[:] = 3.5
        elif kind == 3:
            v[-1] = 2.0
        elif kind == 4:
            v[0] = 1.0
        elif kind == 5:
            v[:max(nz // 4, 1)] = 5.0
        cols.append(v * (1.0 + 0.003 * (c // 6)))
    return np.ascontiguousarray(np.array(cols).T.reshape(nz, ny, nx), F)


def perturbed(truth):
    """the truth with a smooth 3 % perturbation that changes sign over depth and across the grid"""
    nz, ny, nx = truth.shape
    i = np.arange(nx)[None, None, :]; j = np.arange(ny)[None, :, None]; k = np.arange(nz)[:, None, None]
    return np.ascontiguousarray(truth * (1.0 + 0.03 * np.cos(0.9 * i + 0.5 * j) * np.cos(1.1 * k / max(nz - 1, 1) * np.pi * 0.5 + 0.3)), F)


def oracle_curves(vel, depz):
    """pv (K, ncol) and the three kernels (nz, K, ncol) of all of WAVES from the oracle's depthkernel, in slot order"""
    parts = [L.depthkernel("oracle", vel, depz, MINTHK, wave, kind, t) for wave, kind, t in WAVES]
    return tuple(np.concatenate([p[q] for p in parts], axis=0 if q == 0 else 1) for q in range(4))


def loop(h, start, depz, obs, curves, iterations=ITERATIONS, wt=None, after=None):
    """The Gauss-Newton loop on the host: per iteration curves(model) -> (pv, svs, svp, srho), host_combine, host_step on the interior
    columns.  after(iteration, model before, inputs, host result): a hook (the GPU test compares the device's step there and may return the
    model to go on with).  Returns (model, [sum of chi2 before each step], [rms before each step])."""
    nz, ny, nx = start.shape
    model = np.array(start, F, copy=True)
    chi2, rms = [], []
    for it in range(iterations):
        pv, svs, svp, srho = curves(model)
        S = host_combine(h, model.reshape(nz, ny * nx), depz, svs, svp, srho)
        out = host_step(h, obs, wt, pv, S, model.reshape(nz, ny * nx), SMOOTH, DAMP, DVMAX, MINVEL, MAXVEL, interior(nx, ny))
        chi2.append(float(out["chi2"].sum()))
        rms.append(float(np.sqrt(out["chi2"].sum() / max(int(out["nused"].sum()), 1))))
        if after is not None:
            after(it, model, (pv, S), out)
        model = out["vels"].reshape(nz, ny, nx)
    return model, chi2, rms
