"""Test infrastructure for the laterally coupled depth step: the CPU build of dsurftomo_amd/csrc/column_lateral.h
(tests/hostcheck_column_lateral.cpp) behind NumPy, the roughness the coupling penalises, and the Gauss-Newton loop written over any source
of curves and depth kernels -- the device's fetched ones in tests/test_gpu_column_lateral.py, the oracle's in
tests/test_hostcheck_column_lateral.py.  Nothing under dsurftomo_amd/ imports this module."""
import ctypes as C
import os
import subprocess

import numpy as np

import _libs as L
import columns_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libhostcheck_column_lateral.so")
SRC = os.path.join(HERE, "hostcheck_column_lateral.cpp")
HDR = [os.path.join(L.ROOT, "dsurftomo_amd", "csrc", n) for n in ("column_lateral.h", "column_system.h")]
F = np.float32
TOL, MAXIT = 1e-8, 500
# the loop tests' setting (chosen on the oracle's curves, tests/test_hostcheck_column_lateral.py: test_loop_on_the_oracles_dispersion)
LATERAL, NOISE, NOISE_SEED = 0.3, 0.005, 24
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if L._stale(SO, [SRC] + HDR):
        subprocess.check_call(["g++"] + R.FLAGS + ["-shared", "-o", SO, SRC, "-lm"])
    lib = C.CDLL(SO)
    lib.hlat_ws_doubles.argtypes = [L.i32] * 3
    lib.hlat_ws_doubles.restype = C.c_longlong
    lib.hlat_step.argtypes = [L.i32] * 4 + [L.vp] * 4 + [L.f32] * 6 + [C.c_double, L.i32, L.i32] + [L.vp] * 7
    lib.hlat_step.restype = L.i32
    lib.hlat_sum.argtypes = [L.i32, L.vp]
    lib.hlat_sum.restype = C.c_double
    _lib = lib
    return lib


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def host_step(h, nx, ny, obs, wt, pv, S, vels, smooth, damp, lateral, dvmax, minvel, maxvel, tol=TOL, maxit=MAXIT, poll=16):
    """hlat_step on an (ny, nx) grid of columns: obs / wt (K, ny * nx) fp32, pv (K, ny * nx), S (M, K, ny * nx), vels (>= M, ny * nx) fp32.
    Returns dict(vels (the stepped copy), dv, nused, chi2, flag, delta, itn, istop, rz0, rz, started (iterations the loop started))."""
    M, K, n = S.shape
    obs = np.ascontiguousarray(obs, F); pv = np.ascontiguousarray(pv, np.float64); S = np.ascontiguousarray(S, np.float64)
    wt = None if wt is None else np.ascontiguousarray(wt, F)
    assert n == nx * ny and nx >= 3 and ny >= 3 and obs.shape == (K, n) and pv.shape == (K, n) and vels.shape[0] >= M and vels.shape[1] == n
    assert wt is None or wt.shape == (K, n)
    v = np.array(vels, F, copy=True, order="C")
    info = np.zeros(4)
    out = dict(vels=v, dv=np.zeros((M, n), F), nused=np.zeros(n, np.int32), chi2=np.zeros(n), flag=np.zeros(n, np.int32), delta=np.zeros((M, n)))
    out["started"] = h.hlat_step(nx, ny, M, K, L.ptr(obs), L.ptr(wt), L.ptr(pv), L.ptr(S), smooth, damp, lateral, dvmax, minvel, maxvel, tol, maxit, poll, L.ptr(v),
                                 L.ptr(out["dv"]), L.ptr(out["nused"]), L.ptr(out["chi2"]), L.ptr(out["flag"]), L.ptr(info), L.ptr(out["delta"]))
    out.update(itn=int(info[0]), istop=int(info[1]), rz0=float(info[2]), rz=float(info[3]))
    return out


def roughness(vels, nx, ny, M, active=None):
    """the sum over the edges between interior columns (both active, where a mask (ny * nx) is given) of the squared differences of the first
    M rows of vels (>= M, ny * nx), fp64"""
    v = np.asarray(vels, np.float64)[:M].reshape(M, ny, nx)
    on = np.zeros((ny, nx), bool); on[1:-1, 1:-1] = True
    if active is not None:
        on &= np.asarray(active, bool).reshape(ny, nx)
    ex = on[:, 1:] & on[:, :-1]; ey = on[1:, :] & on[:-1, :]
    return float((((v[:, :, 1:] - v[:, :, :-1]) ** 2) * ex).sum() + (((v[:, 1:, :] - v[:, :-1, :]) ** 2) * ey).sum())


def model_rms(model, truth, nx, ny):
    """the rms difference over the interior nodes above the bottom depth, fp64"""
    nz = truth.shape[0]
    inner = R.interior(nx, ny) == 1
    d = np.asarray(model, np.float64).reshape(nz, -1)[:nz - 1, inner] - np.asarray(truth, np.float64).reshape(nz, -1)[:nz - 1, inner]
    return float(np.sqrt((d * d).mean()))


def noisy(obs, level=NOISE, seed=NOISE_SEED):
    """obs (fp64 or fp32 curves) times (1 + level * standard normal) of a fixed seed, fp32"""
    return (np.asarray(obs, np.float64) * (1.0 + level * np.random.default_rng(seed).standard_normal(obs.shape))).astype(F)


def loop(step, start, depz, obs, wt, curves, hs, iterations=R.ITERATIONS, after=None):
    """columns_ref.loop over a step of one's own: per iteration curves(model) -> (pv, svs, svp, srho), host_combine, step(model (nz, ncol), pv,
    S) -> a result with "vels".  after(iteration, model before, (pv, S), result): a hook.  Returns (model, [the results])."""
    nz, ny, nx = start.shape
    model = np.array(start, F, copy=True)
    results = []
    for it in range(iterations):
        pv, svs, svp, srho = curves(model)
        S = R.host_combine(hs, model.reshape(nz, ny * nx), depz, svs, svp, srho)
        out = step(model.reshape(nz, ny * nx), pv, S)
        if after is not None:
            after(it, model, (pv, S), out)
        results.append(out)
        model = out["vels"].reshape(nz, ny, nx)
    return model, results
