"""Test infrastructure for the depth resolution of the columns: the CPU build of
dsurftomo_amd/csrc/column_resolution.h (tests/hostcheck_column_resolution.cpp) behind NumPy, built with columns_ref's flags, and the
comparison of two sets of resolution figures, each quantity on its own scale.  Nothing under dsurftomo_amd/ imports this module."""
import ctypes as C
import os
import subprocess

import numpy as np

import _libs as L
from columns_ref import FLAGS

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libhostcheck_column_resolution.so")
SRC = os.path.join(HERE, "hostcheck_column_resolution.cpp")
HDR = [os.path.join(L.ROOT, "dsurftomo_amd", "csrc", n) for n in ("column_resolution.h", "column_system.h")]
F = np.float32
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if L._stale(SO, [SRC] + HDR):
        subprocess.check_call(["g++"] + FLAGS + ["-shared", "-o", SO, SRC, "-lm"])
    lib = C.CDLL(SO)
    lib.hcr_doubles.argtypes = [L.i32] * 2
    lib.hcr_doubles.restype = C.c_longlong
    lib.hcr_resolution.argtypes = [L.i32] * 3 + [L.vp] * 6 + [L.f32] * 2 + [L.vp] * 7
    lib.hcr_resolution.restype = None
    lib.hcr_rows_by_column_solve.argtypes = [L.i32] * 2 + [L.vp] * 4 + [L.f32] * 2 + [L.vp]
    lib.hcr_finish.argtypes = [L.i32] * 2 + [L.vp] * 7
    _lib = lib
    return lib


def host_resolution(h, obs, wt, pv, S, depz, smooth, damp, only=None, full=True, fill=0.0):
    """hcr_resolution on columns side by side: obs / wt (K, n) fp32, pv (K, n), S (M, K, n), depz (M or more).  Returns dict(measures
    (4, M, n), leverage (K, n), trace, nused, flag (n), T (K, M, n), and with full R (M, M, n)); the fp64 outputs start as fill."""
    M, K, n = S.shape
    obs = np.ascontiguousarray(obs, F); pv = np.ascontiguousarray(pv, np.float64); S = np.ascontiguousarray(S, np.float64)
    wt = None if wt is None else np.ascontiguousarray(wt, F)
    only = None if only is None else np.ascontiguousarray(only, np.uint8)
    depz = np.ascontiguousarray(depz, F)
    assert obs.shape == (K, n) and pv.shape == (K, n) and depz.size >= M
    assert (wt is None or wt.shape == (K, n)) and (only is None or only.shape == (n,))
    out = dict(measures=np.full((4, M, n), fill), leverage=np.full((K, n), fill), trace=np.full(n, fill), nused=np.zeros(n, np.int32),
               flag=np.zeros(n, np.int32), T=np.full((K, M, n), fill))
    if full:
        out["R"] = np.full((M, M, n), fill)
    h.hcr_resolution(M, K, n, L.ptr(only), L.ptr(obs), L.ptr(wt), L.ptr(pv), L.ptr(S), L.ptr(depz), smooth, damp, L.ptr(out["measures"]), L.ptr(out["leverage"]),
                     L.ptr(out["trace"]), L.ptr(out["R"]) if full else None, L.ptr(out["nused"]), L.ptr(out["flag"]), L.ptr(out["T"]))
    return out


def rows_by_column_solve(h, obs, wt, pv, S, smooth, damp):
    """(flag, T (K, M)) of one column (obs, wt, pv (K), S (K, M)): the step's column_solve applied to every row of G"""
    K, M = S.shape
    T = np.zeros((K, M))
    St = np.ascontiguousarray(S.T, np.float64)
    flag = h.hcr_rows_by_column_solve(M, K, L.ptr(np.ascontiguousarray(obs, F)), L.ptr(None if wt is None else np.ascontiguousarray(wt, F)),
                                      L.ptr(np.ascontiguousarray(pv, np.float64)), L.ptr(St), smooth, damp, L.ptr(T))
    return flag, T


def host_finish(h, N, G, depz, full=True):
    """hcr_finish: N (M, M) symmetric (its lower triangle is used), G (K, M), every datum used.  Returns (flag, dict of the outputs)."""
    G = np.ascontiguousarray(G, np.float64)
    K, M = G.shape
    tri = np.array([N[i][j] for i in range(M) for j in range(i + 1)], np.float64)
    out = dict(measures=np.full((4, M), 9.0), leverage=np.full(K, 9.0), trace=np.full(1, 9.0))
    if full:
        out["R"] = np.full((M, M), 9.0)
    flag = h.hcr_finish(M, K, L.ptr(tri), L.ptr(G), L.ptr(np.ascontiguousarray(depz, F)), L.ptr(out["measures"]), L.ptr(out["leverage"]), L.ptr(out["trace"]),
                        L.ptr(out["R"]) if full else None)
    return flag, out


SIZES = [(1, 1, 0), (2, 3, 1), (7, 12, 3), (63, 60, 5)]        # (M, K, data made unused)
# The tolerance of every comparison with the twin, measured on the twin alone: max |R_ldlt - R_pinv| / max |R_pinv|
# of depth.column_resolution_twin's two answers per (M, K) on random_column with seed 11 (test_hostcheck_column_resolution.py prints it
# again), and the factor that covers other seeds -- section 21's margin for the same kind of comparison.
MEASURED = {(1, 1): 3.4e-16, (2, 3): 2.7e-16, (7, 12): 1.0e-15, (63, 60): 8.0e-15}
FACTOR = 4.0
TOL = FACTOR * max(MEASURED.values())


def random_column(M, K, seed, unused=0):
    """a well-posed column as test_hostcheck_columns.py makes them -- positive kernels of the size of real ones (a datum's kernel sums to
    about one over depth), weights around 1 -- with `unused` of its data dropped in turn for no weight, no observation and no root, their
    kernels NaN.  Returns obs, wt (K) fp32, pv (K), S (K, M), depz (M + 1) fp32 with spacings growing from 2 km."""
    rng = np.random.default_rng(seed)
    S = rng.random((K, M)) * (2.0 / M)
    pv = 3.0 + rng.random(K)
    obs = (pv * (1.0 + 0.03 * rng.standard_normal(K))).astype(F)
    wt = (0.5 + rng.random(K)).astype(F)
    for n, k in enumerate(rng.choice(K, unused, replace=False)):
        if n % 3 == 0:
            wt[k] = 0.0
        elif n % 3 == 1:
            obs[k] = 0.0
        else:
            pv[k] = 0.0
        S[k] = np.nan
    depz = np.concatenate([[0.0], np.cumsum(2.0 + 4.0 * np.arange(M) / max(M - 1, 1))]).astype(F)
    return obs, wt, pv, S, depz


def differences(a, b, rmax):
    """The largest differences between two sets of figures of one column, each on its scale: R, R_jj, the leverages and the trace relative to
    rmax, the largest |R| of the case (all are sums of products of the same size); m1, m2 and var, which carry other units, relative to
    their own largest value.  a, b: dicts with R (M, M), measures (4, M), leverage (K), trace.  Returns {name: relative difference}."""
    d = dict(R=np.abs(a["R"] - b["R"]).max() / rmax, rjj=np.abs(a["measures"][0] - b["measures"][0]).max() / rmax,
             leverage=np.abs(a["leverage"] - b["leverage"]).max() / rmax, trace=abs(float(a["trace"]) - float(b["trace"])) / rmax)
    for q, name in ((1, "m1"), (2, "m2"), (3, "var")):
        scale = np.abs(b["measures"][q]).max()
        d[name] = np.abs(a["measures"][q] - b["measures"][q]).max() / scale if scale > 0 else float(np.abs(a["measures"][q]).max())
    return d


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
