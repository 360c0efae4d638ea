"""Test infrastructure for the depth inversion of the maps' 2 psi terms: the CPU build of
dsurftomo_amd/csrc/column_azimuthal.h (tests/hostcheck_column_azimuthal.cpp) behind NumPy, built with columns_ref's flags, the columns of
the CPU checks and the comparison of two sets of figures, each quantity on its own scale.  Nothing under dsurftomo_amd/ imports this
module."""
import ctypes as C
import os
import subprocess

import numpy as np

import _libs as L
from column_resolution_ref import random_column, same_bits          # noqa: F401 (same_bits: for the tests that import this module)
from columns_ref import FLAGS

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libhostcheck_column_azimuthal.so")
SRC = os.path.join(HERE, "hostcheck_column_azimuthal.cpp")
HDR = [os.path.join(L.ROOT, "dsurftomo_amd", "csrc", n) for n in ("column_azimuthal.h", "column_resolution.h", "column_system.h")]
F = np.float32
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if L._stale(SO, [SRC] + HDR):
        subprocess.check_call(["g++"] + FLAGS + ["-shared", "-o", SO, SRC, "-lm"])
    lib = C.CDLL(SO)
    lib.hca_doubles.argtypes = [L.i32] * 2
    lib.hca_doubles.restype = C.c_longlong
    lib.hca_azimuthal.argtypes = [L.i32] * 3 + [L.vp] * 8 + [L.f32] * 2 + [L.vp] * 7
    lib.hca_azimuthal.restype = None
    lib.hca_finish.argtypes = [L.i32] * 2 + [L.vp] * 9
    _lib = lib
    return lib


def effective_weights(wt, love, shape):
    """the weights the engine hands to the kernel: wt (None: 1), 0 at a Love slot -- (K, n) fp32; love: (K) bool or None"""
    w = np.ones(shape, F) if wt is None else np.array(wt, F, copy=True).reshape(shape)
    if love is not None:
        w[np.asarray(love, bool)] = 0.0
    return w


def host_azimuthal(h, obs, a1, a2, wt, pv, Z, love, depz, smooth, damp, only=None, fill=0.0):
    """hca_azimuthal on columns side by side: obs / a1 / a2 / wt (K, n) fp32 (wt None: 1), pv (K, n), Z (M, K, n), love (K) bool or None,
    depz (M or more).  Returns dict(gc, gs (M, n), measures (4, M, n), leverage (K, n), chi2 (4, n), nused, flag (n), T (K, M, n)); the
    fp64 outputs start as fill."""
    M, K, n = Z.shape
    obs = np.ascontiguousarray(obs, F); a1 = np.ascontiguousarray(a1, F); a2 = np.ascontiguousarray(a2, F)
    pv = np.ascontiguousarray(pv, np.float64); Z = np.ascontiguousarray(Z, np.float64)
    weff = effective_weights(wt, love, (K, n))
    only = None if only is None else np.ascontiguousarray(only, np.uint8)
    depz = np.ascontiguousarray(depz, F)
    assert obs.shape == a1.shape == a2.shape == pv.shape == (K, n) and depz.size >= M and (only is None or only.shape == (n,))
    g = np.full((2, M, n), fill)
    out = dict(gc=g[0], gs=g[1], measures=np.full((4, M, n), fill), leverage=np.full((K, n), fill), chi2=np.full((4, n), fill), nused=np.zeros(n, np.int32),
               flag=np.zeros(n, np.int32), T=np.full((K, M, n), fill))
    h.hca_azimuthal(M, K, n, L.ptr(only), L.ptr(obs), L.ptr(weff), L.ptr(pv), L.ptr(Z), L.ptr(a1), L.ptr(a2), L.ptr(depz), smooth, damp, L.ptr(g),
                    L.ptr(out["measures"]), L.ptr(out["leverage"]), L.ptr(out["chi2"]), L.ptr(out["nused"]), L.ptr(out["flag"]), L.ptr(out["T"]))
    return out


def host_one(h, obs, a1, a2, wt, pv, Z, love, depz, smooth, damp, **kw):
    """the header on one column given as the twin takes it (Z (K, M)); the outputs without the column axis"""
    out = host_azimuthal(h, obs[:, None], a1[:, None], a2[:, None], None if wt is None else wt[:, None], pv[:, None], np.ascontiguousarray(Z.T)[:, :, None], love, depz,
                         smooth, damp, **kw)
    return {k: (v[..., 0] if v.ndim > 1 else v[0]) for k, v in out.items()}


def host_finish(h, N, G, a1, a2, depz):
    """hca_finish: N (M, M) symmetric (its lower triangle is used), G (K, M), every datum used at weight 1.  Returns (flag, dict of the outputs)."""
    G = np.ascontiguousarray(G, np.float64)
    K, M = G.shape
    tri = np.array([N[i][j] for i in range(M) for j in range(i + 1)], np.float64)
    g = np.full((2, M), 9.0)
    out = dict(gc=g[0], gs=g[1], measures=np.full((4, M), 9.0), leverage=np.full(K, 9.0), chi2=np.full(4, 9.0))
    flag = h.hca_finish(M, K, L.ptr(tri), L.ptr(G), L.ptr(np.ascontiguousarray(a1, F)), L.ptr(np.ascontiguousarray(a2, F)), L.ptr(np.ascontiguousarray(depz, F)), L.ptr(g),
                        L.ptr(out["measures"]), L.ptr(out["leverage"]), L.ptr(out["chi2"]))
    return flag, out


SIZES = [(1, 1, 0, 0), (2, 3, 0, 1), (7, 12, 3, 2), (63, 60, 5, 6)]        # (M, K, data made unused in the three ways, Love slots)
# The tolerance of every comparison with the twin, measured on the twin alone, the way sections 21 and 22 do it: the
# largest relative difference between depth.column_azimuthal_twin's L D L^T answer and its numpy.linalg.lstsq / pinv answer over all figures
# (differences below) per (M, K) on azimuthal_column with seed 11 (test_hostcheck_column_azimuthal.py prints it again), and those sections'
# factor, which covers other seeds.
MEASURED = {(1, 1): 7.9e-16, (2, 3): 4.2e-16, (7, 12): 1.8e-15, (63, 60): 1.6e-14}
FACTOR = 4.0
TOL = FACTOR * max(MEASURED.values())


def azimuthal_column(M, K, seed, unused=0, nlove=0):
    """column_resolution_ref.random_column's column with A1, A2 of a few per cent of c0 and of both signs and the last nlove slots Love
    slots (never one of the unused data when K allows); the Z and A of every unused datum and of every Love slot are NaN.  Returns obs, a1,
    a2, wt (K) fp32, pv (K), Z (K, M), love (K) bool, depz."""
    obs, wt, pv, Z, depz = random_column(M, K, seed, unused)
    rng = np.random.default_rng(1000 + seed)
    a1 = (0.03 * obs * rng.standard_normal(K)).astype(F)
    a2 = (0.03 * obs * rng.standard_normal(K)).astype(F)
    love = np.zeros(K, bool)
    if nlove:
        love[K - nlove:] = True
    dead = love | ~((wt > 0) & (obs > 0) & (pv > 0))
    Z = np.array(Z, copy=True)
    Z[dead] = np.nan; a1[dead] = np.nan; a2[dead] = np.nan
    return obs, a1, a2, wt, pv, Z, love, depz


def used_of(obs, wt, pv, love):
    """the rule: a Rayleigh slot that the isotropic step would use"""
    w = np.ones(len(obs), F) if wt is None else wt
    return (w > 0) & (obs > 0) & (pv > 0) & ~(np.zeros(len(obs), bool) if love is None else love)


def differences(a, b, rmax):
    """The largest differences between two sets of figures of one column, each on its scale: gc and gs relative to the largest |g| of b, chi2
    to its largest entry, R_jj and the leverages relative to rmax, the largest |R| of the case; m1, m2 and var relative to their own
    largest value.  a, b: dicts with gc, gs (M), chi2 (4), measures (4, M), leverage (K).  Returns {name: relative difference}."""
    gmax = max(np.abs(b["gc"]).max(), np.abs(b["gs"]).max())
    d = dict(g=max(np.abs(a["gc"] - b["gc"]).max(), np.abs(a["gs"] - b["gs"]).max()) / gmax if gmax > 0 else max(np.abs(a["gc"]).max(), np.abs(a["gs"]).max()),
             rjj=np.abs(a["measures"][0] - b["measures"][0]).max() / rmax, leverage=np.abs(a["leverage"] - b["leverage"]).max() / rmax)
    cmax = np.abs(b["chi2"]).max()
    d["chi2"] = np.abs(np.asarray(a["chi2"]) - np.asarray(b["chi2"])).max() / cmax if cmax > 0 else float(np.abs(a["chi2"]).max())
    for q, name in ((1, "m1"), (2, "m2"), (3, "var")):
        scale = np.abs(b["measures"][q]).max()
        d[name] = np.abs(a["measures"][q] - b["measures"][q]).max() / scale if scale > 0 else float(np.abs(a["measures"][q]).max())
    return d
