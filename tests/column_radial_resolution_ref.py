"""Test infrastructure for the depth resolution of the radial step: the CPU build of
dsurftomo_amd/csrc/column_radial_resolution.h (tests/hostcheck_column_radial_resolution.cpp) behind NumPy, built with columns_ref's flags,
the made-up columns of the tests and the comparison of two sets of figures, each quantity on its own scale.  Nothing under dsurftomo_amd/
imports this module."""
import ctypes as C
import os
import subprocess

import numpy as np

import _libs as L
from column_radial_ref import mask, same_bits          # noqa: F401  (same_bits: for the tests)
from columns_ref import FLAGS

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libhostcheck_column_radial_resolution.so")
SRC = os.path.join(HERE, "hostcheck_column_radial_resolution.cpp")
HDR = [os.path.join(L.ROOT, "dsurftomo_amd", "csrc", n) for n in ("column_radial_resolution.h", "column_resolution.h", "column_radial.h", "column_system.h")]
F = np.float32
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if L._stale(SO, [SRC] + HDR):
        subprocess.check_call(["g++"] + FLAGS + ["-shared", "-o", SO, SRC, "-lm"])
    lib = C.CDLL(SO)
    lib.hrr_doubles.argtypes = [L.i32] * 2
    lib.hrr_doubles.restype = C.c_longlong
    lib.hrr_resolution.argtypes = [L.i32] * 3 + [L.vp, C.c_ulonglong] + [L.vp] * 8 + [L.f32] * 3 + [L.vp] * 8
    lib.hrr_resolution.restype = None
    lib.hrr_rows_by_column_solve.argtypes = [L.i32] * 2 + [C.c_ulonglong] + [L.vp] * 7 + [L.f32] * 3 + [L.vp]
    lib.hrr_finish.argtypes = [L.i32] * 2 + [C.c_ulonglong] + [L.vp] * 8
    _lib = lib
    return lib


def host_resolution(h, love, obs, wt, pv, Sv, Sh, depz, vsv, vsh, smooth, damp, aniso, only=None, full=True, fill=0.0):
    """hrr_resolution on columns side by side: obs / wt (K, n) fp32, pv (K, n), Sv / Sh (M, K, n), depz (M or more), vsv / vsh (>= M, n) fp32.
    Returns dict(measures (6, 2M, n), pair (2, M, n), leverage (K, n), trace (2, n), nused (2, n), flag (n), T (K, 2M, n), and with full R
    (2M, 2M, n)); the fp64 outputs start as fill."""
    M, K, n = Sv.shape
    obs = np.ascontiguousarray(obs, F); pv = np.ascontiguousarray(pv, np.float64)
    Sv = np.ascontiguousarray(Sv, np.float64); Sh = np.ascontiguousarray(Sh, np.float64)
    wt = None if wt is None else np.ascontiguousarray(wt, F)
    only = None if only is None else np.ascontiguousarray(only, np.uint8)
    depz = np.ascontiguousarray(depz, F); vsv = np.ascontiguousarray(vsv, F); vsh = np.ascontiguousarray(vsh, F)
    assert obs.shape == (K, n) and pv.shape == (K, n) and Sh.shape == Sv.shape and depz.size >= M and len(love) == K
    assert vsv.shape == vsh.shape and vsv.shape[0] >= M and vsv.shape[1] == n
    assert (wt is None or wt.shape == (K, n)) and (only is None or only.shape == (n,))
    out = dict(measures=np.full((6, 2 * M, n), fill), pair=np.full((2, M, n), fill), leverage=np.full((K, n), fill), trace=np.full((2, n), fill),
               nused=np.zeros((2, n), np.int32), flag=np.zeros(n, np.int32), T=np.full((K, 2 * M, n), fill))
    if full:
        out["R"] = np.full((2 * M, 2 * M, n), fill)
    h.hrr_resolution(M, K, n, L.ptr(only), mask(love), L.ptr(obs), L.ptr(wt), L.ptr(pv), L.ptr(Sv), L.ptr(Sh), L.ptr(depz), L.ptr(vsv), L.ptr(vsh), smooth, damp, aniso,
                     L.ptr(out["measures"]), L.ptr(out["pair"]), L.ptr(out["leverage"]), L.ptr(out["trace"]), L.ptr(out["R"]) if full else None, L.ptr(out["nused"]),
                     L.ptr(out["flag"]), L.ptr(out["T"]))
    return out


def split(S, love, n=1):
    """the twin's compact S (K, M) of one column as the engine holds it: (Sv, Sh), each (M, K, 1), a slot's sensitivities on the model it was
    not run on NaN (they are never read)"""
    love = np.asarray(love, bool)
    St = np.ascontiguousarray(np.asarray(S, np.float64).T)[:, :, None]
    return np.where(love[None, :, None], np.nan, St), np.where(love[None, :, None], St, np.nan)


def host_one(h, love, obs, wt, pv, S, depz, vsv, vsh, smooth, damp, aniso, **kw):
    """the header on one column given as the twin takes it (S compact); the outputs without the column axis"""
    Sv, Sh = split(S, love)
    out = host_resolution(h, love, obs[:, None], None if wt is None else wt[:, None], pv[:, None], Sv, Sh, depz, np.asarray(vsv, F)[:, None], np.asarray(vsh, F)[:, None],
                          smooth, damp, aniso, **kw)
    return {k: v[..., 0] for k, v in out.items()}


def rows_by_column_solve(h, love, obs, wt, pv, S, vsv, vsh, smooth, damp, aniso):
    """(flag, T (K, 2M)) of one column: the step's column_solve on 2M unknowns applied to every row of the expanded G"""
    K, M = S.shape
    T = np.zeros((K, 2 * M))
    Sv, Sh = split(S, love)
    flag = h.hrr_rows_by_column_solve(M, K, mask(love), L.ptr(np.ascontiguousarray(obs, F)), L.ptr(None if wt is None else np.ascontiguousarray(wt, F)),
                                      L.ptr(np.ascontiguousarray(pv, np.float64)), L.ptr(np.ascontiguousarray(Sv[:, :, 0])), L.ptr(np.ascontiguousarray(Sh[:, :, 0])),
                                      L.ptr(np.ascontiguousarray(vsv, F)), L.ptr(np.ascontiguousarray(vsh, F)), smooth, damp, aniso, L.ptr(T))
    return flag, T


def host_finish(h, love, N, G, depz, full=True):
    """hrr_finish: N (2M, 2M) symmetric (its lower triangle is used), G (K, M) compact, every datum used.  Returns (flag, dict of the outputs)."""
    G = np.ascontiguousarray(G, np.float64)
    K, M = G.shape
    n2 = 2 * M
    tri = np.array([N[i][j] for i in range(n2) for j in range(i + 1)], np.float64)
    out = dict(measures=np.full((6, n2), 9.0), pair=np.full((2, M), 9.0), leverage=np.full(K, 9.0), trace=np.full(2, 9.0))
    if full:
        out["R"] = np.full((n2, n2), 9.0)
    flag = h.hrr_finish(M, K, mask(love), L.ptr(tri), L.ptr(G), L.ptr(np.ascontiguousarray(depz, F)), L.ptr(out["measures"]), L.ptr(out["pair"]), L.ptr(out["leverage"]),
                        L.ptr(out["trace"]), L.ptr(out["R"]) if full else None)
    return flag, out


SIZES = [(1, 2, 0), (2, 4, 1), (7, 12, 3), (63, 60, 5)]        # (M, K, data made unused)
SEEDS = (11, 12, 13)
SMOOTH, DAMP, ANISO = 0.3, 0.1, 0.2
# The tolerance of every comparison with the twin, measured on the twin alone: the largest max |R_ldlt - R_pinv| /
# max |R_pinv| of depth.column_radial_resolution_twin's two answers per (M, K) on random_column over SEEDS at SMOOTH, DAMP, ANISO
# (test_hostcheck_column_radial_resolution.py prints it again), and section 22's factor.
MEASURED = {(1, 2): 4.6e-16, (2, 4): 8.1e-16, (7, 12): 2.6e-15, (63, 60): 1.3e-14}
FACTOR = 4.0
TOL = FACTOR * max(MEASURED.values())


def random_column(M, K, seed, unused=0, love=None):
    """a well-posed radial column: column_resolution_ref.random_column's kernels, curves, observations and weights, the odd slots Love slots
    (love (K) bool overrides), `unused` of the data dropped in turn for no weight, no observation and no root, their kernels NaN -- never
    the last used datum of a wave type.  Returns love (K) bool, obs, wt (K) fp32, pv (K), S (K, M) compact, depz (M + 1) fp32, vsv, vsh
    (M + 1) fp32 with Vsh 4 % above Vsv."""
    rng = np.random.default_rng(seed)
    love = (np.arange(K) % 2 == 1) if love is None else np.asarray(love, bool)
    S = rng.random((K, M)) * (2.0 / M)
    pv = 3.0 + rng.random(K)
    obs = (pv * (1.0 + 0.03 * rng.standard_normal(K))).astype(F)
    wt = (0.5 + rng.random(K)).astype(F)
    left = [int((~love).sum()), int(love.sum())]
    n = 0
    for k in rng.permutation(K):
        if n == unused:
            break
        if left[int(love[k])] <= 1:
            continue
        left[int(love[k])] -= 1
        if n % 3 == 0:
            wt[k] = 0.0
        elif n % 3 == 1:
            obs[k] = 0.0
        else:
            pv[k] = 0.0
        S[k] = np.nan
        n += 1
    assert n == unused
    depz = np.concatenate([[0.0], np.cumsum(2.0 + 4.0 * np.arange(M) / max(M - 1, 1))]).astype(F)
    vsv = (3.0 + rng.random(M + 1)).astype(F)
    vsh = (vsv * F(1.04)).astype(F)
    return love, obs, wt, pv, S, depz, vsv, vsh


def differences(a, b, rmax):
    """The largest differences between two sets of figures of one column, each on its scale: R, R_jj, R_cross, the leverages and the traces
    relative to rmax, the largest |R| of the case (all are sums of products of the same size); m1_own, m2_own, m1_cross, var, cov and vard,
    which carry other units, relative to their own largest value.  a, b: dicts with R (2M, 2M), measures (6, 2M), pair (2, M), leverage
    (K), trace (2).  Returns {name: relative difference}."""
    d = dict(R=np.abs(a["R"] - b["R"]).max() / rmax, rjj=np.abs(a["measures"][0] - b["measures"][0]).max() / rmax,
             rcross=np.abs(a["measures"][4] - b["measures"][4]).max() / rmax, leverage=np.abs(a["leverage"] - b["leverage"]).max() / rmax,
             trace=np.abs(np.asarray(a["trace"]) - np.asarray(b["trace"])).max() / rmax)

    def own(x, y):
        scale = np.abs(y).max()
        return np.abs(x - y).max() / scale if scale > 0 else float(np.abs(x).max())

    for q, name in ((1, "m1_own"), (2, "m2_own"), (3, "m1_cross"), (5, "var")):
        d[name] = own(a["measures"][q], b["measures"][q])
    d["cov"] = own(a["pair"][0], b["pair"][0]); d["vard"] = own(a["pair"][1], b["pair"][1])
    return d
