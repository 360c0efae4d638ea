"""Test infrastructure for the Monte-Carlo depth inversion: the CPU build of dsurftomo_amd/csrc/column_sample.h
(tests/hostcheck_column_sample.cpp) behind NumPy.  View mirrors the header's SampleView field by field (load() checks its size against the
library's); Stage owns the arrays of one sample stage in the device's layouts and runs the header's set-up, proposals, Metropolis tests and
finish on them, with whatever fills pv between a proposal and its test in place of the dispersion stage.  Nothing under dsurftomo_amd/
imports this module."""
import ctypes as C
import os
import subprocess

import numpy as np

import _libs as L

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libhostcheck_column_sample.so")
SRC = os.path.join(HERE, "hostcheck_column_sample.cpp")
HDR = [os.path.join(L.ROOT, "dsurftomo_amd", "csrc", n) for n in ("column_sample.h", "column_system.h")]
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-msse2", "-mfpmath=sse"]
F = np.float32
u64 = C.c_ulonglong
_lib = None

IDLE, PENDING, OUT_OF_BOX, ACCEPTED, REJECTED, NO_ROOT = -1, 0, 1, 2, 3, 4          # column_sample.h's marks
STATE = ("models", "phi", "psi", "counters", "S1", "S2", "phisum", "nkept", "best_e", "best_v", "pnode", "pold", "pmark", "reseeded")


class View(C.Structure):
    _fields_ = [(n, L.i32) for n in ("nx", "ny", "nz", "K", "C", "burn")] + [("ncol", C.c_longlong), ("seed", u64)] + \
               [(n, L.f64) for n in ("lam2", "step", "spread", "two_t")] + [(n, L.f32) for n in ("width", "minvel", "maxvel")] + \
               [(n, L.vp) for n in ("obs", "wt", "v0", "pv", "v", "phi", "psi", "cnt", "S1", "S2", "phisum", "nkept", "best_e", "best_v", "pnode", "pold", "pmark",
                                    "reseed", "used", "nused", "flag", "phi0")]


def load():
    global _lib
    if _lib is not None:
        return _lib
    if L._stale(SO, [SRC] + HDR):
        subprocess.check_call(["g++"] + FLAGS + ["-shared", "-o", SO, SRC, "-lm"])
    lib = C.CDLL(SO)
    assert lib.hcs_view_bytes() == C.sizeof(View), "View does not mirror SampleView"
    lib.hcs_bits.argtypes = [u64] * 5
    lib.hcs_bits.restype = u64
    lib.hcs_unit.argtypes = [u64]
    lib.hcs_unit.restype = L.f64
    lib.hcs_draws.argtypes = [C.c_longlong, L.vp, L.vp, L.vp]
    lib.hcs_draws.restype = None
    lib.hcs_neglog.argtypes = [C.c_longlong, L.vp, L.vp]
    lib.hcs_neglog.restype = None
    lib.hcs_psi.argtypes = [L.i32, L.f64, L.vp]
    lib.hcs_psi.restype = L.f64
    for name in ("hcs_setup", "hcs_propose", "hcs_accept"):
        getattr(lib, name).argtypes = [C.POINTER(View), L.i32]
        getattr(lib, name).restype = None
    lib.hcs_finish.argtypes = [C.POINTER(View), L.vp, L.vp, L.vp]
    lib.hcs_finish.restype = None
    lib.hcs_forward.argtypes = [C.POINTER(View), L.vp, L.vp, L.vp]
    lib.hcs_forward.restype = None
    lib.hcs_linear.argtypes = [C.POINTER(View), L.vp, L.vp, L.vp, L.i32, L.i32]
    lib.hcs_linear.restype = None
    _lib = lib
    return lib


def neglog(h, k):
    k = np.ascontiguousarray(k, np.uint64)
    out = np.zeros(k.size)
    h.hcs_neglog(k.size, L.ptr(k), L.ptr(out))
    return out


def draws(h, w):
    """w: (n, 5) seed, column, chain, sweep, draw.  Returns (k, u)."""
    w = np.ascontiguousarray(w, np.uint64)
    k = np.zeros(len(w), np.uint64); u = np.zeros(len(w))
    h.hcs_draws(len(w), L.ptr(w), L.ptr(k), L.ptr(u))
    return k, u


class Stage:
    """The arrays of one sample stage in the device's layouts -- models (nz, C, ncol), pv (C, K, ncol), the per-chain figures (C, ncol), the
    counters (4, C, ncol), S1 / S2 / best_v (M, C, ncol) -- and the header's steps on them.  start (nz, ncol) fp32, obs / wt (K, ncol) fp32
    (wt may be None)."""

    def __init__(self, h, nx, ny, start, obs, wt, nchains, smooth, step, spread, width, temperature, minvel, maxvel, seed, burn):
        self.h = h
        start = np.ascontiguousarray(start, F)
        nz, ncol = start.shape
        assert ncol == nx * ny
        self.nx, self.ny, self.nz, self.M, self.ncol, self.C = nx, ny, nz, nz - 1, ncol, int(nchains)
        self.obs = np.ascontiguousarray(obs, F)
        self.K = K = self.obs.shape[0]
        self.wt = None if wt is None else np.ascontiguousarray(wt, F)
        self.start = start
        Cn, M = self.C, self.M
        a = self.a = dict(models=np.zeros((nz, Cn, ncol), F), phi=np.zeros((Cn, ncol)), psi=np.zeros((Cn, ncol)), counters=np.zeros((4, Cn, ncol), np.int32),
                          S1=np.zeros((M, Cn, ncol)), S2=np.zeros((M, Cn, ncol)), phisum=np.zeros((Cn, ncol)), nkept=np.zeros((Cn, ncol), np.int32),
                          best_e=np.zeros((Cn, ncol)), best_v=np.zeros((M, Cn, ncol), F), pnode=np.zeros((Cn, ncol), np.int32), pold=np.zeros((Cn, ncol), F),
                          pmark=np.zeros((Cn, ncol), np.int32), reseeded=np.zeros((Cn, ncol), np.int32))
        self.pv = np.zeros((Cn, K, ncol))
        self.used = np.zeros(ncol, np.uint64); self.nused = np.zeros(ncol, np.int32); self.flag = np.zeros(ncol, np.int32); self.phi0 = np.zeros(ncol)
        v = self.view = View()
        v.nx, v.ny, v.nz, v.K, v.C, v.burn, v.ncol, v.seed = nx, ny, nz, K, Cn, int(burn), ncol, int(seed)
        v.lam2 = float(F(smooth)) * float(F(smooth)); v.step = float(F(step)); v.spread = float(F(spread)); v.two_t = 2.0 * float(F(temperature))
        v.width, v.minvel, v.maxvel = float(width), float(minvel), float(maxvel)
        v.obs, v.wt, v.v0, v.pv, v.v = L.ptr(self.obs), L.ptr(self.wt), L.ptr(self.start), L.ptr(self.pv), L.ptr(a["models"])
        v.phi, v.psi, v.cnt, v.S1, v.S2, v.phisum, v.nkept = (L.ptr(a[n]) for n in ("phi", "psi", "counters", "S1", "S2", "phisum", "nkept"))
        v.best_e, v.best_v, v.pnode, v.pold, v.pmark, v.reseed = (L.ptr(a[n]) for n in ("best_e", "best_v", "pnode", "pold", "pmark", "reseeded"))
        v.used, v.nused, v.flag, v.phi0 = L.ptr(self.used), L.ptr(self.nused), L.ptr(self.flag), L.ptr(self.phi0)
        self.sweep = 0

    def setup_models(self):
        self.h.hcs_setup(C.byref(self.view), 0)

    def setup_state(self, pv=None):
        if pv is not None:
            self.pv[...] = np.asarray(pv).reshape(self.pv.shape)
        self.h.hcs_setup(C.byref(self.view), 1)

    def propose(self):
        self.sweep += 1
        self.h.hcs_propose(C.byref(self.view), self.sweep)

    def accept(self, pv=None):
        if pv is not None:
            self.pv[...] = np.asarray(pv).reshape(self.pv.shape)
        self.h.hcs_accept(C.byref(self.view), self.sweep)

    def forward(self, pv0, A):
        """pv = pv0 (K, ncol) + A (K, M, ncol) (v - start) on every chain"""
        self.h.hcs_forward(C.byref(self.view), L.ptr(pv0), L.ptr(A), L.ptr(self.pv))

    def linear(self, pv0, A, nsweeps):
        self.h.hcs_linear(C.byref(self.view), L.ptr(pv0), L.ptr(A), L.ptr(self.pv), self.sweep + 1, int(nsweeps))
        self.sweep += int(nsweeps)

    def finish(self):
        nodes = np.zeros((5, self.M, self.ncol)); cols = np.zeros((3, self.ncol)); counts = np.zeros((8, self.ncol), np.int32)
        self.h.hcs_finish(C.byref(self.view), L.ptr(nodes), L.ptr(cols), L.ptr(counts))
        return nodes, cols, counts

    def state(self):
        return {n: self.a[n].copy() for n in STATE}
