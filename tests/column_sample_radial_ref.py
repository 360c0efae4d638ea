"""Test infrastructure for the Monte-Carlo radial depth inversion: the CPU build of
dsurftomo_amd/csrc/column_sample_radial.h (tests/hostcheck_column_sample_radial.cpp) behind NumPy.  View mirrors the header's
SampleRadialView field by field (load() checks its size against the library's); Stage owns the arrays of one radial sample stage in the
device's layouts and runs the header's set-up, proposals, Metropolis tests and finish on them, with whatever fills pv between a proposal and
its test in place of the dispersion stage.  Nothing under dsurftomo_amd/ imports this module."""
import ctypes as C
import os
import subprocess

import numpy as np

import _libs as L
import columns_ref

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libhostcheck_column_sample_radial.so")
SRC = os.path.join(HERE, "hostcheck_column_sample_radial.cpp")
HDR = [os.path.join(L.ROOT, "dsurftomo_amd", "csrc", n) for n in ("column_sample_radial.h", "column_sample.h", "column_system.h")]
FLAGS = columns_ref.FLAGS
F = np.float32
u64 = C.c_ulonglong
_lib = None

IDLE, PENDING, OUT_OF_BOX, ACCEPTED, REJECTED, NO_ROOT = -1, 0, 1, 2, 3, 4          # column_sample.h's marks
# the raw state, in dsa_columns_sample_radial_state's order and under engine.columns_sample_radial_state's names
STATE = ("vsv", "vsh", "phi", "psi", "counters", "kinds", "S1v", "S2v", "S1h", "S2h", "Pvh", "X1", "X2", "npos", "phisum", "nkept", "best_e", "best_vsv", "best_vsh",
         "pnode", "pold_v", "pold_h", "pmark", "reseeded")
NODES = ("mean_v", "var_v", "W_v", "B_v", "mean_h", "var_h", "W_h", "B_h", "mean_xi", "var_xi", "W_xi", "B_xi", "best_v", "best_h", "cov_vh", "p_pos")
COUNTS = ("nused_r", "nused_l", "flag", "accepted", "rejected", "out_of_box", "no_root", "proposed_v", "proposed_h", "proposed_pair", "accepted_v", "accepted_h",
          "accepted_pair", "reseeded", "nkept")


class View(C.Structure):
    _fields_ = [(n, L.i32) for n in ("nx", "ny", "nz", "K", "C", "burn", "pairs")] + [("ncol", C.c_longlong), ("seed", u64), ("love", u64)] + \
               [(n, L.f64) for n in ("lam2", "gam2", "step", "spread", "two_t")] + [(n, L.f32) for n in ("width", "minvel", "maxvel")] + \
               [(n, L.vp) for n in ("obs", "wt", "v0v", "v0h", "pv", "vv", "vh", "phi", "psi", "cnt", "kcnt", "S1v", "S2v", "S1h", "S2h", "Pvh", "X1", "X2", "npos",
                                    "phisum", "nkept", "best_e", "best_vv", "best_vh", "pnode", "pold_v", "pold_h", "pmark", "reseed", "used", "nused_r", "nused_l",
                                    "flag", "phi0")]


def load():
    global _lib
    if _lib is not None:
        return _lib
    if L._stale(SO, [SRC] + HDR):
        subprocess.check_call(["g++"] + FLAGS + ["-shared", "-o", SO, SRC, "-lm"])
    lib = C.CDLL(SO)
    assert lib.hcr_view_bytes() == C.sizeof(View), "View does not mirror SampleRadialView"
    for name in ("hcr_setup", "hcr_propose", "hcr_accept"):
        getattr(lib, name).argtypes = [C.POINTER(View), L.i32]
        getattr(lib, name).restype = None
    lib.hcr_finish.argtypes = [C.POINTER(View), L.vp, L.vp, L.vp]
    lib.hcr_finish.restype = None
    lib.hcr_forward.argtypes = [C.POINTER(View), L.vp, L.vp, L.vp]
    lib.hcr_forward.restype = None
    lib.hcr_linear.argtypes = [C.POINTER(View), L.vp, L.vp, L.vp, L.i32, L.i32]
    lib.hcr_linear.restype = None
    _lib = lib
    return lib


def love_mask(love):
    """the bit mask of a (K) bool array: bit k set iff slot k is a Love slot"""
    return sum(1 << k for k, x in enumerate(love) if x)


class Stage:
    """The arrays of one radial sample stage in the device's layouts -- both model stores (nz, C, ncol), pv (C, K, ncol), the per-chain
    figures (C, ncol), the counters (4, C, ncol) and kinds (6, C, ncol), the per-depth sums (M, C, ncol) -- and the header's steps on them.
    start_v, start_h (nz, ncol) fp32, obs / wt (K, ncol) fp32 (wt may be None), love (K) bool."""

    def __init__(self, h, nx, ny, start_v, start_h, obs, wt, love, nchains, smooth, aniso, step, spread, width, temperature, minvel, maxvel, seed, burn, pairs=True):
        self.h = h
        self.start_v = start_v = np.ascontiguousarray(start_v, F)
        self.start_h = start_h = np.ascontiguousarray(start_h, F)
        nz, ncol = start_v.shape
        assert ncol == nx * ny and start_h.shape == start_v.shape
        self.nx, self.ny, self.nz, self.M, self.ncol, self.C = nx, ny, nz, nz - 1, ncol, int(nchains)
        self.obs = np.ascontiguousarray(obs, F)
        self.K = K = self.obs.shape[0]
        self.wt = None if wt is None else np.ascontiguousarray(wt, F)
        self.love = np.asarray(love, bool)
        assert self.love.shape == (K,)
        Cn, M = self.C, self.M
        f64 = lambda *s: np.zeros(s)
        i32 = lambda *s: np.zeros(s, np.int32)
        f32 = lambda *s: np.zeros(s, F)
        a = self.a = dict(vsv=f32(nz, Cn, ncol), vsh=f32(nz, Cn, ncol), phi=f64(Cn, ncol), psi=f64(Cn, ncol), counters=i32(4, Cn, ncol), kinds=i32(6, Cn, ncol),
                          S1v=f64(M, Cn, ncol), S2v=f64(M, Cn, ncol), S1h=f64(M, Cn, ncol), S2h=f64(M, Cn, ncol), Pvh=f64(M, Cn, ncol), X1=f64(M, Cn, ncol),
                          X2=f64(M, Cn, ncol), npos=i32(M, Cn, ncol), phisum=f64(Cn, ncol), nkept=i32(Cn, ncol), best_e=f64(Cn, ncol), best_vsv=f32(M, Cn, ncol),
                          best_vsh=f32(M, Cn, ncol), pnode=i32(Cn, ncol), pold_v=f32(Cn, ncol), pold_h=f32(Cn, ncol), pmark=i32(Cn, ncol), reseeded=i32(Cn, ncol))
        assert tuple(a) == STATE
        self.pv = np.zeros((Cn, K, ncol))
        self.used = np.zeros(ncol, np.uint64); self.nused_r = i32(ncol); self.nused_l = i32(ncol); self.flag = i32(ncol); self.phi0 = f64(ncol)
        v = self.view = View()
        v.nx, v.ny, v.nz, v.K, v.C, v.burn, v.pairs, v.ncol, v.seed, v.love = nx, ny, nz, K, Cn, int(burn), int(pairs), ncol, int(seed), love_mask(self.love)
        v.lam2 = float(F(smooth)) * float(F(smooth)); v.gam2 = float(F(aniso)) * float(F(aniso))
        v.step = float(F(step)); v.spread = float(F(spread)); v.two_t = 2.0 * float(F(temperature))
        v.width, v.minvel, v.maxvel = float(width), float(minvel), float(maxvel)
        v.obs, v.wt, v.v0v, v.v0h, v.pv, v.vv, v.vh = L.ptr(self.obs), L.ptr(self.wt), L.ptr(start_v), L.ptr(start_h), L.ptr(self.pv), L.ptr(a["vsv"]), L.ptr(a["vsh"])
        v.phi, v.psi, v.cnt, v.kcnt = (L.ptr(a[n]) for n in ("phi", "psi", "counters", "kinds"))
        v.S1v, v.S2v, v.S1h, v.S2h, v.Pvh, v.X1, v.X2, v.npos = (L.ptr(a[n]) for n in ("S1v", "S2v", "S1h", "S2h", "Pvh", "X1", "X2", "npos"))
        v.phisum, v.nkept, v.best_e, v.best_vv, v.best_vh = (L.ptr(a[n]) for n in ("phisum", "nkept", "best_e", "best_vsv", "best_vsh"))
        v.pnode, v.pold_v, v.pold_h, v.pmark, v.reseed = (L.ptr(a[n]) for n in ("pnode", "pold_v", "pold_h", "pmark", "reseeded"))
        v.used, v.nused_r, v.nused_l, v.flag, v.phi0 = L.ptr(self.used), L.ptr(self.nused_r), L.ptr(self.nused_l), L.ptr(self.flag), L.ptr(self.phi0)
        self.sweep = 0

    def setup_models(self):
        self.h.hcr_setup(C.byref(self.view), 0)

    def setup_state(self, pv=None):
        if pv is not None:
            self.pv[...] = np.asarray(pv).reshape(self.pv.shape)
        self.h.hcr_setup(C.byref(self.view), 1)

    def propose(self):
        self.sweep += 1
        self.h.hcr_propose(C.byref(self.view), self.sweep)

    def accept(self, pv=None):
        if pv is not None:
            self.pv[...] = np.asarray(pv).reshape(self.pv.shape)
        self.h.hcr_accept(C.byref(self.view), self.sweep)

    def forward(self, pv0, A):
        """pv = pv0 (K, ncol) + A (K, M, ncol) (v - start) on every chain, v the chain's Vsh at a Love slot and its Vsv elsewhere"""
        self.h.hcr_forward(C.byref(self.view), L.ptr(pv0), L.ptr(A), L.ptr(self.pv))

    def linear(self, pv0, A, nsweeps):
        self.h.hcr_linear(C.byref(self.view), L.ptr(pv0), L.ptr(A), L.ptr(self.pv), self.sweep + 1, int(nsweeps))
        self.sweep += int(nsweeps)

    def finish(self):
        """dict of NODES (M, ncol), phi_start, best_energy, mean_phi (ncol) and COUNTS (ncol) int32, engine.columns_sample_radial_fetch's"""
        nodes = np.zeros((16, self.M, self.ncol)); cols = np.zeros((3, self.ncol)); counts = np.zeros((15, self.ncol), np.int32)
        self.h.hcr_finish(C.byref(self.view), L.ptr(nodes), L.ptr(cols), L.ptr(counts))
        out = dict(zip(NODES, nodes))
        out.update(zip(("phi_start", "best_energy", "mean_phi"), cols))
        out.update(zip(COUNTS, counts))
        return out

    def state(self):
        return {n: self.a[n].copy() for n in STATE}
