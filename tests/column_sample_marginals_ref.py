"""Test infrastructure for the posterior marginals of the Monte-Carlo depth inversion: the CPU build of
dsurftomo_amd/csrc/column_sample.h with them (tests/hostcheck_column_sample_marginals.cpp) behind NumPy.  MarginalView mirrors the header's
SampleMarginalView field by field (load() checks all three views' sizes against the library's); MarginalStage is
column_sample_block_ref.BlockStage with the marginals' state beside it: every accept also takes the sweep's counts and products, as the
device does after its Metropolis test.  Nothing under dsurftomo_amd/ imports this module."""
import ctypes as C
import os
import subprocess

import numpy as np

import _libs as L
import column_sample_block_ref as B
import column_sample_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libhostcheck_column_sample_marginals.so")
SRC = os.path.join(HERE, "hostcheck_column_sample_marginals.cpp")
FLAGS = R.FLAGS
F = np.float32
_lib = None

LEVELS = (0.025, 0.16, 0.5, 0.84, 0.975)


class MarginalView(C.Structure):
    _fields_ = [("nbins", L.i32), ("hist", L.vp), ("P", L.vp)]


def load():
    global _lib
    if _lib is not None:
        return _lib
    if L._stale(SO, [SRC, B.SRC, R.SRC] + R.HDR):
        subprocess.check_call(["g++"] + FLAGS + ["-shared", "-o", SO, SRC, "-lm"])
    lib = C.CDLL(SO)
    assert lib.hcs_view_bytes() == C.sizeof(R.View), "View does not mirror SampleView"
    assert lib.hcb_block_bytes() == C.sizeof(B.BlockView), "BlockView does not mirror SampleBlockView"
    assert lib.hcm_marginal_bytes() == C.sizeof(MarginalView), "MarginalView does not mirror SampleMarginalView"
    lib.hcm_bin.argtypes = [C.POINTER(R.View), C.c_longlong, L.i32, L.i32, C.c_longlong, L.vp, L.vp]
    lib.hcm_bin.restype = None
    lib.hcm_accumulate.argtypes = [C.POINTER(R.View), C.POINTER(MarginalView), L.i32]
    lib.hcm_accumulate.restype = None
    lib.hcm_linear.argtypes = [C.POINTER(R.View), C.POINTER(B.BlockView), C.POINTER(MarginalView), L.vp, L.vp, L.vp, L.i32, L.i32]
    lib.hcm_linear.restype = None
    lib.hcm_finish.argtypes = [C.POINTER(R.View), C.POINTER(MarginalView), L.i32, L.vp, L.vp, L.vp, L.vp]
    lib.hcm_finish.restype = None
    lib.hcb_shape.argtypes = [L.i32] * 4 + [L.vp] * 4 + [L.f32] * 2 + [L.vp] * 4
    lib.hcb_shape.restype = None
    for name in ("hcb_propose", "hcb_accept"):
        getattr(lib, name).argtypes = [C.POINTER(R.View), C.POINTER(B.BlockView), L.i32]
        getattr(lib, name).restype = None
    lib.hcs_setup.argtypes = [C.POINTER(R.View), L.i32]
    lib.hcs_setup.restype = None
    lib.hcs_finish.argtypes = [C.POINTER(R.View), L.vp, L.vp, L.vp]
    lib.hcs_finish.restype = None
    lib.hcs_forward.argtypes = [C.POINTER(R.View), L.vp, L.vp, L.vp]
    lib.hcs_forward.restype = None
    _lib = lib
    return lib


def build_main(exe, extra=()):
    """the stand-alone program of the host check (its own main, -DHOSTCHECK_COLUMN_SAMPLE_MARGINALS_MAIN) at the path exe"""
    subprocess.check_call(["g++"] + FLAGS + list(extra) + ["-DHOSTCHECK_COLUMN_SAMPLE_MARGINALS_MAIN", "-o", exe, SRC, "-lm"])
    return exe


class MarginalStage(B.BlockStage):
    """BlockStage with a SampleMarginalView beside its views: hist (nbins, M, C, ncol) uint32 and, with_cov, P (M (M + 1) / 2, C, ncol) in
    self.m.  nbins = 0: the marginals are off and nothing of them is called.  h: this module's load()."""

    def __init__(self, h, *args, nbins=0, with_cov=False, **kw):
        super().__init__(h, *args, **kw)
        M, Cn, ncol = self.M, self.C, self.ncol
        self.nbins, self.with_cov = int(nbins), bool(with_cov) and nbins > 0
        self.m = dict(hist=np.zeros((self.nbins, M, Cn, ncol), np.uint32))
        if self.with_cov:
            self.m["P"] = np.zeros((B.tri_size(M), Cn, ncol))
        g = self.marginal = MarginalView()
        g.nbins, g.hist, g.P = self.nbins, L.ptr(self.m["hist"]) if self.nbins else None, L.ptr(self.m["P"]) if self.with_cov else None

    def _g(self):
        return C.byref(self.marginal) if self.nbins else None

    def bins(self, c, l, v):
        v = np.ascontiguousarray(v, F)
        out = np.zeros(v.size, np.int32)
        self.h.hcm_bin(C.byref(self.view), int(c), int(l), self.nbins, v.size, L.ptr(v), L.ptr(out))
        return out

    def accumulate(self):
        """the counts and products of the last sweep, from the state as it lies"""
        if self.nbins:
            self.h.hcm_accumulate(C.byref(self.view), C.byref(self.marginal), self.sweep)

    def accept(self, pv=None):
        super().accept(pv)
        self.accumulate()

    def linear(self, pv0, A, nsweeps):
        self.h.hcm_linear(C.byref(self.view), C.byref(self.block), self._g(), L.ptr(pv0), L.ptr(A), L.ptr(self.pv), self.sweep + 1, int(nsweeps))
        self.sweep += int(nsweeps)

    def take(self, dev, sweep):
        """the device's fetched state (columns_sample_state's dict) in place of the stage's own, at sweep `sweep`"""
        for name in R.STATE:
            self.a[name][...] = dev[name]
        self.sweep = int(sweep)

    def marginal_finish(self, levels=LEVELS):
        """dict(hist (nbins, M, ncol) uint32: pooled; mode (M, ncol); quantiles (len(levels), M, ncol); with_cov: cov (tri, ncol))"""
        lv = np.ascontiguousarray(levels, np.float64)
        pooled = np.zeros((self.nbins, self.M, self.ncol), np.uint32)
        figures = np.zeros((1 + lv.size, self.M, self.ncol))
        out = dict(hist=pooled, mode=figures[0], quantiles=figures[1:])
        if self.with_cov:
            out["cov"] = np.zeros((B.tri_size(self.M), self.ncol))
        self.h.hcm_finish(C.byref(self.view), C.byref(self.marginal), lv.size, L.ptr(lv) if lv.size else None, L.ptr(pooled), L.ptr(figures),
                          L.ptr(out["cov"]) if self.with_cov else None)
        return out

    def marginal_state(self):
        return {n: a.copy() for n, a in self.m.items()}
