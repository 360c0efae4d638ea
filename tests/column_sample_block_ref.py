"""Test infrastructure for the block proposals of the Monte-Carlo depth inversion: the CPU build of
dsurftomo_amd/csrc/column_sample.h with them (tests/hostcheck_column_sample_block.cpp) behind NumPy.  BlockView mirrors the header's
SampleBlockView field by field (load() checks both views' sizes against the library's); BlockStage is column_sample_ref.Stage with the block
state beside it, its proposals and Metropolis tests the header's block ones.  Nothing under dsurftomo_amd/ imports this module."""
import ctypes as C
import os
import subprocess

import numpy as np

import _libs as L
import column_sample_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libhostcheck_column_sample_block.so")
SRC = os.path.join(HERE, "hostcheck_column_sample_block.cpp")
FLAGS = R.FLAGS
F = np.float32
_lib = None

BLOCK_STATE = ("pold_all", "block_counters")


class BlockView(C.Structure):
    _fields_ = [(n, L.vp) for n in ("tri", "r", "flag", "pold_all", "cnt")] + [("block_every", L.i32), ("block_scale", L.f64)]


def tri_size(M):
    return M * (M + 1) // 2


def load():
    global _lib
    if _lib is not None:
        return _lib
    if L._stale(SO, [SRC, R.SRC] + R.HDR):
        subprocess.check_call(["g++"] + FLAGS + ["-shared", "-o", SO, SRC, "-lm"])
    lib = C.CDLL(SO)
    assert lib.hcs_view_bytes() == C.sizeof(R.View), "View does not mirror SampleView"
    assert lib.hcb_block_bytes() == C.sizeof(BlockView), "BlockView does not mirror SampleBlockView"
    lib.hcb_rsqrt.argtypes = [C.c_longlong, L.vp, L.vp]
    lib.hcb_rsqrt.restype = None
    lib.hcb_shape.argtypes = [L.i32] * 4 + [L.vp] * 4 + [L.f32] * 2 + [L.vp] * 4
    lib.hcb_shape.restype = None
    for name in ("hcb_propose", "hcb_accept"):
        getattr(lib, name).argtypes = [C.POINTER(R.View), C.POINTER(BlockView), L.i32]
        getattr(lib, name).restype = None
    lib.hcb_linear.argtypes = [C.POINTER(R.View), C.POINTER(BlockView), L.vp, L.vp, L.vp, L.i32, L.i32]
    lib.hcb_linear.restype = None
    for name in ("hcs_setup",):
        getattr(lib, name).argtypes = [C.POINTER(R.View), L.i32]
        getattr(lib, name).restype = None
    lib.hcs_finish.argtypes = [C.POINTER(R.View), L.vp, L.vp, L.vp]
    lib.hcs_finish.restype = None
    lib.hcs_forward.argtypes = [C.POINTER(R.View), L.vp, L.vp, L.vp]
    lib.hcs_forward.restype = None
    _lib = lib
    return lib


def rsqrt(h, d):
    d = np.ascontiguousarray(d, np.float64)
    out = np.zeros(d.size)
    h.hcb_rsqrt(d.size, L.ptr(d), L.ptr(out))
    return out


def shape(h, nx, ny, obs, wt, pv, S, smooth, damp):
    """the header's shape of every interior column: obs / wt (K, ncol) fp32 (wt may be None), pv (K, ncol), S (M, K, ncol) fp64.  Returns
    dict(tri (M (M + 1) / 2, ncol), r (M, ncol), flag, nused (ncol))."""
    obs = np.ascontiguousarray(obs, F); pv = np.ascontiguousarray(pv, np.float64); S = np.ascontiguousarray(S, np.float64)
    wt = None if wt is None else np.ascontiguousarray(wt, F)
    M, K, ncol = S.shape
    assert ncol == nx * ny and obs.shape == (K, ncol) and pv.shape == (K, ncol)
    out = dict(tri=np.zeros((tri_size(M), ncol)), r=np.zeros((M, ncol)), flag=np.zeros(ncol, np.int32), nused=np.zeros(ncol, np.int32))
    h.hcb_shape(nx, ny, M, K, L.ptr(obs), L.ptr(wt), L.ptr(pv), L.ptr(S), float(smooth), float(damp), L.ptr(out["tri"]), L.ptr(out["r"]), L.ptr(out["flag"]),
                L.ptr(out["nused"]))
    return out


class BlockStage(R.Stage):
    """column_sample_ref.Stage with a SampleBlockView beside its view: shape = dict(tri, r, flag) of every column (None: zeros, every column
    flagged 1 -- for block_every = 0), pold_all (M, C, ncol) fp32 and block_counters (3, C, ncol) in self.a.  h: this module's load()."""

    def __init__(self, h, nx, ny, start, obs, wt, nchains, smooth, step, spread, width, temperature, minvel, maxvel, seed, burn, shape=None, block_every=0,
                 block_scale=1.0):
        super().__init__(h, nx, ny, start, obs, wt, nchains, smooth, step, spread, width, temperature, minvel, maxvel, seed, burn)
        M, Cn, ncol = self.M, self.C, self.ncol
        if shape is None:
            shape = dict(tri=np.zeros((tri_size(M), ncol)), r=np.zeros((M, ncol)), flag=np.ones(ncol, np.int32))
        self.tri = np.ascontiguousarray(shape["tri"], np.float64); self.r = np.ascontiguousarray(shape["r"], np.float64)
        self.sflag = np.ascontiguousarray(shape["flag"], np.int32)
        assert self.tri.shape == (tri_size(M), ncol) and self.r.shape == (M, ncol) and self.sflag.shape == (ncol,)
        self.a["pold_all"] = np.zeros((M, Cn, ncol), F); self.a["block_counters"] = np.zeros((3, Cn, ncol), np.int32)
        b = self.block = BlockView()
        b.tri, b.r, b.flag, b.pold_all, b.cnt = L.ptr(self.tri), L.ptr(self.r), L.ptr(self.sflag), L.ptr(self.a["pold_all"]), L.ptr(self.a["block_counters"])
        b.block_every, b.block_scale = int(block_every), float(block_scale)

    def propose(self):
        self.sweep += 1
        self.h.hcb_propose(C.byref(self.view), C.byref(self.block), self.sweep)

    def accept(self, pv=None):
        if pv is not None:
            self.pv[...] = np.asarray(pv).reshape(self.pv.shape)
        self.h.hcb_accept(C.byref(self.view), C.byref(self.block), self.sweep)

    def linear(self, pv0, A, nsweeps):
        self.h.hcb_linear(C.byref(self.view), C.byref(self.block), L.ptr(pv0), L.ptr(A), L.ptr(self.pv), self.sweep + 1, int(nsweeps))
        self.sweep += int(nsweeps)

    def state(self):
        return {n: self.a[n].copy() for n in R.STATE + BLOCK_STATE}
