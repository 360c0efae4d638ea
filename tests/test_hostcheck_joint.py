"""Where the Laplacian rows of the joint Vs | gc | gs system lie (dsurftomo_amd/csrc/joint_system.h), on the CPU through
tests/hostcheck_joint.cpp: the closed form of an unknown's first entry, the entries per block, and every entry's column and value must be
those of the Python loop analyses.azimuthal.laplacian_rows, for three blocks with two different weights, value bits included.  Grids
without an interior unknown are where a closed form goes wrong."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _libs as L
from dsurftomo_amd import invert

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libhostcheck_joint.so")
I64 = C.c_longlong
GRIDS = [(1, 1, 1), (2, 5, 3), (3, 3, 3), (8, 7, 3), (5, 4, 6), (3, 1, 4), (4, 4, 2), (6, 5, 4), (1, 4, 5), (2, 2, 2), (3, 3, 1)]


@pytest.fixture(scope="module")
def h():
    src = os.path.join(HERE, "hostcheck_joint.cpp")
    hdr = [os.path.join(L.ROOT, "dsurftomo_amd", "csrc", "joint_system.h")]
    if L._stale(SO, [src] + hdr):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-msse2",
                               "-mfpmath=sse", "-shared", "-o", SO, src, "-lm"])
    lib = C.CDLL(SO)
    lib.hcj_block_entries.restype = I64
    lib.hcj_block_entries.argtypes = [L.i32] * 3
    lib.hcj_block.restype = I64
    lib.hcj_block.argtypes = [L.i32] * 3 + [L.f32, L.i32, L.i32, I64] + [L.vp] * 5
    return lib


def block(h, grid, w, row0, col0):
    nvx, nvz, nl = grid
    maxvp = nvx * nvz * nl
    cap = int(h.hcj_block_entries(nvx, nvz, nl))
    first = np.full(maxvp, -1, np.int64); count = np.zeros(maxvp, np.int32)
    rw = np.full(cap, np.nan, np.float32); row = np.full(cap, -1, np.int32); col = np.full(cap, -1, np.int32)
    outside = h.hcj_block(nvx, nvz, nl, w, row0, col0, cap, L.ptr(first), L.ptr(count), L.ptr(rw), L.ptr(row), L.ptr(col))
    return dict(cap=cap, first=first, count=count, rw=rw, row=row, col=col, outside=int(outside))


@pytest.mark.parametrize("grid", GRIDS)
def test_blocks_equal_the_python_loop(h, grid):
    """three blocks at row0 = dall + B maxvp, col0 = B maxvp, weight0 on block 0 and another weight on blocks 1 and 2"""
    nvx, nvz, nl = grid
    maxvp, dall = nvx * nvz * nl, 37
    w0, wa = np.float32(2.0), np.float32(0.05)
    for B in range(3):
        w = w0 if B == 0 else wa
        want_rw, want_row, want_col = invert.laplacian_rows(nvx, nvz, nl, w, dall + B * maxvp, B * maxvp)
        got = block(h, grid, w, dall + B * maxvp, B * maxvp)
        assert got["outside"] == 0
        assert got["cap"] == want_rw.size
        # the rows are written in (k, j, i) order, one after the other: a row's first entry is where its number first appears
        want_first = np.searchsorted(want_row, dall + B * maxvp + 1 + np.arange(maxvp))
        assert (got["first"] == want_first).all()
        assert (got["count"] == np.bincount(want_row - (dall + B * maxvp + 1), minlength=maxvp)).all()
        assert (got["rw"].view(np.uint32) == want_rw.view(np.uint32)).all()
        assert (got["row"] == want_row).all() and (got["col"] == want_col).all()


def test_the_grids_cover_both_kinds():
    """at least one grid with all of nvx, nvz, nl >= 4, and several without an interior unknown"""
    interior = [max(a - 2, 0) * max(b - 2, 0) * max(c - 2, 0) for a, b, c in GRIDS]
    assert any(min(g) >= 4 for g in GRIDS) and sum(1 for v in interior if v == 0) >= 4 and max(interior) >= 24


def test_awkward_weights_are_one_rounded_product(h):
    """weights whose products with 2, 6 and -1 round: the stored values are fl(c * w), the reference's 2.0f * w, 6.0f * w, -1.0f * w"""
    f = np.float32
    for w in (f(0.1), f(1.0 / 3.0), f(1e-30), f(3.4e37), f(0.0)):
        want = invert.laplacian_rows(5, 4, 6, w, 10, 0)[0]
        got = block(h, (5, 4, 6), w, 10, 0)["rw"]
        with np.errstate(over="ignore"):
            assert (got.view(np.uint32) == want.view(np.uint32)).all()
