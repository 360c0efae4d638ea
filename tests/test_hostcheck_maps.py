"""Where the 2-D Laplacian rows of the per-period map system lie (dsurftomo_amd/csrc/map_system.h), on the CPU through
tests/hostcheck_maps.cpp: the closed form of an unknown's first entry, the entries per plane, and every entry's row, column, coefficient
and order must be those of the Python loop maps.laplacian_rows_2d, value bits included.  Planes without an interior vertex are where a
closed form goes wrong."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _libs as L
from dsurftomo_amd import maps

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libhostcheck_maps.so")
I64 = C.c_longlong
SHAPES = [(1, 1, 1), (2, 5, 2), (3, 3, 1), (3, 4, 3), (8, 7, 6)]          # (nvx, nvz, planes)


@pytest.fixture(scope="module")
def h():
    src = os.path.join(HERE, "hostcheck_maps.cpp")
    hdr = [os.path.join(L.ROOT, "dsurftomo_amd", "csrc", "map_system.h")]
    if L._stale(SO, [src] + hdr):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-msse2",
                               "-mfpmath=sse", "-shared", "-o", SO, src, "-lm"])
    lib = C.CDLL(SO)
    lib.hcm_plane_entries.restype = I64
    lib.hcm_plane_entries.argtypes = [L.i32] * 2
    lib.hcm_rows.restype = I64
    lib.hcm_rows.argtypes = [L.i32] * 4 + [L.f32, L.f32, L.i32, I64] + [L.vp] * 5
    return lib


def rows(h, shape, planes0, w0, wa, row0):
    nvx, nvz, planes = shape
    n = nvx * nvz * planes
    cap = planes * int(h.hcm_plane_entries(nvx, nvz))
    first = np.full(n, -1, np.int64); count = np.zeros(n, np.int32)
    rw = np.full(cap, np.nan, np.float32); row = np.full(cap, -1, np.int32); col = np.full(cap, -1, np.int32)
    outside = h.hcm_rows(nvx, nvz, planes, planes0, w0, wa, row0, cap, L.ptr(first), L.ptr(count), L.ptr(rw), L.ptr(row), L.ptr(col))
    return dict(cap=cap, first=first, count=count, rw=rw, row=row, col=col, outside=int(outside))


@pytest.mark.parametrize("shape", SHAPES)
def test_rows_equal_the_python_loop(h, shape):
    """the planes as one block (planes0 = planes) and, where there are three or more, as three blocks with another weight on the last two"""
    nvx, nvz, planes = shape
    n, dall = nvx * nvz * planes, 37
    w0, wa = np.float32(2.0), np.float32(0.05)
    for planes0 in sorted({planes, planes // 3 if planes % 3 == 0 else planes}):
        w = np.where(np.arange(planes) < planes0, w0, wa).astype(np.float32)
        want_rw, want_row, want_col = maps.laplacian_rows_2d(nvx, nvz, planes, w, dall)
        got = rows(h, shape, planes0, w0, wa, dall)
        assert got["outside"] == 0
        assert got["cap"] == want_rw.size
        want_first = np.searchsorted(want_row, dall + 1 + np.arange(n))
        assert (got["first"] == want_first).all()
        assert (got["count"] == np.bincount(want_row - (dall + 1), minlength=n)).all()
        assert (got["rw"].view(np.uint32) == want_rw.view(np.uint32)).all()
        assert (got["row"] == want_row).all() and (got["col"] == want_col).all()
        # planes never couple: every column of a row lies in the row's own plane
        layer = nvx * nvz
        assert ((got["col"] - 1) // layer == (got["row"] - dall - 1) // layer).all()


def test_the_shapes_cover_both_kinds():
    """planes with no interior vertex, with exactly one, and several planes with many"""
    interior = [max(a - 2, 0) * max(b - 2, 0) for a, b, _ in SHAPES]
    assert 0 in interior and 1 in interior and max(interior) >= 30 and max(p for _, _, p in SHAPES) >= 6


def test_awkward_weights_are_one_rounded_product(h):
    f = np.float32
    for w in (f(0.1), f(1.0 / 3.0), f(1e-30), f(3.4e37), f(0.0)):
        want = maps.laplacian_rows_2d(5, 4, 3, w, 10)[0]
        got = rows(h, (5, 4, 3), 3, w, w, 10)["rw"]
        with np.errstate(over="ignore"):
            assert (got.view(np.uint32) == want.view(np.uint32)).all()
