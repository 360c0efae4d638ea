"""The placement rules of the radial system (csrc/radial_system.h) on the CPU, through
tests/hostcheck_radial_system.cpp: every position, row, column and coefficient bit of what k_radial_system writes below the data rows must
be the NumPy twin's (dsurftomo_amd.radial.radial_system), whose rows come from explicit loops; the node of every unknown must be
dsa_model_update's.  Grids with no, one and many interior unknowns, nl = 1, 2, 3 and 5, aniso 0 and 0.3."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _libs as L
from dsurftomo_amd import radial

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck_radial_system.cpp")
SO = os.path.join(HERE, "libhostcheck_radial_system.so")
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-msse2", "-mfpmath=sse"]
F = np.float32

# (nvx, nvz, nl): interior unknowns 0 (a dimension below 3, or nl below 3), 1, many
GRIDS = [(1, 1, 1), (2, 2, 2), (4, 5, 1), (5, 4, 2), (3, 3, 3), (8, 7, 3), (6, 3, 5), (3, 9, 5), (5, 6, 5)]


def load():
    hdr = [os.path.join(L.ROOT, "dsurftomo_amd", "csrc", n) for n in ("radial_system.h", "joint_system.h")]
    if L._stale(SO, [SRC] + hdr):
        subprocess.check_call(["g++"] + FLAGS + ["-shared", "-o", SO, SRC])
    h = C.CDLL(SO)
    for fn, args in (("hcr_entries", [L.i32] * 3), ("hcr_rows", [L.i32] * 3 + [C.c_longlong]), ("hcr_columns", [L.i32] * 3), ("hcr_node", [L.i32] * 2 + [C.c_longlong])):
        getattr(h, fn).argtypes = args
        getattr(h, fn).restype = C.c_longlong
    h.hcr_system.argtypes = [L.i32] * 4 + [L.f32] * 3 + [C.c_longlong] + [L.vp] * 4
    h.hcr_system.restype = C.c_longlong
    return h


@pytest.fixture(scope="module")
def h():
    return load()


def interior(nvx, nvz, nl):
    return max(nvx - 2, 0) * max(nvz - 2, 0) * max(nl - 2, 0)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.mark.parametrize("aniso", [0.0, 0.3])
@pytest.mark.parametrize("grid", GRIDS)
def test_rows_below_the_data_equal_the_twin(h, grid, aniso):
    nvx, nvz, nl = grid
    nx, ny, nz = nvx + 2, nvz + 2, nl + 1
    maxvp = nvx * nvz * nl
    dall, w0, wh = 13, F(2.0), F(0.7)
    rng = np.random.default_rng(nvx * 100 + nvz * 10 + nl)
    vsv = (3.0 + rng.random((nz, ny, nx))).astype(F); vsh = (vsv * F(1.04)).astype(F)
    # a few made-up data entries in front, so that the twin's rows below them start where the device's do
    nd = 9
    S = radial.radial_system(nx, ny, nz, rng.random(nd).astype(F), rng.integers(1, dall + 1, nd), rng.integers(1, 2 * maxvp + 1, nd),
                             rng.standard_normal(dall).astype(F), np.ones(dall, F), w0, wh, aniso, vsv, vsh)
    n = h.hcr_entries(nvx, nvz, nl)
    assert n == 2 * (maxvp + 6 * interior(nvx, nvz, nl)) + 2 * maxvp == S["rw"].size - nd
    assert h.hcr_rows(nvx, nvz, nl, dall) == S["m"] == dall + 3 * maxvp and h.hcr_columns(nvx, nvz, nl) == S["n"] == 2 * maxvp
    rw = np.full(n, np.nan, F); row = np.zeros(n, np.int32); col = np.zeros(n, np.int32); hits = np.zeros(n, np.int32)
    assert h.hcr_system(nvx, nvz, nl, dall, w0, wh, F(aniso), n, L.ptr(rw), L.ptr(row), L.ptr(col), L.ptr(hits)) == 0
    assert (hits == 1).all()
    assert (bits(rw) == bits(S["rw"][nd:])).all() and (row == S["row"][nd:]).all() and (col == S["col"][nd:]).all()
    # the tie rows: two entries each, -aniso on the Vsv column and +aniso on the Vsh column of the same cell, also at aniso = 0
    tie = row > dall + 2 * maxvp
    assert tie.sum() == 2 * maxvp and (row[tie].reshape(-1, 2) == (dall + 2 * maxvp + 1 + np.arange(maxvp))[:, None]).all()
    assert (col[tie].reshape(-1, 2) == np.stack([1 + np.arange(maxvp), maxvp + 1 + np.arange(maxvp)], axis=1)).all()
    assert (bits(rw[tie].reshape(-1, 2)) == bits(np.array([F(0.0) - F(aniso), F(aniso)], F))).all()
    # one entry short: the entry outside is counted and nothing is written beyond the arrays
    assert h.hcr_system(nvx, nvz, nl, dall, w0, wh, F(aniso), n - 1, L.ptr(rw), L.ptr(row), L.ptr(col), L.ptr(hits)) == 1


@pytest.mark.parametrize("grid", GRIDS)
def test_nodes_are_the_model_updates(h, grid):
    """the node of unknown index is the element dsa_model_update steps with dv[index]: (k, j + 1, i + 1) of a model (nz, ny, nx)"""
    nvx, nvz, nl = grid
    nx, ny, nz = nvx + 2, nvz + 2, nl + 1
    want = radial.unknown_nodes(nx, ny, nz)
    got = np.array([h.hcr_node(nvx, nvz, i) for i in range(nvx * nvz * nl)])
    assert (got == want).all()
    k, r = np.divmod(np.arange(nvx * nvz * nl), nvx * nvz)
    j, i = np.divmod(r, nvx)
    assert (want == (k * ny + j + 1) * nx + i + 1).all() and want.max() < (nz - 1) * ny * nx


def test_the_stand_alone_program_runs(tmp_path):
    """the same file as a program with its own main (what a sanitizer build runs): every entry written once, inside the system"""
    exe = str(tmp_path / "hostcheck_radial_system")
    subprocess.check_call(["g++"] + [f for f in FLAGS if f != "-fPIC"] + ["-DHOSTCHECK_RADIAL_SYSTEM_MAIN", "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
