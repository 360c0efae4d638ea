"""The azimuthal step's host side (dsurftomo_amd.invert: azimuthal_system, azimuthal_weights, the axis and strength formulas, the Azim.dat
file, the argument checks).  No GPU: the one library call here, dsa_iteration_system, is host code."""
import ctypes as C

import numpy as np
import pytest

from dsurftomo_amd import invert

F = np.float32
GRID = dict(nx=7, ny=6, nz=4)             # 5 x 4 x 3 unknowns per block


def dense_laplacian(nvx, nvz, nl, w):
    """the reference's first-difference Laplacian as a dense matrix, from 3-D index arithmetic: a vertex on a face of the block has 2 w on
    the diagonal; an inner one 6 w and -w towards its six neighbours"""
    n = nvx * nvz * nl
    D = np.zeros((n, n), np.float32)
    idx = lambda k, j, i: np.ravel_multi_index((k, j, i), (nl, nvz, nvx))
    for k in range(nl):
        for j in range(nvz):
            for i in range(nvx):
                r = idx(k, j, i)
                if min(i, j, k) == 0 or i == nvx - 1 or j == nvz - 1 or k == nl - 1:
                    D[r, r] = F(2) * F(w)
                    continue
                D[r, r] = F(6) * F(w)
                for dk, dj, di in ((0, 0, 1), (0, 0, -1), (0, 1, 0), (0, -1, 0), (1, 0, 0), (-1, 0, 0)):
                    D[r, idx(k + dk, j + dj, i + di)] = -F(w)
    return D


def test_joint_system_against_a_dense_construction():
    nvx, nvz, nl = 5, 4, 3
    maxvp, dall = nvx * nvz * nl, 9
    c = dict(GRID, ndata=dall)
    rng = np.random.default_rng(7)
    nnz = 70
    pairs = np.sort(rng.choice(dall * 3 * maxvp, nnz, replace=False))    # no duplicate (row, col); rows in order, like the rays' data
    row = (pairs // (3 * maxvp)).astype(np.int32) + 1
    col = (pairs % (3 * maxvp)).astype(np.int32) + 1
    rw = rng.standard_normal(nnz).astype(F)
    res = rng.standard_normal(dall).astype(F)
    w = np.array([1, 0, 1, 1, 0, 1, 1, 1, 1], F)
    w0, wa = 1.7, 0.45
    S = invert.azimuthal_system(c, rw, row, col, res, w, w0, wa)
    assert (S["m"], S["n"]) == (dall + 3 * maxvp, 3 * maxvp)
    assert S["rw"].dtype == F and S["row"].dtype == np.int32 and S["col"].dtype == np.int32 and S["b"].dtype == F
    assert S["rw"].size == S["row"].size == S["col"].size
    # the data entries stay first and in order, scaled by their datum's weight
    assert (S["row"][:nnz] == row).all() and (S["col"][:nnz] == col).all()
    assert (S["rw"][:nnz].view(np.uint32) == (rw * w[row - 1]).view(np.uint32)).all()
    # rows are non-decreasing: block B's Laplacian rows at dall + B maxvp + index, one row per unknown
    assert (np.diff(S["row"]) >= 0).all() and S["row"].max() == S["m"]
    A = np.zeros((S["m"], S["n"]), np.float32)
    assert len(set(zip(S["row"].tolist(), S["col"].tolist()))) == S["rw"].size
    A[S["row"] - 1, S["col"] - 1] = S["rw"]
    want = np.zeros_like(A)
    want[row - 1, col - 1] = rw * w[row - 1]
    for B, wt in enumerate((w0, wa, wa)):
        a = dall + B * maxvp
        want[a:a + maxvp, B * maxvp:(B + 1) * maxvp] = dense_laplacian(nvx, nvz, nl, wt)
    assert (A.view(np.uint32) == want.view(np.uint32)).all()
    assert (S["b"][:dall].view(np.uint32) == (res * w).view(np.uint32)).all() and not S["b"][dall:].any()
    # the Vs block's Laplacian rows are dsa_iteration_system's, entry for entry
    lap = invert.laplacian_rows(nvx, nvz, nl, w0, dall, 0)
    assert lap[0].size == 7 * (nvx - 2) * (nvz - 2) * (nl - 2) + (maxvp - (nvx - 2) * (nvz - 2) * (nl - 2))


def test_laplacian_rows_equal_the_iteration_systems():
    """dsa_iteration_system (host code) appends the same rows below the data rows: values bit for bit, rows and columns"""
    lib = invert.bind(invert.load_library())
    nx, ny, nz, dall = GRID["nx"], GRID["ny"], GRID["nz"], 8
    maxvp = (nx - 2) * (ny - 2) * (nz - 1)
    cap = 4096
    rw = np.zeros(cap, F); col = np.zeros(cap, np.int32); iw = np.zeros(2 * cap + 1, np.int32)
    rw[:3] = [1, 2, 3]; iw[1:4] = [1, 4, 8]; col[:3] = [5, 17, 60]
    obst = np.linspace(0.0, 1.0, dall).astype(F); dsyn = np.zeros(dall, F)
    cbst = np.zeros(dall + maxvp, F); dw = np.zeros(dall, F); norm = np.zeros(maxvp, F); dws = np.zeros(2, F)
    m, nar = C.c_int(0), C.c_longlong(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.dsa_iteration_system(nx, ny, nz, dall, 3, cap, p(rw), p(iw), p(col), p(obst), p(dsyn), F(1.5), F(2.25), p(cbst), p(dw), p(norm),
                                    C.byref(m), C.byref(nar), p(dws)) == 0
    n = nar.value
    got = invert.laplacian_rows(nx - 2, ny - 2, nz - 1, 2.25, dall, 0)
    assert n - 3 == got[0].size
    assert (rw[3:n].view(np.uint32) == got[0].view(np.uint32)).all() and (iw[4:n + 1] == got[1]).all() and (col[3:n] == got[2]).all()


@pytest.mark.parametrize("n,threshold0,seed", [(8, 1.5, 1), (37, 1.0, 2), (200, 2.5, 3), (1001, 0.5, 4), (64, 1.5, 5)])
def test_weight_rule_equals_the_iteration_systems(n, threshold0, seed):
    """azimuthal_weights against dsa_iteration_system's datweight on the same residuals (ties among them included)"""
    lib = invert.bind(invert.load_library())
    rng = np.random.default_rng(seed)
    obst = rng.standard_normal(n).astype(F)
    if seed == 5:
        obst = np.round(obst * 2).astype(F) / 2                            # many equal residuals
    dsyn = (0.1 * rng.standard_normal(n)).astype(F)
    nx, ny, nz = 3, 3, 2
    cap = 64
    rw = np.zeros(cap, F); col = np.ones(cap, np.int32); iw = np.ones(2 * cap + 1, np.int32)
    cbst = np.zeros(n + 1, F); dw = np.zeros(n, F); norm = np.zeros(1, F); dws = np.zeros(2, F)
    m, nar = C.c_int(0), C.c_longlong(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.dsa_iteration_system(nx, ny, nz, n, 0, cap, p(rw), p(iw), p(col), p(obst), p(dsyn), F(threshold0), F(1.0), p(cbst), p(dw), p(norm),
                                    C.byref(m), C.byref(nar), p(dws)) == 0
    got = invert.azimuthal_weights((obst - dsyn).astype(F), threshold0)
    assert got.dtype == F and (got == dw).all()
    assert 0 < got.sum() <= n
    with pytest.raises(ValueError):
        invert.azimuthal_weights(np.zeros(3, F), 1.5)


def test_axis_and_strength_at_the_four_quadrants():
    g = 0.04                                                               # 4 % : strength 2 % of Vs
    for axis_deg in (30.0, 75.0, -30.0, -75.0, 0.0, 45.0, 90.0, -45.0):   # 2 psi in each quadrant, and on the axes between them
        gc, gs = g * np.cos(np.radians(2 * axis_deg)), g * np.sin(np.radians(2 * axis_deg))
        assert abs(invert.azimuthal_axis(gc, gs) - axis_deg) < 1e-10
        assert abs(invert.azimuthal_strength(gc, gs) - 50.0 * g) < 1e-12
    # the fast axis is where c(psi) = c0 + A1 cos 2psi + A2 sin 2psi peaks
    psi = np.radians(np.arange(-90.0, 90.0, 0.25))
    for gc, gs in ((0.01, 0.03), (-0.02, 0.01), (-0.01, -0.03), (0.03, -0.02)):
        peak = np.degrees(psi[np.argmax(gc * np.cos(2 * psi) + gs * np.sin(2 * psi))])
        assert abs(invert.azimuthal_axis(gc, gs) - peak) <= 0.25
    out = invert.azimuthal_axis(np.array([1.0, -1.0]), np.array([0.0, 1e-300]))
    assert out.shape == (2,) and out[0] == 0.0 and abs(out[1] - 90.0) < 1e-9 and invert.azimuthal_strength(0.0, 0.0) == 0.0


def test_azim_file_round_trips(tmp_path):
    nx, ny, nz = GRID["nx"], GRID["ny"], GRID["nz"]
    c = dict(GRID, goxd=F(24.0), gozd=F(121.0), dvxd=F(0.05), dvzd=F(0.05), depz=np.array([0.0, 3.0, 7.0, 12.0], F))
    rng = np.random.default_rng(3)
    vsf = np.asfortranarray((2.5 + rng.random((nx, ny, nz))).astype(F))
    maxvp = (nx - 2) * (ny - 2) * (nz - 1)
    gc, gs = (0.05 * rng.standard_normal(maxvp)).astype(F), (0.05 * rng.standard_normal(maxvp)).astype(F)
    path = tmp_path / "DSurfTomo.inAzim.dat"
    invert.write_azimuthal(str(path), c, vsf, gc, gs)
    rows = path.read_text().splitlines()
    assert len(rows) == maxvp and all(len(r.split()) == 8 for r in rows)
    a = invert.read_azimuthal(str(path))
    assert np.abs(a["gc"] - gc).max() <= 0.5e-8 + 1e-12 and np.abs(a["gs"] - gs).max() <= 0.5e-8 + 1e-12
    assert np.abs(a["strength"] - invert.azimuthal_strength(gc, gs)).max() <= 0.5e-5 + 1e-12
    assert np.abs(a["axis"] - invert.azimuthal_axis(gc, gs)).max() <= 0.5e-5 + 1e-12
    # the first four columns are a model file's: the same text as write_model's lines
    model = tmp_path / "model"
    invert.write_model(str(model), c, vsf)
    assert [r[:40] for r in rows] == model.read_text().splitlines()
    want_vs = vsf[1:-1, 1:-1, :-1].transpose(2, 1, 0).reshape(-1)
    assert np.abs(a["vs"] - want_vs).max() <= 0.5e-5 + 1e-7 and (a["depth"] == np.repeat(c["depz"][:nz - 1], (nx - 2) * (ny - 2))).all()
    path.write_text("1 2 3\n")
    with pytest.raises(ValueError):
        invert.read_azimuthal(str(path))


def test_system_builder_rejects_bad_arguments():
    c = dict(GRID, ndata=4)
    maxvp = 60
    ok = dict(rw=np.ones(2, F), row=np.array([1, 4], np.int32), col=np.array([1, 3 * maxvp], np.int32), res=np.zeros(4, F), datweight=np.ones(4, F),
              weight0=1.0, weight_azi=1.0)
    invert.azimuthal_system(c, **ok)
    for bad in (dict(row=np.array([1, 5], np.int32)), dict(row=np.array([0, 1], np.int32)), dict(col=np.array([1, 3 * maxvp + 1], np.int32)),
                dict(col=np.array([0, 1], np.int32)), dict(rw=np.ones(3, F)), dict(res=np.zeros(5, F)), dict(datweight=np.ones(3, F)),
                dict(weight0=-1.0), dict(weight_azi=float("nan"))):
        with pytest.raises(ValueError):
            invert.azimuthal_system(c, **dict(ok, **bad))


@pytest.mark.parametrize("argv", [["--azimuthal-weight", "1"], ["--azimuthal-damp", "1"], ["--azimuthal", "--azimuthal-weight", "-1"],
                                  ["--azimuthal", "--azimuthal-damp", "nan"], ["--azimuthal", "--azimuthal-weight", "x"]])
def test_cli_rejects_bad_azimuthal_arguments_before_the_library(monkeypatch, tmp_path, argv):
    def refuse():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(invert, "load_library", refuse)
    with pytest.raises(SystemExit) as exc:
        invert.main([str(tmp_path)] + argv)
    assert exc.value.code == 2


@pytest.mark.parametrize("kw", [dict(azimuthal_weight=1.0), dict(azimuthal_damp=0.5), dict(azimuthal=True, azimuthal_weight=-2.0),
                                dict(azimuthal=True, azimuthal_damp=float("inf"))])
def test_run_rejects_bad_azimuthal_arguments_before_the_library(monkeypatch, tmp_path, kw):
    def refuse():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(invert, "load_library", refuse)
    with pytest.raises(ValueError):
        invert.run(str(tmp_path), **kw)
