"""The host side of the per-period map inversion (dsurftomo_amd/maps.py), no GPU: the plan against the input file's
own order, the NumPy twins of the regulariser and of the update rule, the file's round trip, the command line's refusals, and the new
symbols in the header, the binding and the built library."""
import os
import re

import numpy as np
import pytest

import _libs as L
from dsurftomo_amd import io, maps

F = np.float32
NEW = ("dsa_solve_rows_maps", "dsa_iteration_system_maps_device", "dsa_update_maps", "dsa_get_maps")


@pytest.fixture(scope="module")
def taipei():
    return io.load()


def test_plan_is_the_dropins_unit_order(taipei):
    """one unit per (period slot, source), slot outer; the map of a unit is its slot; the data run on in file order, which is the drop-in's
    data order: the distance of every datum from the plan's own coordinates is the one io.load computed line by line, bit for bit"""
    c = taipei
    u = maps.period_plan(c)
    nunits = int(np.sum(c["nsrcsurf1"]))
    assert u["map_index"].size == nunits == u["nrec"].size and u["nmaps"] == c["kmax"] == len(maps.period_list(c))
    assert (u["map_index"] == np.repeat(np.arange(c["kmax"]), c["nsrcsurf1"])).all()
    assert (u["mode"] == 3).all()
    assert u["ndata"] == c["ndata"] == int(u["nrec"].sum()) == u["rcx"].size
    assert (u["data_first"] == np.concatenate([[0], np.cumsum(u["nrec"])[:-1]])).all()
    # every unit is a source of the file: its period and type are those of its slot
    per = maps.period_list(c)
    k = 0
    for slot in range(c["kmax"]):
        for s in range(int(c["nsrcsurf1"][slot])):
            wave, kind, _ = per[slot]
            assert c["wavetype"][s, slot] == wave and c["igrt"][s, slot] == kind
            assert u["scx"][k] == c["scxf"][s, slot] and u["nrec"][k] == c["nrc1"][s, slot]
            k += 1
    dist = np.zeros(u["ndata"], F)
    for k in range(nunits):
        for q in range(u["data_first"][k], u["data_first"][k] + u["nrec"][k]):
            dist[q] = io.delsph(u["scx"][k], u["scz"][k], u["rcx"][q], u["rcz"][q])
    assert (dist.view(np.uint32) == c["dist"].view(np.uint32)).all()
    dm = maps.datum_maps(u)
    assert (np.diff(dm) >= 0).all() and dm[0] == 0 and dm[-1] == c["kmax"] - 1


def test_period_order(taipei):
    c = dict(taipei, tRc=np.array([4.0, 6.0]), tRg=np.array([5.0]), tLc=np.zeros(0), tLg=np.array([8.0]))
    assert maps.period_list(c) == [(2, 0, 4.0), (2, 0, 6.0), (2, 1, 5.0), (1, 1, 8.0)]


def test_laplacian_2d_against_a_dense_construction():
    """D^T-free statement: row of an interior unknown sums to zero with 4 on the diagonal; an edge row is 2 on the diagonal; nothing
    crosses a plane"""
    nvx, nvz, planes = 5, 4, 3
    layer = nvx * nvz
    w = np.array([2.0, 0.5, 0.5], F)
    rw, row, col = maps.laplacian_rows_2d(nvx, nvz, planes, w, 9)
    A = np.zeros((planes * layer, planes * layer))
    A[row - 10, col - 1] = rw
    for idx in range(planes * layer):
        p, r = divmod(idx, layer)
        j, i = divmod(r, nvx)
        inside = 0 < i < nvx - 1 and 0 < j < nvz - 1
        want = np.zeros(planes * layer)
        if inside:
            want[idx] = 4 * w[p]
            for d in (-1, 1, -nvx, nvx):
                want[idx + d] = -w[p]
        else:
            want[idx] = 2 * w[p]
        assert (A[idx] == want).all(), idx
    assert rw.size == planes * (layer + 4 * (nvx - 2) * (nvz - 2))
    assert (np.diff(row) >= 0).all()


def test_map_system_layout():
    nx, ny, nmaps, nblocks, dall = 6, 5, 2, 3, 8
    layer = 12
    n = nblocks * nmaps * layer
    rw = np.array([0.5, -0.25, 2.0], F); row = np.array([1, 3, 8], np.int32); col = np.array([1, layer + 2, n], np.int32)
    res = np.arange(dall, dtype=F) - 3; dw = np.array([1, 1, 0, 1, 1, 1, 1, 1], F)
    S = maps.map_system(nx, ny, nmaps, nblocks, rw, row, col, res, dw, 2.0, 0.05)
    assert S["m"] == dall + n and S["n"] == n and (S["b"][:dall] == res * dw).all() and not S["b"][dall:].any()
    assert (S["rw"][:3] == np.array([0.5, 0.0, 2.0], F)).all()
    reg_row, reg_rw, reg_col = S["row"][3:], S["rw"][3:], S["col"][3:]
    assert reg_row.min() == dall + 1 and reg_row.max() == dall + n
    blk = (reg_col - 1) // (nmaps * layer)
    assert set(np.abs(reg_rw[blk == 0]).tolist()) == {4.0, 8.0, 2.0} and set(np.abs(reg_rw[blk > 0]).tolist()) == {F(0.1).item(), F(0.2).item(), F(0.05).item()}
    with pytest.raises(ValueError):
        maps.map_system(nx, ny, nmaps, nblocks, rw, row, np.array([1, 2, n + 1], np.int32), res, dw, 2.0, 0.05)


def test_update_twin_clamps_ring_and_nan():
    nx, ny = 5, 4
    v = (3.0 + 0.01 * np.arange(2 * nx * ny, dtype=F)).reshape(2, nx * ny)
    dv = np.zeros((2, 6), F)
    dv[0] = [0.1, 0.9, -0.9, 0.5, -0.5, np.nan]
    dv[1] = [0.3, -0.3, 0.0, 0.49999, -0.2, 0.2]
    out = maps.update_maps_twin(v, dv, 0.5, 2.9, 3.2, nx, ny)
    a, b = v.reshape(2, ny, nx), out.reshape(2, ny, nx)
    ring = np.ones((ny, nx), bool); ring[1:-1, 1:-1] = False
    assert (a[:, ring].view(np.uint32) == b[:, ring].view(np.uint32)).all()
    inner0 = b[0, 1:-1, 1:-1].ravel()
    base0 = a[0, 1:-1, 1:-1].ravel()
    assert inner0[0] == F(base0[0] + F(0.1)) and inner0[1] == F(3.2) and inner0[2] == F(2.9)       # +0.9 -> +0.5 -> maxvel; -0.9 -> -0.5 -> minvel
    assert inner0[3] == min(F(base0[3] + F(0.5)), F(3.2)) and inner0[4] == max(F(base0[4] - F(0.5)), F(2.9))
    assert np.isnan(inner0[5]) and np.isfinite(np.delete(b.ravel(), np.flatnonzero(np.isnan(b.ravel())))).all()
    assert (b[1, 1:-1, 1:-1] <= F(3.2)).all() and (b[1, 1:-1, 1:-1] >= F(2.9)).all()
    assert (v.reshape(2, ny, nx) == a).all()                                                        # the input is not modified


@pytest.mark.parametrize("azimuthal", [False, True])
def test_maps_file_round_trips(tmp_path, taipei, azimuthal):
    c = dict(taipei, nx=6, ny=5, tRc=np.array([4.0, 6.5]), tRg=np.array([5.0]), tLc=np.zeros(0), tLg=np.zeros(0))
    rng = np.random.default_rng(4)
    nm, layer = 3, 12
    velv = (3.0 + rng.random((nm, 30))).astype(F)
    norm = rng.random(nm * layer * (3 if azimuthal else 1)).astype(F)
    a1 = (0.05 * rng.standard_normal((nm, layer))).astype(F) if azimuthal else None
    a2 = (0.05 * rng.standard_normal((nm, layer))).astype(F) if azimuthal else None
    path = str(tmp_path / "Maps.dat")
    maps.write_maps(path, c, velv, norm, a1, a2)
    rows = maps.read_maps(path)
    assert len(rows) == nm * layer
    inner = velv.reshape(nm, 5, 6)[:, 1:-1, 1:-1].reshape(nm, layer)
    assert [r["c0"] for r in rows] == inner.ravel().astype(np.float64).tolist()
    assert [r["dws"] for r in rows] == norm[:nm * layer].astype(np.float64).tolist()
    assert [(r["wave"], r["kind"], r["period"]) for r in rows[::layer]] == [(2, 0, 4.0), (2, 0, 6.5), (2, 1, 5.0)]
    assert rows[1]["lat"] < rows[0]["lat"] and rows[1]["lon"] == rows[0]["lon"] and rows[4]["lon"] > rows[0]["lon"]     # latitude index fastest
    if azimuthal:
        assert [r["a1"] for r in rows] == a1.ravel().astype(np.float64).tolist() and [r["a2"] for r in rows] == a2.ravel().astype(np.float64).tolist()
        k = 7
        assert rows[k]["strength"] == pytest.approx(100.0 * np.hypot(float(a1.ravel()[k]), float(a2.ravel()[k])) / float(inner.ravel()[k]), rel=1e-15)
        assert rows[k]["axis"] == pytest.approx(np.degrees(0.5 * np.arctan2(float(a2.ravel()[k]), float(a1.ravel()[k]))), rel=1e-15)
    else:
        assert "a1" not in rows[0]


def test_axis_and_strength():
    for axis_deg in (30.0, 75.0, -30.0, -75.0, 0.0, 45.0, 90.0, -45.0):
        a1, a2 = 0.06 * np.cos(np.radians(2 * axis_deg)), 0.06 * np.sin(np.radians(2 * axis_deg))
        assert maps.fast_axis(a1, a2) == pytest.approx(axis_deg, abs=1e-12)
        assert maps.strength_percent(3.0, a1, a2) == pytest.approx(2.0, rel=1e-12)


def test_parser_defaults():
    a = maps.parser().parse_args(["dir"])
    assert (a.start, a.iterations, a.weight, a.damp, a.dvmax, a.azimuthal, a.azimuthal_weight) == ("mean", 3, None, None, 0.5, False, None)
    a = maps.parser().parse_args(["dir", "--start", "model", "--iterations", "5", "--weight", "3", "--damp", "0.1", "--dvmax", "0.2", "--azimuthal", "--azimuthal-weight", "9"])
    assert (a.start, a.iterations, a.weight, a.damp, a.dvmax, a.azimuthal, a.azimuthal_weight) == ("model", 5, 3.0, 0.1, 0.2, True, 9.0)


@pytest.mark.parametrize("argv", [["--iterations", "0"], ["--weight", "-1"], ["--weight", "nan"], ["--damp", "-0.5"], ["--damp", "inf"], ["--dvmax", "0"],
                                  ["--dvmax", "nan"], ["--azimuthal-weight", "2"], ["--azimuthal", "--azimuthal-weight", "-2"], ["--start", "flat"]])
def test_cli_refuses_before_the_library(monkeypatch, tmp_path, argv):
    import dsurftomo_amd.engine as E

    def refuse(*_):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(E, "load_library", refuse)
    monkeypatch.setattr(io, "load", refuse)
    with pytest.raises(SystemExit) as exc:
        maps.main([str(tmp_path)] + argv)
    assert exc.value.code == 2


@pytest.mark.parametrize("kw", [dict(iterations=0), dict(weight=-1.0), dict(damp=float("nan")), dict(dvmax=-0.5), dict(azimuthal_weight=1.0), dict(start="flat")])
def test_run_refuses_before_the_input_is_read(monkeypatch, tmp_path, kw):
    def refuse(*_):
        raise AssertionError("the input was read")
    monkeypatch.setattr(io, "load", refuse)
    with pytest.raises(ValueError):
        maps.run(str(tmp_path), **kw)


def test_new_symbols_declared_bound_and_exported():
    """the four entry points: declared in the public header, argtypes set by engine.py, Engine methods present, exported by the built library"""
    from dsurftomo_amd import build
    from dsurftomo_amd import engine as E
    build.build()
    with open(os.path.join(L.ROOT, "include", "dsurftomo_amd.h")) as fh:
        header = fh.read()
    lib = E.load_library()
    for name in NEW:
        assert re.search(r"^int %s\(dsa_engine\* e" % name, header, re.M), name
        assert getattr(lib, name).argtypes, name
    for method in ("solve_rows_maps", "solve_rows_maps_device", "iteration_system_maps_device", "update_maps", "get_maps"):
        assert callable(getattr(E.Engine, method))
    assert os.path.exists(os.path.join(L.ROOT, "dsurftomo_amd", "csrc", "map_system.h"))
