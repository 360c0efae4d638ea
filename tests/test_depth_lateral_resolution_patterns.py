"""The host side of `python -m dsurftomo_amd.depth --lateral W --lateral-resolution` and of dsa_columns_resolution_lateral (DESIGN.md section
27), no GPU: the flags' defaults and refusals, the files' round trips, the log on a stand-in engine, and the symbol in the public header, on
both kinds of handle, in the built library and in the build's list of headers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _libs as L
from dsurftomo_amd import depth, io

F = np.float32


def test_parser_defaults_and_old_attributes():
    a = depth.parser().parse_args(["dir"])
    assert (a.lateral_resolution, a.lateral_resolution_stride, a.lateral_checkerboard) == (False, 1, None) and depth.DEFAULT_CHECKER_AMP == 0.1
    assert (a.maps, a.iterations, a.smooth, a.damp, a.dvmax, a.min_dws, a.out, a.resolution, a.sigma, a.radial, a.aniso, a.lateral, a.lateral_tol, a.lateral_maxit,
            a.radial_lateral, a.radial_lateral_aniso, a.radial_resolution) == (None, 4, 0.5, 0.1, 0.5, 0.0, ".", False, None, False, 0.2, None, 1e-8, 500, None, None, False)
    a = depth.parser().parse_args(["dir", "--lateral", "0.7", "--lateral-resolution", "--lateral-resolution-stride", "3", "--lateral-checkerboard", "2,2,3,0.05", "--sigma", "0.02"])
    assert (a.lateral, a.lateral_resolution, a.lateral_resolution_stride, a.lateral_checkerboard, a.sigma) == (0.7, True, 3, "2,2,3,0.05", 0.02)
    assert depth.parse_checkerboard("2,2,3,0.05") == (2, 2, 3, 0.05) and depth.parse_checkerboard("1,4,2") == (1, 4, 2, 0.1)
    old = dict(iterations=4, smooth=0.5, damp=0.1, dvmax=0.5, min_dws=0.0, sigma=None, aniso=None, radial=False, resolution=False, lateral=0.3, lateral_tol=1e-8,
               lateral_maxit=500, radial_lateral=None, radial_lateral_aniso=None)
    new = dict(old, radial_resolution=False, lateral_resolution=True, lateral_resolution_stride=2, lateral_checkerboard="3,1,2")
    assert depth.check_options(depth.options_over_defaults(new)) == (None, None, (3, 1, 2, 0.1))
    assert depth.check_options(depth.options_over_defaults(old)) == (None, None, None)              # the old call: the later options at their defaults


@pytest.mark.parametrize("argv,message", [
    (["--lateral-resolution"], "--lateral-resolution needs --lateral"),
    (["--lateral-resolution", "--radial"], "--lateral-resolution and --radial exclude each other"),
    (["--lateral-resolution", "--radial", "--radial-lateral", "0.2"], "--lateral-resolution and --radial exclude each other"),
    (["--lateral", "0.2", "--lateral-resolution", "--radial"], "--lateral and --radial exclude each other"),           # the old refusals come first
    (["--lateral", "0.2", "--lateral-resolution", "--resolution"], "--lateral and --resolution exclude each other"),   # and stay
    (["--lateral", "0.2", "--resolution"], "--lateral and --resolution exclude each other"),
    (["--lateral", "0.2", "--lateral-resolution-stride", "2"], "--lateral-resolution-stride needs --lateral-resolution"),
    (["--lateral", "0.2", "--lateral-checkerboard", "2,2,2"], "--lateral-checkerboard needs --lateral-resolution"),
    (["--lateral", "0.2", "--lateral-resolution", "--lateral-resolution-stride", "0"], "--lateral-resolution-stride must be at least 1"),
    (["--lateral", "0.2", "--lateral-resolution", "--lateral-checkerboard", "2,2"], "--lateral-checkerboard takes NX,NY,NZ[,AMP]"),
    (["--lateral", "0.2", "--lateral-resolution", "--lateral-checkerboard", "2,x,2"], "--lateral-checkerboard takes NX,NY,NZ[,AMP]"),
    (["--lateral", "0.2", "--lateral-resolution", "--lateral-checkerboard", "2,0,2"], "the blocks must be at least 1 x 1 x 1"),
    (["--lateral", "0.2", "--lateral-resolution", "--lateral-checkerboard", "2,2,2,nan"], "AMP finite and not 0"),
    (["--lateral", "0.2", "--lateral-resolution", "--sigma", "0"], "--sigma must be finite and > 0"),
    (["--lateral", "0.2", "--lateral-resolution", "--lateral-maxit", "0"], "--lateral-maxit must be at least 1")])
def test_cli_refuses_before_the_library(monkeypatch, tmp_path, capsys, argv, message):
    import dsurftomo_amd.engine as E

    def refuse(*_):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(E, "load_library", refuse)
    monkeypatch.setattr(io, "load", refuse)
    with pytest.raises(SystemExit) as exc:
        depth.main([str(tmp_path)] + argv)
    assert exc.value.code == 2
    assert message in capsys.readouterr().err


def test_run_refuses_before_the_input_is_read(monkeypatch, tmp_path):
    import dsurftomo_amd.engine as E

    def refuse(*_):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(E, "load_library", refuse)
    monkeypatch.setattr(io, "load", refuse)
    with pytest.raises(ValueError, match="needs --lateral"):
        depth.run(str(tmp_path), lateral_resolution=True)
    with pytest.raises(ValueError, match="--lateral-resolution and --radial exclude"):
        depth.run(str(tmp_path), lateral_resolution=True, radial=True)
    with pytest.raises(ValueError, match="--lateral and --resolution exclude"):
        depth.run(str(tmp_path), lateral=0.2, lateral_resolution=True, resolution=True)
    with pytest.raises(ValueError, match="stride must be at least 1"):
        depth.run(str(tmp_path), lateral=0.2, lateral_resolution=True, lateral_resolution_stride=0)
    with pytest.raises(ValueError, match="needs --lateral-resolution"):
        depth.run(str(tmp_path), lateral=0.2, lateral_checkerboard="2,2,2")
    with pytest.raises(AssertionError, match="the library was loaded"):              # a good set of flags goes on to read the input
        depth.run(str(tmp_path), lateral=0.2, lateral_resolution=True, lateral_resolution_stride=4, lateral_checkerboard="2,2,2,0.2")


def grid(nx=6, ny=5, nz=4):
    return dict(nx=nx, ny=ny, nz=nz, depz=np.array([0.0, 3.0, 7.5, 13.0][:nz], F), goxd=24.5, gozd=121.0, dvxd=0.25, dvzd=0.3)


def test_checkerboard_model():
    m = depth.checkerboard_model(4, 3, 3, (2, 1, 2, 0.2))
    assert m.shape == (3, 12) and set(np.unique(m).tolist()) == {-0.2, 0.2}
    cube = m.reshape(3, 3, 4)
    assert cube[0, 0].tolist() == [0.2, 0.2, -0.2, -0.2] and cube[0, 1].tolist() == [-0.2, -0.2, 0.2, 0.2] and np.array_equal(cube[0], cube[1]) and np.array_equal(cube[2], -cube[0])


def test_the_files_round_trip(tmp_path):
    c = grid()
    M, nint = 3, 12
    rng = np.random.default_rng(4)
    index = np.arange(0, nint * M, 5, dtype=np.int32)
    psf = rng.random((len(index), 7)) + 0.1; unit = rng.random((len(index), 7))
    psf[2, 1:] = 0.0                                                             # a node that does not answer: lengths and share 0, not NaN
    cols = depth.lateral_resolution_columns(index, psf, unit, 0.04)
    assert cols["length_x"][2] == 0.0 and cols["own"][2] == 0.0 and np.isfinite(np.array(list(cols.values()))).all()
    assert cols["sd"][1] == 0.04 * np.sqrt(unit[1, 6]) and cols["length_z"][0] == np.sqrt(psf[0, 2] / psf[0, 1]) and cols["own"][0] == psf[0, 5] / psf[0, 1]
    path = str(tmp_path / "r.dat")
    depth.write_lateral_resolution(path, c, index, cols)
    back = depth.read_lateral_resolution(path)
    assert len(back) == len(index) and list(back[0]) == ["lon", "lat", "depth", "rjj", "length_z", "length_x", "length_y", "own", "sd_unit", "sd"]
    for q, row in enumerate(back):
        for name in cols:
            assert row[name] == cols[name][q]                                    # 17 significant digits: the same doubles
        b, l = divmod(int(index[q]), M)
        lon, lat = depth._lonlat(c, b % 4, b // 4)
        assert (row["lon"], row["lat"], row["depth"]) == (float(lon), float(lat), float(c["depz"][l]))
    model = depth.checkerboard_model(4, 3, M, (2, 2, 1, 0.1)); rec = model * rng.random((M, nint))
    path = str(tmp_path / "c.dat")
    depth.write_lateral_checker(path, c, model, rec)
    back = depth.read_lateral_checker(path)
    assert len(back) == M * nint and [r["input"] for r in back] == model.ravel().tolist() and [r["recovered"] for r in back] == rec.ravel().tolist()
    assert back[nint]["depth"] == 3.0 and back[0]["depth"] == 0.0


class StandIn:
    """an engine that records the calls of resolve_lateral"""
    def __init__(self, nx, ny, nz):
        self._disp = (nx, ny, nz)
        self.calls = []

    def dispersion_run(self, *a):
        self.calls.append(("run",) + a[:2])

    def columns_resolution_lateral(self, obs, wt, smooth, damp, lateral, kind, index, models, tol, maxit, full=False):
        nx, ny, nz = self._disp
        n, nint = len(kind), (nx - 2) * (ny - 2)
        self.calls.append(("resolution", smooth, damp, lateral, tol, maxit, full, np.array(kind), np.array(index), models))
        m = np.zeros((n, 7))
        m[:, 0] = 0.5; m[:, 1] = 4.0; m[:, 2] = 16.0; m[:, 3] = 1.0; m[:, 4] = 3.0; m[:, 5] = 1.0; m[:, 6] = np.where(np.asarray(kind) == 1, 0.25, 0.0)
        m[np.asarray(kind) == 2] = 0.0
        itn = np.arange(n, dtype=np.int32) % 7 + 3
        istop = np.ones(n, np.int32); istop[3] = 2
        out = dict(measures=m, itn=itn, istop=istop, rz0=np.ones(n), rz=np.zeros(n), nused=np.zeros(nx * ny, np.int32), flag=np.zeros(nx * ny, np.int32))
        if full:
            out["full"] = np.zeros((n, nz - 1, nint))
            out["full"][-1] = 0.5 * models[0]
        return out


def test_resolve_lateral_on_a_stand_in_engine(tmp_path):
    c = grid()
    plan = [(2, 0, np.array([4.0, 8.0]), 0), (1, 1, np.array([5.0]), 2)]
    obs = np.zeros((3, 30), F)
    eng = StandIn(6, 5, 4); lines = []
    out = depth.resolve_lateral(eng, c, plan, obs, None, 0.5, 0.1, 0.3, 1e-6, 40, 0.04, str(tmp_path), 4, (2, 2, 3, 0.1), lines.append)
    assert [k[0] for k in eng.calls] == ["run", "run", "resolution"] and eng.calls[2][1:7] == (0.5, 0.1, 0.3, 1e-6, 40, True)
    kind, index, models = eng.calls[2][7:]
    assert kind.tolist() == [0] * 9 + [1] * 9 + [2] and index.tolist() == list(range(0, 36, 4)) * 2 + [0] and models.shape == (1, 3, 12)
    assert out["columns"]["length_z"].tolist() == [2.0] * 9 and out["columns"]["own"].tolist() == [0.25] * 9 and out["columns"]["sd"].tolist() == [0.04 * 0.5] * 9
    rows = depth.read_lateral_resolution(out["lateral_resolution_path"])
    assert len(rows) == 9 and rows[0]["length_x"] == 0.5 and rows[0]["length_y"] == np.sqrt(0.75) and rows[0]["rjj"] == 0.5 and rows[0]["sd_unit"] == 0.5
    assert os.path.basename(out["lateral_resolution_path"]) == "DSurfTomo.inDepthLateralResolution.dat"
    assert os.path.basename(out["lateral_checker_path"]) == "DSurfTomo.inDepthLateralChecker.dat"
    back = depth.read_lateral_checker(out["lateral_checker_path"])
    assert len(back) == 36 and all(r["recovered"] == 0.5 * r["input"] for r in back)
    text = "\n".join(lines)
    assert "median own share 0.2500, median lateral length 1.0000 cells" in text and "19 members, 3 to 9 conjugate-gradient iterations" in text
    assert "1 members stopped at --lateral-maxit (istop 2), the first: member 3 (kind 0, index 12)" in text
    assert "recovered amplitude median 0.5000 of the input" in text and "sd for a data standard deviation of 0.040000 km/s" in text
    eng = StandIn(6, 5, 4); lines = []
    out = depth.resolve_lateral(eng, c, plan, obs, None, 0.5, 0.1, 0.3, 1e-8, 500, 0.04, str(tmp_path / "."), log=lines.append)          # no checkerboard: every unknown
    assert eng.calls[2][6] is False and len(eng.calls[2][7]) == 72 and eng.calls[2][9] is None and "lateral_checker_path" not in out


def test_new_symbol_declared_bound_and_exported():
    """declared in the public header, argtypes set by engine.py on both kinds of handle (load_library's and a bare CDLL through
    declare_solvers), an Engine method, exported by the built library; the new header is in the build's list"""
    from dsurftomo_amd import build
    from dsurftomo_amd import engine as E
    build.build()
    with open(os.path.join(L.ROOT, "include", "dsurftomo_amd.h")) as fh:
        header = fh.read()
    assert re.search(r"^int dsa_columns_resolution_lateral\(dsa_engine\* e, int nmaps, const float\* obs, const float\* wt, float smooth, float damp, float lateral, double tol,\s*"
                     r"int maxit, int nmembers, const int\* kind, const int\* index, const double\* models, int nrows, double\* measures,\s*"
                     r"double\* info, double\* full, int\* nused, int\* flag\);", header, re.M)
    lib = E.load_library()
    bare = E.declare_solvers(C.CDLL(build.LIB))
    for handle in (lib, bare):
        args = handle.dsa_columns_resolution_lateral.argtypes
        assert len(args) == 19 and args[7] is C.c_double and args[4:7] == [C.c_float] * 3 and args[8] is C.c_int and args[9] is C.c_int and args[13] is C.c_int
    assert callable(E.Engine.columns_resolution_lateral)
    assert "column_lateral_resolution.h" in build.HEADERS and "column_lateral.h" in build.HEADERS and "column_kernels.hip" in build.SOURCES
    assert os.path.exists(os.path.join(L.ROOT, "dsurftomo_amd", "csrc", "column_lateral_resolution.h"))
    assert len(lib.dsa_columns_step_lateral.argtypes) == 17 and len(lib.dsa_columns_resolution.argtypes) == 12           # the old entry points are as they were
    assert callable(depth.column_lateral_resolution_twin) and callable(depth.resolve_lateral)
