"""The host side of `python -m dsurftomo_amd.depth --radial --radial-lateral` and of dsa_columns_step_radial_lateral,
no GPU: the flags' defaults and refusals, the loop's choice of entry point and its log on a stand-in engine, and the symbol in the public
header, on both kinds of handle, in the built library and in the build's list of headers."""
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
    assert (a.radial_lateral, a.radial_lateral_aniso) == (None, None)
    assert (a.maps, a.iterations, a.smooth, a.damp, a.dvmax, a.min_dws, a.out, a.resolution, a.sigma, a.radial, a.aniso, a.lateral, a.lateral_tol, a.lateral_maxit) == \
        (None, 4, 0.5, 0.1, 0.5, 0.0, ".", False, None, False, 0.2, None, 1e-8, 500)                                   # as they were
    a = depth.parser().parse_args(["dir", "--radial", "--radial-lateral", "0.3", "--radial-lateral-aniso", "0.6", "--lateral-tol", "1e-6", "--lateral-maxit", "40"])
    assert (a.radial, a.radial_lateral, a.radial_lateral_aniso, a.lateral, a.lateral_tol, a.lateral_maxit) == (True, 0.3, 0.6, None, 1e-6, 40)
    assert depth.parser().parse_args(["dir", "--radial", "--radial-lateral", "0"]).radial_lateral == 0.0


@pytest.mark.parametrize("argv,message", [
    (["--radial-lateral", "0.3"], "--radial-lateral needs --radial"), (["--radial-lateral", "0"], "--radial-lateral needs --radial"),
    (["--radial", "--radial-lateral-aniso", "0.6"], "--radial-lateral-aniso needs --radial-lateral"),
    (["--radial-lateral-aniso", "0.6"], "--radial-lateral-aniso needs --radial-lateral"),
    (["--radial-lateral", "0.3", "--lateral", "0.2"], "--radial-lateral needs --radial"),
    (["--radial", "--radial-lateral", "0.3", "--lateral", "0.2"], "--lateral and --radial exclude each other"),               # the old refusal, as it was
    (["--radial", "--radial-lateral", "0.3", "--resolution"], "--radial and --resolution exclude each other"),                # the old refusal, as it was
    (["--radial", "--radial-lateral", "-0.1"], "--radial-lateral must be finite and >= 0"), (["--radial", "--radial-lateral", "nan"], "--radial-lateral must be finite and >= 0"),
    (["--radial", "--radial-lateral", "inf"], "--radial-lateral must be finite and >= 0"),
    (["--radial", "--radial-lateral", "0.3", "--radial-lateral-aniso=-1"], "--radial-lateral-aniso must be finite and >= 0"),
    (["--radial", "--radial-lateral", "0.3", "--radial-lateral-aniso", "nan"], "--radial-lateral-aniso must be finite and >= 0"),
    (["--radial", "--radial-lateral", "0.3", "--lateral-tol", "0"], "--lateral-tol must be finite and > 0"),
    (["--radial", "--radial-lateral", "0.3", "--lateral-maxit", "0"], "--lateral-maxit must be at least 1"),
    (["--radial", "--radial-lateral", "0.3", "--iterations", "0", "--lateral-maxit", "0"], "--iterations must be at least 1")])      # the old refusals come first
def test_cli_refuses_before_the_library(monkeypatch, tmp_path, capsys, argv, message):
    """check(), check_lateral(), check_radial() and check_radial_lateral() refuse with their own messages (a parser error would give the same
    exit code)"""
    import dsurftomo_amd.engine as E

    def refuse(*_):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(E, "load_library", refuse)
    monkeypatch.setattr(io, "load", refuse)
    with pytest.raises(SystemExit) as exc:
        depth.main([str(tmp_path)] + argv)
    assert exc.value.code == 2
    assert message in capsys.readouterr().err


def test_the_companions_are_looked_at_with_either_coupling(monkeypatch, tmp_path):
    """without --lateral and --radial-lateral, --lateral-tol and --lateral-maxit are not looked at, so the call goes on to read the input; a
    good --radial --radial-lateral call gets that far too"""
    def reached(*_):
        raise AssertionError("the input was read")
    monkeypatch.setattr(io, "load", reached)
    out = str(tmp_path / "out")
    for argv in (["--radial", "--lateral-maxit", "0", "--lateral-tol", "0"], ["--radial", "--radial-lateral", "0.3", "--radial-lateral-aniso", "0.6"],
                 ["--radial", "--radial-lateral", "0"]):
        with pytest.raises(AssertionError, match="the input was read"):
            depth.main([out, "--out", out] + argv)
    with pytest.raises(AssertionError, match="the input was read"):
        depth.run(str(tmp_path), radial=True, lateral_tol=0.0, lateral_maxit=0)


def test_run_refuses_before_the_input_is_read(monkeypatch, tmp_path):
    import dsurftomo_amd.engine as E

    def refuse(*_):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(E, "load_library", refuse)
    monkeypatch.setattr(io, "load", refuse)
    d = str(tmp_path)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="--radial-lateral must"):
            depth.run(d, radial=True, radial_lateral=bad)
        with pytest.raises(ValueError, match="--radial-lateral-aniso must"):
            depth.run(d, radial=True, radial_lateral=0.3, radial_lateral_aniso=bad)
    with pytest.raises(ValueError, match="--lateral-tol"):
        depth.run(d, radial=True, radial_lateral=0.3, lateral_tol=0.0)
    with pytest.raises(ValueError, match="--lateral-maxit"):
        depth.run(d, radial=True, radial_lateral=0.3, lateral_maxit=0)
    with pytest.raises(ValueError, match="--radial-lateral needs --radial"):
        depth.run(d, radial_lateral=0.3)
    with pytest.raises(ValueError, match="--radial-lateral-aniso needs --radial-lateral"):
        depth.run(d, radial=True, radial_lateral_aniso=0.3)
    with pytest.raises(ValueError, match="--lateral and --radial exclude"):
        depth.run(d, radial=True, radial_lateral=0.3, lateral=0.2)
    with pytest.raises(ValueError, match="--radial and --resolution exclude"):
        depth.run(d, radial=True, radial_lateral=0.3, resolution=True)
    with pytest.raises(ValueError, match="--radial-lateral and --lateral exclude"):
        depth.check_radial_lateral(0.3, None, True, 0.2, False)
    with pytest.raises(ValueError, match="--radial-lateral and --resolution exclude"):
        depth.check_radial_lateral(0.3, 0.6, True, None, True)
    depth.check(radial_lateral=0.0, radial_lateral_aniso=0.0, lateral_tol=1e-3, lateral_maxit=1)
    depth.check_radial_lateral()
    depth.check_radial_lateral(0.0, None, True)


class StandIn:
    """an engine that records the calls of the radial loop"""
    def __init__(self, nx, ny, nz):
        self._disp = (nx, ny, nz)
        self.calls = []

    def dispersion_run(self, *a):
        self.calls.append(("run",) + a[:2])

    def _result(self):
        nx, ny, nz = self._disp
        nused = np.zeros((2, ny, nx), np.int32); nused[:, 1:-1, 1:-1] = 3
        nused[:, 2, 2] = 0; nused[:, 1, 1] = 0
        nused = nused.reshape(2, -1)
        return dict(dv_sv=np.zeros((nz - 1, nx * ny), F), dv_sh=np.zeros((nz - 1, nx * ny), F), nused=nused, chi2=np.where(nused > 0, 0.03, 0.0),
                    flag=np.zeros(nx * ny, np.int32))

    def columns_step_radial(self, *a):
        self.calls.append(("radial",) + a[2:])
        out = self._result()
        out["flag"][out["nused"].sum(axis=0) == 0] = 2
        out["flag"][0] = 0
        return out

    def columns_step_radial_lateral(self, *a):
        self.calls.append(("radial_lateral",) + a[2:])
        out = self._result()
        out["flag"][1 * self._disp[0] + 1] = 1                                  # of the two columns without data one is flagged: not carried
        return dict(out, itn=17, istop=2, rz0=1.0, rz=1e-3, carried=1)


def test_the_loop_calls_the_new_entry_only_with_the_flag():
    plan = [(2, 0, np.array([4.0, 8.0]), 0), (1, 1, np.array([5.0]), 2)]
    obs = np.zeros((3, 30), F)
    old = StandIn(6, 5, 4); lines = []
    out = depth.iterate_radial(old, plan, obs, None, 2, 0.5, 0.1, 0.2, 0.4, 1.0, 5.0, lines.append)
    assert [c[0] for c in old.calls] == ["run", "run", "radial"] * 2 and old.calls[2][1:] == (0.5, 0.1, 0.2, 0.4, 1.0, 5.0)
    assert len(lines) == 2 and all("lateral" not in l and "conjugate" not in l for l in lines)
    assert sorted(out["history"][0]) == ["chi2", "flagged1", "flagged2", "iteration", "nused", "nused_l", "nused_r", "rms", "rms_l", "rms_r"]      # as it was
    new = StandIn(6, 5, 4); lines = []
    out = depth.iterate_radial(new, plan, obs, None, 2, 0.5, 0.1, 0.2, 0.4, 1.0, 5.0, lines.append, 0.3, 0.6, 1e-6, 40)
    assert [c[0] for c in new.calls] == ["run", "run", "radial_lateral"] * 2 and new.calls[2][1:] == (0.5, 0.1, 0.2, 0.3, 0.6, 0.4, 1.0, 5.0, 1e-6, 40)
    assert len(lines) == 4 and lines[0].startswith(" depth iteration 1 (radial): ")
    assert "(radial, lateral 0.3, on Vsh - Vsv 0.6): 17 conjugate-gradient iterations, istop 2 (--lateral-maxit was reached), 1 columns without data carried" in lines[1]
    assert (out["history"][1]["itn"], out["history"][1]["istop"], out["history"][1]["carried"]) == (17, 2, 1)
    same = StandIn(6, 5, 4)
    depth.iterate_radial(same, plan, obs, None, 1, 0.5, 0.1, 0.2, 0.4, 1.0, 5.0, lambda s: None, 0.3)                # A defaults to W
    assert same.calls[-1][0] == "radial_lateral" and same.calls[-1][4:6] == (0.3, 0.3) and same.calls[-1][-2:] == (1e-8, 500)
    zero = StandIn(6, 5, 4)
    depth.iterate_radial(zero, plan, obs, None, 1, 0.5, 0.1, 0.2, 0.4, 1.0, 5.0, lambda s: None, 0.0)                # --radial-lateral 0 is the new entry too
    assert zero.calls[-1][0] == "radial_lateral" and zero.calls[-1][4:6] == (0.0, 0.0)


def test_new_symbol_declared_bound_and_exported():
    """declared in the public header, argtypes set by engine.py on both kinds of handle (load_library's and a bare CDLL through
    declare_solvers), an Engine method, exported by the built library; the new header is in the build's list"""
    from dsurftomo_amd import build
    from dsurftomo_amd import engine as E
    build.build()
    with open(os.path.join(L.ROOT, "include", "dsurftomo_amd.h")) as fh:
        header = fh.read()
    assert re.search(r"^int dsa_columns_step_radial_lateral\(dsa_engine\* e, int nmaps, const float\* obs, const float\* wt, float smooth, float damp, float aniso, float lateral,\s*"
                     r"float lateral_aniso, float dvmax, float minvel, float maxvel, double tol, int maxit, float\* dv, int\* nused,\s*double\* chi2, int\* flag, double\* info\);",
                     header, re.M)
    lib = E.load_library()
    bare = E.declare_solvers(C.CDLL(build.LIB))
    for handle in (lib, bare):
        args = handle.dsa_columns_step_radial_lateral.argtypes
        assert len(args) == 19 and args[12] is C.c_double and args[13] is C.c_int and args[4:12] == [C.c_float] * 8
    assert callable(E.Engine.columns_step_radial_lateral)
    for name in ("column_radial_lateral.h", "column_lateral.h", "column_radial.h", "column_system.h"):
        assert name in build.HEADERS and os.path.exists(os.path.join(L.ROOT, "dsurftomo_amd", "csrc", name))
    assert "column_kernels.hip" in build.SOURCES
    assert len(lib.dsa_columns_step_radial.argtypes) == 14 and len(lib.dsa_columns_step_lateral.argtypes) == 17        # the old entry points are as they were
    assert callable(depth.column_radial_lateral_twin) and callable(depth.check_radial_lateral)
