"""The host side of `python -m dsurftomo_amd.depth --lateral` and of dsa_columns_step_lateral, no GPU: the flags'
defaults and refusals, the loop's choice of entry point and its log on a stand-in engine, and the symbol in the public header, on both kinds
of handle, in the built library and in the build's list of headers."""
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
    assert (a.lateral, a.lateral_tol, a.lateral_maxit) == (None, 1e-8, 500) and (depth.DEFAULT_LATERAL_TOL, depth.DEFAULT_LATERAL_MAXIT) == (1e-8, 500)
    assert (a.maps, a.iterations, a.smooth, a.damp, a.dvmax, a.min_dws, a.out, a.resolution, a.sigma, a.radial, a.aniso) == \
        (None, 4, 0.5, 0.1, 0.5, 0.0, ".", False, None, False, 0.2)                                                    # as they were
    a = depth.parser().parse_args(["dir", "--lateral", "0.7", "--lateral-tol", "1e-6", "--lateral-maxit", "40", "--damp", "0.3"])
    assert (a.lateral, a.lateral_tol, a.lateral_maxit, a.damp, a.smooth) == (0.7, 1e-6, 40, 0.3, 0.5)
    assert depth.parser().parse_args(["dir", "--lateral", "0"]).lateral == 0.0


@pytest.mark.parametrize("argv,message", [
    (["--lateral", "-0.1"], "--lateral must be finite and >= 0"), (["--lateral", "nan"], "--lateral must be finite and >= 0"),
    (["--lateral", "inf"], "--lateral must be finite and >= 0"), (["--lateral", "0.2", "--radial"], "--lateral and --radial exclude each other"),
    (["--lateral", "0.2", "--resolution"], "--lateral and --resolution exclude each other"),
    (["--lateral", "0", "--resolution", "--sigma", "0.05"], "--lateral and --resolution exclude each other"),
    (["--lateral", "0.2", "--lateral-tol", "0"], "--lateral-tol must be finite and > 0"), (["--lateral", "0.2", "--lateral-tol", "nan"], "--lateral-tol must be finite and > 0"),
    (["--lateral", "0.2", "--lateral-tol=-1e-8"], "--lateral-tol must be finite and > 0"), (["--lateral", "0.2", "--lateral-maxit", "0"], "--lateral-maxit must be at least 1"),
    (["--lateral", "0.2", "--iterations", "0", "--lateral-maxit", "0"], "--iterations must be at least 1")])      # the old refusals come first
def test_cli_refuses_before_the_library(monkeypatch, tmp_path, capsys, argv, message):
    """check() and check_lateral() refuse with their own messages (a parser error would give the same exit code)"""
    import dsurftomo_amd.engine as E

    def refuse(*_):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(E, "load_library", refuse)
    monkeypatch.setattr(io, "load", refuse)
    with pytest.raises(SystemExit) as exc:
        depth.main([str(tmp_path)] + argv)
    assert exc.value.code == 2
    assert message in capsys.readouterr().err


def test_the_companions_are_looked_at_only_with_the_flag(monkeypatch, tmp_path):
    """main() and run() agree: without --lateral, --lateral-tol and --lateral-maxit are not looked at, so the call goes on to read the input"""
    def reached(*_):
        raise AssertionError("the input was read")
    monkeypatch.setattr(io, "load", reached)
    with pytest.raises(AssertionError, match="the input was read"):
        depth.main([str(tmp_path / "out"), "--out", str(tmp_path / "out"), "--lateral-maxit", "0", "--lateral-tol", "0"])
    with pytest.raises(AssertionError, match="the input was read"):
        depth.run(str(tmp_path), lateral_tol=0.0, lateral_maxit=0)


def test_run_refuses_before_the_input_is_read(monkeypatch, tmp_path):
    import dsurftomo_amd.engine as E

    def refuse(*_):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(E, "load_library", refuse)
    monkeypatch.setattr(io, "load", refuse)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="--lateral must"):
            depth.run(str(tmp_path), lateral=bad)
    with pytest.raises(ValueError, match="--lateral-tol"):
        depth.run(str(tmp_path), lateral=0.2, lateral_tol=0.0)
    with pytest.raises(ValueError, match="--lateral-maxit"):
        depth.run(str(tmp_path), lateral=0.2, lateral_maxit=0)
    with pytest.raises(ValueError, match="--lateral and --radial exclude"):
        depth.run(str(tmp_path), lateral=0.2, radial=True)
    with pytest.raises(ValueError, match="--lateral and --resolution exclude"):
        depth.run(str(tmp_path), lateral=0.2, resolution=True)
    depth.check(lateral=0.0, lateral_tol=1e-3, lateral_maxit=1)
    depth.check_lateral()


class StandIn:
    """an engine that records the calls of the loop"""
    def __init__(self, nx, ny, nz):
        self._disp = (nx, ny, nz)
        self.calls = []

    def dispersion_run(self, *a):
        self.calls.append(("run",) + a[:2])

    def _result(self):
        nx, ny, nz = self._disp
        nused = np.zeros((ny, nx), np.int32); nused[1:-1, 1:-1] = 3
        nused[2, 2] = 0; nused[1, 1] = 0
        flag = np.zeros(nx * ny, np.int32)
        return dict(dv=np.zeros((nz - 1, nx * ny), F), nused=nused.ravel(), chi2=np.where(nused.ravel() > 0, 0.03, 0.0), flag=flag)

    def columns_step(self, *a):
        self.calls.append(("step",) + a[2:])
        out = self._result()
        out["flag"][out["nused"] == 0] = 2
        out["flag"][0] = 0
        return out

    def columns_step_lateral(self, *a):
        self.calls.append(("lateral",) + a[2:])
        out = self._result()
        out["flag"][1 * self._disp[0] + 1] = 1                                  # of the two columns without data one is flagged: not carried
        return dict(out, itn=17, istop=2, rz0=1.0, rz=1e-3, carried=1)


def test_the_loop_calls_the_new_entry_only_with_the_flag():
    plan = [(2, 0, np.array([4.0, 8.0]), 0), (1, 1, np.array([5.0]), 2)]
    obs = np.zeros((3, 30), F)
    old = StandIn(6, 5, 4); lines = []
    out = depth.iterate(old, plan, obs, None, 2, 0.5, 0.1, 0.4, 1.0, 5.0, lines.append)
    assert [c[0] for c in old.calls] == ["run", "run", "step"] * 2 and old.calls[2][1:] == (0.5, 0.1, 0.4, 1.0, 5.0)
    assert len(lines) == 2 and all("lateral" not in l and "conjugate" not in l for l in lines)
    assert sorted(out["history"][0]) == ["chi2", "flagged1", "flagged2", "iteration", "nused", "rms"]             # as it was
    new = StandIn(6, 5, 4); lines = []
    out = depth.iterate(new, plan, obs, None, 2, 0.5, 0.1, 0.4, 1.0, 5.0, lines.append, 0.3, 1e-6, 40)
    assert [c[0] for c in new.calls] == ["run", "run", "lateral"] * 2 and new.calls[2][1:] == (0.5, 0.1, 0.3, 0.4, 1.0, 5.0, 1e-6, 40)
    assert len(lines) == 4 and lines[0].startswith(" depth iteration 1: ") and "(lateral 0.3): 17 conjugate-gradient iterations, istop 2 (--lateral-maxit was reached), 1 columns without data carried" in lines[1]
    assert (out["history"][1]["itn"], out["history"][1]["istop"], out["history"][1]["carried"]) == (17, 2, 1)
    zero = StandIn(6, 5, 4)
    depth.iterate(zero, plan, obs, None, 1, 0.5, 0.1, 0.4, 1.0, 5.0, lambda s: None, 0.0)                          # --lateral 0 is the new entry too
    assert zero.calls[-1][0] == "lateral" and zero.calls[-1][3] == 0.0


def test_new_symbol_declared_bound_and_exported():
    """declared in the public header, argtypes set by engine.py on both kinds of handle (load_library's and a bare CDLL through
    declare_solvers), an Engine method, exported by the built library; the new header is in the build's list"""
    from dsurftomo_amd import build
    from dsurftomo_amd import engine as E
    build.build()
    with open(os.path.join(L.ROOT, "include", "dsurftomo_amd.h")) as fh:
        header = fh.read()
    assert re.search(r"^int dsa_columns_step_lateral\(dsa_engine\* e, int nmaps, const float\* obs, const float\* wt, float smooth, float damp, float lateral, float dvmax,\s*"
                     r"float minvel, float maxvel, double tol, int maxit, float\* dv, int\* nused, double\* chi2, int\* flag, double\* info\);", header, re.M)
    lib = E.load_library()
    bare = E.declare_solvers(C.CDLL(build.LIB))
    for handle in (lib, bare):
        args = handle.dsa_columns_step_lateral.argtypes
        assert len(args) == 17 and args[10] is C.c_double and args[11] is C.c_int and args[4:10] == [C.c_float] * 6
    assert callable(E.Engine.columns_step_lateral)
    assert "column_lateral.h" in build.HEADERS and "column_system.h" in build.HEADERS and "column_kernels.hip" in build.SOURCES
    assert os.path.exists(os.path.join(L.ROOT, "dsurftomo_amd", "csrc", "column_lateral.h"))
    assert len(lib.dsa_columns_step.argtypes) == 13 and len(lib.dsa_columns_step_radial.argtypes) == 14           # the old entry points are as they were
    assert callable(depth.column_lateral_twin) and callable(depth.lateral_sum)
