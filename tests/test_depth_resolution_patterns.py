"""The host side of the depth resolution (dsurftomo_amd/depth.py --resolution), no GPU: the new flags and what they
leave alone, the refusals before the library is loaded, the two files' round trips, the log's summary, the new symbol in the header, the
binding and the built library -- and the twin next to the CPU build of the header on the oracle's curves of tests/test_gpu_columns.py's
smooth model."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _libs as L
import column_resolution_ref as CR
import columns_ref as R
from dsurftomo_amd import depth, io, maps

F = np.float32
NEW = "dsa_columns_resolution"


@pytest.fixture(scope="module")
def taipei():
    return io.load()


def small_case(taipei):
    return dict(taipei, nx=6, ny=5, nz=3, depz=np.array([0.0, 2.0, 5.0], F), tRc=np.array([4.0, 6.5]), tRg=np.array([5.0]), tLc=np.zeros(0), tLg=np.array([8.0]), kmax=4)


def test_parser_defaults_and_old_attributes():
    a = depth.parser().parse_args(["dir"])
    assert (a.resolution, a.sigma) == (False, None)
    assert (a.maps, a.iterations, a.smooth, a.damp, a.dvmax, a.min_dws, a.out) == (None, 4, 0.5, 0.1, 0.5, 0.0, ".")      # as they were
    a = depth.parser().parse_args(["dir", "--resolution"])
    assert (a.resolution, a.sigma) == (True, None)
    a = depth.parser().parse_args(["dir", "--resolution", "--sigma", "0.04", "--damp", "0.3"])
    assert (a.resolution, a.sigma, a.damp, a.smooth) == (True, 0.04, 0.3, 0.5)


@pytest.mark.parametrize("argv", [["--resolution", "--sigma", "0"], ["--resolution", "--sigma", "-0.1"], ["--resolution", "--sigma", "nan"],
                                  ["--resolution", "--sigma", "inf"], ["--sigma", "0"]])
def test_cli_refuses_before_the_library(monkeypatch, tmp_path, argv):
    import dsurftomo_amd.engine as E

    def refuse(*_):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(E, "load_library", refuse)
    monkeypatch.setattr(io, "load", refuse)
    with pytest.raises(SystemExit) as exc:
        depth.main([str(tmp_path)] + argv)
    assert exc.value.code == 2


@pytest.mark.parametrize("sigma", [0.0, -1.0, float("nan"), float("inf")])
def test_run_refuses_before_the_input_is_read(monkeypatch, tmp_path, sigma):
    def refuse(*_):
        raise AssertionError("the input was read")
    monkeypatch.setattr(io, "load", refuse)
    with pytest.raises(ValueError, match="--sigma"):
        depth.run(str(tmp_path), resolution=True, sigma=sigma)
    depth.check(sigma=0.05)
    depth.check(sigma=None)


def test_resolution_files_round_trip(tmp_path, taipei):
    c = small_case(taipei)
    nx, ny, nz, nm = 6, 5, 3, 4
    M = nz - 1
    rng = np.random.default_rng(9)
    measures = rng.random((4, M, ny * nx))
    measures[0] -= 0.05                                                            # (R_jj may be negative)
    measures[1, 0, 7] = 0.0                                                        # m1 = 0: the length is written as 0
    measures[:, :, 0] = 0.0                                                        # a ring column: zeros
    sigma = 0.0371
    path = str(tmp_path / "DepthResolution.dat")
    depth.write_resolution(path, c, measures, sigma)
    rows = depth.read_resolution(path)
    assert len(rows) == M * ny * nx
    m = measures.reshape(4, -1)
    assert [r["rjj"] for r in rows] == m[0].tolist()
    want = np.sqrt(np.divide(m[2], m[1], out=np.zeros(m.shape[1]), where=m[1] > 0))
    assert [r["length"] for r in rows] == want.tolist() and rows[7]["length"] == 0.0 and rows[0]["length"] == 0.0
    assert [r["sd_unit"] for r in rows] == np.sqrt(m[3]).tolist() and [r["sd"] for r in rows] == (sigma * np.sqrt(m[3])).tolist()
    assert [r["depth"] for r in rows[::nx * ny]] == [0.0, 2.0]                    # the bottom depth has no line
    lon, lat = maps._lonlat(c, 0, 0)
    k = 1 * nx + 1
    assert rows[k]["lon"] == float(lon) and rows[k]["lat"] == float(lat)           # node order: Depth.dat's
    with open(path) as fh:
        assert re.search(r"\d\.\d{15,16}(e[-+]\d+)?\b", fh.read())               # 17 significant digits
    leverage = rng.random((nm, ny * nx))
    lpath = str(tmp_path / "DepthLeverage.dat")
    depth.write_leverage(lpath, c, leverage)
    rows = depth.read_leverage(lpath)
    assert len(rows) == nm * ny * nx
    per = maps.period_list(c)
    assert [(r["wave"], r["kind"], r["period"]) for r in rows[:nm]] == per == [(2, 0, 4.0), (2, 0, 6.5), (2, 1, 5.0), (1, 1, 8.0)]
    assert [r["leverage"] for r in rows] == leverage.T.ravel().tolist()          # column by column, the periods in slot order
    assert rows[k * nm]["lon"] == float(lon) and rows[k * nm + nm - 1]["lat"] == float(lat)
    assert depth.psf_length([0.0, 4.0], [5.0, 16.0]).tolist() == [0.0, 2.0]


def test_summary_of_the_log(taipei):
    c = small_case(taipei)
    nx, ny, M = 6, 5, 2
    flag = np.zeros(ny * nx, np.int32); trace = np.zeros(ny * nx); measures = np.zeros((4, M, ny * nx))
    inner = R.interior(nx, ny) == 1
    trace[inner] = np.linspace(1.0, 2.1, inner.sum())
    measures[0, 0, inner] = 0.6; measures[0, 1, inner] = 0.05
    flag[1 * nx + 1] = 2; flag[1 * nx + 2] = 1                                   # two interior columns flagged: not in the statistics
    sm = depth.resolution_summary(c, dict(flag=flag, trace=trace, measures=measures))
    ok = inner & (flag == 0)
    assert (sm["flagged1"], sm["flagged2"], sm["columns"]) == (1, 1, 10) and ok.sum() == 10
    assert sm["trace"] == (float(np.median(trace[ok])), float(trace[ok].min()), float(trace[ok].max()))
    assert sm["depth"] == 2.0                                                      # the median R_jj is under 0.1 from the second depth down
    measures[0, 1, inner] = 0.3
    assert depth.resolution_summary(c, dict(flag=flag, trace=trace, measures=measures))["depth"] is None
    flag[:] = 2
    assert depth.resolution_summary(c, dict(flag=flag, trace=trace, measures=measures))["trace"] is None


def test_new_symbol_declared_bound_and_exported():
    """declared in the public header, argtypes set by engine.py on both kinds of handle (load_library's and a bare CDLL through
    declare_solvers), an Engine method, exported by the built library; the new header is in the build's list"""
    from dsurftomo_amd import build
    from dsurftomo_amd import engine as E
    build.build()
    with open(os.path.join(L.ROOT, "include", "dsurftomo_amd.h")) as fh:
        header = fh.read()
    assert re.search(r"^int %s\(dsa_engine\* e, int nmaps, const float\* obs, const float\* wt, float smooth, float damp, double\* measures,\s*double\* leverage, "
                     r"double\* trace, double\* R, int\* nused, int\* flag\);" % NEW, header, re.M)
    lib = E.load_library()
    bare = E.declare_solvers(C.CDLL(build.LIB))
    for handle in (lib, bare):
        assert len(getattr(handle, NEW).argtypes) == 12
    assert callable(E.Engine.columns_resolution)
    assert "column_resolution.h" in build.HEADERS and "column_system.h" in build.HEADERS
    assert os.path.exists(os.path.join(L.ROOT, "dsurftomo_amd", "csrc", "column_resolution.h"))
    assert len(lib.dsa_columns_step.argtypes) == 13                               # the step's entry point is as it was


@pytest.mark.parametrize("nz", [3, 8])
def test_twin_and_header_on_the_oracles_curves(nz):
    """tests/test_gpu_columns.py's smooth model, 5 x 5, its 12 periods, the curves and kernels from the oracle's depthkernel: the CPU build
    of the header against the twin within the measured tolerance in every interior column, the twin's own two answers printed; the sum
    of the leverages is the trace, more damping resolves less, nothing is flagged.  The traces are printed beside the figures of a run with
    numpy.linalg.solve on the same curves (damp 0.05 / 0.5: nz = 8 3.29-3.41 / 2.22-2.31, nz = 3 1.02-1.05 / 0.91-0.93), not asserted."""
    h = CR.load()
    hs = R.load()
    depz = R.depths(nz)
    vel = R.smooth_model(R.NX, R.NY, nz)
    ncol = R.NX * R.NY
    pv, svs, svp, srho = R.oracle_curves(vel, depz)
    S = R.host_combine(hs, vel.reshape(nz, ncol), depz, svs, svp, srho)
    obs = pv.astype(F)
    inner = np.flatnonzero(R.interior(R.NX, R.NY))
    assert (pv[:, inner] > 0).all()
    traces = {}
    for damp in (0.05, 0.5):
        got = CR.host_resolution(h, obs, None, pv, S, depz, R.SMOOTH, damp, R.interior(R.NX, R.NY))
        assert not got["flag"].any() and (got["nused"][inner] == R.K).all()
        worst = 0.0
        for c in inner:
            twin = depth.column_resolution_twin(obs[:, c], None, pv[:, c], S[:, :, c].T, depz, R.SMOOTH, damp)
            rmax = np.abs(twin["other"]["R"]).max()
            worst = max(worst, np.abs(twin["R"] - twin["other"]["R"]).max() / rmax)
            one = {k: (v[..., c] if v.ndim > 1 else v[c]) for k, v in got.items()}
            assert twin["flag"] == 0 and max(CR.differences(one, twin, rmax).values()) <= CR.TOL
            assert abs(one["leverage"].sum() - one["trace"]) <= CR.TOL * rmax
            assert (one["leverage"] > 0).all() and (one["leverage"] < 1).all() and (one["measures"][3] > 0).all()
        traces[damp] = got["trace"][inner]
        ring = R.interior(R.NX, R.NY) == 0
        assert not got["trace"][ring].any() and not got["R"][:, :, ring].any()
        print("nz %d damp %g: trace %.4f to %.4f; the twin's ldlt against pinv at most %.3g" % (nz, damp, traces[damp].min(), traces[damp].max(), worst))
    assert (traces[0.5] < traces[0.05]).all() and (traces[0.05] < nz - 1).all() and (traces[0.5] > 0).all()
