"""The host side of the resolution of the radial step (dsurftomo_amd/depth.py --radial --radial-resolution), no GPU:
the new flag and what it leaves alone, the refusals before the library is loaded, the two files' round trips, the log's summary, the new
symbol in the header, the binding and the built library -- and the twin next to the CPU build of the header on the oracle's curves of
tests/test_gpu_columns.py's smooth model with Vsh 3 % above Vsv."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _libs as L
import column_radial_ref as RR
import column_radial_resolution_ref as RS
import columns_ref as R
from dsurftomo_amd import depth, io, maps

F = np.float32
NEW = "dsa_columns_resolution_radial"


@pytest.fixture(scope="module")
def taipei():
    return io.load()


def small_case(taipei):
    return dict(taipei, nx=6, ny=5, nz=3, depz=np.array([0.0, 2.0, 5.0], F), tRc=np.array([4.0, 6.5]), tRg=np.array([5.0]), tLc=np.zeros(0), tLg=np.array([8.0]), kmax=4)


def made_up_result(rng, nx, ny, M, nm):
    ncol = nx * ny
    measures = rng.random((6, 2 * M, ncol))
    measures[0] -= 0.05                                                            # (R_jj and R_cross may be negative)
    measures[4] -= 0.5
    pair = np.stack([0.2 * (rng.random((M, ncol)) - 0.5), rng.random((M, ncol))])
    return dict(measures=measures, pair=pair, leverage=rng.random((nm, ncol)), trace=rng.random((2, ncol)), nused=np.ones((2, ncol), np.int32),
                flag=np.zeros(ncol, np.int32))


def test_parser_default_and_old_attributes():
    a = depth.parser().parse_args(["dir"])
    assert a.radial_resolution is False
    assert (a.maps, a.iterations, a.smooth, a.damp, a.dvmax, a.min_dws, a.out) == (None, 4, 0.5, 0.1, 0.5, 0.0, ".")      # as they were
    assert (a.resolution, a.sigma, a.radial, a.aniso, a.lateral, a.lateral_tol, a.lateral_maxit, a.radial_lateral, a.radial_lateral_aniso) == \
        (False, None, False, 0.2, None, 1e-8, 500, None, None)
    a = depth.parser().parse_args(["dir", "--radial", "--radial-resolution", "--sigma", "0.04"])
    assert (a.radial, a.radial_resolution, a.sigma, a.resolution) == (True, True, 0.04, False)


@pytest.mark.parametrize("argv", [["--radial-resolution"], ["--radial-resolution", "--resolution"], ["--radial", "--radial-resolution", "--radial-lateral", "0.2"],
                                  ["--radial", "--radial-resolution", "--sigma", "0"], ["--radial", "--radial-resolution", "--sigma", "nan"],
                                  ["--radial", "--radial-resolution", "--sigma", "-0.1"], ["--radial", "--resolution"],
                                  ["--radial", "--radial-resolution", "--resolution"]])
def test_cli_refuses_before_the_library(monkeypatch, tmp_path, argv):
    import dsurftomo_amd.engine as E

    def refuse(*_):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(E, "load_library", refuse)
    monkeypatch.setattr(io, "load", refuse)
    with pytest.raises(SystemExit) as exc:
        depth.main([str(tmp_path)] + argv)
    assert exc.value.code == 2


def test_run_refuses_before_the_input_is_read(monkeypatch, tmp_path):
    def refuse(*_):
        raise AssertionError("the input was read")
    monkeypatch.setattr(io, "load", refuse)
    with pytest.raises(ValueError, match="--radial-resolution needs --radial"):
        depth.run(str(tmp_path), radial_resolution=True)
    with pytest.raises(ValueError, match="--radial-resolution and --radial-lateral exclude each other: the resolution of the laterally coupled system is not computed"):
        depth.run(str(tmp_path), radial=True, radial_resolution=True, radial_lateral=0.2)
    for sigma in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="--sigma"):
            depth.run(str(tmp_path), radial=True, radial_resolution=True, sigma=sigma)
    with pytest.raises(ValueError, match="the resolution of the coupled Vsv / Vsh system is not computed"):          # as it was
        depth.run(str(tmp_path), radial=True, resolution=True, radial_resolution=True)
    depth.check_radial_resolution(False, False, 0.2)
    depth.check_radial_resolution(True, True, None)
    old = dict(iterations=4, smooth=0.5, damp=0.1, dvmax=0.5, min_dws=0.0, sigma=None, aniso=0.2, radial=True, resolution=False, lateral=None, lateral_tol=1e-8,
               lateral_maxit=500, radial_lateral=None, radial_lateral_aniso=None)
    depth.check_options(depth.options_over_defaults(old))                            # the old call still answers: the later options at their defaults
    depth.check_options(depth.options_over_defaults(dict(old, sigma=0.05, radial_resolution=True)))


def test_files_round_trip(tmp_path, taipei):
    c = small_case(taipei)
    nx, ny, nz, nm = 6, 5, 3, 4
    M = nz - 1
    ncol = nx * ny
    rng = np.random.default_rng(9)
    res = made_up_result(rng, nx, ny, M, nm)
    m, pair = res["measures"], res["pair"]
    m[1, 0, 7] = 0.0; m[3, 0, 7] = 0.0                                             # m1_own = m1_cross = 0: length and leak share are written as 0
    m[:, :, 0] = 0.0; pair[:, :, 0] = 0.0                                          # a ring column: zeros
    pair[0, 1, 9] = 10.0                                                           # a covariance that makes the radicand of sd_xi negative: clamped
    vsv = (3.0 + rng.random((nz, ncol))).astype(F); vsh = (vsv * F(1.05)).astype(F)
    sigma = 0.0371
    path = str(tmp_path / "DepthRadialResolution.dat")
    depth.write_radial_resolution(path, c, res, vsv, vsh, sigma)
    rows = depth.read_radial_resolution(path)
    assert len(rows) == M * ncol and sorted(rows[0]) == sorted(("lon", "lat", "depth") + depth.RADIAL_RESOLUTION_NAMES)
    flat = lambda a: np.asarray(a).reshape(-1).tolist()
    v = vsv[:M].astype(np.float64); hh = vsh[:M].astype(np.float64)
    for q, blk in (("v", slice(0, M)), ("h", slice(M, 2 * M))):
        assert [r["rjj_" + q] for r in rows] == flat(m[0][blk])
        assert [r["length_" + q] for r in rows] == flat(np.sqrt(np.divide(m[2][blk], m[1][blk], out=np.zeros((M, ncol)), where=m[1][blk] > 0)))
        tot = m[1][blk] + m[3][blk]
        assert [r["leak_" + q] for r in rows] == flat(np.divide(m[3][blk], tot, out=np.zeros((M, ncol)), where=tot > 0))
        assert [r["sd_" + q] for r in rows] == flat(sigma * np.sqrt(m[5][blk]))
    assert rows[7]["length_v"] == 0.0 and rows[7]["leak_v"] == 0.0 and rows[0]["leak_h"] == 0.0
    assert [r["r_aniso"] for r in rows] == flat(0.5 * (m[0][:M] + m[0][M:] - m[4][:M] - m[4][M:]))
    assert [r["sd_diff"] for r in rows] == flat(sigma * np.sqrt(pair[1]))
    xi = (hh / v) ** 2
    rad = np.maximum(m[5][:M] / (v * v) + m[5][M:] / (hh * hh) - 2.0 * pair[0] / (v * hh), 0.0)
    assert np.allclose([r["sd_xi"] for r in rows], flat(2.0 * xi * sigma * np.sqrt(rad)), rtol=1e-15, atol=0.0)
    assert rows[ncol + 9]["sd_xi"] == 0.0 and rows[8]["sd_xi"] > 0.0                # clamped at 0
    assert [r["depth"] for r in rows[::ncol]] == [0.0, 2.0]                        # the bottom depth has no line
    lon, lat = maps._lonlat(c, 0, 0)
    k = 1 * nx + 1
    assert rows[k]["lon"] == float(lon) and rows[k]["lat"] == float(lat)           # node order: Depth.dat's
    with open(path) as fh:
        assert re.search(r"\d\.\d{15,16}(e[-+]\d+)?\b", fh.read())               # 17 significant digits
    again = str(tmp_path / "again.dat")
    io.write_table(again, depth.RADIAL_RESOLUTION_TABLE, rows)
    assert depth.read_radial_resolution(again) == rows                             # the round trip loses nothing
    lpath = str(tmp_path / "DepthRadialLeverage.dat")
    depth.write_radial_leverage(lpath, c, res["leverage"])
    lrows = depth.read_radial_leverage(lpath)
    assert len(lrows) == nm * ncol and lrows == depth.read_leverage(lpath)         # DepthLeverage.dat's layout
    per = maps.period_list(c)
    assert [(r["wave"], r["kind"], r["period"]) for r in lrows[:nm]] == per
    assert [r["leverage"] for r in lrows] == res["leverage"].T.ravel().tolist()
    assert depth.leak_share([0.0, 3.0, 0.0], [0.0, 1.0, 2.0]).tolist() == [0.0, 0.25, 1.0]


def test_summary_of_the_log(taipei):
    c = small_case(taipei)
    nx, ny, M = 6, 5, 2
    ncol = nx * ny
    inner = R.interior(nx, ny) == 1
    flag = np.zeros(ncol, np.int32); trace = np.zeros((2, ncol)); measures = np.zeros((6, 2 * M, ncol)); pair = np.zeros((2, M, ncol))
    trace[0, inner] = np.linspace(1.0, 2.1, inner.sum()); trace[1, inner] = np.linspace(0.2, 0.5, inner.sum())
    measures[1] = 3.0; measures[3, :M] = 1.0; measures[3, M:] = 9.0                # leak shares 0.25 (Vsv) and 0.75 (Vsh)
    measures[5] = 1e-4                                                             # var: sd_xi = 2 xi S sqrt(2e-4 / 9)
    flag[1 * nx + 1] = 2; flag[1 * nx + 2] = 1                                   # two interior columns flagged: not in the statistics
    vsv = np.full((M + 1, ncol), 3.0, F); vsh = vsv.copy()
    vsh[0, 2 * nx + 3] = 3.3; vsh[1, 1 * nx + 1] = 3.3                             # one clear xi anomaly in a resolved column, one in a flagged one
    res = dict(flag=flag, trace=trace, measures=measures, pair=pair)
    sm = depth.radial_resolution_summary(c, res, vsv, vsh, 0.05)
    ok = inner & (flag == 0)
    assert (sm["flagged1"], sm["flagged2"], sm["columns"], sm["nodes"]) == (1, 1, 10, 20) and ok.sum() == 10
    for q, name in enumerate(("trace_v", "trace_h")):
        assert sm[name] == (float(np.median(trace[q][ok])), float(trace[q][ok].min()), float(trace[q][ok].max()))
    assert (sm["leak_v"], sm["leak_h"]) == (0.25, 0.75)
    assert sm["significant"] == 1                                                  # xi = 1.21 against 2 sd_xi = 0.0011; xi = 1 is never significant
    lines = depth.radial_resolution_log(c, sm)
    assert len(lines) == 4 and "10 columns resolved, 2 flagged (1 not positive definite, 1 without data)" in lines[0]
    assert "Vsv block" in lines[1] and "median leak share 0.2500" in lines[1] and "Vsh block" in lines[2] and "median leak share 0.7500" in lines[2]
    assert "|xi - 1| > 2 sd_xi at 1 of 20 unflagged nodes" in lines[3]
    flag[:] = 2
    sm = depth.radial_resolution_summary(c, res, vsv, vsh, 0.05)
    assert sm["trace_v"] is None and sm["significant"] == 0 and len(depth.radial_resolution_log(c, sm)) == 1


def test_new_symbol_declared_bound_and_exported():
    """declared in the public header, argtypes set by engine.py on both kinds of handle (load_library's and a bare CDLL through
    declare_solvers), an Engine method, exported by the built library; the new header is in the build's list"""
    from dsurftomo_amd import build
    from dsurftomo_amd import engine as E
    build.build()
    with open(os.path.join(L.ROOT, "include", "dsurftomo_amd.h")) as fh:
        header = fh.read()
    assert re.search(r"^int %s\(dsa_engine\* e, int nmaps, const float\* obs, const float\* wt, float smooth, float damp, float aniso,\s*double\* measures, "
                     r"double\* pair, double\* leverage, double\* trace, int\* nused, int\* flag, double\* R\);" % NEW, header, re.M)
    lib = E.load_library()
    bare = E.declare_solvers(C.CDLL(build.LIB))
    for handle in (lib, bare):
        assert len(getattr(handle, NEW).argtypes) == 14
    assert callable(E.Engine.columns_resolution_radial)
    assert "column_radial_resolution.h" in build.HEADERS and "column_resolution.h" in build.HEADERS and "column_radial.h" in build.HEADERS
    assert os.path.exists(os.path.join(L.ROOT, "dsurftomo_amd", "csrc", "column_radial_resolution.h"))
    assert len(lib.dsa_columns_resolution.argtypes) == 12 and len(lib.dsa_columns_step_radial.argtypes) == 14      # the neighbours are as they were


@pytest.mark.parametrize("nz", [3, 8])
def test_twin_and_header_on_the_oracles_curves(nz):
    """tests/test_gpu_columns.py's smooth model, 5 x 5, its 12 periods, Vsh 3 % above Vsv, the curves and kernels from the oracle's
    depthkernel (Love on Vsh, Rayleigh on Vsv): the CPU build of the header against the twin within the measured tolerance in every
    interior column, the twin's own two answers printed; the sum of the leverages is the sum of the traces, more damping resolves less,
    nothing is flagged"""
    h = RS.load()
    hs = R.load()
    depz = R.depths(nz)
    vsv = R.smooth_model(R.NX, R.NY, nz)
    vsh = np.array(vsv, F, copy=True)
    vsh[:-1] = (vsh[:-1] * F(1.03)).astype(F)
    ncol = R.NX * R.NY
    love = RR.LOVE
    pv, svs, svp, srho = RR.oracle_curves_radial(vsv, vsh, depz)
    Sv = R.host_combine(hs, vsv.reshape(nz, ncol), depz, svs, svp, srho)
    Sh = R.host_combine(hs, vsh.reshape(nz, ncol), depz, svs, svp, srho)
    obs = pv.astype(F)
    inner = np.flatnonzero(R.interior(R.NX, R.NY))
    ring = R.interior(R.NX, R.NY) == 0
    assert (pv[:, inner] > 0).all()
    traces = {}
    for damp in (0.05, 0.5):
        got = RS.host_resolution(h, love, obs, None, pv, Sv, Sh, depz, vsv.reshape(nz, ncol), vsh.reshape(nz, ncol), R.SMOOTH, damp, RR.ANISO, R.interior(R.NX, R.NY))
        assert not got["flag"].any() and (got["nused"][:, inner] == R.K // 2).all()
        worst = 0.0
        for c in inner:
            S = np.where(love[:, None], Sh[:, :, c].T, Sv[:, :, c].T)
            twin = depth.column_radial_resolution_twin(obs[:, c], None, pv[:, c], S, love, depz, R.SMOOTH, damp, RR.ANISO)
            rmax = np.abs(twin["other"]["R"]).max()
            worst = max(worst, np.abs(twin["R"] - twin["other"]["R"]).max() / rmax)
            one = {k: v[..., c] for k, v in got.items()}
            assert twin["flag"] == 0 and max(RS.differences(one, twin, rmax).values()) <= RS.TOL
            assert abs(one["leverage"].sum() - one["trace"].sum()) <= RS.TOL * rmax
            assert (one["leverage"] > 0).all() and (one["leverage"] < 1).all() and (one["measures"][5] > 0).all() and (one["pair"][1] > 0).all()
        traces[damp] = got["trace"][:, inner].sum(axis=0)
        assert not got["trace"][:, ring].any() and not got["R"][:, :, ring].any()
        print("nz %d damp %g: sum of the two traces %.4f to %.4f; the twin's ldlt against pinv at most %.3g" % (nz, damp, traces[damp].min(), traces[damp].max(), worst))
    assert (traces[0.5] < traces[0.05]).all() and (traces[0.05] < 2 * (nz - 1)).all() and (traces[0.5] > 0).all()
