"""The host side of the maps' resolution, no GPU: maps --resolution's files and their round trips, the two
propagation formulas against a central-difference Jacobian, the refusals of both drivers before the library is loaded, depth --map-sigma's
weights and where they go (test_depth_driver_replay.py's recording engine), the new symbol in the header, the binding and the built library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _libs as L
import columns_ref as R
import test_depth_azimuthal_patterns as DA
import test_depth_driver_replay as DR
from dsurftomo_amd import depth, io, maps

F = np.float32
NEW = "dsa_maps_resolution"
NX, NY, NZ, NMAPS = DR.NX, DR.NY, DR.NZ, DR.NMAPS
LAYER = (NX - 2) * (NY - 2)
INNER = R.interior(NX, NY) == 1


def made_up_result(nblocks, seed=4):
    """what Engine.maps_resolution returns, of the small case's shape: map 2 flagged 1"""
    rng = np.random.default_rng(seed)
    meas = rng.random((9, nblocks, NMAPS, LAYER))
    meas[1] *= 1e-2
    meas[8] = 0.3 * np.sqrt(meas[1] * np.roll(meas[1], -1, axis=0)) * np.sign(rng.random(meas[8].shape) - 0.5)
    flag = np.zeros(NMAPS, np.int32); flag[2] = 1
    meas[:, :, 2] = 0.0
    return dict(measures=meas, flag=flag, nused=np.full(NMAPS, 7, np.int32), trace=meas[0].sum(axis=2), leverage=rng.random(30))


def columns_of(c, nblocks, sigma=(0.5, 0.6, 0.7, 0.8)):
    rng = np.random.default_rng(9)
    velv = (3.0 + rng.random((NMAPS, NX * NY))).astype(F)
    a1 = 0.1 * (rng.random((NMAPS, LAYER)) - 0.5); a2 = 0.1 * (rng.random((NMAPS, LAYER)) - 0.5)
    a1[0, 3] = a2[0, 3] = 0.0
    res = made_up_result(nblocks)
    return res, velv, a1, a2, maps.resolution_columns(c, res, np.array(sigma), velv, a1, a2)


@pytest.mark.parametrize("nblocks", [1, 3])
def test_resolution_file_round_trip(tmp_path, nblocks):
    c = DR.small_case()
    res, velv, a1, a2, cols = columns_of(c, nblocks)
    path = str(tmp_path / "MapsResolution.dat")
    maps.write_maps_resolution(path, c, cols)
    rows = maps.read_maps_resolution(path, azimuthal=nblocks == 3)
    table = maps.RESOLUTION_AZI_TABLE if nblocks == 3 else maps.RESOLUTION_TABLE
    assert len(rows) == NMAPS * LAYER and list(rows[0]) == [n for n, _, _ in table[1]]
    assert list(rows[0])[:13] == ["wave", "kind", "period", "lon", "lat", "rjj", "psf_x", "psf_y", "share", "sd_unit", "sd", "sigma", "flag"]
    flat = lambda a: np.asarray(a, np.float64).reshape(-1).tolist()
    for name in cols:
        assert [r[name] for r in rows] == (np.asarray(cols[name]).reshape(-1).tolist() if name == "flag" else flat(cols[name])), name
    m = res["measures"]
    assert [r["rjj"] for r in rows] == flat(m[0, 0]) and [r["sd_unit"] for r in rows] == flat(np.sqrt(m[1, 0]))
    sig = np.repeat([0.5, 0.6, 0.7, 0.8], LAYER)
    assert [r["sigma"] for r in rows] == sig.tolist() and np.allclose([r["sd"] for r in rows], sig * np.sqrt(m[1, 0]).ravel(), rtol=1e-15)
    assert [r["flag"] for r in rows] == np.repeat(res["flag"], LAYER).tolist()
    dx = maps.EARTH_RADIUS_KM * np.radians(float(c["dvxd"]))
    ok = m[2, 0] > 0
    assert np.allclose(np.array([r["psf_x"] for r in rows]).reshape(NMAPS, LAYER)[ok], np.sqrt(m[3, 0][ok] / m[2, 0][ok]) * dx, rtol=1e-14)
    lat = np.array([r["lat"] for r in rows]).reshape(NMAPS, LAYER)
    dy = maps.EARTH_RADIUS_KM * np.radians(float(c["dvzd"])) * np.cos(np.radians(lat))
    assert np.allclose(np.array([r["psf_y"] for r in rows]).reshape(NMAPS, LAYER)[ok], (np.sqrt(m[4, 0][ok] / m[2, 0][ok]) * dy[ok]), rtol=1e-14)
    assert all(r["psf_x"] == r["psf_y"] == r["share"] == r["sd"] == 0.0 for r in rows[2 * LAYER:3 * LAYER])      # the flagged map: zeros, no NaN
    if nblocks == 3:
        s2 = sig.reshape(NMAPS, LAYER) ** 2
        assert np.allclose(np.array([r["cov_a12"] for r in rows]).reshape(NMAPS, LAYER), s2 * m[8, 1], rtol=1e-15)
        assert np.allclose(np.array([r["sd_a2"] for r in rows]).reshape(NMAPS, LAYER), np.sqrt(s2 * m[1, 2]), rtol=1e-15)
        assert rows[3]["sd_strength"] == 0.0 and rows[3]["sd_axis"] == 0.0             # A1 = A2 = 0: 0, not NaN
        assert np.isfinite([[r["sd_strength"], r["sd_axis"]] for r in rows]).all()
        plain = str(tmp_path / "Plain.dat")                                            # the plain file asked for the 2psi columns
        maps.write_maps_resolution(plain, c, {k: v for k, v in cols.items() if k in [n for n, _, _ in maps.RESOLUTION_TABLE[1]]})
        assert "rjj_a1" not in maps.read_maps_resolution(plain)[0]
        with pytest.raises(ValueError, match=re.escape(plain)):
            maps.read_maps_resolution(plain, azimuthal=True)
    with open(path) as fh:
        assert re.search(r"\d\.\d{15,16}(e[-+]\d+)?\b", fh.read())                   # 17 significant digits


def test_leverage_file_round_trip(tmp_path):
    rng = np.random.default_rng(2)
    dmap = rng.integers(0, NMAPS, 30); w = (rng.random(30) > 0.2).astype(F); lev = rng.random(30) * w
    path = str(tmp_path / "MapsLeverage.dat")
    maps.write_maps_leverage(path, dmap, w, lev)
    rows = maps.read_maps_leverage(path)
    assert [r["datum"] for r in rows] == list(range(30)) and [r["map"] for r in rows] == dmap.tolist()
    assert [r["weight"] for r in rows] == w.astype(np.float64).tolist() and [r["leverage"] for r in rows] == lev.tolist()


def test_the_propagation_formulas_against_a_central_difference_jacobian():
    """var = J C J^T with J the central-difference Jacobian of strength_percent and fast_axis in (A1, A2), c0 known"""
    rng = np.random.default_rng(6)
    for _ in range(20):
        c0, a1, a2 = 3.0 + rng.random(), 0.2 * (rng.random() - 0.5), 0.2 * (rng.random() - 0.5)
        s1, s2 = 0.01 * (0.5 + rng.random()), 0.01 * (0.5 + rng.random())
        c12 = 0.8 * (rng.random() - 0.5) * 2 * s1 * s2
        Cm = np.array([[s1 * s1, c12], [c12, s2 * s2]])
        h = 1e-6
        Js = np.array([(maps.strength_percent(c0, a1 + h, a2) - maps.strength_percent(c0, a1 - h, a2)) / (2 * h),
                       (maps.strength_percent(c0, a1, a2 + h) - maps.strength_percent(c0, a1, a2 - h)) / (2 * h)])
        Ja = np.radians([(maps.fast_axis(a1 + h, a2) - maps.fast_axis(a1 - h, a2)) / (2 * h), (maps.fast_axis(a1, a2 + h) - maps.fast_axis(a1, a2 - h)) / (2 * h)])
        assert np.isclose(maps.strength_variance(c0, a1, a2, s1 * s1, s2 * s2, c12), Js @ Cm @ Js, rtol=1e-6)
        assert np.isclose(maps.axis_variance(a1, a2, s1 * s1, s2 * s2, c12), Ja @ Cm @ Ja, rtol=1e-6)
    assert maps.strength_variance(3.0, 0.0, 0.0, 1.0, 1.0, 0.0) == 0.0 and maps.axis_variance(0.0, 0.0, 1.0, 1.0, 0.0) == 0.0
    v = maps.axis_variance(np.array([0.0, 0.1]), np.array([0.0, 0.0]), 1e-4, 4e-4, 0.0)
    assert v[0] == 0.0 and np.isclose(v[1], 0.25 * 4e-4 * 0.01 / 1e-4)


def refuse(*_):
    raise AssertionError("the library was loaded")


@pytest.mark.parametrize("argv", [["--resolution", "--sigma-time", "0"], ["--resolution", "--sigma-time", "-0.5"], ["--resolution", "--sigma-time", "nan"],
                                  ["--sigma-time", "0.5"]])
def test_maps_cli_refuses_before_the_library(monkeypatch, tmp_path, argv):
    import dsurftomo_amd.engine as E
    monkeypatch.setattr(E, "load_library", refuse)
    monkeypatch.setattr(io, "load", refuse)
    with pytest.raises(SystemExit) as exc:
        maps.main([str(tmp_path)] + argv)
    assert exc.value.code == 2
    with pytest.raises(ValueError, match="--sigma-time"):
        a = maps.parser().parse_args([str(tmp_path)] + argv)
        maps.run(str(tmp_path), resolution=a.resolution, sigma_time=a.sigma_time)
    a = maps.parser().parse_args(["dir"])
    assert (a.resolution, a.sigma_time, a.iterations, a.dvmax, a.azimuthal) == (False, None, 3, 0.5, False)
    maps.check(resolution=True, sigma_time=0.3)
    maps.check(resolution=True)


def test_depth_refuses_a_file_without_the_columns_before_the_library(monkeypatch, tmp_path):
    """--map-sigma on a Maps.dat, on a plain MapsResolution.dat with --azimuthal, on a missing file: exit 2 from main(), a ValueError naming
    the file from run(), the library never loaded and the input never read"""
    import dsurftomo_amd.engine as E
    c = DR.small_case()
    monkeypatch.setattr(E, "load_library", refuse)
    monkeypatch.setattr(E, "Engine", refuse)
    monkeypatch.setattr(io, "load", refuse)
    mpath = str(tmp_path / "Maps.dat")
    DR.write_maps(mpath, c)
    plain = str(tmp_path / "PlainResolution.dat")
    maps.write_maps_resolution(plain, c, columns_of(c, 1)[4])
    for path, extra in ((mpath, []), (plain, ["--azimuthal"]), (str(tmp_path / "missing.dat"), [])):
        with pytest.raises(SystemExit) as exc:
            depth.main([str(tmp_path), "--map-sigma", path] + extra)
        assert exc.value.code == 2
        with pytest.raises(ValueError, match=re.escape(path)):
            depth.run(str(tmp_path), map_sigma=path, azimuthal=bool(extra))
    a = depth.parser().parse_args(["dir"])
    assert a.map_sigma is None
    keywords = [k for _, k, _, _ in depth.OPTIONS]
    assert keywords.index("sigma") < keywords.index("map_sigma") < keywords.index("radial")
    assert [s[0] for s in depth.STAGES] == ["depth resolution", "depth lateral resolution", None, "depth sample", "depth radial resolution"]      # no new stage


def sd_file(tmp_path, c, nblocks=3):
    path = str(tmp_path / "MapsResolution.dat")
    cols = columns_of(c, nblocks)[4]
    maps.write_maps_resolution(path, c, cols)
    return path, cols


def test_map_sigma_weights(tmp_path):
    c = DR.small_case()
    path, cols = sd_file(tmp_path, c)
    rows = maps.read_maps_resolution(path)
    wt, ref = depth.map_sigma_weights(rows, c)
    assert wt.shape == (NMAPS, NY * NX) and wt.dtype == F
    sd = np.zeros((NMAPS, NY, NX)); sd[:, 1:-1, 1:-1] = cols["sd"].reshape(NMAPS, NY - 2, NX - 2)
    sd = sd.reshape(NMAPS, -1)
    keep = np.tile(INNER, (NMAPS, 1)) & (sd > 0)
    keep[2] = False                                                                   # the flagged map
    assert ref == np.median(sd[keep]) > 0
    assert np.array_equal(wt > 0, keep) and not wt[2].any() and not wt[:, ~INNER].any()
    assert np.array_equal(wt[keep], (ref / sd[keep]).astype(F))
    w = np.sort(wt[keep].astype(np.float64))                                          # the median weight is 1: the middle weight, or the
    assert w[(w.size - 1) // 2] <= 1.0 <= w[w.size // 2]                              # two middle ones on either side of it (an even count)
    odd = depth.map_sigma_weights(rows, c, np.arange(NMAPS * NY * NX).reshape(NMAPS, -1) != np.flatnonzero(keep.ravel())[0])[0]
    assert (odd > 0).sum() % 2 == 1 and np.median(odd[odd > 0]) == 1.0
    mask = np.ones((NMAPS, NY * NX), bool); mask[0] = False; mask[1, INNER.nonzero()[0][:3]] = False
    wt2, ref2 = depth.map_sigma_weights(rows, c, mask)
    assert not wt2[0].any() and np.array_equal(wt2 > 0, keep & mask) and ref2 == np.median(sd[keep & mask])
    wa, refa = depth.map_sigma_weights(rows, c, None, azimuthal=True)
    sda = np.sqrt(0.5 * (cols["sd_a1"] ** 2 + cols["sd_a2"] ** 2))
    assert refa == np.median(sda[[0, 1, 3]]) and np.array_equal(wa[1][INNER], (refa / sda[1]).astype(F))
    with pytest.raises(ValueError, match="lines"):
        depth.map_sigma_weights(rows[:-1], c)
    swapped = [dict(r) for r in rows]
    swapped[LAYER]["period"] = 99.0
    with pytest.raises(ValueError, match="map 1"):
        depth.map_sigma_weights(swapped, c)
    assert depth.map_sigma_weights([dict(r, flag=2) for r in rows], c)[1] == 0.0      # nothing kept: no weights, reference 0


def test_map_sigma_reaches_every_stage(tmp_path, monkeypatch):
    """with --map-sigma every stage's wt is sigma_ref / sd under the --min-dws mask, the 2psi stage's its own; without --sigma the stages
    take sigma_ref (the log says so) and the sampler's weights are 1 / sd"""
    c = DR.small_case()
    path, cols = sd_file(tmp_path, c)
    (out, _, _), calls, lines, _, _, case = DA.driven(tmp_path, monkeypatch, azimuthal=True, resolution=True, sample="4,10", min_dws=4.0, iterations=2, map_sigma=path)
    rows = maps.read_maps(str(tmp_path / "Maps.dat"))
    obs, dws = depth.maps_to_obs(rows, case)
    mask = depth.dws_weights(dws, 4.0) > 0
    sd_rows = maps.read_maps_resolution(path)
    wt, ref = depth.map_sigma_weights(sd_rows, case, mask)
    wt_azi, _ = depth.map_sigma_weights(sd_rows, case, mask, azimuthal=True)
    assert 0 < (wt > 0).sum() < (np.tile(INNER, (NMAPS, 1))).sum() and not np.array_equal(wt, wt_azi)
    by_name = {}
    for call in calls:
        by_name.setdefault(call[0], []).append(call)
    assert len(by_name["columns_step"]) == 2
    for call in by_name["columns_step"] + by_name["columns_resolution"]:
        assert call[1][1] == DR.encode(wt), call[0]
    assert by_name["columns_azimuthal"][0][1][3] == DR.encode(wt_azi)
    w, lam = depth.sample_scaling(wt, depth.DEFAULT_SMOOTH, ref, obs.shape)
    begin = by_name["columns_sample_begin"][0][1]
    assert begin[5] == DR.encode(w) and begin[7] == lam == depth.DEFAULT_SMOOTH / ref
    sd = np.zeros((NMAPS, NY, NX)); sd[:, 1:-1, 1:-1] = cols["sd"].reshape(NMAPS, NY - 2, NX - 2)
    sd = sd.reshape(NMAPS, -1)
    kept = wt > 0
    assert np.allclose(w[kept], 1.0 / sd[kept], rtol=3 * np.finfo(F).eps) and not w[~kept].any()       # 1 / sd, two fp32 roundings
    text = "\n".join(lines)
    assert text.count("--map-sigma's reference") == 2 and "sigma_ref %.6f" % ref in text and "weights of the 2psi stage" in text
    assert "the rms before the last step, " not in text
    # --sigma still wins
    (_, _, _), calls2, lines2, _, _, _ = DA.driven(tmp_path, monkeypatch, resolution=True, sigma=0.04, map_sigma=path)
    assert "the data's standard deviation is --sigma 0.040000" in "\n".join(lines2) and "--map-sigma's reference" not in "\n".join(lines2)
    assert [c_ for c_ in calls2 if c_[0] == "columns_step"][0][1][1] == DR.encode(depth.map_sigma_weights(sd_rows, case)[0])


def test_without_the_option_the_calls_are_the_recorded_ones(tmp_path):
    import json
    with open(DR.GOLDEN) as fh:
        golden = json.load(fh)
    for name in ("sample_all", "min_dws"):
        sub = tmp_path / name
        sub.mkdir()
        rec = DR.replay(DR.RUNS[name], str(sub), "run")
        assert rec["calls"] == golden[name]["calls"] and rec["log"] == golden[name]["log"]


def test_the_symbol_is_exported_declared_and_bound():
    with open(os.path.join(L.ROOT, "include", "dsurftomo_amd.h")) as fh:
        header = fh.read()
    assert re.search(r"\bint %s\(dsa_engine\* e, int nx, int ny, int nmaps, int nblocks, int ndata, float damp, int r_map," % NEW, header)
    from dsurftomo_amd import build, engine
    assert "map_kernels.hip" in build.SOURCES and "map_resolution.h" in build.HEADERS
    lib = C.CDLL(build.build())
    assert getattr(lib, NEW) is not None
    engine.declare_solvers(lib)
    assert len(getattr(lib, NEW).argtypes) == 14
    assert callable(engine.Engine.maps_resolution)
