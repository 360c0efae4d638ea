"""The host side of the depth inversion of the maps' 2 psi terms (dsurftomo_amd/depth.py --azimuthal), no GPU: the new
flags and what they leave alone, the refusals before the library is loaded and before the input is read, maps_to_azimuthal on a maps file
with and without the azimuthal columns, what the stage calls and in which order (test_depth_driver_replay.py's recording engine with the new
method), the stage before the sample stage, the two files' round trips, the sd_axis cap, the new symbol in the header, the binding and the
built library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _libs as L
import columns_ref as R
import test_depth_driver_replay as DR
from dsurftomo_amd import depth, io, maps
from dsurftomo_amd.analyses import azimuthal as AZ

F = np.float32
NEW = "dsa_columns_azimuthal"
NX, NY, NZ, NMAPS = DR.NX, DR.NY, DR.NZ, DR.NMAPS
LAYER = (NX - 2) * (NY - 2)


class AzimuthalEngine(DR.RecordingEngine):
    """the recording engine with the new call: gc, gs of a few per cent, one interior column without data and one not positive definite"""

    @DR.recorded
    def columns_azimuthal(self, obs, a1, a2, wt, smooth, damp):
        rng = self._rng()
        flag = self._flags()
        ok = self.inner & (flag == 0)
        measures = rng.random((4, self.M, self.ncol)) * ok
        measures[0, 1] *= 0.05                                                        # the deepest unknown is not resolved: the log names the depth
        measures[3] *= 1e-3
        nused = np.where(ok, 3, 0).astype(np.int32)
        chi2 = 1e-4 * rng.random((4, self.ncol)) * ok
        chi2[2:] *= 0.1
        g = 0.04 * (rng.random((2, self.M, self.ncol)) - 0.5) * ok
        return dict(gc=g[0], gs=g[1], measures=measures, leverage=rng.random((NMAPS, self.ncol)) * ok, chi2=chi2, nused=nused, flag=flag)


def write_maps(path, c, azimuthal=True):
    rng = np.random.default_rng(3)
    velv = (3.0 + rng.random((NMAPS, NX * NY))).astype(F)
    norm = (10.0 * rng.random(NMAPS * LAYER)).astype(F)
    a1 = 0.1 * (rng.random((NMAPS, LAYER)) - 0.5)
    a2 = 0.1 * (rng.random((NMAPS, LAYER)) - 0.5)
    maps.write_maps(path, c, velv, norm, *((a1, a2) if azimuthal else ()))
    return a1, a2


def driven(tmp_path, monkeypatch, azimuthal_maps=True, **kw):
    """depth.run on the small case with the recording engine; returns (result, calls, log lines, a1, a2 as written)"""
    import dsurftomo_amd.engine as E
    case = DR.small_case()
    calls, lines = [], []

    class Engine(AzimuthalEngine):
        pass
    Engine.calls = calls
    monkeypatch.setattr(io, "load", lambda *_: case)
    monkeypatch.setattr(E, "Engine", Engine)
    mpath = str(tmp_path / "Maps.dat")
    a1, a2 = write_maps(mpath, case, azimuthal_maps)
    out = depth.run("case", maps_file=mpath, out_dir=str(tmp_path), log=lines.append, **kw)
    return out, calls, lines, a1, a2, case


def test_parser_defaults_and_old_attributes():
    a = depth.parser().parse_args(["dir"])
    assert (a.azimuthal, a.azimuthal_smooth, a.azimuthal_damp, a.azimuthal_sigma) == (False, None, None, None)
    assert (a.maps, a.iterations, a.smooth, a.damp, a.dvmax, a.min_dws, a.out, a.resolution, a.sigma, a.sample) == (None, 4, 0.5, 0.1, 0.5, 0.0, ".", False, None, None)
    a = depth.parser().parse_args(["dir", "--azimuthal", "--azimuthal-smooth", "0.2", "--azimuthal-damp", "0.05", "--azimuthal-sigma", "0.01"])
    assert (a.azimuthal, a.azimuthal_smooth, a.azimuthal_damp, a.azimuthal_sigma, a.smooth, a.damp) == (True, 0.2, 0.05, 0.01, 0.5, 0.1)
    keywords = [k for _, k, _, _ in depth.OPTIONS]
    assert keywords.index("lateral_checkerboard") < keywords.index("azimuthal") < keywords.index("sample")
    labels = [s[0] for s in depth.STAGES if not s[1]]
    assert labels == ["depth resolution", "depth lateral resolution", None, "depth sample"]       # after the resolutions, before the sample stage


BAD = [["--azimuthal", "--radial"], ["--azimuthal-smooth", "0.2"], ["--azimuthal-damp", "0.2"], ["--azimuthal-sigma", "0.2"], ["--azimuthal", "--azimuthal-smooth", "-1"],
       ["--azimuthal", "--azimuthal-smooth", "nan"], ["--azimuthal", "--azimuthal-damp", "0"], ["--azimuthal", "--azimuthal-damp", "inf"],
       ["--azimuthal", "--azimuthal-sigma", "0"], ["--azimuthal", "--azimuthal-sigma", "nan"]]


@pytest.mark.parametrize("argv", BAD)
def test_cli_refuses_before_the_library(monkeypatch, tmp_path, argv):
    import dsurftomo_amd.engine as E

    def refuse(*_):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(E, "load_library", refuse)
    monkeypatch.setattr(io, "load", refuse)
    with pytest.raises(SystemExit) as exc:
        depth.main([str(tmp_path)] + argv)
    assert exc.value.code == 2


@pytest.mark.parametrize("kw, match", [(dict(azimuthal=True, radial=True), "--radial"), (dict(azimuthal_smooth=0.1), "--azimuthal-smooth needs"),
                                       (dict(azimuthal_damp=0.1), "--azimuthal-damp needs"), (dict(azimuthal_sigma=0.1), "--azimuthal-sigma needs"),
                                       (dict(azimuthal=True, azimuthal_damp=0.0), "--azimuthal-damp"), (dict(azimuthal=True, azimuthal_smooth=-0.1), "--azimuthal-smooth"),
                                       (dict(azimuthal=True, azimuthal_sigma=float("inf")), "--azimuthal-sigma")])
def test_run_refuses_before_the_input_is_read(monkeypatch, tmp_path, kw, match):
    def refuse(*_):
        raise AssertionError("the input was read")
    monkeypatch.setattr(io, "load", refuse)
    with pytest.raises(ValueError, match=match):
        depth.run(str(tmp_path), **kw)
    depth.check_azimuthal(True, False, 0.0, 0.05, 0.01)
    depth.check_azimuthal(True)
    depth.check_azimuthal(False)


def test_maps_to_azimuthal(tmp_path):
    c = DR.small_case()
    path = str(tmp_path / "Maps.dat")
    a1, a2 = write_maps(path, c)
    rows = maps.read_maps(path)
    g1, g2 = depth.maps_to_azimuthal(rows, c)
    obs, _ = depth.maps_to_obs(rows, c)
    assert g1.shape == g2.shape == obs.shape == (NMAPS, NY * NX) and g1.dtype == g2.dtype == F
    inner = R.interior(NX, NY) == 1
    assert not g1[:, ~inner].any() and not g2[:, ~inner].any()                       # the ring: zeros, as maps_to_obs's
    assert np.array_equal(g1[:, inner], a1.astype(F)) and np.array_equal(g2[:, inner], a2.astype(F))      # (17 digits in the file: the fp64 values come back)
    plain = str(tmp_path / "Plain.dat")
    write_maps(plain, c, azimuthal=False)
    with pytest.raises(ValueError, match="a1 / a2"):
        depth.maps_to_azimuthal(maps.read_maps(plain), c)
    with pytest.raises(ValueError, match="lines"):
        depth.maps_to_azimuthal(rows[:-1], c)
    swapped = [dict(r) for r in rows]
    swapped[0]["period"] = 99.0
    with pytest.raises(ValueError, match="map 0"):
        depth.maps_to_azimuthal(swapped, c)


def test_a_maps_file_without_the_columns_is_refused_by_name(tmp_path, monkeypatch):
    import dsurftomo_amd.engine as E

    def refuse(*_):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(E, "load_library", refuse)
    monkeypatch.setattr(E, "Engine", refuse)
    case = DR.small_case()
    monkeypatch.setattr(io, "load", lambda *_: case)
    plain = str(tmp_path / "Plain.dat")
    write_maps(plain, case, azimuthal=False)
    with pytest.raises(ValueError, match=re.escape(plain)):
        depth.run("case", maps_file=plain, out_dir=str(tmp_path), azimuthal=True)


def test_what_the_stage_calls_and_in_which_order(tmp_path, monkeypatch):
    """after the loop: the plan's runs with kernels once more, then one columns_azimuthal with the c0 maps, A1, A2, the loop's weights and
    --smooth / --damp; nothing else before close; the two files and the entries of the result; the log"""
    (out, path, fit), calls, lines, a1, a2, c = driven(tmp_path, monkeypatch, azimuthal=True, iterations=2, min_dws=4.0)
    names = [call[0] for call in calls]
    plan = depth.slot_plan(c)
    per_iteration = ["dispersion_run"] * len(plan) + ["columns_step"]
    assert names == ["Engine", "dispersion_begin"] + per_iteration * 2 + ["dispersion_get_model"] + ["dispersion_run"] * len(plan) + ["columns_azimuthal", "close"]
    rows = maps.read_maps(str(tmp_path / "Maps.dat"))
    obs, dws = depth.maps_to_obs(rows, c)
    g1, g2 = depth.maps_to_azimuthal(rows, c)
    wt = depth.dws_weights(dws, 4.0)
    assert calls[-2][1] == DR.encode((obs, g1, g2, wt, depth.DEFAULT_SMOOTH, depth.DEFAULT_DAMP))
    for call, (wave, kind, t, first) in zip(calls[-2 - len(plan):-2], plan):
        assert call[1] == DR.encode((wave, kind, t, True, first, first))
    assert {"azimuthal", "azimuthal_sigma", "azimuthal_summary", "azimuthal_path", "azimuthal_fit_path"} <= set(out)
    res = out["azimuthal"]
    assert out["azimuthal_sigma"] == depth.azimuthal_sigma(res["chi2"], res["nused"]) == np.sqrt((res["chi2"][2] + res["chi2"][3]).sum() / (2 * res["nused"].sum()))
    assert os.path.basename(out["azimuthal_path"]) == "DSurfTomo.inDepthAzim.dat" and os.path.basename(out["azimuthal_fit_path"]) == "DSurfTomo.inDepthAzimFit.dat"
    assert os.path.exists(path) and os.path.exists(fit)                                # Depth.dat and DepthFit.dat as without the flag
    text = "\n".join(lines)
    for words in ("depth azimuthal: 10 columns solved, 2 flagged (1 not positive definite, 1 without data)", "rms of (A1, A2)", "the rms of the fit's residual",
                  "strength median", "exceeds 2 sd_g at", "median R_jj per depth", "stays under 0.1 from 2 km down", "DSurfTomo.inDepthAzim.dat"):
        assert words in text, words
    assert "the data's standard deviation" not in text                              # (--sigma's line belongs to the other stages)
    sm = out["azimuthal_summary"]
    ok = (R.interior(NX, NY) == 1) & (res["flag"] == 0)
    st = AZ.azimuthal_strength(res["gc"], res["gs"])[:, ok]
    assert sm["strength"] == (float(np.median(st)), float(st.max())) and 0.0 <= sm["significant"] <= 1.0 and len(sm["rjj"]) == NZ - 1


def test_the_options_reach_the_call_and_the_stage_runs_before_the_sample_stage(tmp_path, monkeypatch):
    (out, _, _), calls, lines, _, _, _ = driven(tmp_path, monkeypatch, azimuthal=True, azimuthal_smooth=0.2, azimuthal_damp=0.03, azimuthal_sigma=0.004, resolution=True,
                                                sample="4,10", iterations=1)
    names = [call[0] for call in calls]
    assert names.index("columns_resolution") < names.index("columns_azimuthal") < names.index("columns_sample_begin")
    call = calls[names.index("columns_azimuthal")]
    assert call[1][3] is None and call[1][4:] == [0.2, 0.03]                          # no --min-dws: no weights; the stage's own smooth and damp
    assert out["azimuthal_sigma"] == 0.004 and "--azimuthal-sigma" in "\n".join(lines)
    rows = depth.read_azimuthal(out["azimuthal_path"])
    var = out["azimuthal"]["measures"][3].ravel()
    assert [r["sd_g"] for r in rows] == (0.004 * np.sqrt(var)).tolist()


def test_files_round_trip(tmp_path):
    c = DR.small_case()
    M, ncol = NZ - 1, NX * NY
    rng = np.random.default_rng(5)
    res = dict(gc=0.04 * (rng.random((M, ncol)) - 0.5), gs=0.04 * (rng.random((M, ncol)) - 0.5), measures=rng.random((4, M, ncol)), chi2=1e-3 * rng.random((4, ncol)),
               nused=rng.integers(0, 5, ncol).astype(np.int32), flag=rng.integers(0, 3, ncol).astype(np.int32))
    res["measures"][1, 0, 7] = 0.0                                                   # m1 = 0: the length is written as 0
    res["gc"][1, 3] = res["gs"][1, 3] = 0.0                                          # no amplitude: the axis' sd is the cap
    vels = (3.0 + rng.random((NZ, NY, NX))).astype(F)
    sigma = 0.0123
    path = str(tmp_path / "DepthAzim.dat")
    depth.write_azimuthal(path, c, vels, res, sigma)
    rows = depth.read_azimuthal(path)
    assert len(rows) == M * ncol and list(rows[0]) == [n for n, _, _ in depth.AZIMUTHAL_TABLE[1]]
    flat = lambda a: np.asarray(a, np.float64).reshape(-1).tolist()
    assert [r["gc"] for r in rows] == flat(res["gc"]) and [r["gs"] for r in rows] == flat(res["gs"])
    assert [r["vs"] for r in rows] == flat(vels[:M])
    assert [r["strength"] for r in rows] == flat(AZ.azimuthal_strength(res["gc"], res["gs"])) == flat(50.0 * np.hypot(res["gc"], res["gs"]))
    assert [r["axis"] for r in rows] == flat(AZ.azimuthal_axis(res["gc"], res["gs"]))
    assert [r["rjj"] for r in rows] == flat(res["measures"][0])
    assert [r["length"] for r in rows] == flat(depth.psf_length(res["measures"][1], res["measures"][2])) and rows[7]["length"] == 0.0
    sd_g = sigma * np.sqrt(res["measures"][3])
    assert [r["sd_g"] for r in rows] == flat(sd_g) and [r["sd_strength"] for r in rows] == flat(50.0 * sd_g)
    assert [r["sd_axis"] for r in rows] == flat(depth.azimuthal_sd_axis(res["gc"], res["gs"], sd_g)) and rows[ncol + 3]["sd_axis"] == depth.SD_AXIS_CAP
    assert [r["depth"] for r in rows[::ncol]] == [float(z) for z in c["depz"][:M]]      # the bottom depth has no line
    with open(path) as fh:
        assert re.search(r"\d\.\d{15,16}(e[-+]\d+)?\b", fh.read())                   # 17 significant digits
    fpath = str(tmp_path / "DepthAzimFit.dat")
    depth.write_azimuthal_fit(fpath, c, res)
    rows = depth.read_azimuthal_fit(fpath)
    assert len(rows) == ncol and [r["nused"] for r in rows] == res["nused"].tolist() and [r["flag"] for r in rows] == res["flag"].tolist()
    n = 2.0 * res["nused"]
    for key, q in (("rms_before", 0), ("rms_after", 2)):
        want = np.sqrt(np.divide(res["chi2"][q] + res["chi2"][q + 1], n, out=np.zeros(ncol), where=n > 0))
        assert [r[key] for r in rows] == want.tolist()
    lon, lat = maps._lonlat(c, 0, 0)
    assert rows[NX + 1]["lon"] == float(lon) and rows[NX + 1]["lat"] == float(lat)   # column order: DepthFit.dat's


def test_the_sd_axis_cap():
    cap = 90.0 / np.sqrt(3.0)
    assert depth.SD_AXIS_CAP == cap
    sd = depth.azimuthal_sd_axis([0.02, 0.0, 0.0, 1e-6, -0.03], [0.0, 0.02, 0.0, 0.0, 0.04], [0.001, 0.002, 0.001, 0.001, 0.0])
    assert sd[0] == (90.0 / np.pi) * 0.001 / 0.02 and sd[1] == (90.0 / np.pi) * 0.002 / 0.02
    assert sd[2] == cap and sd[3] == cap and sd[4] == 0.0                            # no amplitude; an amplitude far below its sd; no variance
    assert depth.azimuthal_sd_axis(0.0, 0.0, 0.0) == cap
    assert (depth.azimuthal_sd_axis(np.full(3, 0.01), np.zeros(3), [0.0, 0.01, 1.0]) <= cap).all()


def test_new_symbol_declared_bound_and_exported():
    """declared in the public header, argtypes set by engine.py on both kinds of handle (load_library's and a bare CDLL through
    declare_solvers), an Engine method, exported by the built library; the new header is in the build's list; the neighbours are as they were"""
    from dsurftomo_amd import build
    from dsurftomo_amd import engine as E
    build.build()
    with open(os.path.join(L.ROOT, "include", "dsurftomo_amd.h")) as fh:
        header = fh.read()
    assert re.search(r"^int %s\(dsa_engine\* e, int nmaps, const float\* obs, const float\* a1, const float\* a2, const float\* wt, float smooth, float damp,\s*"
                     r"double\* g, double\* measures, double\* leverage, double\* chi2, int\* nused, int\* flag\);" % NEW, header, re.M)
    lib = E.load_library()
    bare = E.declare_solvers(C.CDLL(build.LIB))
    for handle in (lib, bare):
        assert len(getattr(handle, NEW).argtypes) == 14
    assert callable(E.Engine.columns_azimuthal)
    assert "column_azimuthal.h" in build.HEADERS and os.path.exists(os.path.join(L.ROOT, "dsurftomo_amd", "csrc", "column_azimuthal.h"))
    assert len(lib.dsa_columns_step.argtypes) == 13 and len(lib.dsa_columns_resolution.argtypes) == 12
    assert callable(depth.column_azimuthal_twin) and callable(depth.azimuthal_factor)
