"""The host side of the depth inversion of the period maps (dsurftomo_amd/depth.py), no GPU: the slot plan against the
input file's own order, the maps file as observations, the DWS mask, the files' round trips, the command line's refusals, the new symbols in
the header, the binding and the built library -- and the Gauss-Newton loop of tests/test_gpu_columns.py run on the CPU build of the step
with the oracle's dispersion routine in place of the device's, which is where its perturbation, smooth and damp were chosen."""
import os
import re

import numpy as np
import pytest

import _libs as L
import columns_ref as R
from dsurftomo_amd import depth, io, maps

F = np.float32
NEW = ("dsa_columns_step", "dsa_dispersion_get_model")


@pytest.fixture(scope="module")
def taipei():
    return io.load()


def small_case(taipei):
    return dict(taipei, nx=6, ny=5, nz=3, depz=np.array([0.0, 2.0, 5.0], F), tRc=np.array([4.0, 6.5]), tRg=np.array([5.0]), tLc=np.zeros(0), tLg=np.array([8.0]), kmax=4)


def test_slot_plan_is_the_maps_period_order(taipei):
    """one run per wave type present; map_first = sen_slot = the type's first slot in maps.period_list's order"""
    plan = depth.slot_plan(taipei)
    assert [(w, k, f) for w, k, _, f in plan] == [(2, 0, 0)] and plan[0][2].tolist() == taipei["tRc"].tolist() and len(plan[0][2]) == taipei["kmax"] == 26
    c = small_case(taipei)
    plan = depth.slot_plan(c)
    assert [(w, k, t.tolist(), f) for w, k, t, f in plan] == [(2, 0, [4.0, 6.5], 0), (2, 1, [5.0], 2), (1, 1, [8.0], 3)]
    per = maps.period_list(c)
    for w, k, t, f in plan:
        assert per[f:f + len(t)] == [(w, k, float(x)) for x in t]
    assert sum(len(t) for _, _, t, _ in plan) == len(per)


def test_maps_file_becomes_observations(tmp_path, taipei):
    """maps.write_maps -> maps.read_maps -> maps_to_obs: the interior of every map where get_maps has it, zeros on the ring; a file of other
    periods or of another grid is refused"""
    c = small_case(taipei)
    nm, nx, ny = 4, 6, 5
    rng = np.random.default_rng(3)
    velv = (3.0 + rng.random((nm, nx * ny))).astype(F)
    norm = (10.0 * rng.random(nm * (nx - 2) * (ny - 2))).astype(F)
    path = str(tmp_path / "Maps.dat")
    maps.write_maps(path, c, velv, norm)
    obs, dws = depth.maps_to_obs(maps.read_maps(path), c)
    assert obs.shape == dws.shape == (nm, nx * ny) and obs.dtype == F
    v = velv.reshape(nm, ny, nx); o = obs.reshape(nm, ny, nx); d = dws.reshape(nm, ny, nx)
    assert np.array_equal(o[:, 1:-1, 1:-1], v[:, 1:-1, 1:-1]) and np.array_equal(d[:, 1:-1, 1:-1].ravel(), norm.astype(np.float64))
    ring = np.ones((ny, nx), bool); ring[1:-1, 1:-1] = False
    assert not o[:, ring].any() and not d[:, ring].any()
    with pytest.raises(ValueError, match="is not wave"):
        depth.maps_to_obs(maps.read_maps(path), dict(c, tRc=np.array([4.0, 7.0])))
    with pytest.raises(ValueError, match="lines"):
        depth.maps_to_obs(maps.read_maps(path), dict(c, nx=7))
    # the mask: weight 0 below the threshold, 1 at and above it
    w = depth.dws_weights(dws, 4.0)
    assert w.dtype == F and set(np.unique(w).tolist()) == {0.0, 1.0}
    assert np.array_equal(w == 0, dws < 4.0) and (w[:, ring.ravel()] == 0).all() and (depth.dws_weights(dws, 0.0) == 1).all()
    assert (depth.dws_weights(np.array([3.9999, 4.0, 4.0001]), 4.0) == np.array([0, 1, 1], F)).all()


def test_depth_files_round_trip(tmp_path, taipei):
    c = small_case(taipei)
    nx, ny, nz = 6, 5, 3
    rng = np.random.default_rng(8)
    vels = (2.0 + 2.0 * rng.random((nz, ny, nx))).astype(F)
    path = str(tmp_path / "Depth.dat")
    depth.write_depth(path, c, vels)
    rows = depth.read_depth(path)
    assert len(rows) == nx * ny * nz
    assert [r["vs"] for r in rows] == vels.ravel().astype(np.float64).tolist()
    assert [r["depth"] for r in rows[::nx * ny]] == [0.0, 2.0, 5.0]
    lon, lat = maps._lonlat(c, 0, 0)
    k = 1 * nx + 1                                                                 # node (1, 1): the first interior vertex of the maps file
    assert rows[k]["lon"] == float(lon) and rows[k]["lat"] == float(lat)
    assert rows[1]["lat"] < rows[0]["lat"] and rows[1]["lon"] == rows[0]["lon"] and rows[nx]["lon"] > rows[0]["lon"]
    step = lambda seed: dict(nused=np.random.default_rng(seed).integers(0, 5, nx * ny).astype(np.int32), chi2=np.random.default_rng(seed).random(nx * ny),
                             flag=np.random.default_rng(seed).integers(0, 3, nx * ny).astype(np.int32))
    first, last = step(1), step(2)
    fit = str(tmp_path / "DepthFit.dat")
    depth.write_fit(fit, c, first, last)
    rows = depth.read_fit(fit)
    assert len(rows) == nx * ny
    assert [r["nused"] for r in rows] == last["nused"].tolist() and [r["flag"] for r in rows] == last["flag"].tolist()
    for r, n0, x0, n1, x1 in zip(rows, first["nused"], first["chi2"], last["nused"], last["chi2"]):
        assert r["rms_first"] == (float(np.sqrt(x0 / n0)) if n0 else 0.0) and r["rms_last"] == (float(np.sqrt(x1 / n1)) if n1 else 0.0)
    assert depth.rms_of([1.0, 3.0], [2, 2]) == 1.0 and depth.rms_of([0.0], [0]) == 0.0


def test_parser_defaults():
    a = depth.parser().parse_args(["dir"])
    assert (a.maps, a.iterations, a.smooth, a.damp, a.dvmax, a.min_dws, a.out) == (None, 4, 0.5, 0.1, 0.5, 0.0, ".")
    a = depth.parser().parse_args(["dir", "--maps", "m.dat", "--iterations", "2", "--smooth", "1", "--damp", "0.3", "--dvmax", "0.2", "--min-dws", "5"])
    assert (a.maps, a.iterations, a.smooth, a.damp, a.dvmax, a.min_dws) == ("m.dat", 2, 1.0, 0.3, 0.2, 5.0)


@pytest.mark.parametrize("argv", [["--iterations", "0"], ["--smooth", "-1"], ["--smooth", "nan"], ["--damp", "0"], ["--damp", "-0.5"], ["--damp", "inf"],
                                  ["--dvmax", "0"], ["--dvmax", "nan"], ["--min-dws", "-1"], ["--min-dws", "nan"]])
def test_cli_refuses_before_the_library(monkeypatch, tmp_path, argv):
    import dsurftomo_amd.engine as E

    def refuse(*_):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(E, "load_library", refuse)
    monkeypatch.setattr(io, "load", refuse)
    with pytest.raises(SystemExit) as exc:
        depth.main([str(tmp_path)] + argv)
    assert exc.value.code == 2


@pytest.mark.parametrize("kw", [dict(iterations=0), dict(smooth=-1.0), dict(damp=0.0), dict(damp=float("nan")), dict(dvmax=-0.5), dict(min_dws=-2.0)])
def test_run_refuses_before_the_input_is_read(monkeypatch, tmp_path, kw):
    def refuse(*_):
        raise AssertionError("the input was read")
    monkeypatch.setattr(io, "load", refuse)
    with pytest.raises(ValueError):
        depth.run(str(tmp_path), **kw)


def test_run_refuses_a_missing_or_foreign_maps_file_before_the_library(monkeypatch, tmp_path, taipei):
    import dsurftomo_amd.engine as E

    def refuse(*_):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(E, "load_library", refuse)
    with pytest.raises(FileNotFoundError):
        depth.run(io.HERE, out_dir=str(tmp_path))
    c = small_case(taipei)
    path = str(tmp_path / "Maps.dat")
    maps.write_maps(path, c, np.full((4, 30), 3.0, F), np.ones(4 * 12, F))
    with pytest.raises(ValueError, match="lines"):
        depth.run(io.HERE, maps_file=path, out_dir=str(tmp_path))


def test_twin_regulariser():
    """column_l as the issue states it, and what it does not penalise: a constant"""
    assert depth.column_l(1).shape == (0, 1)
    assert depth.column_l(2).tolist() == [[1.0, -1.0], [-1.0, 1.0]]
    assert depth.column_l(4).tolist() == [[1.0, -1.0, 0.0, 0.0], [0.0, 0.0, -1.0, 1.0], [-1.0, 2.0, -1.0, 0.0], [0.0, -1.0, 2.0, -1.0]]
    for M in (2, 3, 9):
        assert not (depth.column_l(M) @ np.ones(M)).any() and (depth.column_ltl(M) == depth.column_ltl(M).T).all()


def test_loop_on_the_oracles_dispersion():
    """tests/test_gpu_columns.py's loop (c) at nz = 3 with the oracle's depthkernel for the curves and kernels and the CPU build of the
    step: the sum of chi2 before the last step is below the one before the first (nz = 2, 3, 8 give 0.1685 -> 0.0935, 0.0971 -> 0.0890,
    0.2673 -> 0.0063 km^2/s^2 here), every step moves the model, nothing is flagged"""
    h = R.load()
    nz = 3
    depz = R.depths(nz)
    truth = R.smooth_model(R.NX, R.NY, nz)
    obs = R.oracle_curves(truth, depz)[0].astype(F)
    start = R.perturbed(truth)
    assert 0.02 < np.abs(start / truth - 1.0).max() <= 0.0301
    seen = []
    model, chi2, rms = R.loop(h, start, depz, obs, lambda m: R.oracle_curves(m, depz), after=lambda it, m, inputs, out: seen.append((out["flag"].copy(), np.abs(out["dv"]).max())))
    print("rms before each step:", " ".join("%.6f" % r for r in rms))
    assert len(chi2) == R.ITERATIONS and chi2[-1] < chi2[0]
    assert all(not f.any() and d > 0 for f, d in seen)
    ring = R.interior(R.NX, R.NY) == 0
    assert np.array_equal(model.reshape(nz, -1)[:, ring], start.reshape(nz, -1)[:, ring]) and np.array_equal(model[nz - 1], start[nz - 1])


def test_new_symbols_declared_bound_and_exported():
    """the two entry points: declared in the public header, argtypes set by engine.py on both kinds of handle, Engine methods present,
    exported by the built library; the new sources are in the build's lists"""
    from dsurftomo_amd import build
    from dsurftomo_amd import engine as E
    build.build()
    with open(os.path.join(L.ROOT, "include", "dsurftomo_amd.h")) as fh:
        header = fh.read()
    lib = E.load_library()
    for name in NEW:
        assert re.search(r"^int %s\(dsa_engine\* e" % name, header, re.M), name
        assert getattr(lib, name).argtypes, name
    assert len(lib.dsa_columns_step.argtypes) == 13
    for method in ("columns_step", "dispersion_get_model"):
        assert callable(getattr(E.Engine, method))
    assert "column_kernels.hip" in build.SOURCES and "column_system.h" in build.HEADERS
    assert os.path.exists(os.path.join(L.ROOT, "dsurftomo_amd", "csrc", "column_system.h"))
