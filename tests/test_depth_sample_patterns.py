"""The host side of the Monte-Carlo depth inversion (dsurftomo_amd/depth.py --sample), no GPU: the new flags and what
they leave alone, the refusals before the library is loaded, the scaling by sigma, the two files' round trips, the log's R-hat summary, the
new symbols in the header, the binding and the built library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _libs as L
import columns_ref as R
from dsurftomo_amd import depth, io, maps

F = np.float32
NEW = ("dsa_columns_sample_begin", "dsa_columns_sample_run", "dsa_columns_sample_fetch", "dsa_columns_sample_state")


@pytest.fixture(scope="module")
def taipei():
    return io.load()


def small_case(taipei):
    return dict(taipei, nx=6, ny=5, nz=3, depz=np.array([0.0, 2.0, 5.0], F), tRc=np.array([4.0, 6.5]), tRg=np.array([5.0]), tLc=np.zeros(0), tLg=np.array([8.0]), kmax=4)


def test_parser_defaults_and_old_attributes():
    a = depth.parser().parse_args(["dir"])
    assert (a.sample, a.sample_step, a.sample_spread, a.sample_width, a.sample_seed, a.sample_temperature) == (None, 0.05, 0.05, 0.5, 1, 1.0)
    assert (a.maps, a.iterations, a.smooth, a.damp, a.dvmax, a.min_dws, a.out, a.resolution, a.sigma, a.radial, a.lateral) == (None, 4, 0.5, 0.1, 0.5, 0.0, ".", False, None, False, None)
    a = depth.parser().parse_args(["dir", "--sample", "64,1000", "--sample-step", "0.1", "--sample-seed", "9", "--sigma", "0.02"])
    assert (a.sample, a.sample_step, a.sample_seed, a.sigma) == ("64,1000", 0.1, 9, 0.02)
    assert depth.parse_sample("64,1000") == (64, 1000, 500) and depth.parse_sample("3,7") == (3, 7, 3) and depth.parse_sample("1,5,5") == (1, 5, 5)
    assert depth.parse_sample("2,9,0") == (2, 9, 0)
    assert depth.check_sample(None, radial=True, lateral=1.0) is None                # without the flag nothing is looked at


@pytest.mark.parametrize("argv", [["--sample", "64"], ["--sample", "0,100"], ["--sample", "4,0"], ["--sample", "4,10,11"], ["--sample", "4,10,-1"], ["--sample", "a,b"],
                                  ["--sample", "4,10,2,1"], ["--sample", "4.5,10"], ["--sample", "4,10", "--radial"], ["--sample", "4,10", "--lateral", "0.5"],
                                  ["--sample", "4,10", "--sample-step", "0"], ["--sample", "4,10", "--sample-step", "nan"], ["--sample", "4,10", "--sample-spread", "-1"],
                                  ["--sample", "4,10", "--sample-width", "0"], ["--sample", "4,10", "--sample-temperature", "-2"], ["--sample", "4,10", "--sample-seed", "-3"],
                                  ["--sample", "4,10", "--sigma", "0"]])
def test_cli_refuses_before_the_library(monkeypatch, tmp_path, argv):
    import dsurftomo_amd.engine as E

    def refuse(*_):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(E, "load_library", refuse)
    monkeypatch.setattr(io, "load", refuse)
    with pytest.raises(SystemExit) as exc:
        depth.main([str(tmp_path)] + argv)
    assert exc.value.code == 2


@pytest.mark.parametrize("kw,match", [(dict(sample="4,10", radial=True), "--radial"), (dict(sample="4,10", lateral=0.3), "--lateral"), (dict(sample="4"), "--sample"),
                                      (dict(sample="4,10", sample_step=0.0), "--sample-step"), (dict(sample="4,10", sample_spread=-0.1), "--sample-spread"),
                                      (dict(sample="4,10", sample_width=float("inf")), "--sample-width"), (dict(sample="4,10", sample_temperature=0.0), "--sample-temperature")])
def test_run_refuses_before_the_input_is_read(monkeypatch, tmp_path, kw, match):
    def refuse(*_):
        raise AssertionError("the input was read")
    monkeypatch.setattr(io, "load", refuse)
    with pytest.raises(ValueError, match=match):
        depth.run(str(tmp_path), **kw)


def test_sigma_scales_the_weights_and_the_prior():
    w, lam = depth.sample_scaling(None, 0.5, 0.02, (3, 4))
    assert w.dtype == F and w.shape == (3, 4) and (w == F(1.0 / 0.02)).all() and lam == 0.5 / 0.02
    mask = np.array([[1, 0, 1, 1], [0, 0, 1, 1], [1, 1, 1, 0]], F)
    w, lam = depth.sample_scaling(mask, 2.0, 0.04, (3, 4))
    assert (w[mask == 0] == 0).all() and (w[mask == 1] == F(25.0)).all() and lam == 50.0
    # the posterior of a linear column under (w, lam) is the step's normal matrix at unit weights, over sigma^2: the balance is kept
    rng = np.random.default_rng(1)
    S = rng.random((5, 3)); LtL = depth.column_ltl(3)
    N1 = S.T @ S + 0.5 ** 2 * LtL
    w, lam = depth.sample_scaling(None, 0.5, 0.02, (5, 1))
    N2 = S.T @ (w.astype(np.float64) ** 2 * S) + lam ** 2 * LtL
    assert np.allclose(N2 * 0.02 ** 2, N1, rtol=1e-6)


class FakeEngine:
    """what run_sample calls, with a made-up result"""

    def __init__(self, nx, ny, nz):
        self.shape, self.calls = (nx, ny, nz), []

    def columns_sample_begin(self, *args):
        self.calls.append(("begin", args))

    def columns_sample_run(self, n):
        self.calls.append(("run", n))

    def columns_sample_fetch(self):
        return fake_result(*self.shape)


def fake_result(nx, ny, nz, kept=6):
    M, ncol = nz - 1, nx * ny
    rng = np.random.default_rng(2)
    inner = R.interior(nx, ny) == 1
    res = dict(mean=3.0 + rng.random((M, ncol)), var=0.01 * rng.random((M, ncol)), W=0.01 * (0.5 + rng.random((M, ncol))), B=0.001 * rng.random((M, ncol)),
               best=3.0 + rng.random((M, ncol)), phi_start=80 * rng.random(ncol), best_energy=3 * rng.random(ncol), mean_phi=6 * rng.random(ncol),
               nused=np.full(ncol, 4, np.int32), flag=np.zeros(ncol, np.int32), accepted=np.full(ncol, 30, np.int32), rejected=np.full(ncol, 70, np.int32),
               out_of_box=np.full(ncol, 5, np.int32), no_root=np.full(ncol, 2, np.int32), reseeded=np.zeros(ncol, np.int32), nkept=np.full(ncol, kept, np.int32))
    res["var"][0, 8] = -1e-18                                                      # a rounding-negative variance: sd 0
    dead = ~inner
    dead[1 * nx + 2] = True                                                        # an interior column without data
    res["flag"][1 * nx + 2] = 2
    for name in ("mean", "var", "W", "B", "best"):
        res[name][:, dead] = 0.0
    for name in ("best_energy", "mean_phi", "phi_start"):
        res[name][dead] = 0.0
    for name in ("nused", "accepted", "rejected", "out_of_box", "no_root", "nkept"):
        res[name][dead] = 0
    res["reseeded"][1 * nx + 3] = 2
    return res


def test_posterior_files_round_trip(tmp_path, taipei):
    c = small_case(taipei)
    nx, ny, nz = 6, 5, 3
    M = nz - 1
    res = fake_result(nx, ny, nz)
    start = (3.0 + np.random.default_rng(3).random((nz, ny, nx))).astype(F)
    path = str(tmp_path / "DepthPosterior.dat")
    depth.write_posterior(path, c, start, res)
    rows = depth.read_posterior(path)
    assert len(rows) == M * ny * nx and [r["depth"] for r in rows[::nx * ny]] == [0.0, 2.0]      # the bottom depth has no line
    v0 = start.astype(np.float64).reshape(nz, -1)[:M].ravel()
    kept = np.tile(res["nkept"] > 0, M)
    assert [r["start"] for r in rows] == v0.tolist()
    assert [r["mean"] for r in rows] == np.where(kept, res["mean"].ravel(), v0).tolist() and [r["best"] for r in rows] == np.where(kept, res["best"].ravel(), v0).tolist()
    sd = np.sqrt(np.maximum(res["var"], 0.0)).ravel()
    assert [r["sd"] for r in rows] == sd.tolist() and rows[8]["sd"] == 0.0 and rows[0]["sd"] == 0.0
    n = 6.0
    rhat = np.where(kept, np.sqrt((res["W"].ravel() * (n - 1.0) / n + res["B"].ravel()) / np.where(kept, res["W"].ravel(), 1.0)), 1.0)
    assert np.array_equal([r["rhat"] for r in rows], rhat) and rows[0]["rhat"] == 1.0 and rows[1 * nx + 2]["mean"] == v0[1 * nx + 2]
    lon, lat = maps._lonlat(c, 0, 0)
    k = 1 * nx + 1
    assert rows[k]["lon"] == float(lon) and rows[k]["lat"] == float(lat)           # node order: Depth.dat's
    with open(path) as fh:
        assert re.search(r"\d\.\d{15,16}(e[-+]\d+)?\b", fh.read())               # 17 significant digits
    fpath = str(tmp_path / "DepthPosteriorFit.dat")
    depth.write_posterior_fit(fpath, c, res)
    rows = depth.read_posterior_fit(fpath)
    assert len(rows) == ny * nx
    assert [r["phi_start"] for r in rows] == res["phi_start"].tolist() and [r["phi_best"] for r in rows] == res["best_energy"].tolist()
    assert [r["phi_mean"] for r in rows] == res["mean_phi"].tolist() and [r["nused"] for r in rows] == res["nused"].tolist()
    assert (rows[k]["accepted"], rows[k]["out_of_box"], rows[k]["no_root"]) == (0.3, 0.05, 0.02) and rows[0]["accepted"] == 0.0
    assert rows[1 * nx + 2]["flag"] == 2 and rows[1 * nx + 3]["reseeded"] == 2 and rows[k]["lon"] == float(lon)


def test_summary_of_the_log_and_the_driver(tmp_path, taipei):
    c = small_case(taipei)
    nx, ny, nz = 6, 5, 3
    res = fake_result(nx, ny, nz)
    sm = depth.rhat_summary(res)
    r = depth.sample_rhat(res["W"], res["B"], res["nkept"][None])[:, res["nkept"] > 0]
    assert sm == dict(unknowns=r.size, median=float(np.median(r)), worst=float(r.max()), above=float((r > 1.1).mean())) and sm["unknowns"] == 2 * 11
    assert depth.rhat_summary(dict(res, nkept=np.zeros(nx * ny, np.int32))) is None
    assert depth.sample_rhat([0.0, 2.0], [1.0, 2.0], [4, 4]).tolist() == [1.0, float(np.sqrt((2.0 * 0.75 + 2.0) / 2.0))]
    eng = FakeEngine(nx, ny, nz)
    lines = []
    start = np.full((nz, ny, nx), 3.0, F)
    obs = np.full((4, ny * nx), 3.0, F)
    mask = np.ones((4, ny * nx), F); mask[2, 9] = 0.0
    plan = depth.slot_plan(c)
    out = depth.run_sample(eng, c, plan, start, obs, mask, 0.5, 0.025, (8, 40, 10), str(tmp_path), 0.07, 0.03, 0.6, 5, 2.0, lines.append)
    (name, args), (_, n) = eng.calls
    assert name == "begin" and n == 40 and len(eng.calls) == 2
    assert args[0] is start and args[3] is plan and args[4] is obs and args[6:] == (8, 0.5 / 0.025, 0.07, 0.03, 0.6, 2.0, float(c["minvel"]), float(c["maxvel"]), 5, 10)
    assert args[5].dtype == F and args[5][2, 9] == 0 and (args[5][mask == 1] == F(40.0)).all()
    assert os.path.exists(out["posterior_path"]) and os.path.exists(out["posterior_fit_path"]) and out["sample_sigma"] == 0.025 and out["rhat"] == sm
    text = "\n".join(lines)
    assert "R-hat of 22 unknowns median %.4f, worst %.4f, %.1f %% above 1.1" % (sm["median"], sm["worst"], 100 * sm["above"]) in text
    assert "8 chains x 40 sweeps (30 kept)" in text and "1 columns without data" in text and "2 chains put back" in text


def test_new_symbols_declared_bound_and_exported():
    """declared in the public header, argtypes set by engine.py on both kinds of handle, Engine methods, exported by the built library; the
    new header is in the build's list and holds the arithmetic's names"""
    from dsurftomo_amd import build
    from dsurftomo_amd import engine as E
    build.build()
    with open(os.path.join(L.ROOT, "include", "dsurftomo_amd.h")) as fh:
        header = fh.read()
    for name in NEW:
        assert re.search(r"^int %s\(dsa_engine\* e[,)]" % name, header, re.M), name
    lib = E.load_library()
    bare = E.declare_solvers(C.CDLL(build.LIB))
    for handle in (lib, bare):
        assert [len(getattr(handle, n).argtypes) for n in NEW] == [25, 2, 4, 15]
    for method in ("columns_sample_begin", "columns_sample_run", "columns_sample_fetch", "columns_sample_state"):
        assert callable(getattr(E.Engine, method))
    assert "column_sample.h" in build.HEADERS
    with open(os.path.join(L.ROOT, "dsurftomo_amd", "csrc", "column_sample.h")) as fh:
        text = fh.read()
    for name in ("sample_mix", "sample_bits", "sample_neglog", "sample_propose", "sample_accept", "sample_finish", "sample_setup_models", "sample_setup_state"):
        assert re.search(r"\b%s\(" % name, text), name
    assert not re.search(r"\b(sqrt|log|exp|pow)\s*\(", re.sub(r"//.*", "", text))            # no libm call and no square root in the code
    with open(os.path.join(L.ROOT, "dsurftomo_amd", "csrc", "column_kernels.hip")) as fh:
        kernels = fh.read()
    for name in ("k_sample_setup", "k_sample_propose", "k_sample_accept", "k_sample_finish"):
        assert re.search(r"__global__ void __launch_bounds__\(kSampleBlock\) %s\(" % name, kernels), name
    assert len(lib.dsa_columns_step.argtypes) == 13 and len(lib.dsa_dispersion_begin_models.argtypes) == 9      # the old entry points are as they were
    assert callable(depth.column_sample_twin)
