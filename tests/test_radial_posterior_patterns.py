"""The host side of the Monte-Carlo radial depth inversion (dsurftomo_amd/radial_posterior.py), no GPU: the command
line and its refusals before the library is loaded, the scaling of the weights, smooth and aniso by sigma, the two files' round trips, the
log's summary, the driver on a made-up engine, the new symbols in the header, the binding and the built library, and what depth.py keeps:
its STAGES and its refusal of --sample with --radial."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _libs as L
import columns_ref as R
from dsurftomo_amd import depth, depth_twins, io, maps
from dsurftomo_amd import radial_posterior as RP

F = np.float32
NEW = ("dsa_columns_sample_radial_begin", "dsa_columns_sample_radial_run", "dsa_columns_sample_radial_fetch", "dsa_columns_sample_radial_state")
NODES = ("mean_v", "var_v", "W_v", "B_v", "mean_h", "var_h", "W_h", "B_h", "mean_xi", "var_xi", "W_xi", "B_xi", "best_v", "best_h", "cov_vh", "p_pos")


@pytest.fixture(scope="module")
def taipei():
    return io.load()


def small_case(taipei):
    return dict(taipei, nx=6, ny=5, nz=3, depz=np.array([0.0, 2.0, 5.0], F), tRc=np.array([4.0, 6.5]), tRg=np.array([5.0]), tLc=np.zeros(0), tLg=np.array([8.0]), kmax=4)


def test_parser_defaults():
    a = RP.parser().parse_args(["dir"])
    assert (a.sample, a.maps, a.model, a.smooth, a.aniso, a.sigma, a.min_dws, a.map_sigma, a.out, a.no_pairs) == (None, None, None, 0.5, 0.2, None, 0.0, None, ".", False)
    assert (a.sample_step, a.sample_spread, a.sample_width, a.sample_seed, a.sample_temperature) == (0.05, 0.05, 0.5, 1, 1.0)
    assert (a.smooth, a.aniso) == (depth.DEFAULT_SMOOTH, depth.DEFAULT_ANISO)
    a = RP.parser().parse_args(["dir", "--sample", "64,1000", "--no-pairs", "--aniso", "0.4", "--model", "m.dat"])
    assert (a.sample, a.no_pairs, a.aniso, a.model) == ("64,1000", True, 0.4, "m.dat")
    assert RP.check("64,1000") == (64, 1000, 500) and RP.check("3,7,7", aniso=0.0, smooth=0.0) == (3, 7, 7)


@pytest.mark.parametrize("argv", [[], ["--sample", "64"], ["--sample", "0,100"], ["--sample", "4,0"], ["--sample", "4,10,11"], ["--sample", "a,b"],
                                  ["--sample", "4,10", "--sample-step", "0"], ["--sample", "4,10", "--sample-step", "nan"], ["--sample", "4,10", "--sample-spread", "-1"],
                                  ["--sample", "4,10", "--sample-width", "0"], ["--sample", "4,10", "--sample-temperature", "-2"], ["--sample", "4,10", "--sample-seed", "-3"],
                                  ["--sample", "4,10", "--sigma", "0"], ["--sample", "4,10", "--sigma", "nan"], ["--sample", "4,10", "--aniso", "-0.1"],
                                  ["--sample", "4,10", "--aniso", "inf"], ["--sample", "4,10", "--smooth", "-1"], ["--sample", "4,10", "--min-dws", "-1"],
                                  ["--sample", "4,10", "--map-sigma", "MAPSIGMA"]])
def test_cli_refuses_before_the_library(monkeypatch, tmp_path, argv):
    import dsurftomo_amd.engine as E

    def refuse(*_):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(E, "load_library", refuse)
    monkeypatch.setattr(io, "load", refuse)
    bad = tmp_path / "MapsResolution.dat"
    bad.write_text("# lon lat\n1 2\n")                                            # a --map-sigma file without the needed columns
    argv = [str(bad) if a == "MAPSIGMA" else a for a in argv]
    with pytest.raises(SystemExit) as exc:
        RP.main([str(tmp_path)] + argv)
    assert exc.value.code == 2


@pytest.mark.parametrize("kw,match", [(dict(sample=None), "--sample"), (dict(sample="4"), "--sample"), (dict(sample="4,10", aniso=-1.0), "--aniso"),
                                      (dict(sample="4,10", sigma=0.0), "--sigma"), (dict(sample="4,10", sample_step=0.0), "--sample-step"),
                                      (dict(sample="4,10", sample_width=float("inf")), "--sample-width")])
def test_run_refuses_before_the_input_is_read(monkeypatch, tmp_path, kw, match):
    def refuse(*_):
        raise AssertionError("the input was read")
    monkeypatch.setattr(io, "load", refuse)
    kw = dict(kw)
    with pytest.raises(ValueError, match=match):
        RP.run(str(tmp_path), kw.pop("sample"), **kw)


def test_sigma_scales_the_weights_the_smoothing_and_the_tie():
    w, lam, gam = RP.sample_scaling(None, 0.5, 0.2, 0.02, (3, 4))
    assert w.dtype == F and w.shape == (3, 4) and (w == F(1.0 / 0.02)).all() and lam == 0.5 / 0.02 and gam == 0.2 / 0.02
    mask = np.array([[1, 0, 1, 1], [0, 0, 1, 1], [1, 1, 1, 0]], F)
    w, lam, gam = RP.sample_scaling(mask, 2.0, 0.0, 0.04, (3, 4))
    assert (w[mask == 0] == 0).all() and (w[mask == 1] == F(25.0)).all() and lam == 50.0 and gam == 0.0
    w0, lam0 = depth.sample_scaling(mask, 2.0, 0.04, (3, 4))                     # the old function is what it was
    assert np.array_equal(w, w0) and lam == lam0
    # the posterior precision of a linear column under (w, lam, gam) is the radial step's normal matrix at unit weights, over sigma^2
    rng = np.random.default_rng(1)
    K, M, sigma = 6, 3, 0.02
    S = rng.random((K, M)); love = np.arange(K) % 2 == 1
    used = np.ones(K, bool); rho = np.zeros(K); d = np.zeros(M)
    N1, _ = depth_twins._twin_radial_normal(S, used, love, rho, 0.5 ** 2, 0.0, 0.2 ** 2, d)
    w, lam, gam = RP.sample_scaling(None, 0.5, 0.2, sigma, (K, 1))
    N2, _ = depth_twins._twin_radial_normal(w.astype(np.float64) * S, used, love, rho, lam ** 2, 0.0, gam ** 2, d)
    assert np.allclose(N2 * sigma ** 2, N1, rtol=1e-6)


def fake_result(nx, ny, nz, kept=6):
    M, ncol = nz - 1, nx * ny
    rng = np.random.default_rng(2)
    inner = R.interior(nx, ny) == 1
    res = {n: 0.01 * (0.5 + rng.random((M, ncol))) for n in NODES}
    for n in ("mean_v", "mean_h", "best_v", "best_h"):
        res[n] = 3.0 + rng.random((M, ncol))
    res["mean_xi"] = 1.0 + 0.1 * rng.random((M, ncol))
    res["cov_vh"] = 0.004 * (rng.random((M, ncol)) - 0.5)
    res["p_pos"] = rng.random((M, ncol))
    res["p_pos"][0, 8] = 1.0; res["p_pos"][1, 8] = 0.0
    res.update(phi_start=80 * rng.random(ncol), best_energy=3 * rng.random(ncol), mean_phi=6 * rng.random(ncol))
    ints = dict(nused_r=3, nused_l=1, flag=0, accepted=30, rejected=70, out_of_box=5, no_root=2, proposed_v=40, proposed_h=35, proposed_pair=25, accepted_v=10,
                accepted_h=7, accepted_pair=13, reseeded=0, nkept=kept)
    res.update({n: np.full(ncol, v, np.int32) for n, v in ints.items()})
    res["var_v"][0, 8] = -1e-18                                                    # a rounding-negative variance: sd 0
    dead = ~inner
    dead[1 * nx + 2] = True                                                        # an interior column without data
    for n in NODES:
        res[n][:, dead] = 0.0
    for n in ("best_energy", "mean_phi", "phi_start"):
        res[n][dead] = 0.0
    for n in ints:
        res[n][dead] = 0
    res["flag"][1 * nx + 2] = 2
    res["reseeded"][1 * nx + 3] = 2
    return res


def test_posterior_files_round_trip(tmp_path, taipei):
    c = small_case(taipei)
    nx, ny, nz = 6, 5, 3
    M = nz - 1
    res = fake_result(nx, ny, nz)
    rng = np.random.default_rng(3)
    vsv = (3.0 + rng.random((nz, ny, nx))).astype(F); vsh = (vsv * (1.0 + 0.05 * rng.random((nz, ny, nx)))).astype(F)
    path = str(tmp_path / "DepthRadialPosterior.dat")
    RP.write_posterior(path, c, vsv, vsh, res)
    rows = RP.read_posterior(path)
    assert len(rows) == M * ny * nx and [r["depth"] for r in rows[::nx * ny]] == [0.0, 2.0]      # the bottom depth has no line
    assert list(rows[0]) == ["lon", "lat", "depth", "vsv_start", "vsv_mean", "vsv_sd", "vsv_best", "vsv_rhat", "vsh_start", "vsh_mean", "vsh_sd", "vsh_best", "vsh_rhat",
                             "xi_start", "xi_mean", "xi_sd", "xi_rhat", "corr", "sd_diff", "p_pos"]
    v0 = vsv.astype(np.float64).reshape(nz, -1)[:M].ravel(); h0 = vsh.astype(np.float64).reshape(nz, -1)[:M].ravel()
    kept = np.tile(res["nkept"] > 0, M)
    col = lambda name: np.array([r[name] for r in rows])
    assert np.array_equal(col("vsv_start"), v0) and np.array_equal(col("vsh_start"), h0) and np.array_equal(col("xi_start"), (h0 / v0) ** 2)
    n = 6.0
    for t, name, s0 in (("v", "vsv", v0), ("h", "vsh", h0), ("xi", "xi", (h0 / v0) ** 2)):
        assert np.array_equal(col(name + "_mean"), np.where(kept, res["mean_" + t].ravel(), s0)), name
        assert np.array_equal(col(name + "_sd"), np.sqrt(np.maximum(res["var_" + t], 0.0)).ravel()), name
        W, B = res["W_" + t].ravel(), res["B_" + t].ravel()
        assert np.array_equal(col(name + "_rhat"), np.where(kept, np.sqrt((W * (n - 1.0) / n + B) / np.where(kept, W, 1.0)), 1.0)), name
    assert np.array_equal(col("vsv_best"), np.where(kept, res["best_v"].ravel(), v0)) and np.array_equal(col("vsh_best"), np.where(kept, res["best_h"].ravel(), h0))
    sdv, sdh = col("vsv_sd"), col("vsh_sd")
    ok = sdv * sdh > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        want = res["cov_vh"].ravel() / (sdv * sdh)
    assert np.array_equal(col("corr")[ok], want[ok]) and not col("corr")[~ok].any() and rows[8]["vsv_sd"] == 0.0 and rows[8]["corr"] == 0.0
    assert np.array_equal(col("sd_diff"), np.sqrt(np.maximum(res["var_v"] + res["var_h"] - 2 * res["cov_vh"], 0.0)).ravel() * kept)
    assert np.array_equal(col("p_pos"), res["p_pos"].ravel()) and rows[0]["vsv_rhat"] == 1.0 and rows[0]["xi_sd"] == 0.0 and rows[1 * nx + 2]["vsh_mean"] == h0[1 * nx + 2]
    lon, lat = maps._lonlat(c, 0, 0)
    k = 1 * nx + 1
    assert rows[k]["lon"] == float(lon) and rows[k]["lat"] == float(lat)           # node order: Depth.dat's
    with open(path) as fh:
        assert re.search(r"\d\.\d{15,16}(e[-+]\d+)?\b", fh.read())               # 17 significant digits
    fpath = str(tmp_path / "DepthRadialPosteriorFit.dat")
    RP.write_posterior_fit(fpath, c, res)
    rows = RP.read_posterior_fit(fpath)
    assert len(rows) == ny * nx
    assert [r["phi_start"] for r in rows] == res["phi_start"].tolist() and [r["phi_best"] for r in rows] == res["best_energy"].tolist()
    assert [r["phi_mean"] for r in rows] == res["mean_phi"].tolist() and [r["nused_r"] for r in rows] == res["nused_r"].tolist() and [r["nused_l"] for r in rows] == res["nused_l"].tolist()
    assert (rows[k]["accepted"], rows[k]["out_of_box"], rows[k]["no_root"]) == (0.3, 0.05, 0.02) and rows[0]["accepted"] == 0.0
    assert (rows[k]["accepted_v"], rows[k]["accepted_h"], rows[k]["accepted_pair"]) == (10 / 40, 7 / 35, 13 / 25) and rows[0]["accepted_pair"] == 0.0
    assert rows[1 * nx + 2]["flag"] == 2 and rows[1 * nx + 3]["reseeded"] == 2 and rows[k]["lon"] == float(lon)


class FakeEngine:
    """what run() calls, with a made-up result"""
    last = None

    def __init__(self, device=0):
        self.calls = []
        FakeEngine.last = self

    def dispersion_begin_radial(self, vsv, vsh, depz, minthk, kmax, nmaps):
        self.shape = vsv.shape
        self.calls.append(("begin_radial", kmax))

    def dispersion_run(self, wave, kind, t, kernels, slot, first):
        self.calls.append(("run", (wave, kind, kernels, first)))

    def dispersion_fetch(self, first, n, kernels, slot):
        nz, ny, nx = self.shape
        return np.full((n, ny * nx), 3.0) + 0.03 * (np.arange(n)[:, None] % 2 * 2 - 1)

    def columns_sample_radial_begin(self, *args):
        self.calls.append(("sample_begin", args))

    def columns_sample_radial_run(self, n):
        self.calls.append(("sample_run", n))

    def columns_sample_radial_fetch(self):
        return fake_result(6, 5, 3)

    def close(self):
        self.calls.append(("close", None))


def driver_inputs(tmp_path, c, monkeypatch):
    """a maps file and a DepthRadial.dat of the small case, io.load and the engine replaced"""
    nx, ny, nz = c["nx"], c["ny"], c["nz"]
    rng = np.random.default_rng(5)
    vsv = (3.0 + rng.random((nz, ny, nx))).astype(F); vsh = (vsv * F(1.02)).astype(F)
    depth.write_radial(str(tmp_path / "DSurfTomo.inDepthRadial.dat"), c, vsv, vsh)
    import dsurftomo_amd.engine as E
    monkeypatch.setattr(E, "Engine", FakeEngine)
    monkeypatch.setattr(io, "load", lambda *_: c)
    obs = np.full((c["kmax"], ny * nx), 3.0, F)
    monkeypatch.setattr(maps, "read_maps", lambda path: ["rows of " + path])
    monkeypatch.setattr(depth, "maps_to_obs", lambda rows, cc: (obs, np.ones(obs.shape)))
    return vsv, vsh, obs


def test_summary_and_the_driver(tmp_path, taipei, monkeypatch):
    c = small_case(taipei)
    nx, ny, nz = 6, 5, 3
    res = fake_result(nx, ny, nz)
    sm = RP.summary(res)
    kept = res["nkept"] > 0
    r = {t: depth.sample_rhat(res["W_" + t], res["B_" + t], res["nkept"][None])[:, kept] for t in ("v", "h", "xi")}
    both = np.concatenate([r["v"].ravel(), r["h"].ravel()])
    p = res["p_pos"][:, kept]
    assert sm["rhat"] == {t: dict(median=float(np.median(r[t])), worst=float(r[t].max())) for t in r} and sm["unknowns"] == 2 * 2 * 11
    assert sm["above"] == float((both > 1.1).mean()) and sm["accepted"] == dict(v=10 / 40, h=7 / 35, pair=13 / 25)
    assert sm["sure"] == float(((p < 0.025) | (p > 0.975)).mean()) and sm["sure"] >= 2 / p.size
    assert RP.summary(dict(res, nkept=np.zeros(nx * ny, np.int32))) is None
    vsv, vsh, obs = driver_inputs(tmp_path, c, monkeypatch)
    lines = []
    out = RP.run("dir", "8,40,10", out_dir=str(tmp_path), smooth=0.5, aniso=0.2, sigma=0.025, sample_step=0.07, sample_spread=0.03, sample_width=0.6, sample_seed=5,
                 sample_temperature=2.0, pairs=False, log=lines.append)
    eng = FakeEngine.last
    assert [n for n, _ in eng.calls] == ["sample_begin", "sample_run", "close"] and eng.calls[1][1] == 40          # --sigma: no stage to measure it
    args = eng.calls[0][1]
    assert np.array_equal(args[0], vsv) and np.array_equal(args[1], vsh) and args[0].dtype == F and args[5] is obs
    assert args[4] == depth.slot_plan(c) and args[7:] == (8, 0.5 / 0.025, 0.2 / 0.025, 0.07, 0.03, 0.6, 2.0, float(c["minvel"]), float(c["maxvel"]), 5, 10, False)
    assert args[6].dtype == F and (args[6] == F(40.0)).all()
    assert os.path.exists(out["posterior_path"]) and os.path.exists(out["posterior_fit_path"]) and out["sample_sigma"] == 0.025 and out["summary"] == sm
    assert os.path.basename(out["posterior_path"]) == "DSurfTomo.inDepthRadialPosterior.dat" and os.path.basename(out["posterior_fit_path"]) == "DSurfTomo.inDepthRadialPosteriorFit.dat"
    text = "\n".join(lines)
    assert "--sigma 0.025000" in text and "8 chains x 40 sweeps (30 kept)" in text and "1 columns without data" in text and "2 chains put back" in text and "pair proposals off" in text
    assert "Vsv %.4f / %.4f, Vsh %.4f / %.4f, xi %.4f / %.4f; %.1f %% of 44 unknowns above 1.1" % (
        sm["rhat"]["v"]["median"], sm["rhat"]["v"]["worst"], sm["rhat"]["h"]["median"], sm["rhat"]["h"]["worst"], sm["rhat"]["xi"]["median"], sm["rhat"]["xi"]["worst"],
        100 * sm["above"]) in text
    assert "accepted 25.0 % of the Vsv, 20.0 % of the Vsh and 52.0 % of the pair proposals" in text
    assert "P(Vsh > Vsv) is outside [0.025, 0.975] at %.1f %% of the nodes" % (100 * sm["sure"]) in text


def test_sigma_of_the_start(tmp_path, taipei, monkeypatch):
    """without --sigma and --map-sigma: one radial stage, the plan's runs (times only), a fetch; sigma is the weighted rms of obs - pv over the
    interior, and the log says so"""
    c = small_case(taipei)
    driver_inputs(tmp_path, c, monkeypatch)
    lines = []
    out = RP.run("dir", "2,4", out_dir=str(tmp_path), log=lines.append)
    eng = FakeEngine.last
    plan = depth.slot_plan(c)
    assert [n for n, _ in eng.calls] == ["begin_radial"] + ["run"] * len(plan) + ["sample_begin", "sample_run", "close"]
    assert [a for n, a in eng.calls if n == "run"] == [(wave, kind, False, first) for wave, kind, t, first in plan]
    assert abs(out["sample_sigma"] - 0.03) < 1e-6                                  # obs 3.0 against curves 3.0 +- 0.03
    assert "the weighted rms of the start over %d data, %.6f km/s" % (4 * 4 * 3, out["sample_sigma"]) in "\n".join(lines)
    args = [a for n, a in eng.calls if n == "sample_begin"][0]
    assert args[8] == depth.DEFAULT_SMOOTH / out["sample_sigma"] and args[9] == depth.DEFAULT_ANISO / out["sample_sigma"] and args[-1] is True


def test_new_symbols_declared_bound_and_exported():
    """declared in the public header, argtypes set by engine.py on both kinds of handle, Engine methods, exported by the built library; the
    new header is in the build's list, holds the arithmetic's names and no libm call"""
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
        assert [len(getattr(handle, n).argtypes) for n in NEW] == [28, 2, 4, 25]
        assert [len(getattr(handle, n).argtypes) for n in ("dsa_columns_sample_begin", "dsa_columns_sample_state", "dsa_dispersion_begin_radial")] == [25, 15, 10]
    for method in ("columns_sample_radial_begin", "columns_sample_radial_run", "columns_sample_radial_fetch", "columns_sample_radial_state"):
        assert callable(getattr(E.Engine, method))
    assert "column_sample_radial.h" in build.HEADERS and "column_sample.h" in build.HEADERS
    with open(os.path.join(L.ROOT, "dsurftomo_amd", "csrc", "column_sample_radial.h")) as fh:
        text = fh.read()
    assert '#include "column_sample.h"' in text
    for name in ("sample_radial_setup_models", "sample_radial_setup_state", "sample_radial_propose", "sample_radial_accept", "sample_radial_finish", "sample_psi",
                 "sample_neglog", "sample_bits", "sample_interior"):
        assert re.search(r"\b%s\(" % name, text), name
    assert not re.search(r"\b(sqrt|log|exp|pow)\s*\(", re.sub(r"//.*", "", text))            # no libm call and no square root in the code
    with open(os.path.join(L.ROOT, "dsurftomo_amd", "csrc", "column_kernels.hip")) as fh:
        kernels = fh.read()
    for name in ("k_sample_radial_setup", "k_sample_radial_propose", "k_sample_radial_accept", "k_sample_radial_finish"):
        assert re.search(r"__global__ void __launch_bounds__\(kSampleBlock\) %s\(SampleRadialView S" % name, kernels), name
    assert callable(RP.column_sample_radial_twin) and RP.column_sample_radial_twin is depth_twins.column_sample_radial_twin


def test_depth_keeps_its_stages_and_its_refusal():
    assert [s[0] for s in depth.STAGES] == ["depth resolution", "depth lateral resolution", None, "depth sample", "depth radial resolution"]
    assert [s[1] for s in depth.STAGES] == [False, False, False, False, True]
    with pytest.raises(ValueError, match="--sample and --radial exclude each other"):
        depth.check_sample("4,10", radial=True)
    with pytest.raises(SystemExit):
        depth.main(["dir", "--sample", "4,10", "--radial"])
    assert not hasattr(depth, "column_sample_radial_twin")                        # the new twin is reached through the new module
