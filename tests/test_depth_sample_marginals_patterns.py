"""The host side of the posterior marginals (dsurftomo_amd/depth.py --sample-bins), no GPU: the new flags and what
they leave alone, the refusals before the library is loaded and before the input is read, what run_sample calls and logs and in which
order, the three files' round trips, the new symbols in the header, the binding and the built library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _libs as L
import test_depth_sample_block_patterns as T32
import test_depth_sample_patterns as T29
from dsurftomo_amd import depth, io

F = np.float32
NEW = ("dsa_columns_sample_marginals", "dsa_columns_sample_marginals_fetch", "dsa_columns_sample_marginals_state")
DEFAULT_LEVELS = (0.025, 0.16, 0.5, 0.84, 0.975)


def test_parser_defaults():
    a = depth.parser().parse_args(["dir"])
    assert (a.sample_bins, a.sample_quantiles, a.sample_covariance) == (0, "0.025,0.16,0.5,0.84,0.975", False)
    assert (a.sample, a.sample_block, a.sample_block_scale, a.sample_step) == (None, 0, None, 0.05)          # the older flags are as they were
    a = depth.parser().parse_args(["dir", "--sample", "64,1000", "--sample-bins", "64", "--sample-quantiles", "0.1,0.9", "--sample-covariance"])
    assert (a.sample_bins, a.sample_quantiles, a.sample_covariance) == (64, "0.1,0.9", True)
    assert depth.parse_quantiles(a.sample_quantiles) == (0.1, 0.9) and depth.parse_quantiles(depth.DEFAULT_SAMPLE_QUANTILES) == DEFAULT_LEVELS
    assert depth.check_marginals() is None and depth.check_marginals("4,10") is None
    assert depth.check_marginals("4,10", 2) == (2, DEFAULT_LEVELS, False) and depth.check_marginals("4,10", 256, "0.5", True) == (256, (0.5,), True)


@pytest.mark.parametrize("argv", [["--sample-bins", "8"], ["--sample-covariance"], ["--sample-quantiles", "0.5"], ["--sample", "4,10", "--sample-covariance"],
                                  ["--sample", "4,10", "--sample-quantiles", "0.1,0.9"], ["--sample", "4,10", "--sample-bins", "1"],
                                  ["--sample", "4,10", "--sample-bins", "-4"], ["--sample", "4,10", "--sample-bins", "257"], ["--sample", "4,10", "--sample-bins", "7.5"],
                                  ["--sample", "4,10", "--sample-bins", "8", "--sample-quantiles", "0,0.5"], ["--sample", "4,10", "--sample-bins", "8", "--sample-quantiles", "0.5,1"],
                                  ["--sample", "4,10", "--sample-bins", "8", "--sample-quantiles", "a"], ["--sample", "4,10", "--sample-bins", "8", "--sample-quantiles", "nan"],
                                  ["--sample", "4,10", "--sample-bins", "8", "--sample-quantiles", ",".join(["0.5"] * 17)],
                                  ["--sample", "4,10", "--sample-bins", "8", "--radial"]])
def test_cli_refuses_before_the_library(monkeypatch, tmp_path, argv):
    import dsurftomo_amd.engine as E

    def refuse(*_):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(E, "load_library", refuse)
    monkeypatch.setattr(io, "load", refuse)
    with pytest.raises(SystemExit) as exc:
        depth.main([str(tmp_path)] + argv)
    assert exc.value.code == 2


@pytest.mark.parametrize("kw,match", [(dict(sample_bins=8), "--sample-bins needs --sample"), (dict(sample_covariance=True), "--sample-covariance needs --sample"),
                                      (dict(sample_quantiles="0.5"), "--sample-quantiles needs --sample"),
                                      (dict(sample="4,10", sample_covariance=True), "--sample-covariance needs --sample-bins"),
                                      (dict(sample="4,10", sample_quantiles="0.2,0.8"), "--sample-quantiles needs --sample-bins"),
                                      (dict(sample="4,10", sample_bins=1), "--sample-bins must be"), (dict(sample="4,10", sample_bins=300), "--sample-bins must be"),
                                      (dict(sample="4,10", sample_bins=8, sample_quantiles="0.5,2"), "--sample-quantiles takes")])
def test_run_refuses_before_the_input_is_read(monkeypatch, tmp_path, kw, match):
    def refuse(*_):
        raise AssertionError("the input was read")
    monkeypatch.setattr(io, "load", refuse)
    with pytest.raises(ValueError, match=match):
        depth.run(str(tmp_path), **kw)


def fake_marginals(nx, ny, nz, nbins, levels, cov, kept=6, chains=8):
    """a made-up result of columns_sample_marginals_fetch that agrees with T29.fake_result: counts where a sweep was kept, zeros elsewhere"""
    M, ncol = nz - 1, nx * ny
    rng = np.random.default_rng(4)
    moved = T29.fake_result(nx, ny, nz, kept)["nkept"] > 0
    hist = np.zeros((nbins, M, ncol), np.uint32)
    hist[1, :, moved] = kept * chains - 8
    hist[0, :, moved] = 2
    hist[nbins - 1, :, moved] += 6
    hist[0, 1, 7] += 40; hist[1, 1, 7] -= 40                                          # one node leans on its box
    quant = np.sort(3.0 + 0.5 * rng.random((len(levels), M, ncol)), axis=0) * moved
    out = dict(hist=hist, mode=(3.2 + 0.1 * rng.random((M, ncol))) * moved, quantiles=quant)
    if cov:
        tri = np.zeros((M * (M + 1) // 2, ncol))
        for i in range(M):
            for j in range(i + 1):
                tri[depth.column_tri(i, j)] = (0.04 if i == j else -0.01) * (1.0 + rng.random(ncol)) * moved
        tri[depth.column_tri(1, 1), 9] = 0.0                                          # a node that never moved: correlation 0
        out["cov"] = tri
    return out


class FakeEngine(T32.FakeEngine):
    """what run_sample calls with the marginals on, with a made-up result"""

    def columns_sample_marginals(self, *args):
        self.calls.append(("marginals", args))
        self.marginals = args

    def columns_sample_marginals_fetch(self, levels):
        self.calls.append(("marginals_fetch", tuple(levels)))
        return fake_marginals(*self.shape, self.marginals[0], levels, self.marginals[1])


def test_the_driver_calls_the_log_and_the_files(tmp_path):
    c = T29.small_case(io.load())
    nx, ny, nz = 6, 5, 3
    M = nz - 1
    start = (3.0 + np.random.default_rng(3).random((nz, ny, nx))).astype(F)
    obs = np.full((4, ny * nx), 3.0, F)
    plan = depth.slot_plan(c)
    common = (c, plan, start, obs, None, 0.5, 0.025, (8, 40, 10), str(tmp_path), 0.07, 0.03, 0.6, 5, 2.0)
    # off: the calls of before and nothing else
    eng, lines = FakeEngine(nx, ny, nz), []
    out = depth.run_sample(eng, *common, lines.append, block_every=2, damp=0.1)
    assert [n for n, _ in eng.calls] == ["dispersion_run"] * len(plan) + ["shape", "begin", "blocks", "run"]
    assert "marginals" not in out and not any("marginals" in line or "end bins" in line for line in lines)
    assert not os.path.exists(str(tmp_path / "DSurfTomo.inDepthPosteriorQuantiles.dat"))
    # on, with block sweeps: after the begin and the blocks, before the sweeps; the fetch after them
    levels = (0.84, 0.025, 0.5, 0.975)                                               # in no order: the outermost are found by value
    eng, lines = FakeEngine(nx, ny, nz), []
    out = depth.run_sample(eng, *common, lines.append, block_every=2, damp=0.1, marginals=(16, levels, True))
    assert [n for n, _ in eng.calls] == ["dispersion_run"] * len(plan) + ["shape", "begin", "blocks", "marginals", "run", "marginals_fetch"]
    assert eng.calls[-3][1] == (16, True) and eng.calls[-1][1] == levels
    mg = fake_marginals(nx, ny, nz, 16, levels, True)
    kept = T29.fake_result(nx, ny, nz)["nkept"] > 0
    width = float(np.median((mg["quantiles"][3] - mg["quantiles"][1])[:, kept]))
    share = ((mg["hist"][0] + mg["hist"][-1]) / mg["hist"].sum(axis=0).clip(1))[:, kept]
    assert out["marginals_summary"] == dict(nodes=int(kept.sum()) * M, width=width, end_median=float(np.median(share)), end_max=float(share.max()))
    assert share.max() == 48 / 48 and np.median(share) == 8 / 48
    text = "\n".join(lines)
    assert "marginals of %d nodes in 16 bins; the 0.025 to 0.975 interval is %.4f km/s wide (median over the nodes)" % (int(kept.sum()) * M, width) in text
    assert "share of a node's kept states in the end bins of its box: median 16.67 %, largest 100.00 %" in text
    assert "R-hat of 22 unknowns" in text and "block proposals of scale" in text     # the older lines stay
    for key, name in (("quantiles_path", "Quantiles"), ("marginals_path", "Marginals"), ("correlation_path", "Correlation")):
        assert out[key] == str(tmp_path / ("DSurfTomo.inDepthPosterior%s.dat" % name)) and out[key] in text and os.path.exists(out[key])
    # the round trips
    lo, hi = depth.sample_box(start.reshape(nz, -1)[:M], 0.6, float(c["minvel"]), float(c["maxvel"]))
    rows = depth.read_posterior_quantiles(out["quantiles_path"])
    assert len(rows) == M * nx * ny and list(rows[0]) == ["lon", "lat", "depth", "lo", "hi", "mode"] + ["q%.17g" % p for p in levels]
    marg = depth.read_posterior_marginals(out["marginals_path"])
    assert len(marg) == M * nx * ny and list(marg[0]) == ["lon", "lat", "depth"] + ["n%d" % b for b in range(16)]
    post = depth.read_posterior(out["posterior_path"])
    for n, (row, mrow) in enumerate(zip(rows, marg)):
        k, q = divmod(n, nx * ny)
        assert (row["lon"], row["lat"], row["depth"]) == (post[n]["lon"], post[n]["lat"], post[n]["depth"]) == (mrow["lon"], mrow["lat"], mrow["depth"])
        assert row["lo"] == float(lo[k, q]) and row["hi"] == float(hi[k, q]) and row["mode"] == mg["mode"][k, q]
        assert [row["q%.17g" % p] for p in levels] == mg["quantiles"][:, k, q].tolist()          # 17 digits: the doubles come back
        assert [mrow["n%d" % b] for b in range(16)] == mg["hist"][:, k, q].tolist()
    corr = depth.read_posterior_correlation(out["correlation_path"])
    want = depth.sample_correlation(mg["cov"], M)
    assert len(corr) == nx * ny and list(corr[0]) == ["lon", "lat"] + ["r%d_%d" % (i, j) for i in range(M) for j in range(M)]
    for q, row in enumerate(corr):
        assert [[row["r%d_%d" % (i, j)] for j in range(M)] for i in range(M)] == want[:, :, q].tolist()
        if kept[q] and q != 9:
            assert row["r0_0"] == 1.0 and row["r1_1"] == 1.0 and row["r0_1"] == row["r1_0"] and -1.0 < row["r0_1"] < 0.0
        else:
            assert row["r0_1"] == 0.0 and row["r1_1"] == 0.0                          # a variance of 0: correlation 0
    # on without the covariance and without block sweeps: two files, one level: no interval in the log
    eng, lines = FakeEngine(nx, ny, nz), []
    out = depth.run_sample(eng, *common, lines.append, marginals=(2, (0.5,), False))
    assert [n for n, _ in eng.calls] == ["begin", "marginals", "run", "marginals_fetch"] and eng.calls[1][1] == (2, False)
    assert out["correlation_path"] is None and out["marginals_summary"]["width"] is None and not any("interval" in line for line in lines)
    assert len(depth.read_posterior_marginals(out["marginals_path"])[0]) == 3 + 2


def test_the_twin_rules():
    lo, hi = F(3.0), F(3.5)
    assert depth.sample_marginal_bin(F([2.0, 3.0, 3.24, 3.25, 3.5, 9.0]), lo, hi, 2).tolist() == [0, 0, 0, 1, 1, 1]
    assert not depth.sample_marginal_bin(F([2.0, 3.0, 9.0]), hi, lo, 7).any()        # no width: bin 0
    assert depth.sample_marginal_mode([0, 3, 3, 1], lo, hi) == 3.0 + (1.5 / 4) * 0.5 and depth.sample_marginal_mode([0, 0], lo, hi) == 0.0
    assert depth.sample_marginal_quantile([0, 4, 0, 4], lo, hi, 0.5) == 3.0 + (2.0 / 4) * 0.5      # the first bin that reaches the target, at its end
    assert depth.sample_marginal_quantile([0, 4, 0, 4], lo, hi, 0.75) == 3.0 + (3.5 / 4) * 0.5
    assert depth.sample_marginal_quantile([0, 0, 0], lo, hi, 0.5) == 0.0
    counts = depth.sample_marginal_counts(F([[[3.0, 3.4]], [[9.0, 9.0]]]).reshape(2, 1, 2).repeat(3, axis=1), F([[3.2, 3.2], [9.0, 9.0]]), 0.25, 0.0, 10.0, 5)
    assert counts.shape == (5, 1, 2) and counts[:, 0, 0].tolist() == [3, 0, 0, 0, 0] and counts[:, 0, 1].tolist() == [0, 0, 0, 0, 3]


def test_new_symbols_declared_bound_and_exported():
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
        assert [len(getattr(handle, n).argtypes) for n in NEW] == [3, 6, 3]
        assert [len(getattr(handle, n).argtypes) for n in T32.NEW] == [9, 3, 3] and [len(getattr(handle, n).argtypes) for n in T29.NEW] == [25, 2, 4, 15]
    for method in ("columns_sample_marginals", "columns_sample_marginals_fetch", "columns_sample_marginals_state"):
        assert callable(getattr(E.Engine, method))
    with open(os.path.join(L.ROOT, "dsurftomo_amd", "csrc", "column_sample.h")) as fh:
        text = fh.read()
    for name in ("sample_bin", "sample_marginal_hist", "sample_marginal_cov", "sample_marginal_finish", "sample_marginal_cov_finish"):
        assert re.search(r"\b%s\(" % name, text), name
    code = re.sub(r"//.*", "", text)
    assert "struct SampleMarginalView" in text and not re.search(r"\b(sqrt|log|exp|pow|floor|fma)\s*\(", code) and "atomic" not in code      # the header's rules
    assert re.search(r"struct SampleView \{[^}]*double\* phi0;[^}]*\};", text) and "nbins" not in re.search(r"struct SampleView \{[^}]*\};", text).group(0)
    with open(os.path.join(L.ROOT, "dsurftomo_amd", "csrc", "column_kernels.hip")) as fh:
        kernels = fh.read()
    for name in ("k_sample_hist", "k_sample_cov", "k_sample_marginal_finish"):
        assert re.search(r"__global__ void __launch_bounds__\(kSampleBlock\) %s\(" % name, kernels), name
    for name in ("sample_marginal_bin", "sample_marginal_mode", "sample_marginal_quantile", "sample_marginal_counts", "sample_marginal_twin", "sample_correlation"):
        assert callable(getattr(depth, name)), name
