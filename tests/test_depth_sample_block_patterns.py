"""The host side of the block proposals (dsurftomo_amd/depth.py --sample-block), no GPU: the new flags and what they
leave alone, the refusals before the library is loaded, the default scale, what run_sample calls and logs, the posterior files' round trip
with block sweeps on, the new symbols in the header, the binding and the built library."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import _libs as L
import test_depth_sample_patterns as T29
from dsurftomo_amd import depth, io

F = np.float32
NEW = ("dsa_columns_sample_shape", "dsa_columns_sample_blocks", "dsa_columns_sample_block_state")


def test_parser_defaults_and_the_default_scale():
    a = depth.parser().parse_args(["dir"])
    assert (a.sample_block, a.sample_block_scale) == (0, None)
    assert (a.sample, a.sample_step, a.sample_spread, a.sample_width, a.sample_seed, a.sample_temperature) == (None, 0.05, 0.05, 0.5, 1, 1.0)
    a = depth.parser().parse_args(["dir", "--sample", "64,1000", "--sample-block", "2", "--sample-block-scale", "0.7"])
    assert (a.sample, a.sample_block, a.sample_block_scale) == ("64,1000", 2, 0.7)
    assert depth.sample_block_scale(8) == 2.38 * math.sqrt(3.0 / 8.0) and depth.sample_block_scale(3, 2.0) == 2.38 * math.sqrt(6.0 / 3.0)
    assert abs(depth.sample_block_scale(5) ** 2 / 3.0 - 2.38 ** 2 / 5) < 1e-15          # the variance of a step along a unit direction: 2.38^2 / M
    assert depth.check_sample("4,10", block=0) == (4, 10, 5) and depth.check_sample("4,10", block=3, block_scale=0.5) == (4, 10, 5)
    assert depth.check_sample(None, radial=True, lateral=1.0, block=0) is None


@pytest.mark.parametrize("argv", [["--sample-block", "2"], ["--sample", "4,10", "--sample-block", "-1"], ["--sample-block", "-1"],
                                  ["--sample", "4,10", "--sample-block", "1", "--sample-block-scale", "0"], ["--sample", "4,10", "--sample-block-scale", "-0.5"],
                                  ["--sample", "4,10", "--sample-block", "1", "--sample-block-scale", "nan"], ["--sample", "4,10", "--sample-block", "1.5"],
                                  ["--sample", "4,10", "--sample-block", "1", "--radial"]])
def test_cli_refuses_before_the_library(monkeypatch, tmp_path, argv):
    import dsurftomo_amd.engine as E

    def refuse(*_):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(E, "load_library", refuse)
    monkeypatch.setattr(io, "load", refuse)
    with pytest.raises(SystemExit) as exc:
        depth.main([str(tmp_path)] + argv)
    assert exc.value.code == 2


@pytest.mark.parametrize("kw,match", [(dict(sample_block=2), "--sample-block needs --sample"), (dict(sample="4,10", sample_block=-2), "--sample-block"),
                                      (dict(sample="4,10", sample_block=1, sample_block_scale=0.0), "--sample-block-scale"),
                                      (dict(sample="4,10", sample_block=1, sample_block_scale=float("inf")), "--sample-block-scale")])
def test_run_refuses_before_the_input_is_read(monkeypatch, tmp_path, kw, match):
    def refuse(*_):
        raise AssertionError("the input was read")
    monkeypatch.setattr(io, "load", refuse)
    with pytest.raises(ValueError, match=match):
        depth.run(str(tmp_path), **kw)


class FakeEngine(T29.FakeEngine):
    """what run_sample calls with block sweeps on, with a made-up result"""

    def dispersion_run(self, *args):
        self.calls.append(("dispersion_run", args))

    def columns_sample_shape(self, *args):
        self.calls.append(("shape", args))
        nx, ny, nz = self.shape
        flag = np.zeros(nx * ny, np.int32); flag[[8, 9]] = 1; flag[14] = 2
        return dict(tri=np.zeros((nz * (nz - 1) // 2, nx * ny)), r=np.zeros((nz - 1, nx * ny)), flag=flag)

    def columns_sample_blocks(self, *args):
        self.calls.append(("blocks", args))

    def columns_sample_block_state(self):
        nx, ny, nz = self.shape
        bc = np.zeros((3, 8, nx * ny), np.int32)
        bc[0, :, 7], bc[1, :, 7], bc[2, :, 7] = 20, 5, 3
        return dict(pold_all=np.zeros((nz - 1, 8, nx * ny), F), block_counters=bc)


def test_the_driver_calls_and_the_log(tmp_path):
    c = T29.small_case(io.load())
    nx, ny, nz = 6, 5, 3
    start = np.full((nz, ny, nx), 3.0, F)
    obs = np.full((4, ny * nx), 3.0, F)
    mask = np.ones((4, ny * nx), F); mask[2, 9] = 0.0
    plan = depth.slot_plan(c)
    # off: section 29's calls and nothing else
    eng, lines = FakeEngine(nx, ny, nz), []
    out = depth.run_sample(eng, c, plan, start, obs, mask, 0.5, 0.025, (8, 40, 10), str(tmp_path), 0.07, 0.03, 0.6, 5, 2.0, lines.append, block_every=0)
    assert [n for n, _ in eng.calls] == ["begin", "run"] and "block" not in out and not any("block" in line for line in lines)
    # on: the plan's runs with kernels, the shape with the sampler's weights, the begin, the blocks, the sweeps
    eng, lines = FakeEngine(nx, ny, nz), []
    out = depth.run_sample(eng, c, plan, start, obs, mask, 0.5, 0.025, (8, 40, 10), str(tmp_path), 0.07, 0.03, 0.6, 5, 2.0, lines.append, block_every=2, damp=0.1)
    names = [n for n, _ in eng.calls]
    assert names == ["dispersion_run"] * len(plan) + ["shape", "begin", "blocks", "run"]
    for (_, args), (wave, kind, t, first) in zip(eng.calls, plan):
        assert args[:2] == (wave, kind) and args[2] is t and args[3:] == (True, first, first)
    shape_args, begin_args, block_args = (eng.calls[len(plan) + k][1] for k in range(3))
    assert shape_args[0] is obs and shape_args[1].dtype == F and shape_args[1][2, 9] == 0 and (shape_args[1][mask == 1] == F(40.0)).all()
    assert shape_args[2:] == (0.5 / 0.025, 0.1 / 0.025) and begin_args[5] is shape_args[1] and begin_args[7] == shape_args[2]
    assert block_args == (2, depth.sample_block_scale(2, 2.0))
    assert out["block"] == dict(every=2, scale=depth.sample_block_scale(2, 2.0), flagged=2, proposed=160, accepted=40, out_of_box=24)
    text = "\n".join(lines)
    res = T29.fake_result(nx, ny, nz)
    single = int(res["accepted"].sum() + res["rejected"].sum()) - 160
    assert "block proposals of scale %.4f every 2 sweeps, 2 columns with a flagged shape" % depth.sample_block_scale(2, 2.0) in text
    assert "25.0 %% of 160 block proposals accepted (15.0 %% out of the box), %.1f %% of %d single-node proposals" % (100.0 * (res["accepted"].sum() - 40) / single, single) in text
    assert "R-hat of 22 unknowns" in text
    out = depth.run_sample(FakeEngine(nx, ny, nz), c, plan, start, obs, mask, 0.5, 0.025, (8, 40, 10), str(tmp_path), log=lines.append, block_every=1, block_scale=0.25)
    assert out["block"]["scale"] == 0.25 and out["block"]["every"] == 1
    # the files keep their columns
    rows = depth.read_posterior_fit(out["posterior_fit_path"])
    assert len(rows) == nx * ny and sorted(rows[0]) == sorted(n for n, *_ in depth.POSTERIOR_FIT_TABLE[1])
    assert len(depth.read_posterior(out["posterior_path"])) == (nz - 1) * nx * ny


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
        assert [len(getattr(handle, n).argtypes) for n in NEW] == [9, 3, 3]
        assert handle.dsa_columns_sample_blocks.argtypes[2] is C.c_double
        assert [len(getattr(handle, n).argtypes) for n in T29.NEW] == [25, 2, 4, 15]          # section 29's signatures are as they were
    for method in ("columns_sample_shape", "columns_sample_blocks", "columns_sample_block_state"):
        assert callable(getattr(E.Engine, method))
    with open(os.path.join(L.ROOT, "dsurftomo_amd", "csrc", "column_sample.h")) as fh:
        text = fh.read()
    for name in ("sample_rsqrt", "sample_shape", "sample_propose_block", "sample_accept_block", "sample_block_sweep"):
        assert re.search(r"\b%s\(" % name, text), name
    assert "struct SampleBlockView" in text and not re.search(r"\b(sqrt|log|exp|pow)\s*\(", re.sub(r"//.*", "", text))
    with open(os.path.join(L.ROOT, "dsurftomo_amd", "csrc", "column_kernels.hip")) as fh:
        kernels = fh.read()
    for name in ("k_sample_propose_block", "k_sample_accept_block"):
        assert re.search(r"__global__ void __launch_bounds__\(kSampleBlock\) %s\(" % name, kernels), name
    assert re.search(r"__global__ void __launch_bounds__\(64\) k_sample_shape\(", kernels)
    assert callable(depth.column_shape_twin) and callable(depth.sample_rsqrt)
