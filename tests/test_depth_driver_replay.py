"""The wiring of the depth driver (dsurftomo_amd/depth.py: run and main), no GPU: a recording engine stands in for engine.Engine, io.load
returns the small case of the pattern tests, and each of RUNS -- the smallest set of options that reaches every branch of run() -- is driven
to the end, once through depth.run(**keywords) and once through depth.main(argv).  A run's record holds the engine calls in order (method,
every scalar verbatim, every array as dtype, shape and the sha256 of its bytes), every log line, the files written with their sha256 and
the keys of the returned dict.  The two records must be equal, and equal to tests/golden/depth_driver_replay.json, which was recorded once:

    python tests/test_depth_driver_replay.py --record

The engine's answers are np.random.default_rng(fixed seed) and plain arithmetic (nothing of libm but sqrt), the same on every machine."""
import contextlib
import hashlib
import json
import os
import sys
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):                                              # (started as a script: the recorder)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import columns_ref as R
import test_depth_sample_block_patterns as T32
import test_depth_sample_marginals_patterns as T33
import test_depth_sample_patterns as T29
from dsurftomo_amd import depth, io, maps

F = np.float32
NX, NY, NZ, NMAPS = 6, 5, 3, 4
GOLDEN = os.path.join(HERE, "golden", "depth_driver_replay.json")
NO_DATA, NOT_DEFINITE = 1 * NX + 2, 2 * NX + 3                                        # an interior column without data, and one whose pivot fails

RUNS = {
    "defaults": dict(),
    "min_dws": dict(min_dws=4.0, iterations=2),
    "resolution": dict(resolution=True),
    "resolution_sigma": dict(resolution=True, sigma=0.04, smooth=0.7, damp=0.2, dvmax=0.4, iterations=3),
    "lateral": dict(lateral=0.3),
    "lateral_resolution": dict(lateral=0.3, lateral_resolution=True, lateral_resolution_stride=2, lateral_checkerboard="2,2,1", iterations=2, smooth=0.6,
                               damp=0.15, lateral_tol=1e-6, lateral_maxit=40, sigma=0.05),
    "lateral_resolution_plain": dict(lateral=0.2, lateral_resolution=True, min_dws=4.0),
    "radial": dict(radial=True),
    "radial_lateral": dict(radial=True, radial_lateral=0.3, iterations=2),
    "radial_lateral_aniso": dict(radial=True, radial_lateral=0.3, radial_lateral_aniso=0.6, aniso=0.35, iterations=3, lateral_tol=1e-7, lateral_maxit=60, dvmax=0.3),
    "radial_resolution": dict(radial=True, radial_resolution=True),
    "radial_resolution_sigma": dict(radial=True, radial_resolution=True, sigma=0.03, aniso=0.4, smooth=0.8, damp=0.25, min_dws=4.0, iterations=2),
    "sample": dict(sample="4,10"),
    "sample_block": dict(sample="4,10", sample_block=1, iterations=2),
    "sample_all": dict(sample="4,10,3", resolution=True, sigma=0.025, sample_step=0.07, sample_spread=0.03, sample_width=0.6, sample_seed=5, sample_temperature=2.0,
                       sample_block=2, sample_block_scale=0.25, sample_bins=8, sample_quantiles="0.1,0.5,0.9", sample_covariance=True, damp=0.2, smooth=0.4, min_dws=4.0),
}


def small_case():
    """tests/test_depth_patterns.py's small case with a constant starting model"""
    return dict(T29.small_case(io.load()), vels=np.full((NX, NY, NZ), 3.0, F))


def write_maps(path, c):
    rng = np.random.default_rng(3)
    velv = (3.0 + rng.random((NMAPS, NX * NY))).astype(F)
    norm = (10.0 * rng.random(NMAPS * (NX - 2) * (NY - 2))).astype(F)
    maps.write_maps(path, c, velv, norm)


def encode(x):
    """an argument as the record keeps it: a scalar verbatim, an array as 'dtype[shape]:sha256', a sequence item by item"""
    if isinstance(x, np.ndarray):
        return "%s[%s]:%s" % (x.dtype, ",".join(str(n) for n in x.shape), hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest())
    if isinstance(x, np.generic):
        return "%s(%r)" % (x.dtype, x.item())
    if isinstance(x, (list, tuple)):
        return [encode(v) for v in x]
    if x is None or isinstance(x, (bool, int, float, str)):
        return x
    raise TypeError("the recorder does not know %r" % (type(x),))


def recorded(method):
    def wrapper(self, *args, **kw):
        self.calls.append([method.__name__, encode(args)] + ([{k: encode(v) for k, v in sorted(kw.items())}] if kw else []))
        return method(self, *args, **kw)
    return wrapper


class RecordingEngine:
    """every Engine method the driver calls: records the call, answers with made-up arrays of the right shapes"""
    calls = None                                                                     # (the run's list, set by patched())

    def __init__(self, device=0):
        self.calls.append(["Engine", [device]])
        self.ncol, self.M, self.nsteps = NX * NY, NZ - 1, 0
        self.inner = R.interior(NX, NY) == 1

    def _rng(self):
        return np.random.default_rng(1000 + len(self.calls))

    def _flags(self, coupled=False):
        flag = np.zeros(self.ncol, np.int32)
        flag[NOT_DEFINITE] = 1
        if not coupled:
            flag[NO_DATA] = 2
        return flag

    def _step(self, counts, coupled):
        """counts: the data of an interior column per wave type, (4,) or (3, 1)"""
        rng = self._rng()
        self.nsteps += 1
        lead = (len(counts),) if len(counts) > 1 else ()
        nused = np.zeros((len(counts), self.ncol), np.int32)
        nused[:, self.inner] = np.asarray(counts, np.int32)[:, None]
        nused[:, NO_DATA] = 0
        flag = self._flags(coupled)
        chi2 = 0.01 * rng.random((len(counts), self.ncol)) * (nused > 0)
        moved = self.inner & (flag == 0)
        dv = ((0.1 * (rng.random((len(counts), self.M, self.ncol)) - 0.5)) * moved).astype(F)
        for model, d in zip(self.models, dv):
            model[:self.M] += d.reshape(self.M, NY, NX)
        out = dict(nused=nused.reshape(lead + (self.ncol,)), chi2=chi2.reshape(lead + (self.ncol,)), flag=flag)
        out.update(dict(dv=dv[0]) if len(counts) == 1 else dict(dv_sv=dv[0], dv_sh=dv[1]))
        if coupled:
            out.update(itn=7 + self.nsteps, istop=2 if self.nsteps == 2 else 1, rz0=1.0, rz=1e-9 * self.nsteps, carried=1)
        return out

    @recorded
    def close(self):
        pass

    @recorded
    def dispersion_begin(self, vels, depz, minthk, kmax_total, nmaps_total):
        self.models = [np.array(vels, F, copy=True)]

    @recorded
    def dispersion_begin_radial(self, vsv, vsh, depz, minthk, kmax_total, nmaps_total):
        self.models = [np.array(vsv, F, copy=True), np.array(vsh, F, copy=True)]

    @recorded
    def dispersion_run(self, iwave, igr, t, kernels, sen_slot=0, map_first=0):
        pass

    @recorded
    def dispersion_get_model(self):
        return self.models[0].copy()

    @recorded
    def dispersion_get_model_radial(self):
        return self.models[0].copy(), self.models[1].copy()

    @recorded
    def columns_step(self, obs, wt, smooth, damp, dvmax, minvel, maxvel):
        return self._step((4,), False)

    @recorded
    def columns_step_lateral(self, obs, wt, smooth, damp, lateral, dvmax, minvel, maxvel, tol=1e-8, maxit=500):
        return self._step((4,), True)

    @recorded
    def columns_step_radial(self, obs, wt, smooth, damp, aniso, dvmax, minvel, maxvel):
        return self._step((3, 1), False)

    @recorded
    def columns_step_radial_lateral(self, obs, wt, smooth, damp, aniso, lateral, lateral_aniso, dvmax, minvel, maxvel, tol=1e-8, maxit=500):
        return self._step((3, 1), True)

    @recorded
    def columns_resolution(self, obs, wt, smooth, damp, full=False):
        rng = self._rng()
        measures = rng.random((4, self.M, self.ncol))
        measures[0, 1] *= 0.05                                                        # the deepest unknown is not resolved: the log names the depth
        measures[1, 0, 9] = 0.0                                                       # a point-spread function without a first moment: length 0
        nused = np.where(self.inner, 4, 0).astype(np.int32); nused[NO_DATA] = 0
        return dict(measures=measures, leverage=rng.random((NMAPS, self.ncol)), trace=measures[0].sum(axis=0), nused=nused, flag=self._flags())

    @recorded
    def columns_resolution_lateral(self, obs, wt, smooth, damp, lateral, kind, index, models=None, tol=1e-8, maxit=500, full=False):
        rng = self._rng()
        n = len(kind)
        measures = 0.1 + rng.random((n, 7))
        measures[1, 1] = 0.0                                                          # a member that does not answer
        istop = np.ones(n, np.int32); istop[3] = 2                                    # one stopped at maxit
        nused = np.where(self.inner, 4, 0).astype(np.int32); nused[NO_DATA] = 0
        out = dict(measures=measures, nused=nused, flag=self._flags(True), itn=(5 + np.arange(n) % 4).astype(np.int32), istop=istop, rz0=rng.random(n),
                   rz=1e-9 * rng.random(n))
        if full:
            out["full"] = 0.1 * (rng.random((n, self.M, (NX - 2) * (NY - 2))) - 0.25)
        return out

    @recorded
    def columns_resolution_radial(self, obs, wt, smooth, damp, aniso, full=False):
        rng = self._rng()
        measures = 0.05 + rng.random((6, 2 * self.M, self.ncol))
        pair = np.stack([0.01 * (rng.random((self.M, self.ncol)) - 0.5), 0.02 * rng.random((self.M, self.ncol))])
        nused = np.zeros((2, self.ncol), np.int32); nused[:, self.inner] = [[3], [1]]; nused[:, NO_DATA] = 0
        return dict(measures=measures, pair=pair, leverage=rng.random((NMAPS, self.ncol)), trace=np.stack([measures[0, :self.M].sum(axis=0), measures[0, self.M:].sum(axis=0)]),
                    nused=nused, flag=self._flags())

    @recorded
    def columns_sample_shape(self, obs, wt, smooth, damp):
        return T32.FakeEngine(NX, NY, NZ).columns_sample_shape()

    @recorded
    def columns_sample_begin(self, vels, depz, minthk, plan, obs, wt, nchains, smooth, step, spread, width, temperature, minvel, maxvel, seed, burn):
        pass

    @recorded
    def columns_sample_blocks(self, block_every, block_scale):
        pass

    @recorded
    def columns_sample_marginals(self, nbins, with_cov=False):
        self.marginals = (nbins, with_cov)

    @recorded
    def columns_sample_run(self, nsweeps):
        pass

    @recorded
    def columns_sample_fetch(self):
        return T29.fake_result(NX, NY, NZ)

    @recorded
    def columns_sample_marginals_fetch(self, levels=(), hist=True, cov=None):
        return T33.fake_marginals(NX, NY, NZ, self.marginals[0], levels, self.marginals[1])

    @recorded
    def columns_sample_block_state(self):
        return T32.FakeEngine(NX, NY, NZ).columns_sample_block_state()


@contextlib.contextmanager
def patched(case, calls):
    """io.load answers with case and engine.Engine is a RecordingEngine that appends to calls, for the length of the block"""
    import dsurftomo_amd.engine as E

    class Engine(RecordingEngine):
        pass
    Engine.calls = calls
    was = (io.load, E.Engine)
    io.load, E.Engine = (lambda *_: case), Engine
    try:
        yield
    finally:
        io.load, E.Engine = was


def argv_of(kw):
    """the command line that asks for run(**kw)"""
    argv = []
    for key, value in kw.items():
        flag = {"maps_file": "--maps", "out_dir": "--out"}.get(key, "--" + key.replace("_", "-"))
        if value is True:
            argv.append(flag)
        else:
            argv += [flag, str(value)]
    return argv


def replay(kw, tmp, via):
    """one run into a fresh directory under tmp, through depth.run ('run') or depth.main ('main'); returns the record"""
    case = small_case()
    mpath = os.path.join(tmp, "Maps.dat")
    write_maps(mpath, case)
    out_dir = os.path.join(tmp, via)
    os.makedirs(out_dir)
    calls, lines, results = [], [], []
    keep = lambda line: lines.append(line.replace(out_dir, "<OUT>"))
    with patched(case, calls):
        if via == "run":
            results.append(depth.run("case", maps_file=mpath, out_dir=out_dir, log=keep, **kw))
        else:
            real_run = depth.run

            def spy(*args, **kwargs):                                                # (main() logs with print: the spy hands run() the recorder's log)
                results.append(real_run(*args, log=keep, **kwargs))
                return results[-1]
            depth.run = spy
            try:
                assert depth.main(["case", "--maps", mpath, "--out", out_dir] + argv_of(kw)) == 0
            finally:
                depth.run = real_run
    out, *paths = results[0]
    files = {}
    for name in sorted(os.listdir(out_dir)):
        with open(os.path.join(out_dir, name), "rb") as fh:
            files[name] = hashlib.sha256(fh.read()).hexdigest()
    return dict(calls=calls, log=lines, files=files, keys=sorted(out), paths=[os.path.relpath(p, out_dir) for p in paths])


def record(path=GOLDEN):
    """writes the fixture: every run of RUNS through depth.run"""
    records = {}
    for name, kw in RUNS.items():
        with tempfile.TemporaryDirectory() as tmp:
            records[name] = replay(kw, tmp, "run")
    with open(path, "w") as fh:
        json.dump(records, fh, indent=1, sort_keys=True)
        fh.write("\n")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.mark.parametrize("name", sorted(RUNS))
def test_run_and_main_replay_the_recorded_driver(tmp_path, golden, name):
    by_run = replay(RUNS[name], str(tmp_path), "run")
    by_main = replay(RUNS[name], str(tmp_path), "main")
    for key in ("calls", "log", "files", "keys", "paths"):
        assert by_run[key] == by_main[key], "%s: run() and main() differ in %s" % (name, key)
        assert json.loads(json.dumps(by_run[key])) == golden[name][key], "%s: %s is not the recorded one" % (name, key)


def test_the_runs_reach_every_stage_and_every_conditional_line(golden):
    """the fixture is worth its name: every engine method the driver knows is called somewhere, and the lines that depend on the data appear"""
    called = {call[0] for rec in golden.values() for call in rec["calls"]}
    assert called == {"Engine"} | {n for n, v in vars(RecordingEngine).items() if callable(v) and not n.startswith("_")}
    text = "\n".join(line for rec in golden.values() for line in rec["log"])
    for words in ("--lateral-maxit was reached", "the tolerance was met", "columns without data carried", "stays under 0.1 from", "the data's standard deviation is --sigma",
                  "the data's standard deviation is the rms before the last step", "members stopped at --lateral-maxit", "checkerboard of 2 x 2 x 1 blocks", "xi = (Vsh / Vsv)^2 median",
                  "|xi - 1| > 2 sd_xi", "block proposals of scale", "single-node proposals", "chains put back at the set-up", "R-hat of", "end bins of its box",
                  "the correlations of the depths to", "1 not positive definite, 1 without data"):
        assert words in text, words
    assert sorted(golden) == sorted(RUNS)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_depth_driver_replay.py --record")
    record()
