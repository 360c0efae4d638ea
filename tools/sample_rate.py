"""What a sweep of the Monte-Carlo depth inversion costs: on the Taipei example's grid and model (18 x 18 x 9, its 26
periods, one Rayleigh phase run), 64 chains per column -- 20 736 curves per sweep.  The observations are the model's own curves 2 % off, the
data's standard deviation 0.05 km/s.  After the set-up and a warm-up sweep, `sweeps` calls of columns_sample_run(1) are timed one by one:
the median wall time of a sweep, the median device time of its dispersion run (DSA_STAT_MS_DISPERSION) and the rest -- the four new
kernels' two launches per sweep and the host's share.  One call of columns_sample_run(sweeps) follows, for the rate without the per-call
overhead.

The share of the sweep in the new kernels themselves is a kernel trace's:
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/sample_rate.py 50
    python tools/sample_rate.py trace-shares DIR/.../*_kernel_trace.csv
prints per kernel the launches, the median and the sum of their durations, and the share of the sum of all kernels that k_sample_* take.

    python tools/sample_rate.py [sweeps] [chains]      (needs the GPU)

Block mode: the same stage twice in one run -- single-node sweeps, then every sweep a block sweep
(columns_sample_blocks(1, the default scale)) -- and the time of the columns_sample_shape call that precedes them (its dispersion runs with
kernels are timed apart):
    python tools/sample_rate.py block [sweeps] [chains]

Marginals mode: the same stage twice in one run -- the marginals off, then on with `bins` bins and the covariance
(columns_sample_marginals(bins, True)), burn 0 so that every timed sweep is a kept one -- and the time of a columns_sample_marginals_fetch:
    python tools/sample_rate.py marginals [sweeps] [chains] [bins]
The plain mode above is the figure to compare with an older build.

Radial mode: the radial sample stage on the same grid and model, the example's 26 periods dealt out over the four wave
types (it lists no Love periods of its own), Vsv and Vsh both the model, 4 dispersion runs per sweep: the median sweep as above, then
`long` sweeps in one call (burn long / 2) and the chains' figures -- the acceptance per kind of proposal, R-hat of Vsv, Vsh and xi:
    python tools/sample_rate.py radial [sweeps] [chains] [long]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dsurftomo_amd import depth, io                  # noqa: E402
from dsurftomo_amd.engine import Engine             # noqa: E402


def trace_shares(path):
    """per kernel of a rocprofv3 kernel trace (csv): the launches, the median and the sum of the durations; the share of k_sample_*"""
    import csv
    rows = {}
    with open(path, newline="") as fh:
        for r in csv.DictReader(fh):
            name = r["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0].split("::")[-1]
            rows.setdefault(name, []).append(1e-3 * (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    total = sum(sum(d) for d in rows.values())
    for name, d in sorted(rows.items(), key=lambda kv: -sum(kv[1])):
        print("%-28s %6d launches, median %9.1f us, sum %12.1f us (%5.2f %%)" % (name, len(d), np.median(d), sum(d), 100.0 * sum(d) / total))
    new = sum(sum(d) for name, d in rows.items() if name.startswith("k_sample_"))
    print("k_sample_*: %.1f us of %.1f us in all kernels, %.2f %%" % (new, total, 100.0 * new / total))


def block_mode(sweeps, chains):
    """the median sweep with block_every = 1 against single-node sweeps of the same build in the same run, and the shape call"""
    c = io.load()
    plan = depth.slot_plan(c)
    vel = np.ascontiguousarray(np.asarray(c["vels"], np.float32).transpose(2, 1, 0))
    kmax, M = c["kmax"], c["nz"] - 1
    e = Engine(0)
    e.dispersion_begin(vel, c["depz"], c["minthk"], kmax, kmax)
    t0 = time.perf_counter()
    for wave, kind, tt, first in plan:
        e.dispersion_run(wave, kind, tt, True, first, first)
    t_kernels = 1e3 * (time.perf_counter() - t0)
    obs = (e.dispersion_fetch(0, kmax) * 1.02).astype(np.float32)
    sigma = 0.05
    wt, lam = depth.sample_scaling(None, depth.DEFAULT_SMOOTH, sigma, obs.shape)
    t_shape = []
    for _ in range(3):
        t0 = time.perf_counter()
        shape = e.columns_sample_shape(obs, wt, lam, depth.DEFAULT_DAMP / sigma)
        t_shape.append(1e3 * (time.perf_counter() - t0))
    out = {}
    for every in (0, 1):
        e.columns_sample_begin(vel, c["depz"], c["minthk"], plan, obs, wt, chains, lam, depth.DEFAULT_SAMPLE_STEP, depth.DEFAULT_SAMPLE_SPREAD, depth.DEFAULT_SAMPLE_WIDTH,
                               depth.DEFAULT_SAMPLE_TEMPERATURE, float(c["minvel"]), float(c["maxvel"]), depth.DEFAULT_SAMPLE_SEED, 0)
        if every:
            e.columns_sample_blocks(every, depth.sample_block_scale(M, depth.DEFAULT_SAMPLE_TEMPERATURE))
        e.columns_sample_run(1)
        wall, dev = [], []
        for s in range(sweeps):
            ms0 = e.stats()["ms_dispersion"]
            t0 = time.perf_counter()
            e.columns_sample_run(1)
            wall.append(1e3 * (time.perf_counter() - t0)); dev.append(e.stats()["ms_dispersion"] - ms0)
        res = e.columns_sample_fetch()
        out[every] = (float(np.median(wall)), float(np.median(dev)), 100.0 * float(res["accepted"].sum()) / float(res["accepted"].sum() + res["rejected"].sum()))
    e.close()
    print("%d x %d x %d, K = %d, %d chains: the plan's runs with kernels %.1f ms; columns_sample_shape %.3f ms (the first call), %.3f ms (the median of 3), %d columns flagged" %
          (c["nx"], c["ny"], c["nz"], kmax, chains, t_kernels, t_shape[0], float(np.median(t_shape)), int((shape["flag"] == 1).sum())))
    for every, name in ((0, "single-node sweeps"), (1, "block sweeps (block_every = 1)")):
        w, d, acc = out[every]
        print("%s: median of %d -- %.3f ms wall, %.3f ms in the dispersion run on the device, %.3f ms the rest; %.1f %% of the proposals accepted" %
              (name, sweeps, w, d, w - d, acc))
    print("a block sweep costs %.3f ms more than a single-node sweep (%.2f %%)" % (out[1][0] - out[0][0], 100.0 * (out[1][0] - out[0][0]) / out[0][0]))


def marginals_mode(sweeps, chains, bins):
    """the median sweep with the marginals and the covariance on against the same build with them off in the same run, and the fetch"""
    c = io.load()
    plan = depth.slot_plan(c)
    vel = np.ascontiguousarray(np.asarray(c["vels"], np.float32).transpose(2, 1, 0))
    kmax = c["kmax"]
    e = Engine(0)
    e.dispersion_begin(vel, c["depz"], c["minthk"], kmax, kmax)
    for wave, kind, tt, first in plan:
        e.dispersion_run(wave, kind, tt, False, 0, first)
    obs = (e.dispersion_fetch(0, kmax) * 1.02).astype(np.float32)
    sigma = 0.05
    wt, lam = depth.sample_scaling(None, depth.DEFAULT_SMOOTH, sigma, obs.shape)
    out, t_fetch = {}, []
    for on in (0, 1, 0, 1):                                                          # twice each, interleaved: the second pair is reported
        e.columns_sample_begin(vel, c["depz"], c["minthk"], plan, obs, wt, chains, lam, depth.DEFAULT_SAMPLE_STEP, depth.DEFAULT_SAMPLE_SPREAD, depth.DEFAULT_SAMPLE_WIDTH,
                               depth.DEFAULT_SAMPLE_TEMPERATURE, float(c["minvel"]), float(c["maxvel"]), depth.DEFAULT_SAMPLE_SEED, 0)
        if on:
            e.columns_sample_marginals(bins, True)
        e.columns_sample_run(1)
        wall, dev = [], []
        for s in range(sweeps):
            ms0 = e.stats()["ms_dispersion"]
            t0 = time.perf_counter()
            e.columns_sample_run(1)
            wall.append(1e3 * (time.perf_counter() - t0)); dev.append(e.stats()["ms_dispersion"] - ms0)
        t0 = time.perf_counter()
        e.columns_sample_run(sweeps)
        one_call = 1e3 * (time.perf_counter() - t0) / sweeps
        if on:
            for _ in range(3):
                t0 = time.perf_counter()
                mg = e.columns_sample_marginals_fetch((0.025, 0.16, 0.5, 0.84, 0.975))
                t_fetch.append(1e3 * (time.perf_counter() - t0))
        out[on] = (float(np.median(wall)), float(np.median(dev)), one_call)
    kept = e.columns_sample_fetch()["nkept"] > 0
    e.close()
    print("%d x %d x %d, K = %d, %d chains, %d bins with the covariance: columns_sample_marginals_fetch %.3f ms (the median of 3 of the last stage), %d counts in all" %
          (c["nx"], c["ny"], c["nz"], kmax, chains, bins, float(np.median(t_fetch[-3:])), int(mg["hist"].sum(dtype=np.int64))))
    for on, name in ((0, "marginals off"), (1, "marginals on")):
        w, d, one = out[on]
        print("%s: median of %d -- %.3f ms wall, %.3f ms in the dispersion run on the device, %.3f ms the rest; %.3f ms per sweep in one call of %d" % (name, sweeps, w, d, w - d, one, sweeps))
    print("a sweep with the marginals costs %.3f ms more (%.2f %%); in one call %.3f ms more (%.2f %%); %d columns sampled" %
          (out[1][0] - out[0][0], 100.0 * (out[1][0] - out[0][0]) / out[0][0], out[1][2] - out[0][2], 100.0 * (out[1][2] - out[0][2]) / out[0][2], int(kept.sum())))


def radial_mode(sweeps, chains, long):
    """the median sweep of the radial sample stage, and the chains' figures after `long` more sweeps in one call"""
    from dsurftomo_amd import radial_posterior as rp
    c = io.load()
    t = np.asarray(c["tRc"], np.float64)
    c = dict(c, tRc=t[:7], tRg=t[7:14], tLc=t[14:20], tLg=t[20:])
    plan = depth.slot_plan(c)
    vel = np.ascontiguousarray(np.asarray(c["vels"], np.float32).transpose(2, 1, 0))
    kmax, ncol = c["kmax"], c["nx"] * c["ny"]
    e = Engine(0)
    e.dispersion_begin_radial(vel, vel, c["depz"], c["minthk"], kmax, kmax)
    for wave, kind, tt, first in plan:
        e.dispersion_run(wave, kind, tt, False, 0, first)
    obs = (e.dispersion_fetch(0, kmax) * 1.02).astype(np.float32)
    sigma = 0.05
    wt, lam, gam = rp.sample_scaling(None, depth.DEFAULT_SMOOTH, depth.DEFAULT_ANISO, sigma, obs.shape)
    burn = 1 + sweeps + long // 2
    t0 = time.perf_counter()
    e.columns_sample_radial_begin(vel, vel, c["depz"], c["minthk"], plan, obs, wt, chains, lam, gam, depth.DEFAULT_SAMPLE_STEP, depth.DEFAULT_SAMPLE_SPREAD,
                                  depth.DEFAULT_SAMPLE_WIDTH, depth.DEFAULT_SAMPLE_TEMPERATURE, float(c["minvel"]), float(c["maxvel"]), depth.DEFAULT_SAMPLE_SEED, burn, True)
    t_begin = 1e3 * (time.perf_counter() - t0)
    e.columns_sample_radial_run(1)
    wall, dev = [], []
    for s in range(sweeps):
        ms0 = e.stats()["ms_dispersion"]
        t0 = time.perf_counter()
        e.columns_sample_radial_run(1)
        wall.append(1e3 * (time.perf_counter() - t0)); dev.append(e.stats()["ms_dispersion"] - ms0)
    t0 = time.perf_counter()
    e.columns_sample_radial_run(long)
    one_call = 1e3 * (time.perf_counter() - t0) / long
    res = e.columns_sample_radial_fetch()
    e.close()
    w, d = float(np.median(wall)), float(np.median(dev))
    sm = rp.summary(res)
    print("radial: %d x %d x %d, K = %d, %d chains, %d curves per sweep, %d dispersion_run per sweep: begin %.1f ms; median of %d sweeps -- %.3f ms wall, %.3f ms in "
          "the dispersion runs on the device, %.3f ms (%.1f %%) the rest; %.3f ms per sweep in one call of %d" %
          (c["nx"], c["ny"], c["nz"], kmax, chains, ncol * chains, len(plan), t_begin, sweeps, w, d, w - d, 100.0 * (w - d) / w, one_call, long))
    print("radial: after %d sweeps (%d kept): accepted %.1f %% of the Vsv, %.1f %% of the Vsh, %.1f %% of the pair proposals; R-hat median / worst: Vsv %.4f / %.4f, "
          "Vsh %.4f / %.4f, xi %.4f / %.4f; %.1f %% of %d unknowns above 1.1; P(Vsh > Vsv) outside [0.025, 0.975] at %.1f %% of the nodes" %
          (1 + sweeps + long, int(res["nkept"].max()), 100 * sm["accepted"]["v"], 100 * sm["accepted"]["h"], 100 * sm["accepted"]["pair"], sm["rhat"]["v"]["median"],
           sm["rhat"]["v"]["worst"], sm["rhat"]["h"]["median"], sm["rhat"]["h"]["worst"], sm["rhat"]["xi"]["median"], sm["rhat"]["xi"]["worst"], 100 * sm["above"],
           sm["unknowns"], 100 * sm["sure"]))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "radial":
        arg = lambda k, default: int(sys.argv[k]) if len(sys.argv) > k else default
        radial_mode(arg(2, 30), arg(3, 64), arg(4, 400))
        return
    if len(sys.argv) > 1 and sys.argv[1] == "marginals":
        arg = lambda k, default: int(sys.argv[k]) if len(sys.argv) > k else default
        marginals_mode(arg(2, 30), arg(3, 64), arg(4, 64))
        return
    if len(sys.argv) > 2 and sys.argv[1] == "trace-shares":
        trace_shares(sys.argv[2])
        return
    if len(sys.argv) > 1 and sys.argv[1] == "block":
        block_mode(int(sys.argv[2]) if len(sys.argv) > 2 else 30, int(sys.argv[3]) if len(sys.argv) > 3 else 64)
        return
    sweeps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    chains = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    c = io.load()
    plan = depth.slot_plan(c)
    vel = np.ascontiguousarray(np.asarray(c["vels"], np.float32).transpose(2, 1, 0))
    kmax, ncol = c["kmax"], c["nx"] * c["ny"]
    e = Engine(0)
    e.dispersion_begin(vel, c["depz"], c["minthk"], kmax, kmax)
    for wave, kind, tt, first in plan:
        e.dispersion_run(wave, kind, tt, False, 0, first)
    obs = (e.dispersion_fetch(0, kmax) * 1.02).astype(np.float32)
    sigma = 0.05
    wt, lam = depth.sample_scaling(None, depth.DEFAULT_SMOOTH, sigma, obs.shape)
    t0 = time.perf_counter()
    e.columns_sample_begin(vel, c["depz"], c["minthk"], plan, obs, wt, chains, lam, depth.DEFAULT_SAMPLE_STEP, depth.DEFAULT_SAMPLE_SPREAD, depth.DEFAULT_SAMPLE_WIDTH,
                           depth.DEFAULT_SAMPLE_TEMPERATURE, float(c["minvel"]), float(c["maxvel"]), depth.DEFAULT_SAMPLE_SEED, 0)
    t_begin = 1e3 * (time.perf_counter() - t0)
    e.columns_sample_run(1)
    wall, dev = [], []
    for s in range(sweeps):
        ms0 = e.stats()["ms_dispersion"]
        t0 = time.perf_counter()
        e.columns_sample_run(1)
        wall.append(1e3 * (time.perf_counter() - t0)); dev.append(e.stats()["ms_dispersion"] - ms0)
    t0 = time.perf_counter()
    e.columns_sample_run(sweeps)
    one_call = 1e3 * (time.perf_counter() - t0) / sweeps
    res = e.columns_sample_fetch()
    e.close()
    tried = float(res["accepted"].sum() + res["rejected"].sum())
    w, d = float(np.median(wall)), float(np.median(dev))
    print("%d x %d x %d, K = %d, %d chains, %d curves per sweep, %d dispersion_run per sweep: begin %.1f ms; median of %d sweeps -- %.3f ms wall, %.3f ms in the "
          "dispersion run on the device, %.3f ms (%.1f %%) the rest: the two launches of the new kernels and the host; %.3f ms per sweep in one call of %d; "
          "%.1f %% of the proposals accepted" %
          (c["nx"], c["ny"], c["nz"], kmax, chains, ncol * chains, len(plan), t_begin, sweeps, w, d, w - d, 100.0 * (w - d) / w, one_call, sweeps,
           100.0 * float(res["accepted"].sum()) / tried))


if __name__ == "__main__":
    main()
