"""Where the time of one iteration of the depth inversion goes: on the Taipei example's grid and model (18 x 18 x 9,
its 26 periods), the iteration's dispersion_run calls with kernels next to dsa_columns_step -- once with the example's own plan (all 26
periods Rayleigh phase: one run) and once with the 26 periods dealt out over the four wave types (7 + 7 + 6 + 6: four runs).  Per figure the
median of `repeats` timed iterations after a warm-up one: the wall time of the calls, and DSA_STAT_MS_DISPERSION's device time of the runs.
The step's call holds two uploads, k_sen_combine, k_column_step and five downloads; the kernel's own time is what a kernel trace of this
script shows for k_column_step (rocprofv3 --kernel-trace --stats -- python tools/depth_rate.py).

The resolution's leg: dsa_columns_resolution on the same grid and plan (K = 26, M = 8) after one set of runs, without
and with the full R, and at the stage's limits on a 5 x 5 grid (nz = 64, K = 60: 15 phase and 15 group periods of each wave type, the one
launch that asks for more than 64 KB of LDS) -- the wall time of the whole call, `repeats` timed calls after a warm-up one (the call leaves
the state as it is, so the runs are not repeated); k_column_resolution's own time is the kernel trace's.

The radial leg: the four-wave-type plan on a radial stage, Vsh 3 % above Vsv -- the iteration's runs next to
dsa_columns_step_radial, timed as the first leg is -- and one step at the stage's limits (the one launch above 64 KB of LDS);
k_column_step_radial's own time stands beside k_column_step's in the same kernel trace.

The lateral leg: dsa_columns_step_lateral on the example's grid and plan at lateral 0.2 and 1 (tol 1e-8), each timed
call after fresh runs, next to dsa_columns_step on the same state: the conjugate-gradient iterations, the call's wall time, and an upper bound of the
time per iteration: the difference of the two calls' wall times over itn, which also holds the set-up's extra launches, the host's look at
the done flag every 16th iteration and the up to 15 empty iterations launched after the flag was set.

The radial lateral leg: dsa_columns_step_radial_lateral on the radial leg's stage (the four-wave-type plan, Vsh 3 %
above Vsv) at (lateral, lateral_aniso) = (0.2, 0.2), (0.3, 0.6) and (0, 1) (tol 1e-8), timed as the lateral leg is, next to
dsa_columns_step_radial on the same state.

The radial resolution's leg: dsa_columns_resolution_radial on the radial leg's stage (the four-wave-type plan, Vsh 3 %
above Vsv; K = 26, 2M = 16) after one set of runs, without and with the full R, and at the stage's limits on the 5 x 5 grid (nz = 64,
K = 60: the one launch that asks for 158 712 bytes of LDS) -- the wall time of the whole call, `repeats` timed calls after a warm-up one.
On each stage one dsa_columns_step_radial per timed call of the first series (after fresh runs) and, on a plain stage holding the same
model, as many dsa_columns_resolution calls follow, so that one kernel trace of the leg holds k_column_resolution_radial,
k_column_step_radial and k_column_resolution side by side:
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/depth_rate.py 9 radial-resolution
    python tools/depth_rate.py trace-medians DIR/.../*_kernel_trace.csv
prints per kernel and grid size the median duration of its launches, the first one (the warm-up) left out.

The lateral resolution's leg: dsa_columns_resolution_lateral on the lateral leg's stage and observations at lateral
0.2 and 1 (tol 1e-8) after one set of runs (the call leaves the state as it is): every unknown as a point-spread function and as a row of
the averaging kernel (2 x 2 048 members) in one call, next to the first 64 of them one per call -- the wall time of the calls, `repeats`
timed series after a warm-up one, and from them the time per member of either way.

The azimuthal leg: dsa_columns_azimuthal next to dsa_columns_resolution (without R) on the example's grid and plan
(K = 26 Rayleigh periods, M = 8) and at the stage's limits on the 5 x 5 grid (nz = 64, K = 60, 30 of them Love slots: the one launch that
asks for 81 048 bytes of LDS) after one set of runs, the two calls in turn -- the wall time of the whole calls, `repeats` timed pairs after
a warm-up one.  One kernel trace of the leg holds k_column_azimuthal, k_sen_azimuthal, k_column_resolution and k_sen_combine side by side
(trace-medians, as above).

    python tools/depth_rate.py [repeats] [lateral | radial-lateral | radial-resolution | lateral-resolution | azimuthal]      (needs the GPU; with a name: that leg alone)
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dsurftomo_amd import depth, io                  # noqa: E402
from dsurftomo_amd.engine import Engine             # noqa: E402


def trace_medians(path):
    """per (kernel, grid size) of a rocprofv3 kernel trace (csv): the launches and the median of their durations in us without the first"""
    import csv
    rows = {}
    with open(path, newline="") as fh:
        for r in csv.DictReader(fh):
            name = r["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0].split("::")[-1]
            rows.setdefault((name, r.get("Grid_Size_X", r.get("Grid_Size", "?"))), []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    for (name, grid), spans in sorted(rows.items()):
        d = [1e-3 * (b - a) for a, b in sorted(spans)]
        rest = d[1:] if len(d) > 1 else d
        print("%-40s grid %-8s %3d launches, median without the first %.1f us (first %.1f, min %.1f, max %.1f)" % (name, grid, len(d), np.median(rest), d[0], min(rest), max(rest)))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "trace-medians":
        trace_medians(sys.argv[2])
        return
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    c = io.load()
    t = np.asarray(c["tRc"], np.float64)
    cases = (("the example's plan", c), ("four wave types", dict(c, tRc=t[:7], tRg=t[7:14], tLc=t[14:20], tLg=t[20:])))
    vel = np.ascontiguousarray(np.asarray(c["vels"], np.float32).transpose(2, 1, 0))
    kmax = c["kmax"]
    e = Engine(0)
    if "lateral" in sys.argv[2:]:
        lateral_leg(e, repeats, vel, c, depth.slot_plan(c), kmax)
        e.close()
        return
    if "lateral-resolution" in sys.argv[2:]:
        lateral_resolution_leg(e, repeats, vel, c, depth.slot_plan(c), kmax)
        e.close()
        return
    if "azimuthal" in sys.argv[2:]:
        azimuthal_leg(e, repeats, "the example's grid", vel, c["depz"], c["minthk"], depth.slot_plan(c), kmax)
        limits, depz, minthk, lplan, lk = limits_case()
        azimuthal_leg(e, repeats, "the limits", limits, depz, minthk, lplan, lk)
        e.close()
        return
    if "radial-lateral" in sys.argv[2:]:
        radial_lateral_leg(e, repeats, vel, c, depth.slot_plan(cases[1][1]), kmax)
        e.close()
        return
    if "radial-resolution" in sys.argv[2:]:
        radial_resolution_legs(e, repeats, vel, c, depth.slot_plan(cases[1][1]), kmax)
        e.close()
        return
    for name, case in cases:
        plan = depth.slot_plan(case)
        e.dispersion_begin(vel, c["depz"], c["minthk"], kmax, kmax)
        for wave, kind, tt, first in plan:
            e.dispersion_run(wave, kind, tt, False, 0, first)
        obs = (e.dispersion_fetch(0, kmax) * 1.02).astype(np.float32)             # 2 % off the model's own curves: small steps, nothing clipped
        runs, dev, step = [], [], []
        for it in range(repeats + 1):
            ms0 = e.stats()["ms_dispersion"]
            t0 = time.perf_counter()
            for wave, kind, tt, first in plan:
                e.dispersion_run(wave, kind, tt, True, first, first)
            t1 = time.perf_counter()
            out = e.columns_step(obs, None, depth.DEFAULT_SMOOTH, depth.DEFAULT_DAMP, 1e-4, float(c["minvel"]), float(c["maxvel"]))
            t2 = time.perf_counter()
            if it:
                runs.append(1e3 * (t1 - t0)); dev.append(e.stats()["ms_dispersion"] - ms0); step.append(1e3 * (t2 - t1))
        assert not out["flag"].any() and out["nused"].sum() == kmax * (c["nx"] - 2) * (c["ny"] - 2)
        print("%-20s %d x %d x %d, K = %d, %d dispersion_run: median of %d -- runs %.3f ms wall (%.3f ms on the device), columns_step %.3f ms wall; all steps: %s" %
              (name, c["nx"], c["ny"], c["nz"], kmax, len(plan), repeats, np.median(runs), np.median(dev), np.median(step), " ".join("%.3f" % s for s in step)))
    radial_leg(e, repeats, "radial, four types", vel, c["depz"], c["minthk"], depth.slot_plan(cases[1][1]), kmax, float(c["minvel"]), float(c["maxvel"]))
    resolution_leg(e, repeats, "the example's grid", vel, c["depz"], c["minthk"], depth.slot_plan(c), kmax)
    limits, depz, minthk, lplan, lk = limits_case()
    resolution_leg(e, repeats, "the limits", limits, depz, minthk, lplan, lk)
    radial_leg(e, 1, "radial, the limits", limits, depz, minthk, lplan, lk, 0.5, 6.0)
    lateral_leg(e, repeats, vel, c, depth.slot_plan(c), kmax)
    radial_lateral_leg(e, repeats, vel, c, depth.slot_plan(cases[1][1]), kmax)
    radial_resolution_legs(e, repeats, vel, c, depth.slot_plan(cases[1][1]), kmax)
    lateral_resolution_leg(e, repeats, vel, c, depth.slot_plan(c), kmax)
    e.close()


def lateral_resolution_leg(e, repeats, vel, c, plan, kmax):
    nz, ny, nx = vel.shape
    e.dispersion_begin(vel, c["depz"], c["minthk"], kmax, kmax)
    for wave, kind, tt, first in plan:
        e.dispersion_run(wave, kind, tt, True, first, first)
    i = np.arange(nx)[None, :]; j = np.arange(ny)[:, None]
    obs = (e.dispersion_fetch(0, kmax) * (1.0 + 0.02 * np.cos(0.9 * i + 0.5 * j).ravel()[None, :])).astype(np.float32)      # the lateral leg's
    args = (depth.DEFAULT_SMOOTH, depth.DEFAULT_DAMP)
    n = (nx - 2) * (ny - 2) * (nz - 1)
    kind = np.repeat(np.array([0, 1], np.int32), n); index = np.tile(np.arange(n, dtype=np.int32), 2)
    single = 64
    for lateral in (0.2, 1.0):
        call = lambda k, q: e.columns_resolution_lateral(obs, None, *args, lateral, k, q, None, depth.DEFAULT_LATERAL_TOL, depth.DEFAULT_LATERAL_MAXIT)
        batch, alone = [], []
        for it in range(repeats + 1):
            t0 = time.perf_counter()
            out = call(kind, index)
            t1 = time.perf_counter()
            ones = [call(kind[s:s + 1], index[s:s + 1]) for s in range(single)]
            t2 = time.perf_counter()
            if it:
                batch.append(1e3 * (t1 - t0)); alone.append(1e3 * (t2 - t1))
        assert not out["flag"].any() and (out["istop"] == 1).all()
        assert all(np.array_equal(o["measures"][0].view(np.uint64), out["measures"][s].view(np.uint64)) and o["itn"][0] == out["itn"][s] for s, o in enumerate(ones))
        print("%-22s %d x %d x %d, K = %d: median of %d -- %d members in one call %.3f ms wall (%.1f us a member), itn %d to %d; the first %d one per call %.3f ms wall "
              "(%.1f us a member, itn %d to %d): %.1f times as long a member; all batched calls: %s" %
              ("lateral resolution %g" % lateral, nx, ny, nz, kmax, repeats, len(kind), np.median(batch), 1e3 * np.median(batch) / len(kind), out["itn"].min(), out["itn"].max(),
               single, np.median(alone), 1e3 * np.median(alone) / single, out["itn"][:single].min(), out["itn"][:single].max(),
               (np.median(alone) / single) / (np.median(batch) / len(kind)), " ".join("%.3f" % w for w in batch)))


def limits_case():
    """the stage's limits on a 5 x 5 grid: (model (64, 5, 5), depz, minthk, plan of 15 phase and 15 group periods of each wave type, 60)"""
    nz = 64
    k = np.arange(nz)[:, None, None]; i = np.arange(5)[None, None, :]; j = np.arange(5)[None, :, None]
    limits = np.ascontiguousarray((2.6 + 1.9 * k / (nz - 1)) * (1.0 + 0.05 * np.sin(0.7 * i + 0.3 * k) * np.cos(0.5 * j)), np.float32)
    depz = np.concatenate([[0.0], np.cumsum(np.round(2.0 + 4.0 * np.arange(nz - 1) / (nz - 2)))]).astype(np.float32)
    phase, group = np.linspace(3.0, 45.0, 15), np.linspace(4.0, 46.0, 15)
    return limits, depz, 2.0, [(2, 0, phase, 0), (2, 1, group, 15), (1, 0, phase, 30), (1, 1, group, 45)], 60


def radial_resolution_legs(e, repeats, vel, c, plan, kmax):
    radial_resolution_leg(e, repeats, "the example's grid", vel, c["depz"], c["minthk"], plan, kmax, float(c["minvel"]), float(c["maxvel"]))
    limits, depz, minthk, lplan, lk = limits_case()
    radial_resolution_leg(e, repeats, "the limits", limits, depz, minthk, lplan, lk, 0.5, 6.0)


def radial_resolution_leg(e, repeats, name, vel, depz, minthk, plan, kmax, minvel, maxvel):
    nz, ny, nx = vel.shape
    vsh = vel.copy()
    vsh[:-1] = vsh[:-1] * np.float32(1.03)
    args = (depth.DEFAULT_SMOOTH, depth.DEFAULT_DAMP, depth.DEFAULT_ANISO)

    def runs():
        for wave, kind, tt, first in plan:
            e.dispersion_run(wave, kind, tt, True, first, first)

    e.dispersion_begin_radial(vel, vsh, depz, minthk, kmax, kmax)
    t0 = time.perf_counter()
    runs()
    t1 = time.perf_counter()
    pv = e.dispersion_fetch(0, kmax)
    obs = np.where(pv > 0, pv * 1.02, 0.0).astype(np.float32)
    for full in (False, True):
        wall = []
        for it in range(repeats + 1):
            t2 = time.perf_counter()
            out = e.columns_resolution_radial(obs, None, *args, full)
            if it:
                wall.append(1e3 * (time.perf_counter() - t2))
        ok = out["flag"].reshape(ny, nx)[1:-1, 1:-1] == 0
        tr = out["trace"].sum(axis=0).reshape(ny, nx)[1:-1, 1:-1][ok]
        print("%-20s %d x %d x %d, K = %d (runs %.1f ms): columns_resolution_radial %s, median of %d -- %.3f ms wall; %d of %d columns resolved, sum of the traces %.3f to %.3f; all calls: %s" %
              (name, nx, ny, nz, kmax, 1e3 * (t1 - t0), "with the full R" if full else "without R", repeats, np.median(wall), int(ok.sum()), ok.size, tr.min(), tr.max(),
               " ".join("%.3f" % w for w in wall)))
    # the neighbours, for the kernel trace: the radial step on this stage, the plain resolution on a plain stage holding the Vsv model
    for it in range(repeats + 1):
        if it:
            runs()
        e.columns_step_radial(obs, None, *args, 1e-4, minvel, maxvel)
    e.dispersion_begin(vel, depz, minthk, kmax, kmax)
    runs()
    for it in range(repeats + 1):
        e.columns_resolution(obs, None, depth.DEFAULT_SMOOTH, depth.DEFAULT_DAMP)


def radial_lateral_leg(e, repeats, vel, c, plan, kmax):
    nz, ny, nx = vel.shape
    vsh = vel.copy()
    vsh[:-1] = vsh[:-1] * np.float32(1.03)
    e.dispersion_begin_radial(vel, vsh, c["depz"], c["minthk"], kmax, kmax)
    for wave, kind, tt, first in plan:
        e.dispersion_run(wave, kind, tt, False, 0, first)
    # the lateral leg's observations: up to 2 % off the models' own curves, the sign changing across the grid
    i = np.arange(nx)[None, :]; j = np.arange(ny)[:, None]
    pv = e.dispersion_fetch(0, kmax)
    obs = np.where(pv > 0, pv * (1.0 + 0.02 * np.cos(0.9 * i + 0.5 * j).ravel()[None, :]), 0.0).astype(np.float32)
    args = (depth.DEFAULT_SMOOTH, depth.DEFAULT_DAMP, depth.DEFAULT_ANISO)
    clip = (1e-4, float(c["minvel"]), float(c["maxvel"]))

    def timed(call):
        wall = []
        for it in range(repeats + 1):
            for wave, kind, tt, first in plan:
                e.dispersion_run(wave, kind, tt, True, first, first)
            t0 = time.perf_counter()
            out = call()
            if it:
                wall.append(1e3 * (time.perf_counter() - t0))
        return out, wall

    _, alone = timed(lambda: e.columns_step_radial(obs, None, *args, *clip))
    for lateral, aniso in ((0.2, 0.2), (0.3, 0.6), (0.0, 1.0)):
        out, wall = timed(lambda: e.columns_step_radial_lateral(obs, None, *args, lateral, aniso, *clip, depth.DEFAULT_LATERAL_TOL, depth.DEFAULT_LATERAL_MAXIT))
        assert not out["flag"].any() and out["istop"] == 1 and out["itn"] >= 1
        print("%-20s %d x %d x %d, K = %d: median of %d -- columns_step_radial_lateral %.3f ms wall, itn %d (at most %.1f us per iteration: the whole difference over itn), columns_step_radial %.3f ms wall; all calls: %s" %
              ("radial lateral %g %g" % (lateral, aniso), nx, ny, nz, kmax, repeats, np.median(wall), out["itn"], 1e3 * (np.median(wall) - np.median(alone)) / max(out["itn"], 1),
               np.median(alone), " ".join("%.3f" % w for w in wall)))


def lateral_leg(e, repeats, vel, c, plan, kmax):
    nz, ny, nx = vel.shape
    e.dispersion_begin(vel, c["depz"], c["minthk"], kmax, kmax)
    for wave, kind, tt, first in plan:
        e.dispersion_run(wave, kind, tt, False, 0, first)
    # up to 2 % off the model's own curves, the sign changing across the grid: on a laterally uniform model equal misfits everywhere would
    # give every column the same step, which the coupling leaves alone (itn 0)
    i = np.arange(nx)[None, :]; j = np.arange(ny)[:, None]
    obs = (e.dispersion_fetch(0, kmax) * (1.0 + 0.02 * np.cos(0.9 * i + 0.5 * j).ravel()[None, :])).astype(np.float32)
    args = (depth.DEFAULT_SMOOTH, depth.DEFAULT_DAMP)
    clip = (1e-4, float(c["minvel"]), float(c["maxvel"]))

    def timed(call):
        wall = []
        for it in range(repeats + 1):
            for wave, kind, tt, first in plan:
                e.dispersion_run(wave, kind, tt, True, first, first)
            t0 = time.perf_counter()
            out = call()
            if it:
                wall.append(1e3 * (time.perf_counter() - t0))
        return out, wall

    _, alone = timed(lambda: e.columns_step(obs, None, *args, *clip))
    for lateral in (0.2, 1.0):
        out, wall = timed(lambda: e.columns_step_lateral(obs, None, *args, lateral, *clip, depth.DEFAULT_LATERAL_TOL, depth.DEFAULT_LATERAL_MAXIT))
        assert not out["flag"].any() and out["istop"] == 1 and out["itn"] >= 1
        print("%-20s %d x %d x %d, K = %d: median of %d -- columns_step_lateral %.3f ms wall, itn %d (at most %.1f us per iteration: the whole difference over itn), columns_step %.3f ms wall; all calls: %s" %
              ("lateral %g" % lateral, nx, ny, nz, kmax, repeats, np.median(wall), out["itn"], 1e3 * (np.median(wall) - np.median(alone)) / max(out["itn"], 1),
               np.median(alone), " ".join("%.3f" % w for w in wall)))


def radial_leg(e, repeats, name, vel, depz, minthk, plan, kmax, minvel, maxvel):
    nz, ny, nx = vel.shape
    vsh = vel.copy()
    vsh[:-1] = vsh[:-1] * np.float32(1.03)
    e.dispersion_begin_radial(vel, vsh, depz, minthk, kmax, kmax)
    for wave, kind, tt, first in plan:
        e.dispersion_run(wave, kind, tt, False, 0, first)
    pv = e.dispersion_fetch(0, kmax)
    obs = np.where(pv > 0, pv * 1.02, 0.0).astype(np.float32)
    runs, dev, step = [], [], []
    for it in range(repeats + 1):
        ms0 = e.stats()["ms_dispersion"]
        t0 = time.perf_counter()
        for wave, kind, tt, first in plan:
            e.dispersion_run(wave, kind, tt, True, first, first)
        t1 = time.perf_counter()
        out = e.columns_step_radial(obs, None, depth.DEFAULT_SMOOTH, depth.DEFAULT_DAMP, depth.DEFAULT_ANISO, 1e-4, minvel, maxvel)
        t2 = time.perf_counter()
        if it:
            runs.append(1e3 * (t1 - t0)); dev.append(e.stats()["ms_dispersion"] - ms0); step.append(1e3 * (t2 - t1))
    assert not out["flag"].any() and out["nused"].sum() == int((pv.reshape(kmax, ny, nx)[:, 1:-1, 1:-1] > 0).sum())
    print("%-20s %d x %d x %d, K = %d, %d dispersion_run: median of %d -- runs %.3f ms wall (%.3f ms on the device), columns_step_radial %.3f ms wall; all steps: %s" %
          (name, nx, ny, nz, kmax, len(plan), repeats, np.median(runs), np.median(dev), np.median(step), " ".join("%.3f" % s for s in step)))


def resolution_leg(e, repeats, name, vel, depz, minthk, plan, kmax):
    nz, ny, nx = vel.shape
    e.dispersion_begin(vel, depz, minthk, kmax, kmax)
    t0 = time.perf_counter()
    for wave, kind, tt, first in plan:
        e.dispersion_run(wave, kind, tt, True, first, first)
    t1 = time.perf_counter()
    obs = np.where(e.dispersion_fetch(0, kmax) > 0, 3.0, 0.0).astype(np.float32)
    for full in (False, True):
        wall = []
        for it in range(repeats + 1):
            t2 = time.perf_counter()
            out = e.columns_resolution(obs, None, depth.DEFAULT_SMOOTH, depth.DEFAULT_DAMP, full)
            if it:
                wall.append(1e3 * (time.perf_counter() - t2))
        ok = out["flag"].reshape(ny, nx)[1:-1, 1:-1] == 0
        print("%-20s %d x %d x %d, K = %d (runs %.1f ms): columns_resolution %s, median of %d -- %.3f ms wall; %d of %d columns resolved, trace %.3f to %.3f; all calls: %s" %
              (name, nx, ny, nz, kmax, 1e3 * (t1 - t0), "with the full R" if full else "without R", repeats, np.median(wall), int(ok.sum()), ok.size,
               out["trace"].reshape(ny, nx)[1:-1, 1:-1][ok].min(), out["trace"].reshape(ny, nx)[1:-1, 1:-1][ok].max(), " ".join("%.3f" % w for w in wall)))


def azimuthal_leg(e, repeats, name, vel, depz, minthk, plan, kmax):
    nz, ny, nx = vel.shape
    e.dispersion_begin(vel, depz, minthk, kmax, kmax)
    t0 = time.perf_counter()
    for wave, kind, tt, first in plan:
        e.dispersion_run(wave, kind, tt, True, first, first)
    t1 = time.perf_counter()
    pv = e.dispersion_fetch(0, kmax)
    obs = np.where(pv > 0, pv, 0.0).astype(np.float32)
    rng = np.random.default_rng(35)
    a1 = (0.02 * obs * rng.standard_normal(obs.shape)).astype(np.float32); a2 = (0.02 * obs * rng.standard_normal(obs.shape)).astype(np.float32)
    res, azi = [], []
    for it in range(repeats + 1):
        t2 = time.perf_counter()
        e.columns_resolution(obs, None, depth.DEFAULT_SMOOTH, depth.DEFAULT_DAMP)
        t3 = time.perf_counter()
        out = e.columns_azimuthal(obs, a1, a2, None, depth.DEFAULT_SMOOTH, depth.DEFAULT_DAMP)
        t4 = time.perf_counter()
        if it:
            res.append(1e3 * (t3 - t2)); azi.append(1e3 * (t4 - t3))
    ok = out["flag"].reshape(ny, nx)[1:-1, 1:-1] == 0
    print("%-20s %d x %d x %d, K = %d (runs %.1f ms), median of %d -- columns_resolution without R %.3f ms wall, columns_azimuthal %.3f ms wall; %d of %d columns solved, "
          "%d data used; all azimuthal calls: %s" % (name, nx, ny, nz, kmax, 1e3 * (t1 - t0), repeats, np.median(res), np.median(azi), int(ok.sum()), ok.size,
                                                      int(out["nused"].sum()), " ".join("%.3f" % w for w in azi)))


if __name__ == "__main__":
    main()
