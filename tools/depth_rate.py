"""Where the time of one iteration of the depth inversion goes: on the Taipei example's grid and model (18 x 18 x 9,
its 26 periods), the iteration's dispersion_run calls with kernels next to dsa_columns_step -- once with the example's own plan (all 26
periods Rayleigh phase: one run) and once with the 26 periods dealt out over the four wave types (7 + 7 + 6 + 6: four runs).  Per figure the
median of `repeats` timed iterations after a warm-up one: the wall time of the calls, and DSA_STAT_MS_DISPERSION's device time of the runs.
The step's call holds two uploads, k_sen_combine, k_column_step and five downloads; the kernel's own time is what a kernel trace of this
script shows for k_column_step (rocprofv3 --kernel-trace --stats -- python tools/depth_rate.py).

    python tools/depth_rate.py [repeats]      (needs the GPU)
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dsurftomo_amd import depth, io                  # noqa: E402
from dsurftomo_amd.engine import Engine             # noqa: E402


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    c = io.load()
    t = np.asarray(c["tRc"], np.float64)
    cases = (("the example's plan", c), ("four wave types", dict(c, tRc=t[:7], tRg=t[7:14], tLc=t[14:20], tLg=t[20:])))
    vel = np.ascontiguousarray(np.asarray(c["vels"], np.float32).transpose(2, 1, 0))
    kmax = c["kmax"]
    e = Engine(0)
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
    e.close()


if __name__ == "__main__":
    main()
