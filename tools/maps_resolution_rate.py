"""What dsa_maps_resolution costs, next to the iterative route to the same columns.  Two systems, each built on the
device by the map loop's own calls (start maps, plan, dsa_solve_rows_maps with the rows left on the device,
dsa_iteration_system_maps_device):

  taipei    tests/golden/taipei: 26 maps of 16 x 16 = 256 unknowns, the input's weight0 and damp
  fixture   the 35 x 35 synthetic fixture of tests/test_gpu_maps.py: 2 maps of 1089 unknowns, 576 rays, weight 2, damp 0.5

Per system: the wall time of the whole call (the median of `repeats` calls after a warm-up one; the call ends in a stream synchronise),
then dsa_resolution_blocks over ALL n unit spikes of the same system in one call, LSMR_ARGS (one timed call after a warm-up of 64 spikes),
and the largest difference between its fp32 answers and the dense R columns.  The kernels' own times are a kernel trace's:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/maps_resolution_rate.py 5 fixture
    python tools/depth_rate.py trace-medians DIR/.../*_kernel_trace.csv

    python tools/maps_resolution_rate.py [repeats] [taipei | fixture]      (needs the GPU; with a name: that system alone)
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from dsurftomo_amd import io, maps                                  # noqa: E402
from dsurftomo_amd.analyses.common import LSMR_ARGS                 # noqa: E402
from dsurftomo_amd.engine import Engine                             # noqa: E402


def taipei():
    c = io.load(os.path.join(ROOT, "tests", "golden", "taipei"))
    u = maps.period_plan(c)
    e = Engine(0)
    maps.start_maps(e, c, u, "mean")
    maps.plan_engine(e, u)
    obst = np.ascontiguousarray(c["obst"], np.float32)
    dsyn, _ = e.solve_rows_maps_device(False)
    S = e.iteration_system_maps_device(c["nx"], c["ny"], u["nmaps"], 1, obst, dsyn, float(c["threshold0"]), float(c["weight0"]), float(c["weight0"]))
    return e, (c["nx"], c["ny"], u["nmaps"], 1, obst.size, float(c["damp"])), S


def fixture():
    import synth
    import test_gpu_maps as TM
    e, u = TM.fresh()
    dsyn, _ = e.solve_rows_maps_device(False)
    obst = (dsyn * (1.0 + 0.04 * (synth.LCG(91).uniform(dsyn.size) - 0.5))).astype(np.float32)
    S = e.iteration_system_maps_device(TM.NX, TM.NX, TM.NMAPS, 1, obst, dsyn, np.float32(1.2), np.float32(2.0), np.float32(2.0))
    return e, (TM.NX, TM.NX, TM.NMAPS, 1, dsyn.size, 0.5), S


def measure(name, make, repeats):
    e, args, S = make()
    try:
        nx, ny, nmaps, nblocks, ndata, damp = args
        layer = (nx - 2) * (ny - 2)
        nm, n = nblocks * layer, nblocks * nmaps * layer
        e.maps_resolution(*args)
        times = []
        for _ in range(repeats):
            t = time.perf_counter()
            res = e.maps_resolution(*args)
            times.append(time.perf_counter() - t)
        print("%s: %d maps of %d unknowns, %d data (%d used), %d entries: dsa_maps_resolution %.2f ms (median of %d; %.2f to %.2f), flags %s" %
              (name, nmaps, nm, ndata, int(res["nused"].sum()), int(S["nar"]), 1e3 * np.median(times), repeats, 1e3 * min(times), 1e3 * max(times),
               np.bincount(res["flag"], minlength=3).tolist()))
        coords = np.random.default_rng(1).random((nmaps * layer, 3))
        e.lsmr_resolution_blocks(ndata, damp, nblocks, (0, 64), coords, True, *LSMR_ARGS)
        t = time.perf_counter()
        it = e.lsmr_resolution_blocks(ndata, damp, nblocks, (0, n), coords, True, *LSMR_ARGS)
        t_it = time.perf_counter() - t
        worst = 0.0
        for k in range(nmaps):
            R = e.maps_resolution(*args, r_map=k)["R"]
            cols = np.concatenate([np.arange((B * nmaps + k) * layer, (B * nmaps + k + 1) * layer) for B in range(nblocks)])
            X = it["x"][cols][:, cols].astype(np.float64)                      # X[q, l]: the answer at l to the spike at q = R[l, q]
            worst = max(worst, float(np.abs(X.T - R).max()))
        print("%s: dsa_resolution_blocks over all %d spikes %.1f ms (itn median %d, largest %d); largest |x - R column| %.3g" %
              (name, n, 1e3 * t_it, int(np.median(it["itn"])), int(it["itn"].max()), worst))
    finally:
        e.close()


def main(argv):
    repeats = int(argv[0]) if argv and argv[0].isdigit() else 5
    only = [a for a in argv if not a.isdigit()]
    for name, make in (("taipei", taipei), ("fixture", fixture)):
        if not only or name in only:
            measure(name, make, repeats)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
