"""DSA_STAT_MS_RAYS / MS_ROWS of dsa_solve_rows_azimuthal against dsa_solve_rows on the same plan:
bench.py's rays-leg size (256 sources x 32 receivers at 1025^2, smooth map, nz = 9), at one lane per ray and at four.

    python tools/azimuthal_rate.py [repeats] > profiles/r15_azimuthal_rate.log      (needs the GPU)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import synth                                        # noqa: E402
from dsurftomo_amd.engine import Engine             # noqa: E402

NX = 131


def depth_model(nx, ny, nz=9):
    """the synthetic depth kernels of bench.py's rays leg"""
    ncol = nx * ny
    rng = synth.LCG(5)
    vel = (2.5 + 0.2 * np.arange(nz)[:, None, None] + np.zeros((nz, ny, nx))).astype(np.float32)
    depz = (np.arange(nz) * (36.0 / (nz - 2))).astype(np.float32)
    sen = [(0.02 + 0.05 * rng.uniform(nz * ncol)).reshape(nz, 1, ncol) for _ in range(3)]
    return vel, depz, sen


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    u = synth.units(NX, 256, 1, 32)
    vel, depz, sen = depth_model(NX, NX)
    e = Engine(0)
    e.set_maps(NX, NX, synth.GOXD, synth.GOZD, synth.DVD, synth.DVD, synth.medium(NX, "smooth", 0))
    e.set_depth_kernels(vel, depz, *sen)
    e.plan(u["map_index"], u["scx"], u["scz"], u["nrec"], u["rcx"], u["rcz"])
    cap = int(np.sum(u["nrec"])) * 3 * 6000
    print("rays leg: %d rays at %d^2 nodes, nz = %d; best of %d calls" % (int(np.sum(u["nrec"])), e.nnx, vel.shape[0], repeats))
    for lanes in (1, 4):
        e.set_option("ray_lanes", lanes)
        best = {}
        for name, call in (("plain", e.solve_rows), ("azimuthal", e.solve_rows_azimuthal)):
            call(cap)                                                       # warm-up: allocations
            runs = []
            for _ in range(repeats):
                out = call(cap)
                st = e.stats()
                runs.append((st["ms_rays"], st["ms_rows"], out[1].size, st["ray_launches"]))
            best[name] = min(runs)
            print("lanes %d %-9s ms_rays %8.3f  ms_rows %8.3f  entries %9d  launches %d   (all runs: %s)" %
                  (lanes, name, *best[name], " ".join("%.3f/%.3f" % r[:2] for r in runs)))
        print("lanes %d ratio azimuthal / plain: rays %.3f  rows %.3f  entries %.3f" %
              (lanes, best["azimuthal"][0] / best["plain"][0], best["azimuthal"][1] / best["plain"][1], best["azimuthal"][2] / best["plain"][2]))
    e.close()


if __name__ == "__main__":
    main()
