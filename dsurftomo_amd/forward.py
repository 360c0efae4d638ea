"""Forward-model a DSurfTomo example directory on the GPU.

    python -m dsurftomo_amd.forward <directory with DSurfTomo.in, the data file and MOD> [--out PREFIX]

Reads the reference's input files (dsurftomo_amd/io.py), makes the CalSurfG call through the drop-in
entry (dispersion + depth kernels, one eikonal solve per (period, source), receiver times, rays and
Frechet rows) and writes
    PREFIX.residual.dat   per datum: distance, synthetic time, observed time   (the first three
                          columns of the reference's residualFirst.dat, main.f90:397-403)
    PREFIX.G.npz          the sensitivity matrix as COO (rw, row, col; 1-based) with its shape
--model may be repeated: several models (files beside MOD, in MOD's format) are forward-modelled in ONE call of dsa_forward_models,
times only, on the synthetic's grid (dicing 5: the times dsa_synthetic gives for each), and
    PREFIX.mNN.residual.dat    is written for model NN (1-based, in the order given), the same three columns.
There is no CPU path: without a usable GPU this fails with the engine's error text.
"""
import argparse
import sys
import time

import numpy as np

from . import io


def forward_models(args, c, models):
    """several models through one dsa_forward_models call (times only)"""
    vels = [c["vels"]] + [io.load(args.directory, m)["vels"] for m in models[1:]]
    print("%d models %d x %d x %d, %d period slots, %d data each" % (len(models), c["nx"], c["ny"], c["nz"], c["kmax"], c["ndata"]))
    t0 = time.perf_counter()
    dsyn, fails = io.call_forward_models(c, vels, 5)
    dt = time.perf_counter() - t0
    print("%d models forward-modelled in one call: %.3f s" % (len(models), dt))
    for k, m in enumerate(models):
        res = c["obst"] - dsyn[k]
        print(" model %02d %s: residual mean %.1f ms, std %.1f ms, %d dispersion curves without a root" % (k + 1, m, 1e3 * res.mean(), 1e3 * res.std(), fails[k]))
        np.savetxt("%s.m%02d.residual.dat" % (args.out, k + 1), np.column_stack([c["dist"], dsyn[k], c["obst"]]), fmt="%14.6f")
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("directory")
    ap.add_argument("--out", default="forward")
    ap.add_argument("--model", action="append", default=None, help="model file in the directory (default MOD); may be repeated")
    args = ap.parse_args(argv)
    models = args.model or ["MOD"]
    c = io.load(args.directory, models[0])
    if len(models) > 1:
        return forward_models(args, c, models)
    print("model %d x %d x %d, %d period slots, %d data, %d parameters" % (c["nx"], c["ny"], c["nz"], c["kmax"], c["ndata"], c["nparpi"]))
    t0 = time.perf_counter()
    dsyn, rw, row, col = io.call_calsurfg(c)
    dt = time.perf_counter() - t0
    res = c["obst"] - dsyn
    print("CalSurfG on the device: %.3f s; %d matrix entries; residual mean %.1f ms, std %.1f ms" % (dt, rw.size, 1e3 * res.mean(), 1e3 * res.std()))
    np.savetxt(args.out + ".residual.dat", np.column_stack([c["dist"], dsyn, c["obst"]]), fmt="%14.6f")
    np.savez_compressed(args.out + ".G.npz", rw=rw, row=row, col=col, shape=np.array([c["ndata"], c["nparpi"]]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
