#!/usr/bin/env python3
"""What keeping the azimuthal step on the device changes in time.

    python tools/azimuthal_device_rate.py [--reps 5] [--chunk 512] [--skip-rays-leg] > profiles/r16_azimuthal_device_rate.log     (needs the GPU)

Two routes to the solved joint Vs | gc | gs step, on two sizes:
    host     the rows come to the host, the system is assembled in NumPy (azimuthal_weights, azimuthal_system) and goes back through
             dsa_spmv_load: invert.azimuthal_step on the Taipei example (forward + assembly + load + dsa_lsmr)
    device   the rows stay (dsa_calsurfg_azimuthal with null arrays / dsa_solve_rows_azimuthal_device), the system is built where they are
             (dsa_iteration_system_azimuthal_device): anisotropy.joint_step_device on the Taipei example (forward + system + dsa_lsmr)
On bench.py's rays-leg size (256 sources x 32 receivers at 1025^2 nodes, smooth map, nz = 9, synthetic depth kernels) there is no
input directory: the same two routes are made of the engine's calls, up to the loaded system (no LSMR in either).
Section 16's method: every leg is warmed up once, then the legs alternate in this one process, --reps times each, a host clock around each
leg (every call ends in a device synchronise); a line gives the median and the spread (min .. max) in ms, and a difference inside the
spread of the runs is no difference.  The two routes' solutions (Taipei) and systems (rays leg: dsa_spmv of one vector) are compared bit
for bit.
Then one chunk of block PSFs on the Taipei joint system: dsa_resolution_blocks with x = NULL against dsa_lsmr_resolution with x returned
and the per-block sums in NumPy, for the same --chunk spikes starting at the first gc unknown.
The inputs are the product's own (tests/golden/taipei, tests/synth.py): nothing here loads oracle/."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import synth                                           # noqa: E402
from dsurftomo_amd import anisotropy, invert           # noqa: E402
from dsurftomo_amd import io as taipei                 # noqa: E402
from dsurftomo_amd.engine import Engine, load_library  # noqa: E402

NX = 131


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def alternate(legs, reps):
    """warm every leg up once (its result kept), then reps rounds of all legs in turn: ({tag: first result}, {tag: [ms]})"""
    first = {tag: fn() for tag, fn in legs}
    t = {tag: [] for tag, _ in legs}
    for _ in range(reps):
        for tag, fn in legs:
            t0 = time.perf_counter()
            fn()
            t[tag].append(1e3 * (time.perf_counter() - t0))
    return first, t


def line(tag, ms):
    a = np.array(ms)
    return "%-28s %10.2f (%.2f .. %.2f) ms" % (tag, float(np.median(a)), float(a.min()), float(a.max()))


def verdict(t, a, b):
    ma, mb = float(np.median(t[a])), float(np.median(t[b]))
    width = max(max(t[a]) - min(t[a]), max(t[b]) - min(t[b]))
    return "%s - %s: %+.2f ms, %s" % (b, a, mb - ma, "outside the spread of the runs" if abs(mb - ma) > width else "inside the spread of the runs: no difference")


def taipei_step(lib, reps):
    c = taipei.load()
    vsf = np.asfortranarray(c["vels"].copy())
    obst = np.ascontiguousarray(c["obst"])
    quiet = lambda *_: None
    print("# taipei: %d x %d x %d, %d period slots, %d data, %d unknowns per block" % (c["nx"], c["ny"], c["nz"], c["kmax"], c["ndata"], c["nparpi"]), flush=True)
    legs = [("host (azimuthal_step)", lambda: invert.azimuthal_step(lib, c, vsf, obst, quiet)),
            ("device (joint_step_device)", lambda: anisotropy.joint_step_device(lib, c, vsf, obst, quiet))]
    first, t = alternate(legs, reps)
    h, d = first[legs[0][0]], first[legs[1][0]]
    same = bool((h["x"].view(np.uint32) == d["x"].view(np.uint32)).all()) and h["itn"] == d["itn"] and h["istop"] == d["istop"]
    print("  system %d x %d, %d entries, %d from the rays; LSMR %d iterations, istop %d; the two routes' solutions identical: %s" %
          (d["system"]["m"], d["system"]["n"], d["system"]["nar"], d["system"]["nnz_data"], d["itn"], d["istop"], same), flush=True)
    for tag, _ in legs:
        print("  " + line(tag, t[tag]), flush=True)
    print("  " + verdict(t, legs[0][0], legs[1][0]), flush=True)
    hs, ds = h["seconds"], d["seconds"]
    print("  parts of the warm-up run: host forward %.1f ms, load + LSMR %.1f ms; device forward %.1f ms, system %.1f ms, LSMR %.1f ms" %
          (1e3 * hs["forward"], 1e3 * hs["lsmr"], 1e3 * ds["forward"], 1e3 * ds["system"], 1e3 * ds["lsmr"]), flush=True)
    return c, vsf, obst


def rays_leg(lib, reps):
    """bench.py's rays-leg size through the engine's own calls, up to the loaded system"""
    f = np.float32
    nz = 9
    u = synth.units(NX, 256, 1, 32)
    ncol = NX * NX
    rng = synth.LCG(5)
    vel = (2.5 + 0.2 * np.arange(nz)[:, None, None] + np.zeros((nz, NX, NX))).astype(f)
    depz = (np.arange(nz) * (36.0 / (nz - 2))).astype(f)
    sen = [(0.02 + 0.05 * rng.uniform(nz * ncol)).reshape(nz, 1, ncol) for _ in range(3)]
    e = Engine(0)
    try:
        e.set_maps(NX, NX, synth.GOXD, synth.GOZD, synth.DVD, synth.DVD, synth.medium(NX, "smooth", 0))
        e.set_depth_kernels(vel, depz, *sen)
        e.plan(u["map_index"], u["scx"], u["scz"], u["nrec"], u["rcx"], u["rcz"])
        dall = int(np.sum(u["nrec"]))
        cap = dall * 3 * 6000
        c = dict(nx=NX, ny=NX, nz=nz, ndata=dall)
        maxvp = (NX - 2) * (NX - 2) * (nz - 1)
        t0, _ = e.solve_rows_azimuthal_device(cap, host_copy=False)
        obst = (t0 * (1.0 + 0.02 * (synth.LCG(9).uniform(dall) - 0.5))).astype(f)
        thr, w0, wa = f(3.0), f(2.0), f(0.5)
        probe = (np.random.default_rng(1).standard_normal(3 * maxvp)).astype(f)
        print("# rays leg: %d rays at %d^2 nodes, nz = %d, %d unknowns per block" % (dall, e.nnx, nz, maxvp), flush=True)

        def product():
            y = np.zeros(dall + 3 * maxvp, f)
            x = probe.copy()
            assert lib.dsa_spmv(e._h, 1, _p(x), _p(y)) == 0
            return y

        def host():
            dsyn, rw, row, col = e.solve_rows_azimuthal(cap)
            res = (obst - dsyn).astype(f)
            dw = invert.azimuthal_weights(res, thr)
            S = invert.azimuthal_system(c, rw, row, col, res, dw, w0, wa)
            e.spmv_load(S["m"], S["n"], S["rw"], S["row"], S["col"])
            return S["rw"].size, S["b"]

        def device():
            dsyn, _ = e.solve_rows_azimuthal_device(cap, host_copy=False)
            cbst = np.zeros(dall + 3 * maxvp, f); dw = np.zeros(dall, f); norm = np.zeros(3 * maxvp, f); dws = np.zeros(6, f)
            m, nar = C.c_int(0), C.c_longlong(0)
            rc = lib.dsa_iteration_system_azimuthal_device(e._h, NX, NX, nz, dall, _p(obst), _p(dsyn), thr, w0, wa, _p(cbst), _p(dw), _p(norm), C.byref(m),
                                                           C.byref(nar), _p(dws))
            assert rc == 0, lib.dsa_error_string(e._h)
            return nar.value, cbst

        nh, bh = host(); yh = product()
        nd, bd = device(); yd = product()
        same = nh == nd and bool((bh.view(np.uint32) == bd.view(np.uint32)).all()) and bool((yh.view(np.uint32) == yd.view(np.uint32)).all())
        legs = [("host (rows + NumPy + load)", host), ("device (rows + builder)", device)]
        _, t = alternate(legs, reps)
        print("  system %d x %d, %d entries; right-hand sides and A x of the two routes identical: %s" % (dall + 3 * maxvp, 3 * maxvp, nd, same), flush=True)
        for tag, _ in legs:
            print("  " + line(tag, t[tag]), flush=True)
        print("  " + verdict(t, legs[0][0], legs[1][0]), flush=True)
    finally:
        e.close()


def psf_chunk(lib, c, vsf, obst, reps, chunk):
    """one chunk of block PSFs on the Taipei joint system, the two ways"""
    step = anisotropy.joint_step_device(lib, c, vsf, obst, lambda *_: None)
    eng, n, nd, nb, damp = step["system"]["eng"], step["system"]["n"], c["ndata"], c["nparpi"], step["damp"]
    first, R = nb, min(int(chunk), n - nb)
    coords = np.ascontiguousarray(invert.unknown_coords(c))
    istop = np.zeros(R, np.int32); itn = np.zeros(R, np.int32); est = np.zeros((R, 5), np.float32)
    d2r = np.pi / 180.0
    cosl = np.cos(coords[:, 0] * d2r)

    def blocks():
        psf = np.zeros((R, 3, 4))
        assert lib.dsa_resolution_blocks(eng, R, nd, 3, first, _p(coords), damp, *invert.LSMR_ARGS, None, _p(psf), _p(istop), _p(itn), _p(est)) == 0
        return psf

    def plain_numpy():
        x = np.zeros((R, n), np.float32)
        assert lib.dsa_lsmr_resolution(eng, R, nd, None, first, None, damp, *invert.LSMR_ARGS, _p(x), None, _p(istop), _p(itn), _p(est)) == 0
        psf = np.zeros((R, 3, 4))
        for r in range(R):
            cj = (first + r) % nb
            sp = np.sin((coords[:, 0] - coords[cj, 0]) * d2r * 0.5); sl = np.sin((coords[:, 1] - coords[cj, 1]) * d2r * 0.5)
            dh = 2.0 * 6371.0 * np.arcsin(np.minimum(1.0, np.sqrt(sp * sp + cosl * cosl[cj] * sl * sl)))
            dz = coords[:, 2] - coords[cj, 2]
            xb = x[r].astype(np.float64).reshape(3, nb)
            w = xb * xb
            psf[r, :, 0] = xb[:, cj]
            psf[r, :, 1] = w.sum(axis=1); psf[r, :, 2] = (w * dh * dh).sum(axis=1); psf[r, :, 3] = (w * dz * dz).sum(axis=1)
        return psf

    legs = [("dsa_lsmr_resolution + NumPy", plain_numpy), ("dsa_resolution_blocks", blocks)]
    out, t = alternate(legs, reps)
    a, b = out[legs[0][0]], out[legs[1][0]]
    live = a[:, :, 1:] > 0
    worst = float(np.abs(b[:, :, 1:][live] / a[:, :, 1:][live] - 1.0).max()) if live.any() else 0.0
    print("# taipei block PSFs: %d spikes from unknown %d of %d; R_jj and co-located values identical: %s; worst relative difference of the sums %.3g" %
          (R, first, n, bool((a[:, :, 0] == b[:, :, 0]).all()), worst), flush=True)
    for tag, _ in legs:
        print("  " + line(tag, t[tag]), flush=True)
    print("  " + verdict(t, legs[0][0], legs[1][0]), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=512)
    ap.add_argument("--skip-rays-leg", action="store_true")
    args = ap.parse_args(argv)
    lib = invert.bind(load_library())
    c, vsf, obst = taipei_step(lib, args.reps)
    psf_chunk(lib, c, vsf, obst, args.reps, args.chunk)
    if not args.skip_rays_leg:
        rays_leg(lib, args.reps)
    return 0


if __name__ == "__main__":
    sys.exit(main())
