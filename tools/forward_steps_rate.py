#!/usr/bin/env python3
"""What the device-resident ends of dsa_forward_steps add to a K-model forward call.

    python tools/forward_steps_rate.py [--K 16,64] [--reps 5] [--exact-ties 1] [--trace-only K]

On the Taipei example, default mode, dicing 8.  The first iteration's system (weight0, damp of the input file) is built on the drop-in
engine; the K steps are the solutions of one dsa_lsmr_tradeoff call over K (weight, damp) pairs, which also leaves them resident.
Every leg is warmed up once, then the legs alternate in this one process, --reps times each, a host clock around each leg (every call
ends in a device synchronise):
    host_route   line_search_candidates' loop (dsa_model_update on K copies) + dsa_forward_models + line_search_scores: the route the
                 line search takes, and the baseline
    steps_host   one dsa_forward_steps call with the K steps from the host, dsurf and measures returned
    steps_res    one dsa_forward_steps call with steps = NULL (the resident solutions) and dsurf = NULL: only the measures return
One line per K with the median and the spread (min .. max) of each leg in ms; a difference inside the spread of the runs is no
difference.  The weighted rms of the three legs are compared (largest relative difference).  --trace-only K runs nothing but three
steps_res calls (for a kernel trace).  The system is the product's own input (tests/golden/taipei): nothing here loads oracle/."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dsurftomo_amd import invert                       # noqa: E402
from dsurftomo_amd import io as taipei                 # noqa: E402
from dsurftomo_amd.engine import load_library          # noqa: E402


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def first_system(lib, c):
    """the first outer iteration up to the system: (eng, cbst, datweight, m, nar) with the matrix resident on the drop-in engine"""
    f = np.float32
    nx, ny, nz, dall, maxvp = c["nx"], c["ny"], c["nz"], c["ndata"], c["nparpi"]
    dsyn = np.zeros(dall, f)
    nar = C.c_int(0)
    head, tail = taipei._args(c)
    lib.dsa_dropin_set_capacity(0)
    assert lib.dsa_calsurfg(*head, None, None, None, _p(dsyn), *tail, C.byref(nar)) == 0, lib.dsa_dropin_error()
    eng = lib.dsa_dropin_engine()
    cbst = np.zeros(dall + maxvp, f); datweight = np.zeros(dall, f); norm = np.zeros(maxvp, f); dws = np.zeros(2, f)
    m, nar2 = C.c_int(0), C.c_longlong(0)
    rc = lib.dsa_iteration_system_device(eng, nx, ny, nz, dall, _p(np.ascontiguousarray(c["obst"])), _p(dsyn), c["threshold0"], c["weight0"], _p(cbst), _p(datweight),
                                         _p(norm), C.byref(m), C.byref(nar2), _p(dws))
    assert rc == 0, lib.dsa_error_string(eng)
    return eng, cbst, datweight, m.value, nar2.value


def spread(ms):
    a = np.array(ms)
    return dict(median=float(np.median(a)), min=float(a.min()), max=float(a.max()))


def sweep(lib, eng, c, cbst, m, nar, K):
    """K members in ONE dsa_lsmr_tradeoff call: their updates (K, n), also left resident"""
    weights = np.geomspace(0.25 * c["weight0"], 16.0 * c["weight0"], K)
    t = invert.lsmr_tradeoff_sweep(lib, eng, c, cbst, m, nar, weights, [c["damp"]], chunk=64 * ((K + 63) // 64))
    assert t["calls"] == 1
    return t["x"]


def measure(lib, eng, c, cbst, datweight, m, nar, K, reps):
    obst = np.ascontiguousarray(c["obst"])
    vsf = c["vels"]
    x = sweep(lib, eng, c, cbst, m, nar, K)
    ones = np.ones(K)

    def host_route():
        cands = []
        for k in range(K):                      # line_search_candidates with one step per member
            cands += invert.line_search_candidates(lib, c, vsf, x[k], [1.0])
        dsyn, fails = taipei.call_forward_models(c, cands, 8, lib=lib)
        return invert.line_search_scores(obst, dsyn, datweight)[0]

    def steps_host():
        r = taipei.call_forward_steps(c, vsf, x, None, 8, obst, datweight, lib=lib)
        return np.sqrt(r["measures"][:, 0, 0] / c["ndata"])

    def steps_res():
        r = taipei.call_forward_steps(c, vsf, K, None, 8, obst, datweight, want_dsurf=False, lib=lib)
        return np.sqrt(r["measures"][:, 0, 0] / c["ndata"])

    legs = [("host_route", host_route), ("steps_host", steps_host), ("steps_res", steps_res)]
    out = {tag: fn() for tag, fn in legs}       # warm-up of every leg at this K
    t = {tag: [] for tag, _ in legs}
    for _ in range(reps):
        for tag, fn in legs:
            t0 = time.perf_counter()
            fn()
            t[tag].append(1e3 * (time.perf_counter() - t0))
    worst = max(float(np.abs(out[tag] / out["host_route"] - ones).max()) for tag in ("steps_host", "steps_res"))
    r = dict(system="taipei", K=K, reps=reps, worst_relative_rms_difference=worst, **{tag: spread(v) for tag, v in t.items()})
    base = r["host_route"]
    for tag in ("steps_host", "steps_res"):
        d = base["median"] - r[tag]["median"]
        r[tag + "_saves_ms"] = d
        r[tag + "_outside_the_spread"] = bool(abs(d) > max(base["max"] - base["min"], r[tag]["max"] - r[tag]["min"]))
    return r


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--K", default="16,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--exact-ties", type=int, default=1)
    ap.add_argument("--trace-only", type=int, default=0, metavar="K")
    ap.add_argument("--json", default=None, help="also append the result lines to this file")
    args = ap.parse_args(argv)
    lib = invert.bind(load_library())
    lib.dsa_dropin_error.restype = C.c_char_p
    c = taipei.load()
    eng, cbst, datweight, m, nar = first_system(lib, c)
    assert lib.dsa_set_option(C.c_void_p(eng), b"exact_ties", C.c_double(args.exact_ties)) == 0
    if args.trace_only:
        K = args.trace_only
        sweep(lib, eng, c, cbst, m, nar, K)
        for _ in range(3):
            taipei.call_forward_steps(c, c["vels"], K, None, 8, np.ascontiguousarray(c["obst"]), datweight, want_dsurf=False, lib=lib)
        print("traced 3 resident calls of %d models on taipei" % K)
        return 0
    print("# taipei: %d x %d x %d, %d period slots, %d data, %d unknowns" % (c["nx"], c["ny"], c["nz"], c["kmax"], c["ndata"], c["nparpi"]), flush=True)
    for K in (int(v) for v in args.K.split(",")):
        r = measure(lib, eng, c, cbst, datweight, m, nar, K, args.reps)
        line = json.dumps(r)
        print(line, flush=True)
        f = lambda d: "%.2f (%.2f .. %.2f)" % (d["median"], d["min"], d["max"])
        verdict = lambda tag: "%+.2f ms, %s" % (-r[tag + "_saves_ms"], "outside the spread" if r[tag + "_outside_the_spread"] else "no difference")
        print("  taipei K %3d: host route %s ms, steps from the host %s ms (%s), resident steps without dsurf %s ms (%s); worst relative rms difference %.3g" %
              (K, f(r["host_route"]), f(r["steps_host"]), verdict("steps_host"), f(r["steps_res"]), verdict("steps_res"), r["worst_relative_rms_difference"]), flush=True)
        if args.json:
            with open(args.json, "a") as fh:
                fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
