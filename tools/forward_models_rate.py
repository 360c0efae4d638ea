#!/usr/bin/env python3
"""dsa_forward_models (K models in one call) against K sequential single-model calls and against K dsa_calsurfg calls.

    python tools/forward_models_rate.py [--systems taipei[,big]] [--K 1,4,16,64] [--reps 5] [--orders 0,1] [--big-sources 1000]
                                        [--exact-ties 1] [--trace-only K]

Per system, unit order (option forward_models_order: 0 model-major, 1 period-major) and K: the K models are the system's own scaled by
1 + 0.04 (k / K - 1/2), dicing 8, default mode.  Every leg is warmed up once, then the legs run alternating in this one process,
--reps times each, a host clock around each leg (every call ends in a device synchronise):
    batch      one dsa_forward_models call with K models
    single     K dsa_forward_models calls with one model each
    calsurfg   K dsa_calsurfg calls with the rows left on the device: what a line search costs without the entry (it pays for rays and rows)
One line per (system, order, K) with the median and the spread (min .. max) of each leg in ms, the ratios of the medians, and whether
the batch beats the single leg by more than that leg's spread (max - min).  The batch's columns are compared with the single calls'
(largest difference in s).  --trace-only K runs nothing but three batched calls of K models on the first system (for a kernel trace).
The systems are the product's own inputs (tests/golden/taipei, tests/synth.py): nothing here loads oracle/."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _libs as L            # noqa: E402  (L.ptr only)
import synth                 # noqa: E402
from dsurftomo_amd import io as taipei                 # noqa: E402
from dsurftomo_amd.engine import load_library          # noqa: E402


def models_of(c, K):
    return [np.asfortranarray((c["vels"].astype(np.float64) * (1.0 + 0.04 * (k / K - 0.5))).astype(np.float32)) for k in range(K)]


def calsurfg_device_rows(lib, c, m):
    cc = dict(c); cc["vels"] = m
    head, tail = taipei._args(cc)
    dsyn = np.zeros(c["ndata"], np.float32)
    nar = C.c_int(0)
    lib.dsa_dropin_set_capacity(0)
    rc = lib.dsa_calsurfg(*head, None, None, None, L.ptr(dsyn), *tail, C.byref(nar))
    assert rc == 0, lib.dsa_dropin_error()
    return dsyn


def stats(lib):
    st = np.zeros(64)
    assert lib.dsa_get_stats(C.c_void_p(lib.dsa_dropin_engine()), L.ptr(st)) == 0
    return st


def spread(ms):
    a = np.array(ms)
    return dict(median=float(np.median(a)), min=float(a.min()), max=float(a.max()))


def measure(lib, name, c, K, order, reps, with_calsurfg):
    eng = C.c_void_p(lib.dsa_dropin_engine())
    assert lib.dsa_set_option(eng, b"forward_models_order", C.c_double(order)) == 0
    models = models_of(c, K)

    def batch():
        return taipei.call_forward_models(c, models, 8, lib=lib)[0]

    def single():
        return np.stack([taipei.call_forward_models(c, [m], 8, lib=lib)[0][0] for m in models])

    def cals():
        return np.stack([calsurfg_device_rows(lib, c, m) for m in models])

    legs = [("batch", batch), ("single", single)] + ([("calsurfg", cals)] if with_calsurfg else [])
    out = {}
    for tag, fn in legs:          # warm-up of every leg at this K
        out[tag] = fn()
    st = None
    t = {tag: [] for tag, _ in legs}
    for _ in range(reps):
        for tag, fn in legs:
            t0 = time.perf_counter()
            fn()
            t[tag].append(1e3 * (time.perf_counter() - t0))
            if tag == "batch":
                st = stats(lib)
    r = dict(system=name, order=order, K=K, reps=reps, units=int(st[5]), bundle_size=int(st[26]), bundled_units=int(st[28]), ms_dispersion=float(st[17]),
             ms_total=float(st[0]), worst_vs_single=float(np.abs(out["batch"] - out["single"]).max()), **{tag: spread(v) for tag, v in t.items()})
    seq = r["single"]
    r["speedup_vs_single"] = seq["median"] / r["batch"]["median"]
    r["beats_single_by_more_than_its_spread"] = bool(seq["median"] - r["batch"]["median"] > seq["max"] - seq["min"])
    if with_calsurfg:
        r["speedup_vs_calsurfg"] = r["calsurfg"]["median"] / r["batch"]["median"]
    return r


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--systems", default="taipei")
    ap.add_argument("--K", default="1,4,16,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--orders", default="0,1")
    ap.add_argument("--big-sources", type=int, default=1000)
    ap.add_argument("--exact-ties", type=int, default=1)
    ap.add_argument("--no-calsurfg", action="store_true")
    ap.add_argument("--trace-only", type=int, default=0, metavar="K")
    ap.add_argument("--json", default=None, help="also append the result lines to this file")
    args = ap.parse_args(argv)
    lib = load_library()
    lib.dsa_dropin_engine.restype = C.c_void_p
    lib.dsa_dropin_error.restype = C.c_char_p
    eng = C.c_void_p(lib.dsa_dropin_engine())
    assert eng.value, lib.dsa_dropin_error()
    assert lib.dsa_set_option(eng, b"exact_ties", C.c_double(args.exact_ties)) == 0
    systems = {}
    for s in args.systems.split(","):
        if s == "taipei":
            systems[s] = taipei.load()
        elif s == "big":
            systems[s] = synth.boundary_case(nx=20, ny=18, nz=6, nsrc=args.big_sources, nrcf=7, kRc=3, kRg=1, kLc=1, kLg=1, stations=True)
        else:
            ap.error("unknown system %r" % s)
    if args.trace_only:
        name, c = next(iter(systems.items()))
        for _ in range(3):
            taipei.call_forward_models(c, models_of(c, args.trace_only), 8, lib=lib)
        print("traced 3 calls of %d models on %s" % (args.trace_only, name))
        return 0
    for name, c in systems.items():
        print("# %s: %d x %d x %d, %d period slots, %d data" % (name, c["nx"], c["ny"], c["nz"], c["kmax"], c["ndata"]), flush=True)
        for order in (int(v) for v in args.orders.split(",")):
            for K in (int(v) for v in args.K.split(",")):
                r = measure(lib, name, c, K, order, args.reps, not args.no_calsurfg)
                line = json.dumps(r)
                print(line, flush=True)
                f = lambda d: "%.2f (%.2f .. %.2f)" % (d["median"], d["min"], d["max"])
                print("  %s order %d K %3d: batch %s ms, single %s ms%s; x%.2f vs single%s; %d units, %d bundled by %d; worst |dt| vs single %.3g s" %
                      (name, order, K, f(r["batch"]), f(r["single"]), ", calsurfg %s ms" % f(r["calsurfg"]) if "calsurfg" in r else "",
                       r["speedup_vs_single"], ", x%.2f vs calsurfg" % r["speedup_vs_calsurfg"] if "calsurfg" in r else "", r["units"], r["bundled_units"],
                       r["bundle_size"], r["worst_vs_single"]), flush=True)
                if args.json:
                    with open(args.json, "a") as fh:
                        fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
