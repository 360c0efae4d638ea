#!/usr/bin/env python3
"""dsa_lsmr_batch against R sequential dsa_lsmr calls (default placement: products on the device, ordered sums on the host).

    python tools/lsmr_batch_rate.py [--systems taipei,multiblock[,headline]] [--R 1,8,64,256] [--legs bootstrap,resolution[,tradeoff][,voronoi][,crossval]] [--cells 300,1000]
                                    [--cv 13x5,39x5]

Per system and R: bootstrap row scales (dsurftomo_amd.invert.bootstrap_row_scales), one warm-up of each path, then the batch
once and R sequential solves of the explicitly scaled systems (the scaled matrices are loaded outside the timed region; each
solve is timed alone).  Prints one line per (system, R) and checks realisation 0 of the batch against its sequential solve bit
for bit.  Resolution leg (resolution_leg): every unknown's PSF by dsa_lsmr_resolution against sequential dsa_lsmr spike solves.
Trade-off leg (tradeoff_leg, --legs tradeoff): K = each --R (weight, damp) members by dsa_lsmr_tradeoff against sequential rebuilds of
the system with each member's weight + dsa_lsmr, a sample of --seq-max members timed and scaled to K.
Voronoi leg (voronoi_leg, --legs voronoi): K = each --R members of each --cells cells by dsa_lsmr_voronoi against, per member, the numpy
relabelling of the data rows + dsa_spmv_load + dsa_lsmr, a sample of at most 16 members timed and scaled to K.
Cross-validation leg (crossval_leg, --legs crossval): each --cv NCOMBOxNFOLDS by one dsa_lsmr_crossval call against, per member, the masked and
re-weighted system rebuilt in numpy + dsa_spmv_load + dsa_lsmr, a sample of at most 16 members timed and scaled to K = NCOMBO (NFOLDS + 1).  headline: the 1025^2 boundary of tests/tools/headline_boundary.py with 8 receivers per source (minutes of set-up).
The systems are the product's own (dsa_calsurfg + dsa_iteration_system, or tests/synth_matrix.py): nothing here loads oracle/."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctypes as C           # noqa: E402
import _libs as L            # noqa: E402
import inversion as inv      # noqa: E402  (inv.same only: a bitwise comparison)
import synth                 # noqa: E402
from dsurftomo_amd import invert                       # noqa: E402
from dsurftomo_amd import io as taipei                 # noqa: E402
from dsurftomo_amd.engine import Engine, load_library  # noqa: E402


def product_system(c, fwd, obst, threshold0, weight0):
    """the system of main.f90:361-466 by the library's dsa_iteration_system: dict(m, n, nar, iw = [nar, rows, cols], rw, b)"""
    lib = invert.bind(load_library())
    nx, ny, nz, dall = c["nx"], c["ny"], c["nz"], c["ndata"]
    maxvp = (nx - 2) * (ny - 2) * (nz - 1)
    cap = fwd["nar"] + 7 * maxvp
    rw = np.zeros(cap, np.float32); rw[:fwd["nar"]] = fwd["rw"]
    col = np.zeros(cap, np.int32); col[:fwd["nar"]] = fwd["col"]
    iw = np.zeros(2 * cap + 1, np.int32); iw[1:fwd["nar"] + 1] = fwd["iw"]
    cbst = np.zeros(dall + maxvp, np.float32); datweight = np.zeros(dall, np.float32)
    norm = np.zeros(maxvp, np.float32); dws = np.zeros(2, np.float32)
    m, nar = C.c_int(0), C.c_longlong(0)
    p = L.ptr
    rc = lib.dsa_iteration_system(nx, ny, nz, dall, fwd["nar"], cap, p(rw), p(iw), p(col), p(np.ascontiguousarray(obst, np.float32)),
                                  p(np.ascontiguousarray(fwd["dsurf"], np.float32)), threshold0, weight0, p(cbst), p(datweight), p(norm),
                                  C.byref(m), C.byref(nar), p(dws))
    assert rc == 0, rc
    n = nar.value
    return dict(m=m.value, n=maxvp, nar=n, iw=iw[:2 * n + 1].copy(), rw=rw[:n].copy(), b=cbst[:m.value].copy())


def taipei_system():
    c = taipei.load()
    fwd = L.call_boundary(load_library().dsa_calsurfg, c)
    return product_system(c, fwd, c["obst"], 3.0, 4.0), c["ndata"], 1.0, 400, invert.unknown_coords(c)


def grid_coords(ni, nj, nk):
    """latitude, longitude, depth of a regular grid of unknowns, i fastest (the unknowns' order), 0.05 degrees and 2 km apart"""
    k, j, i = np.meshgrid(np.arange(nk), np.arange(nj), np.arange(ni), indexing="ij")
    return np.stack([25.0 - 0.05 * i.ravel(), 121.0 + 0.05 * j.ravel(), 2.0 * k.ravel()], axis=1).astype(np.float64)


def multiblock_system():
    import synth_matrix as SM
    M = SM.system(31522, 47, 47, 31, seed=11)
    m, n, nar = M["m"], M["n"], M["rw"].size
    b = np.zeros(m, np.float32)
    b[:31522] = (SM.mix(np.arange(31522), 12) - 0.5).astype(np.float32)
    S = dict(m=m, n=n, nar=nar, iw=np.concatenate([[nar], M["row"], M["col"]]).astype(np.int32), rw=M["rw"], b=b)
    return S, 31522, 0.7, 35, grid_coords(47, 47, 31)


def headline_system():
    c = synth.boundary_case(nx=131, ny=131, nz=9, kRc=16, kRg=0, kLc=0, kLg=0, nsrc=1000, nrcf=8, dvd=0.01, ragged=False, stations=True)
    c["tRc"] = np.linspace(2.0, 17.0, 16)
    fwd = L.call_boundary(load_library().dsa_calsurfg, c)
    r = synth.LCG(77)
    obst = (fwd["dsurf"] * (1.0 + 0.04 * (r.uniform(c["ndata"]) - 0.5))).astype(np.float32)
    return product_system(c, fwd, obst, 3.0, 2.0), c["ndata"], 1.0, 20, invert.unknown_coords(c)


EST = ("normA", "condA", "normr", "normAr", "normx")


def resolution_leg(name, e, S, ndata, damp, itnlim, coords, seq_max):
    """every unknown's PSF by dsa_lsmr_resolution in chunks of invert.resolution_chunk (x left on the device, PSF measures back)
    against sequential dsa_lsmr spike solves: seq_max spikes spread over the unknowns, each timed alone (its right-hand side formed
    outside the timing), scaled to all n; spike 0 of the sample checked bit for bit"""
    n = S["n"]
    chunk = invert.resolution_chunk(S["m"], n, 10)
    load(e, S)
    e.lsmr_resolution(ndata, damp, spikes=(0, min(chunk, n)), coords=coords, want_x=False, itnlim=2)      # warm-up: the largest chunk
    t0 = time.perf_counter()
    itn, calls = [], 0
    for first in range(0, n, chunk):
        D = e.lsmr_resolution(ndata, damp, spikes=(first, min(chunk, n - first)), coords=coords, want_x=False, itnlim=itnlim)
        itn.append(D["itn"])
        calls += 1
    t_res = time.perf_counter() - t0
    itn = np.concatenate(itn)
    js = np.unique(np.linspace(0, n - 1, min(seq_max, n)).astype(int))
    e.lsmr(S["b"], damp, itnlim=2)
    t_seq, itn_seq, first_seq = 0.0, 0, None
    for j in js:
        sp = np.zeros(n, np.float32)
        sp[j] = 1.0
        b = e.spmv(1, sp, np.zeros(S["m"], np.float32))
        b[ndata:] = 0.0
        t0 = time.perf_counter()
        got = e.lsmr(b, damp, itnlim=itnlim)
        t_seq += time.perf_counter() - t0
        itn_seq += got["itn"]
        if first_seq is None:
            first_seq = got
    one = e.lsmr_resolution(ndata, damp, spikes=(int(js[0]), 1), itnlim=itnlim)
    b0 = dict(x=one["x"][0], istop=int(one["istop"][0]), itn=int(one["itn"][0]), **{k: one[k][0] for k in EST})
    t_seq_all = t_seq * n / len(js)
    print("%s resolution: %d PSFs in %d calls of up to %d: %9.1f ms (itn max %d, total %d) | %d of %d sequential dsa_lsmr %9.1f ms "
          "(%.2f ms per solve, %.1f itn) | speed-up %.1fx | spike %d identical: %s" %
          (name, n, calls, chunk, 1e3 * t_res, int(itn.max()), int(itn.sum()), len(js), n, 1e3 * t_seq_all, 1e3 * t_seq / len(js),
           itn_seq / len(js), t_seq_all / t_res, int(js[0]), inv.same(b0, first_seq) == []), flush=True)


WEIGHT0 = dict(taipei=4.0, multiblock=2.0, headline=2.0)      # the weight the systems' regularisation rows are built with


def tradeoff_leg(name, e, S, ndata, weight0, damp, itnlim, Ks, seq_max):
    """K (weight, damp) members by one dsa_lsmr_tradeoff call (x and the measures back) against what a rerun per member does after its
    forward call: the system rebuilt with the member's weight (its regularisation entries fl(c * weight), loaded: both orderings built)
    and dsa_lsmr with the member's damp.  Up to seq_max members spread over the grid are run that way, each step timed alone, and
    scaled to K; member 0 is checked bit for bit.  Weights: weight0 / 16 .. 16 weight0 (geometric), damps: damp x {0.25, 0.5, 1, 2}
    (K divisible by 4) or damp alone."""
    rows = S["iw"][1:S["nar"] + 1] - 1
    reg = rows >= ndata
    coef = np.rint(S["rw"][reg] / np.float32(weight0)).astype(np.float32)
    assert np.array_equal(coef * np.float32(weight0), S["rw"][reg])
    for K in Ks:
        damps = [0.25 * damp, 0.5 * damp, damp, 2.0 * damp] if K % 4 == 0 else [damp]
        w, d = invert.tradeoff_grid(np.geomspace(weight0 / 16.0, weight0 * 16.0, K // len(damps)), damps)
        load(e, S)
        e.lsmr_tradeoff(S["b"], ndata, weight0, w, d, itnlim=2)            # warm-up: contiguous and coefficient copies, allocations, code
        t0 = time.perf_counter()
        T = e.lsmr_tradeoff(S["b"], ndata, weight0, w, d, itnlim=itnlim)
        t_sweep = time.perf_counter() - t0
        ks = np.unique(np.linspace(0, K - 1, min(seq_max, K)).astype(int))
        e.lsmr(S["b"], damp, itnlim=2)
        t_load, t_seq, itn_seq, first = 0.0, 0.0, 0, None
        for k in ks:
            rw = S["rw"].copy()
            t0 = time.perf_counter()
            rw[reg] = coef * w[k]
            load(e, S, rw)
            t_load += time.perf_counter() - t0
            t0 = time.perf_counter()
            got = e.lsmr(S["b"], float(d[k]), itnlim=itnlim)
            t_seq += time.perf_counter() - t0
            itn_seq += got["itn"]
            if first is None:
                first = got
        k0 = int(ks[0])
        b0 = dict(x=T["x"][k0], istop=int(T["istop"][k0]), itn=int(T["itn"][k0]), **{q: T[q][k0] for q in EST})
        scale = K / len(ks)
        print("%s tradeoff K %4d: sweep %9.1f ms (itn max %d, total %d) | %d of %d sequential: rebuild + load %9.1f ms, dsa_lsmr %9.1f ms "
              "(%.2f + %.2f ms per member, %.1f itn) | speed-up %.1fx over the solves, %.1fx with the rebuilds | member %d identical: %s" %
              (name, K, 1e3 * t_sweep, int(T["itn"].max()), int(T["itn"].sum()), len(ks), K, 1e3 * t_load * scale, 1e3 * t_seq * scale,
               1e3 * t_load / len(ks), 1e3 * t_seq / len(ks), itn_seq / len(ks), t_seq * scale / t_sweep, (t_seq + t_load) * scale / t_sweep, k0,
               inv.same(b0, first) == []), flush=True)


def voronoi_leg(name, e, S, ndata, damp, itnlim, coords, Ks, cells, seq_max):
    """K members of ncells cells by one dsa_lsmr_voronoi call (the statistics back, z and the cells left on the device) against what K
    separate solves do: per member the data rows relabelled in numpy (the cells from the call itself, outside the timing), loaded
    (dsa_spmv_load: both orderings built) and solved by dsa_lsmr.  At most min(seq_max, 16) members spread over the ensemble are run
    that way, each step timed alone, and scaled to K; the first of them is checked bit for bit.  Every call ends in a device
    synchronisation, so the host clock around it is the call's time."""
    nar = S["nar"]
    rows, cols = S["iw"][1:nar + 1], S["iw"][nar + 1:]
    keep = np.flatnonzero(rows <= ndata)
    keep = keep[np.argsort(rows[keep], kind="stable")]
    r_d, c_d, v_d = rows[keep], cols[keep] - 1, np.ascontiguousarray(S["rw"][keep])
    b_d = np.ascontiguousarray(S["b"][:ndata])
    xyz = invert.coords_xyz(coords, 1.0)
    n = S["n"]
    for ncells in cells:
        for K in Ks:
            seeds = invert.voronoi_seeds(n, ncells, K, seed=1)
            load(e, S)
            e.lsmr_voronoi(S["b"], ndata, ncells, xyz, seeds, damp, want_z=False, want_cell=False, itnlim=2)      # warm-up: copies, allocations, code
            runs = []
            for _ in range(3):                                                # (the spread of the ensemble's own time: three runs, the median reported)
                t0 = time.perf_counter()
                V = e.lsmr_voronoi(S["b"], ndata, ncells, xyz, seeds, damp, want_z=False, want_cell=False, itnlim=itnlim)
                runs.append(time.perf_counter() - t0)
            t_ens = sorted(runs)[1]
            ks = np.unique(np.linspace(0, K - 1, min(seq_max, 16, K)).astype(int))
            W = e.lsmr_voronoi(S["b"], ndata, ncells, xyz, seeds[ks], damp, itnlim=itnlim)                         # the sample's cells and solutions
            t_rel, t_load, t_seq, itn_seq, same = 0.0, 0.0, 0, 0, None
            for q, k in enumerate(ks):
                t0 = time.perf_counter()
                cc = (W["cell"][q][c_d] + 1).astype(np.int32)
                t_rel += time.perf_counter() - t0
                t0 = time.perf_counter()
                e.spmv_load(ndata, ncells, v_d, r_d, cc)
                t_load += time.perf_counter() - t0
                t0 = time.perf_counter()
                got = e.lsmr(b_d, damp, itnlim=itnlim)
                t_seq += time.perf_counter() - t0
                itn_seq += got["itn"]
                if same is None:
                    same = inv.same(dict(x=W["z"][q], istop=int(W["istop"][q]), itn=int(W["itn"][q]), **{f: W[f][q] for f in EST}), got) == []
            scale = K / len(ks)
            t_all = (t_rel + t_load + t_seq) * scale
            print("%s voronoi K %4d cells %5d: ensemble %9.1f ms (three runs %.1f .. %.1f; itn max %d, total %d) | %d of %d sequential: relabel %9.1f ms, load %9.1f ms, dsa_lsmr "
                  "%9.1f ms (%.2f + %.2f + %.2f ms per member, %.1f itn) | speed-up %.1fx over the solves, %.1fx with relabel + load | member %d "
                  "identical: %s" %
                  (name, K, ncells, 1e3 * t_ens, 1e3 * min(runs), 1e3 * max(runs), int(V["itn"].max()), int(V["itn"].sum()), len(ks), K, 1e3 * t_rel * scale, 1e3 * t_load * scale,
                   1e3 * t_seq * scale, 1e3 * t_rel / len(ks), 1e3 * t_load / len(ks), 1e3 * t_seq / len(ks), itn_seq / len(ks), t_seq * scale / t_ens,
                   t_all / t_ens, int(ks[0]), same), flush=True)


def crossval_leg(name, e, S, ndata, weight0, damp, itnlim, shapes, seq_max):
    """ncombo combos x (nfolds hold-outs + the full data) by one dsa_lsmr_crossval call (the measures and residuals back, x left on the
    device) against what a rerun per member does after its forward call: the system rebuilt with the combo's weight and the fold's data
    rows zeroed (values and right-hand side), loaded (both orderings built) and solved by dsa_lsmr with the combo's damp.  At most
    min(seq_max, 16) members spread over the grid are run that way, each step timed alone, and scaled to K; the first is checked bit for
    bit.  Weights: weight0 / 16 .. 16 weight0 (geometric); damps: damp x {0.5, 1, 2} where ncombo is divisible by 3, else damp alone;
    folds by datum, seed 1."""
    rows = S["iw"][1:S["nar"] + 1] - 1
    reg = rows >= ndata
    coef = np.rint(S["rw"][reg] / np.float32(weight0)).astype(np.float32)
    assert np.array_equal(coef * np.float32(weight0), S["rw"][reg])
    for ncombo, nfolds in shapes:
        damps = [0.5 * damp, damp, 2.0 * damp] if ncombo % 3 == 0 else [damp]
        w, d = invert.tradeoff_grid(np.geomspace(weight0 / 16.0, weight0 * 16.0, ncombo // len(damps)), damps)
        fold = invert.crossval_folds(dict(ndata=ndata), nfolds, "datum", 1)
        S1, K = nfolds + 1, ncombo * (nfolds + 1)
        load(e, S)
        e.lsmr_crossval(S["b"], ndata, weight0, w, d, fold, nfolds, want_x=False, itnlim=2)      # warm-up: copies, allocations, code
        runs = []
        for _ in range(3):                                                # (three runs, the median reported)
            t0 = time.perf_counter()
            T = e.lsmr_crossval(S["b"], ndata, weight0, w, d, fold, nfolds, want_x=False, itnlim=itnlim)
            runs.append(time.perf_counter() - t0)
        t_cv = sorted(runs)[1]
        ks = np.unique(np.linspace(0, K - 1, min(seq_max, 16, K)).astype(int))
        W = e.lsmr_crossval(S["b"], ndata, weight0, w, d, fold, nfolds, itnlim=itnlim)
        e.lsmr(S["b"], damp, itnlim=2)
        t_load, t_seq, itn_seq, same = 0.0, 0.0, 0, None
        for k in ks:
            q, f = divmod(int(k), S1)
            t0 = time.perf_counter()
            s = np.ones(S["m"], np.float32)
            s[:ndata][fold == f] = 0.0
            rw = S["rw"].copy()
            rw[reg] = coef * w[q]
            rw *= s[rows]
            bk = S["b"] * s
            load(e, S, rw)
            t_load += time.perf_counter() - t0
            t0 = time.perf_counter()
            got = e.lsmr(bk, float(d[q]), itnlim=itnlim)
            t_seq += time.perf_counter() - t0
            itn_seq += got["itn"]
            if same is None:
                same = inv.same(dict(x=W["x"][k], istop=int(W["istop"][k]), itn=int(W["itn"][k]), **{g: W[g][k] for g in EST}), got) == []
        scale = K / len(ks)
        print("%s crossval %d combos x %d folds (K %4d): %9.1f ms (three runs %.1f .. %.1f; itn max %d, total %d) | %d of %d sequential: rebuild + load "
              "%9.1f ms, dsa_lsmr %9.1f ms (%.2f + %.2f ms per member, %.1f itn) | speed-up %.1fx over the solves, %.1fx with the rebuilds | member %d "
              "identical: %s" %
              (name, ncombo, nfolds, K, 1e3 * t_cv, 1e3 * min(runs), 1e3 * max(runs), int(T["itn"].max()), int(T["itn"].sum()), len(ks), K,
               1e3 * t_load * scale, 1e3 * t_seq * scale, 1e3 * t_load / len(ks), 1e3 * t_seq / len(ks), itn_seq / len(ks), t_seq * scale / t_cv,
               (t_seq + t_load) * scale / t_cv, int(ks[0]), same), flush=True)


def load(e, S, rw=None):
    nar = S["nar"]
    e.spmv_load(S["m"], S["n"], S["rw"] if rw is None else rw, S["iw"][1:nar + 1], S["iw"][nar + 1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--systems", default="taipei,multiblock")
    ap.add_argument("--R", default="1,8,64,256")
    ap.add_argument("--seq-max", type=int, default=64, help="sequential solves actually run per R (the rest extrapolated from their mean)")
    ap.add_argument("--legs", default="bootstrap,resolution", help="bootstrap (dsa_lsmr_batch), resolution (dsa_lsmr_resolution) tradeoff (dsa_lsmr_tradeoff), voronoi (dsa_lsmr_voronoi) and / or crossval (dsa_lsmr_crossval)")
    ap.add_argument("--cv", default="13x5,39x5", help="NCOMBOxNFOLDS shapes of the crossval leg")
    ap.add_argument("--cells", default="300,1000", help="cells per member of the voronoi leg")
    args = ap.parse_args()
    Rs = [int(v) for v in args.R.split(",")]
    legs = args.legs.split(",")
    make = dict(taipei=taipei_system, multiblock=multiblock_system, headline=headline_system)
    for name in args.systems.split(","):
        t0 = time.perf_counter()
        S, ndata, damp, itnlim, coords = make[name]()
        print("%s: m %d n %d nar %d (set-up %.1f s), damp %g, itnlim %d" % (name, S["m"], S["n"], S["nar"], time.perf_counter() - t0, damp, itnlim), flush=True)
        rows = S["iw"][1:S["nar"] + 1] - 1
        e = Engine(0)
        try:
            if "resolution" in legs:
                resolution_leg(name, e, S, ndata, damp, itnlim, coords, args.seq_max)
            if "tradeoff" in legs:
                tradeoff_leg(name, e, S, ndata, WEIGHT0[name], damp, itnlim, Rs, args.seq_max)
            if "voronoi" in legs:
                voronoi_leg(name, e, S, ndata, damp, itnlim, coords, Rs, [int(v) for v in args.cells.split(",")], args.seq_max)
            if "crossval" in legs:
                crossval_leg(name, e, S, ndata, WEIGHT0[name], damp, itnlim, [tuple(int(v) for v in t.split("x")) for t in args.cv.split(",")], args.seq_max)
            if "bootstrap" not in legs:
                continue
            scales = invert.bootstrap_row_scales(ndata, S["m"], max(Rs), seed=1)
            load(e, S)
            e.lsmr_batch(S["b"], scales[:2], damp, itnlim=2)              # warm-up: contiguous copies, allocations, code
            e.lsmr(S["b"], damp, itnlim=2)
            for R in Rs:
                load(e, S)
                e.lsmr_batch(S["b"], scales[:R], damp, itnlim=2)
                t0 = time.perf_counter()
                B = e.lsmr_batch(S["b"], scales[:R], damp, itnlim=itnlim)
                t_batch = time.perf_counter() - t0
                nseq = min(R, args.seq_max)
                t_seq, itn_seq, first = 0.0, 0, None
                for r in range(nseq):
                    s = scales[r]
                    load(e, S, (S["rw"] * s[rows]).astype(np.float32))
                    bs = (S["b"] * s).astype(np.float32)
                    t0 = time.perf_counter()
                    got = e.lsmr(bs, damp, itnlim=itnlim)
                    t_seq += time.perf_counter() - t0
                    itn_seq += got["itn"]
                    if r == 0:
                        first = got
                t_seq_all = t_seq * R / nseq
                b0 = dict(x=B["x"][0], istop=int(B["istop"][0]), itn=int(B["itn"][0]), **{k: B[k][0] for k in ("normA", "condA", "normr", "normAr", "normx")})
                print("%s R %4d: batch %9.1f ms (itn max %d, total %d) | %s%d sequential dsa_lsmr %9.1f ms (%.2f ms per solve, %.1f itn) | "
                      "speed-up %.1fx | realisation 0 identical: %s" %
                      (name, R, 1e3 * t_batch, int(B["itn"].max()), int(B["itn"].sum()), "" if nseq == R else "%d of " % nseq, R, 1e3 * t_seq_all,
                       1e3 * t_seq / nseq, itn_seq / nseq, t_seq_all / t_batch, inv.same(b0, first) == []), flush=True)
        finally:
            e.close()


if __name__ == "__main__":
    main()
