"""Depth inversion of the period maps: per-column Vs(z) Gauss-Newton steps on the device.

    python -m dsurftomo_amd.depth <directory with DSurfTomo.in, the data file and MOD> [--maps FILE] [--iterations N] [--smooth L] [--damp D]
                                  [--dvmax V] [--min-dws X] [--out DIR]

The second step of the "two-step" method: the phase- and group-velocity maps of dsurftomo_amd.maps (<input>Maps.dat, --maps; read with
maps.read_maps) are inverted, column by column, for the Vs model the direct inversion is compared with.  The maps' period order -- Rayleigh
phase, Rayleigh group, Love phase, Love group -- is the slot order of the dispersion stage: map k and depth-kernel slot k belong to period k.

The model starts as the input's MOD.  Each of --iterations N (default 4) iterations runs, on one engine and without the model leaving the
device: one dispersion_run with kernels per wave type present, then columns_step -- per interior column the K map values against the
column's own curve, (G^T G + smooth^2 L^T L + damp^2 I) delta = G^T rho with the first-difference Laplacian L over depth (--smooth L, default
0.5; --damp D, default 0.1 -- both in units of the weighted sensitivities, which are dimensionless), the step clipped to +- --dvmax V km/s
(default 0.5) and the model to the input file's [minvel, maxvel].  A datum is used where its weight, its map value and the column's curve are
positive; the weights are 1, or 0 where the map's column DWS is below --min-dws X (default 0: every vertex of the maps counts).  The columns
do not see each other: the lateral smoothness of the result is that of the maps.

The log gives, per iteration, the data used, the flagged columns (1: the factorisation met a pivot <= 0; 2: no datum) and the rms
sqrt(sum chi2 / sum nused) before the step.  <input>Depth.dat (write_depth / read_depth): longitude, latitude, depth, Vs of every node, 17
significant digits.  <input>DepthFit.dat (write_fit / read_fit): per column longitude, latitude, the data used, the rms before the first and
before the last step, and the flag of the last step.

column_l, column_ltl and column_step_twin restate the regulariser and the step in NumPy for the tests (csrc/column_system.h is the arithmetic
the device runs).  Every precondition is checked before the library is loaded.  There is no CPU path.
"""
import argparse
import os
import sys

import numpy as np

from . import io, maps
from .analyses.common import _lonlat

DEFAULT_ITERATIONS = 4
DEFAULT_SMOOTH = 0.5
DEFAULT_DAMP = 0.1
DEFAULT_DVMAX = 0.5

_F64 = lambda *names: tuple((n, "%.17g", "f64") for n in names)
DEPTH_TABLE = (True, _F64("lon", "lat", "depth", "vs"))
FIT_TABLE = (True, _F64("lon", "lat") + (("nused", "%d", "int"),) + _F64("rms_first", "rms_last") + (("flag", "%d", "int"),))


# ---- NumPy twins ----

def column_l(M):
    """The regulariser of one column of M unknowns, row by row: for M >= 2 a top row (1, -1) on unknowns 0, 1 and a bottom row (-1, 1) on
    M-2, M-1; for M >= 3 the rows (-1, 2, -1) centred on 1 .. M-2.  M = 1: no rows.  Returns (rows, M) float64."""
    rows = []
    if M >= 2:
        r = np.zeros(M); r[0], r[1] = 1.0, -1.0; rows.append(r)
        r = np.zeros(M); r[M - 2], r[M - 1] = -1.0, 1.0; rows.append(r)
    for l in range(1, M - 1):
        r = np.zeros(M); r[l - 1], r[l], r[l + 1] = -1.0, 2.0, -1.0; rows.append(r)
    return np.array(rows).reshape(len(rows), M)


def column_ltl(M):
    """L^T L of column_l(M), (M, M) integers"""
    L = column_l(M)
    return np.rint(L.T @ L).astype(np.int64)


def column_step_twin(obs, wt, pv, S, vels, smooth, damp, dvmax, minvel, maxvel, solver="ldlt", n_override=None):
    """dsa_columns_step on one column in NumPy.  obs (K) fp32, wt (K) fp32 or None, pv (K) fp64, S (K, M) fp64 (k_sen_combine's d c / d Vs),
    vels (M or more) fp32: the column's values from the top; only the first M are stepped.  The sums run in column_system.h's order (k
    ascending from 0.0; the factorisation and the substitutions subtract term by term), so solver 'ldlt' follows the device operation by
    operation.  solver 'lstsq': the same step from numpy.linalg.lstsq on the stacked system [diag(a) S; smooth L; damp I] -- another
    algorithm, for the size of the rounding error.  n_override: an (M, M) matrix to factorise in place of the assembled N (tests).
    Returns dict(delta (M) fp64, dv (M) fp32, vels (the stepped copy), nused, chi2, flag)."""
    f = np.float32
    obs = np.asarray(obs, f); pv = np.asarray(pv, np.float64); S = np.asarray(S, np.float64)
    K, M = S.shape
    wt = np.ones(K, f) if wt is None else np.asarray(wt, f)
    vels = np.array(vels, f, copy=True)
    used = (wt > 0) & (obs > 0) & (pv > 0)
    a = wt.astype(np.float64)
    rho = np.where(used, a * (obs.astype(np.float64) - pv), 0.0)
    out = dict(delta=np.zeros(M), dv=np.zeros(M, f), vels=vels, nused=int(used.sum()), chi2=0.0, flag=0)
    chi2 = 0.0
    for k in np.flatnonzero(used):
        chi2 = chi2 + rho[k] * rho[k]
    out["chi2"] = float(chi2)
    if out["nused"] == 0:
        out["flag"] = 2
        return out
    G = np.zeros((K, M))
    G[used] = a[used, None] * S[used]                                  # (the S of an unused datum is never read: it may not be finite)
    lam2, mu2 = float(f(smooth)) * float(f(smooth)), float(f(damp)) * float(f(damp))
    if solver == "lstsq":
        A = np.vstack([G[used], float(f(smooth)) * column_l(M), float(f(damp)) * np.eye(M)])
        rhs = np.concatenate([rho[used], np.zeros(A.shape[0] - int(used.sum()))])
        delta = np.linalg.lstsq(A, rhs, rcond=None)[0]
    else:
        N = np.zeros((M, M)); b = np.zeros(M)
        for k in np.flatnonzero(used):
            N = N + np.outer(G[k], G[k])
            b = b + G[k] * rho[k]
        N = N + lam2 * column_ltl(M).astype(np.float64)
        N[np.diag_indices(M)] = N[np.diag_indices(M)] + mu2
        if n_override is not None:
            N = np.array(n_override, np.float64)
        Lm = np.zeros((M, M)); d = np.zeros(M)
        for j in range(M):
            v = Lm[j, :j] * d[:j]
            col = N[j:, j].copy()                                      # (entry 0: the pivot; the others: column j below it)
            for p in range(j):
                col = col - Lm[j:, p] * v[p]
            if not (np.isfinite(col[0]) and col[0] > 0):
                out["flag"] = 1
                return out
            d[j] = col[0]
            Lm[j + 1:, j] = col[1:] / d[j]
        x = b.copy()
        for p in range(M - 1):
            x[p + 1:] = x[p + 1:] - Lm[p + 1:, p] * x[p]
        x = x / d
        for i in range(M - 2, -1, -1):
            s = x[i]
            for p in range(i + 1, M):
                s = s - Lm[p, i] * x[p]
            x[i] = s
        delta = x
    s = delta.astype(f)
    dvmax, minvel, maxvel = f(dvmax), f(minvel), f(maxvel)
    with np.errstate(invalid="ignore"):
        s = np.where(s >= dvmax, dvmax, s)
        s = np.where(s <= -dvmax, -dvmax, s)
        v = (vels[:M] + s).astype(f)
        v = np.where(v < minvel, minvel, v)
        v = np.where(v > maxvel, maxvel, v)
    vels[:M] = v
    out.update(delta=delta, dv=s.astype(f))
    return out


# ---- the plan ----

def slot_plan(c):
    """[(wave type, velocity kind, periods, first slot)] of the wave types present, in the maps' period order Rc | Rg | Lc | Lg: one
    dispersion_run with kernels each, map_first = sen_slot = first slot"""
    out, first = [], 0
    for wave, kind, key in maps.WAVES:
        t = np.asarray(c[key], np.float64)
        if t.size:
            out.append((wave, kind, t, first))
            first += t.size
    return out


def maps_to_obs(rows, c):
    """The rows of <input>Maps.dat (maps.read_maps) as the step's observations: (obs, dws), both (nmaps, ny * nx) in get_maps' layout, fp32
    map values and fp64 DWS, 0 on the outer ring (which the step does not touch).  ValueError unless the file holds exactly the case's
    periods, in its order, with all interior vertices of each."""
    nx, ny = c["nx"], c["ny"]
    nvx, nvz = nx - 2, ny - 2
    layer = nvx * nvz
    per = maps.period_list(c)
    if len(rows) != len(per) * layer:
        raise ValueError("depth: the maps file holds %d lines, %d periods of %d x %d interior vertices need %d" % (len(rows), len(per), nvx, nvz, len(per) * layer))
    obs = np.zeros((len(per), ny, nx), np.float32); dws = np.zeros((len(per), ny, nx))
    for m, (wave, kind, t) in enumerate(per):
        block = rows[m * layer:(m + 1) * layer]
        if any((r["wave"], r["kind"], r["period"]) != (wave, kind, t) for r in block):
            raise ValueError("depth: map %d of the maps file is not wave %d kind %d period %g of the input" % (m, wave, kind, t))
        obs[m, 1:-1, 1:-1] = np.array([r["c0"] for r in block]).reshape(nvz, nvx)
        dws[m, 1:-1, 1:-1] = np.array([r["dws"] for r in block]).reshape(nvz, nvx)
    return obs.reshape(len(per), ny * nx), dws.reshape(len(per), ny * nx)


def dws_weights(dws, min_dws):
    """the step's weights: 1, or 0 where the map's column DWS is below min_dws"""
    return np.where(np.asarray(dws, np.float64) < float(min_dws), 0.0, 1.0).astype(np.float32)


# ---- the loop ----

def check(iterations=None, smooth=None, damp=None, dvmax=None, min_dws=None):
    """the driver's preconditions, checked before the library is loaded (ValueError)"""
    if iterations is not None and iterations < 1:
        raise ValueError("--iterations must be at least 1, not %r" % (iterations,))
    for name, v in (("--smooth", smooth), ("--min-dws", min_dws)):
        if v is not None and not (np.isfinite(v) and v >= 0):
            raise ValueError("%s must be finite and >= 0, not %r" % (name, v))
    for name, v in (("--damp", damp), ("--dvmax", dvmax)):
        if v is not None and not (np.isfinite(v) and v > 0):
            raise ValueError("%s must be finite and > 0, not %r" % (name, v))


def rms_of(chi2, nused):
    """sqrt(sum chi2 / sum nused), 0 without data"""
    n = int(np.sum(nused))
    return float(np.sqrt(np.sum(np.asarray(chi2, np.float64)) / n)) if n > 0 else 0.0


def iterate(eng, plan, obs, wt, iterations, smooth, damp, dvmax, minvel, maxvel, log=print):
    """The loop on an engine whose dispersion stage holds the starting model (dispersion_begin with as many maps as kernel slots): per
    iteration one dispersion_run with kernels per entry of plan (slot_plan), then columns_step.  Returns dict(history: one dict per iteration
    {iteration, nused, chi2, rms (before the step), flagged1, flagged2}, steps: columns_step's result per iteration)."""
    history, steps = [], []
    for it in range(1, iterations + 1):
        for wave, kind, t, first in plan:
            eng.dispersion_run(wave, kind, t, True, first, first)
        out = eng.columns_step(obs, wt, smooth, damp, dvmax, minvel, maxvel)
        h = dict(iteration=it, nused=int(out["nused"].sum()), chi2=float(out["chi2"].sum()), rms=rms_of(out["chi2"], out["nused"]),
                 flagged1=int((out["flag"] == 1).sum()), flagged2=int((out["flag"] == 2).sum()))
        log(" depth iteration %d: %d data used, rms %.6f km/s before the step, %d columns flagged (%d not positive definite, %d without data)" %
            (it, h["nused"], h["rms"], h["flagged1"] + h["flagged2"], h["flagged1"], h["flagged2"]))
        history.append(h)
        steps.append(out)
    return dict(history=history, steps=steps)


# ---- the files ----

def write_depth(path, c, vels):
    """<input>Depth.dat: vels (nz, ny, nx), every node: depth slowest, then j, then i"""
    nx, ny, nz = c["nx"], c["ny"], c["nz"]
    v = np.asarray(vels, np.float64).reshape(nz, ny, nx)
    rows = []
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                lon, lat = _lonlat(c, i - 1, j - 1)
                rows.append(dict(lon=float(lon), lat=float(lat), depth=float(c["depz"][k]), vs=v[k, j, i]))
    io.write_table(path, DEPTH_TABLE, rows)


def read_depth(path):
    return io.read_table(path, DEPTH_TABLE)


def write_fit(path, c, first, last):
    """<input>DepthFit.dat: first / last = columns_step's results of the first and the last iteration; one line per column, j then i"""
    nx, ny = c["nx"], c["ny"]
    col_rms = lambda s: np.sqrt(np.divide(s["chi2"], s["nused"], out=np.zeros(nx * ny), where=s["nused"] > 0))
    r0, r1 = col_rms(first), col_rms(last)
    rows = []
    for j in range(ny):
        for i in range(nx):
            lon, lat = _lonlat(c, i - 1, j - 1)
            q = j * nx + i
            rows.append(dict(lon=float(lon), lat=float(lat), nused=int(last["nused"][q]), rms_first=float(r0[q]), rms_last=float(r1[q]), flag=int(last["flag"][q])))
    io.write_table(path, FIT_TABLE, rows)


def read_fit(path):
    return io.read_table(path, FIT_TABLE)


def run(directory, maps_file=None, iterations=DEFAULT_ITERATIONS, smooth=DEFAULT_SMOOTH, damp=DEFAULT_DAMP, dvmax=DEFAULT_DVMAX, min_dws=0.0, out_dir=".",
        log=print):
    """the driver behind main(); returns (iterate's result with vels (nz, ny, nx) added, the paths of Depth.dat and DepthFit.dat)"""
    check(iterations, smooth, damp, dvmax, min_dws)
    c = io.load(directory)
    maps_file = os.path.join(out_dir, "DSurfTomo.inMaps.dat") if maps_file is None else maps_file
    obs, dws = maps_to_obs(maps.read_maps(maps_file), c)
    plan = slot_plan(c)
    kmax = c["kmax"]
    if not plan or kmax > 60:
        raise ValueError("depth: %d periods; the step takes 1 to 60" % kmax)
    wt = dws_weights(dws, min_dws) if min_dws > 0 else None
    from .engine import Engine
    eng = Engine(0)
    try:
        eng.dispersion_begin(np.ascontiguousarray(np.asarray(c["vels"], np.float32).transpose(2, 1, 0)), c["depz"], c["minthk"], kmax, kmax)
        out = iterate(eng, plan, obs, wt, iterations, smooth, damp, dvmax, float(c["minvel"]), float(c["maxvel"]), log)
        out["vels"] = eng.dispersion_get_model()
    finally:
        eng.close()
    path = os.path.join(out_dir, "DSurfTomo.inDepth.dat")
    fit = os.path.join(out_dir, "DSurfTomo.inDepthFit.dat")
    write_depth(path, c, out["vels"])
    write_fit(fit, c, out["steps"][0], out["steps"][-1])
    log(" depth: %d x %d x %d nodes written to %s, the fit of %d columns to %s" % (c["nx"], c["ny"], c["nz"], path, c["nx"] * c["ny"], fit))
    return out, path, fit


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("directory")
    ap.add_argument("--maps", default=None, metavar="FILE", help="the maps file of dsurftomo_amd.maps (default: DSurfTomo.inMaps.dat in --out)")
    ap.add_argument("--iterations", type=int, default=DEFAULT_ITERATIONS, metavar="N")
    ap.add_argument("--smooth", type=float, default=DEFAULT_SMOOTH, metavar="L", help="weight of the depth Laplacian (default %g)" % DEFAULT_SMOOTH)
    ap.add_argument("--damp", type=float, default=DEFAULT_DAMP, metavar="D", help="damping of a column's step, > 0 (default %g)" % DEFAULT_DAMP)
    ap.add_argument("--dvmax", type=float, default=DEFAULT_DVMAX, metavar="V", help="largest change of a node per iteration in km/s (default %g)" % DEFAULT_DVMAX)
    ap.add_argument("--min-dws", type=float, default=0.0, metavar="X", help="map vertices whose column DWS is below X get weight 0 (default 0: all count)")
    ap.add_argument("--out", default=".")
    return ap


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    try:
        check(a.iterations, a.smooth, a.damp, a.dvmax, a.min_dws)
    except ValueError as exc:
        ap.error(str(exc))
    os.makedirs(a.out, exist_ok=True)
    run(a.directory, a.maps, a.iterations, a.smooth, a.damp, a.dvmax, a.min_dws, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
