"""Period-by-period 2-D phase- and group-velocity maps on the bent rays, optionally with 2psi terms.

    python -m dsurftomo_amd.maps <directory with DSurfTomo.in, the data file and MOD> [--start model|mean] [--iterations N] [--weight W] [--damp D]
                                 [--dvmax V] [--azimuthal [--azimuthal-weight W]] [--resolution [--sigma-time S]] [--out DIR]

The first step of the "two-step" method, which the direct inversion is routinely compared with: the travel times of every period are
inverted for a 2-D velocity map of that period, on rays bent through that map.  There is one map per period of the input file, in the
reference's period order -- Rayleigh phase, Rayleigh group, Love phase, Love group -- and one unit per (period, source) with its travel
times AND its rays on that period's own map (period_plan: the unit and receiver order of the drop-in, dropin.hip: make_units).  A
group-velocity period is a 2-D map in its own right here, the usual practice; the drop-in's pairing of a group period's times with the
phase map's rays is not used.

--start model: the maps start as the dispersion of MOD through the device dispersion stage; --start mean (default): every period starts
from its mean of distance / time.  Each of --iterations N (default 3) iterations runs, all on one engine: dsa_solve_rows_maps with the rows
left on the device, dsa_iteration_system_maps_device (the reference's 0/1 data weights, one 2-D first-difference Laplacian row per unknown,
--weight W, default the input file's weight0), dsa_lsmr with common.LSMR_ARGS and --damp D (default the input file's), dsa_update_maps (the
step clipped to +- --dvmax V km/s, default 0.5, the maps to the input file's [minvel, maxvel]; the outer ring of vertices keeps its
values) and the plan again.  --azimuthal: three blocks of unknowns c0 | A1 | A2 per map, c(psi) = c0 + A1 cos 2psi + A2 sin 2psi, the A1
and A2 blocks smoothed with --azimuthal-weight W (default --weight); A1 and A2 are REPLACED each iteration by the solution's blocks, not
accumulated, and the rays are not traced through the anisotropic medium.

<input>Maps.dat (write_maps / read_maps): one line per (map, interior vertex) -- wave type (2 Rayleigh, 1 Love) and velocity kind (0 phase,
1 group), period, longitude, latitude, c0, the column's DWS of the last system; with --azimuthal also A1, A2, the strength
100 sqrt(A1^2 + A2^2) / c0 in per cent and the fast axis 0.5 atan2(A2, A1) in degrees from north.  The log gives, per iteration and per
map, the number of data and the weighted mean and rms residual before the step, and the solver's itn / istop.

--resolution: after the last iteration the rows are traced on the final maps, the system is built once more with
the run's weights and dsa_maps_resolution factors every map's normal matrix exactly.  <input>MapsResolution.dat (write_maps_resolution /
read_maps_resolution), per (map, interior vertex): wave, kind, period, longitude, latitude, R_jj, the point-spread lengths in x and y in km,
the own share of the point-spread function, sd_unit = sqrt(var), sd = sigma sd_unit in km/s, sigma -- --sigma-time S in seconds or, by
default, that map's weighted rms residual on the final maps -- and the map's flag; after --azimuthal also R_jj and sd of A1 and A2, their
covariance and the first-order sd of strength (per cent) and fast axis (degrees).  <input>MapsLeverage.dat: per datum its map, weight and
leverage.  Maps.dat and the loop are untouched.  depth --map-sigma reads the file as weights.

laplacian_rows_2d, map_system, update_maps_twin and map_resolution_twin restate the regulariser, the system and the update rule in NumPy for the tests.
Every precondition is checked before the library is loaded.  There is no CPU path.
"""
import argparse
import os
import sys

import numpy as np

from . import io
from .analyses.common import LSMR_ARGS, _lonlat

WAVES = ((2, 0, "tRc"), (2, 1, "tRg"), (1, 0, "tLc"), (1, 1, "tLg"))      # (wave type, velocity kind, the case's period list), the reference's order
DEFAULT_DVMAX = 0.5
DEFAULT_ITERATIONS = 3

_F64 = lambda *names: tuple((n, "%.17g", "f64") for n in names)
MAPS_TABLE = (True, (("wave", "%d", "int"), ("kind", "%d", "int")) + _F64("period", "lon", "lat", "c0", "dws"))
MAPS_AZI_TABLE = (True, MAPS_TABLE[1] + _F64("a1", "a2", "strength", "axis"))
RESOLUTION_TABLE = (True, MAPS_TABLE[1][:5] + _F64("rjj", "psf_x", "psf_y", "share", "sd_unit", "sd", "sigma") + (("flag", "%d", "int"),))
RESOLUTION_AZI_TABLE = (True, RESOLUTION_TABLE[1] + _F64("rjj_a1", "sd_a1", "rjj_a2", "sd_a2", "cov_a12", "sd_strength", "sd_axis"))
MAPS_LEVERAGE_TABLE = (True, (("datum", "%d", "int"), ("map", "%d", "int")) + _F64("weight", "leverage"))
EARTH_RADIUS_KM = 6371.0


# ---- NumPy twins ----

def laplacian_rows_2d(nvx, nvz, nplanes, weight, row0, col0=0):
    """The map system's regularisation rows: nplanes planes of nvx * nvz unknowns, i fastest, one row per unknown in column order; on its
    plane's edge one entry {here, 2 w}, inside {here, 4 w} then -w at -1, +1, -nvx, +nvx (main.f90:421-457 without the depth axis); planes
    never couple.  weight: one value, or one per plane; every stored value is the one rounded fp32 product c * w.  Rows row0 + 1 ..,
    columns col0 + 1 .. (1-based).  Returns (rw, row, col)."""
    f = np.float32
    ws = np.broadcast_to(np.asarray(weight, f), (nplanes,))
    rw, row, col = [], [], []
    r = row0
    for p in range(nplanes):
        w = f(ws[p])
        for j in range(1, nvz + 1):
            for i in range(1, nvx + 1):
                r += 1
                here = p * nvx * nvz + (j - 1) * nvx + i
                if i in (1, nvx) or j in (1, nvz):
                    rw.append(f(2.0) * w); row.append(r); col.append(col0 + here)
                else:
                    for q, nb in enumerate((here, here - 1, here + 1, here - nvx, here + nvx)):
                        rw.append(f(4.0) * w if q == 0 else f(-1.0) * w); row.append(r); col.append(col0 + nb)
    return np.array(rw, f), np.array(row, np.int32), np.array(col, np.int32)


def map_system(nx, ny, nmaps, nblocks, rw, row, col, res, datweight, weight0, weight_azi):
    """The map system from dsa_solve_rows_maps' rows (1-based, columns up to nblocks nmaps layer) and the residuals res: every entry scaled
    by its datum's weight, the right-hand side the weighted residuals, and below the dall data rows laplacian_rows_2d -- weight0 on the nmaps
    planes of block 0, weight_azi on the others.  Returns dict(m, n, rw, row, col, b), COO 1-based, fp32."""
    f = np.float32
    nvx, nvz = nx - 2, ny - 2
    n = nblocks * nmaps * nvx * nvz
    rw = np.ascontiguousarray(rw, f); row = np.ascontiguousarray(row, np.int32); col = np.ascontiguousarray(col, np.int32)
    res = np.ascontiguousarray(res, f); datweight = np.ascontiguousarray(datweight, f)
    dall = res.size
    if not (rw.size == row.size == col.size) or datweight.size != dall:
        raise ValueError("map_system: rw / row / col differ in length, or res and datweight do")
    if rw.size and (row.min() < 1 or row.max() > dall or col.min() < 1 or col.max() > n):
        raise ValueError("map_system: a row outside 1..%d or a column outside 1..%d" % (dall, n))
    w = np.where(np.arange(nblocks * nmaps) < nmaps, f(weight0), f(weight_azi)).astype(f)
    lap = laplacian_rows_2d(nvx, nvz, nblocks * nmaps, w, dall)
    b = np.zeros(dall + n, f)
    b[:dall] = res * datweight
    return dict(m=dall + n, n=n, rw=np.concatenate([rw * datweight[row - 1], lap[0]]).astype(f), row=np.concatenate([row, lap[1]]).astype(np.int32),
                col=np.concatenate([col, lap[2]]).astype(np.int32), b=b)


def update_maps_twin(velv, dv, dvmax, minvel, maxvel, nx, ny):
    """dsa_update_maps in NumPy: velv (nmaps, nx * ny) fp32 vertex maps in set_maps' layout (latitude index fastest), dv (nmaps, layer); interior
    vertices get v + clip(dv, +-dvmax), then the clamp to [minvel, maxvel], in dsa_model_update's order of comparisons (a NaN stays a NaN);
    the outer ring keeps its values.  Returns the updated copy."""
    f = np.float32
    v = np.array(velv, f, copy=True).reshape(-1, ny, nx)
    d = np.array(dv, f, copy=True).reshape(v.shape[0], ny - 2, nx - 2)
    dvmax, minvel, maxvel = f(dvmax), f(minvel), f(maxvel)
    with np.errstate(invalid="ignore"):
        d = np.where(d >= dvmax, dvmax, d)
        d = np.where(d <= -dvmax, -dvmax, d)
        inner = (v[:, 1:-1, 1:-1] + d).astype(f)
        inner = np.where(inner < minvel, minvel, inner)
        inner = np.where(inner > maxvel, maxvel, inner)
    v[:, 1:-1, 1:-1] = inner
    return v.reshape(v.shape[0], ny * nx)


def strength_percent(c0, a1, a2):
    """peak 2psi variation in per cent of c0: 100 sqrt(A1^2 + A2^2) / c0"""
    return 100.0 * np.hypot(np.asarray(a1, np.float64), np.asarray(a2, np.float64)) / np.asarray(c0, np.float64)


def fast_axis(a1, a2):
    """fast axis in degrees from north, in (-90, 90]: 0.5 atan2(A2, A1)"""
    return np.degrees(0.5 * np.arctan2(np.asarray(a2, np.float64), np.asarray(a1, np.float64)))


def map_resolution_twin(nx, ny, nmaps, nblocks, S, ndata, damp, route="normal"):
    """dsa_maps_resolution in NumPy: per map a dense fp64 numpy.linalg route with the library's definitions.  S: the
    system as map_system returns it (m, n, rw, row, col; 1-based COO).  route "normal": N = A_m^T A_m + damp^2 I by a Cholesky check and
    numpy.linalg.solve; route "pinv": the generalised inverse of [A_m; damp I] by numpy.linalg.pinv -- independent of the first, used only
    to size tolerances.  Returns dict(measures (9, nblocks, nmaps, layer), leverage (ndata), trace (nblocks, nmaps), nused, flag (nmaps),
    R: one (n_m, n_m) array per map, zeros where the map is flagged).  ValueError for a row with entries in two maps or a column stored
    twice in a row."""
    nvx, nvz = nx - 2, ny - 2
    layer = nvx * nvz
    nm, n, m = nblocks * layer, nblocks * nmaps * layer, int(S["m"])
    damp = float(np.float32(damp))                                     # (the library's argument is fp32)
    if int(S["n"]) != n:
        raise ValueError("map_resolution_twin: the system has %d unknowns, not %d" % (S["n"], n))
    row = np.asarray(S["row"], np.int64) - 1; col = np.asarray(S["col"], np.int64) - 1
    val = np.asarray(S["rw"], np.float32).astype(np.float64)
    if np.unique(row * n + col).size != row.size:
        raise ValueError("map_resolution_twin: a row stores one column twice")
    emap = (col // layer) % nmaps
    owner = np.full(m, -1, np.int64)
    lo = np.full(m, nmaps, np.int64); hi = np.full(m, -1, np.int64)
    np.minimum.at(lo, row, emap); np.maximum.at(hi, row, emap)
    if (lo[hi >= 0] != hi[hi >= 0]).any():
        raise ValueError("map_resolution_twin: row %d has entries in two maps" % (int(np.flatnonzero((hi >= 0) & (lo != hi))[0]) + 1))
    owner[hi >= 0] = hi[hi >= 0]
    A = np.zeros((m, n))
    A[row, col] = val
    used_row = (np.abs(A).sum(axis=1) > 0) & (np.arange(m) < ndata)
    out = dict(measures=np.zeros((9, nblocks, nmaps, layer)), leverage=np.zeros(ndata), trace=np.zeros((nblocks, nmaps)), nused=np.zeros(nmaps, np.int32),
               flag=np.zeros(nmaps, np.int32), R=[np.zeros((nm, nm)) for _ in range(nmaps)])
    ix, iy = np.arange(layer) % nvx, np.arange(layer) // nvx
    dx2 = (ix[:, None] - ix[None, :]).astype(np.float64) ** 2; dy2 = (iy[:, None] - iy[None, :]).astype(np.float64) ** 2
    for k in range(nmaps):
        cols = np.concatenate([np.arange((B * nmaps + k) * layer, (B * nmaps + k + 1) * layer) for B in range(nblocks)])
        rows = np.flatnonzero(owner == k)
        data = np.flatnonzero(used_row & (owner == k))
        out["nused"][k] = data.size
        if data.size == 0:
            out["flag"][k] = 2
            continue
        Am, G = A[np.ix_(rows, cols)], A[np.ix_(data, cols)]
        if route == "normal":
            N = Am.T @ Am + (float(damp) ** 2) * np.eye(nm)
            try:
                if not np.isfinite(N).all():
                    raise np.linalg.LinAlgError
                np.linalg.cholesky(N)
                T = np.linalg.solve(N, G.T).T
            except np.linalg.LinAlgError:
                out["flag"][k] = 1
                continue
        else:
            full = np.vstack([Am, float(damp) * np.eye(nm)])
            if np.linalg.matrix_rank(full) < nm:
                out["flag"][k] = 1
                continue
            T = np.linalg.pinv(full)[:, np.searchsorted(rows, data)].T
        R = T.T @ G                                                    # R_lq = sum_d t_dl g_dq
        out["R"][k] = R
        R2 = R * R
        meas = np.zeros((9, nm))
        meas[0] = R.diagonal(); meas[1] = (T * T).sum(axis=0); meas[5] = R2.sum(axis=0)
        for B in range(nblocks):
            own = slice(B * layer, (B + 1) * layer)
            blk = R2[own, own]
            meas[2, own] = blk.sum(axis=0); meas[3, own] = (blk * dx2).sum(axis=0); meas[4, own] = (blk * dy2).sum(axis=0)
            if nblocks > 1:
                q = np.arange(layer) + B * layer
                q1, q2 = np.arange(layer) + ((B + 1) % nblocks) * layer, np.arange(layer) + ((B + 2) % nblocks) * layer
                meas[6, own] = R[q1, q]; meas[7, own] = R[q2, q]; meas[8, own] = (T[:, q] * T[:, q1]).sum(axis=0)
        out["measures"][:, :, k, :] = meas.reshape(9, nblocks, layer)
        out["leverage"][data] = (G * T).sum(axis=1)
        out["trace"][:, k] = meas[0].reshape(nblocks, layer).sum(axis=1)
    return out


# ---- the plan ----

def period_list(c):
    """[(wave type, velocity kind, period in s)] of the maps, in the reference's period order Rc | Rg | Lc | Lg"""
    return [(wave, kind, float(t)) for wave, kind, key in WAVES for t in c[key]]


def period_plan(c):
    """The plan of the map inversion from a loaded case: one unit per (period slot, source) in the drop-in's unit order (period slot outer,
    the slot's sources in file order, a unit's receivers in file order), times and rays (mode 3) on the slot's own map.  Returns
    dict(map_index, scx, scz, nrec, rcx, rcz, mode, data_first, ndata, nmaps)."""
    kmax = c["kmax"]
    mp, sx, sz, nr, rx, rz, first = [], [], [], [], [], [], []
    count = 0
    for slot in range(kmax):
        for s in range(int(c["nsrcsurf1"][slot])):
            n = int(c["nrc1"][s, slot])
            mp.append(slot); sx.append(c["scxf"][s, slot]); sz.append(c["sczf"][s, slot]); nr.append(n); first.append(count)
            rx.append(c["rcxf"][:n, s, slot]); rz.append(c["rczf"][:n, s, slot])
            count += n
    cat = lambda parts: np.concatenate(parts).astype(np.float32) if parts else np.zeros(0, np.float32)
    return dict(map_index=np.array(mp, np.int32), scx=np.array(sx, np.float32), scz=np.array(sz, np.float32), nrec=np.array(nr, np.int32),
                rcx=cat(rx), rcz=cat(rz), mode=np.full(len(mp), 3, np.int32), data_first=np.array(first, np.int32), ndata=count, nmaps=kmax)


def plan_engine(eng, u):
    eng.plan(u["map_index"], u["scx"], u["scz"], u["nrec"], u["rcx"], u["rcz"], mode=u.get("mode"), data_first=u.get("data_first"))


def datum_maps(u):
    """the map of every datum of a plan, in data order"""
    out = np.zeros(int(u.get("ndata", np.sum(u["nrec"]))), np.int32)
    first = u.get("data_first")
    if first is None:
        first = np.concatenate([[0], np.cumsum(u["nrec"])[:-1]])
    for k, m in enumerate(u["map_index"]):
        out[first[k]:first[k] + u["nrec"][k]] = m
    return out


# ---- the loop ----

def check(iterations=None, weight=None, damp=None, dvmax=None, azimuthal=False, azimuthal_weight=None, start=None, resolution=False, sigma_time=None):
    """the driver's preconditions, checked before the library is loaded (ValueError)"""
    if sigma_time is not None and not resolution:
        raise ValueError("--sigma-time needs --resolution")
    if sigma_time is not None and not (np.isfinite(sigma_time) and sigma_time > 0):
        raise ValueError("--sigma-time must be finite and > 0, not %r" % (sigma_time,))
    if start is not None and start not in ("model", "mean"):
        raise ValueError("--start is model or mean, not %r" % (start,))
    if iterations is not None and iterations < 1:
        raise ValueError("--iterations must be at least 1, not %r" % (iterations,))
    for name, v in (("--weight", weight), ("--damp", damp), ("--azimuthal-weight", azimuthal_weight)):
        if v is not None and not (np.isfinite(v) and v >= 0):
            raise ValueError("%s must be finite and >= 0, not %r" % (name, v))
    if dvmax is not None and not (np.isfinite(dvmax) and dvmax > 0):
        raise ValueError("--dvmax must be finite and > 0, not %r" % (dvmax,))
    if azimuthal_weight is not None and not azimuthal:
        raise ValueError("--azimuthal-weight needs --azimuthal")


def residual_report(res, datweight, dmap, nmaps):
    """per map: (number of data, weighted mean, weighted rms) of the residuals res under the 0/1 weights (0, 0 where no datum is kept)"""
    out = []
    res = np.asarray(res, np.float64); w = np.asarray(datweight, np.float64)
    for m in range(nmaps):
        sel = dmap == m
        sw = w[sel].sum()
        r = res[sel] * w[sel]
        out.append((int(sel.sum()), float(r.sum() / sw) if sw > 0 else 0.0, float(np.sqrt((r * r).sum() / sw)) if sw > 0 else 0.0))
    return out


def iterate(eng, u, nx, ny, nmaps, obst, iterations, weight, damp, threshold0, dvmax, minvel, maxvel, azimuthal=False, weight_azi=None, log=print):
    """The loop of the map inversion on an engine whose maps are set and whose plan u is planned: per iteration solve_rows_maps_device ->
    iteration_system_maps_device -> lsmr -> update_maps -> plan again.  Returns dict(history: one dict per iteration {rms (weighted rms
    residual of all data before the step), per_map, itn, istop, nar, dws}, norm (the last system's column DWS), a1, a2 ((nmaps, layer) of
    the last solution, or None), x (the last solution))."""
    f = np.float32
    layer = (nx - 2) * (ny - 2)
    nblocks = 3 if azimuthal else 1
    obst = np.ascontiguousarray(obst, f)
    dmap = datum_maps(u)
    history, S, x = [], None, None
    for it in range(1, iterations + 1):
        dsyn, nnz = eng.solve_rows_maps_device(azimuthal)
        S = eng.iteration_system_maps_device(nx, ny, nmaps, nblocks, obst, dsyn, threshold0, weight, weight if weight_azi is None else weight_azi)
        res = (obst - dsyn).astype(f)
        per_map = residual_report(res, S["datweight"], dmap, nmaps)
        sw = float(S["datweight"].sum())
        rms = float(np.sqrt(((res.astype(np.float64) * S["datweight"]) ** 2).sum() / sw)) if sw > 0 else 0.0
        sol = eng.lsmr(S["cbst"], damp, *LSMR_ARGS)
        x = sol["x"]
        eng.update_maps(x[:nmaps * layer], dvmax, minvel, maxvel, nmaps, nx, ny)
        plan_engine(eng, u)
        log(" maps iteration %d: %d x %d, %d entries (%d from the rays), weighted rms residual %.5f s over %d of %d data, itn %d istop %d" %
            (it, S["m"], S["n"], S["nar"], nnz, rms, int(sw), obst.size, sol["itn"], sol["istop"]))
        for m, (nd, mean, r) in enumerate(per_map):
            log(" maps iteration %d map %3d: %6d data, weighted mean %9.5f s rms %9.5f s" % (it, m, nd, mean, r))
        history.append(dict(iteration=it, rms=rms, per_map=per_map, itn=sol["itn"], istop=sol["istop"], nar=S["nar"], dws=S["dws"].tolist()))
    a1 = a2 = None
    if azimuthal:
        a1 = x[nmaps * layer:2 * nmaps * layer].reshape(nmaps, layer).copy()
        a2 = x[2 * nmaps * layer:].reshape(nmaps, layer).copy()
    return dict(history=history, norm=S["norm"], a1=a1, a2=a2, x=x)


def start_maps(eng, c, u, start):
    """the starting maps on the engine: the dispersion of the model (--start model) or, per period, the mean of distance / time"""
    nx, ny, nz, kmax = c["nx"], c["ny"], c["nz"], c["kmax"]
    if start == "model":
        eng.dispersion_begin(np.ascontiguousarray(np.asarray(c["vels"], np.float32).transpose(2, 1, 0)), c["depz"], c["minthk"], kmax, kmax)
        first = 0
        for wave, kind, key in WAVES:
            if len(c[key]):
                eng.dispersion_run(wave, kind, c[key], False, 0, first)
                first += len(c[key])
        eng.maps_from_dispersion(c["goxd"], c["gozd"], c["dvxd"], c["dvzd"], 8)
        return
    dmap = datum_maps(u)
    vel = np.asarray(c["dist"], np.float64) / np.asarray(c["obst"], np.float64)
    pv = np.zeros((kmax, nx * ny))
    for m in range(kmax):
        if not (dmap == m).any():
            raise ValueError("--start mean: period %d has no data" % m)
        pv[m] = vel[dmap == m].mean()
    eng.set_maps(nx, ny, c["goxd"], c["gozd"], c["dvxd"], c["dvzd"], pv, dicing=8)


# ---- the resolution of the maps ----

def strength_variance(c0, a1, a2, v1, v2, c12):
    """first-order variance of the strength s = 100 sqrt(A1^2 + A2^2) / c0 in per cent^2 from the variances v1, v2 of A1, A2 and their covariance
    c12 (c0 taken as known): (100 / c0)^2 (A1^2 v1 + A2^2 v2 + 2 A1 A2 c12) / (A1^2 + A2^2); 0 where A1 = A2 = 0; clamped at 0"""
    c0, a1, a2, v1, v2, c12 = (np.asarray(x, np.float64) for x in (c0, a1, a2, v1, v2, c12))
    r2 = a1 * a1 + a2 * a2
    num = (100.0 / c0) ** 2 * (a1 * a1 * v1 + a2 * a2 * v2 + 2.0 * a1 * a2 * c12)
    return np.maximum(np.divide(num, r2, out=np.zeros(np.broadcast(num, r2).shape), where=r2 > 0), 0.0)


def axis_variance(a1, a2, v1, v2, c12):
    """first-order variance of the fast axis phi = atan2(A2, A1) / 2 in rad^2: (A2^2 v1 + A1^2 v2 - 2 A1 A2 c12) / (4 (A1^2 + A2^2)^2); 0 where
    A1 = A2 = 0; clamped at 0"""
    a1, a2, v1, v2, c12 = (np.asarray(x, np.float64) for x in (a1, a2, v1, v2, c12))
    r2 = a1 * a1 + a2 * a2
    num = 0.25 * (a2 * a2 * v1 + a1 * a1 * v2 - 2.0 * a1 * a2 * c12)
    return np.maximum(np.divide(num, r2 * r2, out=np.zeros(np.broadcast(num, r2).shape), where=r2 > 0), 0.0)


def _ratio_root(num, den):
    num = np.asarray(num, np.float64); den = np.asarray(den, np.float64)
    return np.sqrt(np.maximum(np.divide(num, den, out=np.zeros(num.shape), where=den > 0), 0.0))


def resolution_columns(c, res, sigma_m, velv=None, a1=None, a2=None):
    """The columns of MapsResolution.dat from maps_resolution's result res (measures (9, nblocks, nmaps, layer), flag) and the data's
    standard deviation per map sigma_m (nmaps, s): a dict of (nmaps, layer) arrays -- rjj, psf_x, psf_y (km: sqrt(m3 / m2) and sqrt(m4 / m2)
    times the vertex spacing; x is the fast vertex index, which runs along latitude), share = m2 / m5, sd_unit = sqrt(var), sd = sigma_m
    sd_unit (km/s), sigma, flag; with three blocks (velv (nmaps, nx * ny), a1, a2 (nmaps, layer) given) also rjj and sd of A1 and A2, their
    covariance sigma_m^2 times measure 8 of the A1 unknown, and the sd of strength (per cent) and fast axis (degrees)."""
    nx, ny = c["nx"], c["ny"]
    nvx, nvz = nx - 2, ny - 2
    m = np.asarray(res["measures"], np.float64)
    nblocks, nmaps = m.shape[1], m.shape[2]
    sig = np.asarray(sigma_m, np.float64).reshape(nmaps, 1)
    lat = np.array([[float(_lonlat(c, i, j)[1]) for i in range(nvx)] for j in range(nvz)]).reshape(-1)
    dx_km = EARTH_RADIUS_KM * np.radians(float(c["dvxd"]))
    dy_km = EARTH_RADIUS_KM * np.radians(float(c["dvzd"])) * np.cos(np.radians(lat))
    out = dict(rjj=m[0, 0], psf_x=_ratio_root(m[3, 0], m[2, 0]) * dx_km, psf_y=_ratio_root(m[4, 0], m[2, 0]) * dy_km[None, :],
               share=np.divide(m[2, 0], m[5, 0], out=np.zeros(m[2, 0].shape), where=m[5, 0] > 0), sd_unit=np.sqrt(np.maximum(m[1, 0], 0.0)),
               sigma=np.broadcast_to(sig, m[0, 0].shape).copy(), flag=np.broadcast_to(np.asarray(res["flag"]).reshape(nmaps, 1), m[0, 0].shape).copy())
    out["sd"] = sig * out["sd_unit"]
    if nblocks == 3:
        v1, v2, c12 = sig ** 2 * m[1, 1], sig ** 2 * m[1, 2], sig ** 2 * m[8, 1]
        c0 = np.asarray(velv, np.float64).reshape(nmaps, ny, nx)[:, 1:-1, 1:-1].reshape(nmaps, -1)
        out.update(rjj_a1=m[0, 1], sd_a1=np.sqrt(np.maximum(v1, 0.0)), rjj_a2=m[0, 2], sd_a2=np.sqrt(np.maximum(v2, 0.0)), cov_a12=c12,
                   sd_strength=np.sqrt(strength_variance(c0, a1, a2, v1, v2, c12)), sd_axis=np.degrees(np.sqrt(axis_variance(a1, a2, v1, v2, c12))))
    return out


def write_maps_resolution(path, c, cols):
    """<input>MapsResolution.dat: resolution_columns' arrays, one line per (map, interior vertex) in Maps.dat's order"""
    nvx, nvz = c["nx"] - 2, c["ny"] - 2
    azi = "rjj_a1" in cols
    table = RESOLUTION_AZI_TABLE if azi else RESOLUTION_TABLE
    names = [n for n, _, _ in table[1][5:]]
    rows = []
    for m, (wave, kind, t) in enumerate(period_list(c)):
        for j in range(nvz):
            for i in range(nvx):
                lon, lat = _lonlat(c, i, j)
                r = dict(wave=wave, kind=kind, period=t, lon=float(lon), lat=float(lat))
                r.update({n: (int if n == "flag" else float)(cols[n][m, j * nvx + i]) for n in names})
                rows.append(r)
    io.write_table(path, table, rows)


def read_maps_resolution(path, azimuthal=False):
    """the rows write_maps_resolution wrote; the header line says whether the file carries the 2psi columns.  ValueError naming the file when
    it is not such a file (no sd and flag columns), or, with azimuthal, when it lacks the sd of A1 and A2."""
    return io.read_table(path, RESOLUTION_AZI_TABLE if "rjj_a1" in resolution_header(path, azimuthal) else RESOLUTION_TABLE)


def resolution_header(path, azimuthal=False):
    """the column names of a MapsResolution.dat; ValueError naming the file when it cannot be read, when it has no sd and flag columns or,
    with azimuthal, no sd of A1 and A2"""
    try:
        with open(path) as fh:
            head = fh.readline().split()
    except OSError as exc:
        raise ValueError("%s cannot be read (%s)" % (path, exc.strerror))
    if not {"sd", "flag", "rjj"} <= set(head):
        raise ValueError("%s has no sd / flag columns: it is not a MapsResolution.dat of maps --resolution" % path)
    if azimuthal and not {"sd_a1", "sd_a2"} <= set(head):
        raise ValueError("%s has no sd_a1 / sd_a2 columns; write it with maps --azimuthal --resolution" % path)
    return head


def write_maps_leverage(path, dmap, datweight, leverage):
    """<input>MapsLeverage.dat: one line per datum in data order -- its map, its weight and its leverage"""
    io.write_table(path, MAPS_LEVERAGE_TABLE, [dict(datum=d, map=int(dmap[d]), weight=float(datweight[d]), leverage=float(leverage[d])) for d in range(len(leverage))])


def read_maps_leverage(path):
    return io.read_table(path, MAPS_LEVERAGE_TABLE)


def resolve(eng, c, u, obst, weight, damp, threshold0, out, sigma_time=None, azimuthal=False, weight_azi=None, out_dir=".", log=print):
    """--resolution on an engine that holds the final maps and their plan: the rows traced on them, the system once more with the run's
    weights, maps_resolution, the two files and the log.  out: iterate's result with velv.  sigma per map: sigma_time (s), or that map's
    weighted rms residual on the final maps.  Returns dict(resolution, sigma_m, columns, resolution_path, leverage_path)."""
    f = np.float32
    nx, ny, nmaps = c["nx"], c["ny"], u["nmaps"]
    nblocks = 3 if azimuthal else 1
    obst = np.ascontiguousarray(obst, f)
    dsyn, _ = eng.solve_rows_maps_device(azimuthal)
    S = eng.iteration_system_maps_device(nx, ny, nmaps, nblocks, obst, dsyn, threshold0, weight, weight if weight_azi is None else weight_azi)
    res = eng.maps_resolution(nx, ny, nmaps, nblocks, obst.size, damp)
    dmap = datum_maps(u)
    per_map = residual_report((obst - dsyn).astype(f), S["datweight"], dmap, nmaps)
    sigma_m = np.full(nmaps, float(sigma_time)) if sigma_time is not None else np.array([r for _, _, r in per_map])
    cols = resolution_columns(c, res, sigma_m, out["velv"], out.get("a1"), out.get("a2"))
    rpath = os.path.join(out_dir, "DSurfTomo.inMapsResolution.dat")
    lpath = os.path.join(out_dir, "DSurfTomo.inMapsLeverage.dat")
    write_maps_resolution(rpath, c, cols)
    write_maps_leverage(lpath, dmap, S["datweight"], res["leverage"])
    log(" maps resolution: sigma per map is %s" % ("--sigma-time %.6f s" % sigma_time if sigma_time is not None else "its weighted rms residual on the final maps"))
    for m in range(nmaps):
        lev = res["leverage"][dmap == m]
        log(" maps resolution map %3d: flag %d, %5d data used, trace %s of %d unknowns per block, median R_jj %.4f, sigma %.5f s, median sd %.5f km/s, largest leverage %.4f" %
            (m, int(res["flag"][m]), int(res["nused"][m]), " ".join("%.3f" % t for t in res["trace"][:, m]), (nx - 2) * (ny - 2), float(np.median(cols["rjj"][m])),
             float(sigma_m[m]), float(np.median(cols["sd"][m])), float(lev.max()) if lev.size else 0.0))
    log(" maps resolution: written to %s, the leverages of %d data to %s" % (rpath, obst.size, lpath))
    return dict(resolution=res, sigma_m=sigma_m, columns=cols, resolution_path=rpath, leverage_path=lpath)


# ---- the file ----

def write_maps(path, c, velv, norm, a1=None, a2=None):
    """<input>Maps.dat: velv (nmaps, nx * ny) vertex maps, norm (>= nmaps * layer) the column DWS of the c0 block, a1 / a2 (nmaps, layer) or None"""
    nx, ny = c["nx"], c["ny"]
    nvx, nvz = nx - 2, ny - 2
    per = period_list(c)
    v = np.asarray(velv, np.float64).reshape(len(per), ny, nx)
    dws = np.asarray(norm, np.float64)[:len(per) * nvx * nvz].reshape(len(per), nvz, nvx)
    azi = a1 is not None and a2 is not None
    if azi:
        a1 = np.asarray(a1, np.float64).reshape(len(per), nvz, nvx); a2 = np.asarray(a2, np.float64).reshape(len(per), nvz, nvx)
    rows = []
    for m, (wave, kind, t) in enumerate(per):
        for j in range(nvz):
            for i in range(nvx):
                lon, lat = _lonlat(c, i, j)
                r = dict(wave=wave, kind=kind, period=t, lon=float(lon), lat=float(lat), c0=v[m, j + 1, i + 1], dws=dws[m, j, i])
                if azi:
                    r.update(a1=a1[m, j, i], a2=a2[m, j, i], strength=float(strength_percent(r["c0"], a1[m, j, i], a2[m, j, i])),
                             axis=float(fast_axis(a1[m, j, i], a2[m, j, i])))
                rows.append(r)
    io.write_table(path, MAPS_AZI_TABLE if azi else MAPS_TABLE, rows)


def read_maps(path):
    """the rows write_maps wrote, as a list of dicts; the header line says whether the file carries the 2psi columns"""
    with open(path) as fh:
        head = fh.readline().split()
    return io.read_table(path, MAPS_AZI_TABLE if "a1" in head else MAPS_TABLE)


def run(directory, start="mean", iterations=DEFAULT_ITERATIONS, weight=None, damp=None, dvmax=DEFAULT_DVMAX, azimuthal=False, azimuthal_weight=None,
        out_dir=".", log=print, resolution=False, sigma_time=None):
    """the driver behind main(); returns (iterate's result with velv (nmaps, nx * ny) added, the path of Maps.dat).  With resolution the
    result also holds resolve's entries; Maps.dat and the loop are what they are without it."""
    check(iterations, weight, damp, dvmax, azimuthal, azimuthal_weight, start, resolution, sigma_time)
    c = io.load(directory)
    if c["ifsyn"] == 1:
        raise ValueError("maps: a synthetic input (ifsyn = 1) has no observed data to invert")
    u = period_plan(c)
    if u["ndata"] != c["ndata"] or u["ndata"] < 4:
        raise ValueError("maps: the plan addresses %d data, the input holds %d" % (u["ndata"], c["ndata"]))
    from .engine import Engine
    weight = float(c["weight0"]) if weight is None else float(weight)
    damp = float(c["damp"]) if damp is None else float(damp)
    eng = Engine(0)
    try:
        start_maps(eng, c, u, start)
        plan_engine(eng, u)
        out = iterate(eng, u, c["nx"], c["ny"], u["nmaps"], c["obst"], iterations, weight, damp, float(c["threshold0"]), dvmax, float(c["minvel"]), float(c["maxvel"]),
                      azimuthal, azimuthal_weight, log)
        out["velv"] = eng.get_maps(u["nmaps"], c["nx"], c["ny"])
        if resolution:
            out.update(resolve(eng, c, u, c["obst"], weight, damp, float(c["threshold0"]), out, sigma_time, azimuthal, azimuthal_weight, out_dir, log))
    finally:
        eng.close()
    path = os.path.join(out_dir, "DSurfTomo.inMaps.dat")
    write_maps(path, c, out["velv"], out["norm"], out["a1"], out["a2"])
    log(" maps: %d maps of %d x %d interior vertices written to %s" % (u["nmaps"], c["nx"] - 2, c["ny"] - 2, path))
    return out, path


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("directory")
    ap.add_argument("--start", choices=("model", "mean"), default="mean", help="starting maps: the dispersion of MOD, or each period's mean of distance / time (default)")
    ap.add_argument("--iterations", type=int, default=DEFAULT_ITERATIONS, metavar="N")
    ap.add_argument("--weight", type=float, default=None, metavar="W", help="smoothing weight (default: the input file's weight0)")
    ap.add_argument("--damp", type=float, default=None, metavar="D", help="damping of the solves (default: the input file's damp)")
    ap.add_argument("--dvmax", type=float, default=DEFAULT_DVMAX, metavar="V", help="largest change of a vertex per iteration in km/s (default %g)" % DEFAULT_DVMAX)
    ap.add_argument("--azimuthal", action="store_true", help="three blocks per map: c0, A1 (cos 2psi), A2 (sin 2psi)")
    ap.add_argument("--azimuthal-weight", type=float, default=None, metavar="W", help="smoothing weight of the A1 and A2 blocks (default: --weight)")
    ap.add_argument("--resolution", action="store_true", help="after the last iteration write the exact resolution and standard deviation of every map value (MapsResolution.dat, MapsLeverage.dat)")
    ap.add_argument("--sigma-time", type=float, default=None, metavar="S", help="with --resolution: standard deviation of the travel times in s (default: each map's weighted rms residual)")
    ap.add_argument("--out", default=".")
    return ap


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    try:
        check(a.iterations, a.weight, a.damp, a.dvmax, a.azimuthal, a.azimuthal_weight, a.start, a.resolution, a.sigma_time)
    except ValueError as exc:
        ap.error(str(exc))
    os.makedirs(a.out, exist_ok=True)
    run(a.directory, a.start, a.iterations, a.weight, a.damp, a.dvmax, a.azimuthal, a.azimuthal_weight, a.out, resolution=a.resolution, sigma_time=a.sigma_time)
    return 0


if __name__ == "__main__":
    sys.exit(main())
