"""Period-by-period 2-D phase- and group-velocity maps on the bent rays, optionally with 2psi terms.

    python -m dsurftomo_amd.maps <directory with DSurfTomo.in, the data file and MOD> [--start model|mean] [--iterations N] [--weight W] [--damp D]
                                 [--dvmax V] [--azimuthal [--azimuthal-weight W]] [--out DIR]

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

laplacian_rows_2d, map_system and update_maps_twin restate the regulariser, the system and the update rule in NumPy for the tests.
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

def check(iterations=None, weight=None, damp=None, dvmax=None, azimuthal=False, azimuthal_weight=None, start=None):
    """the driver's preconditions, checked before the library is loaded (ValueError)"""
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
        out_dir=".", log=print):
    """the driver behind main(); returns (iterate's result with velv (nmaps, nx * ny) added, the path of Maps.dat)"""
    check(iterations, weight, damp, dvmax, azimuthal, azimuthal_weight, start)
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
    ap.add_argument("--out", default=".")
    return ap


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    try:
        check(a.iterations, a.weight, a.damp, a.dvmax, a.azimuthal, a.azimuthal_weight, a.start)
    except ValueError as exc:
        ap.error(str(exc))
    os.makedirs(a.out, exist_ok=True)
    run(a.directory, a.start, a.iterations, a.weight, a.damp, a.dvmax, a.azimuthal, a.azimuthal_weight, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
