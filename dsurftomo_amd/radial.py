"""Radial anisotropy in the direct 3-D inversion: Vsv and Vsh from Rayleigh and Love travel times.

    python -m dsurftomo_amd.radial <directory with DSurfTomo.in, the data file and MOD> [--model FILE] [--iterations N] [--weight W]
                                   [--weight-h W] [--damp D] [--aniso G] [--dvmax V] [--resolution] [--out DIR]

The approximation is section 23's: Rayleigh data touch only Vsv, Love data only Vsh, the cross sensitivities are neglected, and each
period's rays are traced through the map of the model of its wave type.  Both models start from the input's model (--model FILE: another
file of the directory in MOD's format).  The unknowns are two blocks on the grid of the isotropic inversion, dVsv then dVsh.

Each of --iterations N (default 3) iterations runs, all on one engine whose dispersion stage is radial: one dispersion run with kernels
per wave type present (depth.slot_plan; the Love runs read Vsh, the Rayleigh runs Vsv), the phase velocities at the group periods in
maps of their own behind the kmax maps of the periods (the reference traces a group period's rays through the phase map of that period),
maps_from_dispersion, kernels_from_dispersion_radial, the plan (radial_plan: the drop-in's units), solve_rows_radial_device,
iteration_system_radial_device -- the reference's 0/1 data weights, the Laplacian rows of the Vsv block weighted --weight W (default
the input file's weight0) and of the Vsh block --weight-h W (default --weight), and one tie row per cell of weight --aniso G (default
0.2) that penalises Vsh - Vsv of the stepped model -- dsa_lsmr with common.LSMR_ARGS and --damp D (default the input file's), and
update_radial (the step clipped to +- --dvmax V km/s, default 0.5, both models to the input file's [minvel, maxvel]).

<input>Radial.dat (depth.write_radial's columns: vsv, vsh, Voigt average, xi per node).  The log gives, per iteration, the weighted rms
residual per wave type before the step and the solver's itn / istop.  --resolution: the block PSFs of all 2 maxvp unknowns of the last
system (dsa_resolution_blocks with nblocks = 2, no solution leaves the device) in <input>RadialResolution.dat -- per block and cell
R_jj, the PSF lengths in the spike's own block, the co-located value and the energy share in the other block -- and the median and
worst Vsv -> Vsh and Vsh -> Vsv shares in the log.

radial_system and update_radial_twin restate the system and the update rule in NumPy for the tests.  Every precondition is checked
before the library is loaded.  There is no CPU path.
"""
import argparse
import os
import sys

import numpy as np

from . import depth, io
from .analyses.azimuthal import azimuthal_weights, laplacian_rows
from .analyses.common import LOCAL_SIZE, LSMR_ARGS, chunks, unknown_coords, vertices
from .analyses.resolution import resolution_chunk
from .anisotropy import block_psf_columns

BLOCKS = ("vsv", "vsh")
DEFAULT_ITERATIONS = 3
DEFAULT_ANISO = 0.2
DEFAULT_DVMAX = 0.5

_F64 = lambda *names: tuple((n, "%.17g", "f64") for n in names)
RADIAL_RESOLUTION_TABLE = (True, _F64("lon", "lat", "depth") + (("block", "%d", "int"),) + _F64("rjj", "psf_h_km", "psf_v_km", "colocated", "share"))


# ---- NumPy twins ----

def unknown_nodes(nx, ny, nz):
    """(maxvp,) the 0-based node, in a model (nz, ny, nx), of every unknown of a block in the order of the LSMR unknowns (i fastest, then j,
    then k): dsa_model_update's"""
    k, j, i = np.meshgrid(np.arange(nz - 1), np.arange(ny - 2), np.arange(nx - 2), indexing="ij")
    return ((k * ny + (j + 1)) * nx + (i + 1)).ravel()


def radial_system(nx, ny, nz, rw, row, col, res, datweight, weight0, weight_h, aniso, vsv, vsh):
    """The radial system from dsa_solve_rows_radial's rows (1-based, columns up to 2 maxvp, blocks Vsv | Vsh), the residuals res and the
    models vsv, vsh (nz, ny, nx): every entry scaled by its datum's weight, the right-hand side the weighted residuals, and below the dall
    data rows the Laplacian rows of block 0 weighted weight0 at rows dall + index, those of block 1 weighted weight_h at rows
    dall + maxvp + index, and maxvp tie rows at dall + 2 maxvp + index with the entries {index + 1, 0 - aniso}, {maxvp + index + 1, aniso}
    and the right-hand side 0 - aniso (vsh - vsv) at the unknown's node, all fp32.  Returns dict(m, n, rw, row, col, b), COO 1-based."""
    f = np.float32
    nvx, nvz, nl = nx - 2, ny - 2, nz - 1
    maxvp = nvx * nvz * nl
    rw = np.ascontiguousarray(rw, f); row = np.ascontiguousarray(row, np.int32); col = np.ascontiguousarray(col, np.int32)
    res = np.ascontiguousarray(res, f); datweight = np.ascontiguousarray(datweight, f)
    dall = res.size
    if not (rw.size == row.size == col.size) or datweight.size != dall:
        raise ValueError("radial_system: rw / row / col differ in length, or res and datweight do")
    if rw.size and (row.min() < 1 or row.max() > dall or col.min() < 1 or col.max() > 2 * maxvp):
        raise ValueError("radial_system: a row outside 1..%d or a column outside 1..%d" % (dall, 2 * maxvp))
    if not all(np.isfinite(v) and v >= 0 for v in (weight0, weight_h, aniso)):
        raise ValueError("radial_system: the weights and aniso must be finite and >= 0")
    g = f(aniso)
    index = np.arange(maxvp, dtype=np.int32)
    tie_rw = np.empty(2 * maxvp, f); tie_rw[0::2] = f(0.0) - g; tie_rw[1::2] = g
    tie_row = np.repeat(dall + 2 * maxvp + index + 1, 2).astype(np.int32)
    tie_col = np.empty(2 * maxvp, np.int32); tie_col[0::2] = index + 1; tie_col[1::2] = maxvp + index + 1
    parts = [(rw * datweight[row - 1], row, col), laplacian_rows(nvx, nvz, nl, weight0, dall, 0), laplacian_rows(nvx, nvz, nl, weight_h, dall + maxvp, maxvp),
             (tie_rw, tie_row, tie_col)]
    node = unknown_nodes(nx, ny, nz)
    d = (np.asarray(vsh, f).ravel()[node] - np.asarray(vsv, f).ravel()[node]).astype(f)
    b = np.zeros(dall + 3 * maxvp, f)
    b[:dall] = res * datweight
    b[dall + 2 * maxvp:] = f(0.0) - (g * d).astype(f)
    return dict(m=dall + 3 * maxvp, n=2 * maxvp, rw=np.concatenate([q[0] for q in parts]).astype(f),
                row=np.concatenate([q[1] for q in parts]).astype(np.int32), col=np.concatenate([q[2] for q in parts]).astype(np.int32), b=b)


def update_radial_twin(vsv, vsh, dv, dvmax, minvel, maxvel):
    """dsa_update_radial in NumPy: vsv, vsh (nz, ny, nx) fp32, dv (2 maxvp,) the Vsv block then the Vsh block; every unknown's node gets
    v + clip(dv, +-dvmax), then the clamp to [minvel, maxvel], in dsa_model_update's order of comparisons (a NaN stays a NaN); the ring and
    the bottom depth keep their values.  Returns the updated copies (vsv, vsh)."""
    f = np.float32
    out = []
    nz, ny, nx = np.asarray(vsv).shape
    d = np.array(dv, f, copy=True).reshape(2, nz - 1, ny - 2, nx - 2)
    dvmax, minvel, maxvel = f(dvmax), f(minvel), f(maxvel)
    for B, model in enumerate((vsv, vsh)):
        v = np.array(model, f, copy=True)
        with np.errstate(invalid="ignore"):
            s = np.where(d[B] >= dvmax, dvmax, d[B])
            s = np.where(s <= -dvmax, -dvmax, s)
            inner = (v[:-1, 1:-1, 1:-1] + s).astype(f)
            inner = np.where(inner < minvel, minvel, inner)
            inner = np.where(inner > maxvel, maxvel, inner)
        v[:-1, 1:-1, 1:-1] = inner
        out.append(v)
    return out[0], out[1]


# ---- the plan ----

def radial_plan(c):
    """The plan of the direct inversion from a loaded case, in the drop-in's unit order (period slot outer, the slot's sources in file
    order): a phase period's unit has its times and its rays (mode 3) on the slot's map; a group period has two units, the times (mode 1)
    on the slot's own map and the rays (mode 2) on the map of the phase velocity at that period, which lies behind the kmax maps of the
    slots (copies: [(wave type, periods, first map)], one dispersion run without kernels each).  sen_slot is the period slot.  Returns
    dict(map_index, scx, scz, nrec, rcx, rcz, mode, sen_slot, data_first, ndata, nmaps, copies, wave (ndata,): every datum's wave type)."""
    kmax = c["kmax"]
    kRc, kRg, kLc = len(c["tRc"]), len(c["tRg"]), len(c["tLc"])
    copies = []
    if kRg:
        copies.append((2, np.asarray(c["tRg"], np.float64), kmax))
    if len(c["tLg"]):
        copies.append((1, np.asarray(c["tLg"], np.float64), kmax + kRg))
    mp, sx, sz, nr, rx, rz, first, mode, slot_of, wave = [], [], [], [], [], [], [], [], [], []
    count = 0
    for slot in range(kmax):
        group = kRc <= slot < kRc + kRg or slot >= kRc + kRg + kLc
        love = slot >= kRc + kRg
        ray_map = slot if not group else (kmax + kRg + slot - (kRc + kRg + kLc) if love else kmax + slot - kRc)
        for s in range(int(c["nsrcsurf1"][slot])):
            n = int(c["nrc1"][s, slot])
            for m, md in (((slot, 3),) if not group else ((slot, 1), (ray_map, 2))):
                mp.append(m); mode.append(md); slot_of.append(slot); first.append(count); nr.append(n)
                sx.append(c["scxf"][s, slot]); sz.append(c["sczf"][s, slot])
                rx.append(c["rcxf"][:n, s, slot]); rz.append(c["rczf"][:n, s, slot])
            wave += [1 if love else 2] * n
            count += n
    cat = lambda parts: np.concatenate(parts).astype(np.float32) if parts else np.zeros(0, np.float32)
    return dict(map_index=np.array(mp, np.int32), scx=np.array(sx, np.float32), scz=np.array(sz, np.float32), nrec=np.array(nr, np.int32), rcx=cat(rx), rcz=cat(rz),
                mode=np.array(mode, np.int32), sen_slot=np.array(slot_of, np.int32), data_first=np.array(first, np.int32), ndata=count,
                nmaps=kmax + sum(t.size for _, t, _ in copies), copies=copies, wave=np.array(wave, np.int32))


def stage(eng, c, u):
    """what every iteration asks of the dispersion stage before the rows: the runs with kernels (depth.slot_plan), the phase velocities at
    the group periods (u's copies), the maps, the radial depth factors, the plan"""
    for wave, kind, t, first in depth.slot_plan(c):
        eng.dispersion_run(wave, kind, t, True, first, first)
    for wave, t, first in u["copies"]:
        eng.dispersion_run(wave, 0, t, False, 0, first)
    eng.maps_from_dispersion(c["goxd"], c["gozd"], c["dvxd"], c["dvzd"], 8)
    eng.kernels_from_dispersion_radial()
    eng.plan(u["map_index"], u["scx"], u["scz"], u["nrec"], u["rcx"], u["rcz"], mode=u["mode"], sen_slot=u["sen_slot"], data_first=u["data_first"])


def begin(eng, c, u, vsv, vsh):
    """a radial stage with room for the plan's maps on the models vsv, vsh (nz, ny, nx)"""
    eng.dispersion_begin_radial(vsv, vsh, c["depz"], c["minthk"], c["kmax"], u["nmaps"])


# ---- the loop ----

def check(iterations=None, weight=None, weight_h=None, damp=None, aniso=None, dvmax=None, c=None):
    """the driver's preconditions on its numbers and on the input c (None: not read yet), checked before the library is loaded (ValueError)"""
    if iterations is not None and iterations < 1:
        raise ValueError("--iterations must be at least 1, not %r" % (iterations,))
    for name, v in (("--weight", weight), ("--weight-h", weight_h), ("--damp", damp), ("--aniso", aniso)):
        if v is not None and not (np.isfinite(v) and v >= 0):
            raise ValueError("%s must be finite and >= 0, not %r" % (name, v))
    if dvmax is not None and not (np.isfinite(dvmax) and dvmax > 0):
        raise ValueError("--dvmax must be finite and > 0, not %r" % (dvmax,))
    if c is None:
        return
    if c["ifsyn"] == 1:
        raise ValueError("radial: a synthetic input (ifsyn = 1) has no observed data to invert")
    nr = len(c["tRc"]) + len(c["tRg"]); nl = len(c["tLc"]) + len(c["tLg"])
    if nr == 0 or nl == 0:
        raise ValueError("radial: Vsv and Vsh need Rayleigh and Love periods, the input lists %d and %d" % (nr, nl))


def wave_rms(res, datweight, wave):
    """{wave type: (data kept, weighted rms of the residuals)} for Rayleigh (2) and Love (1), and under None for all data"""
    r = np.asarray(res, np.float64) * np.asarray(datweight, np.float64)
    out = {}
    for key, sel in ((2, wave == 2), (1, wave == 1), (None, np.ones(r.size, bool))):
        sw = float(np.asarray(datweight, np.float64)[sel].sum())
        out[key] = (int(sw), float(np.sqrt((r[sel] ** 2).sum() / sw)) if sw > 0 else 0.0)
    return out


def iterate(eng, c, u, obst, iterations, weight, weight_h, damp, aniso, dvmax, log=print):
    """The loop on an engine whose stage is radial (begin): per iteration stage -> solve_rows_radial_device ->
    iteration_system_radial_device -> lsmr -> update_radial.  Returns dict(history: one dict per iteration {iteration, rms, rms_r, rms_l
    (weighted rms residuals before the step), kept, itn, istop, nar, dws}, system: the last iteration's, x: the last solution); the last
    system stays resident."""
    f = np.float32
    nx, ny, nz = c["nx"], c["ny"], c["nz"]
    obst = np.ascontiguousarray(obst, f)
    history, S, x = [], None, None
    for it in range(1, iterations + 1):
        stage(eng, c, u)
        dsyn, nnz = eng.solve_rows_radial_device()
        S = eng.iteration_system_radial_device(nx, ny, nz, obst, dsyn, float(c["threshold0"]), weight, weight_h, aniso)
        rms = wave_rms((obst - dsyn).astype(f), S["datweight"], u["wave"])
        sol = eng.lsmr(S["cbst"], damp, *LSMR_ARGS)
        x = sol["x"]
        eng.update_radial(x, dvmax, float(c["minvel"]), float(c["maxvel"]))
        log(" radial iteration %d: %d x %d, %d entries (%d from the rays), weighted rms residual %.5f s over %d of %d data (Rayleigh %.5f s over %d, Love %.5f s over %d), "
            "itn %d istop %d" % (it, S["m"], S["n"], S["nar"], nnz, rms[None][1], rms[None][0], obst.size, rms[2][1], rms[2][0], rms[1][1], rms[1][0], sol["itn"], sol["istop"]))
        history.append(dict(iteration=it, rms=rms[None][1], rms_r=rms[2][1], rms_l=rms[1][1], kept=rms[None][0], itn=sol["itn"], istop=sol["istop"], nar=S["nar"],
                            dws=S["dws"].tolist()))
    return dict(history=history, system=S, x=x)


# ---- the resolution ----

def leakage(psf):
    """From the measures of all spikes of the two-block system (2 maxvp, 2, 4): the energy share of a Vsv spike's image in the Vsh block
    and of a Vsh spike's image in the Vsv block, each as median and worst over the spikes whose image has any energy (0 where there is none).
    Returns dict(v_to_h_median, v_to_h_worst, h_to_v_median, h_to_v_worst, spikes_v, spikes_h)."""
    col = block_psf_columns(psf)
    if col["share"].shape[1] != 2:
        raise ValueError("leakage: two blocks (Vsv, Vsh), not %d" % col["share"].shape[1])
    live = col["share"].sum(axis=1) > 0
    a = col["share"][(col["block"] == 0) & live][:, 1]
    b = col["share"][(col["block"] == 1) & live][:, 0]
    stat = lambda v, fn: float(fn(v)) if v.size else 0.0
    return dict(v_to_h_median=stat(a, np.median), v_to_h_worst=stat(a, np.max), h_to_v_median=stat(b, np.median), h_to_v_worst=stat(b, np.max),
                spikes_v=int(a.size), spikes_h=int(b.size))


def write_radial_resolution(path, c, psf):
    """<input>RadialResolution.dat from the measures of all 2 maxvp spikes: one line per (block, cell) -- R_jj and the PSF lengths in the
    spike's own block, the value at the spike's cell and the energy share in the other block"""
    col = block_psf_columns(psf)
    cells = [(float(lon), float(lat), float(c["depz"][k])) for _, _, k, lon, lat in vertices(c)]
    nb = len(cells)
    rows = []
    for j in range(col["block"].size):
        lon, lat, dep = cells[j % nb]
        rows.append(dict(lon=lon, lat=lat, depth=dep, block=int(col["block"][j]), rjj=col["rjj"][j], psf_h_km=col["psf_h_km"][j], psf_v_km=col["psf_v_km"][j],
                         colocated=col["colocated"][j, 0], share=col["share"][j, col["others"][j, 0]]))
    io.write_table(path, RADIAL_RESOLUTION_TABLE, rows)


def read_radial_resolution(path):
    return io.read_table(path, RADIAL_RESOLUTION_TABLE)


def resolve(eng, c, m, damp, chunk=None):
    """The block PSF measures of every unknown of the resident radial system (m rows): spikes in chunks of `chunk` (default
    resolution_chunk(m, 2 maxvp, LOCAL_SIZE)), one dsa_resolution_blocks call each, x left on the device.  Returns dict(psf (2 maxvp, 2, 4),
    itn, istop, chunk, calls)."""
    n = 2 * c["nparpi"]
    chunk = int(chunk or resolution_chunk(m, n, LOCAL_SIZE))
    coords = np.ascontiguousarray(unknown_coords(c))
    psf = np.zeros((n, 2, 4)); istop = np.zeros(n, np.int32); itn = np.zeros(n, np.int32)
    for q in chunks(n, chunk):
        r = eng.lsmr_resolution_blocks(c["ndata"], damp, 2, (q.start, q.stop - q.start), coords, False, *LSMR_ARGS)
        psf[q] = r["psf"]; istop[q] = r["istop"]; itn[q] = r["itn"]
    return dict(psf=psf, itn=itn, istop=istop, chunk=chunk, calls=len(chunks(n, chunk)))


# ---- the driver ----

def run(directory, model=None, iterations=DEFAULT_ITERATIONS, weight=None, weight_h=None, damp=None, aniso=DEFAULT_ANISO, dvmax=DEFAULT_DVMAX, resolution=False,
        out_dir=".", log=print):
    """the driver behind main(); returns (iterate's result with vsv, vsh (nz, ny, nx) and, with resolution, resolution (resolve's) and
    leakage added, the path of Radial.dat)"""
    check(iterations, weight, weight_h, damp, aniso, dvmax)
    c = io.load(directory) if model is None else io.load(directory, model)
    check(c=c)
    u = radial_plan(c)
    if u["ndata"] != c["ndata"] or u["ndata"] < 4:
        raise ValueError("radial: the plan addresses %d data, the input holds %d" % (u["ndata"], c["ndata"]))
    from .engine import Engine
    weight = float(c["weight0"]) if weight is None else float(weight)
    weight_h = weight if weight_h is None else float(weight_h)
    damp = float(c["damp"]) if damp is None else float(damp)
    start = np.ascontiguousarray(np.asarray(c["vels"], np.float32).transpose(2, 1, 0))
    name = os.path.join(out_dir, "DSurfTomo.in")
    eng = Engine(0)
    try:
        begin(eng, c, u, start, start)
        out = iterate(eng, c, u, c["obst"], iterations, weight, weight_h, damp, aniso, dvmax, log)
        out["vsv"], out["vsh"] = eng.dispersion_get_model_radial()
        if resolution:
            p = resolve(eng, c, out["system"]["m"], damp)
            write_radial_resolution(name + "RadialResolution.dat", c, p["psf"])
            lk = leakage(p["psf"])
            out["resolution"], out["leakage"] = p, lk
            log(" radial resolution: %d spikes in %d calls of up to %d, itn min/max %d/%d" % (p["itn"].size, p["calls"], p["chunk"], int(p["itn"].min()), int(p["itn"].max())))
            log(" radial resolution: energy share Vsv -> Vsh median %.4f worst %.4f over %d spikes; Vsh -> Vsv median %.4f worst %.4f over %d spikes" %
                (lk["v_to_h_median"], lk["v_to_h_worst"], lk["spikes_v"], lk["h_to_v_median"], lk["h_to_v_worst"], lk["spikes_h"]))
    finally:
        eng.close()
    path = name + "Radial.dat"
    depth.write_radial(path, c, out["vsv"], out["vsh"])
    log(" radial: %d x %d x %d nodes of Vsv, Vsh, Voigt average and xi written to %s" % (c["nx"], c["ny"], c["nz"], path))
    return out, path


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("directory")
    ap.add_argument("--model", default=None, metavar="FILE", help="starting model of both Vsv and Vsh: a file of the directory in MOD's format (default: MOD)")
    ap.add_argument("--iterations", type=int, default=DEFAULT_ITERATIONS, metavar="N")
    ap.add_argument("--weight", type=float, default=None, metavar="W", help="smoothing weight of the Vsv block (default: the input file's weight0)")
    ap.add_argument("--weight-h", type=float, default=None, metavar="W", help="smoothing weight of the Vsh block (default: --weight)")
    ap.add_argument("--damp", type=float, default=None, metavar="D", help="damping of the solves (default: the input file's damp)")
    ap.add_argument("--aniso", type=float, default=DEFAULT_ANISO, metavar="G", help="weight of the tie rows on Vsh - Vsv of the stepped model (default %g)" % DEFAULT_ANISO)
    ap.add_argument("--dvmax", type=float, default=DEFAULT_DVMAX, metavar="V", help="largest change of a node per iteration in km/s (default %g)" % DEFAULT_DVMAX)
    ap.add_argument("--resolution", action="store_true", help="block PSFs of all 2 maxvp unknowns of the last system: <input>RadialResolution.dat and the leakage in the log")
    ap.add_argument("--out", default=".", metavar="DIR")
    return ap


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    try:
        check(a.iterations, a.weight, a.weight_h, a.damp, a.aniso, a.dvmax)
    except ValueError as exc:
        ap.error(str(exc))
    os.makedirs(a.out, exist_ok=True)
    run(a.directory, a.model, a.iterations, a.weight, a.weight_h, a.damp, a.aniso, a.dvmax, a.resolution, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
