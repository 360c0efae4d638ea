"""Resolution tests of the joint Vs / 2psi azimuthal step, with the whole step on the device.

    python -m dsurftomo_amd.anisotropy <directory with DSurfTomo.in, the data file and MOD> [--model FILE] [--maxiter N] [--out DIR]
                                       [--weight W] [--damp D] [--resolution] [--checkerboard NX,NY,NZ[,G] ...]

The model is --model FILE (a file of the directory in MOD's format, as for forward.py) or, without it, the model invert.run leaves after
--maxiter iterations (its files are written to --out as usual).  On that model comes ONE joint step for Vs | gc | gs, nothing of it applied:
dsa_calsurfg_azimuthal with null arrays leaves the azimuthal rows on the drop-in engine, dsa_iteration_system_azimuthal_device builds the
joint system where they are (the reference's 0/1 data weights, the Laplacian rows of the three blocks with weight0 on Vs and --weight W,
default weight0, on gc and gs), dsa_lsmr solves it with common.LSMR_ARGS and --damp D (default the input file's).  <input>Azim.dat is
written by analyses.azimuthal.write_azimuthal: the bytes `invert --azimuthal --azimuthal-weight W --azimuthal-damp D` writes for the same
model, because the two routes build the same system bit for bit.

--resolution: the unit spike of every one of the 3 maxvp unknowns through dsa_resolution_blocks (nblocks = 3, the solutions left on the
device), in chunks of resolution_chunk().  <input>AzimResolution.dat (AZIM_RESOLUTION_TABLE) has one line per (block, cell), blocks
0 = Vs, 1 = gc, 2 = gs, cells in the vertex order of the model files: longitude, latitude, depth, block, R_jj, the horizontal and vertical
PSF length of the spike's own block in km (sqrt(sum x^2 d^2 / sum x^2), 0 where sum x^2 = 0), and for each of the two other blocks, in
ascending order, the co-located value x[B nb + cell] and the energy share sum_B x^2 / sum_all x^2: how much of the spike's image leaks into
that block.  The log gives the median and the worst Vs -> (gc, gs) and (gc, gs) -> Vs shares.

--checkerboard NX,NY,NZ[,G] (may be repeated; G: the gc / gs amplitude, default 0.04 = 2 % peak to peak): three test models per board in
one dsa_lsmr_resolution call -- Vs only (analyses.resolution.checkerboard, +-0.1 km/s), gc = +-G only (fast axes 0 / 90 degrees), gs =
+-G only (45 / 135 degrees).  <input>AzimChecker.dat.kNN.vs / .gc / .gs (AZIM_CHECKER_TABLE): longitude, latitude, depth, the three input
blocks and the three recovered blocks.  The log and the history carry recovery_metrics of the driven block and, for the two other blocks,
rms(recovered) / rms(input of the driven block); the Vs block is in km/s, gc and gs are dimensionless, so a ratio across the two kinds
carries that unit (km/s per unit of g, or its inverse).

Every precondition is checked before the library is loaded.  There is no CPU path: without a usable GPU this fails with the engine's error text.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

from . import io
from .analyses.azimuthal import azimuthal_strength, write_azimuthal
from .analyses.common import LOCAL_SIZE, LSMR_ARGS, _p, _solve_stats, _solve_text, arg_type, call_solver, chunks, forward_rows, lsmr, unknown_coords, vertices
from .analyses.resolution import checkerboard, recovery_metrics, resolution_chunk

BLOCKS = ("vs", "gc", "gs")
DEFAULT_G = 0.04

_F64 = lambda *names: tuple((n, "%.17g", "f64") for n in names)
AZIM_RESOLUTION_TABLE = (True, _F64("lon", "lat", "depth") + (("block", "%d", "int"),) +
                         _F64("rjj", "psf_h_km", "psf_v_km", "colocated_a", "share_a", "colocated_b", "share_b"))
AZIM_CHECKER_TABLE = (True, _F64("lon", "lat", "depth", "in_vs", "in_gc", "in_gs", "out_vs", "out_gc", "out_gs"))


def parse_board(text):
    """'NX,NY,NZ' or 'NX,NY,NZ,G' -> (NX, NY, NZ, G): three integers >= 1 and a finite amplitude G > 0 (default DEFAULT_G); ValueError otherwise"""
    usage = "--checkerboard takes NX,NY,NZ[,G]: three integers >= 1 and a finite amplitude G > 0 (got %r)" % text
    parts = text.split(",")
    if len(parts) not in (3, 4):
        raise ValueError(usage)
    try:
        cell = tuple(int(p) for p in parts[:3])
        g = float(parts[3]) if len(parts) == 4 else DEFAULT_G
    except ValueError:
        raise ValueError(usage)
    board = cell + (g,)
    check_boards([board])
    return board


def check_boards(boards):
    for b in boards or ():
        if len(b) != 4 or any(int(v) != v or v < 1 for v in b[:3]) or not (np.isfinite(b[3]) and b[3] > 0):
            raise ValueError("a checkerboard is NX,NY,NZ[,G]: three integers >= 1 and a finite amplitude G > 0 (got %r)" % (tuple(b),))


def check(weight=None, damp=None, boards=(), maxiter=None):
    """the driver's preconditions, checked before the library is loaded (ValueError)"""
    if weight is not None and not (np.isfinite(weight) and weight >= 0):
        raise ValueError("--weight must be finite and >= 0, not %r" % (weight,))
    if damp is not None and not (np.isfinite(damp) and damp >= 0):
        raise ValueError("--damp must be finite and >= 0, not %r" % (damp,))
    if maxiter is not None and maxiter < 1:
        raise ValueError("--maxiter must be at least 1, not %r" % (maxiter,))
    check_boards(boards)


def azimuthal_checkerboards(c, cell, g=DEFAULT_G):
    """(3, 3 maxvp) float32: the three test models of one board over the joint unknowns Vs | gc | gs -- row 0 the Vs checkerboard of
    +-0.1 km/s in block 0, row 1 +-g in block gc (fast axes 0 / 90 degrees), row 2 +-g in block gs (45 / 135 degrees); zero elsewhere"""
    n = c["nparpi"]
    out = np.zeros((3, 3 * n), np.float32)
    out[0, :n] = checkerboard(c, cell)
    out[1, n:2 * n] = checkerboard(c, cell, g)
    out[2, 2 * n:] = checkerboard(c, cell, g)
    return out


def block_psf_columns(psf):
    """The columns of AzimResolution.dat from dsa_resolution_blocks' measures psf (n, nblocks, 4) of all n = nblocks nb spikes in order.
    Returns dict(block (n,) the spike's own block, others (n, nblocks - 1) the other blocks ascending, rjj, psf_h_km, psf_v_km (n,) of the
    own block (lengths sqrt(sum x^2 d^2 / sum x^2), 0 where the own block's sum x^2 = 0), colocated (n, nblocks - 1) the value at the
    spike's cell in each other block, share (n, nblocks) sum_B x^2 / sum_all x^2 (0 where the total is 0), no_data: spikes whose total is 0)."""
    psf = np.asarray(psf, np.float64)
    if psf.ndim != 3 or psf.shape[2] != 4 or psf.shape[1] < 1 or psf.shape[0] % psf.shape[1]:
        raise ValueError("block_psf_columns: psf must be (nblocks * nb, nblocks, 4), not %r" % (psf.shape,))
    n, nblocks = psf.shape[0], psf.shape[1]
    nb = n // nblocks
    own = np.arange(n) // nb
    others = np.array([[B for B in range(nblocks) if B != o] for o in own], np.int64).reshape(n, nblocks - 1)
    rows = np.arange(n)
    home = psf[rows, own]
    s = home[:, 1]
    has = s > 0
    lh = np.zeros(n); lv = np.zeros(n)
    lh[has] = np.sqrt(home[has, 2] / s[has])
    lv[has] = np.sqrt(home[has, 3] / s[has])
    total = psf[:, :, 1].sum(axis=1)
    share = np.zeros((n, nblocks))
    live = total > 0
    share[live] = psf[live, :, 1] / total[live, None]
    return dict(block=own, others=others, rjj=home[:, 0].copy(), psf_h_km=lh, psf_v_km=lv, colocated=psf[rows[:, None], others, 0], share=share,
                no_data=int((~live).sum()))


def leakage_metrics(psf):
    """From the measures of all spikes of a three-block system (n, 3, 4): the energy share that a block-0 (Vs) spike's image has in blocks
    1 and 2 together, and that a block-1 or block-2 spike's image has in block 0, each as median and worst over the spikes whose image has
    any energy (0 where there is none).  Returns dict(vs_to_g_median, vs_to_g_worst, g_to_vs_median, g_to_vs_worst, spikes_vs, spikes_g)."""
    col = block_psf_columns(psf)
    if col["share"].shape[1] != 3:
        raise ValueError("leakage_metrics: three blocks (Vs, gc, gs), not %d" % col["share"].shape[1])
    live = col["share"].sum(axis=1) > 0
    a = col["share"][(col["block"] == 0) & live]
    b = col["share"][(col["block"] > 0) & live]
    v2g, g2v = a[:, 1] + a[:, 2], b[:, 0]
    stat = lambda v, f: float(f(v)) if v.size else 0.0
    return dict(vs_to_g_median=stat(v2g, np.median), vs_to_g_worst=stat(v2g, np.max), g_to_vs_median=stat(g2v, np.median),
                g_to_vs_worst=stat(g2v, np.max), spikes_vs=int(a.shape[0]), spikes_g=int(b.shape[0]))


def _cells(c):
    """(maxvp, 3) float64: longitude, latitude, depth of the cells as the model files print them, in their vertex order"""
    return np.array([(float(lon), float(lat), float(c["depz"][k])) for _, _, k, lon, lat in vertices(c)], np.float64).reshape(-1, 3)


def write_azim_resolution(path, c, psf):
    """<input>AzimResolution.dat from the measures of all 3 maxvp spikes: one line per (block, cell)"""
    col = block_psf_columns(psf)
    cells = _cells(c)
    nb = cells.shape[0]
    rows = []
    for j in range(col["block"].size):
        lon, lat, dep = cells[j % nb]
        oa, ob = col["others"][j]
        rows.append(dict(lon=lon, lat=lat, depth=dep, block=int(col["block"][j]), rjj=col["rjj"][j], psf_h_km=col["psf_h_km"][j], psf_v_km=col["psf_v_km"][j],
                         colocated_a=col["colocated"][j, 0], share_a=col["share"][j, oa], colocated_b=col["colocated"][j, 1], share_b=col["share"][j, ob]))
    io.write_table(path, AZIM_RESOLUTION_TABLE, rows)


def read_azim_resolution(path):
    return io.read_table(path, AZIM_RESOLUTION_TABLE)


def write_azim_checker(path, c, model, x):
    """<input>AzimChecker.dat.kNN.*: per cell the three input blocks of `model` (3 maxvp,) and the three recovered blocks of x"""
    cells = _cells(c)
    nb = cells.shape[0]
    m = np.asarray(model, np.float64).reshape(3, nb)
    r = np.asarray(x, np.float64).reshape(3, nb)
    io.write_table(path, AZIM_CHECKER_TABLE, [dict(lon=cells[q, 0], lat=cells[q, 1], depth=cells[q, 2], in_vs=m[0, q], in_gc=m[1, q], in_gs=m[2, q],
                                                   out_vs=r[0, q], out_gc=r[1, q], out_gs=r[2, q]) for q in range(nb)])


def read_azim_checker(path):
    return io.read_table(path, AZIM_CHECKER_TABLE)


def checker_metrics(c, model, x, driven):
    """recovery_metrics of the driven block and, per other block, rms(recovered) / rms(input of the driven block) (0 where that input is 0)"""
    nb = c["nparpi"]
    m = np.asarray(model, np.float64).reshape(3, nb)
    r = np.asarray(x, np.float64).reshape(3, nb)
    rms = lambda v: float(np.sqrt((v * v).mean()))
    ref = rms(m[driven])
    leak = {BLOCKS[B]: (rms(r[B]) / ref if ref > 0 else 0.0) for B in range(3) if B != driven}
    return dict(recovery_metrics(m[driven], r[driven], c["nz"] - 1), leak=leak)


# ---- the device side ----

def joint_system_device(lib, c, vsf, obst, weight_azi):
    """dsa_calsurfg_azimuthal with no arrays, then dsa_iteration_system_azimuthal_device: the joint system resident on the drop-in engine.
    Returns dict(eng, m, n, nar, nnz_data, cbst, datweight, norm, dws (3, 2), dsyn, seconds=dict(forward, system))."""
    f = np.float32
    nx, ny, nz, dall, maxvp = c["nx"], c["ny"], c["nz"], c["ndata"], c["nparpi"]
    dsyn, nnz_data, t_fwd = forward_rows(lib, c, vsf, entry="dsa_calsurfg_azimuthal")
    eng = lib.dsa_dropin_engine()
    obst = np.ascontiguousarray(obst, f)
    cbst = np.zeros(dall + 3 * maxvp, f); datweight = np.zeros(dall, f); norm = np.zeros(3 * maxvp, f); dws = np.zeros(6, f)
    m, nar = C.c_int(0), C.c_longlong(0)
    t0 = time.perf_counter()
    call_solver(lib, eng, "dsa_iteration_system_azimuthal_device", nx, ny, nz, dall, _p(obst), _p(dsyn), c["threshold0"], c["weight0"], float(weight_azi),
                _p(cbst), _p(datweight), _p(norm), C.byref(m), C.byref(nar), _p(dws))
    return dict(eng=eng, m=m.value, n=3 * maxvp, nar=nar.value, nnz_data=nnz_data, cbst=cbst, datweight=datweight, norm=norm, dws=dws.reshape(3, 2), dsyn=dsyn,
                seconds=dict(forward=t_fwd, system=time.perf_counter() - t0))


def joint_step_device(lib, c, vsf, obst, log, weight=None, damp=None):
    """The joint step of analyses.azimuthal.azimuthal_step with the rows, the system and the solve on the device; the same bits.  Returns
    dict(dvs, gc, gs, x, itn, istop, weight, damp, system (joint_system_device's), seconds)."""
    check(weight, damp)
    maxvp = c["nparpi"]
    weight = float(c["weight0"]) if weight is None else float(weight)
    damp = float(c["damp"]) if damp is None else float(damp)
    S = joint_system_device(lib, c, vsf, obst, weight)
    x, istop, itn, t_lsmr = lsmr(lib, S["eng"], S["cbst"], damp, S["n"])
    dvs, gc, gs = x[:maxvp], x[maxvp:2 * maxvp], x[2 * maxvp:]
    log(" joint step on the device: %d x %d, %d entries (%d from the rays), weight %g damp %g, %d iterations, istop %d (forward %.3f s, system %.3f s, "
        "LSMR %.3f s)" % (S["m"], S["n"], S["nar"], S["nnz_data"], weight, damp, itn, istop, S["seconds"]["forward"], S["seconds"]["system"], t_lsmr))
    log(" joint step on the device: DWS max / mean Vs %g %g, gc %g %g, gs %g %g" % tuple(float(v) for v in S["dws"].ravel()))
    log(" joint step on the device: min and max velocity variation of its Vs block %7.4f%7.4f (not applied); strength max %.3f %% of Vs" %
        (float(dvs.min()), float(dvs.max()), float(azimuthal_strength(gc, gs).max())))
    return dict(dvs=dvs, gc=gc, gs=gs, x=x, itn=itn, istop=istop, weight=weight, damp=damp, system=S, seconds=dict(S["seconds"], lsmr=t_lsmr))


def joint_resolution(lib, eng, c, m, damp, chunk=None):
    """The block PSF measures of every unknown of the resident joint system (m rows): spikes in chunks of `chunk` (default
    resolution_chunk(m, 3 maxvp, LOCAL_SIZE)), one dsa_resolution_blocks call each, x left on the device.  Returns dict(psf (3 maxvp, 3, 4),
    itn, istop, chunk, calls, seconds)."""
    n = 3 * c["nparpi"]
    chunk = int(chunk or resolution_chunk(m, n, LOCAL_SIZE))
    coords = np.ascontiguousarray(unknown_coords(c))
    psf = np.zeros((n, 3, 4))
    istop = np.zeros(n, np.int32); itn = np.zeros(n, np.int32)
    t0 = time.perf_counter()
    for q in chunks(n, chunk):
        est = np.zeros((q.stop - q.start, 5), np.float32)
        call_solver(lib, eng, "dsa_resolution_blocks", q.stop - q.start, c["ndata"], 3, q.start, _p(coords), C.c_float(damp), *LSMR_ARGS, None, _p(psf[q]),
                    _p(istop[q]), _p(itn[q]), _p(est))
    return dict(psf=psf, itn=itn, istop=istop, chunk=chunk, calls=len(chunks(n, chunk)), seconds=time.perf_counter() - t0)


def joint_checkerboard(lib, eng, c, board, damp):
    """The three test models of one board through one dsa_lsmr_resolution call on the resident joint system.  Returns dict(models (3, 3 maxvp),
    x (3, 3 maxvp), itn, istop, metrics [checker_metrics per driven block], seconds)."""
    models = np.ascontiguousarray(azimuthal_checkerboards(c, board[:3], board[3]))
    x = np.zeros_like(models)
    istop = np.zeros(3, np.int32); itn = np.zeros(3, np.int32); est = np.zeros((3, 5), np.float32)
    t0 = time.perf_counter()
    call_solver(lib, eng, "dsa_lsmr_resolution", 3, c["ndata"], _p(models), 0, None, C.c_float(damp), *LSMR_ARGS, _p(x), None, _p(istop), _p(itn), _p(est))
    seconds = time.perf_counter() - t0
    return dict(models=models, x=x, itn=itn, istop=istop, metrics=[checker_metrics(c, models[B], x[B], B) for B in range(3)], seconds=seconds)


def run(directory, model=None, maxiter=None, out_dir=".", log=print, weight=None, damp=None, resolution=False, checkerboards=(), chunk=None):
    """the driver behind main(); returns (the joint step's result, history: a list of dicts, one per stage)"""
    boards = [tuple(b) for b in checkerboards or ()]
    check(weight, damp, boards, maxiter)
    from .engine import declare_solvers, load_library
    c = io.load(directory)
    if c["ifsyn"] == 1:
        raise ValueError("anisotropy: a synthetic input (ifsyn = 1) has no observed data to test the resolution of")
    if model is not None:
        vsf = np.asfortranarray(io.load(directory, model)["vels"].copy())
    else:
        from . import invert
        vsf, _ = invert.run(directory, maxiter, out_dir, log)
    lib = declare_solvers(load_library())
    obst = np.ascontiguousarray(c["obst"])
    name = os.path.join(out_dir, "DSurfTomo.in")
    history = []
    step = joint_step_device(lib, c, vsf, obst, log, weight, damp)
    write_azimuthal(name + "Azim.dat", c, vsf, step["gc"], step["gs"])
    S = step["system"]
    history.append(dict(stage="step", weight=step["weight"], damp=step["damp"], itn=step["itn"], istop=step["istop"], m=S["m"], n=S["n"], nar=S["nar"],
                        dws=[[float(v) for v in r] for r in S["dws"]], seconds=step["seconds"]))
    if resolution:
        p = joint_resolution(lib, S["eng"], c, S["m"], step["damp"], chunk)
        write_azim_resolution(name + "AzimResolution.dat", c, p["psf"])
        lk = leakage_metrics(p["psf"])
        h = dict(stage="resolution", **_solve_stats(p["itn"], p["istop"]), chunk=p["chunk"], calls=p["calls"], seconds=p["seconds"], leakage=lk,
                 no_data=block_psf_columns(p["psf"])["no_data"])
        history.append(h)
        log(" joint resolution: %s, %d unknowns without data, %d calls of up to %d (%.3f s)" % (_solve_text(h), h["no_data"], h["calls"], h["chunk"], h["seconds"]))
        log(" joint resolution: energy share Vs -> (gc, gs) median %.4f worst %.4f over %d spikes; (gc, gs) -> Vs median %.4f worst %.4f over %d spikes" %
            (lk["vs_to_g_median"], lk["vs_to_g_worst"], lk["spikes_vs"], lk["g_to_vs_median"], lk["g_to_vs_worst"], lk["spikes_g"]))
    for q, board in enumerate(boards):
        k = joint_checkerboard(lib, S["eng"], c, board, step["damp"])
        h = dict(stage="checkerboard", board=board, **_solve_stats(k["itn"], k["istop"]), seconds=k["seconds"], patterns=[])
        for B, mt in enumerate(k["metrics"]):
            write_azim_checker(name + "AzimChecker.dat.k%02d.%s" % (q + 1, BLOCKS[B]), c, k["models"][B], k["x"][B])
            h["patterns"].append(dict(driven=BLOCKS[B], **mt))
            log(" joint checkerboard k%02d %d,%d,%d,%g %s: correlation %.3f gain %.3f; rms(recovered) / rms(input %s): %s  (Vs in km/s, gc and gs dimensionless)" %
                ((q + 1,) + tuple(board) + (BLOCKS[B], mt["corr"], mt["gain"], BLOCKS[B], " ".join("%s %.4g" % kv for kv in mt["leak"].items()))))
        history.append(h)
    return step, history


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("directory")
    ap.add_argument("--model", default=None, metavar="FILE", help="model file in the directory, in MOD's format (default: the model invert.run leaves)")
    ap.add_argument("--maxiter", type=int, default=None, help="outer iterations of the inversion that makes the model (without --model)")
    ap.add_argument("--out", default=".")
    ap.add_argument("--weight", type=float, default=None, metavar="W", help="smoothing weight of the gc and gs blocks (default: the input file's weight0)")
    ap.add_argument("--damp", type=float, default=None, metavar="D", help="damping of the joint step's solves (default: the input file's damp)")
    ap.add_argument("--resolution", action="store_true", help="block PSFs of all 3 maxvp unknowns: <input>AzimResolution.dat and the leakage in the log")
    ap.add_argument("--checkerboard", type=arg_type(parse_board), action="append", default=[], metavar="NX,NY,NZ[,G]",
                    help="a Vs, a gc and a gs checkerboard through the joint step (may be repeated): <input>AzimChecker.dat.kNN.vs / .gc / .gs")
    a = ap.parse_args(argv)
    try:
        check(a.weight, a.damp, a.checkerboard, a.maxiter)
    except ValueError as exc:
        ap.error(str(exc))
    os.makedirs(a.out, exist_ok=True)
    run(a.directory, a.model, a.maxiter, a.out, weight=a.weight, damp=a.damp, resolution=a.resolution, checkerboards=a.checkerboard)
    return 0


if __name__ == "__main__":
    sys.exit(main())
