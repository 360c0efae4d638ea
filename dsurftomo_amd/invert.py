"""The reference's inversion loop (main.f90:346-590) driven through this library, without the Fortran host program.

    python -m dsurftomo_amd.invert <directory with DSurfTomo.in, the data file and MOD> [--maxiter N] [--out DIR]
                                   [--bootstrap R [--bootstrap-seed S]] [--resolution] [--checkerboard NX,NY,NZ ...]
                                   [--tradeoff-weights W1,W2,... [--tradeoff-damps D1,...] [--tradeoff-iter N]]
                                   [--voronoi K,NCELLS [--voronoi-seed S] [--voronoi-zscale F] [--voronoi-damp D] [--voronoi-update]]
                                   [--crossval NFOLDS --crossval-weights W1,W2,... [--crossval-damps D1,...] [--crossval-by datum|path]
                                    [--crossval-seed S] [--crossval-iter N] [--crossval-nonlinear]]
                                   [--tradeoff-nonlinear] [--line-search A1,A2,...]
                                   [--azimuthal [--azimuthal-weight W] [--azimuthal-damp D]]

Per outer iteration: CalSurfG on the device (dsa_calsurfg: dispersion, depth kernels, eikonal solves, rays, Frechet rows),
the glue of main.f90:361-466 (residuals, percentile weights, DWS, regularisation rows), LSMR on the device (bit-identical
to the reference's LSMR), the model update of main.f90:520-535.  By default the matrix never leaves the device
(dsa_calsurfg with null rw / iw / col -> dsa_iteration_system_device -> dsa_lsmr); --host-rows hands it through host
arrays the way the reference does (dsa_calsurfg -> dsa_iteration_system -> dsa_lsmr_dropin), with the same numbers.  Then
(dsa_model_update), and the reference's output files: residualFirst.dat / residualLast.dat (main.f90:397-411),
<input>Measure.dat.iterNNN (main.f90:537-546) and <input>Measure.dat (:575-584), in the reference's formats.
Synthetic tests (ifsyn = 1, main.f90:326-343) forward-model MOD.true; the noise there comes from this module's own
generator, not from the reference's gaussian().  There is no CPU path: without a usable GPU this fails with the engine's
error text.

The optional analyses (--bootstrap, --resolution / --checkerboard, --tradeoff-*, --voronoi, --crossval, --line-search, --azimuthal) are the
modules of dsurftomo_amd/analyses, each with its own description (--help shows them all) and the names analyses/common.py lists.  This module
knows them by four tuples.  ANALYSES = IN_PASS + AFTER_LOOP: in that order their options and descriptions appear in --help and their checks
run; the plans of IN_PASS are iteration_device's keywords, AFTER_LOOP runs once on the final model.  SOLVE_ORDER: the stages of a pass between
dsa_lsmr and the update, as (plan keyword, stage) in the order they run -- the batch solves share the drop-in engine's buffers, so the order
decides what is still resident (iteration_device); the line search or the update comes last.  REPORT_ORDER: the reports of a pass as
(result key, report) in the order of their log lines, which is not the solve order.
"""
import argparse
import ctypes as C
import os
import sys
import time
import types

import numpy as np

from . import io
from .analyses import azimuthal, bootstrap, crossval, line_search, resolution, tradeoff, voronoi
from .engine import declare_solvers as bind, load_library         # (and, below, the rest of what callers and tests reach as invert.<name>)
from .analyses.common import (LOCAL_SIZE, LSMR_ARGS, _p, batch_bytes, forward_rows, lsmr, nonlinear_measures, unknown_coords, unknowns_grid, write_model)
from .analyses.bootstrap import (bootstrap_row_scales, write_std)
from .analyses.resolution import (checkerboard, great_circle_km, parse_checkerboard, psf_columns, recovery_metrics, resolution_chunk)
from .analyses.tradeoff import (TRADEOFF_COLUMNS, check_tradeoff_nonlinear, lcurve_corner, parse_tradeoff_list, read_tradeoff, tradeoff_bytes,
                                tradeoff_chunk, tradeoff_corners, tradeoff_grid, tradeoff_members, tradeoff_nonlinear_rows,
                                tradeoff_nonlinear_select, write_tradeoff)
from .analyses.crossval import (CROSSVAL_COLUMNS, check_crossval, check_crossval_nonlinear, crossval_by_slot, crossval_bytes, crossval_chunk,
                                crossval_folds, crossval_members, crossval_nonlinear_rows, crossval_nonlinear_select, crossval_select, datum_table,
                                read_crossval, write_crossval, write_crossval_residuals)
from .analyses.voronoi import (check_voronoi, parse_voronoi, read_voronoi, voronoi_bytes, voronoi_cells, voronoi_chunk, voronoi_seeds, voronoi_stats,
                               voronoi_xyz, write_voronoi)
from .analyses.line_search import (check_line_search, line_search_candidates, line_search_scores, line_search_select, line_search_step,
                                   parse_line_search)
from .analyses.azimuthal import (azimuthal_axis, azimuthal_step, azimuthal_strength, azimuthal_system, azimuthal_weights, laplacian_rows,
                                 read_azimuthal, write_azimuthal)

IN_PASS = (bootstrap, resolution, tradeoff, voronoi, crossval, line_search)
PLAN_KEYWORDS = tuple(mod.__name__.rsplit(".", 1)[1] for mod in IN_PASS)            # a plan keyword is its module's name
AFTER_LOOP = (azimuthal,)
ANALYSES = IN_PASS + AFTER_LOOP
SOLVE_ORDER = (("bootstrap", bootstrap.solve), ("resolution", resolution.solve_psf), ("resolution", resolution.solve_checkerboards),
               ("tradeoff", tradeoff.solve), ("crossval", crossval.solve), ("voronoi", voronoi.solve), ("crossval", crossval.solve_nonlinear),
               ("tradeoff", tradeoff.solve_nonlinear))
REPORT_ORDER = (("line_search", line_search.report), ("boot", bootstrap.report), ("res", resolution.report_psf), ("res", resolution.report_checkerboards),
                ("trade", tradeoff.report), ("crossval", crossval.report), ("trade_nl", tradeoff.report_nonlinear), ("crossval_nl", crossval.report_nonlinear),
                ("voronoi", voronoi.report))


def write_residuals(path, c, dsyn, obst, datweight):
    """list-directed rows: dist, dsyn, obst, dsyn*w, obst*w, w (main.f90:397-403)"""
    np.savetxt(path, np.column_stack([c["dist"], dsyn, obst, dsyn * datweight, obst * datweight, datweight]), fmt="%16.8f")


def _pass_result(r, dv, ii, **arrays):
    """what iteration() and iteration_device() return of a pass: the statistics of the weighted residuals r (mean and standard deviation in
    fp32 as main.f90 forms them, in ms; rms) and of the update dv as it stands (before it is clamped into the model), LSMR's (istop, itn) = ii,
    dv and the pass's own arrays"""
    f = np.float32
    nd = r.size
    mean = f(r.sum(dtype=f) / f(nd))
    std = f(np.sqrt(f((r * r).sum(dtype=f) / f(nd)) - mean * mean))
    rms = f(np.sqrt((r.astype(np.float64) ** 2).sum()) / np.sqrt(nd))
    return dict(mean_ms=1e3 * float(mean), std_ms=1e3 * float(std), rms=float(rms), dv_min=float(f(dv.min())), dv_max=float(f(dv.max())),
                itn=ii[1], istop=ii[0], dv=dv, **arrays)


def iteration_device(lib, c, vsf, obst, log, **plans):
    """One pass of main.f90:349-535 with the matrix resident on the device from CalSurfG to LSMR: dsa_calsurfg leaves the
    rows there (null rw / iw / col), dsa_iteration_system_device applies weights / appends the regularisation rows / builds
    both orderings in place, dsa_lsmr solves.  Same numbers as iteration() (tests/test_gpu_lsmr.py compares every bit).
    plans: what the analyses add to the pass, by PLAN_KEYWORDS, each what its module's plan() returns (None: not in this pass); the stages
    run in SOLVE_ORDER on the system dsa_lsmr just used.
    bootstrap = (R, seed): R row-resampled solves by dsa_lsmr_batch (returned as "boot").
    resolution = dict(psf=bool, chunk=int or None, cells=[(NX, NY, NZ), ...]): the resolution tests (returned as "res": "psf" from
    resolution_psf, "checker" from checkerboard_tests).
    tradeoff = dict(weights=[...], damps=[...], chunk=int or None): the trade-off sweep (returned as "trade" from lsmr_tradeoff_sweep).
    voronoi = dict(nreal, ncells, seed, zscale, damp, chunk, update): the Poisson-Voronoi ensemble of the data rows (returned as "voronoi"
    from lsmr_voronoi_ensemble); with update, float32 of its mean is the update applied to vsf and returned as "dv" (dv_min / dv_max are
    its), dsa_lsmr's own stays in "dv_lsmr".
    crossval = dict(weights=[...], damps=[...], fold=(ndata,) int32, nfolds, chunk=int or None, want_x=bool): the K-fold cross-validation
    (returned as "crossval" from lsmr_crossval_sweep).
    line_search = [A1, A2, ...]: the update is applied at the step length among these whose model has the smallest true misfit
    (line_search_step, returned as "line_search"); "dv" stays the full-length update.
    tradeoff["nonlinear"] / crossval["nonlinear"]: after all of the above and before the line search / the update, the sweep's members
    through forward_steps_members on the model as it stands (returned as "trade_nl" / "crossval_nl"; the forward call re-dices the maps
    and leaves the resident matrix alone).
    The stages take the pass's system s (m rows of nar entries, nnz_data of them from the rays) and their plan, and put their result into res.
    Three things are the pass's own and written out here: the cross-validation's updates stay resident for its nonlinear stage only when one
    call held all pairs (crossval.solve) and no Voronoi batch solve comes between the two; Voronoi's update replaces dv; the line search
    replaces dsa_model_update."""
    unknown = sorted(set(plans) - set(PLAN_KEYWORDS))
    if unknown:
        raise TypeError("iteration_device() got an unexpected keyword argument %r" % unknown[0])
    f = np.float32
    nx, ny, nz, dall = c["nx"], c["ny"], c["nz"], c["ndata"]
    maxvp = c["nparpi"]
    dsyn, nnz_data, t_fwd = forward_rows(lib, c, vsf)
    eng = lib.dsa_dropin_engine()
    cbst = np.zeros(dall + maxvp, f); datweight = np.zeros(dall, f); norm = np.zeros(maxvp, f); dws = np.zeros(2, f)
    m, nar2 = C.c_int(0), C.c_longlong(0)
    t0 = time.perf_counter()
    rc = lib.dsa_iteration_system_device(eng, nx, ny, nz, dall, _p(obst), _p(dsyn), c["threshold0"], c["weight0"], _p(cbst), _p(datweight), _p(norm),
                                         C.byref(m), C.byref(nar2), _p(dws))
    if rc != 0:
        raise RuntimeError("dsa_iteration_system_device failed (%d): %s" % (rc, lib.dsa_error_string(eng).decode()))
    t_glue = time.perf_counter() - t0
    log("Maximum and Average DWS values: %g %g" % (dws[0], dws[1]))
    dv, istop, itn, t_lsmr = lsmr(lib, eng, cbst, c["damp"], maxvp)
    s = types.SimpleNamespace(lib=lib, eng=eng, c=c, vsf=vsf, obst=obst, cbst=cbst, datweight=datweight, m=m.value, nar=nar2.value, nnz_data=nnz_data)
    s.crossval_may_stay = not plans.get("voronoi")      # a Voronoi batch solve would overwrite the solutions dsa_forward_steps(steps = NULL) reads
    res = {}
    for key, stage in SOLVE_ORDER:
        if plans.get(key):
            stage(s, plans[key], res)
    if "voronoi" in res:
        res["dv_lsmr"] = dv
        if plans["voronoi"].get("update"):      # Voronoi's update replaces dv: the ensemble's mean is the step of this pass, dsa_lsmr's is only kept
            dv = np.ascontiguousarray(res["voronoi"]["mean"].astype(f))
    out = _pass_result(cbst[:dall], dv, (istop, itn), dsyn=dsyn, datweight=datweight, nar=nar2.value, m=m.value, dws=(float(dws[0]), float(dws[1])),
                       seconds=dict(forward=t_fwd, glue=t_glue, lsmr=t_lsmr), norm=norm, cbst=cbst, **res)
    if plans.get("line_search"):                # the line search replaces dsa_model_update: the winner among its candidate models is the model the pass leaves
        ls = out["line_search"] = line_search_step(lib, c, vsf, dv, obst, datweight, plans["line_search"])
        vsf[...] = ls["models"][ls["chosen"]]
    else:
        lib.dsa_model_update(nx, ny, nz, _p(dv), _p(vsf), c["minvel"], c["maxvel"])
    return out


def iteration(lib, c, vsf, obst, log):
    """One pass of main.f90:349-535 on the model vsf (updated in place), the matrix going through host arrays like in the
    reference (dsa_calsurfg -> dsa_iteration_system -> dsa_lsmr_dropin).  Returns the statistics of the pass."""
    f = np.float32
    nx, ny, nz, dall = c["nx"], c["ny"], c["nz"], c["ndata"]
    maxvp = c["nparpi"]
    maxnar = int(f(c["spfra"]) * dall * nx * ny * nz)                                  # main.f90:287
    rw = np.zeros(maxnar, f); col = np.zeros(maxnar, np.int32); iw = np.zeros(2 * maxnar + 1, np.int32)
    dsyn, nar, t_fwd = forward_rows(lib, c, vsf, iw, rw, col)
    cbst = np.zeros(dall + maxvp, f); datweight = np.zeros(dall, f); norm = np.zeros(maxvp, f); dws = np.zeros(2, f)
    m, nar2 = C.c_int(0), C.c_longlong(0)
    t0 = time.perf_counter()
    rc = lib.dsa_iteration_system(nx, ny, nz, dall, nar, maxnar, _p(rw), _p(iw), _p(col), _p(obst), _p(dsyn), c["threshold0"], c["weight0"],
                                  _p(cbst), _p(datweight), _p(norm), C.byref(m), C.byref(nar2), _p(dws))
    if rc != 0:
        raise RuntimeError("increase sparsity fraction(spfra)" if rc == -6 else "dsa_iteration_system failed (%d)" % rc)
    t_glue = time.perf_counter() - t0
    log("Maximum and Average DWS values: %g %g" % (dws[0], dws[1]))
    dv = np.zeros(maxvp, f)
    ii = [C.c_int(0), C.c_int(0)]
    ff = [C.c_float(0) for _ in range(5)]
    i32 = lambda v: C.byref(C.c_int(int(v)))
    f32 = lambda v: C.byref(C.c_float(float(v)))
    n = nar2.value
    t0 = time.perf_counter()
    rc = lib.dsa_lsmr_dropin(i32(m.value), i32(maxvp), i32(2 * n + 1), i32(n), _p(iw), _p(rw), _p(cbst), f32(c["damp"]), *map(f32, LSMR_ARGS[:3]),
                             *map(i32, LSMR_ARGS[3:]), i32(0), _p(dv), C.byref(ii[0]), C.byref(ii[1]), *[C.byref(v) for v in ff])
    if rc != 0:
        raise RuntimeError("dsa_lsmr_dropin: %s" % lib.dsa_dropin_error().decode())
    t_lsmr = time.perf_counter() - t0
    out = _pass_result(cbst[:dall], dv, (ii[0].value, ii[1].value), dsyn=dsyn, datweight=datweight, nar=n, m=m.value, dws=(float(dws[0]), float(dws[1])),
                       seconds=dict(forward=t_fwd, glue=t_glue, lsmr=t_lsmr), norm=norm, cbst=cbst)
    lib.dsa_model_update(nx, ny, nz, _p(dv), _p(vsf), c["minvel"], c["maxvel"])
    return out


def check_options(options, host_rows, maxiter, c=None):
    """run()'s analysis keywords over the defaults of the modules' OPTIONS -- one that no analysis declares is a TypeError, like any unknown
    keyword -- and every analysis's preconditions on them (ValueError), before anything touches the GPU; c: the case once it is read.
    Returns the resolved options."""
    o = {keyword: default for mod in ANALYSES for _, keyword, default, _ in mod.OPTIONS}
    unknown = sorted(set(options) - set(o))
    if unknown:
        raise TypeError("run() got an unexpected keyword argument %r" % unknown[0])
    o.update(options)
    for mod in ANALYSES:
        mod.check(o, host_rows, maxiter, c)
    return o


def run(directory, maxiter=None, out_dir=".", log=print, seed=1, host_rows=False, **options):
    """options: the analyses' keywords (check_options), which are the destinations of main()'s flags"""
    o = check_options(options, host_rows, maxiter)
    lib = bind(load_library())
    c = io.load(directory)
    maxiter = c["maxiter"] if maxiter is None else maxiter
    check_options(options, host_rows, maxiter, c)
    vsf = np.asfortranarray(c["vels"].copy())
    obst = np.ascontiguousarray(c["obst"])
    vsftrue = None
    if c["ifsyn"] == 1:                                                                 # main.f90:326-343
        vsftrue = io.load(directory, "MOD.true")["vels"]
        ct = dict(c); ct["vels"] = vsftrue
        obst = io.call_synthetic(ct, 0.0)
        g = np.random.default_rng(seed).standard_normal(obst.size).astype(np.float32)
        obst = (obst * (np.float32(1.0) + c["noiselevel"] * g)).astype(np.float32)
    name = os.path.join(out_dir, "DSurfTomo.in")
    history = []
    ctx = types.SimpleNamespace(o=o, lib=lib, c=c, vsf=vsf, obst=obst, name=name, log=log, history=history)     # what the reports take; it and plans per pass
    for it in range(1, maxiter + 1):
        ctx.it, ctx.plans = it, dict(zip(PLAN_KEYWORDS, (mod.plan(o, c, it, maxiter) for mod in IN_PASS)))          # (with host_rows the checks leave no plan)
        st = iteration(lib, c, vsf, obst, log) if host_rows else iteration_device(lib, c, vsf, obst, log, **ctx.plans)
        log("%2dth iteration..." % it)
        log(" mean,std_devs and rms of residual after weighting: %8.1fms %8.2fms %8.3f" % (st["mean_ms"], st["std_ms"], st["rms"]))
        log(" min and max velocity variation %7.4f%7.4f" % (st["dv_min"], st["dv_max"]))
        log("   (forward %.3f s, system %.3f s, LSMR %.3f s: %d iterations, istop %d, %d x %d, %d entries)" %
            (st["seconds"]["forward"], st["seconds"]["glue"], st["seconds"]["lsmr"], st["itn"], st["istop"], st["m"], c["nparpi"], st["nar"]))
        if it == 1:
            write_residuals(os.path.join(out_dir, "residualFirst.dat"), c, st["dsyn"], obst, st["datweight"])
        if it == maxiter:
            write_residuals(os.path.join(out_dir, "residualLast.dat"), c, st["dsyn"], obst, st["datweight"])
        write_model(name + "Measure.dat.iter%03d" % it, c, vsf)
        h = {k: st[k] for k in ("mean_ms", "std_ms", "rms", "dv_min", "dv_max", "itn", "istop", "nar", "m", "dws", "seconds")}      # what the history keeps of a pass
        for key, report in REPORT_ORDER:
            if key in st:
                report(ctx, st, h)
        history.append(h)
    for mod in AFTER_LOOP:                      # a step on the final model; nothing of it is applied
        plan = mod.plan(o, c, maxiter, maxiter)
        if plan:
            st, h = {}, {}
            mod.solve(ctx, plan, st)
            mod.report(ctx, st, h)
            history.append(h)
    if vsftrue is not None:
        write_model(os.path.join(out_dir, "Vs_model.real"), c, vsftrue)
        write_model(name + "Syn.dat", c, vsf)
    else:
        write_model(name + "Measure.dat", c, vsf)
    log("Program finishes successfully")
    return vsf, history


def main(argv=None):
    ap = argparse.ArgumentParser(description="\n".join([__doc__] + [mod.__doc__ for mod in ANALYSES]), formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("directory")
    ap.add_argument("--maxiter", type=int, default=None)
    ap.add_argument("--out", default=".")
    ap.add_argument("--host-rows", action="store_true", help="hand the matrix through host arrays like the reference (default: it stays on the device)")
    for mod in ANALYSES:
        for flag, _, default, arguments in mod.OPTIONS:
            if flag:
                ap.add_argument(flag, **dict(dict(default=default), **arguments))
    args = vars(ap.parse_args(argv))
    directory, maxiter, out, host_rows = (args.pop(k) for k in ("directory", "maxiter", "out", "host_rows"))
    try:
        check_options(args, host_rows, maxiter)
    except ValueError as exc:
        ap.error(str(exc))
    os.makedirs(out, exist_ok=True)
    run(directory, maxiter, out, host_rows=host_rows, **args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
