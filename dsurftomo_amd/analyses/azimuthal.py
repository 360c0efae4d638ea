"""--azimuthal adds one joint step for Vs and 2psi azimuthal anisotropy (Liu et al. 2019) after the last outer iteration:
c(psi) = c0 + A1 cos 2psi + A2 sin 2psi with A1 = int (Vs/2)(dc/dVs) gc dz, A2 likewise with gs; the unknowns gc = Gc/L and gs = Gs/L live on
the Vs unknowns' grid.  azimuthal_step calls dsa_calsurfg_azimuthal once on the final model (the rays carry the 2psi weights of every step into
two more blocks of columns, Rayleigh periods only) and assembles the joint system in NumPy (azimuthal_system): the reference's 0/1 data
weights (azimuthal_weights: its percentile rule), rows scaled by them, and its first-difference Laplacian rows once per block -- weight0 on
the Vs block, --azimuthal-weight W (default weight0) on gc and gs -- then dsa_spmv_load and dsa_lsmr with the loop's LSMR arguments (common.LSMR_ARGS) and
--azimuthal-damp D (default the input file's damp).  <input>Azim.dat lists longitude, latitude, depth, Vs, gc, gs, the strength
50 sqrt(gc^2 + gs^2) in per cent of Vs and the fast axis 0.5 atan2(gs, gc) in degrees clockwise from north (write_azimuthal /
read_azimuthal).  The Vs block of the joint solution is logged (min / max) and NOT applied: every other file is a plain run's, byte for byte.
"""
import ctypes as C
import time

import numpy as np

from .common import _p, call_solver, forward_rows, lsmr, vertices


def azimuthal_weights(res, threshold0):
    """the reference's 0/1 data weights of the residuals res (main.f90:361-372 with getpercentile.f90:27-30): weight 0 outside
    [q25, q75] * threshold0, q25 / q75 the elements int(0.25 N) and int(0.75 N) (1-based) of the sorted residuals; fp32 like
    dsa_iteration_system"""
    f = np.float32
    res = np.ascontiguousarray(res, f).ravel()
    n = res.size
    i25, i75 = int(f(0.25) * f(n)), int(f(0.75) * f(n))
    if i25 < 1 or i75 < 1:
        raise ValueError("azimuthal_weights: %d residuals are too few for the quartile rule" % n)
    ra = np.sort(res)
    lo, hi = f(ra[i25 - 1] * f(threshold0)), f(ra[i75 - 1] * f(threshold0))
    return np.where((res < lo) | (res > hi), f(0), f(1)).astype(f)


def laplacian_rows(nvx, nvz, nl, weight, row0, col0):
    """the reference's first-difference Laplacian rows (main.f90:420-457; dsa_iteration_system's) for one block of nvx*nvz*nl unknowns,
    one row per unknown in (k, j, i) order: 2 w on the block's faces, 6 w and six -w inside, fp32.  Rows row0 + 1 .., columns col0 + 1 ..
    (1-based).  Returns (rw, row, col)."""
    f = np.float32
    w = f(weight)
    plane = nvz * nvx
    rw, row, col = [], [], []
    r = row0
    for k in range(1, nl + 1):
        for j in range(1, nvz + 1):
            for i in range(1, nvx + 1):
                r += 1
                here = (k - 1) * plane + (j - 1) * nvx + i
                if i in (1, nvx) or j in (1, nvz) or k in (1, nl):
                    rw.append(f(2.0) * w); row.append(r); col.append(col0 + here)
                else:
                    for q, nb in enumerate((here, here - 1, here + 1, here - nvx, here + nvx, here - plane, here + plane)):
                        rw.append(f(6.0) * w if q == 0 else f(-1.0) * w); row.append(r); col.append(col0 + nb)
    return np.array(rw, f), np.array(row, np.int32), np.array(col, np.int32)


def azimuthal_system(c, rw, row, col, res, datweight, weight0, weight_azi):
    """The joint system of the azimuthal step from dsa_calsurfg_azimuthal's rows (rw, row, col: 1-based, columns up to 3 maxvp, blocks
    Vs | gc | gs) and the residuals res: every entry scaled by its datum's weight, the right-hand side the weighted residuals, and below the
    dall data rows the Laplacian rows of the three blocks -- block B's at rows dall + B maxvp + index, weight0 on Vs, weight_azi on gc and
    gs.  Returns dict(m, n, rw, row, col, b): m = dall + 3 maxvp rows, n = 3 maxvp columns, COO 1-based, fp32."""
    f = np.float32
    nvx, nvz, nl, dall = c["nx"] - 2, c["ny"] - 2, c["nz"] - 1, c["ndata"]
    maxvp = nvx * nvz * nl
    rw = np.ascontiguousarray(rw, f); row = np.ascontiguousarray(row, np.int32); col = np.ascontiguousarray(col, np.int32)
    res = np.ascontiguousarray(res, f); datweight = np.ascontiguousarray(datweight, f)
    if not (rw.size == row.size == col.size) or res.size != dall or datweight.size != dall:
        raise ValueError("azimuthal_system: rw / row / col differ in length, or res / datweight do not hold ndata = %d values" % dall)
    if rw.size and (row.min() < 1 or row.max() > dall or col.min() < 1 or col.max() > 3 * maxvp):
        raise ValueError("azimuthal_system: a row outside 1..%d or a column outside 1..%d" % (dall, 3 * maxvp))
    if not (np.isfinite(weight0) and np.isfinite(weight_azi) and weight0 >= 0 and weight_azi >= 0):
        raise ValueError("azimuthal_system: the smoothing weights must be finite and >= 0")
    parts = [(rw * datweight[row - 1], row, col)]
    for B in range(3):
        parts.append(laplacian_rows(nvx, nvz, nl, weight0 if B == 0 else weight_azi, dall + B * maxvp, B * maxvp))
    b = np.zeros(dall + 3 * maxvp, f)
    b[:dall] = res * datweight
    return dict(m=dall + 3 * maxvp, n=3 * maxvp, rw=np.concatenate([q[0] for q in parts]).astype(f),
                row=np.concatenate([q[1] for q in parts]).astype(np.int32), col=np.concatenate([q[2] for q in parts]).astype(np.int32), b=b)


def azimuthal_strength(gc, gs):
    """peak-to-peak 2psi variation of Vs in per cent: 50 sqrt(gc^2 + gs^2)"""
    return 50.0 * np.hypot(np.asarray(gc, np.float64), np.asarray(gs, np.float64))


def azimuthal_axis(gc, gs):
    """fast axis in degrees clockwise from north, in (-90, 90]: 0.5 atan2(gs, gc)"""
    return np.degrees(0.5 * np.arctan2(np.asarray(gs, np.float64), np.asarray(gc, np.float64)))


def write_azimuthal(path, c, vsf, gc, gs):
    """<input>Azim.dat: per interior vertex in write_model's order longitude, latitude, depth, Vs ('(4f10.5)'), gc, gs ('(2f13.8)'), strength in
    per cent of Vs and fast axis in degrees from north ('(2f11.5)'); gc / gs: (maxvp,) in the order of the LSMR unknowns"""
    nx, ny, nz = c["nx"], c["ny"], c["nz"]
    gc = np.asarray(gc, np.float64).reshape(nz - 1, ny - 2, nx - 2); gs = np.asarray(gs, np.float64).reshape(nz - 1, ny - 2, nx - 2)
    st, ax = azimuthal_strength(gc, gs), azimuthal_axis(gc, gs)
    with open(path, "w") as fh:
        for i, j, k, lon, lat in vertices(c):
            fh.write("%10.5f%10.5f%10.5f%10.5f%13.8f%13.8f%11.5f%11.5f\n" %
                     (lon, lat, c["depz"][k], vsf[i + 1, j + 1, k], gc[k, j, i], gs[k, j, i], st[k, j, i], ax[k, j, i]))


def read_azimuthal(path):
    """the columns of <input>Azim.dat as a dict of float64 arrays, one entry per line: lon, lat, depth, vs, gc, gs, strength, axis"""
    a = np.loadtxt(path, ndmin=2)
    if a.shape[1] != 8:
        raise ValueError("%s: %d columns, not the 8 of an Azim.dat" % (path, a.shape[1]))
    return dict(zip(("lon", "lat", "depth", "vs", "gc", "gs", "strength", "axis"), a.T.copy()))


def check_azimuthal(azimuthal, weight=None, damp=None):
    """the azimuthal step's preconditions, checked before anything touches the GPU"""
    if not azimuthal:
        if weight is not None or damp is not None:
            raise ValueError("--azimuthal-weight / --azimuthal-damp need --azimuthal")
        return
    for name, v in (("--azimuthal-weight", weight), ("--azimuthal-damp", damp)):
        if v is not None and not (np.isfinite(v) and v >= 0):
            raise ValueError("%s must be finite and >= 0, not %r" % (name, v))


def azimuthal_step(lib, c, vsf, obst, log, weight=None, damp=None):
    """The joint Vs / gc / gs step on the model vsf (not modified): one dsa_calsurfg_azimuthal, azimuthal_system, dsa_spmv_load and dsa_lsmr
    on the drop-in engine.  weight: the smoothing weight of the gc and gs blocks (default weight0), damp: LSMR's (default the input file's).
    Returns dict(dvs, gc, gs (maxvp,), x, itn, istop, dsyn, datweight, rw / row / col (the call's rows as they came: unweighted), system,
    seconds)."""
    check_azimuthal(True, weight, damp)
    f = np.float32
    nx, ny, nz, dall, maxvp = c["nx"], c["ny"], c["nz"], c["ndata"], c["nparpi"]
    weight = float(c["weight0"]) if weight is None else float(weight)
    damp = float(c["damp"]) if damp is None else float(damp)
    maxnar = 3 * int(f(c["spfra"]) * dall * nx * ny * nz)                               # main.f90:287, once per block
    rw = np.zeros(maxnar, f); col = np.zeros(maxnar, np.int32); iw = np.zeros(maxnar + 1, np.int32)
    try:
        dsyn, n, t_fwd = forward_rows(lib, c, vsf, iw, rw, col, "dsa_calsurfg_azimuthal")
    finally:
        lib.dsa_dropin_set_capacity(0)
    rw, row, col = rw[:n].copy(), iw[1:n + 1].copy(), col[:n].copy()
    obst = np.ascontiguousarray(obst, f)
    res = (obst - dsyn).astype(f)
    datweight = azimuthal_weights(res, c["threshold0"])
    S = azimuthal_system(c, rw, row, col, res, datweight, c["weight0"], weight)
    eng = lib.dsa_dropin_engine()
    t0 = time.perf_counter()
    call_solver(lib, eng, "dsa_spmv_load", S["m"], S["n"], C.c_longlong(S["rw"].size), _p(S["rw"]), _p(S["row"]), _p(S["col"]))
    x, istop, itn, _ = lsmr(lib, eng, S["b"], damp, S["n"])
    t_lsmr = time.perf_counter() - t0
    dvs, gc, gs = x[:maxvp], x[maxvp:2 * maxvp], x[2 * maxvp:]
    log(" azimuthal step: %d x %d, %d entries (%d from the rays: %d Vs, %d gc, %d gs), weight %g damp %g, %d iterations, istop %d "
        "(forward %.3f s, LSMR %.3f s)" % (S["m"], S["n"], S["rw"].size, n, int((col <= maxvp).sum()), int(((col > maxvp) & (col <= 2 * maxvp)).sum()),
                                           int((col > 2 * maxvp).sum()), weight, damp, itn, istop, t_fwd, t_lsmr))
    log(" azimuthal step: min and max velocity variation of its Vs block %7.4f%7.4f (not applied); strength max %.3f %% of Vs" %
        (float(dvs.min()), float(dvs.max()), float(azimuthal_strength(gc, gs).max())))
    return dict(dvs=dvs, gc=gc, gs=gs, x=x, itn=itn, istop=istop, dsyn=dsyn, datweight=datweight, rw=rw, row=row, col=col,
                system=S, weight=weight, damp=damp, seconds=dict(forward=t_fwd, lsmr=t_lsmr))


OPTIONS = (
    ("--azimuthal", "azimuthal", False, dict(action="store_true",
        help="after the last iteration, one joint step for Vs and the 2psi azimuthal anisotropy gc = Gc/L, gs = Gs/L on the final model "
             "(Rayleigh periods): <input>Azim.dat (Vs, gc, gs, strength in per cent of Vs, fast axis in degrees from north); nothing of it "
             "is applied to the model")),
    ("--azimuthal-weight", "azimuthal_weight", None, dict(type=float, metavar="W", help="smoothing weight of the gc and gs blocks (default: the input file's weight0)")),
    ("--azimuthal-damp", "azimuthal_damp", None, dict(type=float, metavar="D", help="damping of the azimuthal step's solve (default: the input file's damp)")),
)


def check(o, host_rows, maxiter, c):
    check_azimuthal(o["azimuthal"], o["azimuthal_weight"], o["azimuthal_damp"])


def plan(o, c, it, maxiter):
    """a step after the loop, not a stage of a pass: run() asks once, with it = maxiter"""
    return dict(weight=o["azimuthal_weight"], damp=o["azimuthal_damp"]) if o["azimuthal"] and it == maxiter else None


def solve(s, plan, res):
    res["azimuthal"] = azimuthal_step(s.lib, s.c, s.vsf, s.obst, s.log, plan["weight"], plan["damp"])


def report(ctx, st, h):
    az = st["azimuthal"]
    write_azimuthal(ctx.name + "Azim.dat", ctx.c, ctx.vsf, az["gc"], az["gs"])
    h["azimuthal"] = dict(weight=az["weight"], damp=az["damp"], itn=az["itn"], istop=az["istop"], nar=int(az["rw"].size), dvs_min=float(az["dvs"].min()),
                          dvs_max=float(az["dvs"].max()), strength_max=float(azimuthal_strength(az["gc"], az["gs"]).max()), seconds=az["seconds"])
