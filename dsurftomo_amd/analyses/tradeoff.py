"""--tradeoff-weights W1,W2,... adds the regularisation trade-off (L-) curve of one outer iteration's linearised step (--tradeoff-iter N,
default 1): after that iteration's dsa_lsmr, dsa_lsmr_tradeoff solves the same resident system once per (weight, damp) pair of the grid
weights x damps (--tradeoff-damps, default the input file's damp; weight-major, tradeoff_grid), member k with the regularisation rows
rebuilt with its weight in place of weight0 and its own damp: what a rerun of this program with those two parameters would solve in that
iteration, bit for bit, without its forward call.  The calls are chunked in multiples of 64 members (tradeoff_chunk).
<input>Tradeoff.dat lists per member: weight, damp, the data misfit ||r||, the roughness ||C x|| (C the integer coefficients of the
regularisation rows: free of the weight), ||x||, itn, istop, min and max of the update; the log and the history add, per damp, the corner
of the curve (lcurve_corner: the largest Menger curvature of (log ||C x||, log ||r||) over increasing weight).  The inversion itself
runs on with the input file's parameters: no other output changes.  Device-resident rows only (not with --host-rows); combines with
--bootstrap / --resolution / --checkerboard.

--tradeoff-nonlinear (with --tradeoff-weights) and --crossval-nonlinear (with --crossval) judge the members of those two sweeps by the TRUE
travel times through the models they would produce, not by the linearised residual b - A x alone.  After all linear
analyses of the swept iteration, just before the line search / the model update, every member's raw update goes through dsa_forward_steps
(io.call_forward_steps: dicing 8, no alpha, the input file's minvel / maxvel, this iteration's datweight, in chunks): the member's model --
what a rerun with its (weight, damp) would hold after that iteration -- is built on the device, forward-modelled with the others, and its
misfit sums { sum (w r)^2, sum r^2 } (nonlinear_measures restates them) are reduced there.  <input>TradeoffNonlinear.dat lists per member:
weight, damp, the weighted rms the linear system predicts (sqrt(measures[0] / ndata) of the sweep), the true weighted rms, the true plain rms
(rms = sqrt(sum / ndata)) and its dispersion curves without a root; the log names, per damp, the member with the smallest true weighted rms
and the corner of (roughness, true misfit) beside the linear one.  17 significant digits (io.read_tradeoff_nonlinear /
read_crossval_nonlinear return the numbers bit for bit).  No other output changes.  Device-resident rows only.
"""
import ctypes as C
import time

import numpy as np

from .. import io
from .common import LOCAL_SIZE, LSMR_ARGS, _check_outer, _check_values, _fit, _p, _solve_stats, _solve_text, arg_type, batch_bytes, call_solver, chunks, forward_steps_members


def tradeoff_bytes(m, n, nar, local_size, nreal):
    """device bytes of a dsa_lsmr_tradeoff call for nreal members on an m x n system of nar entries: the batch buffers (batch_bytes,
    whose temporary bounds the call's nreal n + m + nreal), the two coefficient copies of the values (nar floats each) and the measures'
    block partials and results (fp64: two per 64 rows, one per 1024 unknowns, three per member, in groups of 64)"""
    Rp = 64 * ((nreal + 63) // 64)
    return batch_bytes(m, n, local_size, nreal) + 8 * nar + 8 * Rp * (2 * -(-m // 64) + -(-n // 1024) + 3)


def tradeoff_chunk(m, n, nar, local_size, budget=32 << 30, cap=4096):
    """members per dsa_lsmr_tradeoff call on an m x n system of nar entries: cap, lowered in multiples of 64 until tradeoff_bytes fits
    `budget` (64 at the least)"""
    return _fit(cap, 64, lambda k: tradeoff_bytes(m, n, nar, local_size, k), budget)


def parse_tradeoff_list(text):
    """'V1,V2,...' -> [V1, V2, ...]: at least one float, every one finite and >= 0 (ValueError otherwise)"""
    try:
        vals = [float(p) for p in text.split(",")]
    except ValueError:
        vals = []
    if not vals or not all(np.isfinite(v) and v >= 0 for v in vals):
        raise ValueError("a trade-off list is V1,V2,...: at least one finite number >= 0 (got %r)" % text)
    return vals


def tradeoff_grid(weights, damps):
    """(weight, damp) float32 arrays of the len(weights) * len(damps) members, weight-major: member i * len(damps) + j = (weights[i], damps[j])"""
    w = np.asarray(weights, np.float32).ravel()
    d = np.asarray(damps, np.float32).ravel()
    return np.repeat(w, d.size), np.tile(d, w.size)


def lcurve_corner(misfit, rough):
    """Index of the corner of a trade-off curve given in order of increasing weight, or None.  Points where either value is not a
    finite number > 0 are skipped; every three consecutive remaining points P1 P2 P3 = (log rough, log misfit) give P2 the Menger
    curvature 2 |P1P2 x P2P3| / (|P1P2| |P2P3| |P1P3|), signed so that the vertex of an L-shaped curve is positive: with increasing
    weight the roughness falls at first at little cost in misfit (the curve runs towards -x), then the misfit rises (towards +y), a
    clockwise turn.  Returns the index (into the arrays given) of the largest positive curvature; None with fewer than three usable
    points or no positive curvature (a turn whose sine is below 1e-12 counts as none)."""
    mis = np.asarray(misfit, np.float64).ravel()
    rou = np.asarray(rough, np.float64).ravel()
    use = [i for i in range(min(mis.size, rou.size)) if np.isfinite(mis[i]) and np.isfinite(rou[i]) and mis[i] > 0 and rou[i] > 0]
    best, where = 0.0, None
    for a, b, c in zip(use, use[1:], use[2:]):
        x1, y1, x2, y2, x3, y3 = (np.log(v) for v in (rou[a], mis[a], rou[b], mis[b], rou[c], mis[c]))
        cross = (x2 - x1) * (y3 - y2) - (y2 - y1) * (x3 - x2)
        legs = np.hypot(x2 - x1, y2 - y1) * np.hypot(x3 - x2, y3 - y2)
        den = legs * np.hypot(x3 - x1, y3 - y1)
        if abs(cross) <= 1e-12 * legs:                      # (the sine of the turn is rounding noise of the logarithms: a straight line)
            continue
        if den > 0 and -2.0 * cross / den > best:
            best, where = -2.0 * cross / den, b
    return where


TRADEOFF_TABLE = (False, (("weight", "%.9g", "f32"), ("damp", "%.9g", "f32"), ("misfit", "%.17g", "f64"), ("rough", "%.17g", "f64"), ("xnorm", "%.17g", "f64"),
                          ("itn", "%d", "int"), ("istop", "%d", "int"), ("dv_min", "%.9g", "f32"), ("dv_max", "%.9g", "f32")))
TRADEOFF_COLUMNS = io.column_names(TRADEOFF_TABLE)


def write_tradeoff(path, members):
    """one line per member: weight damp ||r|| ||C x|| ||x|| itn istop min(dv) max(dv), no header line (io.write_table with TRADEOFF_TABLE);
    the float32 values with 9 significant digits, the norms (float64) with 17: read_tradeoff gives the same values back"""
    io.write_table(path, TRADEOFF_TABLE, members)


def read_tradeoff(path):
    """the members of a file of write_tradeoff: a list of dicts with the keys TRADEOFF_COLUMNS (weight, damp and the update's extremes
    are float32 values, the norms float64)"""
    return io.read_table(path, TRADEOFF_TABLE)


def tradeoff_corners(members):
    """per damp (in order of first appearance) the corner of its curve over increasing weight: [dict(damp, weight, member)], weight and
    member (index into members) None where lcurve_corner finds none"""
    out = []
    for d in dict.fromkeys(t["damp"] for t in members):
        idx = sorted((i for i, t in enumerate(members) if t["damp"] == d), key=lambda i: members[i]["weight"])
        k = lcurve_corner([members[i]["misfit"] for i in idx], [members[i]["rough"] for i in idx])
        out.append(dict(damp=d, weight=None if k is None else members[idx[k]]["weight"], member=None if k is None else idx[k]))
    return out


def tradeoff_members(t):
    """the rows of <input>Tradeoff.dat from lsmr_tradeoff_sweep's result: dicts with the keys TRADEOFF_COLUMNS"""
    nrm = np.sqrt(t["measures"])
    return [dict(weight=float(t["weight"][k]), damp=float(t["damp"][k]), misfit=float(nrm[k, 0]), rough=float(nrm[k, 1]), xnorm=float(nrm[k, 2]),
                 itn=int(t["itn"][k]), istop=int(t["istop"][k]), dv_min=float(t["x"][k].min()), dv_max=float(t["x"][k].max()))
            for k in range(t["weight"].size)]


def tradeoff_nonlinear_rows(weight, damp, predicted, measures, failures, ndata):
    """the rows of <input>TradeoffNonlinear.dat (keys io.TRADEOFF_NONLINEAR_COLUMNS): per member its weight and damp, predicted_rms =
    sqrt(predicted[k] / ndata) from the sweep's linear sum of squared data residuals, weighted_rms and rms = sqrt(sum / ndata) of the true
    sums measures (K, 1, 2) = { sum (w r)^2, sum r^2 }, and its dispersion failures"""
    meas = np.asarray(measures, np.float64).reshape(-1, 2)
    nd = float(ndata)
    return [dict(weight=float(weight[k]), damp=float(damp[k]), predicted_rms=float(np.sqrt(predicted[k] / nd)), weighted_rms=float(np.sqrt(meas[k, 0] / nd)),
                 rms=float(np.sqrt(meas[k, 1] / nd)), disp_failures=int(failures[k])) for k in range(meas.shape[0])]


def tradeoff_nonlinear_select(rows, rough):
    """per damp (in order of first appearance): dict(damp, best = the member (index into rows) with the smallest true weighted rms among
    those with a finite one, ties to the first, None where there is none; weight = its weight; corner / corner_weight = the member and the
    weight lcurve_corner finds on (rough, true weighted rms) over increasing weight, None where it finds none).  rough: ||C x|| per member."""
    out = []
    for d in dict.fromkeys(t["damp"] for t in rows):
        idx = sorted((i for i, t in enumerate(rows) if t["damp"] == d), key=lambda i: rows[i]["weight"])
        ok = [i for i in idx if np.isfinite(rows[i]["weighted_rms"])]
        best = min(ok, key=lambda i: (rows[i]["weighted_rms"], i)) if ok else None
        k = lcurve_corner([rows[i]["weighted_rms"] for i in idx], [rough[i] for i in idx])
        out.append(dict(damp=d, best=best, weight=None if best is None else rows[best]["weight"], corner=None if k is None else idx[k],
                        corner_weight=None if k is None else rows[idx[k]]["weight"]))
    return out


def lsmr_tradeoff_sweep(lib, eng, c, cbst, m, nar, weights, damps, chunk=None):
    """The trade-off sweep of the resident m-row system of nar entries (regularisation rows built with the input file's weight0): the
    members of tradeoff_grid(weights, damps) in chunks of `chunk` (default tradeoff_chunk(m, maxvp, nar, LOCAL_SIZE)), one dsa_lsmr_tradeoff call
    each with the arguments of the pass's dsa_lsmr call.  Returns dict(weight, damp (K,), x=(K, maxvp) raw updates, measures=(K, 3)
    {sum r^2, sum (C x)^2, sum x^2}, itn, istop, est=(K, 5), chunk, calls, seconds)."""
    f = np.float32
    n = c["nparpi"]
    w, d = tradeoff_grid(weights, damps)
    K = w.size
    chunk = int(chunk or tradeoff_chunk(m, n, nar, LOCAL_SIZE))
    x = np.zeros((K, n), f); meas = np.zeros((K, 3))
    istop = np.zeros(K, np.int32); itn = np.zeros(K, np.int32); est = np.zeros((K, 5), f)
    t0 = time.perf_counter()
    for q in chunks(K, chunk):
        wk, dk = np.ascontiguousarray(w[q]), np.ascontiguousarray(d[q])
        call_solver(lib, eng, "dsa_lsmr_tradeoff", wk.size, c["ndata"], _p(cbst), C.c_float(c["weight0"]), _p(wk), _p(dk), *LSMR_ARGS, _p(x[q]), _p(meas[q]),
                    _p(istop[q]), _p(itn[q]), _p(est[q]))
    return dict(weight=w, damp=d, x=x, measures=meas, itn=itn, istop=istop, est=est, chunk=chunk, calls=len(chunks(K, chunk)), seconds=time.perf_counter() - t0)


def check_tradeoff(weights, damps, iteration, host_rows, maxiter=None, chunk=None):
    """the trade-off sweep's preconditions, checked before anything touches the GPU (weights None: no sweep)"""
    if weights is None:
        if damps is not None:
            raise ValueError("--tradeoff-damps needs --tradeoff-weights")
        return
    _check_values(("--tradeoff-weights", weights), ("--tradeoff-damps", damps))
    if host_rows:
        raise ValueError("--tradeoff-weights solves on the device-resident system: it cannot be combined with --host-rows")
    _check_outer("--tradeoff-iter", iteration, maxiter)
    if chunk is not None and (chunk < 64 or chunk % 64):
        raise ValueError("tradeoff_chunk must be a multiple of 64 (got %d)" % chunk)


def check_tradeoff_nonlinear(nonlinear, weights, host_rows):
    """--tradeoff-nonlinear's preconditions, checked before anything touches the GPU"""
    if not nonlinear:
        return
    if weights is None:
        raise ValueError("--tradeoff-nonlinear needs --tradeoff-weights")
    if host_rows:
        raise ValueError("--tradeoff-nonlinear judges the members of the sweep on the device-resident system: it cannot be combined with --host-rows")


OPTIONS = (
    ("--tradeoff-weights", "tradeoff_weights", None, dict(type=arg_type(parse_tradeoff_list), metavar="W1,W2,...",
        help="the trade-off curve of one iteration's step over these smoothing weights (and --tradeoff-damps): <input>Tradeoff.dat, "
             "misfit against roughness per (weight, damp), and the curve's corner per damp in the log")),
    ("--tradeoff-damps", "tradeoff_damps", None, dict(type=arg_type(parse_tradeoff_list), metavar="D1,...",
        help="damps of the trade-off sweep (default: the input file's damp)")),
    ("--tradeoff-iter", "tradeoff_iter", 1, dict(type=int, metavar="N", help="the outer iteration whose step is swept, 1..maxiter (default 1)")),
    (None, "tradeoff_chunk", None, None),
    ("--tradeoff-nonlinear", "tradeoff_nonlinear", False, dict(action="store_true",
        help="with --tradeoff-weights: judge every member of the sweep by the true travel times through the model it would produce "
             "(built and forward-modelled on the device in one call per chunk): <input>TradeoffNonlinear.dat, predicted against true rms "
             "per (weight, damp), and the best member and the corner on the true misfit per damp in the log")),
)


def check(o, host_rows, maxiter, c):
    check_tradeoff_nonlinear(o["tradeoff_nonlinear"], o["tradeoff_weights"], host_rows)
    check_tradeoff(o["tradeoff_weights"], o["tradeoff_damps"], o["tradeoff_iter"], host_rows, maxiter, o["tradeoff_chunk"])


def plan(o, c, it, maxiter):
    if o["tradeoff_weights"] is None or it != o["tradeoff_iter"]:
        return None
    return dict(weights=list(o["tradeoff_weights"]), damps=[float(c["damp"])] if o["tradeoff_damps"] is None else list(o["tradeoff_damps"]),
                chunk=o["tradeoff_chunk"], nonlinear=bool(o["tradeoff_nonlinear"]))


def solve(s, plan, res):
    res["trade"] = lsmr_tradeoff_sweep(s.lib, s.eng, s.c, s.cbst, s.m, s.nar, plan["weights"], plan["damps"], plan.get("chunk"))


def solve_nonlinear(s, plan, res):
    if plan.get("nonlinear"):
        res["trade_nl"] = forward_steps_members(s.lib, s.c, s.vsf, res["trade"]["x"], s.obst, s.datweight, chunk=plan.get("nonlinear_chunk"))


def report(ctx, st, h):
    t, sweep = st["trade"], ctx.plans["tradeoff"]
    members = tradeoff_members(t)
    write_tradeoff(ctx.name + "Tradeoff.dat", members)
    ht = h["tradeoff"] = dict(_solve_stats(t["itn"], t["istop"]), iteration=ctx.it, weights=sweep["weights"], damps=sweep["damps"], chunk=t["chunk"],
                              calls=t["calls"], seconds=t["seconds"], members=members, corners=tradeoff_corners(members))
    ctx.log(" tradeoff: %d weights x %d damps at iteration %d: %s, %d calls of up to %d (%.3f s)" %
            (len(sweep["weights"]), len(sweep["damps"]), ctx.it, _solve_text(ht), ht["calls"], ht["chunk"], ht["seconds"]))
    for cn in ht["corners"]:
        ctx.log(" tradeoff damp %g: corner %s" % (cn["damp"], "not found" if cn["weight"] is None else "at weight %g" % cn["weight"]))


def report_nonlinear(ctx, st, h):
    t, nl = st["trade"], st["trade_nl"]
    rows = tradeoff_nonlinear_rows(t["weight"], t["damp"], t["measures"][:, 0], nl["measures"], nl["failures"], ctx.c["ndata"])
    io.write_tradeoff_nonlinear(ctx.name + "TradeoffNonlinear.dat", rows)
    picks = tradeoff_nonlinear_select(rows, [mb["rough"] for mb in h["tradeoff"]["members"]])
    h["tradeoff_nonlinear"] = dict(iteration=ctx.it, members=rows, picks=picks, calls=nl["calls"], seconds=nl["seconds"], dsyn=nl["dsyn"])
    ctx.log(" tradeoff nonlinear: %d members through %d forward call%s (%.3f s), %d dispersion curves without a root" %
            (len(rows), nl["calls"], "" if nl["calls"] == 1 else "s", nl["seconds"], int(np.sum(nl["failures"]))))
    for pk, cn in zip(picks, h["tradeoff"]["corners"]):
        ctx.log(" tradeoff nonlinear damp %g: smallest true weighted rms %s; corner on the true misfit %s (linear: %s)" %
                (pk["damp"], "none" if pk["best"] is None else "%.6g at weight %g (predicted %.6g)" % (rows[pk["best"]]["weighted_rms"], pk["weight"], rows[pk["best"]]["predicted_rms"]),
                 "not found" if pk["corner"] is None else "at weight %g" % pk["corner_weight"], "not found" if cn["weight"] is None else "at weight %g" % cn["weight"]))
