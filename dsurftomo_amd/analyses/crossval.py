"""--crossval NFOLDS (>= 2) with --crossval-weights adds the K-fold cross-validation of one outer iteration's linearised step (--crossval-iter N,
default 1), the objective counterpart of the trade-off curve's corner: the data are dealt into NFOLDS folds (crossval_folds: --crossval-by datum
at random, or path, all data of one station pair in one fold; --crossval-seed), and after that iteration's dsa_lsmr, dsa_lsmr_crossval solves,
for every (weight, damp) pair of the grid weights x damps (--crossval-damps, default the input file's damp; weight-major), the system without
each fold in turn and the full system -- NFOLDS + 1 members per pair, all on the resident matrix: a held-out row is a row scaled by 0, which
gives LSMR what deleting the row gives, bit for bit.  <input>Crossval.dat lists per pair: weight, damp, the held-out rms cv_rms, the standard
error cv_se of its square, the training rms, the full fit's ||r||, ||C x||, ||x|| and the smallest and largest itn (crossval_members); the log
and the history name the pair of the smallest cv_rms (best) and the smoothest pair within one standard error of it (one_se, crossval_select);
<input>CrossvalResiduals.dat lists, for the one_se pair, every datum's held-out and full-fit residual.  The calls hold whole pairs
(crossval_chunk).  The inversion itself runs on with the input file's parameters: no other output changes.  Device-resident rows only (not with
--host-rows); combines with the other analysis flags.

--crossval-nonlinear judges the members by the true travel times, as --tradeoff-nonlinear does those of the trade-off sweep.  The
cross-validation passes the fold of every datum as its group:
<input>CrossvalNonlinear.dat lists per pair: weight, damp, the true held-out rms (over the folds f, group f's weighted sum of the member that
held f out, divided by ndata), the true full-fit rms of the full member, the linear cv_rms and the dispersion failures summed over the pair's
members; the log names the pair with the smallest true held-out rms.  Where one dsa_lsmr_crossval call holds all pairs and no other batch
solve follows it, the members' updates never leave the device (dsa_forward_steps with steps = NULL).
"""
import ctypes as C
import time

import numpy as np

from .. import io
from .common import LOCAL_SIZE, LSMR_ARGS, _check_outer, _check_values, _fit, _p, _solve_stats, _solve_text, arg_type, call_solver, chunks, forward_steps_members
from .tradeoff import parse_tradeoff_list, tradeoff_bytes, tradeoff_grid


def datum_table(c):
    """per datum, in the data order of dsurf (period slot, then source, then receiver: CalSurfG's loops): (slot (ndata,) int32 0-based
    period slot, src (ndata, 2) and rec (ndata, 2) uint32: the float32 bits of the source's and the receiver's two coordinates)"""
    slot, src, rec = [], [], []
    for k in range(c["kmax"]):
        for s in range(int(c["nsrcsurf1"][k])):
            nr = int(c["nrc1"][s, k])
            slot.append(np.full(nr, k, np.int32))
            one = np.array([c["scxf"][s, k], c["sczf"][s, k]], np.float32).view(np.uint32)
            src.append(np.broadcast_to(one, (nr, 2)))
            rec.append(np.stack([np.asarray(c["rcxf"][:nr, s, k], np.float32), np.asarray(c["rczf"][:nr, s, k], np.float32)], axis=1).view(np.uint32))
    cat = lambda parts, shape: np.concatenate(parts) if parts else np.zeros(shape, np.uint32)
    return (np.concatenate(slot) if slot else np.zeros(0, np.int32)), cat(src, (0, 2)), cat(rec, (0, 2))


def crossval_folds(c, nfolds, by="datum", seed=1):
    """(ndata,) int32 fold of every datum, each in [0, nfolds).  by 'datum': default_rng(seed).permutation(ndata) % nfolds (sizes differ by
    at most 1).  by 'path': the data of one unordered station pair -- across all periods and wave types -- share a fold: stations are told
    apart by the float32 bits of their coordinates (datum_table), the distinct pairs (in sorted order) are shuffled by
    default_rng(seed).permutation and dealt round-robin.  A pair's dispersion curve is strongly correlated along period, so holding out
    single data of it flatters the fit: 'path' is the honest hold-out for surface-wave data."""
    nfolds = int(nfolds)
    if nfolds < 1:
        raise ValueError("nfolds must be at least 1 (got %d)" % nfolds)
    nd = int(c["ndata"])
    rng = np.random.default_rng(seed)
    if by == "datum":
        return (rng.permutation(nd) % nfolds).astype(np.int32)
    if by != "path":
        raise ValueError("folds are made by 'datum' or by 'path' (got %r)" % (by,))
    _, src, rec = datum_table(c)
    a = (src[:, 0].astype(np.uint64) << np.uint64(32)) | src[:, 1].astype(np.uint64)
    b = (rec[:, 0].astype(np.uint64) << np.uint64(32)) | rec[:, 1].astype(np.uint64)
    pairs = np.stack([np.minimum(a, b), np.maximum(a, b)], axis=1)
    uniq, inverse = np.unique(pairs, axis=0, return_inverse=True)
    of_pair = np.zeros(len(uniq), np.int32)
    of_pair[rng.permutation(len(uniq))] = np.arange(len(uniq)) % nfolds
    return of_pair[np.asarray(inverse).ravel()].astype(np.int32)


CROSSVAL_TABLE = (False, (("weight", "%.9g", "f32"), ("damp", "%.9g", "f32")) + tuple((n, "%.17g", "f64") for n in ("cv_rms", "cv_se", "train_rms", "misfit", "rough", "xnorm")) +
                  (("itn_min", "%d", "int"), ("itn_max", "%d", "int")))
CROSSVAL_COLUMNS = io.column_names(CROSSVAL_TABLE)


def write_crossval(path, members):
    """one line per combo: weight damp cv_rms cv_se train_rms ||r|| ||C x|| ||x|| itn_min itn_max (the last five of the full member / over
    the combo's members), no header line (io.write_table with CROSSVAL_TABLE); the float32 values with 9 significant digits, the float64 ones
    with 17: read_crossval gives the same values back"""
    io.write_table(path, CROSSVAL_TABLE, members)


def read_crossval(path):
    """the members of a file of write_crossval: a list of dicts with the keys CROSSVAL_COLUMNS"""
    return io.read_table(path, CROSSVAL_TABLE)


def crossval_members(result, fold):
    """one dict per combo (keys CROSSVAL_COLUMNS) from a cross-validation result (weight, damp (ncombo,), nfolds, measures (K, 4), itn) and
    the fold of every datum.  With held_f / kept_f the held-out / kept sum of squares of the member that holds out fold f and cnt_f the
    fold's size: cv_rms = sqrt(sum_f held_f / sum_f cnt_f); cv_se = the sample standard deviation (ddof 1) over the non-empty folds of
    held_f / cnt_f, divided by sqrt(their number) (0 with fewer than two), the standard error of cv_rms^2; train_rms = sqrt(sum_f kept_f /
    sum_f (ndata - cnt_f)); misfit, rough, xnorm = the full member's ||r||, ||C x||, ||x||; itn_min / itn_max over the combo's members"""
    fold = np.asarray(fold).ravel()
    nf = int(result["nfolds"])
    S = nf + 1
    cnt = np.bincount(fold, minlength=nf).astype(np.float64)
    meas = np.asarray(result["measures"], np.float64).reshape(-1, S, 4)
    itn = np.asarray(result["itn"]).reshape(-1, S)
    used = cnt > 0
    out = []
    for q in range(meas.shape[0]):
        held, kept = meas[q, :nf, 1], meas[q, :nf, 0]
        per = held[used] / cnt[used]
        se = float(per.std(ddof=1) / np.sqrt(per.size)) if per.size > 1 else 0.0
        ntrain = float((fold.size - cnt).sum())
        out.append(dict(weight=float(result["weight"][q]), damp=float(result["damp"][q]), cv_rms=float(np.sqrt(held.sum() / cnt.sum())), cv_se=se,
                        train_rms=float(np.sqrt(kept.sum() / ntrain)) if ntrain > 0 else 0.0, misfit=float(np.sqrt(meas[q, nf, 0])),
                        rough=float(np.sqrt(meas[q, nf, 2])), xnorm=float(np.sqrt(meas[q, nf, 3])), itn_min=int(itn[q].min()), itn_max=int(itn[q].max())))
    return out


def crossval_select(members):
    """dict(best, one_se): indices into members.  best: the smallest cv_rms^2, ties to the larger weight, then the larger damp.  one_se
    (the one-standard-error rule): among the combos whose cv_rms^2 is at most best's cv_rms^2 + best's cv_se, the largest weight, then the
    largest damp -- the smoothest model that predicts unseen data as well as the best one, within the noise of the estimate"""
    if not members:
        raise ValueError("no members to select from")
    sq = [t["cv_rms"] ** 2 for t in members]
    best = min(range(len(members)), key=lambda i: (sq[i], -members[i]["weight"], -members[i]["damp"]))
    lim = sq[best] + members[best]["cv_se"]
    one = max((i for i in range(len(members)) if sq[i] <= lim), key=lambda i: (members[i]["weight"], members[i]["damp"]))
    return dict(best=best, one_se=one)


def crossval_bytes(m, n, nar, local_size, ncombo, nfolds, ndata):
    """device bytes of a dsa_lsmr_crossval call for ncombo combos of nfolds folds on an m x n system of nar entries with ndata data rows:
    tradeoff_bytes of its ncombo (nfolds + 1) members, the combos' weights and the folds, one more block partial per 64 rows and one more
    measure per member (fp64, in groups of 64) and the residuals (fp64, 2 ncombo ndata)"""
    nreal = ncombo * (nfolds + 1)
    Rp = 64 * ((nreal + 63) // 64)
    return tradeoff_bytes(m, n, nar, local_size, nreal) + 4 * (ncombo + ndata) + 8 * Rp * (-(-m // 64) + 1) + 16 * ncombo * ndata


def crossval_chunk(m, n, nar, local_size, ncombo, nfolds, ndata, budget=32 << 30, cap=4096):
    """combos per dsa_lsmr_crossval call: a call holds whole combos (its members are a multiple of nfolds + 1, so every datum's held-out
    and full member sit in one call) -- as many as give at most `cap` members, lowered one combo at a time until crossval_bytes fits
    `budget` (1 at the least)"""
    return _fit(max(1, min(int(ncombo), cap // (nfolds + 1))), 1, lambda k: crossval_bytes(m, n, nar, local_size, k, nfolds, ndata), budget)


def write_crossval_residuals(path, slot, dist, fold, datweight, held, full):
    """one line per datum: index (1-based), period slot (1-based), dist (km), fold, datweight, the residual in the member that held the
    datum out and in the full fit -- weighted seconds, as the system holds them (float64, 17 significant digits)"""
    with open(path, "w") as fh:
        for i in range(len(fold)):
            fh.write("%d %d %.9g %d %.9g %.17g %.17g\n" % (i + 1, slot[i] + 1, dist[i], fold[i], datweight[i], held[i], full[i]))


def crossval_by_slot(slot, held, nslots):
    """per period slot the root mean square of the held-out residuals of its data (None for a slot without data)"""
    slot = np.asarray(slot)
    sq = np.asarray(held, np.float64) ** 2
    return [float(np.sqrt(sq[slot == k].mean())) if (slot == k).any() else None for k in range(nslots)]


def crossval_nonlinear_rows(weight, damp, nfolds, measures, failures, cv_rms, ndata):
    """the rows of <input>CrossvalNonlinear.dat (keys io.CROSSVAL_NONLINEAR_COLUMNS) from the true sums measures (ncombo (nfolds + 1), nfolds, 2)
    of the members' models with the fold as group: per pair q, heldout_rms = sqrt(sum_f measures[q S + f, f, 0] / ndata) -- every datum judged
    by the member that never saw it --, full_rms = sqrt(sum_g measures[q S + nfolds, g, 0] / ndata) of the full member, the linear cv_rms,
    and the dispersion failures summed over the pair's S = nfolds + 1 members"""
    nf = int(nfolds)
    S = nf + 1
    meas = np.asarray(measures, np.float64).reshape(-1, S, nf, 2)
    fails = np.asarray(failures).reshape(-1, S)
    nd = float(ndata)
    out = []
    for q in range(meas.shape[0]):
        held = sum(meas[q, f, f, 0] for f in range(nf))
        full = sum(meas[q, nf, g, 0] for g in range(nf))
        out.append(dict(weight=float(weight[q]), damp=float(damp[q]), heldout_rms=float(np.sqrt(held / nd)), full_rms=float(np.sqrt(full / nd)),
                        cv_rms=float(cv_rms[q]), disp_failures=int(fails[q].sum())))
    return out


def crossval_nonlinear_select(rows):
    """index of the pair with the smallest finite true held-out rms (ties to the larger weight, then the larger damp, as crossval_select), or None"""
    ok = [i for i, t in enumerate(rows) if np.isfinite(t["heldout_rms"])]
    return min(ok, key=lambda i: (rows[i]["heldout_rms"], -rows[i]["weight"], -rows[i]["damp"])) if ok else None


def lsmr_crossval_sweep(lib, eng, c, cbst, m, nar, weights, damps, fold, nfolds, chunk=None, want_x=False):
    """K-fold cross-validation on the resident m-row system of nar entries (regularisation rows built with the input file's weight0): the
    combos of tradeoff_grid(weights, damps), each with the nfolds hold-outs of `fold` and its full member, in calls of `chunk` combos
    (default crossval_chunk(...)) with the arguments of the pass's dsa_lsmr call.  A call holds whole combos and returns every datum's
    held-out and full-fit residual, so several calls give what one gives.  Returns dict(weight, damp (ncombo,), nfolds, measures=(K, 4)
    {kept, held-out sum r^2, sum (C x)^2, sum x^2}, resid=(ncombo, 2, ndata), x=(K, maxvp) raw updates or None, itn, istop, est=(K, 5),
    chunk, calls, seconds), K = ncombo (nfolds + 1)."""
    f = np.float32
    n, nd = c["nparpi"], c["ndata"]
    w, d = tradeoff_grid(weights, damps)
    nc, S = w.size, int(nfolds) + 1
    K = nc * S
    fold = np.ascontiguousarray(fold, np.int32)
    chunk = int(chunk or crossval_chunk(m, n, nar, LOCAL_SIZE, nc, int(nfolds), nd))
    x = np.zeros((K, n), f) if want_x else None
    meas = np.zeros((K, 4)); resid = np.zeros((nc, 2, nd))
    istop = np.zeros(K, np.int32); itn = np.zeros(K, np.int32); est = np.zeros((K, 5), f)
    t0 = time.perf_counter()
    for q in chunks(nc, chunk):
        k = slice(q.start * S, q.stop * S)
        wk, dk = np.ascontiguousarray(w[q]), np.ascontiguousarray(d[q])
        call_solver(lib, eng, "dsa_lsmr_crossval", wk.size, int(nfolds), nd, _p(cbst), C.c_float(c["weight0"]), _p(wk), _p(dk), _p(fold), *LSMR_ARGS,
                    _p(x[k]) if want_x else None, _p(meas[k]), _p(resid[q]), _p(istop[k]), _p(itn[k]), _p(est[k]))
    return dict(weight=w, damp=d, nfolds=int(nfolds), measures=meas, resid=resid, x=x, itn=itn, istop=istop, est=est, chunk=chunk, calls=len(chunks(nc, chunk)),
                seconds=time.perf_counter() - t0)


def check_crossval(nfolds, weights=None, damps=None, by="datum", iteration=1, host_rows=False, maxiter=None, chunk=None):
    """the cross-validation's preconditions, checked before anything touches the GPU (nfolds None: no cross-validation)"""
    if nfolds is None:
        if weights is not None or damps is not None:
            raise ValueError("--crossval-weights / --crossval-damps need --crossval")
        return
    if int(nfolds) != nfolds or nfolds < 2:
        raise ValueError("--crossval needs at least 2 folds (got %r)" % (nfolds,))
    if weights is None:
        raise ValueError("--crossval needs --crossval-weights")
    _check_values(("--crossval-weights", weights), ("--crossval-damps", damps))
    if by not in ("datum", "path"):
        raise ValueError("--crossval-by is datum or path (got %r)" % (by,))
    if host_rows:
        raise ValueError("--crossval solves on the device-resident system: it cannot be combined with --host-rows")
    _check_outer("--crossval-iter", iteration, maxiter)
    if chunk is not None and chunk < 1:
        raise ValueError("crossval_chunk must be at least 1 combo (got %d)" % chunk)


def check_crossval_nonlinear(nonlinear, nfolds, host_rows):
    """--crossval-nonlinear's preconditions, checked before anything touches the GPU"""
    if not nonlinear:
        return
    if nfolds is None:
        raise ValueError("--crossval-nonlinear needs --crossval")
    if host_rows:
        raise ValueError("--crossval-nonlinear judges the members of the cross-validation on the device-resident system: it cannot be combined with --host-rows")


OPTIONS = (
    ("--crossval", "crossval", None, dict(type=int, metavar="NFOLDS",
        help="K-fold cross-validation (NFOLDS >= 2) of one iteration's step over --crossval-weights x --crossval-damps: every pair is "
             "solved once per held-out fold and once on all data, side by side on the resident system: <input>Crossval.dat (held-out and "
             "training rms per pair), <input>CrossvalResiduals.dat (per datum, for the one-standard-error pair) and both selections in the log")),
    ("--crossval-weights", "crossval_weights", None, dict(type=arg_type(parse_tradeoff_list), metavar="W1,W2,...", help="smoothing weights of the cross-validation")),
    ("--crossval-damps", "crossval_damps", None, dict(type=arg_type(parse_tradeoff_list), metavar="D1,...",
        help="damps of the cross-validation (default: the input file's damp)")),
    ("--crossval-by", "crossval_by", "datum", dict(choices=("datum", "path"),
        help="how the folds are made: datum deals single data at random; path keeps all data of one station pair, across periods and wave "
             "types, in one fold.  A pair's dispersion curve is strongly correlated along period, so path is the honest hold-out for "
             "surface-wave data (default datum)")),
    ("--crossval-seed", "crossval_seed", 1, dict(type=int, metavar="S", help="seed of the folds (default 1)")),
    ("--crossval-iter", "crossval_iter", 1, dict(type=int, metavar="N", help="the outer iteration whose step is cross-validated, 1..maxiter (default 1)")),
    (None, "crossval_chunk", None, None),
    ("--crossval-nonlinear", "crossval_nonlinear", False, dict(action="store_true",
        help="with --crossval: the same for the cross-validation's members, every datum judged by the model of the member that held its "
             "fold out: <input>CrossvalNonlinear.dat, true held-out and full-fit rms per pair beside the linear cv_rms")),
)


def check(o, host_rows, maxiter, c):
    check_crossval_nonlinear(o["crossval_nonlinear"], o["crossval"], host_rows)
    check_crossval(o["crossval"], o["crossval_weights"], o["crossval_damps"], o["crossval_by"], o["crossval_iter"], host_rows, maxiter, o["crossval_chunk"])


def plan(o, c, it, maxiter):
    if o["crossval"] is None or it != o["crossval_iter"]:
        return None
    return dict(weights=list(o["crossval_weights"]), damps=[float(c["damp"])] if o["crossval_damps"] is None else list(o["crossval_damps"]),
                nfolds=int(o["crossval"]), fold=crossval_folds(c, int(o["crossval"]), o["crossval_by"], o["crossval_seed"]), chunk=o["crossval_chunk"],
                nonlinear=bool(o["crossval_nonlinear"]))


def solve(s, plan, res):
    """the members' updates stay on the device for solve_nonlinear where it asks for them, one call holds all pairs and the pass lets them
    (s.crossval_may_stay)"""
    ncombo = len(plan["weights"]) * len(plan["damps"])
    chunk = int(plan.get("chunk") or crossval_chunk(s.m, s.c["nparpi"], s.nar, LOCAL_SIZE, ncombo, int(plan["nfolds"]), s.c["ndata"]))
    s.crossval_resident = bool(plan.get("nonlinear")) and ncombo <= chunk and s.crossval_may_stay
    res["crossval"] = lsmr_crossval_sweep(s.lib, s.eng, s.c, s.cbst, s.m, s.nar, plan["weights"], plan["damps"], plan["fold"], plan["nfolds"], chunk,
                                          plan.get("want_x", False) or (bool(plan.get("nonlinear")) and not s.crossval_resident))


def solve_nonlinear(s, plan, res):
    if plan.get("nonlinear"):
        cv = res["crossval"]
        res["crossval_nl"] = forward_steps_members(s.lib, s.c, s.vsf, None if s.crossval_resident else cv["x"], s.obst, s.datweight, plan["fold"], cv["nfolds"],
                                                   plan.get("nonlinear_chunk"), cv["weight"].size * (cv["nfolds"] + 1))


def report(ctx, st, h):
    v, cvrun, c = st["crossval"], ctx.plans["crossval"], ctx.c
    fold = cvrun["fold"]
    members = crossval_members(v, fold)
    sel = crossval_select(members)
    write_crossval(ctx.name + "Crossval.dat", members)
    slot = datum_table(c)[0]
    one = sel["one_se"]
    write_crossval_residuals(ctx.name + "CrossvalResiduals.dat", slot, c["dist"], fold, st["datweight"], v["resid"][one, 0], v["resid"][one, 1])
    hx = h["crossval"] = dict(_solve_stats(v["itn"], v["istop"]), iteration=ctx.it, nfolds=cvrun["nfolds"], by=ctx.o["crossval_by"], seed=ctx.o["crossval_seed"],
                              weights=cvrun["weights"], damps=cvrun["damps"], chunk=v["chunk"], calls=v["calls"], seconds=v["seconds"], members=members,
                              best=sel["best"], one_se=sel["one_se"], cv_rms_by_slot=crossval_by_slot(slot, v["resid"][one, 0], c["kmax"]))
    ctx.log(" crossval: %d folds by %s, %d weights x %d damps at iteration %d: %s, %d calls of up to %d combos (%.3f s)" %
            (hx["nfolds"], hx["by"], len(cvrun["weights"]), len(cvrun["damps"]), ctx.it, _solve_text(hx), hx["calls"], hx["chunk"], hx["seconds"]))
    for tag, i in (("best", sel["best"]), ("one-SE", sel["one_se"])):
        t = members[i]
        ctx.log(" crossval %s: weight %g damp %g, held-out rms %.6g (se of its square %.3g), training rms %.6g" %
                (tag, t["weight"], t["damp"], t["cv_rms"], t["cv_se"], t["train_rms"]))


def report_nonlinear(ctx, st, h):
    v, nl = st["crossval"], st["crossval_nl"]
    rows = crossval_nonlinear_rows(v["weight"], v["damp"], v["nfolds"], nl["measures"], nl["failures"], [mb["cv_rms"] for mb in h["crossval"]["members"]], ctx.c["ndata"])
    io.write_crossval_nonlinear(ctx.name + "CrossvalNonlinear.dat", rows)
    best = crossval_nonlinear_select(rows)
    h["crossval_nonlinear"] = dict(iteration=ctx.it, members=rows, best=best, calls=nl["calls"], resident=nl["resident"], seconds=nl["seconds"], dsyn=nl["dsyn"])
    ctx.log(" crossval nonlinear: %d members through %d forward call%s (%.3f s; updates %s), %d dispersion curves without a root" %
            (len(nl["failures"]), nl["calls"], "" if nl["calls"] == 1 else "s", nl["seconds"], "resident on the device" if nl["resident"] else "from the host",
             int(np.sum(nl["failures"]))))
    if best is not None:
        t = rows[best]
        ctx.log(" crossval nonlinear best: weight %g damp %g, true held-out rms %.6g (linear %.6g), true full-fit rms %.6g" %
                (t["weight"], t["damp"], t["heldout_rms"], t["cv_rms"], t["full_rms"]))
