"""--line-search A1,A2,... (finite, each >= 0; duplicates dropped, order kept) adds a step-length line search on the TRUE travel-time misfit to
every outer iteration -- the reference applies every LSMR step at full length and never checks it.  After dsa_lsmr, candidate k is the model
updated by dsa_model_update with float32(Ak) * dv (line_search_candidates); all candidates are forward-modelled in ONE dsa_forward_models call
(times only) and scored by the rms of the weighted residual with this iteration's weights (line_search_scores: at Ak = 0
the `rms` of the log line, bit for bit).  A candidate with a dispersion curve without a root is not eligible; the smallest score wins, ties to
the first listed (line_search_select); the winner's model is the one the iteration leaves.  <input>LineSearch.dat lists per (iteration,
candidate): iteration, alpha, weighted rms, plain rms, dispersion failures, chosen 0/1 (io.write_line_search / read_line_search).  --line-search 1
writes the model files of a plain run, byte for byte.  Device-resident rows only (not with --host-rows); combines with the analysis flags.
"""
import time

import numpy as np

from .. import io
from .common import _p, arg_type, nonlinear_measures


def parse_line_search(text):
    """'A1,A2,...' -> the step lengths of --line-search: finite values >= 0, duplicates (as float32, which is what scales the update)
    dropped, the order kept"""
    try:
        vals = [float(t) for t in str(text).split(",") if t.strip()]
    except ValueError:
        raise ValueError("--line-search takes comma-separated numbers (got %r)" % (text,))
    if not vals or not all(np.isfinite(v) and v >= 0 for v in vals):
        raise ValueError("--line-search takes at least one step length, every one finite and >= 0 (got %r)" % (text,))
    out = []
    for v in vals:
        if float(np.float32(v)) not in [float(np.float32(u)) for u in out]:
            out.append(v)
    return out


def line_search_candidates(lib, c, vsf, dv, alphas):
    """the candidate models of a step: candidate k is a copy of vsf (nx, ny, nz; Fortran order) updated by dsa_model_update with
    float32(alphas[k]) * dv -- on a copy of dv, which dsa_model_update clips in place.  Host only.  Returns a list of Fortran-ordered arrays."""
    f = np.float32
    out = []
    for a in alphas:
        step = np.ascontiguousarray(f(a) * np.asarray(dv, f), f)
        cand = np.asfortranarray(np.array(vsf, f, copy=True))
        if lib.dsa_model_update(c["nx"], c["ny"], c["nz"], _p(step), _p(cand), c["minvel"], c["maxvel"]) != 0:
            raise RuntimeError("dsa_model_update failed")
        out.append(cand)
    return out


def line_search_scores(obst, dsyn, datweight):
    """per candidate (rows of dsyn): the rms of the weighted residual float32(w_i * r_i), r = obst - dsyn_k in float32, summed in float64 --
    the data term LSMR has just minimised, evaluated as the `rms` of the iteration's log line (so that step 0 reproduces it exactly) --
    and the rms of the plain residual.  Returns (weighted (K,), plain (K,)) float64."""
    sums = nonlinear_measures(obst, dsyn, datweight)[:, 0, :]
    rms = (np.sqrt(sums) / np.sqrt(np.size(obst))).astype(np.float32).astype(np.float64)
    return rms[:, 0].copy(), rms[:, 1].copy()


def line_search_select(scores, failures):
    """index of the winning candidate: the smallest score among the candidates without a dispersion failure (and with a finite score);
    ties go to the candidate listed first.  Raises when no candidate is eligible."""
    best = None
    for k, (sc, nf) in enumerate(zip(scores, failures)):
        if nf != 0 or not np.isfinite(sc):
            continue
        if best is None or sc < scores[best]:
            best = k
    if best is None:
        raise RuntimeError("line search: no candidate is eligible (every one has a dispersion curve without a root or no finite misfit)")
    return best


def line_search_step(lib, c, vsf, dv, obst, datweight, alphas):
    """the step-length line search of one outer iteration: every candidate of line_search_candidates through ONE dsa_forward_models call
    (CalSurfG's grid), scored by line_search_scores, the winner picked by line_search_select.  Returns dict(alphas, weighted_rms, rms,
    failures, chosen, models, dsyn (K, ndata), seconds)."""
    cands = line_search_candidates(lib, c, vsf, dv, alphas)
    t0 = time.perf_counter()
    dsyn, fails = io.call_forward_models(c, cands, 8, lib=lib)
    dt = time.perf_counter() - t0
    wr, pr = line_search_scores(obst, dsyn, datweight)
    k = line_search_select(wr, fails)
    return dict(alphas=[float(a) for a in alphas], weighted_rms=wr, rms=pr, failures=[int(v) for v in fails], chosen=k, models=cands, dsyn=dsyn, seconds=dt)


def check_line_search(alphas, host_rows):
    """the line search's preconditions, checked before anything touches the GPU (alphas None: no line search)"""
    if alphas is None:
        return
    alphas = list(alphas)
    if not alphas or not all(np.isfinite(a) and a >= 0 for a in alphas):
        raise ValueError("--line-search takes at least one step length, every one finite and >= 0 (got %r)" % (alphas,))
    if host_rows:
        raise ValueError("--line-search forward-models its candidates beside the device-resident system: it cannot be combined with --host-rows")


OPTIONS = (
    ("--line-search", "line_search", None, dict(type=arg_type(parse_line_search), metavar="A1,A2,...",
        help="step-length line search: in every outer iteration the update is tried at these fractions of its length (each >= 0; 0 keeps "
             "the model), all candidate models are forward-modelled in one call, and the one with the smallest rms of the weighted "
             "travel-time residual is applied: <input>LineSearch.dat, one row per (iteration, step)")),
)


def check(o, host_rows, maxiter, c):
    check_line_search(o["line_search"], host_rows)


def plan(o, c, it, maxiter):
    return None if o["line_search"] is None else list(o["line_search"])


def report(ctx, st, h):
    """<input>LineSearch.dat holds the rows of every iteration so far: of the history's entries and of this pass's h"""
    ls = st["line_search"]
    k = ls["chosen"]
    hl = h["line_search"] = dict(alphas=ls["alphas"], weighted_rms=[float(v) for v in ls["weighted_rms"]], rms=[float(v) for v in ls["rms"]],
                                 failures=ls["failures"], chosen=k, alpha=ls["alphas"][k], seconds=ls["seconds"])
    io.write_line_search(ctx.name + "LineSearch.dat", [
        dict(iteration=it, alpha=a, weighted_rms=e["weighted_rms"][q], rms=e["rms"][q], disp_failures=e["failures"][q], chosen=int(q == e["chosen"]))
        for it, e in enumerate((p.get("line_search") for p in ctx.history + [h]), 1) if e for q, a in enumerate(e["alphas"])])
    ctx.log(" line search: step %g of %s taken, rms of the weighted residual %s -> %.6g (%d candidates in one forward call, %.3f s)" %
            (hl["alpha"], ",".join("%g" % a for a in hl["alphas"]), " ".join("%.6g" % v for v in ls["weighted_rms"]), ls["weighted_rms"][k],
             len(hl["alphas"]), hl["seconds"]))
