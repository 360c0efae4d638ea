"""--bootstrap R (R >= 2) adds what the reference declared and never filled (main.f90:67, :290-291: dvsub, dvstd, dvall): a
standard deviation of the last iteration's velocity update.  The data rows of that iteration's system are resampled with
replacement R times (bootstrap_row_scales: row r of realisation k weighted by sqrt(how often it was drawn)), the R weighted
systems are solved by dsa_lsmr_batch on the matrix dsa_lsmr just used, and <input>Std.dat lists the sample standard deviation
(ddof 1) of the R raw updates per vertex in the layout of <input>Measure.dat.  Device-resident rows only (not with --host-rows).
"""
import ctypes as C
import time

import numpy as np

from .common import LSMR_ARGS, _p, _solve_stats, _solve_text, call_solver, unknowns_grid, write_model

OPTIONS = (
    ("--bootstrap", "bootstrap", 0, dict(type=int, metavar="R",
        help="R >= 2 row-resampled solves of the last iteration's system: <input>Std.dat, the standard deviation of the update. "
             "The R solves run side by side and cost about the same for any R up to a few hundred: below about R = 8 to 16 "
             "they take about as long as, or longer than, R separate solves (NOTEBOOK.md)")),
    ("--bootstrap-seed", "bootstrap_seed", 1, dict(type=int, metavar="S", help="seed of the bootstrap's resampling (default 1)")),
)


def bootstrap_row_scales(ndata, m, nreal, seed):
    """(nreal, m) float32 row scales of a bootstrap over the ndata data rows: per realisation ndata draws of a row, uniform with
    replacement (numpy default_rng(seed)), each data row scaled by sqrt(how often it was drawn); the regularisation rows
    (ndata .. m-1) keep 1"""
    rng = np.random.default_rng(seed)
    s = np.ones((nreal, m), np.float32)
    for r in range(nreal):
        cnt = np.bincount(rng.integers(0, ndata, size=ndata), minlength=ndata)
        s[r, :ndata] = np.sqrt(cnt).astype(np.float32)
    return s


def write_std(path, c, std):
    """write_model's layout with the per-parameter values std (maxvp, the order of the LSMR unknowns: i fastest, then j, then k) as
    the fourth column"""
    write_model(path, c, unknowns_grid(c, std))


def lsmr_bootstrap(lib, eng, c, cbst, m, nreal, seed):
    """nreal solves of the resident system with bootstrap row scales (dsa_lsmr_batch, the arguments of the pass's dsa_lsmr call).
    Returns dict(x=(nreal, maxvp) raw updates, std=(maxvp,) float64 sample standard deviation, itn, istop, est=(nreal, 5), seconds)."""
    f = np.float32
    maxvp = c["nparpi"]
    scales = bootstrap_row_scales(c["ndata"], m, nreal, seed)
    x = np.zeros((nreal, maxvp), f)
    istop = np.zeros(nreal, np.int32); itn = np.zeros(nreal, np.int32); est = np.zeros((nreal, 5), f)
    t0 = time.perf_counter()
    call_solver(lib, eng, "dsa_lsmr_batch", nreal, _p(cbst), _p(scales), C.c_float(c["damp"]), *LSMR_ARGS, _p(x), _p(istop), _p(itn), _p(est))
    seconds = time.perf_counter() - t0
    return dict(x=x, std=x.astype(np.float64).std(axis=0, ddof=1), itn=itn, istop=istop, est=est, seconds=seconds)


def check_bootstrap(bootstrap, host_rows):
    """the bootstrap's preconditions, checked before anything touches the GPU"""
    if bootstrap and bootstrap < 2:
        raise ValueError("--bootstrap needs at least 2 realisations (got %d)" % bootstrap)
    if bootstrap and host_rows:
        raise ValueError("--bootstrap solves on the device-resident system: it cannot be combined with --host-rows")


def check(o, host_rows, maxiter, c):
    check_bootstrap(o["bootstrap"], host_rows)


def plan(o, c, it, maxiter):
    return (o["bootstrap"], o["bootstrap_seed"]) if o["bootstrap"] and it == maxiter else None


def solve(s, plan, res):
    res["boot"] = lsmr_bootstrap(s.lib, s.eng, s.c, s.cbst, s.m, *plan)


def report(ctx, st, h):
    b = st["boot"]
    write_std(ctx.name + "Std.dat", ctx.c, b["std"])
    hb = h["bootstrap"] = dict(_solve_stats(b["itn"], b["istop"]), std_max=float(b["std"].max()), std_mean=float(b["std"].mean()), seconds=b["seconds"])
    ctx.log(" bootstrap: %s, std of the update max %.5f mean %.5f km/s (%.3f s)" % (_solve_text(hb), hb["std_max"], hb["std_mean"], hb["seconds"]))
