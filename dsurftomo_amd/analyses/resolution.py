"""--resolution and --checkerboard NX,NY,NZ add linearised resolution tests of the last iteration's step, run by
dsa_lsmr_resolution on the same resident system with the arguments of the dsa_lsmr call (the resolution of the step as it was
run, early stopping included): the right-hand side of a test model m is A m on the data rows and 0 on the regularisation rows.
--resolution solves for the unit spike of every unknown (its point-spread function, a column of the resolution matrix), in
chunks of resolution_chunk() spikes, and writes <input>Resolution.dat in the layout of <input>Measure.dat with three value
columns: R_jj (the diagonal element), the horizontal and the vertical PSF length sqrt(sum x^2 d^2 / sum x^2) in km (great-circle
distance / depth difference from the spike's vertex); unknowns without data are written as 0 and counted in the log line.  Each
--checkerboard (may be repeated) is a block checkerboard of +-0.1 km/s flipping sign every NX unknowns along the latitude index,
NY along longitude, NZ along depth, first block positive (checkerboard()); all patterns go in one call, <input>Checker.dat.kNN
lists longitude, latitude, depth, input and recovered update, and the log and the history give the Pearson correlation and the
gain <m,x>/<m,m>, whole model and per depth layer.  Device-resident rows only (not with --host-rows); they combine with
--bootstrap.
"""
import ctypes as C
import time

import numpy as np

from .common import EARTH_KM, LOCAL_SIZE, LSMR_ARGS, _fit, _p, _solve_stats, _solve_text, arg_type, batch_bytes, call_solver, chunks, parse_ints, unknown_coords, unknowns_grid, write_model


def great_circle_km(lat, lon, lat0, lon0):
    """haversine distance in km on a sphere of EARTH_KM from (lat0, lon0) (degrees); the formula dsa_lsmr_resolution uses"""
    d2r = np.pi / 180.0
    sp = np.sin((lat - lat0) * d2r * 0.5)
    sl = np.sin((lon - lon0) * d2r * 0.5)
    a = sp * sp + np.cos(lat * d2r) * np.cos(lat0 * d2r) * sl * sl
    return 2.0 * EARTH_KM * np.arcsin(np.minimum(1.0, np.sqrt(a)))


def checkerboard(c, cell, amplitude=0.1):
    """(maxvp,) float32 block checkerboard of +-amplitude over the unknowns: the sign flips every cell[0] unknowns along the latitude
    index i, cell[1] along the longitude index j, cell[2] along depth k; the first block is positive"""
    ni, nj, nk = c["nx"] - 2, c["ny"] - 2, c["nz"] - 1
    cx, cy, cz = cell
    par = (np.arange(nk)[:, None, None] // cz) + (np.arange(nj)[None, :, None] // cy) + (np.arange(ni)[None, None, :] // cx)
    return np.where(par % 2 == 0, np.float32(amplitude), np.float32(-amplitude)).astype(np.float32).ravel()


def parse_checkerboard(text):
    """'NX,NY,NZ' -> (NX, NY, NZ), three integers >= 1 (ValueError otherwise)"""
    return parse_ints(text, 3, "--checkerboard takes NX,NY,NZ: three integers >= 1")


def resolution_chunk(m, n, local_size, budget=32 << 30, cap=4096):
    """spikes per dsa_lsmr_resolution call on an m x n system: cap, lowered in multiples of 64 until batch_bytes fits `budget`
    (64 at the least)"""
    return _fit(cap, 64, lambda k: batch_bytes(m, n, local_size, k), budget)


def psf_columns(psf):
    """(R_jj, horizontal PSF length, vertical PSF length, unknowns without data) from dsa_lsmr_resolution's measures (maxvp, 4):
    lengths sqrt(sum x^2 dh^2 / sum x^2), sqrt(sum x^2 dz^2 / sum x^2) in km; an unknown with sum x^2 = 0 gets zeros"""
    psf = np.asarray(psf, np.float64).reshape(-1, 4)
    s = psf[:, 1]
    has = s > 0
    lh = np.zeros(len(psf))
    lv = np.zeros(len(psf))
    lh[has] = np.sqrt(psf[has, 2] / s[has])
    lv[has] = np.sqrt(psf[has, 3] / s[has])
    return np.where(has, psf[:, 0], 0.0), lh, lv, int((~has).sum())


def recovery_metrics(model, x, nlayers):
    """Pearson correlation and gain <m,x>/<m,m> (float64) of the recovered x against the input model, over the whole model and per
    depth layer (the unknowns in nlayers equal consecutive slices); 0 where a variance or <m,m> is 0"""
    m = np.asarray(model, np.float64).ravel()
    x = np.asarray(x, np.float64).ravel()

    def one(a, b):
        da, db = a - a.mean(), b - b.mean()
        den = np.sqrt((da * da).sum() * (db * db).sum())
        mm = (a * a).sum()
        return (float((da * db).sum() / den) if den > 0 else 0.0), (float((a * b).sum() / mm) if mm > 0 else 0.0)

    corr, gain = one(m, x)
    layers = [one(a, b) for a, b in zip(m.reshape(nlayers, -1), x.reshape(nlayers, -1))]
    return dict(corr=corr, gain=gain, corr_layers=[v[0] for v in layers], gain_layers=[v[1] for v in layers])


def _lsmr_resolution(lib, eng, c, nreal, istop, itn, models=None, first=0, coords=None, x=None, psf=None):
    """one dsa_lsmr_resolution call with the arguments of the pass's dsa_lsmr call; istop / itn / x / psf filled in place"""
    est = np.zeros((nreal, 5), np.float32)
    call_solver(lib, eng, "dsa_lsmr_resolution", nreal, c["ndata"], _p(models), first, _p(coords), C.c_float(c["damp"]), *LSMR_ARGS, _p(x), _p(psf), _p(istop), _p(itn), _p(est))


def resolution_psf(lib, eng, c, m, chunk=None):
    """The point-spread function of every unknown of the resident m-row system: spikes in chunks of `chunk` (default
    resolution_chunk(m, maxvp, LOCAL_SIZE)), one dsa_lsmr_resolution call each, x left on the device, only the PSF measures returned.
    Returns dict(psf=(maxvp, 4) {R_jj, sum x^2, sum x^2 dh^2, sum x^2 dz^2}, itn, istop, chunk, calls, seconds)."""
    n = c["nparpi"]
    chunk = int(chunk or resolution_chunk(m, n, LOCAL_SIZE))
    coords = np.ascontiguousarray(unknown_coords(c))
    psf = np.zeros((n, 4))
    istop = np.zeros(n, np.int32); itn = np.zeros(n, np.int32)
    t0 = time.perf_counter()
    for q in chunks(n, chunk):
        _lsmr_resolution(lib, eng, c, q.stop - q.start, istop[q], itn[q], first=q.start, coords=coords, psf=psf[q])
    return dict(psf=psf, itn=itn, istop=istop, chunk=chunk, calls=len(chunks(n, chunk)), seconds=time.perf_counter() - t0)


def checkerboard_tests(lib, eng, c, cells):
    """One dsa_lsmr_resolution call with a checkerboard() per cell as host models, the recovered updates returned.  Returns
    dict(models=(K, maxvp), x=(K, maxvp), itn, istop, metrics=[recovery_metrics per pattern], seconds)."""
    models = np.ascontiguousarray(np.stack([checkerboard(c, cell) for cell in cells]))
    K, n = models.shape
    x = np.zeros((K, n), np.float32)
    istop = np.zeros(K, np.int32); itn = np.zeros(K, np.int32)
    t0 = time.perf_counter()
    _lsmr_resolution(lib, eng, c, K, istop, itn, models=models, x=x)
    seconds = time.perf_counter() - t0
    metrics = [recovery_metrics(models[k], x[k], c["nz"] - 1) for k in range(K)]
    return dict(models=models, x=x, itn=itn, istop=istop, metrics=metrics, seconds=seconds)


def check_resolution(resolution, checkerboards, host_rows, chunk=None):
    """the resolution tests' preconditions, checked before anything touches the GPU"""
    for cell in checkerboards or ():
        if len(cell) != 3 or any(int(v) != v or v < 1 for v in cell):
            raise ValueError("a checkerboard cell is NX,NY,NZ: three integers >= 1 (got %r)" % (cell,))
    if (resolution or checkerboards) and host_rows:
        raise ValueError("--resolution / --checkerboard solve on the device-resident system: they cannot be combined with --host-rows")
    if chunk is not None and chunk < 1:
        raise ValueError("resolution_chunk must be at least 1 (got %d)" % chunk)


OPTIONS = (
    ("--resolution", "resolution", False, dict(action="store_true",
        help="the point-spread function of every unknown of the last iteration's step: <input>Resolution.dat (R_jj, horizontal and "
             "vertical PSF length in km)")),
    ("--checkerboard", "checkerboard", (), dict(type=arg_type(parse_checkerboard), action="append", default=[], metavar="NX,NY,NZ",   # (argparse appends to its own list)
        help="a +-0.1 km/s block checkerboard through the last iteration's step (may be repeated): <input>Checker.dat.kNN and "
             "its recovery in the log")),
    (None, "resolution_chunk", None, None),
)


def check(o, host_rows, maxiter, c):
    check_resolution(o["resolution"], o["checkerboard"], host_rows, o["resolution_chunk"])


def plan(o, c, it, maxiter):
    cells = [tuple(int(v) for v in cell) for cell in o["checkerboard"] or ()]
    return dict(psf=o["resolution"], chunk=o["resolution_chunk"], cells=cells) if (o["resolution"] or cells) and it == maxiter else None


def solve_psf(s, plan, res):
    if plan.get("psf"):
        res.setdefault("res", {})["psf"] = resolution_psf(s.lib, s.eng, s.c, s.m, plan.get("chunk"))


def solve_checkerboards(s, plan, res):
    if plan.get("cells"):
        res.setdefault("res", {})["checker"] = checkerboard_tests(s.lib, s.eng, s.c, plan["cells"])


def report_psf(ctx, st, h):
    p = st["res"].get("psf")
    if not p:
        return
    rjj, lh, lv, nodata = psf_columns(p["psf"])
    write_model(ctx.name + "Resolution.dat", ctx.c, unknowns_grid(ctx.c, rjj), unknowns_grid(ctx.c, lh), unknowns_grid(ctx.c, lv))
    hr = h["resolution"] = dict(_solve_stats(p["itn"], p["istop"]), no_data=nodata, chunk=p["chunk"], calls=p["calls"],
                                rjj_max=float(rjj.max()), rjj_mean=float(rjj.mean()), seconds=p["seconds"])
    ctx.log(" resolution: %s, %d unknowns without data, R_jj max %.5f mean %.5f, %d calls of up to %d (%.3f s)" %
            (_solve_text(hr), nodata, hr["rjj_max"], hr["rjj_mean"], hr["calls"], hr["chunk"], hr["seconds"]))


def report_checkerboards(ctx, st, h):
    k = st["res"].get("checker")
    if not k:
        return
    hc = h["checkerboard"] = dict(_solve_stats(k["itn"], k["istop"]), seconds=k["seconds"], patterns=[])
    ctx.log(" checkerboard: %s (%.3f s)" % (_solve_text(hc), hc["seconds"]))
    for q, (cell, mt) in enumerate(zip(ctx.plans["resolution"]["cells"], k["metrics"])):
        write_model(ctx.name + "Checker.dat.k%02d" % (q + 1), ctx.c, unknowns_grid(ctx.c, k["models"][q]), unknowns_grid(ctx.c, k["x"][q]))
        hc["patterns"].append(dict(cell=cell, **mt))
        ctx.log(" checkerboard k%02d %d,%d,%d: correlation %.3f gain %.3f; by layer correlation %s gain %s" %
                ((q + 1,) + cell + (mt["corr"], mt["gain"], " ".join("%.2f" % v for v in mt["corr_layers"]), " ".join("%.2f" % v for v in mt["gain_layers"]))))
