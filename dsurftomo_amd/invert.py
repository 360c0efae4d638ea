"""The reference's inversion loop (main.f90:346-590) driven through this library, without the Fortran host program.

    python -m dsurftomo_amd.invert <directory with DSurfTomo.in, the data file and MOD> [--maxiter N] [--out DIR]
                                   [--bootstrap R [--bootstrap-seed S]] [--resolution] [--checkerboard NX,NY,NZ ...]

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

--bootstrap R (R >= 2) adds what the reference declared and never filled (main.f90:67, :290-291: dvsub, dvstd, dvall): a
standard deviation of the last iteration's velocity update.  The data rows of that iteration's system are resampled with
replacement R times (bootstrap_row_scales: row r of realisation k weighted by sqrt(how often it was drawn)), the R weighted
systems are solved by dsa_lsmr_batch on the matrix dsa_lsmr just used, and <input>Std.dat lists the sample standard deviation
(ddof 1) of the R raw updates per vertex in the layout of <input>Measure.dat.  Device-resident rows only (not with --host-rows).

--resolution and --checkerboard NX,NY,NZ add linearised resolution tests of the last iteration's step, run by
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
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

from . import io
from .engine import load_library

EARTH_KM = 6371.0                # the sphere of the PSF lengths (dsa_lsmr_resolution)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f10(v):
    return "%10.5f" % v


def _lonlat(c, i, j):
    """longitude and latitude (float32) that the model files print for interior vertex (i + 1, j + 1)"""
    f = np.float32
    return f(c["gozd"] + f(f(j) * c["dvzd"])), f(c["goxd"] - f(f(i) * c["dvxd"]))


def write_model(path, c, vsf, *extra):
    """'(5f10.5)' lines: longitude, latitude, depth, Vs for the interior vertices, k / j / i order (main.f90:539-545); every array
    of `extra` (shaped like vsf) adds one more column in the same format"""
    nx, ny, nz = c["nx"], c["ny"], c["nz"]
    with open(path, "w") as fh:
        for k in range(nz - 1):
            for j in range(ny - 2):
                for i in range(nx - 2):
                    lon, lat = _lonlat(c, i, j)
                    fh.write(_f10(lon) + _f10(lat) + _f10(c["depz"][k]) + _f10(vsf[i + 1, j + 1, k]) +
                             "".join(_f10(e[i + 1, j + 1, k]) for e in extra) + "\n")


def unknowns_grid(c, values):
    """(nx, ny, nz) float64 grid of per-unknown values (maxvp, the order of the LSMR unknowns: i fastest, then j, then k) on the
    interior vertices, 0 elsewhere: what write_model takes"""
    nx, ny, nz = c["nx"], c["ny"], c["nz"]
    v = np.zeros((nx, ny, nz), np.float64)
    v[1:-1, 1:-1, :-1] = np.asarray(values, np.float64).reshape(nz - 1, ny - 2, nx - 2).transpose(2, 1, 0)
    return v


def write_std(path, c, std):
    """write_model's layout with the per-parameter values std (maxvp, the order of the LSMR unknowns: i fastest, then j, then k) as
    the fourth column"""
    write_model(path, c, unknowns_grid(c, std))


def unknown_coords(c):
    """(maxvp, 3) float64: latitude, longitude (degrees) and depth (km) of every LSMR unknown, the values its row of a model file
    prints"""
    nx, ny, nz = c["nx"], c["ny"], c["nz"]
    out = np.zeros((nz - 1, ny - 2, nx - 2, 3))
    for j in range(ny - 2):
        for i in range(nx - 2):
            lon, lat = _lonlat(c, i, j)
            out[:, j, i, 0] = lat
            out[:, j, i, 1] = lon
    out[:, :, :, 2] = np.asarray(c["depz"][:nz - 1], np.float64)[:, None, None]
    return out.reshape(-1, 3)


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
    parts = text.split(",")
    try:
        cell = tuple(int(p) for p in parts)
    except ValueError:
        cell = ()
    if len(parts) != 3 or len(cell) != 3 or min(cell) < 1:
        raise ValueError("--checkerboard takes NX,NY,NZ: three integers >= 1 (got %r)" % text)
    return cell


def _checkerboard_arg(text):
    try:
        return parse_checkerboard(text)
    except ValueError as exc:
        raise argparse.ArgumentTypeError(str(exc))


def batch_bytes(m, n, local_size, nreal):
    """device bytes of dsa_lsmr_batch's buffers for nreal realisations on an m x n system (lsmr_batch.hip: u and the row scales of m
    floats, v h hbar x of n, the local-V queue of n per vector, the norms' terms of max(m, n), block maxima, parameters, and the
    temporary of max(nreal m + m, nreal n)), all in groups of 64 realisations"""
    Rp = 64 * ((nreal + 63) // 64)
    L = max(0, min(local_size, m, n))
    mx = max(m, n)
    floats = Rp * (2 * m + (4 + L) * n + mx + -(-mx // 256) + 15) + max(nreal * m + m, nreal * n)
    return 4 * floats


def resolution_chunk(m, n, local_size, budget=32 << 30, cap=4096):
    """spikes per dsa_lsmr_resolution call on an m x n system: cap, lowered in multiples of 64 until batch_bytes fits `budget`
    (64 at the least)"""
    k = cap
    while k > 64 and batch_bytes(m, n, local_size, k) > budget:
        k -= 64
    return k


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


def write_residuals(path, c, dsyn, obst, datweight):
    """list-directed rows: dist, dsyn, obst, dsyn*w, obst*w, w (main.f90:397-403)"""
    np.savetxt(path, np.column_stack([c["dist"], dsyn, obst, dsyn * datweight, obst * datweight, datweight]), fmt="%16.8f")


def iteration_device(lib, c, vsf, obst, log, bootstrap=None, resolution=None):
    """One pass of main.f90:349-535 with the matrix resident on the device from CalSurfG to LSMR: dsa_calsurfg leaves the
    rows there (null rw / iw / col), dsa_iteration_system_device applies weights / appends the regularisation rows / builds
    both orderings in place, dsa_lsmr solves.  Same numbers as iteration() (tests/test_gpu_lsmr.py compares every bit).
    bootstrap = (R, seed): after dsa_lsmr, R row-resampled solves of the same system by dsa_lsmr_batch (returned as "boot").
    resolution = dict(psf=bool, chunk=int or None, cells=[(NX, NY, NZ), ...]): after dsa_lsmr, the resolution tests of the same
    system (returned as "res": "psf" from resolution_psf, "checker" from checkerboard_tests)."""
    f = np.float32
    nx, ny, nz, dall = c["nx"], c["ny"], c["nz"], c["ndata"]
    maxvp = c["nparpi"]
    dsyn = np.zeros(dall, f)
    nar = C.c_int(0)
    cc = dict(c); cc["vels"] = vsf
    head, tail = io._args(cc)
    lib.dsa_dropin_set_capacity(0)
    t0 = time.perf_counter()
    if lib.dsa_calsurfg(*head, None, None, None, _p(dsyn), *tail, C.byref(nar)) != 0:
        raise RuntimeError("dsa_calsurfg: %s" % lib.dsa_dropin_error().decode())
    t_fwd = time.perf_counter() - t0
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
    dv = np.zeros(maxvp, f)
    ii = [C.c_int(0), C.c_int(0)]
    ff = [C.c_float(0) for _ in range(5)]
    t0 = time.perf_counter()
    rc = lib.dsa_lsmr(eng, _p(cbst), C.c_float(c["damp"]), C.c_float(1e-6), C.c_float(1e-6), C.c_float(100.0), 400, 10, _p(dv),
                      C.byref(ii[0]), C.byref(ii[1]), *[C.byref(v) for v in ff])
    if rc != 0:
        raise RuntimeError("dsa_lsmr: %s" % lib.dsa_error_string(eng).decode())
    t_lsmr = time.perf_counter() - t0
    boot = None
    if bootstrap:
        boot = lsmr_bootstrap(lib, eng, c, cbst, m.value, *bootstrap)
    res = None
    if resolution:
        res = {}
        if resolution.get("psf"):
            res["psf"] = resolution_psf(lib, eng, c, m.value, resolution.get("chunk"))
        if resolution.get("cells"):
            res["checker"] = checkerboard_tests(lib, eng, c, resolution["cells"])
    r = cbst[:dall]
    mean = f(r.sum(dtype=f) / f(dall))
    std = f(np.sqrt(f((r * r).sum(dtype=f) / f(dall)) - mean * mean))
    rms = f(np.sqrt((r.astype(np.float64) ** 2).sum()) / np.sqrt(dall))
    dv_raw = (f(dv.min()), f(dv.max()))
    lib.dsa_model_update(nx, ny, nz, _p(dv), _p(vsf), c["minvel"], c["maxvel"])
    out = dict(dsyn=dsyn, datweight=datweight, mean_ms=1e3 * float(mean), std_ms=1e3 * float(std), rms=float(rms), dv_min=float(dv_raw[0]),
               dv_max=float(dv_raw[1]), itn=ii[1].value, istop=ii[0].value, nar=nar2.value, m=m.value, dws=(float(dws[0]), float(dws[1])),
               seconds=dict(forward=t_fwd, glue=t_glue, lsmr=t_lsmr), dv=dv, norm=norm, cbst=cbst)
    if boot is not None:
        out["boot"] = boot
    if res is not None:
        out["res"] = res
    return out


def lsmr_bootstrap(lib, eng, c, cbst, m, nreal, seed):
    """nreal solves of the resident system with bootstrap row scales (dsa_lsmr_batch, the arguments of the dsa_lsmr call above).
    Returns dict(x=(nreal, maxvp) raw updates, std=(maxvp,) float64 sample standard deviation, itn, istop, est=(nreal, 5), seconds)."""
    f = np.float32
    maxvp = c["nparpi"]
    scales = bootstrap_row_scales(c["ndata"], m, nreal, seed)
    x = np.zeros((nreal, maxvp), f)
    istop = np.zeros(nreal, np.int32); itn = np.zeros(nreal, np.int32); est = np.zeros((nreal, 5), f)
    t0 = time.perf_counter()
    rc = lib.dsa_lsmr_batch(eng, nreal, _p(cbst), _p(scales), C.c_float(c["damp"]), C.c_float(1e-6), C.c_float(1e-6), C.c_float(100.0), 400, 10,
                            _p(x), _p(istop), _p(itn), _p(est))
    if rc != 0:
        raise RuntimeError("dsa_lsmr_batch: %s" % lib.dsa_error_string(eng).decode())
    seconds = time.perf_counter() - t0
    return dict(x=x, std=x.astype(np.float64).std(axis=0, ddof=1), itn=itn, istop=istop, est=est, seconds=seconds)


def _lsmr_resolution(lib, eng, c, nreal, istop, itn, models=None, first=0, coords=None, x=None, psf=None):
    """one dsa_lsmr_resolution call with the arguments of the dsa_lsmr call above; istop / itn / x / psf filled in place"""
    est = np.zeros((nreal, 5), np.float32)
    opt = lambda a: None if a is None else _p(a)
    rc = lib.dsa_lsmr_resolution(eng, nreal, c["ndata"], opt(models), first, opt(coords), C.c_float(c["damp"]), C.c_float(1e-6), C.c_float(1e-6),
                                 C.c_float(100.0), 400, 10, opt(x), opt(psf), _p(istop), _p(itn), _p(est))
    if rc != 0:
        raise RuntimeError("dsa_lsmr_resolution: %s" % lib.dsa_error_string(eng).decode())


def resolution_psf(lib, eng, c, m, chunk=None):
    """The point-spread function of every unknown of the resident m-row system: spikes in chunks of `chunk` (default
    resolution_chunk(m, maxvp, 10)), one dsa_lsmr_resolution call each, x left on the device, only the PSF measures returned.
    Returns dict(psf=(maxvp, 4) {R_jj, sum x^2, sum x^2 dh^2, sum x^2 dz^2}, itn, istop, chunk, calls, seconds)."""
    n = c["nparpi"]
    chunk = int(chunk or resolution_chunk(m, n, 10))
    coords = np.ascontiguousarray(unknown_coords(c))
    psf = np.zeros((n, 4))
    istop = np.zeros(n, np.int32); itn = np.zeros(n, np.int32)
    t0 = time.perf_counter()
    calls = 0
    for first in range(0, n, chunk):
        k = min(chunk, n - first)
        _lsmr_resolution(lib, eng, c, k, istop[first:first + k], itn[first:first + k], first=first, coords=coords, psf=psf[first:first + k])
        calls += 1
    return dict(psf=psf, itn=itn, istop=istop, chunk=chunk, calls=calls, seconds=time.perf_counter() - t0)


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


def iteration(lib, c, vsf, obst, log):
    """One pass of main.f90:349-535 on the model vsf (updated in place), the matrix going through host arrays like in the
    reference (dsa_calsurfg -> dsa_iteration_system -> dsa_lsmr_dropin).  Returns the statistics of the pass."""
    f = np.float32
    nx, ny, nz, dall = c["nx"], c["ny"], c["nz"], c["ndata"]
    maxvp = c["nparpi"]
    maxnar = int(f(c["spfra"]) * dall * nx * ny * nz)                                  # main.f90:287
    rw = np.zeros(maxnar, f); col = np.zeros(maxnar, np.int32); iw = np.zeros(2 * maxnar + 1, np.int32)
    dsyn = np.zeros(dall, f)
    nar = C.c_int(0)
    cc = dict(c); cc["vels"] = vsf
    head, tail = io._args(cc)
    lib.dsa_dropin_set_capacity(maxnar)
    t0 = time.perf_counter()
    if lib.dsa_calsurfg(*head, _p(iw), _p(rw), _p(col), _p(dsyn), *tail, C.byref(nar)) != 0:
        raise RuntimeError("dsa_calsurfg: %s" % lib.dsa_dropin_error().decode())
    t_fwd = time.perf_counter() - t0
    cbst = np.zeros(dall + maxvp, f); datweight = np.zeros(dall, f); norm = np.zeros(maxvp, f); dws = np.zeros(2, f)
    m, nar2 = C.c_int(0), C.c_longlong(0)
    t0 = time.perf_counter()
    rc = lib.dsa_iteration_system(nx, ny, nz, dall, nar.value, maxnar, _p(rw), _p(iw), _p(col), _p(obst), _p(dsyn), c["threshold0"], c["weight0"],
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
    rc = lib.dsa_lsmr_dropin(i32(m.value), i32(maxvp), i32(2 * n + 1), i32(n), _p(iw), _p(rw), _p(cbst), f32(c["damp"]), f32(1e-6), f32(1e-6),
                             f32(100.0), i32(400), i32(10), i32(0), _p(dv), C.byref(ii[0]), C.byref(ii[1]), *[C.byref(v) for v in ff])
    if rc != 0:
        raise RuntimeError("dsa_lsmr_dropin: %s" % lib.dsa_dropin_error().decode())
    t_lsmr = time.perf_counter() - t0
    r = cbst[:dall]
    mean = f(r.sum(dtype=f) / f(dall))
    std = f(np.sqrt(f((r * r).sum(dtype=f) / f(dall)) - mean * mean))
    rms = f(np.sqrt((r.astype(np.float64) ** 2).sum()) / np.sqrt(dall))
    dv_raw = (f(dv.min()), f(dv.max()))
    lib.dsa_model_update(nx, ny, nz, _p(dv), _p(vsf), c["minvel"], c["maxvel"])
    return dict(dsyn=dsyn, datweight=datweight, mean_ms=1e3 * float(mean), std_ms=1e3 * float(std), rms=float(rms), dv_min=float(dv_raw[0]),
                dv_max=float(dv_raw[1]), itn=ii[1].value, istop=ii[0].value, nar=n, m=m.value, dws=(float(dws[0]), float(dws[1])),
                seconds=dict(forward=t_fwd, glue=t_glue, lsmr=t_lsmr), dv=dv, norm=norm, cbst=cbst)


def bind(lib):
    lib.dsa_iteration_system.argtypes = [C.c_int] * 4 + [C.c_longlong] * 2 + [C.c_void_p] * 5 + [C.c_float] * 2 + [C.c_void_p] * 6
    lib.dsa_iteration_system_device.argtypes = [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 2 + [C.c_float] * 2 + [C.c_void_p] * 6
    lib.dsa_model_update.argtypes = [C.c_int] * 3 + [C.c_void_p] * 2 + [C.c_float] * 2
    lib.dsa_dropin_engine.restype = C.c_void_p
    lib.dsa_dropin_engine.argtypes = []
    lib.dsa_lsmr.argtypes = [C.c_void_p, C.c_void_p] + [C.c_float] * 4 + [C.c_int] * 2 + [C.c_void_p] * 8
    lib.dsa_lsmr_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p] + [C.c_float] * 4 + [C.c_int] * 2 + [C.c_void_p] * 4
    lib.dsa_lsmr_resolution.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p] + [C.c_float] * 4 + [C.c_int] * 2 + [C.c_void_p] * 5
    lib.dsa_error_string.restype = C.c_char_p
    lib.dsa_error_string.argtypes = [C.c_void_p]
    return lib


def check_bootstrap(bootstrap, host_rows):
    """the bootstrap's preconditions, checked before anything touches the GPU"""
    if bootstrap and bootstrap < 2:
        raise ValueError("--bootstrap needs at least 2 realisations (got %d)" % bootstrap)
    if bootstrap and host_rows:
        raise ValueError("--bootstrap solves on the device-resident system: it cannot be combined with --host-rows")


def check_resolution(resolution, checkerboards, host_rows, chunk=None):
    """the resolution tests' preconditions, checked before anything touches the GPU"""
    for cell in checkerboards or ():
        if len(cell) != 3 or any(int(v) != v or v < 1 for v in cell):
            raise ValueError("a checkerboard cell is NX,NY,NZ: three integers >= 1 (got %r)" % (cell,))
    if (resolution or checkerboards) and host_rows:
        raise ValueError("--resolution / --checkerboard solve on the device-resident system: they cannot be combined with --host-rows")
    if chunk is not None and chunk < 1:
        raise ValueError("resolution_chunk must be at least 1 (got %d)" % chunk)


def _solve_stats(itn, istop):
    stops = {int(k): int(v) for k, v in zip(*np.unique(istop, return_counts=True))}
    return dict(realisations=int(itn.size), itn_min=int(itn.min()), itn_median=float(np.median(itn)), itn_max=int(itn.max()), istop=stops)


def _solve_text(h):
    return "%d realisations, itn min/median/max %d/%g/%d, istop %s" % (h["realisations"], h["itn_min"], h["itn_median"], h["itn_max"],
                                                                     " ".join("%d:%d" % kv for kv in sorted(h["istop"].items())))


def run(directory, maxiter=None, out_dir=".", log=print, seed=1, host_rows=False, bootstrap=0, bootstrap_seed=1, resolution=False, checkerboard=(),
        resolution_chunk=None):
    check_bootstrap(bootstrap, host_rows)
    check_resolution(resolution, checkerboard, host_rows, resolution_chunk)
    cells = [tuple(int(v) for v in cell) for cell in checkerboard or ()]
    lib = bind(load_library())
    c = io.load(directory)
    maxiter = c["maxiter"] if maxiter is None else maxiter
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
    for it in range(1, maxiter + 1):
        if host_rows:
            st = iteration(lib, c, vsf, obst, log)
        else:
            last = it == maxiter
            st = iteration_device(lib, c, vsf, obst, log, (bootstrap, bootstrap_seed) if bootstrap and last else None,
                                  dict(psf=resolution, chunk=resolution_chunk, cells=cells) if (resolution or cells) and last else None)
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
        h = {k: v for k, v in st.items() if k not in ("dsyn", "datweight", "dv", "norm", "cbst", "boot", "res")}
        if "boot" in st:
            b = st["boot"]
            write_std(name + "Std.dat", c, b["std"])
            stops = {int(k): int(v) for k, v in zip(*np.unique(b["istop"], return_counts=True))}
            h["bootstrap"] = dict(realisations=int(b["itn"].size), itn_min=int(b["itn"].min()), itn_median=float(np.median(b["itn"])),
                                  itn_max=int(b["itn"].max()), istop=stops, std_max=float(b["std"].max()), std_mean=float(b["std"].mean()),
                                  seconds=b["seconds"])
            hb = h["bootstrap"]
            log(" bootstrap: %d realisations, itn min/median/max %d/%g/%d, istop %s, std of the update max %.5f mean %.5f km/s (%.3f s)" %
                (hb["realisations"], hb["itn_min"], hb["itn_median"], hb["itn_max"], " ".join("%d:%d" % kv for kv in sorted(stops.items())),
                 hb["std_max"], hb["std_mean"], hb["seconds"]))
        res = st.get("res", {})
        if "psf" in res:
            p = res["psf"]
            rjj, lh, lv, nodata = psf_columns(p["psf"])
            write_model(name + "Resolution.dat", c, unknowns_grid(c, rjj), unknowns_grid(c, lh), unknowns_grid(c, lv))
            hr = h["resolution"] = dict(_solve_stats(p["itn"], p["istop"]), no_data=nodata, chunk=p["chunk"], calls=p["calls"],
                                        rjj_max=float(rjj.max()), rjj_mean=float(rjj.mean()), seconds=p["seconds"])
            log(" resolution: %s, %d unknowns without data, R_jj max %.5f mean %.5f, %d calls of up to %d (%.3f s)" %
                (_solve_text(hr), nodata, hr["rjj_max"], hr["rjj_mean"], hr["calls"], hr["chunk"], hr["seconds"]))
        if "checker" in res:
            k = res["checker"]
            hc = h["checkerboard"] = dict(_solve_stats(k["itn"], k["istop"]), seconds=k["seconds"], patterns=[])
            log(" checkerboard: %s (%.3f s)" % (_solve_text(hc), hc["seconds"]))
            for q, (cell, mt) in enumerate(zip(cells, k["metrics"])):
                write_model(name + "Checker.dat.k%02d" % (q + 1), c, unknowns_grid(c, k["models"][q]), unknowns_grid(c, k["x"][q]))
                hc["patterns"].append(dict(cell=cell, **mt))
                log(" checkerboard k%02d %d,%d,%d: correlation %.3f gain %.3f; by layer correlation %s gain %s" %
                    ((q + 1,) + cell + (mt["corr"], mt["gain"], " ".join("%.2f" % v for v in mt["corr_layers"]),
                                        " ".join("%.2f" % v for v in mt["gain_layers"]))))
        history.append(h)
    if vsftrue is not None:
        write_model(os.path.join(out_dir, "Vs_model.real"), c, vsftrue)
        write_model(name + "Syn.dat", c, vsf)
    else:
        write_model(name + "Measure.dat", c, vsf)
    log("Program finishes successfully")
    return vsf, history


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("directory")
    ap.add_argument("--maxiter", type=int, default=None)
    ap.add_argument("--out", default=".")
    ap.add_argument("--host-rows", action="store_true", help="hand the matrix through host arrays like the reference (default: it stays on the device)")
    ap.add_argument("--bootstrap", type=int, default=0, metavar="R",
                    help="R >= 2 row-resampled solves of the last iteration's system: <input>Std.dat, the standard deviation of the update. "
                         "The R solves run side by side and cost about the same for any R up to a few hundred: below about R = 8 to 16 "
                         "they take about as long as, or longer than, R separate solves (NOTEBOOK.md)")
    ap.add_argument("--bootstrap-seed", type=int, default=1, metavar="S", help="seed of the bootstrap's resampling (default 1)")
    ap.add_argument("--resolution", action="store_true",
                    help="the point-spread function of every unknown of the last iteration's step: <input>Resolution.dat (R_jj, horizontal and "
                         "vertical PSF length in km)")
    ap.add_argument("--checkerboard", type=_checkerboard_arg, action="append", default=[], metavar="NX,NY,NZ",
                    help="a +-0.1 km/s block checkerboard through the last iteration's step (may be repeated): <input>Checker.dat.kNN and "
                         "its recovery in the log")
    args = ap.parse_args(argv)
    try:
        check_bootstrap(args.bootstrap, args.host_rows)
        check_resolution(args.resolution, args.checkerboard, args.host_rows)
    except ValueError as exc:
        ap.error(str(exc))
    os.makedirs(args.out, exist_ok=True)
    run(args.directory, args.maxiter, args.out, host_rows=args.host_rows, bootstrap=args.bootstrap, bootstrap_seed=args.bootstrap_seed,
        resolution=args.resolution, checkerboard=args.checkerboard)
    return 0


if __name__ == "__main__":
    sys.exit(main())
