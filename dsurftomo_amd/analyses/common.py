"""What more than one analysis of the inversion loop uses: the LSMR arguments of every solve, the sizing of the batch solver's calls, the
model-file writers, the statistics of a batch of solves, the true misfit of a sweep's members, and the adapter of the option parsers.

An analysis module (bootstrap, resolution, tradeoff, crossval, voronoi, line_search, azimuthal) holds its host helpers, its device driver and
its check_* function, and describes itself to invert.py by the same few names:
    OPTIONS     its options, once: (flag or None for a keyword-only option, run() keyword = argparse destination, default, argparse arguments)
    check(o, host_rows, maxiter, c)     its check_* on the resolved options o; c is the loaded case, or None before the input is read
    plan(o, c, it, maxiter)             None, or what iteration_device takes under the module's plan keyword in outer iteration `it`
    solve*(s, plan, res)                a stage of the pass: s is the pass's system (iteration_device), the result goes into res
    report*(ctx, st, h)                 the files, the history entry h[...] and the log lines of the pass result st; ctx is run()'s
"""
import argparse
import ctypes as C
import time

import numpy as np

from .. import io

EARTH_KM = 6371.0                # the sphere of the PSF lengths (dsa_lsmr_resolution) and of the Voronoi cells' frame
# atol, btol, conlim, itnlim, localSize of every LSMR solve here (main.f90:470-489); LOCAL_SIZE is what the *_chunk defaults size for
LSMR_ARGS = (1e-6, 1e-6, 100.0, 400, 10)
LOCAL_SIZE = LSMR_ARGS[4]


def arg_type(parse):
    """an argparse type from a parse_* function: its ValueError becomes the ArgumentTypeError that argparse reports with the option's name"""
    def convert(text):
        try:
            return parse(text)
        except ValueError as exc:
            raise argparse.ArgumentTypeError(str(exc))
    return convert


def call_solver(lib, eng, name, *args):
    """one call of the solver entry point `name` on the engine eng; its error text raised"""
    if getattr(lib, name)(eng, *args) != 0:
        raise RuntimeError("%s: %s" % (name, lib.dsa_error_string(eng).decode()))


def forward_rows(lib, c, vsf, iw=None, rw=None, col=None, entry="dsa_calsurfg"):
    """the forward call `entry` (dsa_calsurfg, dsa_calsurfg_azimuthal) on the model vsf; its rows go to the host arrays iw / rw / col, whose
    capacity the drop-in is told, or (all None) stay on the device.  Returns (dsyn, the number of row entries, seconds)."""
    dsyn = np.zeros(c["ndata"], np.float32)
    nar = C.c_int(0)
    head, tail = io._args(dict(c, vels=vsf))
    lib.dsa_dropin_set_capacity(0 if rw is None else rw.size)
    t0 = time.perf_counter()
    if getattr(lib, entry)(*head, _p(iw), _p(rw), _p(col), _p(dsyn), *tail, C.byref(nar)) != 0:
        raise RuntimeError("%s: %s" % (entry, lib.dsa_dropin_error().decode()))
    return dsyn, nar.value, time.perf_counter() - t0


def lsmr(lib, eng, b, damp, n):
    """dsa_lsmr on the system resident on the engine eng, right-hand side b, LSMR_ARGS.  Returns (x (n,) float32, istop, itn, seconds)."""
    x = np.zeros(n, np.float32)
    ii = [C.c_int(0), C.c_int(0)]
    ff = [C.c_float(0) for _ in range(5)]
    t0 = time.perf_counter()
    call_solver(lib, eng, "dsa_lsmr", _p(b), C.c_float(damp), *LSMR_ARGS, _p(x), C.byref(ii[0]), C.byref(ii[1]), *[C.byref(v) for v in ff])
    return x, ii[0].value, ii[1].value, time.perf_counter() - t0


def parse_ints(text, n, usage):
    """'N1,N2,...' -> a tuple of n integers >= 1 (ValueError with `usage` otherwise)"""
    parts = text.split(",")
    try:
        v = tuple(int(p) for p in parts)
    except ValueError:
        v = ()
    if len(parts) != n or len(v) != n or min(v) < 1:
        raise ValueError("%s (got %r)" % (usage, text))
    return v


def chunks(n, chunk):
    """the slices of 0..n in steps of chunk: one per call of a batch driver"""
    return [slice(first, min(first + chunk, n)) for first in range(0, n, chunk)]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _lonlat(c, i, j):
    """longitude and latitude (float32) that the model files print for interior vertex (i + 1, j + 1)"""
    f = np.float32
    return f(c["gozd"] + f(f(j) * c["dvzd"])), f(c["goxd"] - f(f(i) * c["dvxd"]))


def vertices(c):
    """(i, j, k, longitude, latitude) of the interior vertices (i + 1, j + 1, k) in the order of the model files: k, then j, then i"""
    for k in range(c["nz"] - 1):
        for j in range(c["ny"] - 2):
            for i in range(c["nx"] - 2):
                yield (i, j, k) + _lonlat(c, i, j)


def write_model(path, c, vsf, *extra):
    """'(5f10.5)' lines: longitude, latitude, depth, Vs for the interior vertices, k / j / i order (main.f90:539-545); every array
    of `extra` (shaped like vsf) adds one more column in the same format"""
    with open(path, "w") as fh:
        for i, j, k, lon, lat in vertices(c):
            fh.write("%10.5f%10.5f%10.5f" % (lon, lat, c["depz"][k]) + "".join("%10.5f" % e[i + 1, j + 1, k] for e in (vsf,) + extra) + "\n")


def unknowns_grid(c, values):
    """(nx, ny, nz) float64 grid of per-unknown values (maxvp, the order of the LSMR unknowns: i fastest, then j, then k) on the
    interior vertices, 0 elsewhere: what write_model takes"""
    nx, ny, nz = c["nx"], c["ny"], c["nz"]
    v = np.zeros((nx, ny, nz), np.float64)
    v[1:-1, 1:-1, :-1] = np.asarray(values, np.float64).reshape(nz - 1, ny - 2, nx - 2).transpose(2, 1, 0)
    return v


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


def batch_bytes(m, n, local_size, nreal):
    """device bytes of dsa_lsmr_batch's buffers for nreal realisations on an m x n system (lsmr_batch.hip: u and the row scales of m
    floats, v h hbar x of n, the local-V queue of n per vector, the norms' terms of max(m, n), block maxima, parameters, and the
    temporary of max(nreal m + m, nreal n)), all in groups of 64 realisations"""
    Rp = 64 * ((nreal + 63) // 64)
    L = max(0, min(local_size, m, n))
    mx = max(m, n)
    floats = Rp * (2 * m + (4 + L) * n + mx + -(-mx // 256) + 15) + max(nreal * m + m, nreal * n)
    return 4 * floats


def _fit(k, step, bytes_of, budget):
    """k lowered in steps of `step` until bytes_of(k) fits `budget` (step at the least)"""
    while k > step and bytes_of(k) > budget:
        k -= step
    return k


def _check_values(*options):
    """every (option name, value list or None) given: at least one value, every one finite and >= 0"""
    for name, vals in options:
        if vals is None:
            continue
        vals = list(vals)
        if not vals or not all(np.isfinite(v) and v >= 0 for v in vals):
            raise ValueError("%s takes at least one value, every one finite and >= 0 (got %r)" % (name, vals))


def _check_outer(name, iteration, maxiter):
    """the outer iteration an option names lies in 1..maxiter"""
    if iteration < 1 or (maxiter is not None and iteration > maxiter):
        raise ValueError("%s must be an outer iteration 1..maxiter (got %d%s)" % (name, iteration, "" if maxiter is None else ", maxiter %d" % maxiter))


def _solve_stats(itn, istop):
    stops = {int(k): int(v) for k, v in zip(*np.unique(istop, return_counts=True))}
    return dict(realisations=int(itn.size), itn_min=int(itn.min()), itn_median=float(np.median(itn)), itn_max=int(itn.max()), istop=stops)


def _solve_text(h):
    return "%d realisations, itn min/median/max %d/%g/%d, istop %s" % (h["realisations"], h["itn_min"], h["itn_median"], h["itn_max"],
                                                                     " ".join("%d:%d" % kv for kv in sorted(h["istop"].items())))


def nonlinear_measures(obst, dsyn, datweight, group=None, ngroups=1):
    """the misfit sums of dsa_forward_steps restated in numpy: per row k of dsyn (K, ndata) and group g of data, { sum (double)wr^2, sum
    (double)r^2 } over the data of the group, r = float32(obst - dsyn_k), wr = float32(datweight * r) (datweight None: w = 1), squared and
    summed in float64.  group: (ndata,) ids in [0, ngroups), None = one group; an empty group gives 0.  Returns (K, ngroups, 2) float64."""
    f = np.float32
    obst = np.asarray(obst, f).ravel()
    dsyn = np.asarray(dsyn, f).reshape(-1, obst.size)
    ngroups = int(ngroups)
    if ngroups < 1:
        raise ValueError("ngroups must be at least 1 (got %d)" % ngroups)
    if group is None:
        group = np.zeros(obst.size, np.int64)
    group = np.asarray(group).ravel()
    if group.size != obst.size or (group.size and (group.min() < 0 or group.max() >= ngroups)):
        raise ValueError("group holds one id in [0, %d) per datum" % ngroups)
    out = np.zeros((dsyn.shape[0], ngroups, 2))
    for k, row in enumerate(dsyn):
        r = (obst - row).astype(f)
        wr = r if datweight is None else (np.asarray(datweight, f).ravel() * r).astype(f)
        for g in range(ngroups):
            sel = group == g
            out[k, g, 0] = (wr[sel].astype(np.float64) ** 2).sum()
            out[k, g, 1] = (r[sel].astype(np.float64) ** 2).sum()
    return out


def forward_steps_members(lib, c, vsf, steps, obst, datweight, group=None, ngroups=1, chunk=None, nmembers=None):
    """the true misfit of the members of a sweep: their raw updates `steps` (K, nparpi) through dsa_forward_steps on the model vsf (dicing 8,
    no alpha, the case's minvel / maxvel), `chunk` members per call (default 256); steps None: the nmembers solutions the last batch solve
    left on the drop-in engine, in one call.  Returns dict(measures (K, ngroups, 2), failures (K,), dsyn (K, ndata), calls, resident, seconds)."""
    t0 = time.perf_counter()
    if steps is None:
        r = io.call_forward_steps(c, vsf, int(nmembers), None, 8, obst, datweight, group, ngroups, lib=lib)
        return dict(measures=r["measures"], failures=r["failures"], dsyn=r["dsurf"], calls=1, resident=True, seconds=time.perf_counter() - t0)
    steps = np.asarray(steps, np.float32).reshape(-1, c["nparpi"])
    K = steps.shape[0]
    chunk = int(chunk or 256)
    meas = np.zeros((K, int(ngroups), 2)); fails = np.zeros(K, np.int64); dsyn = np.zeros((K, c["ndata"]), np.float32)
    for q in chunks(K, chunk):
        r = io.call_forward_steps(c, vsf, steps[q], None, 8, obst, datweight, group, ngroups, lib=lib)
        meas[q] = r["measures"]; fails[q] = r["failures"]; dsyn[q] = r["dsurf"]
    return dict(measures=meas, failures=fails, dsyn=dsyn, calls=len(chunks(K, chunk)), resident=False, seconds=time.perf_counter() - t0)
