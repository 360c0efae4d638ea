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

--tradeoff-weights W1,W2,... adds the regularisation trade-off (L-) curve of one outer iteration's linearised step (--tradeoff-iter N,
default 1): after that iteration's dsa_lsmr, dsa_lsmr_tradeoff solves the same resident system once per (weight, damp) pair of the grid
weights x damps (--tradeoff-damps, default the input file's damp; weight-major, tradeoff_grid), member k with the regularisation rows
rebuilt with its weight in place of weight0 and its own damp: what a rerun of this program with those two parameters would solve in that
iteration, bit for bit, without its forward call.  The calls are chunked in multiples of 64 members (tradeoff_chunk).
<input>Tradeoff.dat lists per member: weight, damp, the data misfit ||r||, the roughness ||C x|| (C the integer coefficients of the
regularisation rows: free of the weight), ||x||, itn, istop, min and max of the update; the log and the history add, per damp, the corner
of the curve (lcurve_corner: the largest Menger curvature of (log ||C x||, log ||r||) over increasing weight).  The inversion itself
runs on with the input file's parameters: no other output changes.  Device-resident rows only (not with --host-rows); combines with
--bootstrap / --resolution / --checkerboard.

--voronoi K,NCELLS adds a Poisson-Voronoi subspace ensemble (Fang et al. 2020) of the last iteration's step, after its dsa_lsmr and on the
same resident system: each of K members draws NCELLS of the unknowns as seeds (voronoi_seeds: default_rng(--voronoi-seed + iteration - 1),
without replacement within a member), every unknown joins its nearest seed (voronoi_xyz: a local Cartesian frame in km, the depth axis
stretched by --voronoi-zscale; voronoi_cells restates the assignment), and dsa_lsmr_voronoi solves the data rows projected onto the cells
with the damping --voronoi-damp (default the input file's damp) and no smoothing rows -- the projection is the regularisation.  A member's
update is piecewise constant over its cells; <input>Voronoi.dat lists, in the layout of <input>Std.dat with two value columns, the ensemble
mean and the sample standard deviation of the update per vertex.  The members go in calls of voronoi_chunk() (multiples of 64); one call
returns the statistics from the device, several calls bring the members' updates to the host, which combines them in member order
(voronoi_stats, the same fp64 loop).  --voronoi-update runs the ensemble in every outer iteration and applies float32(mean) as that
iteration's update in place of dsa_lsmr's (which still runs and is logged).  The K solves run side by side: below about K = 8 to 16 they
take as long as, or longer than, K separate solves.  Device-resident rows only (not with --host-rows); combines with
--bootstrap / --resolution / --checkerboard / --tradeoff-*.

--crossval NFOLDS (>= 2) with --crossval-weights adds the K-fold cross-validation of one outer iteration's linearised step (--crossval-iter N,
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

--line-search A1,A2,... (finite, each >= 0; duplicates dropped, order kept) adds a step-length line search on the TRUE travel-time misfit to
every outer iteration -- the reference applies every LSMR step at full length and never checks it.  After dsa_lsmr, candidate k is the model
updated by dsa_model_update with float32(Ak) * dv (line_search_candidates); all candidates are forward-modelled in ONE dsa_forward_models call
(times only) and scored by the rms of the weighted residual with this iteration's weights (line_search_scores: at Ak = 0
the `rms` of the log line, bit for bit).  A candidate with a dispersion curve without a root is not eligible; the smallest score wins, ties to
the first listed (line_search_select); the winner's model is the one the iteration leaves.  <input>LineSearch.dat lists per (iteration,
candidate): iteration, alpha, weighted rms, plain rms, dispersion failures, chosen 0/1 (io.write_line_search / read_line_search).  --line-search 1
writes the model files of a plain run, byte for byte.  Device-resident rows only (not with --host-rows); combines with the analysis flags.

--tradeoff-nonlinear (with --tradeoff-weights) and --crossval-nonlinear (with --crossval) judge the members of those two sweeps by the TRUE
travel times through the models they would produce, not by the linearised residual b - A x alone.  After all linear
analyses of the swept iteration, just before the line search / the model update, every member's raw update goes through dsa_forward_steps
(io.call_forward_steps: dicing 8, no alpha, the input file's minvel / maxvel, this iteration's datweight, in chunks): the member's model --
what a rerun with its (weight, damp) would hold after that iteration -- is built on the device, forward-modelled with the others, and its
misfit sums { sum (w r)^2, sum r^2 } (nonlinear_measures restates them) are reduced there.  <input>TradeoffNonlinear.dat lists per member:
weight, damp, the weighted rms the linear system predicts (sqrt(measures[0] / ndata) of the sweep), the true weighted rms, the true plain rms
(rms = sqrt(sum / ndata)) and its dispersion curves without a root; the log names, per damp, the member with the smallest true weighted rms
and the corner of (roughness, true misfit) beside the linear one.  The cross-validation passes the fold of every datum as its group:
<input>CrossvalNonlinear.dat lists per pair: weight, damp, the true held-out rms (over the folds f, group f's weighted sum of the member that
held f out, divided by ndata), the true full-fit rms of the full member, the linear cv_rms and the dispersion failures summed over the pair's
members; the log names the pair with the smallest true held-out rms.  Where one dsa_lsmr_crossval call holds all pairs and no other batch
solve follows it, the members' updates never leave the device (dsa_forward_steps with steps = NULL).  17 significant digits
(io.read_tradeoff_nonlinear / read_crossval_nonlinear return the numbers bit for bit).  No other output changes.  Device-resident rows only.

--azimuthal adds one joint step for Vs and 2psi azimuthal anisotropy (Liu et al. 2019) after the last outer iteration:
c(psi) = c0 + A1 cos 2psi + A2 sin 2psi with A1 = int (Vs/2)(dc/dVs) gc dz, A2 likewise with gs; the unknowns gc = Gc/L and gs = Gs/L live on
the Vs unknowns' grid.  azimuthal_step calls dsa_calsurfg_azimuthal once on the final model (the rays carry the 2psi weights of every step into
two more blocks of columns, Rayleigh periods only) and assembles the joint system in NumPy (azimuthal_system): the reference's 0/1 data
weights (azimuthal_weights: its percentile rule), rows scaled by them, and its first-difference Laplacian rows once per block -- weight0 on
the Vs block, --azimuthal-weight W (default weight0) on gc and gs -- then dsa_spmv_load and dsa_lsmr with this module's LSMR arguments and
--azimuthal-damp D (default the input file's damp).  <input>Azim.dat lists longitude, latitude, depth, Vs, gc, gs, the strength
50 sqrt(gc^2 + gs^2) in per cent of Vs and the fast axis 0.5 atan2(gs, gc) in degrees clockwise from north (write_azimuthal /
read_azimuthal).  The Vs block of the joint solution is logged (min / max) and NOT applied: every other file is a plain run's, byte for byte.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

from . import io
from .engine import declare_solvers, load_library

EARTH_KM = 6371.0                # the sphere of the PSF lengths (dsa_lsmr_resolution)
# atol, btol, conlim, itnlim, localSize of every LSMR solve here (main.f90:470-489); LOCAL_SIZE is what the *_chunk defaults size for
LSMR_ARGS = (1e-6, 1e-6, 100.0, 400, 10)
LOCAL_SIZE = LSMR_ARGS[4]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


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


def _fit(k, step, bytes_of, budget):
    """k lowered in steps of `step` until bytes_of(k) fits `budget` (step at the least)"""
    while k > step and bytes_of(k) > budget:
        k -= step
    return k


def resolution_chunk(m, n, local_size, budget=32 << 30, cap=4096):
    """spikes per dsa_lsmr_resolution call on an m x n system: cap, lowered in multiples of 64 until batch_bytes fits `budget`
    (64 at the least)"""
    return _fit(cap, 64, lambda k: batch_bytes(m, n, local_size, k), budget)


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


def voronoi_xyz(c, zscale=1.0):
    """(maxvp, 3) float64 points in km of the unknowns (unknown_coords) for the Voronoi assignment: coords_xyz of them"""
    return coords_xyz(unknown_coords(c), zscale)


def coords_xyz(coords, zscale=1.0):
    """(n, 3) float64 points in km from (n, 3) latitude, longitude (degrees) and depth (km), a local Cartesian frame about the mean
    latitude and longitude: x = 6371 (lat - mean lat) pi/180, y = 6371 cos(mean lat) (lon - mean lon) pi/180, z = zscale depth"""
    co = np.asarray(coords, np.float64).reshape(-1, 3)
    d2r = np.pi / 180.0
    lat0, lon0 = co[:, 0].mean(), co[:, 1].mean()
    out = np.empty((co.shape[0], 3))
    out[:, 0] = EARTH_KM * (co[:, 0] - lat0) * d2r
    out[:, 1] = EARTH_KM * np.cos(lat0 * d2r) * (co[:, 1] - lon0) * d2r
    out[:, 2] = float(zscale) * co[:, 2]
    return out


def voronoi_seeds(n, ncells, nreal, seed):
    """(nreal, ncells) int32 seed unknowns (0-based) of nreal tessellations: per member ncells of the n unknowns drawn without
    replacement, members in order from numpy default_rng(seed)"""
    if not 1 <= ncells <= n:
        raise ValueError("ncells must lie in 1..%d (got %d)" % (n, ncells))
    rng = np.random.default_rng(seed)
    return np.stack([rng.choice(n, size=ncells, replace=False) for _ in range(nreal)]).astype(np.int32)


def voronoi_cells(xyz, seeds, block=4096):
    """(nreal, n) int32: cell_k(j), the index s of the seed of member k nearest to unknown j -- the numpy restatement of
    dsa_lsmr_voronoi's assignment: d2 = ((xj-xs)*(xj-xs) + (yj-ys)*(yj-ys)) + (zj-zs)*(zj-zs) in float64 in that association, the
    lowest s on ties (argmin's first minimum)"""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    seeds = np.asarray(seeds).reshape(len(seeds), -1)
    out = np.zeros((seeds.shape[0], xyz.shape[0]), np.int32)
    for k, sd in enumerate(seeds):
        p = xyz[sd]
        for j0 in range(0, xyz.shape[0], block):
            q = xyz[j0:j0 + block]
            dx = q[:, None, 0] - p[None, :, 0]
            dy = q[:, None, 1] - p[None, :, 1]
            dz = q[:, None, 2] - p[None, :, 2]
            out[k, j0:j0 + block] = np.argmin((dx * dx + dy * dy) + dz * dz, axis=1)
    return out


def voronoi_stats(x):
    """(2, n) float64 {mean, sample standard deviation} over the members of x (K, n), dsa_lsmr_voronoi's fixed order: every sum float64
    over k = 0 .. K-1 in order, mean = sum / K, std = sqrt(sum (x - mean)^2 / (K - 1)), 0 for K = 1"""
    x = np.asarray(x)
    K, n = x.shape
    s = np.zeros(n)
    for k in range(K):
        s = s + x[k].astype(np.float64)
    mean = s / float(K)
    ss = np.zeros(n)
    for k in range(K):
        d = x[k].astype(np.float64) - mean
        ss = ss + d * d
    return np.stack([mean, np.sqrt(ss / float(K - 1)) if K > 1 else np.zeros(n)])


def voronoi_bytes(ndata, n, ncells, nnz, local_size, nreal):
    """device bytes of a dsa_lsmr_voronoi call for nreal members of ncells cells on ndata data rows of nnz entries over n unknowns: the
    batch buffers at (ndata, ncells) (batch_bytes, whose temporary bounds the call's nreal ncells + ndata), per member (in groups of 64) the
    expanded temporary and the two cell maps (3 n), u member-major (ndata), the sorted list (nnz) and its cell pointers (ncells + 1); the
    row of every position (nnz), one lane group's sort (keys in and out, positions: 3 x 64 nnz, and as much again for the radix sort's
    own double buffers), the points (fp64, 3 n), the seeds and the statistics (fp64, 2 n: they have no block partials)"""
    Rp = 64 * ((nreal + 63) // 64)
    ints = Rp * (3 * n + ndata + nnz + ncells + 1) + nnz + 6 * 64 * nnz + nreal * ncells
    return batch_bytes(ndata, ncells, local_size, nreal) + 4 * ints + 8 * 5 * n


def voronoi_chunk(ndata, n, ncells, nnz, local_size, budget=32 << 30, cap=4096):
    """members per dsa_lsmr_voronoi call: cap, lowered in multiples of 64 until voronoi_bytes fits `budget` (64 at the least)"""
    return _fit(cap, 64, lambda k: voronoi_bytes(ndata, n, ncells, nnz, local_size, k), budget)


def parse_voronoi(text):
    """'K,NCELLS' -> (K, NCELLS), two integers >= 1 (ValueError otherwise)"""
    parts = text.split(",")
    try:
        v = tuple(int(p) for p in parts)
    except ValueError:
        v = ()
    if len(parts) != 2 or len(v) != 2 or min(v) < 1:
        raise ValueError("--voronoi takes K,NCELLS: two integers >= 1 (got %r)" % text)
    return v


def _voronoi_arg(text):
    try:
        return parse_voronoi(text)
    except ValueError as exc:
        raise argparse.ArgumentTypeError(str(exc))


def write_voronoi(path, c, mean, std):
    """write_model's layout with the per-unknown ensemble mean and standard deviation (maxvp each, the order of the LSMR unknowns) as
    the fourth and fifth columns"""
    write_model(path, c, unknowns_grid(c, mean), unknowns_grid(c, std))


def read_voronoi(path):
    """(mean, std) float64 arrays in the order of the LSMR unknowns from a file of write_voronoi ('(5f10.5)' lines)"""
    rows = []
    with open(path) as fh:
        for line in fh:
            line = line.rstrip("\n")
            if len(line) != 50:
                raise ValueError("%s: a line of %d characters, not 50" % (path, len(line)))
            rows.append((float(line[30:40]), float(line[40:50])))
    a = np.array(rows, np.float64).reshape(-1, 2)
    return a[:, 0].copy(), a[:, 1].copy()


def parse_tradeoff_list(text):
    """'V1,V2,...' -> [V1, V2, ...]: at least one float, every one finite and >= 0 (ValueError otherwise)"""
    try:
        vals = [float(p) for p in text.split(",")]
    except ValueError:
        vals = []
    if not vals or not all(np.isfinite(v) and v >= 0 for v in vals):
        raise ValueError("a trade-off list is V1,V2,...: at least one finite number >= 0 (got %r)" % text)
    return vals


def _tradeoff_arg(text):
    try:
        return parse_tradeoff_list(text)
    except ValueError as exc:
        raise argparse.ArgumentTypeError(str(exc))


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


TRADEOFF_COLUMNS = ("weight", "damp", "misfit", "rough", "xnorm", "itn", "istop", "dv_min", "dv_max")


def write_tradeoff(path, members):
    """one line per member: weight damp ||r|| ||C x|| ||x|| itn istop min(dv) max(dv); the float32 values with 9 significant digits,
    the norms (float64) with 17: read_tradeoff gives the same values back"""
    with open(path, "w") as fh:
        for t in members:
            fh.write("%.9g %.9g %.17g %.17g %.17g %d %d %.9g %.9g\n" % tuple(t[k] for k in TRADEOFF_COLUMNS))


def read_tradeoff(path):
    """the members of a file of write_tradeoff: a list of dicts with the keys TRADEOFF_COLUMNS (weight, damp and the update's extremes
    are float32 values, the norms float64)"""
    out = []
    with open(path) as fh:
        for line in fh:
            v = line.split()
            if len(v) != len(TRADEOFF_COLUMNS):
                raise ValueError("%s: a line of %d columns, not %d" % (path, len(v), len(TRADEOFF_COLUMNS)))
            kind = lambda k: int if k in ("itn", "istop") else float if k in ("misfit", "rough", "xnorm") else lambda t: float(np.float32(t))
            out.append({k: kind(k)(t) for k, t in zip(TRADEOFF_COLUMNS, v)})
    return out


def tradeoff_corners(members):
    """per damp (in order of first appearance) the corner of its curve over increasing weight: [dict(damp, weight, member)], weight and
    member (index into members) None where lcurve_corner finds none"""
    out = []
    for d in dict.fromkeys(t["damp"] for t in members):
        idx = sorted((i for i, t in enumerate(members) if t["damp"] == d), key=lambda i: members[i]["weight"])
        k = lcurve_corner([members[i]["misfit"] for i in idx], [members[i]["rough"] for i in idx])
        out.append(dict(damp=d, weight=None if k is None else members[idx[k]]["weight"], member=None if k is None else idx[k]))
    return out


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


CROSSVAL_COLUMNS = ("weight", "damp", "cv_rms", "cv_se", "train_rms", "misfit", "rough", "xnorm", "itn_min", "itn_max")


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


def write_crossval(path, members):
    """one line per combo: weight damp cv_rms cv_se train_rms ||r|| ||C x|| ||x|| itn_min itn_max (the last five of the full member / over
    the combo's members); the float32 values with 9 significant digits, the float64 ones with 17: read_crossval gives the same values back"""
    with open(path, "w") as fh:
        for t in members:
            fh.write("%.9g %.9g %.17g %.17g %.17g %.17g %.17g %.17g %d %d\n" % tuple(t[k] for k in CROSSVAL_COLUMNS))


def read_crossval(path):
    """the members of a file of write_crossval: a list of dicts with the keys CROSSVAL_COLUMNS"""
    out = []
    with open(path) as fh:
        for line in fh:
            v = line.split()
            if len(v) != len(CROSSVAL_COLUMNS):
                raise ValueError("%s: a line of %d columns, not %d" % (path, len(v), len(CROSSVAL_COLUMNS)))
            kind = lambda k: int if k in ("itn_min", "itn_max") else (lambda t: float(np.float32(t))) if k in ("weight", "damp") else float
            out.append({k: kind(k)(t) for k, t in zip(CROSSVAL_COLUMNS, v)})
    return out


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


def _line_search_arg(text):
    try:
        return parse_line_search(text)
    except ValueError as exc:
        raise argparse.ArgumentTypeError(str(exc))


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
    f = np.float32
    obst = np.asarray(obst, f); w = np.asarray(datweight, f)
    dsyn = np.asarray(dsyn, f).reshape(-1, obst.size)
    dall = obst.size
    wr, pr = [], []
    for row in dsyn:
        r = (obst - row).astype(f)
        wr.append(float(f(np.sqrt(((w * r).astype(f).astype(np.float64) ** 2).sum()) / np.sqrt(dall))))
        pr.append(float(f(np.sqrt((r.astype(np.float64) ** 2).sum()) / np.sqrt(dall))))
    return np.array(wr), np.array(pr)


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
    calls = 0
    for first in range(0, K, chunk):
        q = slice(first, min(first + chunk, K))
        r = io.call_forward_steps(c, vsf, steps[q], None, 8, obst, datweight, group, ngroups, lib=lib)
        meas[q] = r["measures"]; fails[q] = r["failures"]; dsyn[q] = r["dsurf"]
        calls += 1
    return dict(measures=meas, failures=fails, dsyn=dsyn, calls=calls, resident=False, seconds=time.perf_counter() - t0)


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
        for k in range(nz - 1):
            for j in range(ny - 2):
                for i in range(nx - 2):
                    lon, lat = _lonlat(c, i, j)
                    fh.write(_f10(lon) + _f10(lat) + _f10(c["depz"][k]) + _f10(vsf[i + 1, j + 1, k]) +
                             "%13.8f%13.8f%11.5f%11.5f\n" % (gc[k, j, i], gs[k, j, i], st[k, j, i], ax[k, j, i]))


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
    dsyn = np.zeros(dall, f)
    nar = C.c_int(0)
    cc = dict(c); cc["vels"] = vsf
    head, tail = io._args(cc)
    lib.dsa_dropin_set_capacity(maxnar)
    t0 = time.perf_counter()
    rc = lib.dsa_calsurfg_azimuthal(*head, _p(iw), _p(rw), _p(col), _p(dsyn), *tail, C.byref(nar))
    lib.dsa_dropin_set_capacity(0)
    if rc != 0:
        raise RuntimeError("dsa_calsurfg_azimuthal: %s" % lib.dsa_dropin_error().decode())
    t_fwd = time.perf_counter() - t0
    n = nar.value
    rw, row, col = rw[:n].copy(), iw[1:n + 1].copy(), col[:n].copy()
    obst = np.ascontiguousarray(obst, f)
    res = (obst - dsyn).astype(f)
    datweight = azimuthal_weights(res, c["threshold0"])
    S = azimuthal_system(c, rw, row, col, res, datweight, c["weight0"], weight)
    eng = lib.dsa_dropin_engine()
    t0 = time.perf_counter()
    if lib.dsa_spmv_load(eng, S["m"], S["n"], C.c_longlong(S["rw"].size), _p(S["rw"]), _p(S["row"]), _p(S["col"])) != 0:
        raise RuntimeError("dsa_spmv_load: %s" % lib.dsa_error_string(eng).decode())
    x = np.zeros(S["n"], f)
    ii = [C.c_int(0), C.c_int(0)]
    ff = [C.c_float(0) for _ in range(5)]
    if lib.dsa_lsmr(eng, _p(S["b"]), C.c_float(damp), *LSMR_ARGS, _p(x), C.byref(ii[0]), C.byref(ii[1]), *[C.byref(v) for v in ff]) != 0:
        raise RuntimeError("dsa_lsmr: %s" % lib.dsa_error_string(eng).decode())
    t_lsmr = time.perf_counter() - t0
    dvs, gc, gs = x[:maxvp], x[maxvp:2 * maxvp], x[2 * maxvp:]
    log(" azimuthal step: %d x %d, %d entries (%d from the rays: %d Vs, %d gc, %d gs), weight %g damp %g, %d iterations, istop %d "
        "(forward %.3f s, LSMR %.3f s)" % (S["m"], S["n"], S["rw"].size, n, int((col <= maxvp).sum()), int(((col > maxvp) & (col <= 2 * maxvp)).sum()),
                                           int((col > 2 * maxvp).sum()), weight, damp, ii[1].value, ii[0].value, t_fwd, t_lsmr))
    log(" azimuthal step: min and max velocity variation of its Vs block %7.4f%7.4f (not applied); strength max %.3f %% of Vs" %
        (float(dvs.min()), float(dvs.max()), float(azimuthal_strength(gc, gs).max())))
    return dict(dvs=dvs, gc=gc, gs=gs, x=x, itn=ii[1].value, istop=ii[0].value, dsyn=dsyn, datweight=datweight, rw=rw, row=row, col=col,
                system=S, weight=weight, damp=damp, seconds=dict(forward=t_fwd, lsmr=t_lsmr))


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
                itn=ii[1].value, istop=ii[0].value, dv=dv, **arrays)


def iteration_device(lib, c, vsf, obst, log, bootstrap=None, resolution=None, tradeoff=None, voronoi=None, crossval=None, line_search=None):
    """One pass of main.f90:349-535 with the matrix resident on the device from CalSurfG to LSMR: dsa_calsurfg leaves the
    rows there (null rw / iw / col), dsa_iteration_system_device applies weights / appends the regularisation rows / builds
    both orderings in place, dsa_lsmr solves.  Same numbers as iteration() (tests/test_gpu_lsmr.py compares every bit).
    bootstrap = (R, seed): after dsa_lsmr, R row-resampled solves of the same system by dsa_lsmr_batch (returned as "boot").
    resolution = dict(psf=bool, chunk=int or None, cells=[(NX, NY, NZ), ...]): after dsa_lsmr, the resolution tests of the same
    system (returned as "res": "psf" from resolution_psf, "checker" from checkerboard_tests).
    tradeoff = dict(weights=[...], damps=[...], chunk=int or None): after dsa_lsmr, the trade-off sweep of the same system (returned as
    "trade" from lsmr_tradeoff_sweep).
    voronoi = dict(nreal, ncells, seed, zscale, damp, chunk, update): after dsa_lsmr, the Poisson-Voronoi ensemble of the same system's
    data rows (returned as "voronoi" from lsmr_voronoi_ensemble); with update, float32 of its mean is the update applied to vsf and
    returned as "dv" (dv_min / dv_max are its), dsa_lsmr's own stays in "dv_lsmr".
    crossval = dict(weights=[...], damps=[...], fold=(ndata,) int32, nfolds, chunk=int or None, want_x=bool): after dsa_lsmr, the K-fold
    cross-validation of the same system (returned as "crossval" from lsmr_crossval_sweep).
    line_search = [A1, A2, ...]: the update is applied at the step length among these whose model has the smallest true misfit
    (line_search_step, returned as "line_search"); "dv" stays the full-length update.
    tradeoff["nonlinear"] / crossval["nonlinear"]: after all of the above and before the line search / the update, the sweep's members
    through forward_steps_members on the model as it stands (returned as "trade_nl" / "crossval_nl"; the forward call re-dices the maps
    and leaves the resident matrix alone).  The cross-validation's updates stay on the device where one call held all pairs and no
    other batch solve follows it."""
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
    rc = lib.dsa_lsmr(eng, _p(cbst), C.c_float(c["damp"]), *LSMR_ARGS, _p(dv), C.byref(ii[0]), C.byref(ii[1]), *[C.byref(v) for v in ff])
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
    trade = None
    if tradeoff:
        trade = lsmr_tradeoff_sweep(lib, eng, c, cbst, m.value, nar2.value, tradeoff["weights"], tradeoff["damps"], tradeoff.get("chunk"))
    cv = None
    cv_resident = False
    if crossval:
        ncombo = len(crossval["weights"]) * len(crossval["damps"])
        cv_chunk = int(crossval.get("chunk") or crossval_chunk(m.value, maxvp, nar2.value, LOCAL_SIZE, ncombo, int(crossval["nfolds"]), dall))
        cv_resident = bool(crossval.get("nonlinear")) and ncombo <= cv_chunk and not voronoi
        cv = lsmr_crossval_sweep(lib, eng, c, cbst, m.value, nar2.value, crossval["weights"], crossval["damps"], crossval["fold"], crossval["nfolds"],
                                 cv_chunk, crossval.get("want_x", False) or (bool(crossval.get("nonlinear")) and not cv_resident))
    vor = None
    dv_lsmr = dv
    if voronoi:
        vor = lsmr_voronoi_ensemble(lib, eng, c, cbst, nar.value, voronoi["nreal"], voronoi["ncells"], voronoi["seed"], voronoi.get("zscale", 1.0),
                                    voronoi.get("damp"), voronoi.get("chunk"))
        if voronoi.get("update"):
            dv = np.ascontiguousarray(vor["mean"].astype(f))
    out = _pass_result(cbst[:dall], dv, ii, dsyn=dsyn, datweight=datweight, nar=nar2.value, m=m.value, dws=(float(dws[0]), float(dws[1])),
                       seconds=dict(forward=t_fwd, glue=t_glue, lsmr=t_lsmr), norm=norm, cbst=cbst)
    trade_nl = cv_nl = None
    if crossval and crossval.get("nonlinear"):
        K = cv["weight"].size * (cv["nfolds"] + 1)
        cv_nl = forward_steps_members(lib, c, vsf, None if cv_resident else cv["x"], obst, datweight, crossval["fold"], cv["nfolds"],
                                      crossval.get("nonlinear_chunk"), K)
    if tradeoff and tradeoff.get("nonlinear"):
        trade_nl = forward_steps_members(lib, c, vsf, trade["x"], obst, datweight, chunk=tradeoff.get("nonlinear_chunk"))
    ls = None
    if line_search:
        ls = line_search_step(lib, c, vsf, dv, obst, datweight, line_search)
        vsf[...] = ls["models"][ls["chosen"]]
    else:
        lib.dsa_model_update(nx, ny, nz, _p(dv), _p(vsf), c["minvel"], c["maxvel"])
    if ls is not None:
        out["line_search"] = ls
    if boot is not None:
        out["boot"] = boot
    if res is not None:
        out["res"] = res
    if trade is not None:
        out["trade"] = trade
    if cv is not None:
        out["crossval"] = cv
    if trade_nl is not None:
        out["trade_nl"] = trade_nl
    if cv_nl is not None:
        out["crossval_nl"] = cv_nl
    if vor is not None:
        out["voronoi"] = vor
        out["dv_lsmr"] = dv_lsmr
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
    rc = lib.dsa_lsmr_batch(eng, nreal, _p(cbst), _p(scales), C.c_float(c["damp"]), *LSMR_ARGS, _p(x), _p(istop), _p(itn), _p(est))
    if rc != 0:
        raise RuntimeError("dsa_lsmr_batch: %s" % lib.dsa_error_string(eng).decode())
    seconds = time.perf_counter() - t0
    return dict(x=x, std=x.astype(np.float64).std(axis=0, ddof=1), itn=itn, istop=istop, est=est, seconds=seconds)


def _lsmr_resolution(lib, eng, c, nreal, istop, itn, models=None, first=0, coords=None, x=None, psf=None):
    """one dsa_lsmr_resolution call with the arguments of the dsa_lsmr call above; istop / itn / x / psf filled in place"""
    est = np.zeros((nreal, 5), np.float32)
    rc = lib.dsa_lsmr_resolution(eng, nreal, c["ndata"], _p(models), first, _p(coords), C.c_float(c["damp"]), *LSMR_ARGS, _p(x), _p(psf), _p(istop), _p(itn), _p(est))
    if rc != 0:
        raise RuntimeError("dsa_lsmr_resolution: %s" % lib.dsa_error_string(eng).decode())


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


def lsmr_tradeoff_sweep(lib, eng, c, cbst, m, nar, weights, damps, chunk=None):
    """The trade-off sweep of the resident m-row system of nar entries (regularisation rows built with the input file's weight0): the
    members of tradeoff_grid(weights, damps) in chunks of `chunk` (default tradeoff_chunk(m, maxvp, nar, LOCAL_SIZE)), one dsa_lsmr_tradeoff call
    each with the arguments of the dsa_lsmr call above.  Returns dict(weight, damp (K,), x=(K, maxvp) raw updates, measures=(K, 3)
    {sum r^2, sum (C x)^2, sum x^2}, itn, istop, est=(K, 5), chunk, calls, seconds)."""
    f = np.float32
    n = c["nparpi"]
    w, d = tradeoff_grid(weights, damps)
    K = w.size
    chunk = int(chunk or tradeoff_chunk(m, n, nar, LOCAL_SIZE))
    x = np.zeros((K, n), f); meas = np.zeros((K, 3))
    istop = np.zeros(K, np.int32); itn = np.zeros(K, np.int32); est = np.zeros((K, 5), f)
    t0 = time.perf_counter()
    calls = 0
    for first in range(0, K, chunk):
        q = slice(first, min(first + chunk, K))
        wk, dk = np.ascontiguousarray(w[q]), np.ascontiguousarray(d[q])
        rc = lib.dsa_lsmr_tradeoff(eng, wk.size, c["ndata"], _p(cbst), C.c_float(c["weight0"]), _p(wk), _p(dk), *LSMR_ARGS, _p(x[q]), _p(meas[q]),
                                   _p(istop[q]), _p(itn[q]), _p(est[q]))
        if rc != 0:
            raise RuntimeError("dsa_lsmr_tradeoff: %s" % lib.dsa_error_string(eng).decode())
        calls += 1
    return dict(weight=w, damp=d, x=x, measures=meas, itn=itn, istop=istop, est=est, chunk=chunk, calls=calls, seconds=time.perf_counter() - t0)


def lsmr_crossval_sweep(lib, eng, c, cbst, m, nar, weights, damps, fold, nfolds, chunk=None, want_x=False):
    """K-fold cross-validation on the resident m-row system of nar entries (regularisation rows built with the input file's weight0): the
    combos of tradeoff_grid(weights, damps), each with the nfolds hold-outs of `fold` and its full member, in calls of `chunk` combos
    (default crossval_chunk(...)) with the arguments of the dsa_lsmr call above.  A call holds whole combos and returns every datum's
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
    calls = 0
    for first in range(0, nc, chunk):
        q = slice(first, min(first + chunk, nc))
        k = slice(q.start * S, q.stop * S)
        wk, dk = np.ascontiguousarray(w[q]), np.ascontiguousarray(d[q])
        rc = lib.dsa_lsmr_crossval(eng, wk.size, int(nfolds), nd, _p(cbst), C.c_float(c["weight0"]), _p(wk), _p(dk), _p(fold), *LSMR_ARGS,
                                   _p(x[k]) if want_x else None, _p(meas[k]), _p(resid[q]), _p(istop[k]), _p(itn[k]), _p(est[k]))
        if rc != 0:
            raise RuntimeError("dsa_lsmr_crossval: %s" % lib.dsa_error_string(eng).decode())
        calls += 1
    return dict(weight=w, damp=d, nfolds=int(nfolds), measures=meas, resid=resid, x=x, itn=itn, istop=istop, est=est, chunk=chunk, calls=calls,
                seconds=time.perf_counter() - t0)


def lsmr_voronoi_ensemble(lib, eng, c, cbst, nnz, nreal, ncells, seed, zscale=1.0, damp=None, chunk=None):
    """The Poisson-Voronoi ensemble of the resident system's data rows (nnz entries, or a bound of them: it sizes the calls): nreal members
    of ncells cells from voronoi_seeds(maxvp, ncells, nreal, seed) on the points voronoi_xyz(c, zscale), damping damp (default the input
    file's), in calls of `chunk` members (default voronoi_chunk(...)) with the other arguments of the dsa_lsmr call above.  One call: z and
    the cells stay on the device and the statistics come from it.  Several calls: every call returns z and its cells, the host expands them
    to x_k[j] = z_k[cell_k(j)] and voronoi_stats combines all members in order -- the same fp64 loop, so the same bits as one call.
    Returns dict(mean, std (maxvp,) float64, itn, istop, est=(nreal, 5), seeds, chunk, calls, seconds)."""
    f = np.float32
    n, nd = c["nparpi"], c["ndata"]
    damp = float(c["damp"]) if damp is None else float(damp)
    xyz = np.ascontiguousarray(voronoi_xyz(c, zscale))
    seeds = np.ascontiguousarray(voronoi_seeds(n, ncells, nreal, seed))
    chunk = int(chunk or voronoi_chunk(nd, n, ncells, int(nnz), LOCAL_SIZE))
    istop = np.zeros(nreal, np.int32); itn = np.zeros(nreal, np.int32); est = np.zeros((nreal, 5), f)
    single = nreal <= chunk
    stats = np.zeros((2, n))
    x = None if single else np.zeros((nreal, n), f)
    t0 = time.perf_counter()
    calls = 0
    for first in range(0, nreal, chunk):
        q = slice(first, min(first + chunk, nreal))
        k = q.stop - q.start
        sd = np.ascontiguousarray(seeds[q])
        z = None if single else np.zeros((k, ncells), f)
        cell = None if single else np.zeros((k, n), np.int32)
        rc = lib.dsa_lsmr_voronoi(eng, k, nd, ncells, _p(cbst), _p(xyz), _p(sd), C.c_float(damp), *LSMR_ARGS, _p(z), _p(cell), _p(stats) if single else None,
                                  _p(istop[q]), _p(itn[q]), _p(est[q]))
        if rc != 0:
            raise RuntimeError("dsa_lsmr_voronoi: %s" % lib.dsa_error_string(eng).decode())
        if not single:
            x[q] = np.take_along_axis(z, cell, axis=1)
        calls += 1
    if not single:
        stats = voronoi_stats(x)
    return dict(mean=stats[0].copy(), std=stats[1].copy(), itn=itn, istop=istop, est=est, seeds=seeds, chunk=chunk, calls=calls,
                seconds=time.perf_counter() - t0)


def tradeoff_members(t):
    """the rows of <input>Tradeoff.dat from lsmr_tradeoff_sweep's result: dicts with the keys TRADEOFF_COLUMNS"""
    nrm = np.sqrt(t["measures"])
    return [dict(weight=float(t["weight"][k]), damp=float(t["damp"][k]), misfit=float(nrm[k, 0]), rough=float(nrm[k, 1]), xnorm=float(nrm[k, 2]),
                 itn=int(t["itn"][k]), istop=int(t["istop"][k]), dv_min=float(t["x"][k].min()), dv_max=float(t["x"][k].max()))
            for k in range(t["weight"].size)]


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
    rc = lib.dsa_lsmr_dropin(i32(m.value), i32(maxvp), i32(2 * n + 1), i32(n), _p(iw), _p(rw), _p(cbst), f32(c["damp"]), *map(f32, LSMR_ARGS[:3]),
                             *map(i32, LSMR_ARGS[3:]), i32(0), _p(dv), C.byref(ii[0]), C.byref(ii[1]), *[C.byref(v) for v in ff])
    if rc != 0:
        raise RuntimeError("dsa_lsmr_dropin: %s" % lib.dsa_dropin_error().decode())
    t_lsmr = time.perf_counter() - t0
    out = _pass_result(cbst[:dall], dv, ii, dsyn=dsyn, datweight=datweight, nar=n, m=m.value, dws=(float(dws[0]), float(dws[1])),
                       seconds=dict(forward=t_fwd, glue=t_glue, lsmr=t_lsmr), norm=norm, cbst=cbst)
    lib.dsa_model_update(nx, ny, nz, _p(dv), _p(vsf), c["minvel"], c["maxvel"])
    return out


def bind(lib):
    """the argtypes of what this module calls, on load_library()'s handle or a bare ctypes.CDLL of the library (engine.declare_solvers)"""
    return declare_solvers(lib)


def check_bootstrap(bootstrap, host_rows):
    """the bootstrap's preconditions, checked before anything touches the GPU"""
    if bootstrap and bootstrap < 2:
        raise ValueError("--bootstrap needs at least 2 realisations (got %d)" % bootstrap)
    if bootstrap and host_rows:
        raise ValueError("--bootstrap solves on the device-resident system: it cannot be combined with --host-rows")


def check_line_search(alphas, host_rows):
    """the line search's preconditions, checked before anything touches the GPU (alphas None: no line search)"""
    if alphas is None:
        return
    alphas = list(alphas)
    if not alphas or not all(np.isfinite(a) and a >= 0 for a in alphas):
        raise ValueError("--line-search takes at least one step length, every one finite and >= 0 (got %r)" % (alphas,))
    if host_rows:
        raise ValueError("--line-search forward-models its candidates beside the device-resident system: it cannot be combined with --host-rows")


def check_resolution(resolution, checkerboards, host_rows, chunk=None):
    """the resolution tests' preconditions, checked before anything touches the GPU"""
    for cell in checkerboards or ():
        if len(cell) != 3 or any(int(v) != v or v < 1 for v in cell):
            raise ValueError("a checkerboard cell is NX,NY,NZ: three integers >= 1 (got %r)" % (cell,))
    if (resolution or checkerboards) and host_rows:
        raise ValueError("--resolution / --checkerboard solve on the device-resident system: they cannot be combined with --host-rows")
    if chunk is not None and chunk < 1:
        raise ValueError("resolution_chunk must be at least 1 (got %d)" % chunk)


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


def check_tradeoff_nonlinear(nonlinear, weights, host_rows):
    """--tradeoff-nonlinear's preconditions, checked before anything touches the GPU"""
    if not nonlinear:
        return
    if weights is None:
        raise ValueError("--tradeoff-nonlinear needs --tradeoff-weights")
    if host_rows:
        raise ValueError("--tradeoff-nonlinear judges the members of the sweep on the device-resident system: it cannot be combined with --host-rows")


def check_crossval_nonlinear(nonlinear, nfolds, host_rows):
    """--crossval-nonlinear's preconditions, checked before anything touches the GPU"""
    if not nonlinear:
        return
    if nfolds is None:
        raise ValueError("--crossval-nonlinear needs --crossval")
    if host_rows:
        raise ValueError("--crossval-nonlinear judges the members of the cross-validation on the device-resident system: it cannot be combined with --host-rows")


def check_voronoi(voronoi, update=False, host_rows=False, zscale=1.0, damp=None, nunknowns=None, chunk=None):
    """the Voronoi ensemble's preconditions, checked before anything touches the GPU (voronoi None: no ensemble; nunknowns: the number
    of unknowns once the input is read)"""
    if voronoi is None:
        if update:
            raise ValueError("--voronoi-update needs --voronoi")
        return
    try:
        ok = len(voronoi) == 2 and all(int(v) == v and v >= 1 for v in voronoi)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("--voronoi takes K,NCELLS: two integers >= 1 (got %r)" % (voronoi,))
    if host_rows:
        raise ValueError("--voronoi solves on the device-resident system: it cannot be combined with --host-rows")
    if not (np.isfinite(zscale) and zscale >= 0):
        raise ValueError("--voronoi-zscale must be a finite number >= 0 (got %r)" % (zscale,))
    if damp is not None and not (np.isfinite(damp) and damp >= 0):
        raise ValueError("--voronoi-damp must be a finite number >= 0 (got %r)" % (damp,))
    if nunknowns is not None and voronoi[1] > nunknowns:
        raise ValueError("--voronoi: %d cells are more than the %d unknowns" % (voronoi[1], nunknowns))
    if chunk is not None and (chunk < 64 or chunk % 64):
        raise ValueError("voronoi_chunk must be a multiple of 64 (got %d)" % chunk)


def _solve_stats(itn, istop):
    stops = {int(k): int(v) for k, v in zip(*np.unique(istop, return_counts=True))}
    return dict(realisations=int(itn.size), itn_min=int(itn.min()), itn_median=float(np.median(itn)), itn_max=int(itn.max()), istop=stops)


def _solve_text(h):
    return "%d realisations, itn min/median/max %d/%g/%d, istop %s" % (h["realisations"], h["itn_min"], h["itn_median"], h["itn_max"],
                                                                     " ".join("%d:%d" % kv for kv in sorted(h["istop"].items())))


def run(directory, maxiter=None, out_dir=".", log=print, seed=1, host_rows=False, bootstrap=0, bootstrap_seed=1, resolution=False, checkerboard=(),
        resolution_chunk=None, tradeoff_weights=None, tradeoff_damps=None, tradeoff_iter=1, tradeoff_chunk=None, voronoi=None, voronoi_seed=1,
        voronoi_zscale=1.0, voronoi_damp=None, voronoi_update=False, voronoi_chunk=None, crossval=None, crossval_weights=None, crossval_damps=None,
        crossval_by="datum", crossval_seed=1, crossval_iter=1, crossval_chunk=None, line_search=None, tradeoff_nonlinear=False,
        crossval_nonlinear=False, azimuthal=False, azimuthal_weight=None, azimuthal_damp=None):
    check_azimuthal(azimuthal, azimuthal_weight, azimuthal_damp)
    check_tradeoff_nonlinear(tradeoff_nonlinear, tradeoff_weights, host_rows)
    check_crossval_nonlinear(crossval_nonlinear, crossval, host_rows)
    check_bootstrap(bootstrap, host_rows)
    check_line_search(line_search, host_rows)
    check_crossval(crossval, crossval_weights, crossval_damps, crossval_by, crossval_iter, host_rows, maxiter, crossval_chunk)
    check_voronoi(voronoi, voronoi_update, host_rows, voronoi_zscale, voronoi_damp, None, voronoi_chunk)
    check_resolution(resolution, checkerboard, host_rows, resolution_chunk)
    check_tradeoff(tradeoff_weights, tradeoff_damps, tradeoff_iter, host_rows, maxiter, tradeoff_chunk)
    cells = [tuple(int(v) for v in cell) for cell in checkerboard or ()]
    lib = bind(load_library())
    c = io.load(directory)
    maxiter = c["maxiter"] if maxiter is None else maxiter
    check_tradeoff(tradeoff_weights, tradeoff_damps, tradeoff_iter, host_rows, maxiter, tradeoff_chunk)
    check_voronoi(voronoi, voronoi_update, host_rows, voronoi_zscale, voronoi_damp, c["nparpi"], voronoi_chunk)
    check_crossval(crossval, crossval_weights, crossval_damps, crossval_by, crossval_iter, host_rows, maxiter, crossval_chunk)
    cvrun = None
    if crossval is not None:
        cvrun = dict(weights=list(crossval_weights), damps=[float(c["damp"])] if crossval_damps is None else list(crossval_damps), nfolds=int(crossval),
                     fold=crossval_folds(c, int(crossval), crossval_by, crossval_seed), chunk=crossval_chunk, nonlinear=bool(crossval_nonlinear))
    sweep = None
    if tradeoff_weights is not None:
        sweep = dict(weights=list(tradeoff_weights), damps=[float(c["damp"])] if tradeoff_damps is None else list(tradeoff_damps), chunk=tradeoff_chunk,
                     nonlinear=bool(tradeoff_nonlinear))
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
    ls_rows = []
    for it in range(1, maxiter + 1):
        if host_rows:
            st = iteration(lib, c, vsf, obst, log)
        else:
            last = it == maxiter
            vor = None
            if voronoi is not None and (last or voronoi_update):
                vor = dict(nreal=int(voronoi[0]), ncells=int(voronoi[1]), seed=voronoi_seed + it - 1, zscale=voronoi_zscale, damp=voronoi_damp,
                           chunk=voronoi_chunk, update=voronoi_update)
            st = iteration_device(lib, c, vsf, obst, log, (bootstrap, bootstrap_seed) if bootstrap and last else None,
                                  dict(psf=resolution, chunk=resolution_chunk, cells=cells) if (resolution or cells) and last else None,
                                  sweep if it == tradeoff_iter else None, vor, cvrun if it == crossval_iter else None,
                                  list(line_search) if line_search is not None else None)
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
        h = {k: v for k, v in st.items() if k not in ("dsyn", "datweight", "dv", "norm", "cbst", "boot", "res", "trade", "voronoi", "dv_lsmr", "crossval", "line_search", "trade_nl", "crossval_nl")}
        if "line_search" in st:
            ls = st["line_search"]
            k = ls["chosen"]
            for q, a in enumerate(ls["alphas"]):
                ls_rows.append(dict(iteration=it, alpha=a, weighted_rms=float(ls["weighted_rms"][q]), rms=float(ls["rms"][q]),
                                    disp_failures=ls["failures"][q], chosen=int(q == k)))
            io.write_line_search(name + "LineSearch.dat", ls_rows)
            h["line_search"] = dict(alphas=ls["alphas"], weighted_rms=[float(v) for v in ls["weighted_rms"]], rms=[float(v) for v in ls["rms"]],
                                    failures=ls["failures"], chosen=k, alpha=ls["alphas"][k], seconds=ls["seconds"])
            log(" line search: step %g of %s taken, rms of the weighted residual %s -> %.6g (%d candidates in one forward call, %.3f s)" %
                (ls["alphas"][k], ",".join("%g" % a for a in ls["alphas"]), " ".join("%.6g" % v for v in ls["weighted_rms"]), ls["weighted_rms"][k],
                 len(ls["alphas"]), ls["seconds"]))
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
        if "trade" in st:
            t = st["trade"]
            members = tradeoff_members(t)
            write_tradeoff(name + "Tradeoff.dat", members)
            ht = h["tradeoff"] = dict(_solve_stats(t["itn"], t["istop"]), iteration=it, weights=sweep["weights"], damps=sweep["damps"], chunk=t["chunk"],
                                      calls=t["calls"], seconds=t["seconds"], members=members, corners=tradeoff_corners(members))
            log(" tradeoff: %d weights x %d damps at iteration %d: %s, %d calls of up to %d (%.3f s)" %
                (len(sweep["weights"]), len(sweep["damps"]), it, _solve_text(ht), ht["calls"], ht["chunk"], ht["seconds"]))
            for cn in ht["corners"]:
                log(" tradeoff damp %g: corner %s" % (cn["damp"], "not found" if cn["weight"] is None else "at weight %g" % cn["weight"]))
        if "crossval" in st:
            v = st["crossval"]
            fold = cvrun["fold"]
            members = crossval_members(v, fold)
            sel = crossval_select(members)
            write_crossval(name + "Crossval.dat", members)
            slot = datum_table(c)[0]
            one = sel["one_se"]
            write_crossval_residuals(name + "CrossvalResiduals.dat", slot, c["dist"], fold, st["datweight"], v["resid"][one, 0], v["resid"][one, 1])
            hx = h["crossval"] = dict(_solve_stats(v["itn"], v["istop"]), iteration=it, nfolds=cvrun["nfolds"], by=crossval_by, seed=crossval_seed,
                                      weights=cvrun["weights"], damps=cvrun["damps"], chunk=v["chunk"], calls=v["calls"], seconds=v["seconds"], members=members,
                                      best=sel["best"], one_se=sel["one_se"], cv_rms_by_slot=crossval_by_slot(slot, v["resid"][one, 0], c["kmax"]))
            log(" crossval: %d folds by %s, %d weights x %d damps at iteration %d: %s, %d calls of up to %d combos (%.3f s)" %
                (hx["nfolds"], crossval_by, len(cvrun["weights"]), len(cvrun["damps"]), it, _solve_text(hx), hx["calls"], hx["chunk"], hx["seconds"]))
            for tag, i in (("best", sel["best"]), ("one-SE", sel["one_se"])):
                t = members[i]
                log(" crossval %s: weight %g damp %g, held-out rms %.6g (se of its square %.3g), training rms %.6g" %
                    (tag, t["weight"], t["damp"], t["cv_rms"], t["cv_se"], t["train_rms"]))
        if "trade_nl" in st:
            t, nl = st["trade"], st["trade_nl"]
            rows = tradeoff_nonlinear_rows(t["weight"], t["damp"], t["measures"][:, 0], nl["measures"], nl["failures"], c["ndata"])
            io.write_tradeoff_nonlinear(name + "TradeoffNonlinear.dat", rows)
            picks = tradeoff_nonlinear_select(rows, [mb["rough"] for mb in h["tradeoff"]["members"]])
            h["tradeoff_nonlinear"] = dict(iteration=it, members=rows, picks=picks, calls=nl["calls"], seconds=nl["seconds"], dsyn=nl["dsyn"])
            log(" tradeoff nonlinear: %d members through %d forward call%s (%.3f s), %d dispersion curves without a root" %
                (len(rows), nl["calls"], "" if nl["calls"] == 1 else "s", nl["seconds"], int(np.sum(nl["failures"]))))
            for pk, cn in zip(picks, h["tradeoff"]["corners"]):
                log(" tradeoff nonlinear damp %g: smallest true weighted rms %s; corner on the true misfit %s (linear: %s)" %
                    (pk["damp"], "none" if pk["best"] is None else "%.6g at weight %g (predicted %.6g)" % (rows[pk["best"]]["weighted_rms"], pk["weight"], rows[pk["best"]]["predicted_rms"]),
                     "not found" if pk["corner"] is None else "at weight %g" % pk["corner_weight"], "not found" if cn["weight"] is None else "at weight %g" % cn["weight"]))
        if "crossval_nl" in st:
            v, nl = st["crossval"], st["crossval_nl"]
            rows = crossval_nonlinear_rows(v["weight"], v["damp"], v["nfolds"], nl["measures"], nl["failures"], [mb["cv_rms"] for mb in h["crossval"]["members"]], c["ndata"])
            io.write_crossval_nonlinear(name + "CrossvalNonlinear.dat", rows)
            best = crossval_nonlinear_select(rows)
            h["crossval_nonlinear"] = dict(iteration=it, members=rows, best=best, calls=nl["calls"], resident=nl["resident"], seconds=nl["seconds"], dsyn=nl["dsyn"])
            log(" crossval nonlinear: %d members through %d forward call%s (%.3f s; updates %s), %d dispersion curves without a root" %
                (len(nl["failures"]), nl["calls"], "" if nl["calls"] == 1 else "s", nl["seconds"], "resident on the device" if nl["resident"] else "from the host",
                 int(np.sum(nl["failures"]))))
            if best is not None:
                t = rows[best]
                log(" crossval nonlinear best: weight %g damp %g, true held-out rms %.6g (linear %.6g), true full-fit rms %.6g" %
                    (t["weight"], t["damp"], t["heldout_rms"], t["cv_rms"], t["full_rms"]))
        if "voronoi" in st:
            v = st["voronoi"]
            write_voronoi(name + "Voronoi.dat", c, v["mean"], v["std"])
            hv = h["voronoi"] = dict(_solve_stats(v["itn"], v["istop"]), iteration=it, cells=int(voronoi[1]), seed=voronoi_seed + it - 1, applied=bool(voronoi_update),
                                     std_max=float(v["std"].max()), std_mean=float(v["std"].mean()), seconds=v["seconds"], chunk=v["chunk"], calls=v["calls"])
            log(" voronoi: %d cells, %s, std of the update max %.5f mean %.5f km/s%s, %d calls of up to %d (%.3f s)" %
                (hv["cells"], _solve_text(hv), hv["std_max"], hv["std_mean"], ", the mean applied as the update" if voronoi_update else "", hv["calls"],
                 hv["chunk"], hv["seconds"]))
        history.append(h)
    if azimuthal:           # the joint Vs / gc / gs step on the final model; nothing of it is applied
        az = azimuthal_step(lib, c, vsf, obst, log, azimuthal_weight, azimuthal_damp)
        write_azimuthal(name + "Azim.dat", c, vsf, az["gc"], az["gs"])
        history.append(dict(azimuthal=dict(weight=az["weight"], damp=az["damp"], itn=az["itn"], istop=az["istop"], nar=int(az["rw"].size),
                                           dvs_min=float(az["dvs"].min()), dvs_max=float(az["dvs"].max()),
                                           strength_max=float(azimuthal_strength(az["gc"], az["gs"]).max()), seconds=az["seconds"])))
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
    ap.add_argument("--tradeoff-weights", type=_tradeoff_arg, default=None, metavar="W1,W2,...",
                    help="the trade-off curve of one iteration's step over these smoothing weights (and --tradeoff-damps): <input>Tradeoff.dat, "
                         "misfit against roughness per (weight, damp), and the curve's corner per damp in the log")
    ap.add_argument("--tradeoff-damps", type=_tradeoff_arg, default=None, metavar="D1,...", help="damps of the trade-off sweep (default: the input file's damp)")
    ap.add_argument("--tradeoff-iter", type=int, default=1, metavar="N", help="the outer iteration whose step is swept, 1..maxiter (default 1)")
    ap.add_argument("--voronoi", type=_voronoi_arg, default=None, metavar="K,NCELLS",
                    help="a Poisson-Voronoi ensemble of the last iteration's step: K members, each the data rows projected onto NCELLS random "
                         "Voronoi cells of the unknowns and solved with damping only: <input>Voronoi.dat, the ensemble mean and standard deviation "
                         "of the update.  The K solves run side by side and cost about the same for any K up to a few hundred: below about "
                         "K = 8 to 16 they take as long as, or longer than, K separate solves (DESIGN.md section 14)")
    ap.add_argument("--voronoi-seed", type=int, default=1, metavar="S", help="seed of the tessellations (default 1; iteration it uses S + it - 1)")
    ap.add_argument("--voronoi-zscale", type=float, default=1.0, metavar="F", help="stretch of the depth axis in the cells' metric (default 1.0)")
    ap.add_argument("--voronoi-damp", type=float, default=None, metavar="D", help="damping of the members' solves (default: the input file's damp)")
    ap.add_argument("--voronoi-update", action="store_true",
                    help="run the ensemble in every outer iteration and apply its mean as that iteration's update (dsa_lsmr still runs and is logged)")
    ap.add_argument("--crossval", type=int, default=None, metavar="NFOLDS",
                    help="K-fold cross-validation (NFOLDS >= 2) of one iteration's step over --crossval-weights x --crossval-damps: every pair is "
                         "solved once per held-out fold and once on all data, side by side on the resident system: <input>Crossval.dat (held-out and "
                         "training rms per pair), <input>CrossvalResiduals.dat (per datum, for the one-standard-error pair) and both selections in the log")
    ap.add_argument("--crossval-weights", type=_tradeoff_arg, default=None, metavar="W1,W2,...", help="smoothing weights of the cross-validation")
    ap.add_argument("--crossval-damps", type=_tradeoff_arg, default=None, metavar="D1,...", help="damps of the cross-validation (default: the input file's damp)")
    ap.add_argument("--crossval-by", choices=("datum", "path"), default="datum",
                    help="how the folds are made: datum deals single data at random; path keeps all data of one station pair, across periods and wave "
                         "types, in one fold.  A pair's dispersion curve is strongly correlated along period, so path is the honest hold-out for "
                         "surface-wave data (default datum)")
    ap.add_argument("--crossval-seed", type=int, default=1, metavar="S", help="seed of the folds (default 1)")
    ap.add_argument("--crossval-iter", type=int, default=1, metavar="N", help="the outer iteration whose step is cross-validated, 1..maxiter (default 1)")
    ap.add_argument("--tradeoff-nonlinear", action="store_true",
                    help="with --tradeoff-weights: judge every member of the sweep by the true travel times through the model it would produce "
                         "(built and forward-modelled on the device in one call per chunk): <input>TradeoffNonlinear.dat, predicted against true rms "
                         "per (weight, damp), and the best member and the corner on the true misfit per damp in the log")
    ap.add_argument("--crossval-nonlinear", action="store_true",
                    help="with --crossval: the same for the cross-validation's members, every datum judged by the model of the member that held its "
                         "fold out: <input>CrossvalNonlinear.dat, true held-out and full-fit rms per pair beside the linear cv_rms")
    ap.add_argument("--line-search", type=_line_search_arg, default=None, metavar="A1,A2,...",
                    help="step-length line search: in every outer iteration the update is tried at these fractions of its length (each >= 0; 0 keeps "
                         "the model), all candidate models are forward-modelled in one call, and the one with the smallest rms of the weighted "
                         "travel-time residual is applied: <input>LineSearch.dat, one row per (iteration, step)")
    ap.add_argument("--azimuthal", action="store_true",
                    help="after the last iteration, one joint step for Vs and the 2psi azimuthal anisotropy gc = Gc/L, gs = Gs/L on the final model "
                         "(Rayleigh periods): <input>Azim.dat (Vs, gc, gs, strength in per cent of Vs, fast axis in degrees from north); nothing of it "
                         "is applied to the model")
    ap.add_argument("--azimuthal-weight", type=float, default=None, metavar="W", help="smoothing weight of the gc and gs blocks (default: the input file's weight0)")
    ap.add_argument("--azimuthal-damp", type=float, default=None, metavar="D", help="damping of the azimuthal step's solve (default: the input file's damp)")
    args = ap.parse_args(argv)
    try:
        check_azimuthal(args.azimuthal, args.azimuthal_weight, args.azimuthal_damp)
        check_tradeoff_nonlinear(args.tradeoff_nonlinear, args.tradeoff_weights, args.host_rows)
        check_crossval_nonlinear(args.crossval_nonlinear, args.crossval, args.host_rows)
        check_bootstrap(args.bootstrap, args.host_rows)
        check_line_search(args.line_search, args.host_rows)
        check_crossval(args.crossval, args.crossval_weights, args.crossval_damps, args.crossval_by, args.crossval_iter, args.host_rows, args.maxiter)
        check_voronoi(args.voronoi, args.voronoi_update, args.host_rows, args.voronoi_zscale, args.voronoi_damp)
        check_resolution(args.resolution, args.checkerboard, args.host_rows)
        check_tradeoff(args.tradeoff_weights, args.tradeoff_damps, args.tradeoff_iter, args.host_rows, args.maxiter)
    except ValueError as exc:
        ap.error(str(exc))
    os.makedirs(args.out, exist_ok=True)
    run(args.directory, args.maxiter, args.out, host_rows=args.host_rows, bootstrap=args.bootstrap, bootstrap_seed=args.bootstrap_seed,
        resolution=args.resolution, checkerboard=args.checkerboard, tradeoff_weights=args.tradeoff_weights, tradeoff_damps=args.tradeoff_damps,
        tradeoff_iter=args.tradeoff_iter, voronoi=args.voronoi, voronoi_seed=args.voronoi_seed, voronoi_zscale=args.voronoi_zscale,
        voronoi_damp=args.voronoi_damp, voronoi_update=args.voronoi_update, crossval=args.crossval, crossval_weights=args.crossval_weights,
        crossval_damps=args.crossval_damps, crossval_by=args.crossval_by, crossval_seed=args.crossval_seed, crossval_iter=args.crossval_iter,
        line_search=args.line_search, tradeoff_nonlinear=args.tradeoff_nonlinear, crossval_nonlinear=args.crossval_nonlinear,
        azimuthal=args.azimuthal, azimuthal_weight=args.azimuthal_weight, azimuthal_damp=args.azimuthal_damp)
    return 0


if __name__ == "__main__":
    sys.exit(main())
