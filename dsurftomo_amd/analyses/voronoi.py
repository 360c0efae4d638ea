"""--voronoi K,NCELLS adds a Poisson-Voronoi subspace ensemble (Fang et al. 2020) of the last iteration's step, after its dsa_lsmr and on the
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
"""
import ctypes as C
import time

import numpy as np

from .common import EARTH_KM, LOCAL_SIZE, LSMR_ARGS, _fit, _p, _solve_stats, _solve_text, arg_type, batch_bytes, call_solver, chunks, parse_ints, unknown_coords, unknowns_grid, write_model


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


def voronoi_xyz(c, zscale=1.0):
    """(maxvp, 3) float64 points in km of the unknowns (unknown_coords) for the Voronoi assignment: coords_xyz of them"""
    return coords_xyz(unknown_coords(c), zscale)


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
    return parse_ints(text, 2, "--voronoi takes K,NCELLS: two integers >= 1")


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


def lsmr_voronoi_ensemble(lib, eng, c, cbst, nnz, nreal, ncells, seed, zscale=1.0, damp=None, chunk=None):
    """The Poisson-Voronoi ensemble of the resident system's data rows (nnz entries, or a bound of them: it sizes the calls): nreal members
    of ncells cells from voronoi_seeds(maxvp, ncells, nreal, seed) on the points voronoi_xyz(c, zscale), damping damp (default the input
    file's), in calls of `chunk` members (default voronoi_chunk(...)) with the other arguments of the pass's dsa_lsmr call.  One call: z and
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
    for q in chunks(nreal, chunk):
        k = q.stop - q.start
        sd = np.ascontiguousarray(seeds[q])
        z = None if single else np.zeros((k, ncells), f)
        cell = None if single else np.zeros((k, n), np.int32)
        call_solver(lib, eng, "dsa_lsmr_voronoi", k, nd, ncells, _p(cbst), _p(xyz), _p(sd), C.c_float(damp), *LSMR_ARGS, _p(z), _p(cell), _p(stats) if single else None,
                    _p(istop[q]), _p(itn[q]), _p(est[q]))
        if not single:
            x[q] = np.take_along_axis(z, cell, axis=1)
    if not single:
        stats = voronoi_stats(x)
    return dict(mean=stats[0].copy(), std=stats[1].copy(), itn=itn, istop=istop, est=est, seeds=seeds, chunk=chunk, calls=len(chunks(nreal, chunk)),
                seconds=time.perf_counter() - t0)


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


OPTIONS = (
    ("--voronoi", "voronoi", None, dict(type=arg_type(parse_voronoi), metavar="K,NCELLS",
        help="a Poisson-Voronoi ensemble of the last iteration's step: K members, each the data rows projected onto NCELLS random "
             "Voronoi cells of the unknowns and solved with damping only: <input>Voronoi.dat, the ensemble mean and standard deviation "
             "of the update.  The K solves run side by side and cost about the same for any K up to a few hundred: below about "
             "K = 8 to 16 they take as long as, or longer than, K separate solves (DESIGN.md section 14)")),
    ("--voronoi-seed", "voronoi_seed", 1, dict(type=int, metavar="S", help="seed of the tessellations (default 1; iteration it uses S + it - 1)")),
    ("--voronoi-zscale", "voronoi_zscale", 1.0, dict(type=float, metavar="F", help="stretch of the depth axis in the cells' metric (default 1.0)")),
    ("--voronoi-damp", "voronoi_damp", None, dict(type=float, metavar="D", help="damping of the members' solves (default: the input file's damp)")),
    ("--voronoi-update", "voronoi_update", False, dict(action="store_true",
        help="run the ensemble in every outer iteration and apply its mean as that iteration's update (dsa_lsmr still runs and is logged)")),
    (None, "voronoi_chunk", None, None),
)


def check(o, host_rows, maxiter, c):
    check_voronoi(o["voronoi"], o["voronoi_update"], host_rows, o["voronoi_zscale"], o["voronoi_damp"], None if c is None else c["nparpi"], o["voronoi_chunk"])


def plan(o, c, it, maxiter):
    if o["voronoi"] is None or not (it == maxiter or o["voronoi_update"]):
        return None
    return dict(nreal=int(o["voronoi"][0]), ncells=int(o["voronoi"][1]), seed=o["voronoi_seed"] + it - 1, zscale=o["voronoi_zscale"], damp=o["voronoi_damp"],
                chunk=o["voronoi_chunk"], update=o["voronoi_update"])


def solve(s, plan, res):
    res["voronoi"] = lsmr_voronoi_ensemble(s.lib, s.eng, s.c, s.cbst, s.nnz_data, plan["nreal"], plan["ncells"], plan["seed"], plan.get("zscale", 1.0),
                                           plan.get("damp"), plan.get("chunk"))


def report(ctx, st, h):
    v, p = st["voronoi"], ctx.plans["voronoi"]
    write_voronoi(ctx.name + "Voronoi.dat", ctx.c, v["mean"], v["std"])
    hv = h["voronoi"] = dict(_solve_stats(v["itn"], v["istop"]), iteration=ctx.it, cells=p["ncells"], seed=p["seed"], applied=bool(p["update"]),
                             std_max=float(v["std"].max()), std_mean=float(v["std"].mean()), seconds=v["seconds"], chunk=v["chunk"], calls=v["calls"])
    ctx.log(" voronoi: %d cells, %s, std of the update max %.5f mean %.5f km/s%s, %d calls of up to %d (%.3f s)" %
            (hv["cells"], _solve_text(hv), hv["std_max"], hv["std_mean"], ", the mean applied as the update" if p["update"] else "", hv["calls"],
             hv["chunk"], hv["seconds"]))
