"""Freeze the bits of the depth column family (DESIGN.md sections 21-25) in tests/golden/column_family.npz.

    python tests/golden/make_column_family.py          # CPU only; writes the fixture next to this file

Per case the file holds the inputs and every array that the five host harnesses (tests/columns_ref.py, column_resolution_ref.py,
column_radial_ref.py, column_lateral_ref.py, column_radial_lateral_ref.py) and the five NumPy twins of dsurftomo_amd/depth.py return for
them -- the twins' answers through lstsq / pinv excepted: LAPACK's bits are not ours.  tests/test_column_family_frozen.py recomputes all of
it with compute() from the stored inputs and compares bit patterns, so a change of these functions that moves one bit of one figure fails
there.  The fixture is written once, by the commit before the family's headers were merged into one; it is regenerated only by a change
that is meant to change the arithmetic.

The cases: grids (3, 3) (one interior column), (5, 4) and (6, 5); (M, K) = (1, 2), (2, 4), (5, 7) with the odd slots Love; weights given
and None; from four interior columns on, one column without a usable datum whose kernels are NaN (every weight 0, or every observation 0
where no weights are given) and one whose used kernels are NaN (flag 1), both beside active neighbours; the coupled steps at every
setting of SETTINGS_LATERAL / SETTINGS_RADIAL_LATERAL: with and without edges, stopped by the tolerance and by maxit = 1, poll 0, 1, 16.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for p in (os.path.dirname(TESTS), TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)

PATH = os.path.join(HERE, "column_family.npz")
F = np.float32
SMOOTH, DAMP, ANISO, DVMAX, MINVEL, MAXVEL, TOL = 0.2, 0.05, 0.2, 0.1, 0.5, 6.0, 1e-8
# (name, nx, ny, M, K, weights given, twins too)
CASES = [("g33_m1", 3, 3, 1, 2, True, True), ("g33_m1_nowt", 3, 3, 1, 2, False, False), ("g54_m2", 5, 4, 2, 4, True, True), ("g54_m2_nowt", 5, 4, 2, 4, False, True),
         ("g65_m5", 6, 5, 5, 7, True, False), ("g65_m5_nowt", 6, 5, 5, 7, False, False), ("g65_m1", 6, 5, 1, 2, True, False),
         ("g33_m2", 3, 3, 2, 4, True, False)]
# (lateral, maxit, poll)
SETTINGS_LATERAL = [(0.0, 500, 16), (0.3, 500, 16), (0.3, 500, 0), (0.3, 500, 1), (0.3, 1, 16)]
# (lateral, lateral_aniso, maxit, poll)
SETTINGS_RADIAL_LATERAL = [(0.0, 0.0, 500, 16), (0.3, 0.0, 500, 16), (0.3, 0.6, 500, 16), (0.0, 0.5, 500, 16), (0.3, 0.6, 500, 0), (0.3, 0.6, 500, 1), (0.3, 0.6, 1, 16)]


def make_inputs(nx, ny, M, K, weights, twins, seed):
    """the stored inputs of one case: dims, love (K), obs, wt (K, n) fp32 (wt absent where none are given), pv (K, n), Sv, Sh (M, K, n), vsv,
    vsh (M + 1, n) fp32, depz (M + 1) fp32, and for M <= 2 raw (3, M + 1, K, n): kernels for the combination"""
    rng = np.random.default_rng(seed)
    n = nx * ny
    Sv = rng.random((M, K, n)) * (2.0 / M); Sh = Sv * (1.0 + 0.2 * rng.random((M, K, n)))
    pv = 3.0 + rng.random((K, n))
    obs = (pv * (1.0 + 0.03 * rng.standard_normal((K, n)))).astype(F)
    wt = (0.5 + rng.random((K, n))).astype(F)
    wt[0, :] = np.where(np.arange(n) % 3 == 0, 0.0, wt[0, :])          # some data dropped everywhere, the three ways
    obs[1, n // 2] = 0.0; pv[K - 1, 0] = 0.0; pv[K - 1, n - 1 - nx - 1] = 0.0
    vsv = (3.0 + 0.3 * rng.random((M + 1, n))).astype(F); vsh = (vsv * (1.0 + 0.05 * rng.random((M + 1, n)))).astype(F)
    vsv[0, ::4] = F(MINVEL + 0.01); vsh[M - 1, 1::4] = F(MAXVEL - 0.01)    # the model's clip at both ends
    interior = [j * nx + i for j in range(1, ny - 1) for i in range(1, nx - 1)]
    if len(interior) >= 4:
        dead, bad = interior[1], interior[2]
        if weights:
            wt[:, dead] = 0.0
        else:
            obs[:, dead] = 0.0
        Sv[:, :, dead] = np.nan; Sh[:, :, dead] = np.inf
        obs[:, bad] = np.abs(obs[:, bad]) + F(1.0); wt[:, bad] = 1.0; pv[:, bad] = 3.5
        Sv[M - 1, :, bad] = np.nan; Sh[M - 1, :, bad] = np.nan
    depz = np.concatenate([[0.0], np.cumsum(2.0 + 4.0 * np.arange(M) / max(M - 1, 1))]).astype(F)
    depz[M - 1] = F(34.0) if seed % 2 else F(36.0)                       # both coefficient sets of the combination (depz[nz - 2] < 35)
    inp = dict(dims=np.array([nx, ny, M, K, int(twins)], np.int64), love=(np.arange(K) % 2 == 1), obs=obs, pv=pv, Sv=Sv, Sh=Sh, vsv=vsv, vsh=vsh, depz=depz)
    if M <= 2:                                                          # (the combination works element by element: the small cases say all)
        inp["raw"] = rng.random((3, M + 1, K, n)) * 0.1
    if weights:
        inp["wt"] = wt
    return inp


def _arrays(prefix, d, skip=()):
    return {"%s/%s" % (prefix, k): np.ascontiguousarray(v) for k, v in d.items() if k not in skip and v is not None}


def _stack(results, skip):
    """per-column twin results side by side: one array per field, the column index last"""
    return {k: np.stack([np.asarray(r[k]) for r in results], axis=-1) for k in results[0] if k not in skip}


def compute(inp):
    """every output of one case, {"<function>/<field>": array}, from the stored inputs"""
    import column_lateral_ref as LR
    import column_radial_lateral_ref as RLR
    import column_radial_ref as RR
    import column_resolution_ref as CR
    import columns_ref as R
    from dsurftomo_amd import depth

    nx, ny, M, K, twins = (int(v) for v in inp["dims"])
    n = nx * ny
    love, obs, wt, pv, Sv, Sh, vsv, vsh, depz = (inp.get(k) for k in ("love", "obs", "wt", "pv", "Sv", "Sh", "vsv", "vsh", "depz"))
    only = R.interior(nx, ny)
    out = {}
    hs = R.load()
    if "raw" in inp:
        out["host_combine/S"] = R.host_combine(hs, vsv, depz, *inp["raw"])
    out.update(_arrays("host_step", R.host_step(hs, obs, wt, pv, Sv, vsv, SMOOTH, DAMP, DVMAX, MINVEL, MAXVEL, only)))
    for full in (True, False):
        out.update(_arrays("host_resolution%d" % full, CR.host_resolution(CR.load(), obs, wt, pv, Sv, depz, SMOOTH, DAMP, only, full=full, fill=7.0)))
    out.update(_arrays("host_radial", RR.host_step(RR.load(), love, obs, wt, pv, Sv, Sh, vsv, vsh, SMOOTH, DAMP, ANISO, DVMAX, MINVEL, MAXVEL, only), ("dv_sv", "dv_sh")))
    out.update(_arrays("host_radial_g0", RR.host_step(RR.load(), love, obs, wt, pv, Sv, Sh, vsv, vsh, SMOOTH, DAMP, 0.0, DVMAX, MINVEL, MAXVEL, only), ("dv_sv", "dv_sh")))
    scalars = lambda r: dict(r, **{k: np.array(r[k]) for k in ("itn", "istop", "rz0", "rz", "started") if k in r})
    for lat, maxit, poll in SETTINGS_LATERAL:
        r = LR.host_step(LR.load(), nx, ny, obs, wt, pv, Sv, vsv, SMOOTH, DAMP, lat, DVMAX, MINVEL, MAXVEL, TOL, maxit, poll)
        out.update(_arrays("host_lateral_%g_%d_%d" % (lat, maxit, poll), scalars(r)))
    for lat, lata, maxit, poll in SETTINGS_RADIAL_LATERAL:
        r = RLR.host_step(RLR.load(), nx, ny, love, obs, wt, pv, Sv, Sh, vsv, vsh, SMOOTH, DAMP, ANISO, lat, lata, DVMAX, MINVEL, MAXVEL, TOL, maxit, poll)
        out.update(_arrays("host_radial_lateral_%g_%g_%d_%d" % (lat, lata, maxit, poll), scalars(r), ("dv_sv", "dv_sh")))
    if not twins:
        return out
    cols = np.flatnonzero(only)
    w = lambda c: None if wt is None else wt[:, c]
    S = np.where(love[None, :, None], Sh, Sv)                            # the radial twins' S: slot k's sensitivities to the model it was run on
    out.update(_arrays("twin_step", _stack([depth.column_step_twin(obs[:, c], w(c), pv[:, c], Sv[:, :, c].T, vsv[:, c], SMOOTH, DAMP, DVMAX, MINVEL, MAXVEL)
                                            for c in cols], ())))
    out.update(_arrays("twin_radial", _stack([depth.column_radial_twin(obs[:, c], w(c), pv[:, c], S[:, :, c].T, love, vsv[:, c], vsh[:, c], SMOOTH, DAMP, ANISO, DVMAX,
                                                                       MINVEL, MAXVEL) for c in cols], ())))
    out.update(_arrays("twin_resolution", _stack([depth.column_resolution_twin(obs[:, c], w(c), pv[:, c], Sv[:, :, c].T, depz, SMOOTH, DAMP) for c in cols], ("other",))))
    for lat, maxit in sorted(set((s[0], s[1]) for s in SETTINGS_LATERAL)):
        r = depth.column_lateral_twin(nx, ny, obs, wt, pv, Sv, vsv, SMOOTH, DAMP, lat, DVMAX, MINVEL, MAXVEL, TOL, maxit)
        out.update(_arrays("twin_lateral_%g_%d" % (lat, maxit), {k: np.asarray(v) for k, v in r.items()}, ("delta_lstsq",)))
    for lat, lata, maxit in sorted(set(s[:3] for s in SETTINGS_RADIAL_LATERAL)):
        r = depth.column_radial_lateral_twin(nx, ny, obs, wt, pv, S, love, vsv, vsh, SMOOTH, DAMP, ANISO, lat, lata, DVMAX, MINVEL, MAXVEL, TOL, maxit)
        out.update(_arrays("twin_radial_lateral_%g_%g_%d" % (lat, lata, maxit), {k: np.asarray(v) for k, v in r.items()}, ("delta_lstsq",)))
    return out


def pack(out):
    """the outputs of a case as two arrays -- the bytes of all fields on end, and "field dtype shape" per line -- so that the archive holds
    a dozen members per case and not hundreds"""
    names = sorted(out)
    index = "\n".join("%s %s %s" % (k, out[k].dtype.str, ",".join(str(d) for d in out[k].shape)) for k in names)
    return np.concatenate([np.ascontiguousarray(out[k]).reshape(-1).view(np.uint8) for k in names]), np.array(index)


def unpack(blob, index):
    out, at = {}, 0
    for line in str(index).split("\n"):
        name, dtype, shape = line.split(" ")
        shape = tuple(int(d) for d in shape.split(",") if d)
        size = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
        out[name] = blob[at:at + size].view(dtype).reshape(shape)
        at += size
    assert at == blob.size
    return out


def load(path=PATH):
    """{case: (inputs, outputs)} of the fixture"""
    cases = {}
    with np.load(path) as z:
        for key in z.files:
            case, kind, name = key.split(":")
            if kind == "in":
                cases.setdefault(case, ({}, {}))[0][name] = z[key]
        for case in cases:
            cases[case][1].update(unpack(z[case + ":out:bytes"], z[case + ":out:index"]))
    return cases


def main():
    arrays = {}
    for seed, (name, nx, ny, M, K, weights, twins) in enumerate(CASES):
        inp = make_inputs(nx, ny, M, K, weights, twins, 100 + seed)
        arrays.update({"%s:in:%s" % (name, k): v for k, v in inp.items()})
        arrays["%s:out:bytes" % name], arrays["%s:out:index" % name] = pack(compute(inp))
    np.savez_compressed(PATH, **arrays)
    print("%s: %d arrays, %d bytes" % (PATH, len(arrays), os.path.getsize(PATH)))


if __name__ == "__main__":
    main()
