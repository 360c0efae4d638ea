"""The azimuthal step on the device: dsa_solve_rows_azimuthal_device, dsa_calsurfg_azimuthal with null arrays,
dsa_iteration_system_azimuthal_device, dsa_resolution_blocks and the driver dsurftomo_amd.anisotropy.

Everything is held against the host route of section 18, bit for bit: the rows against dsa_solve_rows_azimuthal, the joint system against
azimuthal_weights + azimuthal_system + dsa_spmv_load on the host rows of the same call, the block PSF solves against dsa_lsmr_resolution.
The fp64 sums of the block PSFs are held against NumPy on the fetched solutions to 1e-9, the tolerance test_gpu_resolution.py uses for the
same arithmetic.
"""
import ctypes as C
import os

import numpy as np
import pytest

import _libs as L
import synth
import synth_matrix as SM
import test_gpu_azimuthal as TA
import test_gpu_rows as R
from dsurftomo_amd import anisotropy as A
from dsurftomo_amd import invert
from dsurftomo_amd import io as taipei
from dsurftomo_amd.analyses.common import _p, call_solver
from dsurftomo_amd.engine import Engine, EngineError, load_library
from test_gpu_lsmr_batch import EST, assert_all_equal, load, realisation
from test_gpu_resolution import psf_numpy

pytestmark = pytest.mark.gpu
bits = TA.bits
NX = TA.NX


def bits64(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- 1. rows ----

@pytest.mark.parametrize("lanes", [1, 4])
def test_device_rows_equal_host_rows(lanes):
    """576 rays over three launches: the device entry's host copy == dsa_solve_rows_azimuthal in times, rw, iw, col; with null arrays the
    same nar and statistics; the option rows_on_device is left as found; the plain and the host-row calls afterwards are unchanged"""
    e = Engine(0)
    try:
        u, dm = TA.plan(), R.depth_model(NX, NX)
        TA.prepare(e, u, dm)
        cap = TA.capacity(u)
        per_ray = (3 * NX * NX + (NX - 2) * (NX - 2)) * 4 + 32
        e.set_option("ray_lanes", lanes)
        e.set_option("ray_budget", 200 * per_ray)
        t_iso, rw_iso, iw_iso, col_iso = e.solve_rows(cap)
        t0, rw0, iw0, col0 = e.solve_rows_azimuthal(cap)
        st0 = e.stats()
        t1, rw1, iw1, col1 = e.solve_rows_azimuthal_device(cap)
        st1 = e.stats()
        assert st1["ray_launches"] == 3 and st1["rays"] == 576
        assert rw1.size == rw0.size > 0
        assert (bits(t1) == bits(t0)).all() and (bits(rw1) == bits(rw0)).all() and (iw1 == iw0).all() and (col1 == col0).all()
        t2, nar2 = e.solve_rows_azimuthal_device(cap, host_copy=False)
        st2 = e.stats()
        assert nar2 == rw0.size and (bits(t2) == bits(t0)).all()
        for k in ("nar", "rays", "ray_launches", "ray_steps", "rays_clamped"):
            assert st2[k] == st1[k] == st0[k], k
        # exactly enough room, and one entry short
        e.solve_rows_azimuthal_device(rw0.size, host_copy=False)
        with pytest.raises(EngineError) as exc:
            e.solve_rows_azimuthal_device(rw0.size - 1, host_copy=False)
        assert exc.value.code == -6
        # the option was off and is off: the host entry still works, and gives its earlier bits, as does the plain call
        t3, rw3, iw3, col3 = e.solve_rows_azimuthal(cap)
        assert (bits(rw3) == bits(rw0)).all() and (iw3 == iw0).all() and (col3 == col0).all() and (bits(t3) == bits(t0)).all()
        t4, rw4, iw4, col4 = e.solve_rows(cap)
        assert (bits(rw4) == bits(rw_iso)).all() and (iw4 == iw_iso).all() and (col4 == col_iso).all() and (bits(t4) == bits(t_iso)).all()
        # the option on: the host entry refuses as before, the device entry works and leaves it on
        e.set_option("rows_on_device", 1)
        with pytest.raises(EngineError) as exc:
            e.solve_rows_azimuthal(cap)
        assert exc.value.code == -5
        t5, rw5, iw5, col5 = e.solve_rows_azimuthal_device(cap)
        assert (bits(rw5) == bits(rw0)).all() and (col5 == col0).all()
        with pytest.raises(EngineError) as exc:
            e.solve_rows_azimuthal(cap)
        assert exc.value.code == -5
        # only some of the three arrays
        nar = C.c_longlong(0)
        out = np.zeros(e.ndata, np.float32); rw = np.zeros(cap, np.float32)
        assert e._L.dsa_solve_rows_azimuthal_device(e._h, _p(out), _p(rw), None, None, C.c_longlong(cap), C.byref(nar)) == -2
    finally:
        e.close()


# ---- 2. the joint system ----

def joint_case():
    c = synth.boundary_case(nx=10, ny=9, nz=4, kRc=3, kRg=1, kLc=1, kLg=0, nsrc=8, nrcf=8, ragged=False)
    c.update(spfra=1.0, threshold0=np.float32(1.2), weight0=np.float32(2.0), damp=np.float32(0.5), minvel=np.float32(1.5), maxvel=np.float32(5.5))
    assert c["nparpi"] == 168
    return c


def solve_on(lib, eng, b, damp, n, m, seed):
    """dsa_spmv both ways on seeded vectors and dsa_lsmr, on whatever is resident on eng"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n).astype(np.float32); y0 = np.zeros(m, np.float32)
    assert lib.dsa_spmv(eng, 1, _p(x), _p(y0)) == 0
    y = rng.standard_normal(m).astype(np.float32); x0 = np.zeros(n, np.float32)
    assert lib.dsa_spmv(eng, 2, _p(x0), _p(y)) == 0
    sol = np.zeros(n, np.float32)
    ii = [C.c_int(-1), C.c_int(-1)]
    ff = [C.c_float(0) for _ in range(5)]
    call_solver(lib, eng, "dsa_lsmr", _p(b), C.c_float(damp), *invert.LSMR_ARGS, _p(sol), C.byref(ii[0]), C.byref(ii[1]), *[C.byref(v) for v in ff])
    return dict(Ax=y0, Aty=x0, x=sol, istop=ii[0].value, itn=ii[1].value, est=np.array([v.value for v in ff], np.float32))


def same_solves(a, b):
    for k in ("Ax", "Aty", "x", "est"):
        assert (bits(a[k]) == bits(b[k])).all(), k
    assert a["istop"] == b["istop"] and a["itn"] == b["itn"]


@pytest.fixture(scope="module")
def host_rows():
    """the host rows and times of the joint case, and data with about a fifth of the weights at zero: once for the module"""
    lib = invert.bind(load_library())
    c = joint_case()
    fwd = TA.call_azimuthal(lib, c)
    r = synth.LCG(91)
    obst = (fwd["dsurf"] * (1.0 + 0.04 * (r.uniform(c["ndata"]) - 0.5))).astype(np.float32)
    return lib, c, fwd, obst


@pytest.mark.parametrize("weight_azi", [0.05, 2.0])
def test_joint_system_equals_the_host_route(host_rows, weight_azi):
    lib, c, fwd, obst = host_rows
    f = np.float32
    dall, maxvp, damp = c["ndata"], c["nparpi"], float(c["damp"])
    vsf = np.asfortranarray(c["vels"].copy())
    D = A.joint_system_device(lib, c, vsf, obst, weight_azi)
    eng = D["eng"]
    assert (bits(D["dsyn"]) == bits(fwd["dsurf"])).all() and D["nnz_data"] == fwd["nar"]
    dev = solve_on(lib, eng, D["cbst"], damp, D["n"], D["m"], 17)
    res = (obst - fwd["dsurf"]).astype(f)
    dw = invert.azimuthal_weights(res, c["threshold0"])
    assert 0 < int((dw == 0).sum()) < dall
    S = invert.azimuthal_system(c, fwd["rw"], fwd["iw"], fwd["col"], res, dw, c["weight0"], weight_azi)
    assert D["m"] == S["m"] == dall + 3 * maxvp and D["n"] == S["n"] and D["nar"] == S["rw"].size
    assert (bits(D["datweight"]) == bits(dw)).all() and (bits(D["cbst"]) == bits(S["b"])).all()
    # norm: per column the sequential fp32 sum of |entry| over the scaled data entries in storage order
    want_norm = np.zeros(3 * maxvp, f)
    scaled = np.abs(S["rw"][:fwd["nar"]])
    for k in range(fwd["nar"]):
        j = fwd["col"][k] - 1
        want_norm[j] = want_norm[j] + scaled[k]
    assert (bits(D["norm"]) == bits(want_norm)).all() and want_norm[maxvp:].max() > 0
    # the Vs block against dsa_iteration_system on the isotropic rows alone
    iso = fwd["col"] <= maxvp
    nin = int(iso.sum()); cap = nin + 7 * maxvp
    rw = np.zeros(cap, f); rw[:nin] = fwd["rw"][iso]
    col = np.zeros(cap, np.int32); col[:nin] = fwd["col"][iso]
    iw = np.zeros(2 * cap + 1, np.int32); iw[1:nin + 1] = fwd["iw"][iso]
    cbst = np.zeros(dall + maxvp, f); dwi = np.zeros(dall, f); norm = np.zeros(maxvp, f); dws = np.zeros(2, f)
    m, nar = C.c_int(0), C.c_longlong(0)
    assert lib.dsa_iteration_system(c["nx"], c["ny"], c["nz"], dall, nin, cap, _p(rw), _p(iw), _p(col), _p(obst), _p(fwd["dsurf"]), c["threshold0"], c["weight0"],
                                    _p(cbst), _p(dwi), _p(norm), C.byref(m), C.byref(nar), _p(dws)) == 0
    assert (bits(D["norm"][:maxvp]) == bits(norm)).all() and (bits(D["dws"][0]) == bits(dws)).all()
    for B in (1, 2):
        nb = D["norm"][B * maxvp:(B + 1) * maxvp]
        tot = f(0)
        for v in nb:
            tot = f(tot + v)
        assert (bits(D["dws"][B]) == bits(np.array([nb.max(), tot / f(maxvp)], f))).all()
    if weight_azi == float(c["weight0"]):
        # one weight: the trade-off sweep takes the resident joint matrix, and its member at (weight0, damp) is dsa_lsmr
        K = 2
        w = np.array([c["weight0"], 0.5 * c["weight0"]], f); d = np.array([damp, damp], f)
        x = np.zeros((K, D["n"]), f); meas = np.zeros((K, 3)); istop = np.zeros(K, np.int32); itn = np.zeros(K, np.int32); est = np.zeros((K, 5), f)
        call_solver(lib, eng, "dsa_lsmr_tradeoff", K, dall, _p(D["cbst"]), c["weight0"], _p(w), _p(d), *invert.LSMR_ARGS, _p(x), _p(meas), _p(istop), _p(itn), _p(est))
        assert (bits(x[0]) == bits(dev["x"])).all() and istop[0] == dev["istop"] and itn[0] == dev["itn"] and (bits(est[0]) == bits(dev["est"])).all()
        assert not (bits(x[1]) == bits(x[0])).all()
    # the host route on the same engine
    call_solver(lib, eng, "dsa_spmv_load", S["m"], S["n"], C.c_longlong(S["rw"].size), _p(S["rw"]), _p(S["row"]), _p(S["col"]))
    same_solves(dev, solve_on(lib, eng, S["b"], damp, S["n"], S["m"], 17))
    assert dev["itn"] > 3 and dev["x"][maxvp:].any()


# ---- 3. errors ----

def test_errors(host_rows):
    lib, c, fwd, obst = host_rows
    f = np.float32
    dall, maxvp = c["ndata"], c["nparpi"]
    vsf = np.asfortranarray(c["vels"].copy())
    cbst = np.zeros(dall + 3 * maxvp, f); dw = np.zeros(dall, f); norm = np.zeros(3 * maxvp, f); dws = np.zeros(6, f)
    m, nar = C.c_int(0), C.c_longlong(0)

    def joint(eng, w0=2.0, wa=0.05):
        return lib.dsa_iteration_system_azimuthal_device(eng, c["nx"], c["ny"], c["nz"], dall, _p(obst), _p(fwd["dsurf"]), c["threshold0"], w0, wa, _p(cbst), _p(dw),
                                                         _p(norm), C.byref(m), C.byref(nar), _p(dws))

    def iso(eng):
        return lib.dsa_iteration_system_device(eng, c["nx"], c["ny"], c["nz"], dall, _p(obst), _p(fwd["dsurf"]), c["threshold0"], c["weight0"], _p(cbst), _p(dw),
                                               _p(norm), C.byref(m), C.byref(nar), _p(dws))
    e = Engine(0)
    try:
        assert joint(e._h) == -5 and "azimuthal" in lib.dsa_error_string(e._h).decode()          # nothing resident
    finally:
        e.close()
    eng = lib.dsa_dropin_engine()
    invert.forward_rows(lib, c, vsf)                                                              # isotropic rows on the device
    assert joint(eng) == -5 and "isotropic" in lib.dsa_error_string(eng).decode()
    assert iso(eng) == 0                                                                          # ... which their own builder takes
    _, n, _ = invert.forward_rows(lib, c, vsf, entry="dsa_calsurfg_azimuthal")                    # azimuthal rows on the device
    assert n == fwd["nar"]
    assert iso(eng) == -5 and "azimuthal" in lib.dsa_error_string(eng).decode()
    for w0, wa in ((-1.0, 0.05), (2.0, -0.05), (float("nan"), 0.05), (2.0, float("nan")), (2.0, float("inf"))):
        assert joint(eng, w0, wa) == -2
    assert lib.dsa_iteration_system_azimuthal_device(eng, c["nx"], c["ny"], c["nz"], dall, None, _p(fwd["dsurf"]), c["threshold0"], 2.0, 0.05, _p(cbst), _p(dw),
                                                     _p(norm), C.byref(m), C.byref(nar), _p(dws)) == -2
    assert lib.dsa_iteration_system_azimuthal_device(eng, 2, c["ny"], c["nz"], dall, _p(obst), _p(fwd["dsurf"]), c["threshold0"], 2.0, 0.05, _p(cbst), _p(dw),
                                                     _p(norm), C.byref(m), C.byref(nar), _p(dws)) == -2
    assert joint(eng) == 0 and m.value == dall + 3 * maxvp                                       # the refusals left the rows alone
    assert joint(eng) == -5 and iso(eng) == -5                                                    # a built joint system is not rows to build from
    # dsa_calsurfg_azimuthal with only some of the three arrays
    nd = c["ndata"]; cap = 16
    iw = np.zeros(cap + 1, np.int32); rw = np.zeros(cap, f); col = np.zeros(cap, np.int32); dsurf = np.zeros(nd, f); na = C.c_int(0)
    head, tail = taipei._args(c)
    for arrays in ((None, _p(rw), _p(col)), (_p(iw), None, _p(col)), (_p(iw), _p(rw), None), (None, None, _p(col))):
        assert lib.dsa_calsurfg_azimuthal(*head, *arrays, _p(dsurf), *tail, C.byref(na)) == -2


# ---- 4. block PSFs ----

@pytest.fixture(scope="module")
def taipei_system():
    import inversion as inv
    c = taipei.load()
    return c, inv.build_system(c, L.call_boundary(load_library().dsa_calsurfg, c), c["obst"], 3.0, 4.0)


def blocks_numpy(x, coords, j, nblocks):
    """psf[B] = {x[B nb + cj], the three fp64 sums over block B measured from cell cj}"""
    nb = x.size // nblocks
    cj = j % nb
    out = np.zeros((nblocks, 4))
    for B in range(nblocks):
        xb = x[B * nb:(B + 1) * nb]
        out[B, 0] = xb[cj]
        out[B, 1:] = psf_numpy(xb, coords, cj)
    return out


def check_blocks(e, nd, n, nblocks, first, Rn, coords, damp, itnlim):
    plain = e.lsmr_resolution(nd, damp, spikes=(first, Rn), itnlim=itnlim)
    D = e.lsmr_resolution_blocks(nd, damp, nblocks, (first, Rn), coords, itnlim=itnlim)
    D2 = e.lsmr_resolution_blocks(nd, damp, nblocks, (first, Rn), coords, want_x=False, itnlim=itnlim)
    assert_all_equal(D, [realisation(plain, r) for r in range(Rn)])
    assert D2["x"] is None and (bits64(D2["psf"]) == bits64(D["psf"])).all()
    assert np.array_equal(D2["itn"], D["itn"]) and np.array_equal(D2["istop"], D["istop"])
    nb = n // nblocks
    assert D["psf"].shape == (Rn, nblocks, 4)
    for r in range(Rn):
        want = blocks_numpy(D["x"][r], coords, first + r, nblocks)
        assert (D["psf"][r, :, 0] == want[:, 0]).all(), r
        np.testing.assert_allclose(D["psf"][r, :, 1:], want[:, 1:], rtol=1e-9, atol=0, err_msg=str(r))
    assert D["psf"][:, :, 1].min() >= 0 and D["psf"][:, :, 1].max() > 0
    return plain, D


def test_block_psfs_taipei(taipei_system):
    """n = 2048, spikes (1000, 130): nblocks = 1 is dsa_lsmr_resolution bit for bit, psf included; nblocks = 2 has exactly one chunk per block"""
    c, S = taipei_system
    n, nd = S["n"], c["ndata"]
    coords = invert.unknown_coords(c)
    first, Rn = 1000, 130
    e = Engine(0)
    try:
        load(e, S)
        ref = e.lsmr_resolution(nd, 1.0, spikes=(first, Rn), coords=coords)
        plain, D1 = check_blocks(e, nd, n, 1, first, Rn, coords, 1.0, 400)
        assert (bits64(D1["psf"].reshape(Rn, 4)) == bits64(ref["psf"])).all()
        assert_all_equal(D1, [realisation(ref, r) for r in range(Rn)])
        check_blocks(e, nd, n, 2, first, Rn, coords[:1024], 1.0, 400)
        # argument errors
        for args, code in (((0, (first, Rn), coords), -2), ((3, (first, Rn), coords[:682]), -2), ((2, (-1, 4), coords[:1024]), -2),
                           ((2, (n - 3, 4), coords[:1024]), -2), ((2, (first, 0), coords[:1024]), -2), ((2, (first, 4), None), -2)):
            with pytest.raises(EngineError) as exc:
                e.lsmr_resolution_blocks(nd, 1.0, *args)
            assert exc.value.code == code, args
        with pytest.raises(EngineError) as exc:
            e.lsmr_resolution_blocks(0, 1.0, 2, (first, 4), coords[:1024])
        assert exc.value.code == -2
        istop = np.zeros(4, np.int32); itn = np.zeros(4, np.int32); est = np.zeros((4, 5), np.float32); psf = np.zeros((4, 2, 4))
        xyz = np.ascontiguousarray(coords[:1024])
        for out in ((None, _p(istop), _p(itn), _p(est)), (_p(psf), None, _p(itn), _p(est)), (_p(psf), _p(istop), None, _p(est)), (_p(psf), _p(istop), _p(itn), None)):
            assert e._L.dsa_resolution_blocks(e._h, 4, nd, 2, first, _p(xyz), 1.0, *invert.LSMR_ARGS, None, *out) == -2
    finally:
        e.close()
    fresh = Engine(0)
    try:
        with pytest.raises(EngineError) as exc:                 # no matrix
            fresh._mn = (1, 2)
            fresh.lsmr_resolution_blocks(1, 1.0, 2, (0, 1), coords[:1])
        assert exc.value.code == -5
    finally:
        fresh.close()


def test_block_psfs_ragged_chunks_and_a_block_boundary():
    """n = 3300 in three blocks of 1100 cells (a full chunk and a ragged one of 76); spikes 1060 .. 1139 cross the boundary between blocks 0
    and 1 and a lane group; itnlim 35; the coordinates of the cells are made up"""
    M = SM.system(3000, 15, 11, 20, seed=5)
    n, nd = M["n"], 3000
    assert n == 3300
    rng = np.random.default_rng(8)
    coords = np.column_stack([24.0 + 0.9 * rng.random(1100), 121.0 + 0.8 * rng.random(1100), np.repeat(np.arange(20) * 2.5, 55)])
    e = Engine(0)
    try:
        e.spmv_load(M["m"], n, M["rw"], M["row"], M["col"])
        plain, D = check_blocks(e, nd, n, 3, 1060, 80, coords, 0.3, 35)
    finally:
        e.close()
    assert D["itn"].max() > 5
    # a spike's own block holds R_jj: psf[r, block of j, 0] = x_r[j]
    for r in (0, 39, 40, 79):
        j = 1060 + r
        assert D["psf"][r, j // 1100, 0] == D["x"][r, j]


def test_block_psfs_of_a_column_without_data():
    """every data entry of one column removed: its spike has b = 0 -> x = 0 and all-zero rows in every block"""
    M = SM.system(600, 6, 5, 4, seed=3)
    n, nd = M["n"], 600
    data = M["row"] <= nd
    j0 = int(np.argmax(np.bincount(M["col"][data] - 1, minlength=n)))
    keep = ~((M["col"] == j0 + 1) & data)
    coords = np.column_stack([24.0 + 0.01 * np.arange(n // 2), 121.0 + 0.02 * (np.arange(n // 2) % 7), 3.0 * (np.arange(n // 2) // 30)])
    first = max(0, j0 - 1)
    Rn = min(3, n - first)
    e = Engine(0)
    try:
        e.spmv_load(M["m"], n, M["rw"][keep], M["row"][keep], M["col"][keep])
        D = e.lsmr_resolution_blocks(nd, 0.5, 2, (first, Rn), coords)
    finally:
        e.close()
    r0 = j0 - first
    assert D["itn"][r0] == 0 and D["istop"][r0] == 0 and not D["x"][r0].any() and not D["psf"][r0].any()
    assert D["psf"][r0 ^ 1].any()


# ---- 5. the driver ----

def write_directory(path, c, vel_obs):
    """DSurfTomo.in, the data file and MOD of a boundary case (Rayleigh and Love phase / group slots as the case has them), the way
    dsurftomo_amd.io.load reads them; the case that load() returns from it is the case of the test"""
    kmax = c["kmax"]
    per = [c["tRc"], c["tRg"], c["tLc"], c["tLg"]]
    lines = ["c", "c", "c", "surfdata.dat", "%d %d %d" % (c["nx"], c["ny"], c["nz"]), "%.6f %.6f" % (c["goxd"], c["gozd"]), "%.6f %.6f" % (c["dvxd"], c["dvzd"]),
             "%d" % max(c["nsrcsurf"], c["nrcf"]), "2.0 0.5", "%.6f" % c["minthk"], "1.5 5.5", "1", "1.0"]
    for p in per:
        lines += ["%d" % len(p)] + ([" ".join("%g" % t for t in p)] if len(p) else [])
    lines += ["0", "0.02", "1.2"]
    (path / "DSurfTomo.in").write_text("\n".join(lines) + "\n")
    deg = lambda r: float(r) * 180.0 / np.pi
    out, q = [], 0
    for slot in range(kmax):
        for s in range(int(c["nsrcsurf1"][slot])):
            out.append("# %.7f %.7f %d %d %d" % (90.0 - deg(c["scxf"][s, slot]), deg(c["sczf"][s, slot]), c["periods"][s, slot], c["wavetype"][s, slot], c["igrt"][s, slot]))
            for k in range(int(c["nrc1"][s, slot])):
                out.append("%.7f %.7f %.6f" % (90.0 - deg(c["rcxf"][k, s, slot]), deg(c["rczf"][k, s, slot]), vel_obs[q]))
                q += 1
    (path / "surfdata.dat").write_text("\n".join(out) + "\n")
    vels = np.asarray(c["vels"])
    mod = [" ".join("%.3f" % d for d in c["depz"])]
    for k in range(c["nz"]):
        for j in range(c["ny"]):
            mod.append(" ".join("%.5f" % vels[i, j, k] for i in range(c["nx"])))
    (path / "MOD").write_text("\n".join(mod) + "\n")


def test_driver(tmp_path):
    """anisotropy.main on a small directory: Azim.dat == the host route's bytes (invert.azimuthal_step + write_azimuthal on the same model),
    AzimResolution.dat == the NumPy restatement from dsa_lsmr_resolution with x returned, every checkerboard file's recovered blocks ==
    dsa_lsmr on b = A model"""
    src, out = tmp_path / "case", tmp_path / "out"
    src.mkdir(); out.mkdir()
    c0 = joint_case()
    r = synth.LCG(5)
    write_directory(src, c0, 3.0 * (1.0 + 0.05 * (r.uniform(c0["ndata"]) - 0.5)))
    c = taipei.load(str(src))
    assert c["ndata"] == c0["ndata"] and c["nparpi"] == 168 and c["kRc"] == 3 and c["kRg"] == 1 and c["kLc"] == 1
    log = []
    assert A.main([str(src), "--model", "MOD", "--out", str(out), "--resolution", "--checkerboard", "2,2,1"]) == 0
    names = ["DSurfTomo.inAzim.dat", "DSurfTomo.inAzimResolution.dat"] + ["DSurfTomo.inAzimChecker.dat.k01." + b for b in A.BLOCKS]
    assert sorted(os.listdir(out)) == sorted(names)
    # the host route on the same model
    lib = invert.bind(load_library())
    vsf = np.asfortranarray(c["vels"].copy())
    obst = np.ascontiguousarray(c["obst"])
    host = invert.azimuthal_step(lib, c, vsf, obst, log.append)
    invert.write_azimuthal(str(tmp_path / "want_azim.dat"), c, vsf, host["gc"], host["gs"])
    assert (out / names[0]).read_bytes() == (tmp_path / "want_azim.dat").read_bytes()
    assert host["itn"] > 3 and (host["datweight"] == 0).any() and np.abs(host["gc"]).max() > 0
    # the host system is resident now (azimuthal_step's dsa_spmv_load): spikes with x returned, and the test models one by one
    S = host["system"]
    n, nd, maxvp, damp = S["n"], c["ndata"], c["nparpi"], float(c["damp"])
    eng = lib.dsa_dropin_engine()
    x = np.zeros((n, n), np.float32); istop = np.zeros(n, np.int32); itn = np.zeros(n, np.int32); est = np.zeros((n, 5), np.float32)
    call_solver(lib, eng, "dsa_lsmr_resolution", n, nd, None, 0, None, C.c_float(damp), *invert.LSMR_ARGS, _p(x), None, _p(istop), _p(itn), _p(est))
    coords = invert.unknown_coords(c)
    want = np.stack([blocks_numpy(x[j], coords, j, 3) for j in range(n)])
    col = A.block_psf_columns(want)
    rows = A.read_azim_resolution(str(out / names[1]))
    assert len(rows) == n and [q["block"] for q in rows] == col["block"].tolist()
    assert [q["rjj"] for q in rows] == col["rjj"].tolist()
    assert [q["colocated_a"] for q in rows] == col["colocated"][:, 0].tolist() and [q["colocated_b"] for q in rows] == col["colocated"][:, 1].tolist()
    for key, val in (("psf_h_km", col["psf_h_km"]), ("psf_v_km", col["psf_v_km"]), ("share_a", col["share"][np.arange(n), col["others"][:, 0]]),
                     ("share_b", col["share"][np.arange(n), col["others"][:, 1]])):
        np.testing.assert_allclose([q[key] for q in rows], val, rtol=1e-9, atol=0, err_msg=key)
    models = A.azimuthal_checkerboards(c, (2, 2, 1))
    for B, name in enumerate(A.BLOCKS):
        b = np.zeros(S["m"], np.float32)
        assert lib.dsa_spmv(eng, 1, _p(models[B]), _p(b)) == 0
        b[nd:] = 0.0
        sol, _, _, _ = invert.lsmr(lib, eng, b, damp, n)
        got = A.read_azim_checker(str(out / ("DSurfTomo.inAzimChecker.dat.k01." + name)))
        rec = np.array([[q["out_vs"], q["out_gc"], q["out_gs"]] for q in got], np.float32).T.ravel()
        assert (bits(rec) == bits(sol)).all(), name
        assert (np.array([[q["in_vs"], q["in_gc"], q["in_gs"]] for q in got], np.float32).T.ravel() == models[B]).all()
