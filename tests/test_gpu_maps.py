"""Period-by-period 2-D maps on the device: dsa_solve_rows_maps, dsa_iteration_system_maps_device, dsa_update_maps,
dsa_get_maps and the loop of dsurftomo_amd.maps.

The map rows are held against the existing emitters under a depth factor of exactly 1.0 (one layer, sen_vs = 1, sen_vp = sen_rho = 0,
vels = 2: S = (0 a + 0 r) + 1 and Sazi = 1 * (double)(0.5f * 2.0f) are both 1.0), bit for bit; the system against the NumPy route
(analyses.azimuthal's quartile weights, maps.laplacian_rows_2d, dsa_spmv_load) bit for bit, dsa_lsmr's solution included; the update
against dsa_set_maps of the host twin's values bit for bit.  The two recoveries are consistency checks of the chain against SciPy's fp64
LSMR on the same assembled system (section 18's kind) and through maps.iterate.  Shapes of test_gpu_azimuthal.py: 35 x 35 vertices,
dicing 8, 6 sources x 2 maps x 48 receivers = 576 rays.  Every test uses engines of its own; the host rows of the smooth maps are made
once for the module.
"""
import ctypes as C

import numpy as np
import pytest

import synth
import test_gpu_azimuthal as TA
from dsurftomo_amd import maps as M
from dsurftomo_amd.analyses.azimuthal import azimuthal_weights
from dsurftomo_amd.analyses.common import LSMR_ARGS, _p
from dsurftomo_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu
bits = TA.bits
NX, GD = TA.NX, TA.GD
NVX = NX - 2
LAYER = NVX * NVX
NMAPS = 2
F = np.float32
GEOM = (NX, NX, synth.GOXD, synth.GOZD, synth.DVD, synth.DVD)
SLAB, VLIST = NX * NX, LAYER
PER_RAY = {True: (3 * SLAB + VLIST) * 4 + 32, False: (SLAB + VLIST) * 4 + 32}      # Engine::trace_chunk's budget per ray


def unit_depth_model():
    """depth kernels under which every depth factor is exactly 1.0: nz = 2 (one layer), kmax = 2"""
    ncol = NX * NX
    vels = np.full((2, NX, NX), 2.0, F)
    depz = np.array([0.0, 10.0], F)
    return vels, depz, np.ones((2, 2, ncol)), np.zeros((2, 2, ncol)), np.zeros((2, 2, ncol))


def fresh(pv=None, u=None, depth=False):
    e = Engine(0)
    u = TA.plan() if u is None else u
    e.set_maps(*GEOM, TA.maps() if pv is None else pv, dicing=GD)
    if depth:
        e.set_depth_kernels(*unit_depth_model())
    e.plan(u["map_index"], u["scx"], u["scz"], u["nrec"], u["rcx"], u["rcz"], sen_slot=u["map_index"] if depth else None)
    return e, u


def map_cols(col, iw, u, blocks):
    """the map columns of the existing emitters' entries under nz = 2: their col = B * layer + i + 1 -> (B * nmaps + m) * layer + i + 1"""
    m = M.datum_maps(u)[iw - 1]
    B = (col - 1) // LAYER
    assert B.max() == blocks - 1
    return ((B * NMAPS + m) * LAYER + (col - B * LAYER)).astype(np.int32)


def same_rows(a, b):
    assert a[1].size == b[1].size > 0
    assert (bits(a[0]) == bits(b[0])).all(), "dsurf"
    assert (bits(a[1]) == bits(b[1])).all(), "rw"
    assert (a[2] == b[2]).all() and (a[3] == b[3]).all()


# ---- 1. rows ----

@pytest.mark.parametrize("lanes", [1, 4])
def test_map_rows_equal_the_existing_emitters_under_a_unit_depth_factor(lanes):
    e, u = fresh(depth=True)
    try:
        cap = TA.capacity(u)
        iso0 = e.solve_rows(cap)
        assert e.stats()["rays"] == 576
        e.set_option("ray_lanes", lanes)
        for azimuthal in (True, False):
            e.set_option("ray_budget", 200 * PER_RAY[azimuthal])
            want = e.solve_rows_azimuthal(cap) if azimuthal else e.solve_rows(cap)
            assert e.stats()["ray_launches"] == 3
            az_want = e.ray_azimuths() if azimuthal else None
            got = e.solve_rows_maps(cap, azimuthal)
            st = e.stats()
            assert st["ray_launches"] == 3 and st["rays"] == 576 and st["nar"] == got[1].size
            same_rows(got, (want[0], want[1], want[2], map_cols(want[3], want[2], u, 3 if azimuthal else 1)))
            assert got[3].min() >= 1 and got[3].max() <= (3 if azimuthal else 1) * NMAPS * LAYER
            assert (np.diff(got[2]) >= 0).all()
            if azimuthal:
                az = e.ray_azimuths()
                assert (az[0] == az_want[0]).all() and (az[1] == az_want[1]).all() and (bits(az[2]) == bits(az_want[2])).all()
                assert ((got[3] - 1) // (NMAPS * LAYER)).max() == 2
                # the rows left on the device: the same count, and exactly enough room / one entry short
                t, nar = e.solve_rows_maps_device(True)
                assert nar == got[1].size and (bits(t) == bits(got[0])).all()
                e.solve_rows_maps_device(True, capacity=nar)
                with pytest.raises(EngineError) as exc:
                    e.solve_rows_maps_device(True, capacity=nar - 1)
                assert exc.value.code == -6
            else:
                with pytest.raises(EngineError) as exc:          # an isotropic map solve leaves no sums
                    e.ray_azimuths()
                assert exc.value.code == -5
        keep = got
        # the plain call afterwards gives what it gave before
        e.set_option("ray_lanes", 0); e.set_option("ray_budget", 0)
        same_rows(e.solve_rows(cap), iso0)
    finally:
        e.close()
    # a fresh engine that never saw depth kernels gives the same map rows
    e2, _ = fresh()
    try:
        e2.set_option("ray_lanes", lanes)
        same_rows(e2.solve_rows_maps(cap, False), keep)
        got3 = e2.solve_rows_maps(cap, True)
        iso = got3[3] <= NMAPS * LAYER
        same_rows((got3[0], got3[1][iso], got3[2][iso], got3[3][iso]), keep)
    finally:
        e2.close()


# ---- 2. the system ----

@pytest.fixture(scope="module")
def smooth_rows():
    """the three-block map rows and the times of the smooth maps on the standard plan, fetched to the host: once for the module"""
    e, u = fresh()
    try:
        t, rw, iw, col = e.solve_rows_maps(TA.capacity(u), True)
    finally:
        e.close()
    return dict(u=u, t=t, rw=rw, iw=iw, col=col)


def lsmr_on(e, b, damp):
    return e.lsmr(b, damp, *LSMR_ARGS)


@pytest.mark.parametrize("nblocks,weight_azi", [(1, 2.0), (3, 0.05)])
def test_system_equals_the_host_route(smooth_rows, nblocks, weight_azi):
    R = smooth_rows
    u, dsyn = R["u"], R["t"]
    sel = R["col"] <= nblocks * NMAPS * LAYER
    rw, iw, col = R["rw"][sel], R["iw"][sel], R["col"][sel]
    dall, n = dsyn.size, nblocks * NMAPS * LAYER
    r = synth.LCG(91)
    obst = (dsyn * (1.0 + 0.04 * (r.uniform(dall) - 0.5))).astype(F)
    threshold0, weight0, damp = F(1.2), F(2.0), 0.5
    e, _ = fresh()
    try:
        t, nar = e.solve_rows_maps_device(nblocks == 3)
        assert nar == rw.size and (bits(t) == bits(dsyn)).all()
        D = e.iteration_system_maps_device(NX, NX, NMAPS, nblocks, obst, dsyn, threshold0, weight0, weight_azi)
        dev = lsmr_on(e, D["cbst"], damp)
        res = (obst - dsyn).astype(F)
        dw = azimuthal_weights(res, threshold0)
        assert 0 < int((dw == 0).sum()) < dall
        S = M.map_system(NX, NX, NMAPS, nblocks, rw, iw, col, res, dw, weight0, weight_azi)
        assert D["m"] == S["m"] == dall + n and D["n"] == S["n"] == n and D["nar"] == S["rw"].size
        assert (bits(D["datweight"]) == bits(dw)).all() and (bits(D["cbst"]) == bits(S["b"])).all()
        want_norm = np.zeros(n, F)
        scaled = np.abs(S["rw"][:rw.size])
        for k in range(rw.size):
            j = col[k] - 1
            want_norm[j] = want_norm[j] + scaled[k]
        assert (bits(D["norm"]) == bits(want_norm)).all() and want_norm[-NMAPS * LAYER:].max() > 0
        per = NMAPS * LAYER
        for B in range(nblocks):
            nb = D["norm"][B * per:(B + 1) * per]
            tot = F(0)
            for v in nb:
                tot = F(tot + v)
            assert (bits(D["dws"][B]) == bits(np.array([nb.max(), tot / F(per)], F))).all()
        # the host route on the same engine
        e.spmv_load(S["m"], S["n"], S["rw"], S["row"], S["col"])
        host = lsmr_on(e, S["b"], damp)
        assert (bits(dev["x"]) == bits(host["x"])).all() and dev["itn"] == host["itn"] and dev["istop"] == host["istop"]
        assert dev["itn"] > 3 and dev["x"][-per:].any()
    finally:
        e.close()


# ---- 3. the update ----

def test_update_maps_equals_set_maps_of_the_twin():
    pv = TA.maps()
    u = TA.plan(nsrc=3, nper=2, nrec=24)
    r = synth.LCG(12)
    dv = (1.6 * (r.uniform(NMAPS * LAYER) - 0.5)).astype(F).reshape(NMAPS, LAYER)        # +-0.8: elements beyond +-dvmax
    dvmax, minvel, maxvel = 0.5, 2.75, 3.0
    v0 = pv.astype(F).reshape(NMAPS, NX * NX)
    want = M.update_maps_twin(v0, dv, dvmax, minvel, maxvel, NX, NX)
    inner = want.reshape(NMAPS, NX, NX)[:, 1:-1, 1:-1]
    assert (np.abs(dv) > dvmax).any() and (inner == F(minvel)).any() and (inner == F(maxvel)).any() and ((inner > F(minvel)) & (inner < F(maxvel))).any()
    a, _ = fresh(pv, u)
    b = Engine(0)
    try:
        assert (bits(a.get_maps(NMAPS, NX, NX)) == bits(v0)).all()
        with pytest.raises(ValueError):                         # the binding refuses a step of another size: the library would read past it
            a.update_maps(dv[:, :-1], dvmax, minvel, maxvel, NMAPS, NX, NX)
        a.update_maps(dv, dvmax, minvel, maxvel, NMAPS, NX, NX)
        with pytest.raises(EngineError) as exc:                  # the plan was dropped
            a.solve()
        assert exc.value.code == -5
        a.plan(u["map_index"], u["scx"], u["scz"], u["nrec"], u["rcx"], u["rcz"])
        b.set_maps(*GEOM, want.astype(np.float64), dicing=GD)
        b.plan(u["map_index"], u["scx"], u["scz"], u["nrec"], u["rcx"], u["rcz"])
        assert (bits(a.get_maps(NMAPS, NX, NX)) == bits(want)).all() and (bits(b.get_maps(NMAPS, NX, NX)) == bits(want)).all()
        for m in range(NMAPS):
            assert (bits(a.velocity(m)) == bits(b.velocity(m))).all()
        ta, tb = a.solve(), b.solve()
        assert ta.size == 144 and ta.min() > 0 and (bits(ta) == bits(tb)).all()
    finally:
        a.close(); b.close()


# ---- 4. errors ----

def test_errors():
    """the error codes of the four entry points that the public interface can reach, and the engine usable afterwards.  Not covered, because
    no test shape reaches them: more than 2^31-1 columns (dsa_solve_rows_maps) or rows (the builder's dall + n), the builder's
    DSA_ERR_CAPACITY (more than 2^31-1 entries), and the DSA_ERR_STATE of several engines sharing a call (set only inside the drop-in)"""
    u = TA.plan(nsrc=2, nper=2, nrec=8)
    dall = int(u["nrec"].sum())
    e = Engine(0)
    try:
        L, h = e._L, e._h
        nar = C.c_longlong(0)
        out = np.zeros(dall, F); rw = np.zeros(100000, F); iw = np.zeros(100000, np.int32); col = np.zeros(100000, np.int32)
        rows = lambda azi, a, b, c, cap=100000: L.dsa_solve_rows_maps(h, azi, _p(out), a, b, c, C.c_longlong(cap), C.byref(nar))
        n1, n3 = NMAPS * LAYER, 3 * NMAPS * LAYER
        cbst = np.zeros(dall + n3, F); dw = np.zeros(dall, F); norm = np.zeros(n3, F); dws = np.zeros(6, F); m = C.c_int(0); no = C.c_longlong(0)
        obst = np.ones(dall, F); dsyn = np.ones(dall, F)

        def system(nblocks=1, nx=NX, ny=NX, nmaps=NMAPS, w0=2.0, wa=0.05, obs=obst, d=dall):
            return L.dsa_iteration_system_maps_device(h, nx, ny, nmaps, nblocks, d, _p(obs), _p(dsyn), 1.2, w0, wa, _p(cbst), _p(dw), _p(norm), C.byref(m), C.byref(no), _p(dws))
        dv = np.zeros((NMAPS, LAYER), F)
        # no maps
        assert rows(0, _p(rw), _p(iw), _p(col)) == -5
        assert L.dsa_update_maps(h, NMAPS, _p(dv), 0.5, 1.0, 5.0) == -5 and L.dsa_get_maps(h, NMAPS, _p(np.zeros(NMAPS * NX * NX, F))) == -5
        e.set_maps(*GEOM, TA.maps(), dicing=GD)
        assert rows(0, _p(rw), _p(iw), _p(col)) == -5                                       # no plan
        assert system() == -5                                                                # nothing resident
        e.plan(u["map_index"], u["scx"], u["scz"], u["nrec"], u["rcx"], u["rcz"])
        assert rows(2, _p(rw), _p(iw), _p(col)) == -2 and rows(-1, None, None, None) == -2   # azimuthal not 0 / 1
        for arrays in ((None, _p(iw), _p(col)), (_p(rw), None, _p(col)), (_p(rw), _p(iw), None), (None, None, _p(col))):
            assert rows(0, *arrays) == -2
        assert rows(0, _p(rw), _p(iw), _p(col), cap=10) == -6
        assert rows(0, _p(rw), _p(iw), _p(col)) == 0 and nar.value > 0                       # the refusals left the engine usable
        host = (rw[:nar.value].copy(), iw[:nar.value].copy(), col[:nar.value].copy())
        assert system() == -5                                                                # host rows: still nothing resident
        assert rows(0, None, None, None) == 0 and nar.value == host[0].size
        # the builder's arguments, all before the device: the rows survive every refusal
        assert system(nblocks=3) == -5 and system(nblocks=2) == -2 and system(nblocks=0) == -2
        assert system(nx=2) == -2 and system(ny=2) == -2 and system(nmaps=0) == -2 and system(d=0) == -2 and system(obs=None) == -2
        assert system(nx=NX - 1) == -2 and system(nmaps=NMAPS + 1) == -2
        for w0, wa in ((-1.0, 0.05), (2.0, -0.05), (float("nan"), 0.05), (2.0, float("inf"))):
            assert system(w0=w0, wa=wa) == -2
        assert system(d=3) == -2                                                             # too few data for the quartile rule
        assert system() == 0 and m.value == dall + n1
        assert system() == -5 and "already" in L.dsa_error_string(h).decode()                # a built system is not rows to build from
        iso = L.dsa_iteration_system_device(h, NX, NX, 2, dall, _p(obst), _p(dsyn), 1.2, 2.0, _p(cbst), _p(dw), _p(norm), C.byref(m), C.byref(no), _p(dws))
        assert iso == -5
        assert rows(1, None, None, None) == 0
        assert system(nblocks=1) == -5 and system(nblocks=3) == 0 and m.value == dall + n3
        # the update's arguments
        for args in ((NMAPS + 1, _p(dv), 0.5, 1.0, 5.0), (NMAPS, _p(dv), 0.0, 1.0, 5.0), (NMAPS, _p(dv), -0.5, 1.0, 5.0), (NMAPS, _p(dv), float("nan"), 1.0, 5.0),
                     (NMAPS, _p(dv), float("inf"), 1.0, 5.0), (NMAPS, _p(dv), 0.5, 5.0, 1.0), (NMAPS, None, 0.5, 1.0, 5.0)):
            assert L.dsa_update_maps(h, *args) == -2, args
        assert L.dsa_get_maps(h, NMAPS + 1, _p(np.zeros(3 * NX * NX, F))) == -2 and L.dsa_get_maps(h, NMAPS, None) == -2
        # still usable: the same host rows as before
        assert rows(0, _p(rw), _p(iw), _p(col)) == 0 and nar.value == host[0].size
        assert (bits(rw[:nar.value]) == bits(host[0])).all() and (col[:nar.value] == host[2]).all()
    finally:
        e.close()


# ---- 5. recovery, linear ----

# What fp32 LSMR on the device showed against SciPy's fp64 LSMR on the same assembled system in the first run of the recoveries below
# (DESIGN.md section 20): (device figure, SciPy figure); the tests allow the device to exceed SciPy by twice the observed excess.
RECOVERY_WEIGHT, RECOVERY_DAMP, RECOVERY_THRESHOLD = 1.0, 0.01, 1000.0
# iso: 0.000608637 km/s against 0.000608634 (the anomaly's rms over those vertices: 0.031810), itn 136; with the 2psi blocks: 0.003396980
# against 0.003396976 km/s, itn 245, and a median fast-axis error of 0.639710 against 0.639696 degrees.
OBSERVED = {"iso_rms": (0.000608637, 0.000608634), "azi_rms": (0.003396980, 0.003396976), "azi_axis_deg": (0.639710, 0.639696)}


def gaussian_dc(sign_by_map=(1.0, -1.0), percent=3.0, sigma=5.0):
    """(NMAPS, LAYER) float64: a Gaussian of `percent` of 2.8 km/s in the middle of each map, sigma in vertex spacings, +, - by map (so
    that the pooled residuals have both signs and the quartile rule keeps the data)"""
    j, i = np.meshgrid(np.arange(NVX), np.arange(NVX), indexing="ij")
    g = np.exp(-0.5 * ((i - (NVX - 1) / 2.0) ** 2 + (j - (NVX - 1) / 2.0) ** 2) / sigma ** 2).ravel()
    return np.stack([s * 0.01 * percent * 2.8 * g for s in sign_by_map])


def allowed(key, err_ref):
    dev, ref = OBSERVED[key]
    return err_ref + 2.0 * max(dev - ref, 0.0)


@pytest.mark.parametrize("azimuthal", [False, True])
def test_linear_recovery_against_scipy(smooth_rows, azimuthal):
    import scipy.sparse as sp
    from scipy.sparse.linalg import lsmr
    R = smooth_rows
    nblocks = 3 if azimuthal else 1
    per = NMAPS * LAYER
    n = nblocks * per
    sel = R["col"] <= n
    rw, iw, col = R["rw"][sel], R["iw"][sel], R["col"][sel]
    dsyn = R["t"]
    dall = dsyn.size
    G = sp.csr_matrix((rw.astype(np.float64), (iw - 1, col - 1)), shape=(dall, n))
    truth = np.zeros(n)
    truth[:per] = gaussian_dc().ravel()
    axis0 = 30.0
    if azimuthal:
        a = 0.02 * 2.8
        truth[per:2 * per] = a * np.cos(np.radians(2 * axis0)); truth[2 * per:] = a * np.sin(np.radians(2 * axis0))
    obst = (dsyn.astype(np.float64) + G @ truth).astype(F)
    e, _ = fresh()
    try:
        e.solve_rows_maps_device(azimuthal)
        D = e.iteration_system_maps_device(NX, NX, NMAPS, nblocks, obst, dsyn, RECOVERY_THRESHOLD, RECOVERY_WEIGHT, RECOVERY_WEIGHT)
        dev = lsmr_on(e, D["cbst"], RECOVERY_DAMP)
    finally:
        e.close()
    assert D["datweight"].mean() > 0.9
    S = M.map_system(NX, NX, NMAPS, nblocks, rw, iw, col, (obst - dsyn).astype(F), D["datweight"], RECOVERY_WEIGHT, RECOVERY_WEIGHT)
    A = sp.csr_matrix((S["rw"].astype(np.float64), (S["row"] - 1, S["col"] - 1)), shape=(S["m"], S["n"]))
    atol, btol, conlim, itnlim, _ = LSMR_ARGS
    x = lsmr(A, S["b"].astype(np.float64), damp=RECOVERY_DAMP, atol=atol, btol=btol, conlim=conlim, maxiter=itnlim)[0]
    dws = D["norm"][:per]
    cells = dws > np.median(dws)
    rms = lambda v: float(np.sqrt(np.mean(np.square(v))))
    err_ref, err_dev, size = rms((x - truth)[:per][cells]), rms((dev["x"].astype(np.float64) - truth)[:per][cells]), rms(truth[:per][cells])
    key = "azi_rms" if azimuthal else "iso_rms"
    print("map recovery (%s): rms error of c0 over %d vertices: scipy fp64 %.9f km/s, device fp32 %.9f km/s, rms of the anomaly %.6f km/s; device itn %d istop %d" %
          (key, int(cells.sum()), err_ref, err_dev, size, dev["itn"], dev["istop"]))
    if azimuthal:
        def axis_err(v):
            d = np.abs(M.fast_axis(v[per:2 * per], v[2 * per:]) - axis0) % 180.0
            return float(np.median(np.minimum(d, 180.0 - d)[cells]))
        ax_ref, ax_dev = axis_err(x), axis_err(dev["x"].astype(np.float64))
        print("map recovery (azi_axis_deg): median fast-axis error: scipy fp64 %.6f deg, device fp32 %.6f deg" % (ax_ref, ax_dev))
    assert err_ref < 0.5 * size, "the yardstick itself must recover the anomaly"
    assert err_dev <= allowed(key, err_ref)
    if azimuthal:
        assert ax_ref < 5.0, "the yardstick itself must recover the axis"
        assert ax_dev <= allowed("azi_axis_deg", ax_ref)


# ---- 6. recovery, nonlinear ----

def test_nonlinear_recovery_through_the_loop():
    """true maps = smooth maps + the Gaussian; obst their times; three iterations of maps.iterate from the smooth maps.  Conditions, not
    measurements; what the first run showed: weighted rms residual 0.06429 -> 0.00103 -> 0.00016 -> 0.00009 s (ratio
    last / first 0.0015), rms map error over the 1089 well-covered vertices 0.000210 km/s of 0.031749 at the start (ratio 0.0066)"""
    u = TA.plan()
    smooth = TA.maps().astype(F).reshape(NMAPS, NX * NX)
    dc = gaussian_dc()
    true = smooth.astype(np.float64).reshape(NMAPS, NX, NX).copy()
    true[:, 1:-1, 1:-1] += dc.reshape(NMAPS, NVX, NVX)
    t_eng, _ = fresh(true.reshape(NMAPS, -1), u)
    try:
        obst = t_eng.solve()
    finally:
        t_eng.close()
    e, _ = fresh(None, u)
    log = []
    try:
        out = M.iterate(e, u, NX, NX, NMAPS, obst, 3, RECOVERY_WEIGHT, RECOVERY_DAMP, RECOVERY_THRESHOLD, 0.5, 1.0, 6.0, log=log.append)
        final = e.solve()
        got = e.get_maps(NMAPS, NX, NX)
    finally:
        e.close()
    res = (obst - final).astype(F)
    w = azimuthal_weights(res, RECOVERY_THRESHOLD).astype(np.float64)
    rms = [h["rms"] for h in out["history"]] + [float(np.sqrt((np.square(res.astype(np.float64) * w)).sum() / w.sum()))]
    cells = (out["norm"] > np.median(out["norm"])).reshape(NMAPS, NVX, NVX)
    err = (got.astype(np.float64).reshape(NMAPS, NX, NX) - true)[:, 1:-1, 1:-1][cells]
    err0 = dc.reshape(NMAPS, NVX, NVX)[cells]
    e1, e0 = float(np.sqrt(np.mean(err ** 2))), float(np.sqrt(np.mean(err0 ** 2)))
    print("nonlinear map recovery: rms residual %s s (ratio last / first %.4f); rms map error over %d vertices %.6f km/s of %.6f at the start (ratio %.4f)" %
          (" ".join("%.5f" % r for r in rms), rms[-1] / rms[0], int(cells.sum()), e1, e0, e1 / e0))
    assert len(log) == 3 * (1 + NMAPS) and all(h["itn"] > 0 for h in out["history"])
    assert all(b < a for a, b in zip(rms, rms[1:])), rms
    assert e1 < e0


# ---- 7. the driver ----

@pytest.mark.parametrize("start,azimuthal", [("mean", False), ("model", True)])
def test_driver_on_the_taipei_example(tmp_path, start, azimuthal):
    """maps.run on tests/golden/taipei, two iterations: one line per (period, interior vertex) in the reference's period order, c0 the
    engine's resident maps inside the input file's [minvel, maxvel], the DWS of the last system, the 2psi columns with --azimuthal; the
    weighted rms residual falls from the first iteration to the second"""
    from dsurftomo_amd import io
    c = io.load()
    log = []
    out, path = M.run(io.HERE, start=start, iterations=2, azimuthal=azimuthal, azimuthal_weight=20.0 if azimuthal else None, out_dir=str(tmp_path), log=log.append)
    rows = M.read_maps(path)
    layer, per = (c["nx"] - 2) * (c["ny"] - 2), M.period_list(c)
    assert len(rows) == len(per) * layer and path.endswith("DSurfTomo.inMaps.dat")
    assert [(r["wave"], r["kind"], r["period"]) for r in rows[::layer]] == per
    inner = out["velv"].reshape(len(per), c["ny"], c["nx"])[:, 1:-1, 1:-1].ravel()
    assert [r["c0"] for r in rows] == inner.astype(np.float64).tolist()
    assert np.isfinite(inner).all() and inner.min() >= c["minvel"] and inner.max() <= c["maxvel"]
    assert [r["dws"] for r in rows] == out["norm"][:len(per) * layer].astype(np.float64).tolist() and out["norm"].max() > 0
    h = out["history"]
    assert len(h) == 2 and all(q["itn"] > 0 for q in h) and h[1]["rms"] < h[0]["rms"]
    assert sum(nd for nd, _, _ in h[0]["per_map"]) == c["ndata"]
    assert len(log) == 2 * (1 + len(per)) + 1
    if azimuthal:
        assert [r["a1"] for r in rows] == out["a1"].ravel().astype(np.float64).tolist() and np.abs(out["a1"]).max() > 0 and np.abs(out["a2"]).max() > 0
        assert all(-90.0 <= r["axis"] <= 90.0 and r["strength"] >= 0 for r in rows)
    else:
        assert out["a1"] is None and "a1" not in rows[0]
