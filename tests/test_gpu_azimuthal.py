"""Azimuthal anisotropy on the device: dsa_solve_rows_azimuthal, dsa_set_azimuthal_slots, dsa_ray_azimuths,
dsa_calsurfg_azimuthal and invert.azimuthal_step.

The isotropic block must be dsa_solve_rows' bit for bit, whatever the lanes per ray and the launches per call; the gc and gs blocks and the
per-ray sums must be the host twin's (tests/hostcheck_azimuthal.cpp: the same trace_ray<., true> on the CPU) run on the engine's own
fields and composed by the entry rule in NumPy.  Every test uses an engine of its own.
"""
import ctypes as C

import numpy as np
import pytest

import _libs as L
import synth
import test_gpu_rows as R
import test_hostcheck_azimuthal as T

NX, GD = 35, 8
FTOL = np.float32(1e-4)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture
def eng():
    from dsurftomo_amd import build
    from dsurftomo_amd.engine import Engine
    build.build()
    e = Engine(0)
    yield e
    e.close()


def plan(nsrc=6, nper=2, nrec=48):
    """nsrc sources x nper periods (maps) x nrec receivers, period slot outer like the reference; receivers of their own per unit, all
    inside the grid and away from the source"""
    N = synth.nprop(NX, GD)
    gox, goz, dnx, dnz = synth.grid_origin(NX, GD)
    sx, sz = synth.sources(NX, nsrc, GD, inner=0.8)
    r = synth.LCG(77)
    rcx, rcz = [], []
    for p in range(nper):
        for s in range(nsrc):
            k = 0
            while k < nrec:
                u = r.uniform(2)
                px, pz = 2.2 + u[0] * (N - 5.4), 2.2 + u[1] * (N - 5.4)
                if np.hypot(px - (sx[s] - gox) / dnx, pz - (sz[s] - goz) / dnz) < 12:
                    continue
                rcx.append(np.float32(gox + np.float32(px) * dnx)); rcz.append(np.float32(goz + np.float32(pz) * dnz))
                k += 1
    return dict(map_index=np.repeat(np.arange(nper, dtype=np.int32), nsrc), scx=np.tile(sx, nper), scz=np.tile(sz, nper),
                nrec=np.full(nsrc * nper, nrec, np.int32), rcx=np.array(rcx, np.float32), rcz=np.array(rcz, np.float32))


def maps(nper=2):
    return np.stack([synth.medium(NX, "smooth", p) for p in range(nper)])


def prepare(e, u, dm, sen_slot=None, keep=False):
    e.set_maps(NX, NX, synth.GOXD, synth.GOZD, synth.DVD, synth.DVD, maps(), dicing=GD)
    e.keep_fields(keep)
    e.set_depth_kernels(*dm)
    e.plan(u["map_index"], u["scx"], u["scz"], u["nrec"], u["rcx"], u["rcz"], sen_slot=sen_slot)


def capacity(u):
    return int(np.sum(u["nrec"])) * 3 * 4000


def maxvp_of(dm):
    return (NX - 2) * (NX - 2) * (dm[0].shape[0] - 1)


def twin_entries(u, dm, fields, slots, slot_on=None):
    """the gc / gs entries (rw, iw, col) of every ray, in order, from the host twin on the given fields by the entry rule, and the per-ray
    (steps, sums): val = (float)(Sazi * (double)f) over the isotropic row's vertices (|fdm| >= ftol), layers outer; kept when |val| > ftol"""
    h = T.load()
    g = L.grid(NX, NX, synth.GOXD, synth.GOZD, synth.DVD, synth.DVD, GD)
    vels, depz, sen_vs = dm[0], dm[1], dm[2]
    nz, kmax = sen_vs.shape[0], sen_vs.shape[1]
    nvx, nvz, ncol = NX - 2, NX - 2, NX * NX
    maxvp = nvx * nvz * (nz - 1)
    half = (np.float32(0.5) * vels.reshape(nz, ncol)).astype(np.float32)               # 0.5f * vels, one fp32 rounding
    sazi = sen_vs[:nz - 1] * half[:nz - 1, None, :].astype(np.float64)                 # (nz-1, kmax, ncol), one fp64 rounding
    jj, kk = np.meshgrid(np.arange(1, nvz + 1), np.arange(1, nvx + 1), indexing="ij")  # loop order: jj outer, kk inner
    jj, kk = jj.ravel(), kk.ravel()
    first = np.concatenate([[0], np.cumsum(u["nrec"])])
    rw, iw, col, steps, sums = [], [], [], [], []
    for k in range(len(u["map_index"])):
        vn, Tc, Tr, Sr = fields(k)
        b = L.Box()
        assert L.oracle().dso_source_box(C.byref(g), u["scx"][k], u["scz"][k], C.byref(b)) == 0
        sol = dict(box=b, T=Tc, Tr=np.ascontiguousarray(Tr), Sr=np.ascontiguousarray(Sr, np.int32))
        for q in range(first[k], first[k + 1]):
            fdm3, fl, st, sm = T.twin(h, NX, GD, g, vn, sol, u["scx"][k], u["scz"][k], u["rcx"][q], u["rcz"][q], 1)
            steps.append(st); sums.append(sm)
            if slot_on is not None and not slot_on[slots[k]]:
                continue
            keep = np.flatnonzero(np.abs(fdm3[0][kk, jj]) >= FTOL)                     # fdm[vx, vz]: the slab element (jj, kk)
            c = jj[keep] * NX + kk[keep]
            for B in (1, 2):
                f = fdm3[B][kk[keep], jj[keep]].astype(np.float64)
                val = (sazi[:, slots[k], :][:, c] * f[None, :]).astype(np.float32)     # (nz-1, kept)
                lay, e = np.nonzero(np.abs(val) > FTOL)                                # layers outer, kept vertices inner
                rw.append(val[lay, e]); iw.append(np.full(lay.size, q + 1, np.int32))
                col.append((B * maxvp + lay * (nvx * nvz) + keep[e] + 1).astype(np.int32))
    return (np.concatenate(rw), np.concatenate(iw), np.concatenate(col), np.array(steps), np.array(sums, np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 4])
def test_isotropic_block_equals_solve_rows_across_launches(eng, lanes):
    """col <= maxvp filtered out of dsa_solve_rows_azimuthal = dsa_solve_rows' rw, iw, col and times, bit for bit, with one and four lanes
    per ray and a ray_budget that splits the 576 rays over three launches"""
    e = eng
    u, dm = plan(), R.depth_model(NX, NX)
    prepare(e, u, dm)
    t0, rw0, iw0, col0 = e.solve_rows(capacity(u))
    st0 = e.stats()
    assert st0["rays"] == 576 and st0["ray_launches"] == 1
    slab, vlist = (NX * NX), (NX - 2) * (NX - 2)
    per_ray = (3 * slab + vlist) * 4 + 32                      # Engine::trace_chunk's budget per azimuthal ray
    e.set_option("ray_lanes", lanes)
    e.set_option("ray_budget", 200 * per_ray)
    t1, rw1, iw1, col1 = e.solve_rows_azimuthal(capacity(u))
    st1 = e.stats()
    assert st1["ray_launches"] == 3 and st1["rays"] == 576 and st1["ray_steps"] == st0["ray_steps"] and st1["nar"] == rw1.size
    maxvp = maxvp_of(dm)
    iso = col1 <= maxvp
    assert iso.sum() == rw0.size and (~iso).sum() > rw0.size // 10
    assert (bits(rw1[iso]) == bits(rw0)).all() and (iw1[iso] == iw0).all() and (col1[iso] == col0).all()
    assert (bits(t1) == bits(t0)).all()
    # within a ray: the isotropic entries, then block gc, then block gs; rays in data order
    assert (np.diff(iw1) >= 0).all()
    blk = (col1 - 1) // maxvp
    assert blk.max() == 2 and (np.diff(blk)[np.diff(iw1) == 0] >= 0).all()
    assert col1.max() <= 3 * maxvp and col1.min() >= 1
    # and the plain call afterwards is unchanged by the azimuthal one (shared scratch, other strides)
    t2, rw2, iw2, col2 = e.solve_rows(capacity(u))
    assert (bits(rw2) == bits(rw0)).all() and (iw2 == iw0).all() and (col2 == col0).all() and (bits(t2) == bits(t0)).all()


@pytest.mark.gpu
def test_gc_gs_blocks_and_sums_equal_the_host_twin(eng):
    """the gc and gs entries, bit for bit and in order, and dsa_ray_azimuths, against the host twin on the engine's own fetched fields"""
    e = eng
    u, dm = plan(nsrc=3, nper=2, nrec=24), R.depth_model(NX, NX, kmax=2)
    slots = np.asarray(u["map_index"])
    prepare(e, u, dm, sen_slot=slots, keep=True)
    t, rw, iw, col = e.solve_rows_azimuthal(capacity(u))
    datum, steps, sums = e.ray_azimuths()
    wrw, wiw, wcol, wsteps, wsums = twin_entries(u, dm, R.engine_fields(e, u), slots)
    azi = col > maxvp_of(dm)
    assert azi.sum() == wrw.size, (int(azi.sum()), wrw.size)
    assert (bits(rw[azi]) == bits(wrw)).all() and (iw[azi] == wiw).all() and (col[azi] == wcol).all()
    assert (datum == np.arange(1, datum.size + 1)).all() and datum.size == 144
    assert (steps == wsteps).all() and (bits(sums) == bits(wsums)).all()
    assert steps.min() > 10 and np.abs(sums).max() > 1.0


@pytest.mark.gpu
def test_slot_mask(eng):
    """a masked depth-kernel slot emits no gc / gs entries; its isotropic entries and everything of the other slot are unchanged"""
    e = eng
    u, dm = plan(nsrc=3, nper=2, nrec=24), R.depth_model(NX, NX, kmax=2)
    slots = np.asarray(u["map_index"])
    prepare(e, u, dm, sen_slot=slots)
    _, rw0, iw0, col0 = e.solve_rows_azimuthal(capacity(u))
    e.set_azimuthal_slots([1, 0])
    _, rw1, iw1, col1 = e.solve_rows_azimuthal(capacity(u))
    maxvp = maxvp_of(dm)
    off = iw0 > 72                                  # data of the units of slot 1 (period 1): rays 73 .. 144
    keep = ~(off & (col0 > maxvp))
    assert (col0[off] > maxvp).any() and (col0[~off] > maxvp).any()
    assert rw1.size == keep.sum() and (bits(rw1) == bits(rw0[keep])).all() and (iw1 == iw0[keep]).all() and (col1 == col0[keep]).all()
    assert not (col1[iw1 > 72] > maxvp).any()
    e.set_azimuthal_slots(None)                     # NULL: every slot emits again
    _, rw2, iw2, col2 = e.solve_rows_azimuthal(capacity(u))
    assert (bits(rw2) == bits(rw0)).all() and (col2 == col0).all()
    e.set_azimuthal_slots([1, 0, 1])                # not the depth kernels' slot count
    with pytest.raises(Exception) as exc:
        e.solve_rows_azimuthal(capacity(u))
    assert exc.value.code == -2


@pytest.mark.gpu
def test_errors(eng):
    from dsurftomo_amd.engine import EngineError
    e = eng
    u, dm = plan(nsrc=2, nper=1, nrec=8), R.depth_model(NX, NX)
    prepare(e, u, dm)
    with pytest.raises(EngineError) as exc:                    # before an azimuthal solve
        e.ray_azimuths()
    assert exc.value.code == -5
    e.solve_rows(capacity(u))
    with pytest.raises(EngineError) as exc:                    # a plain solve is not one
        e.ray_azimuths()
    assert exc.value.code == -5
    t, rw, iw, col = e.solve_rows_azimuthal(capacity(u))
    assert rw.size > 0
    with pytest.raises(EngineError) as exc:                    # capacity one short
        e.solve_rows_azimuthal(rw.size - 1)
    assert exc.value.code == -6
    with pytest.raises(EngineError) as exc:                    # ... and the failed call left no sums behind
        e.ray_azimuths()
    assert exc.value.code == -5
    t2, rw2, iw2, col2 = e.solve_rows_azimuthal(rw.size)       # exactly enough
    assert (bits(rw2) == bits(rw)).all()
    e.set_option("rows_on_device", 1)
    with pytest.raises(EngineError) as exc:
        e.solve_rows_azimuthal(capacity(u))
    assert exc.value.code == -5
    e.set_option("rows_on_device", 0)
    e.plan(u["map_index"], u["scx"], u["scz"], u["nrec"], u["rcx"], u["rcz"])
    with pytest.raises(EngineError) as exc:                    # a new plan: the old rays' sums are gone
        e.ray_azimuths()
    assert exc.value.code == -5


def call_azimuthal(lib, c):
    """dsa_calsurfg_azimuthal on a boundary case, arrays sized for three blocks (L.call_boundary's conventions)"""
    from dsurftomo_amd import io
    nd, npar = c["ndata"], c["nparpi"]
    cap = 3 * nd * npar + 1
    iw = np.zeros(cap + 1, np.int32); rw = np.zeros(cap, np.float32); col = np.zeros(cap, np.int32); dsurf = np.zeros(nd, np.float32)
    nar = C.c_int(0)
    head, tail = io._args(c)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    lib.dsa_dropin_set_capacity(cap)
    rc = lib.dsa_calsurfg_azimuthal(*head, p(iw), p(rw), p(col), p(dsurf), *tail, C.byref(nar))
    lib.dsa_dropin_set_capacity(0)
    assert rc == 0, lib.dsa_dropin_error().decode()
    n = nar.value
    assert iw[0] == n
    return dict(dsurf=dsurf, nar=n, rw=rw[:n].copy(), iw=iw[1:n + 1].copy(), col=col[:n].copy())


@pytest.mark.gpu
def test_dropin_isotropic_block_and_rayleigh_only():
    from dsurftomo_amd import invert
    from dsurftomo_amd.engine import load_library
    lib = invert.bind(load_library())
    c = synth.boundary_case(kRc=3, kRg=2, kLc=2, kLg=0)
    want = L.call_boundary(lib.dsa_calsurfg, c)
    got = call_azimuthal(lib, c)
    maxvp = c["nparpi"]
    iso = got["col"] <= maxvp
    assert iso.sum() == want["nar"] and (bits(got["rw"][iso]) == bits(want["rw"])).all() and (got["iw"][iso] == want["iw"]).all() and \
        (got["col"][iso] == want["col"]).all()
    assert (bits(got["dsurf"]) == bits(want["dsurf"])).all()
    # data run slot by slot (Rc, Rg, Lc), source by source: the Love data are those of the last kLc slots
    per_slot = np.asarray(c["nrc1"]).sum(axis=0)
    first_love = int(per_slot[:c["kRc"] + c["kRg"]].sum())
    assert first_love < c["ndata"]
    azi = ~iso
    assert azi.any() and (got["iw"][azi] <= first_love).all(), "a gc / gs entry sits on a Love datum"
    with_iso = np.unique(got["iw"][iso & (got["iw"] <= first_love)])
    assert with_iso.size > 0 and np.isin(with_iso, np.unique(got["iw"][azi])).all(), "a Rayleigh datum with isotropic entries has no gc / gs entry"
    assert got["col"].max() <= 3 * maxvp
    # the plain call afterwards is the plain call
    again = L.call_boundary(lib.dsa_calsurfg, c)
    assert again["nar"] == want["nar"] and (bits(again["rw"]) == bits(want["rw"])).all()


# What fp32 LSMR on the device showed against SciPy's fp64 LSMR in the recovery below: the device's median fast-axis
# error was 1.6697 degrees against SciPy's 1.6565: it exceeded it by RECOVERY_GAP_DEG degrees; the test allows twice that.
RECOVERY_GAP_DEG = 0.0132
RECOVERY_W, RECOVERY_DAMP = 0.05, 0.01


def axis_error_deg(gc, gs, want_deg):
    from dsurftomo_amd import invert
    d = np.abs(invert.azimuthal_axis(gc, gs) - want_deg) % 180.0
    return np.minimum(d, 180.0 - d)


@pytest.mark.gpu
def test_recovery_of_a_uniform_fast_axis():
    """A consistency check of the chain, on data that are first-order by construction: obst = dsyn + G_c gc0 + G_s gs0 for a uniform 4 %
    gc / gs at N30E, through azimuthal_step; against scipy's fp64 LSMR on the same assembled system with the same damp and limits"""
    import scipy.sparse as sp
    from scipy.sparse.linalg import lsmr
    from dsurftomo_amd import invert
    from dsurftomo_amd.engine import load_library
    lib = invert.bind(load_library())
    c = synth.boundary_case(nx=10, ny=9, nz=4, kRc=3, kRg=1, kLc=1, kLg=0, nsrc=8, nrcf=8, ragged=False)
    c.update(spfra=1.0, threshold0=np.float32(3.0), weight0=np.float32(2.0), damp=np.float32(0.5), minvel=np.float32(1.5), maxvel=np.float32(5.5))
    vsf = np.asfortranarray(c["vels"].copy())
    quiet = lambda *_: None
    maxvp = c["nparpi"]
    first = invert.azimuthal_step(lib, c, vsf, np.zeros(c["ndata"], np.float32), quiet, RECOVERY_W, RECOVERY_DAMP)
    assert (bits(vsf) == bits(np.asfortranarray(c["vels"]))).all(), "the step must not touch the model"
    rw, row, col = first["rw"].astype(np.float64), first["row"], first["col"]
    g0, axis0 = 0.04, 30.0
    gc0, gs0 = g0 * np.cos(np.radians(2 * axis0)), g0 * np.sin(np.radians(2 * axis0))
    isc, iss = (col > maxvp) & (col <= 2 * maxvp), col > 2 * maxvp
    dt = np.bincount(row[isc] - 1, rw[isc] * gc0, c["ndata"]) + np.bincount(row[iss] - 1, rw[iss] * gs0, c["ndata"])
    assert np.abs(dt).max() > 0.01
    obst = (first["dsyn"].astype(np.float64) + dt).astype(np.float32)
    got = invert.azimuthal_step(lib, c, vsf, obst, quiet, RECOVERY_W, RECOVERY_DAMP)
    S = got["system"]
    A = sp.csr_matrix((S["rw"].astype(np.float64), (S["row"] - 1, S["col"] - 1)), shape=(S["m"], S["n"]))
    atol, btol, conlim, itnlim, _ = invert.LSMR_ARGS
    x = lsmr(A, S["b"].astype(np.float64), damp=RECOVERY_DAMP, atol=atol, btol=btol, conlim=conlim, maxiter=itnlim)[0]
    colsum = np.bincount(col[isc] - 1 - maxvp, np.abs(rw[isc]), maxvp)
    cells = colsum > np.median(colsum)
    assert cells.sum() >= maxvp // 4
    err_ref = float(np.median(axis_error_deg(x[maxvp:2 * maxvp], x[2 * maxvp:], axis0)[cells]))
    err_dev = float(np.median(axis_error_deg(got["gc"], got["gs"], axis0)[cells]))
    amp = float(np.median(invert.azimuthal_strength(got["gc"], got["gs"])[cells]))
    print("recovery: median fast-axis error over %d cells: scipy fp64 %.4f deg, device fp32 %.4f deg; median strength %.3f %% (input %.3f %%); "
          "device itn %d istop %d" % (int(cells.sum()), err_ref, err_dev, amp, 50.0 * g0, got["itn"], got["istop"]))
    assert err_ref < 5.0, "the yardstick itself must recover the axis: under 10 degrees with a factor two to spare"
    assert err_dev <= err_ref + 2.0 * RECOVERY_GAP_DEG
