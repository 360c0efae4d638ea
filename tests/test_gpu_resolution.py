"""dsa_lsmr_resolution (csrc/lsmr_batch.hip): LSMR solves of the resident system whose right-hand sides the device forms from test
models, b_r = A m_r on the data rows and +0 on the regularisation rows.  Realisation r must equal, in every output bit (x, itn, istop,
normA, condA, normr, normAr, normx), dsa_lsmr on b_r formed on the host from Engine.spmv(1, m_r, 0) with the rows from ndata up set to
zero; the PSF measures must match numpy on the fetched solutions.  The product library and the oracle's compiled LSMR only."""
import ctypes as C
import os

import numpy as np
import pytest

import _libs as L
import inversion as inv
import synth
from dsurftomo_amd import invert
from dsurftomo_amd import io as taipei
from dsurftomo_amd.engine import Engine, EngineError, load_library
from test_gpu_lsmr import system
from test_gpu_lsmr_batch import EST, assert_all_equal, boundary_scales, load, realisation

pytestmark = pytest.mark.gpu


def rhs(e, S, ndata, model):
    """b = A m on the data rows (dsa_spmv mode 1 from y = 0), +0 on the rows from ndata up"""
    b = e.spmv(1, np.asarray(model, np.float32), np.zeros(S["m"], np.float32))
    b[ndata:] = 0.0
    return b


def pick(B, idx):
    return dict(x=B["x"][idx], istop=B["istop"][idx], itn=B["itn"][idx], **{k: B[k][idx] for k in EST})


def spikes(n, first, R):
    E = np.zeros((R, n), np.float32)
    E[np.arange(R), first + np.arange(R)] = 1.0
    return E


def psf_numpy(x, coords, j):
    x = np.asarray(x, np.float64)
    w = x * x
    dh = invert.great_circle_km(coords[:, 0], coords[:, 1], coords[j, 0], coords[j, 1])
    dz = coords[:, 2] - coords[j, 2]
    return np.array([w.sum(), (w * dh * dh).sum(), (w * dz * dz).sum()])


def boundary_system():
    c = synth.boundary_case()
    return c, system(c, fwd=L.call_boundary(load_library().dsa_calsurfg, c))


def boundary_models(c, n):
    rng = np.random.default_rng(7)
    spike = np.zeros(n, np.float32)
    spike[n // 3] = 1.0
    return np.stack([invert.checkerboard(c, (2, 2, 1)), (rng.random(n) - 0.5).astype(np.float32), spike, np.zeros(n, np.float32),
                     invert.checkerboard(c, (3, 1, 2))])


@pytest.fixture(scope="module")
def taipei_system():
    c = taipei.load()
    return c, inv.build_system(c, L.call_boundary(load_library().dsa_calsurfg, c), c["obst"], 3.0, 4.0)


@pytest.mark.parametrize("damp,local_size,itnlim", [(1.0, 10, 400), (0.0, 10, 60), (0.5, 0, 100), (1.0, 3, 7)])
def test_host_models_boundary_case(damp, local_size, itnlim):
    """host models on the boundary case: every realisation == dsa_lsmr on its host-formed b_r == the oracle's LSMR on it"""
    c, S = boundary_system()
    nd = c["ndata"]
    assert nd == S["m"] - S["n"]
    M = boundary_models(c, S["n"])
    e = Engine(0)
    try:
        load(e, S)
        got = e.lsmr_resolution(nd, damp, models=M, itnlim=itnlim, local_size=local_size)
        bs = [rhs(e, S, nd, mm) for mm in M]
        wants = [e.lsmr(b, damp, itnlim=itnlim, local_size=local_size) for b in bs]
    finally:
        e.close()
    assert got["psf"] is None
    assert_all_equal(got, wants)
    assert_all_equal(got, [inv.call_lsmr(L.oracle().dso_lsmr, dict(S, b=b), damp, itnlim=itnlim, local_size=local_size) for b in bs])
    assert got["itn"][3] == 0 and got["istop"][3] == 0 and not got["x"][3].any()          # m = 0: b = 0
    assert max(w["itn"] for w in wants) > 3


def test_host_models_taipei_crosses_a_lane_group(taipei_system):
    """R = 1, 64, 65 host models on the Taipei system, each realisation against dsa_lsmr on its host-formed b_r (65: two groups)"""
    c, S = taipei_system
    n, nd = S["n"], c["ndata"]
    M = (0.05 * np.random.default_rng(12).standard_normal((65, n))).astype(np.float32)
    M[5] = invert.checkerboard(c, (4, 4, 2))
    M[64] = invert.checkerboard(c, (2, 3, 1))
    e = Engine(0)
    try:
        load(e, S)
        wants = [e.lsmr(rhs(e, S, nd, mm), 1.0) for mm in M]
        for R in (1, 64, 65):
            assert_all_equal(e.lsmr_resolution(nd, 1.0, models=M[:R]), wants[:R])
    finally:
        e.close()
    assert len(set(w["itn"] for w in wants)) >= 2


def test_spikes_and_psf_taipei(taipei_system):
    """device spikes == the same spikes as host models (three lane groups); a few against dsa_lsmr; R_jj == x_r[j] bit for bit, the
    three sums == numpy fp64 on the fetched x to 1e-9; a second call without x: the same bits"""
    c, S = taipei_system
    n, nd = S["n"], c["ndata"]
    coords = invert.unknown_coords(c)
    first, R = 1000, 130
    E = spikes(n, first, R)
    some = [0, 63, 64, 129]
    e = Engine(0)
    try:
        load(e, S)
        D = e.lsmr_resolution(nd, 1.0, spikes=(first, R), coords=coords)
        D2 = e.lsmr_resolution(nd, 1.0, spikes=(first, R), coords=coords, want_x=False)
        H = e.lsmr_resolution(nd, 1.0, models=E)
        seq = [e.lsmr(rhs(e, S, nd, E[r]), 1.0) for r in some]
    finally:
        e.close()
    assert_all_equal(D, [realisation(H, r) for r in range(R)])
    assert_all_equal(pick(D, some), seq)
    assert D2["x"] is None and np.array_equal(D2["psf"].view(np.uint64), D["psf"].view(np.uint64))
    assert np.array_equal(D2["itn"], D["itn"]) and np.array_equal(D2["istop"], D["istop"])
    for r in range(R):
        j = first + r
        assert D["psf"][r, 0] == np.float64(D["x"][r][j]), r
        want = psf_numpy(D["x"][r], coords, j)
        assert np.allclose(D["psf"][r, 1:], want, rtol=1e-9, atol=0.0), (r, D["psf"][r], want)
    assert (D["psf"][:, 1] > 0).sum() > R // 2 and (D["psf"][:, 2] > 0).any() and (D["psf"][:, 3] > 0).any()


def test_vertex_without_rays_gives_zeros():
    """the boundary system with every data entry of one column removed: its spike has b = 0 -> x = 0, itn 0, istop 0, psf all 0"""
    c, S = boundary_system()
    nd, n, nar = c["ndata"], S["n"], S["nar"]
    rows, cols = S["iw"][1:nar + 1], S["iw"][nar + 1:]
    j0 = int(np.argmax(np.bincount(cols[rows <= nd] - 1, minlength=n)))
    keep = ~((cols == j0 + 1) & (rows <= nd))
    T = dict(S, nar=int(keep.sum()), rw=S["rw"][keep], iw=np.concatenate([[keep.sum()], rows[keep], cols[keep]]).astype(np.int32))
    first = max(0, j0 - 1)
    R = min(3, n - first)
    coords = invert.unknown_coords(c)
    e = Engine(0)
    try:
        load(e, T)
        D = e.lsmr_resolution(nd, 1.0, spikes=(first, R), coords=coords)
        wants = [e.lsmr(rhs(e, T, nd, row), 1.0) for row in spikes(n, first, R)]
    finally:
        e.close()
    r0 = j0 - first
    assert D["itn"][r0] == 0 and D["istop"][r0] == 0 and not D["x"][r0].any() and not D["psf"][r0].any()
    assert_all_equal(D, wants)


def test_spikes_cross_a_block_of_the_multiblock_system():
    """the 100 001 x 68 479 system of test_lsmr_multiblock_system: spikes 32 728 .. 32 807 straddle the first 32 768-column block of
    the row ordering; device spikes == host models, four of them == dsa_lsmr"""
    import synth_matrix as SM
    M = SM.system(31522, 47, 47, 31, seed=11)
    m, n, nar = M["m"], M["n"], M["rw"].size
    S = dict(m=m, n=n, nar=nar, iw=np.concatenate([[nar], M["row"], M["col"]]).astype(np.int32), rw=M["rw"], b=np.zeros(m, np.float32))
    nd = 31522
    first, R = SM.BLOCK - 40, 80
    E = spikes(n, first, R)
    some = [0, 39, 40, 79]
    e = Engine(0)
    try:
        load(e, S)
        D = e.lsmr_resolution(nd, 0.7, spikes=(first, R), itnlim=35)
        H = e.lsmr_resolution(nd, 0.7, models=E, itnlim=35)
        seq = [e.lsmr(rhs(e, S, nd, E[r]), 0.7, itnlim=35) for r in some]
    finally:
        e.close()
    assert_all_equal(D, [realisation(H, r) for r in range(R)])
    assert_all_equal(pick(D, some), seq)
    assert int(D["itn"].max()) > 3


def test_resolution_errors():
    lib = load_library()
    c, S = boundary_system()
    m, n, nd = S["m"], S["n"], c["ndata"]
    coords = np.ascontiguousarray(invert.unknown_coords(c))
    mod = np.zeros((2, n), np.float32)
    x = np.zeros((2, n), np.float32); psf = np.zeros((2, 4)); ii = np.zeros(2, np.int32); it = np.zeros(2, np.int32); est = np.zeros(10, np.float32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    e = Engine(0)
    try:
        def call(R=2, ndata=nd, models=None, first=0, co=coords, xx=x, ps=psf, a=ii, b=it, es=est, h=e._h):
            return lib.dsa_lsmr_resolution(h, R, ndata, p(models), first, p(co), 1.0, 1e-6, 1e-6, 100.0, 400, 10, p(xx), p(ps), p(a), p(b), p(es))
        assert call() == -5                                                   # DSA_ERR_STATE: no matrix yet
        assert "dsa_spmv_load" in lib.dsa_error_string(e._h).decode()
        load(e, S)
        for kw in (dict(R=0), dict(ndata=0), dict(ndata=m + 1), dict(first=-1), dict(first=n - 1), dict(models=mod), dict(co=None),
                   dict(a=None), dict(b=None), dict(es=None), dict(h=None)):
            assert call(**kw) == -2, kw                                       # DSA_ERR_ARGUMENT
        assert call() == 0 and call(first=n - 2) == 0 and call(ndata=m) == 0 and call(xx=None) == 0
        assert call(models=mod, ps=None) == 0 and (it == 0).all()              # zero models: b = 0
        with pytest.raises(EngineError):
            e.lsmr_resolution(nd, 1.0, models=np.zeros((0, n), np.float32))
        with pytest.raises(EngineError):
            e.lsmr_resolution(nd, 1.0, spikes=(n - 1, 2))
    finally:
        e.close()


def test_resolution_leaves_the_engine_as_it_was():
    """dsa_lsmr and dsa_lsmr_batch keep their bits after resolution calls (spikes with PSF measures, host models without x)"""
    c, S = boundary_system()
    want = inv.call_lsmr(L.oracle().dso_lsmr, S, 1.0)
    sc = boundary_scales(S["m"], S["n"])
    coords = invert.unknown_coords(c)
    for dvec in (0, 1):
        e = Engine(0)
        try:
            e.set_option("lsmr_device_vectors", dvec)
            load(e, S)
            B0 = e.lsmr_batch(S["b"], sc, 1.0)
            e.lsmr_resolution(c["ndata"], 1.0, spikes=(0, 70), coords=coords)
            assert inv.same(e.lsmr(S["b"], 1.0), want) == []
            B1 = e.lsmr_batch(S["b"], sc, 1.0)
            e.lsmr_resolution(c["ndata"], 1.0, models=np.ones((3, S["n"]), np.float32), want_x=False)
            assert inv.same(e.lsmr(S["b"], 1.0), want) == []
            B2 = e.lsmr_batch(S["b"], sc, 1.0)
        finally:
            e.close()
        assert_all_equal(B1, [realisation(B0, r) for r in range(len(sc))])
        assert_all_equal(B2, [realisation(B0, r) for r in range(len(sc))])


def test_invert_resolution_and_checkerboards(tmp_path):
    """invert.run(..., resolution=True, resolution_chunk=100, two checkerboards): every file of the plain run byte-identical, plus
    Resolution.dat (rows of 40 unknowns == write_model of sequential dsa_lsmr spike solves of the second iteration's system) and
    Checker.dat.k01 / k02 (== one dsa_lsmr solve each)"""
    plain, res = tmp_path / "plain", tmp_path / "res"
    plain.mkdir(); res.mkdir()
    lp, lr = [], []
    cells = [(4, 4, 2), (2, 3, 1)]
    invert.run(taipei.HERE, maxiter=2, out_dir=str(plain), log=lp.append)
    _, hist = invert.run(taipei.HERE, maxiter=2, out_dir=str(res), log=lr.append, resolution=True, resolution_chunk=100, checkerboard=cells)
    names = sorted(os.listdir(plain))
    new = ["DSurfTomo.inResolution.dat", "DSurfTomo.inChecker.dat.k01", "DSurfTomo.inChecker.dat.k02"]
    assert sorted(os.listdir(res)) == sorted(names + new)
    for nm in names:
        assert (plain / nm).read_bytes() == (res / nm).read_bytes(), nm
    ours = (" resolution:", " checkerboard")
    assert [l for l in lr if not l.startswith(ours) and "(forward" not in l] == [l for l in lp if "(forward" not in l]
    hr = hist[-1]["resolution"]
    assert hr["realisations"] == 2048 and hr["chunk"] == 100 and hr["calls"] == 21 and "resolution" not in hist[0]
    hc = hist[-1]["checkerboard"]
    assert [tuple(p["cell"]) for p in hc["patterns"]] == cells and hc["realisations"] == 2
    # the second iteration's system from the host, as test_invert_bootstrap_writes_std builds it
    c = taipei.load()
    lib = invert.bind(load_library())
    vsf = np.asfortranarray(c["vels"].copy())
    invert.iteration_device(lib, c, vsf, np.ascontiguousarray(c["obst"]), lambda *_: None)
    cc = dict(c); cc["vels"] = vsf
    S = inv.build_system(c, L.call_boundary(lib.dsa_calsurfg, cc), c["obst"], float(c["threshold0"]), float(c["weight0"]))
    n, nd, damp = S["n"], c["ndata"], float(c["damp"])
    coords = invert.unknown_coords(c)
    js = np.sort(np.random.default_rng(5).choice(n, 40, replace=False))
    psf = np.zeros((n, 4))
    e = Engine(0)
    try:
        load(e, S)
        for j in js:
            x = e.lsmr(rhs(e, S, nd, spikes(n, int(j), 1)[0]), damp)["x"]
            psf[j, 0] = x[j]
            psf[j, 1:] = psf_numpy(x, coords, int(j))
        xs = [e.lsmr(rhs(e, S, nd, invert.checkerboard(c, cell)), damp)["x"] for cell in cells]
    finally:
        e.close()
    rjj, lh, lv, _ = invert.psf_columns(psf)
    invert.write_model(str(tmp_path / "want_res.dat"), c, *[invert.unknowns_grid(c, v) for v in (rjj, lh, lv)])
    want_rows = (tmp_path / "want_res.dat").read_text().splitlines()
    got_rows = (res / "DSurfTomo.inResolution.dat").read_text().splitlines()
    assert len(got_rows) == n
    assert [got_rows[j] for j in js] == [want_rows[j] for j in js]
    for q, (cell, x) in enumerate(zip(cells, xs)):
        mk = invert.checkerboard(c, cell)
        invert.write_model(str(tmp_path / "want_k.dat"), c, invert.unknowns_grid(c, mk), invert.unknowns_grid(c, x))
        assert (tmp_path / "want_k.dat").read_text() == (res / ("DSurfTomo.inChecker.dat.k%02d" % (q + 1))).read_text()
        mt = invert.recovery_metrics(mk, x, c["nz"] - 1)
        assert hc["patterns"][q]["corr"] == mt["corr"] and hc["patterns"][q]["gain"] == mt["gain"]
