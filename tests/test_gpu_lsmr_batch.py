"""dsa_lsmr_batch (csrc/lsmr_batch.hip): R row-scaled LSMR solves on the resident matrix.  Realisation r must equal, in every
output bit (x, itn, istop, normA, condA, normr, normAr, normx), dsa_lsmr -- or the oracle's restatement of the reference's
LSMR -- on the explicitly scaled system: entries fl(a * s_r[row]), right-hand side fl(b * s_r)."""
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

pytestmark = pytest.mark.gpu

EST = ("normA", "condA", "normr", "normAr", "normx")


def scaled(S, s):
    """the system with row i scaled by s[i], as the contract states it"""
    s = np.asarray(s, np.float32)
    nar = S["nar"]
    rows = S["iw"][1:nar + 1]
    T = dict(S)
    T["rw"] = (S["rw"] * s[rows - 1]).astype(np.float32)
    T["b"] = (S["b"] * s).astype(np.float32)
    return T


def realisation(B, r):
    return dict(x=B["x"][r], istop=int(B["istop"][r]), itn=int(B["itn"][r]), **{k: B[k][r] for k in EST})


def load(e, S):
    nar = S["nar"]
    e.spmv_load(S["m"], S["n"], S["rw"], S["iw"][1:nar + 1], S["iw"][nar + 1:])


def batch(S, scales, damp, **kw):
    e = Engine(0)
    try:
        load(e, S)
        return e.lsmr_batch(S["b"], scales, damp, **kw)
    finally:
        e.close()


def sequential(S, scales, damp, **kw):
    """dsa_lsmr (default placement) on every explicitly scaled system"""
    e = Engine(0)
    out = []
    try:
        for s in scales:
            T = scaled(S, s)
            load(e, T)
            out.append(e.lsmr(T["b"], damp, **kw))
    finally:
        e.close()
    return out


def assert_all_equal(B, wants):
    assert B["x"].shape[0] == len(wants)
    bad = {r: inv.same(realisation(B, r), w) for r, w in enumerate(wants)}
    bad = {r: v for r, v in bad.items() if v}
    assert not bad, "realisations differing (fields): %s" % bad


def boundary_scales(m, n):
    rng = np.random.default_rng(21)
    ndata = m - n
    return np.stack([
        np.ones(m, np.float32),                                          # the unscaled system
        invert.bootstrap_row_scales(ndata, m, 1, seed=5)[0],              # sqrt(count), zeros included
        (0.5 + rng.random(m)).astype(np.float32),                        # smooth random
        np.where(np.arange(m) % 3 == 0, 2.0, 0.75).astype(np.float32),   # exact and inexact multipliers
        invert.bootstrap_row_scales(ndata, m, 1, seed=9)[0],
    ])


@pytest.mark.parametrize("damp,local_size,itnlim", [(1.0, 10, 400), (0.0, 10, 60), (0.5, 0, 100), (1.0, 3, 7)])
def test_batch_boundary_case_against_the_oracle(damp, local_size, itnlim):
    S = system(synth.boundary_case())
    sc = boundary_scales(S["m"], S["n"])
    B = batch(S, sc, damp, itnlim=itnlim, local_size=local_size)
    wants = [inv.call_lsmr(L.oracle().dso_lsmr, scaled(S, s), damp, itnlim=itnlim, local_size=local_size) for s in sc]
    assert_all_equal(B, wants)
    assert max(w["itn"] for w in wants) > 3
    if itnlim > 7:
        assert len(set(int(v) for v in B["itn"])) >= 2           # realisations stop at different iterations


def test_batch_multiblock_system():
    """the 100 001 x 68 479 system of test_lsmr_multiblock_system: both products over several blocks of the resident orderings"""
    import synth_matrix as SM
    M = SM.system(31522, 47, 47, 31, seed=11)
    m, n, nar = M["m"], M["n"], M["rw"].size
    b = np.zeros(m, np.float32)
    b[:31522] = (SM.mix(np.arange(31522), 12) - 0.5).astype(np.float32)
    S = dict(m=m, n=n, nar=nar, iw=np.concatenate([[nar], M["row"], M["col"]]).astype(np.int32), rw=M["rw"], b=b)
    sc = np.stack([invert.bootstrap_row_scales(31522, m, 1, seed=s)[0] for s in (1, 2)] + [(0.25 + SM.mix(np.arange(m), 3)).astype(np.float32)])
    B = batch(S, sc, 0.7, itnlim=35)
    wants = [inv.call_lsmr(L.oracle().dso_lsmr, scaled(S, s), 0.7, itnlim=35) for s in sc]
    assert max(w["itn"] for w in wants) > 3
    assert_all_equal(B, wants)


@pytest.fixture(scope="module")
def taipei_system():
    c = taipei.load()
    fwd = L.call_boundary(load_library().dsa_calsurfg, c)
    return c, inv.build_system(c, fwd, c["obst"], 3.0, 4.0)


def test_batch_taipei_crosses_a_lane_group(taipei_system):
    """R = 1, 64, 65 on the first iteration's Taipei system, each realisation against dsa_lsmr on its scaled system (65: two groups)"""
    c, S = taipei_system
    sc = invert.bootstrap_row_scales(c["ndata"], S["m"], 65, seed=2)
    wants = sequential(S, sc, 1.0)
    e = Engine(0)
    try:
        load(e, S)
        for R in (1, 64, 65):
            assert_all_equal(e.lsmr_batch(S["b"], sc[:R], 1.0), wants[:R])
    finally:
        e.close()
    assert len(set(w["itn"] for w in wants)) >= 2


def test_batch_identical_copies(taipei_system):
    """70 copies of one scale vector: 70 identical solutions, equal to dsa_lsmr on the scaled system"""
    c, S = taipei_system
    s = invert.bootstrap_row_scales(c["ndata"], S["m"], 1, seed=8)[0]
    B = batch(S, np.repeat(s[None, :], 70, axis=0), 1.0)
    want = sequential(S, [s], 1.0)[0]
    assert_all_equal(B, [want] * 70)


def test_batch_on_the_device_resident_system(taipei_system):
    """batch after dsa_iteration_system_device (rows never on the host) == batch on the same system loaded by spmv_load"""
    c, S = taipei_system
    lib = invert.bind(load_library())
    vsf = np.asfortranarray(c["vels"].copy())
    st = invert.iteration_device(lib, c, vsf, np.ascontiguousarray(c["obst"]), lambda *_: None, bootstrap=(8, 5))
    Sd = inv.build_system(c, L.call_boundary(lib.dsa_calsurfg, c), c["obst"], float(c["threshold0"]), float(c["weight0"]))
    assert np.array_equal(st["cbst"].view(np.uint32), Sd["b"].view(np.uint32))
    sc = invert.bootstrap_row_scales(c["ndata"], Sd["m"], 8, seed=5)
    H = batch(Sd, sc, float(c["damp"]))
    bo = st["boot"]
    D = dict(x=bo["x"], istop=bo["istop"], itn=bo["itn"], **{k: bo["est"][:, j] for j, k in enumerate(EST)})
    assert_all_equal(D, [realisation(H, r) for r in range(8)])
    assert np.allclose(bo["std"], bo["x"].astype(np.float64).std(axis=0, ddof=1))


def test_batch_leaves_the_engine_as_it_was():
    """dsa_lsmr keeps its bits after a batch; a new matrix of the same shape is seen by the next batch; b = 0 realisations"""
    S = system(synth.boundary_case())
    want = inv.call_lsmr(L.oracle().dso_lsmr, S, 1.0)
    sc = boundary_scales(S["m"], S["n"])
    S2 = dict(S); S2["rw"] = (S["rw"] * np.float32(1.5) + np.float32(0.01)).astype(np.float32)
    for dvec in (0, 1):
        e = Engine(0)
        try:
            e.set_option("lsmr_device_vectors", dvec)
            load(e, S)
            assert inv.same(e.lsmr(S["b"], 1.0), want) == []
            e.lsmr_batch(S["b"], sc, 1.0)
            assert inv.same(e.lsmr(S["b"], 1.0), want) == []
            load(e, S2)
            B2 = e.lsmr_batch(S2["b"], sc[:3], 1.0)
        finally:
            e.close()
        assert_all_equal(B2, [inv.call_lsmr(L.oracle().dso_lsmr, scaled(S2, s), 1.0) for s in sc[:3]])
    z = sc[:3].copy(); z[1] = 0.0                                         # realisation 1: b_r = 0
    B = batch(S, z, 1.0)
    assert B["itn"][1] == 0 and B["istop"][1] == 0 and not B["x"][1].any()
    assert_all_equal(dict(x=B["x"][[0, 2]], istop=B["istop"][[0, 2]], itn=B["itn"][[0, 2]], **{k: B[k][[0, 2]] for k in EST}),
                     [inv.call_lsmr(L.oracle().dso_lsmr, scaled(S, s), 1.0) for s in z[[0, 2]]])


def test_batch_errors():
    lib = load_library()
    S = system(synth.boundary_case())
    e = Engine(0)
    try:
        b = np.ascontiguousarray(S["b"])
        sc = np.ones((2, S["m"]), np.float32)
        x = np.zeros((2, S["n"]), np.float32); ii = np.zeros(2, np.int32); it = np.zeros(2, np.int32); est = np.zeros(10, np.float32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        args = lambda R, bb: (e._h, R, bb, p(sc), 1.0, 1e-6, 1e-6, 100.0, 400, 10, p(x), p(ii), p(it), p(est))
        assert lib.dsa_lsmr_batch(*args(2, p(b))) == -5                   # DSA_ERR_STATE: no matrix yet
        assert "dsa_spmv_load" in lib.dsa_error_string(e._h).decode()
        load(e, S)
        assert lib.dsa_lsmr_batch(*args(0, p(b))) == -2                   # DSA_ERR_ARGUMENT
        assert lib.dsa_lsmr_batch(*args(2, None)) == -2
        assert lib.dsa_lsmr_batch(None, 2, p(b), p(sc), 1.0, 1e-6, 1e-6, 100.0, 400, 10, p(x), p(ii), p(it), p(est)) == -2
        assert lib.dsa_lsmr_batch(*args(2, p(b))) == 0
        with pytest.raises(EngineError):
            e.lsmr_batch(b, np.ones((0, S["m"]), np.float32), 1.0)
    finally:
        e.close()


def test_invert_bootstrap_writes_std(tmp_path):
    """invert.run(..., bootstrap=16): every file of the plain run byte-identical, plus DSurfTomo.inStd.dat = the standard deviation
    of 16 sequential dsa_lsmr solves of the last iteration's scaled systems"""
    plain, boot = tmp_path / "plain", tmp_path / "boot"
    plain.mkdir(); boot.mkdir()
    lp, lb = [], []
    invert.run(taipei.HERE, maxiter=2, out_dir=str(plain), log=lp.append)
    _, hist = invert.run(taipei.HERE, maxiter=2, out_dir=str(boot), log=lb.append, bootstrap=16, bootstrap_seed=3)
    names = sorted(os.listdir(plain))
    assert sorted(os.listdir(boot)) == sorted(names + ["DSurfTomo.inStd.dat"])
    for nm in names:
        assert (plain / nm).read_bytes() == (boot / nm).read_bytes(), nm
    hb = hist[-1]["bootstrap"]
    assert hb["realisations"] == 16 and hb["std_max"] > 0 and "bootstrap" not in hist[0]
    assert [l for l in lb if "bootstrap:" not in l and "(forward" not in l] == [l for l in lp if "(forward" not in l]
    std = np.loadtxt(str(boot / "DSurfTomo.inStd.dat"))
    assert std.shape == (2048, 4) and np.isfinite(std).all() and (std[:, 3] >= 0).all() and (std[:, 3] > 0).any()
    # the same from the host: iteration 1 as run() does it, the second iteration's system by the oracle, 16 dsa_lsmr solves
    c = taipei.load()
    lib = invert.bind(load_library())
    vsf = np.asfortranarray(c["vels"].copy())
    invert.iteration_device(lib, c, vsf, np.ascontiguousarray(c["obst"]), lambda *_: None)
    cc = dict(c); cc["vels"] = vsf
    S = inv.build_system(c, L.call_boundary(lib.dsa_calsurfg, cc), c["obst"], float(c["threshold0"]), float(c["weight0"]))
    sc = invert.bootstrap_row_scales(c["ndata"], S["m"], 16, seed=3)
    xs = np.stack([w["x"] for w in sequential(S, sc, float(c["damp"]))])
    invert.write_std(str(tmp_path / "want.dat"), c, xs.astype(np.float64).std(axis=0, ddof=1))
    assert (tmp_path / "want.dat").read_text() == (boot / "DSurfTomo.inStd.dat").read_text()
    # the vertex of every Std.dat row, checked without write_std: row q holds unknown q (the order dsa_model_update applies the
    # update in, iteration.hip), on the same vertex as row q of the model files -- the second iteration's own update, from
    # dsa_lsmr on the unscaled system, is the change between Measure.dat.iter001 and .iter002 row by row
    want_std = xs.astype(np.float64).std(axis=0, ddof=1)
    assert np.abs(std[:, 3] - want_std).max() <= 5.01e-6
    m1 = np.loadtxt(str(boot / "DSurfTomo.inMeasure.dat.iter001"))
    m2 = np.loadtxt(str(boot / "DSurfTomo.inMeasure.dat.iter002"))
    assert np.array_equal(std[:, :3], m1[:, :3])
    dv2 = np.clip(sequential(S, [np.ones(S["m"], np.float32)], float(c["damp"]))[0]["x"].astype(np.float64), -0.5, 0.5)
    moved = np.abs(dv2) > 1e-3
    assert moved.sum() > 100
    assert (np.abs((m2[:, 3] - m1[:, 3]) - dv2)[moved] <= 2e-5).mean() > 0.99
