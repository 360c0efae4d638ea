"""dsa_lsmr_tradeoff (csrc/lsmr_batch.hip): K (weight, damp) LSMR solves of one resident system whose regularisation rows were built
with weight0.  Member k must equal, in every output bit (x, itn, istop, normA, condA, normr, normAr, normx), dsa_lsmr -- or the oracle's
restatement of the reference's LSMR -- with damp_k on the system REBUILT with weight_k (regularisation entries fl(c * weight_k), the
system dsa_iteration_system makes), and the measures must match numpy float64 on the returned solutions within the worst-case bound
of two fp64 evaluations in different orders."""
import os

import numpy as np
import pytest

import _libs as L
import inversion as inv
import synth
import synth_matrix as SM
from dsurftomo_amd import invert
from dsurftomo_amd import io as taipei
from dsurftomo_amd.engine import Engine, EngineError, load_library
from test_gpu_lsmr import system
from test_gpu_lsmr_batch import EST, assert_all_equal, load, realisation

pytestmark = pytest.mark.gpu

MEMBERS = [(2.0, 1.0), (0.5, 0.0), (3.0, 0.3), (0.7, 1.0), (0.0, 0.5), (11.3, 2.0)]


def f32(v):
    return float(np.float32(v))


def pick(T, idx):
    return dict(x=T["x"][idx], istop=T["istop"][idx], itn=T["itn"][idx], **{k: T[k][idx] for k in EST})


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def assert_same_result(A, B):
    """two lsmr_tradeoff results: every array the same bits"""
    for k in ("x", "measures", "istop", "itn") + EST:
        assert same_bits(A[k], B[k]), k


def measures_numpy(S, nd, coef, x):
    """({sum r^2 over the data rows, sum (C x)^2 over the rows from nd up, sum x^2}, their bounds) in numpy float64 on the solution x:
    coef holds the values of S with the integer coefficients on the rows from nd up.  Bound of each sum: 4 (Lmax + m) 2^-53 sum T_i^2,
    T_i = sum_j |a_ij x_j| + |b_i| (for sum x^2: T_j = |x_j|), the worst case of two fp64 evaluations in different orders"""
    nar, m = S["nar"], S["m"]
    rows, cols = S["iw"][1:nar + 1] - 1, S["iw"][nar + 1:] - 1
    x64 = np.asarray(x, np.float64)
    prod = coef.astype(np.float64) * x64[cols]
    ax = np.bincount(rows, weights=prod, minlength=m)
    t = np.bincount(rows, weights=np.abs(prod), minlength=m) + np.abs(S["b"].astype(np.float64))
    r = S["b"].astype(np.float64) - ax
    lmax = int(np.bincount(rows, minlength=m).max())
    eps = 4.0 * (lmax + m) * 2.0 ** -53
    want = np.array([(r[:nd] ** 2).sum(), (ax[nd:] ** 2).sum(), (x64 ** 2).sum()])
    bound = eps * np.array([(t[:nd] ** 2).sum(), (t[nd:] ** 2).sum(), (x64 ** 2).sum()])
    return want, bound


def assert_measures(T, S, nd, weight0):
    nar = S["nar"]
    rows = S["iw"][1:nar + 1] - 1
    coef = np.where(rows >= nd, np.rint(S["rw"] / np.float32(weight0)), S["rw"]).astype(np.float32)
    assert (coef[rows >= nd] != 0).all()
    for k in range(T["x"].shape[0]):
        want, bound = measures_numpy(S, nd, coef, T["x"][k])
        got = T["measures"][k]
        print("member %d: measures %s numpy %s |difference| %s bound %s" % (k, got, want, np.abs(got - want), bound))
        assert (np.abs(got - want) <= bound).all(), (k, got, want, bound)
        assert (got >= 0).all() and got[0] > 0


@pytest.fixture(scope="module")
def boundary():
    c = synth.boundary_case()
    return c, L.call_boundary(load_library().dsa_calsurfg, c)


@pytest.mark.parametrize("local_size,itnlim", [(10, 400), (0, 100), (3, 7)])
def test_tradeoff_boundary_case_against_the_oracle(boundary, local_size, itnlim):
    """six members (weight 0, damp 0, the resident weight among them): each == the oracle's LSMR on the system rebuilt with its weight;
    the measures == numpy on the returned x, and the same bits without x"""
    c, fwd = boundary
    S = system(c, weight0=2.0, fwd=fwd)
    nd = c["ndata"]
    assert nd == S["m"] - S["n"]
    w = [m[0] for m in MEMBERS]
    d = [m[1] for m in MEMBERS]
    e = Engine(0)
    try:
        load(e, S)
        T = e.lsmr_tradeoff(S["b"], nd, 2.0, w, d, itnlim=itnlim, local_size=local_size)
        T2 = e.lsmr_tradeoff(S["b"], nd, 2.0, w, d, want_x=False, itnlim=itnlim, local_size=local_size)
        own = e.lsmr(S["b"], 1.0, itnlim=itnlim, local_size=local_size)
    finally:
        e.close()
    wants = []
    for wk, dk in MEMBERS:
        Sk = system(c, weight0=f32(wk), fwd=fwd)
        assert Sk["nar"] == S["nar"] and np.array_equal(Sk["iw"], S["iw"]) and same_bits(Sk["b"], S["b"])
        wants.append(inv.call_lsmr(L.oracle().dso_lsmr, Sk, f32(dk), itnlim=itnlim, local_size=local_size))
    assert_all_equal(T, wants)
    assert inv.same(realisation(T, 0), own) == []                   # (2.0, 1.0): the resident system itself
    assert max(v["itn"] for v in wants) > 3
    if itnlim > 7:
        assert len(set(int(v) for v in T["itn"])) >= 2              # members stop at different iterations
    assert_measures(T, S, nd, 2.0)
    assert T2["x"] is None and same_bits(T2["measures"], T["measures"])
    assert np.array_equal(T2["itn"], T["itn"]) and np.array_equal(T2["istop"], T["istop"])
    if itnlim > 7:                                                  # the roughness is free of the weight: without smoothing (member 4) it is larger
        assert T["measures"][4, 1] > T["measures"][0, 1]


@pytest.fixture(scope="module")
def taipei_forward():
    c = taipei.load()
    return c, L.call_boundary(load_library().dsa_calsurfg, c)


def test_tradeoff_taipei_crosses_a_lane_group(taipei_forward):
    """K = 65 on the first iteration's Taipei system (built with weight 4): members 0, 31, 63, 64 against dsa_lsmr on the rebuilt
    systems; dsa_lsmr, dsa_lsmr_batch and a second trade-off call keep their bits"""
    c, fwd = taipei_forward
    S = inv.build_system(c, fwd, c["obst"], 3.0, 4.0)
    nd = c["ndata"]
    w, d = invert.tradeoff_grid(np.geomspace(0.25, 64.0, 13), [0.0, 0.3, 1.0, 2.5, 4.0])
    assert w.size == 65
    some = [0, 31, 63, 64]
    ones = np.ones((1, S["m"]), np.float32)
    e = Engine(0)
    try:
        load(e, S)
        own0 = e.lsmr(S["b"], 1.0)
        B0 = e.lsmr_batch(S["b"], ones, 1.0)
        T = e.lsmr_tradeoff(S["b"], nd, 4.0, w, d)
        own1 = e.lsmr(S["b"], 1.0)
        B1 = e.lsmr_batch(S["b"], ones, 1.0)
        T2 = e.lsmr_tradeoff(S["b"], nd, 4.0, w, d)
        wants = []
        for k in some:
            Sk = inv.build_system(c, fwd, c["obst"], 3.0, float(w[k]))
            assert same_bits(Sk["b"], S["b"]) and np.array_equal(Sk["iw"], S["iw"])
            load(e, Sk)
            wants.append(e.lsmr(Sk["b"], float(d[k])))
    finally:
        e.close()
    assert_all_equal(pick(T, some), wants)
    assert inv.same(own1, own0) == []
    assert inv.same(realisation(B1, 0), realisation(B0, 0)) == [] and inv.same(realisation(B0, 0), own0) == []
    assert_same_result(T2, T)
    assert len(set(int(v) for v in T["itn"])) >= 2
    for j in range(5):                                              # per damp the roughness falls with the weight, end to end (0.25 -> 64)
        assert T["measures"][j, 1] > T["measures"][60 + j, 1]


def multiblock():
    M = SM.system(31522, 47, 47, 31, seed=11)
    m, n, nar = M["m"], M["n"], M["rw"].size
    b = np.zeros(m, np.float32)
    b[:31522] = (SM.mix(np.arange(31522), 12) - 0.5).astype(np.float32)
    return dict(m=m, n=n, nar=nar, iw=np.concatenate([[nar], M["row"], M["col"]]).astype(np.int32), rw=M["rw"], b=b), M["nar_data"]


def test_tradeoff_multiblock_system():
    """the 100 001 x 68 479 system of test_lsmr_multiblock_system (regularisation rows of weight 2): three members against the
    oracle's LSMR on the systems whose regularisation rows synth_matrix rebuilds with their weights; the measures against numpy"""
    S, nar_data = multiblock()
    nd = 31522
    members = [(0.5, 0.7), (2.0, 0.0), (7.25, 1.5)]
    e = Engine(0)
    try:
        load(e, S)
        T = e.lsmr_tradeoff(S["b"], nd, 2.0, [m[0] for m in members], [m[1] for m in members], itnlim=35)
        T2 = e.lsmr_tradeoff(S["b"], nd, 2.0, [m[0] for m in members], [m[1] for m in members], want_x=False, itnlim=35)
    finally:
        e.close()
    wants = []
    for wk, dk in members:
        rr, rc, rv = SM.regularisation_rows(47, 47, 31, wk, nd)
        assert np.array_equal(rr + 1, S["iw"][1 + nar_data:S["nar"] + 1]) and np.array_equal(rc + 1, S["iw"][S["nar"] + 1 + nar_data:])
        Sk = dict(S, rw=np.concatenate([S["rw"][:nar_data], rv]).astype(np.float32))
        wants.append(inv.call_lsmr(L.oracle().dso_lsmr, Sk, dk, itnlim=35))
    assert max(v["itn"] for v in wants) > 3
    assert_all_equal(T, wants)
    assert_measures(T, S, nd, 2.0)
    assert T2["x"] is None and same_bits(T2["measures"], T["measures"])


def test_tradeoff_errors(boundary):
    c, fwd = boundary
    S = system(c, weight0=2.0, fwd=fwd)
    nd, m = c["ndata"], S["m"]
    e = Engine(0)
    try:
        e._mn = (S["m"], S["n"])                                      # (what spmv_load would note: the binding sizes its arrays from it)
        with pytest.raises(EngineError) as exc:
            e.lsmr_tradeoff(S["b"], nd, 2.0, [1.0], [1.0])
        assert exc.value.code == -5 and "dsa_spmv_load" in str(exc.value)            # DSA_ERR_STATE: no matrix yet
        load(e, S)
        want = e.lsmr(S["b"], 1.0)
        bad = [dict(weight0=3.0), dict(ndata=0), dict(ndata=m + 1), dict(weights=[1.0, -0.5]), dict(damps=[1.0, float("nan")]),
               dict(weights=[float("inf"), 1.0]), dict(damps=[-1.0, 1.0]), dict(weight0=0.0), dict(weight0=float("nan")), dict(weight0=-2.0),
               dict(weights=[], damps=[])]
        for kw in bad:
            a = dict(ndata=nd, weight0=2.0, weights=[1.0, 2.0], damps=[1.0, 1.0])
            a.update(kw)
            with pytest.raises(EngineError) as exc:
                e.lsmr_tradeoff(S["b"], a["ndata"], a["weight0"], a["weights"], a["damps"])
            assert exc.value.code == -2, kw                                        # DSA_ERR_ARGUMENT
            # the engine is still usable, with the weight it was built with
            assert inv.same(e.lsmr(S["b"], 1.0), want) == [], kw
        T = e.lsmr_tradeoff(S["b"], nd, 2.0, [2.0], [1.0])
        assert inv.same(realisation(T, 0), want) == []
        # ndata = m: no regularisation rows, every weight gives the resident system
        T = e.lsmr_tradeoff(S["b"], m, 2.0, [0.0, 5.0], [1.0, 1.0])
        assert_all_equal(T, [want, want])
        assert (T["measures"][:, 1] == 0).all()
    finally:
        e.close()


def test_invert_tradeoff_writes_the_curve(tmp_path):
    """invert.run(..., maxiter=1, tradeoff_weights with the file's weight0, tradeoff_damps its damp): every file of the plain run
    byte-identical, plus Tradeoff.dat with one line per member; the member with the file's parameters is the iteration's own update"""
    c = taipei.load()
    w0, damp = float(c["weight0"]), float(c["damp"])
    weights = [f32(0.25 * w0), w0, f32(4.0 * w0), f32(16.0 * w0)]
    damps = [damp, f32(0.5 * damp)]
    plain, sweep = tmp_path / "plain", tmp_path / "sweep"
    plain.mkdir(); sweep.mkdir()
    lp, ls = [], []
    invert.run(taipei.HERE, maxiter=1, out_dir=str(plain), log=lp.append)
    _, hist = invert.run(taipei.HERE, maxiter=1, out_dir=str(sweep), log=ls.append, tradeoff_weights=weights, tradeoff_damps=damps)
    names = sorted(os.listdir(plain))
    assert sorted(os.listdir(sweep)) == sorted(names + ["DSurfTomo.inTradeoff.dat"])
    for nm in names:
        assert (plain / nm).read_bytes() == (sweep / nm).read_bytes(), nm
    assert [l for l in ls if not l.startswith(" tradeoff") and "(forward" not in l] == [l for l in lp if "(forward" not in l]
    assert sum(l.startswith(" tradeoff") for l in ls) == 1 + len(damps)
    ht = hist[0]["tradeoff"]
    assert ht["realisations"] == 8 and ht["iteration"] == 1 and ht["chunk"] % 64 == 0 and ht["calls"] == 1 and len(ht["corners"]) == 2
    rows = invert.read_tradeoff(str(sweep / "DSurfTomo.inTradeoff.dat"))
    assert len(rows) == 8 and rows == ht["members"]
    assert [(r["weight"], r["damp"]) for r in rows] == [(w, d) for w in weights for d in damps]
    # the iteration's own update against the member (weight0, damp)
    lib = invert.bind(load_library())
    vsf = np.asfortranarray(c["vels"].copy())
    st = invert.iteration_device(lib, c, vsf, np.ascontiguousarray(c["obst"]), lambda *_: None,
                                 tradeoff=dict(weights=weights, damps=damps, chunk=None))
    t = st["trade"]
    k = 2                                                            # (weights[1], damps[0])
    assert t["weight"][k] == np.float32(w0) and t["damp"][k] == np.float32(damp)
    assert same_bits(t["x"][k], st["dv"]) and int(t["itn"][k]) == st["itn"] and int(t["istop"][k]) == st["istop"]
    assert invert.tradeoff_members(t) == rows
    assert rows[k]["dv_min"] == st["dv_min"] and rows[k]["dv_max"] == st["dv_max"]
