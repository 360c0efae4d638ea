"""dsa_lsmr_crossval (csrc/lsmr_batch.hip): K-fold cross-validation of (weight, damp) combos on one resident system whose regularisation
rows were built with weight0.  Member q (nfolds + 1) + f must equal, in every output bit (x, itn, istop, normA, condA, normr, normAr,
normx), dsa_lsmr -- or the oracle's restatement of the reference's LSMR -- with damp_q on the system REBUILT with weight_q whose data
rows of fold f are zeroed (entries fl(a * 0), right-hand side fl(b * 0)); member q (nfolds + 1) + nfolds on the rebuilt system itself.
The residuals must have the bits of a Python loop adding the fp64 products in storage order, and the measures must match numpy float64
within the worst-case bound of two fp64 evaluations in different orders.

Not tested: the DSA_ERR_ARGUMENT for a resid whose 2 ncombo ndata overflows.  The limit of 64 x 65535 members bounds ncombo below 2^22
and ndata is an int, so the product stays below 2^54: no call reaches that check on a 64-bit host."""
import ctypes as C
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
from test_gpu_tradeoff import same_bits

pytestmark = pytest.mark.gpu

COMBOS = [(2.0, 1.0), (0.0, 0.5), (3.0, 0.0)]
U = 2.0 ** -53


def f32(v):
    return float(np.float32(v))


def pick(T, idx):
    return dict(x=T["x"][idx], istop=T["istop"][idx], itn=T["itn"][idx], **{k: T[k][idx] for k in EST})


def rows_of(S):
    return S["iw"][1:S["nar"] + 1] - 1


def masked(S, nd, fold, f):
    """the system the contract writes out: every data row i < nd with fold[i] == f scaled by 0 (entries and right-hand side), the others by 1"""
    s = np.ones(S["m"], np.float32)
    s[:nd][np.asarray(fold[:nd]) == f] = 0.0
    T = dict(S)
    T["rw"] = (S["rw"] * s[rows_of(S)]).astype(np.float32)
    T["b"] = (S["b"] * s).astype(np.float32)
    return T


def deleted(S, nd, fold, f):
    """the system without the data rows of fold f, the remaining rows renumbered"""
    keep_row = np.ones(S["m"], bool)
    keep_row[:nd][np.asarray(fold[:nd]) == f] = False
    new = np.cumsum(keep_row) - 1
    rows, cols = rows_of(S), S["iw"][S["nar"] + 1:]
    k = keep_row[rows]
    nar = int(k.sum())
    return dict(m=int(keep_row.sum()), n=S["n"], nar=nar, rw=S["rw"][k].copy(), b=S["b"][keep_row].copy(),
                iw=np.concatenate([[nar], new[rows[k]] + 1, cols[k]]).astype(np.int32))


def coefficients(S, nd, weight0):
    rows = rows_of(S)
    coef = np.where(rows >= nd, np.rint(S["rw"] / np.float32(weight0)), S["rw"]).astype(np.float32)
    assert (coef[rows >= nd] != 0).all()
    return coef


def ordered_rows(S, coef, x, upto):
    """(A x)_i for the rows i < upto, float64, every row adding its products in storage order from 0 -- the loop the kernel runs"""
    rows, cols = rows_of(S), S["iw"][S["nar"] + 1:] - 1
    sel = np.flatnonzero(rows < upto)
    order = sel[np.argsort(rows[sel], kind="stable")]
    r = rows[order]
    prod = coef[order].astype(np.float64) * np.asarray(x, np.float64)[cols[order]]
    start = np.searchsorted(r, np.arange(upto))
    pos = np.arange(r.size) - start[r]
    acc = np.zeros(upto)
    for p in range(int(pos.max()) + 1 if pos.size else 0):
        at = pos == p
        acc[r[at]] = acc[r[at]] + prod[at]
    return acc


def resid_python(S, nd, coef, T, fold, nfolds):
    """resid as the contract states it, from the returned solutions"""
    S1 = nfolds + 1
    nc = T["x"].shape[0] // S1
    out = np.zeros((nc, 2, nd))
    b = S["b"][:nd].astype(np.float64)
    for q in range(nc):
        out[q, 1] = b - ordered_rows(S, coef, T["x"][q * S1 + nfolds], nd)
        for f in range(nfolds):
            at = np.asarray(fold[:nd]) == f
            if at.any():
                out[q, 0, at] = (b - ordered_rows(S, coef, T["x"][q * S1 + f], nd))[at]
    return out


def measures_numpy(S, nd, coef, x, held):
    """({kept sum r^2, held-out sum r^2, sum (C x)^2 over the rows from nd up, sum x^2}, their bounds) in numpy float64 on the solution x.
    Bound of each sum: 4 (Lmax + m) 2^-53 sum T_i^2, T_i = sum_j |a_ij x_j| + |b_i| (for sum x^2: T_j = |x_j|), the worst case of two fp64
    evaluations in different orders (test_gpu_tradeoff.measures_numpy, the data rows split by `held`); and per data row the residual
    with its bound 2 (L_i + 2) 2^-53 T_i: each evaluation of b_i - sum_j a_ij x_j rounds at most L_i + 1 times, each by at most 2^-53 of
    a partial sum that T_i bounds, and one more unit covers the second-order terms"""
    nar, m = S["nar"], S["m"]
    rows, cols = rows_of(S), S["iw"][nar + 1:] - 1
    x64 = np.asarray(x, np.float64)
    prod = coef.astype(np.float64) * x64[cols]
    ax = np.bincount(rows, weights=prod, minlength=m)
    t = np.bincount(rows, weights=np.abs(prod), minlength=m) + np.abs(S["b"].astype(np.float64))
    r = S["b"].astype(np.float64) - ax
    cnt = np.bincount(rows, minlength=m)
    eps = 4.0 * (int(cnt.max()) + m) * U
    h = np.zeros(m, bool); h[:nd] = held
    k = np.zeros(m, bool); k[:nd] = ~np.asarray(held)
    want = np.array([(r[k] ** 2).sum(), (r[h] ** 2).sum(), (ax[nd:] ** 2).sum(), (x64 ** 2).sum()])
    bound = eps * np.array([(t[k] ** 2).sum(), (t[h] ** 2).sum(), (t[nd:] ** 2).sum(), (x64 ** 2).sum()])
    return want, bound, r[:nd], 2.0 * (cnt[:nd] + 2) * U * t[:nd]


def assert_measures(T, S, nd, weight0, fold, nfolds, members=None):
    coef = coefficients(S, nd, weight0)
    S1 = nfolds + 1
    for k in (range(T["x"].shape[0]) if members is None else members):
        f = k % S1
        want, bound, _, _ = measures_numpy(S, nd, coef, T["x"][k], np.asarray(fold[:nd]) == f)
        got = T["measures"][k]
        print("member %d: measures %s numpy %s |difference| %s bound %s" % (k, got, want, np.abs(got - want), bound))
        assert (np.abs(got - want) <= bound).all(), (k, got, want, bound)
        assert (got >= 0).all()
        if f == nfolds:
            assert got[1] == 0.0 and not np.signbit(got[1])


def assert_resid_bound(T, S, nd, weight0, fold, nfolds, combos):
    coef = coefficients(S, nd, weight0)
    S1 = nfolds + 1
    for q in combos:
        for f in range(S1):
            _, _, r, rb = measures_numpy(S, nd, coef, T["x"][q * S1 + f], np.zeros(nd, bool))
            at = np.ones(nd, bool) if f == nfolds else np.asarray(fold[:nd]) == f
            got = T["resid"][q, 1 if f == nfolds else 0]
            print("combo %d member %d: max |resid - numpy| %.3g, max bound %.3g" % (q, f, np.abs(got - r)[at].max(initial=0.0), rb[at].max(initial=0.0)))
            assert (np.abs(got - r)[at] <= rb[at]).all(), (q, f)


def assert_same_result(A, B):
    for k in ("x", "measures", "resid", "istop", "itn") + EST:
        assert same_bits(A[k], B[k]), k


@pytest.fixture(scope="module")
def boundary():
    c = synth.boundary_case()
    return c, L.call_boundary(load_library().dsa_calsurfg, c)


def boundary_fold(nd, nfolds=3):
    return (np.random.default_rng(8).permutation(nd) % nfolds).astype(np.int32)


@pytest.mark.parametrize("local_size,itnlim", [(10, 400), (0, 100), (3, 7)])
def test_crossval_boundary_case_against_the_oracle(boundary, local_size, itnlim):
    """3 combos x (3 folds + full) = 12 members: each == the oracle's LSMR on the explicitly masked system rebuilt with its weight; the
    full members == lsmr_tradeoff; resid == the ordered Python loop; the measures == numpy; the same bits without x"""
    c, fwd = boundary
    S = system(c, weight0=2.0, fwd=fwd)
    nd, nf = c["ndata"], 3
    assert nd == S["m"] - S["n"]
    fold = boundary_fold(nd)
    w = [m[0] for m in COMBOS]
    d = [m[1] for m in COMBOS]
    kw = dict(itnlim=itnlim, local_size=local_size)
    e = Engine(0)
    try:
        load(e, S)
        T = e.lsmr_crossval(S["b"], nd, 2.0, w, d, fold, nf, **kw)
        T2 = e.lsmr_crossval(S["b"], nd, 2.0, w, d, fold, nf, want_x=False, **kw)
        T3 = e.lsmr_crossval(S["b"], nd, 2.0, w, d, fold, nf, want_x=False, want_resid=False, **kw)
        R = e.lsmr_tradeoff(S["b"], nd, 2.0, w, d, **kw)
    finally:
        e.close()
    assert T["x"].shape == (12, S["n"]) and T["measures"].shape == (12, 4) and T["resid"].shape == (3, 2, nd)
    wants = []
    for wk, dk in COMBOS:
        Sk = system(c, weight0=f32(wk), fwd=fwd)
        assert Sk["nar"] == S["nar"] and np.array_equal(Sk["iw"], S["iw"]) and same_bits(Sk["b"], S["b"])
        for f in range(nf + 1):
            wants.append(inv.call_lsmr(L.oracle().dso_lsmr, masked(Sk, nd, fold, f), f32(dk), **kw))
    assert_all_equal(T, wants)
    assert max(v["itn"] for v in wants) > 3
    full = [q * (nf + 1) + nf for q in range(3)]
    assert_all_equal(pick(T, full), [realisation(R, q) for q in range(3)])
    for j, col in ((0, 0), (2, 1), (3, 2)):
        assert same_bits(np.ascontiguousarray(T["measures"][full, j]), np.ascontiguousarray(R["measures"][:, col])), j
    assert (T["measures"][full, 1] == 0).all() and not np.signbit(T["measures"][full, 1]).any()
    assert same_bits(T["resid"], resid_python(S, nd, coefficients(S, nd, 2.0), T, fold, nf))
    assert_measures(T, S, nd, 2.0, fold, nf)
    assert T2["x"] is None and same_bits(T2["measures"], T["measures"]) and same_bits(T2["resid"], T["resid"])
    assert T3["x"] is None and T3["resid"] is None and same_bits(T3["measures"], T["measures"])
    assert np.array_equal(T2["itn"], T["itn"]) and np.array_equal(T2["istop"], T["istop"])
    if itnlim == 400:                                               # a held-out fold is predicted worse than it is fitted
        held = T["measures"][:nf, 1].sum()
        fit = (T["resid"][0, 1] ** 2).sum()
        assert held > fit > 0


def test_crossval_masked_equals_deleted(boundary):
    """two members against dsa_lsmr on the system with their held-out rows removed and the rest renumbered"""
    c, fwd = boundary
    S = system(c, weight0=2.0, fwd=fwd)
    nd, nf = c["ndata"], 3
    fold = boundary_fold(nd)
    e = Engine(0)
    try:
        load(e, S)
        T = e.lsmr_crossval(S["b"], nd, 2.0, [2.0], [1.0], fold, nf)
        for f in (0, 2):
            D = deleted(S, nd, fold, f)
            assert D["m"] == S["m"] - int((fold == f).sum()) < S["m"]
            load(e, D)
            want = e.lsmr(D["b"], 1.0)
            got = realisation(T, f)
            assert np.array_equal(got["x"], want["x"]) and got["itn"] == want["itn"] and got["istop"] == want["istop"]
            assert inv.same(got, want) == []
            assert want["itn"] > 3
    finally:
        e.close()


@pytest.fixture(scope="module")
def taipei_forward():
    c = taipei.load()
    return c, L.call_boundary(load_library().dsa_calsurfg, c)


def test_crossval_taipei_crosses_a_lane_group(taipei_forward):
    """5 folds by path x 11 weights = 66 members on the first iteration's Taipei system (built with weight 4): combo 10 straddles lanes
    63|64; members 0, 5, 31, 63, 64, 65 against dsa_lsmr on the rebuilt, masked systems; the other solvers and a second call keep their bits"""
    c, fwd = taipei_forward
    S = inv.build_system(c, fwd, c["obst"], 3.0, 4.0)
    nd, nf = c["ndata"], 5
    fold = invert.crossval_folds(c, nf, "path", 1)
    w, d = invert.tradeoff_grid(np.geomspace(0.25, 64.0, 11), [1.0])
    assert w.size * (nf + 1) == 66
    some = [0, 5, 31, 63, 64, 65]
    ones = np.ones((1, S["m"]), np.float32)
    e = Engine(0)
    try:
        load(e, S)
        own0 = e.lsmr(S["b"], 1.0)
        B0 = e.lsmr_batch(S["b"], ones, 1.0)
        R0 = e.lsmr_tradeoff(S["b"], nd, 4.0, w[:3], d[:3])
        T = e.lsmr_crossval(S["b"], nd, 4.0, w, d, fold, nf)
        own1 = e.lsmr(S["b"], 1.0)
        B1 = e.lsmr_batch(S["b"], ones, 1.0)
        R1 = e.lsmr_tradeoff(S["b"], nd, 4.0, w[:3], d[:3])
        T2 = e.lsmr_crossval(S["b"], nd, 4.0, w, d, fold, nf)
        wants = []
        for k in some:
            q, f = divmod(k, nf + 1)
            Sk = inv.build_system(c, fwd, c["obst"], 3.0, float(w[q]))
            assert same_bits(Sk["b"], S["b"]) and np.array_equal(Sk["iw"], S["iw"])
            Mk = masked(Sk, nd, fold, f)
            load(e, Mk)
            wants.append(e.lsmr(Mk["b"], float(d[q])))
    finally:
        e.close()
    assert_all_equal(pick(T, some), wants)
    assert inv.same(own1, own0) == []
    assert inv.same(realisation(B1, 0), realisation(B0, 0)) == [] and inv.same(realisation(B0, 0), own0) == []
    for k in ("x", "measures", "istop", "itn") + EST:
        assert same_bits(R0[k], R1[k]), k
    assert_all_equal(pick(T, [5, 11, 17]), [realisation(R0, q) for q in range(3)])
    assert_same_result(T2, T)
    assert len(set(int(v) for v in T["itn"])) >= 2
    assert_resid_bound(T, S, nd, 4.0, fold, nf, [10])
    assert_measures(T, S, nd, 4.0, fold, nf, members=[60, 63, 64, 65])


def multiblock():
    M = SM.system(31522, 47, 47, 31, seed=11)
    m, n, nar = M["m"], M["n"], M["rw"].size
    b = np.zeros(m, np.float32)
    b[:31522] = (SM.mix(np.arange(31522), 12) - 0.5).astype(np.float32)
    return dict(m=m, n=n, nar=nar, iw=np.concatenate([[nar], M["row"], M["col"]]).astype(np.int32), rw=M["rw"], b=b), M["nar_data"]


def test_crossval_multiblock_system():
    """the 100 001 x 68 479 system of test_lsmr_multiblock_system (regularisation rows of weight 2): 1 combo x 2 folds = 3 members
    against the oracle's LSMR on the masked systems whose regularisation rows synth_matrix rebuilds with the weight; measures against numpy"""
    S, nar_data = multiblock()
    nd, nf = 31522, 2
    wk, dk = 0.5, 0.7
    fold = (SM.mix(np.arange(nd), 5) * nf).astype(np.int32)
    assert set(fold.tolist()) == {0, 1}
    e = Engine(0)
    try:
        load(e, S)
        T = e.lsmr_crossval(S["b"], nd, 2.0, [wk], [dk], fold, nf, itnlim=35)
    finally:
        e.close()
    rr, rc, rv = SM.regularisation_rows(47, 47, 31, wk, nd)
    assert np.array_equal(rr + 1, S["iw"][1 + nar_data:S["nar"] + 1]) and np.array_equal(rc + 1, S["iw"][S["nar"] + 1 + nar_data:])
    Sk = dict(S, rw=np.concatenate([S["rw"][:nar_data], rv]).astype(np.float32))
    wants = [inv.call_lsmr(L.oracle().dso_lsmr, masked(Sk, nd, fold, f), dk, itnlim=35) for f in range(nf + 1)]
    assert max(v["itn"] for v in wants) > 3
    assert_all_equal(T, wants)
    assert_measures(T, S, nd, 2.0, fold, nf)
    assert_resid_bound(T, S, nd, 2.0, fold, nf, [0])


def test_crossval_edges(boundary):
    c, fwd = boundary
    S = system(c, weight0=2.0, fwd=fwd)
    nd, m = c["ndata"], S["m"]
    assert not S["b"][nd:].any()
    e = Engine(0)
    try:
        load(e, S)
        own = e.lsmr(S["b"], 1.0)
        # nfolds = 1: member 0 holds out every datum, its right-hand side is zero
        T = e.lsmr_crossval(S["b"], nd, 2.0, [2.0], [1.0], np.zeros(nd, np.int32), 1)
        assert not T["x"][0].any() and T["itn"][0] == 0 and T["istop"][0] == 0
        assert T["measures"][0, 0] == 0 and T["measures"][0, 2] == 0 and T["measures"][0, 3] == 0
        b64 = S["b"][:nd].astype(np.float64)
        want = (b64 ** 2).sum()
        bound = 4.0 * (int(np.bincount(rows_of(S), minlength=m).max()) + m) * U * want
        print("nfolds 1: held-out %r sum b^2 %r |difference| %.3g bound %.3g" % (T["measures"][0, 1], want, abs(T["measures"][0, 1] - want), bound))
        assert abs(T["measures"][0, 1] - want) <= bound
        assert same_bits(T["resid"][0, 0], b64)
        assert inv.same(realisation(T, 1), own) == []
        # a fold id nobody uses: that member is the full member
        fold = np.array([0, 1, 3], np.int32)[np.arange(nd) % 3]
        T = e.lsmr_crossval(S["b"], nd, 2.0, [0.7], [0.3], fold, 4)
        assert inv.same(realisation(T, 2), realisation(T, 4)) == []
        assert same_bits(T["measures"][2], T["measures"][4]) and T["measures"][2, 1] == 0
        assert inv.same(realisation(T, 0), realisation(T, 4)) != []
        # ndata = m: no regularisation rows, every row may be held out and every weight gives the resident system
        fold = (np.random.default_rng(3).permutation(m) % 2).astype(np.int32)
        T = e.lsmr_crossval(S["b"], m, 2.0, [0.0, 5.0], [1.0, 1.0], fold, 2)
        assert T["resid"].shape == (2, 2, m)
    finally:
        e.close()
    wants = [inv.call_lsmr(L.oracle().dso_lsmr, masked(S, m, fold, f), 1.0) for f in range(3)]
    assert_all_equal(T, wants + wants)
    assert inv.same(wants[2], own) == []
    assert (T["measures"][:, 2] == 0).all()


def raw(e, S, nd, **kw):
    """dsa_lsmr_crossval through ctypes with 2 combos x (3 folds + full) by default; a key set to None passes a null pointer"""
    f = np.float32
    a = dict(ncombo=2, nfolds=3, ndata=nd, b=S["b"], weight0=2.0, weight=np.array([1.0, 2.0], f), damp=np.array([1.0, 1.0], f),
             fold=(np.arange(max(nd, 1)) % 3).astype(np.int32))
    a.update(kw)
    K = 8
    out = dict(x=np.zeros((K, S["n"]), f), measures=np.zeros((K, 4)), resid=np.zeros((2, 2, max(nd, 1) + 1)), istop=np.zeros(K, np.int32),
               itn=np.zeros(K, np.int32), est=np.zeros((K, 5), f))
    out.update({k: kw[k] for k in out if k in kw})
    ptr = lambda v: None if v is None else np.ascontiguousarray(v).ctypes.data_as(C.c_void_p)
    keep = [np.ascontiguousarray(a[k]) if a[k] is not None else None for k in ("b", "weight", "damp", "fold")]
    return e._L.dsa_lsmr_crossval(e._h, a["ncombo"], a["nfolds"], a["ndata"], ptr(keep[0]), a["weight0"], ptr(keep[1]), ptr(keep[2]), ptr(keep[3]),
                                  1e-6, 1e-6, 100.0, 400, 10, ptr(out["x"]), ptr(out["measures"]), ptr(out["resid"]), ptr(out["istop"]), ptr(out["itn"]),
                                  ptr(out["est"]))


def test_crossval_errors(boundary):
    c, fwd = boundary
    S = system(c, weight0=2.0, fwd=fwd)
    nd, m = c["ndata"], S["m"]
    f = np.float32
    fold = (np.arange(nd) % 3).astype(np.int32)
    e = Engine(0)
    try:
        e._mn = (S["m"], S["n"])                                      # (what spmv_load would note: the binding sizes its arrays from it)
        with pytest.raises(EngineError) as exc:
            e.lsmr_crossval(S["b"], nd, 2.0, [1.0], [1.0], fold, 3)
        assert exc.value.code == -5 and "dsa_spmv_load" in str(exc.value)            # DSA_ERR_STATE: no matrix yet
        load(e, S)
        want = e.lsmr(S["b"], 1.0)
        low, high = fold.copy(), fold.copy()
        low[nd // 2] = -1
        high[nd - 1] = 3
        bad = [dict(ncombo=0), dict(ncombo=-1), dict(nfolds=0), dict(nfolds=-2),
               dict(nfolds=64 * 65535 // 2),                          # 2 x (nfolds + 1) members: two more than one call takes (rejected before any array is touched)
               dict(ndata=0), dict(ndata=m + 1), dict(b=None), dict(weight=None), dict(damp=None), dict(fold=None), dict(istop=None), dict(itn=None),
               dict(est=None), dict(weight0=float("nan")), dict(weight0=float("inf")), dict(weight0=0.0), dict(weight0=-2.0),
               dict(weight=np.array([1.0, -0.5], f)), dict(weight=np.array([float("inf"), 1.0], f)), dict(damp=np.array([1.0, float("nan")], f)),
               dict(damp=np.array([-1.0, 1.0], f)), dict(fold=low), dict(fold=high),
               dict(weight0=3.0)]                                     # the regularisation entries are fl(c * 2), not fl(c * 3)
        for kw in bad:
            assert raw(e, S, nd, **kw) == -2, kw                     # DSA_ERR_ARGUMENT
            # the engine is still usable, with the weight it was built with
            assert inv.same(e.lsmr(S["b"], 1.0), want) == [], kw
        assert raw(e, S, nd) == 0
        assert raw(e, S, nd, x=None, measures=None, resid=None) == 0
        T = e.lsmr_crossval(S["b"], nd, 2.0, [2.0], [1.0], fold, 3)
        assert inv.same(realisation(T, 3), want) == []
    finally:
        e.close()


def test_invert_crossval_writes_the_scores(tmp_path):
    """invert.run(..., maxiter=1, crossval=5 by path over three weights): every file of the plain run byte-identical, plus Crossval.dat and
    CrossvalResiduals.dat; the full member with the file's parameters is the iteration's own update"""
    c = taipei.load()
    w0, damp = float(c["weight0"]), float(c["damp"])
    weights = [f32(0.25 * w0), w0, f32(4.0 * w0)]
    plain, cv = tmp_path / "plain", tmp_path / "cv"
    plain.mkdir(); cv.mkdir()
    lp, lc = [], []
    invert.run(taipei.HERE, maxiter=1, out_dir=str(plain), log=lp.append)
    _, hist = invert.run(taipei.HERE, maxiter=1, out_dir=str(cv), log=lc.append, crossval=5, crossval_weights=weights, crossval_by="path", crossval_seed=2)
    names = sorted(os.listdir(plain))
    assert sorted(os.listdir(cv)) == sorted(names + ["DSurfTomo.inCrossval.dat", "DSurfTomo.inCrossvalResiduals.dat"])
    for nm in names:
        assert (plain / nm).read_bytes() == (cv / nm).read_bytes(), nm
    assert [l for l in lc if not l.startswith(" crossval") and "(forward" not in l] == [l for l in lp if "(forward" not in l]
    assert sum(l.startswith(" crossval") for l in lc) == 3
    hx = hist[0]["crossval"]
    assert hx["realisations"] == 18 and hx["iteration"] == 1 and hx["nfolds"] == 5 and hx["calls"] == 1 and hx["by"] == "path"
    assert len(hx["cv_rms_by_slot"]) == c["kmax"]
    rows = invert.read_crossval(str(cv / "DSurfTomo.inCrossval.dat"))
    assert len(rows) == 3 and rows == hx["members"]
    assert [(r["weight"], r["damp"]) for r in rows] == [(w, damp) for w in weights]
    assert invert.crossval_select(rows) == dict(best=hx["best"], one_se=hx["one_se"])
    assert all(r["cv_rms"] > r["train_rms"] > 0 and r["cv_se"] > 0 for r in rows)
    res = np.loadtxt(str(cv / "DSurfTomo.inCrossvalResiduals.dat"))
    fold = invert.crossval_folds(c, 5, "path", 2)
    assert res.shape == (c["ndata"], 7) and np.array_equal(res[:, 0], np.arange(1, c["ndata"] + 1)) and np.array_equal(res[:, 3], fold)
    one = rows[hx["one_se"]]
    assert np.sqrt((res[:, 5] ** 2).sum() / c["ndata"]) == pytest.approx(one["cv_rms"], rel=1e-12)
    assert np.sqrt((res[:, 6] ** 2).sum()) == pytest.approx(one["misfit"], rel=1e-12)
    # the iteration's own update against the full member of (weight0, damp)
    lib = invert.bind(load_library())
    vsf = np.asfortranarray(c["vels"].copy())
    st = invert.iteration_device(lib, c, vsf, np.ascontiguousarray(c["obst"]), lambda *_: None,
                                 crossval=dict(weights=weights, damps=[damp], fold=fold, nfolds=5, chunk=2, want_x=True))
    t = st["crossval"]
    k = 1 * 6 + 5
    assert t["calls"] == 2 and t["weight"][1] == np.float32(w0) and t["damp"][1] == np.float32(damp)
    assert same_bits(t["x"][k], st["dv"]) and int(t["itn"][k]) == st["itn"] and int(t["istop"][k]) == st["istop"]
    assert invert.crossval_members(t, fold) == rows                   # two calls give what one gives
