"""The batched LSMR entry points (csrc/lsmr_batch.hip) share one kernel for u and the row scales and one set of measure kernels.  What
that sharing must keep equal across the entry points is pinned here side by side, in one process: the same system solved through dsa_lsmr,
dsa_lsmr_batch, dsa_lsmr_tradeoff and the full member of dsa_lsmr_crossval has the same bits everywhere, and the trade-off's measures are
the cross-validation's kept / roughness / size.  Then the tails of the measures' row kernel on the smallest system that has them all,
against the kernel's own order of additions in numpy float64: bit for bit, since every product of two floats is exact in fp64 and every
addition is the same IEEE operation on the same operands."""
import numpy as np
import pytest

import _libs as L
import inversion as inv
import synth
import synth_matrix as SM
from dsurftomo_amd.engine import Engine, load_library
from test_gpu_crossval import coefficients, ordered_rows, resid_python
from test_gpu_lsmr import system
from test_gpu_lsmr_batch import load, realisation
from test_gpu_tradeoff import same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def boundary():
    c = synth.boundary_case()
    S = system(c, weight0=2.0, fwd=L.call_boundary(load_library().dsa_calsurfg, c))
    assert c["ndata"] == S["m"] - S["n"]
    return S, c["ndata"]


@pytest.mark.parametrize("nreal,ncombo,nfolds", [(1, 1, 1), (65, 13, 4)])
def test_entry_points_agree_on_the_resident_system(boundary, nreal, ncombo, nfolds):
    """nreal members of (weight0, damp) = (2, 1) with row scales 1 -- 63 padding lanes, or a second lane group of one member: every member
    of dsa_lsmr_batch and dsa_lsmr_tradeoff and every full member of dsa_lsmr_crossval (ncombo x (nfolds + 1) members: 2, or 65) == dsa_lsmr
    in x, itn, istop and the estimates; the trade-off's measures == the full members' kept / roughness / size, held-out +0"""
    S, nd = boundary
    stride = nfolds + 1
    fold = (np.random.default_rng(8).permutation(nd) % nfolds).astype(np.int32)
    e = Engine(0)
    try:
        load(e, S)
        own = e.lsmr(S["b"], 1.0)
        B = e.lsmr_batch(S["b"], np.ones((nreal, S["m"]), np.float32), 1.0)
        T = e.lsmr_tradeoff(S["b"], nd, 2.0, [2.0] * nreal, [1.0] * nreal)
        V = e.lsmr_crossval(S["b"], nd, 2.0, [2.0] * ncombo, [1.0] * ncombo, fold, nfolds)
    finally:
        e.close()
    assert own["itn"] > 3
    assert B["x"].shape[0] == nreal and T["x"].shape[0] == nreal and V["x"].shape[0] == ncombo * stride
    for r in range(nreal):
        assert inv.same(realisation(B, r), own) == [], r
        assert inv.same(realisation(T, r), own) == [], r
        assert same_bits(T["measures"][r], T["measures"][0]), r
    for q in range(ncombo):
        full = q * stride + nfolds
        assert inv.same(realisation(V, full), own) == [], q
        assert same_bits(V["measures"][full, [0, 2, 3]], T["measures"][0]), q
        assert V["measures"][full, 1] == 0.0 and not np.signbit(V["measures"][full, 1])
        assert same_bits(V["resid"][q], V["resid"][0]), q
    assert T["measures"][0, 0] > 0 and T["measures"][0, 2] > 0


def tail_system():
    """58 ray-like data rows over 5 x 5 x 3 unknowns and their 75 regularisation rows (weight 2): m = 133 = 2 x 64 + 5, so the third block
    of the measures' row kernel has 5 rows and three of its wavefronts none"""
    M = SM.system(58, 5, 5, 3, seed=3, long_rows=0, mean_len=6)
    m, n, nar = M["m"], M["n"], M["rw"].size
    b = np.zeros(m, np.float32)
    b[:58] = (SM.mix(np.arange(58), 12) - 0.5).astype(np.float32)
    return dict(m=m, n=n, nar=nar, iw=np.concatenate([[nar], M["row"], M["col"]]).astype(np.int32), rw=M["rw"], b=b), 58


def block_sums(terms, per_block):
    """the kernels' order in float64: blocks of per_block terms, each of four wavefronts' consecutive quarters summed in order from 0, the
    four added ((w0 + w1) + w2) + w3, then the blocks in order from 0"""
    total = 0.0
    quarter = per_block // 4
    for b0 in range(0, len(terms), per_block):
        w = [0.0] * 4
        for k in range(4):
            for t in terms[b0 + k * quarter:min(b0 + (k + 1) * quarter, b0 + per_block)]:
                w[k] = w[k] + float(t)
        total = total + (((w[0] + w[1]) + w[2]) + w[3])
    return np.float64(total)


def test_measure_row_tails():
    """one combo x (2 folds + full) on tail_system: the measures and residuals of every member == the kernel's additions in the kernel's
    order, bit for bit; the trade-off's measures == the full member's"""
    S, nd = tail_system()
    m, n = S["m"], S["n"]
    lens = np.bincount(S["iw"][1:S["nar"] + 1] - 1, minlength=m)[:nd]
    assert m % 64 in range(1, 16)                                    # a last block of fewer than 16 rows: wavefronts without a row
    assert ((lens >= 1) & (lens <= 3)).any()                         # data rows that take the remainder loop alone
    assert ((lens >= 5) & (lens % 4 != 0)).any()                     # ... and the unrolled loop, then a remainder
    assert ((lens >= 4) & (lens % 4 == 0)).any()                     # ... and the unrolled loop alone
    fold = (np.arange(nd) % 2).astype(np.int32)
    e = Engine(0)
    try:
        load(e, S)
        V = e.lsmr_crossval(S["b"], nd, 2.0, [3.0], [0.5], fold, 2, itnlim=12)
        T = e.lsmr_tradeoff(S["b"], nd, 2.0, [3.0], [0.5], itnlim=12)
    finally:
        e.close()
    assert int(V["itn"].min()) > 3
    coef = coefficients(S, nd, 2.0)
    b = S["b"].astype(np.float64)
    zero = np.zeros(m)
    for k in range(3):
        x = V["x"][k]
        ax = ordered_rows(S, coef, x, m)
        d2 = np.concatenate([(b[:nd] - ax[:nd]) ** 2, zero[nd:]])
        held = np.concatenate([fold == k, np.zeros(m - nd, bool)])
        want = np.array([block_sums(np.where(held, 0.0, d2), 64), block_sums(np.where(held, d2, 0.0), 64),
                         block_sums(np.concatenate([zero[:nd], ax[nd:] ** 2]), 64), block_sums(x.astype(np.float64) ** 2, 1024)])
        assert same_bits(V["measures"][k], want), "member %d: measures %s, in the kernel's order %s" % (k, V["measures"][k], want)
    assert same_bits(V["resid"], resid_python(S, nd, coef, V, fold, 2))
    assert same_bits(T["x"][0], V["x"][2]) and same_bits(T["measures"][0], V["measures"][2, [0, 2, 3]])
