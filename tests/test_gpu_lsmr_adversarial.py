"""The LSMR family's ordered reductions and member masks on the adversarial inputs of tests/lsmr_adversarial.py: host_nrm2, k_nrm2 and
k_dot (csrc/lsmr.hip, both placements of the vectors) and k_pm_blockmax / k_pm_scan / k_pm_terms / k_b_chain with batch_solve's
F_ACT / F_BPOS / F_APOS / F_SLOT / F_LIM masks (csrc/lsmr_batch.hip) against the oracle's dso_lsmr and dso_dnrm2 (pinned to the
reference's own objects by test_oracle_lsmr.py) and a NumPy fp32 twin of dnrm2 -- every comparison bit for bit.  What the inputs are
and that they do what they are for is tests/test_lsmr_adversarial_patterns.py (no device)."""
import numpy as np
import pytest

import _libs as L
import inversion as inv
import lsmr_adversarial as A
import parity_log
from dsurftomo_amd.engine import Engine
from test_gpu_lsmr_batch import load, realisation, scaled

pytestmark = pytest.mark.gpu


def probe_paths(W, empty=False):
    """the norm probe of every row of W (R, n) through the three device paths; returns {path: list of dict(itn, istop, normr, x)}"""
    n = W.shape[1]
    S = A.probe_system(W[0], empty)
    out = {}
    e = Engine(0)
    try:
        load(e, S)
        for dvec in (0, 1):
            e.set_option("lsmr_device_vectors", dvec)
            out["dsa_lsmr, vectors on the %s" % ("device" if dvec else "host")] = [e.lsmr(w, 0.0) for w in W]
        e.set_option("lsmr_device_vectors", 0)
        B = e.lsmr_batch(np.ones(n, np.float32), W, 0.0)                 # u_r = fl(1 * w_r) = w_r
        out["dsa_lsmr_batch"] = [realisation(B, r) for r in range(W.shape[0])]
    finally:
        e.close()
    return out


def assert_probe(n, empty=False):
    labels, W = A.probe_vectors(n)
    assert len(labels) > 64                                              # more than one lane group in the batch
    twin, _ = A.dnrm2_twin(W)
    O = L.oracle()
    wants = [inv.call_lsmr(O.dso_lsmr, A.probe_system(w, empty), 0.0) for w in W]
    for k, w in enumerate(W):                                            # the three references agree (also asserted without a device)
        assert wants[k]["itn"] == 0 and wants[k]["istop"] == 0 and not wants[k]["x"].any()
        assert A.bits(wants[k]["normr"]) == A.bits(A.oracle_dnrm2(w)) == A.bits(twin[k]), labels[k]
    bad = {}
    for path, got in probe_paths(W, empty).items():
        for k, g in enumerate(got):
            if A.bits(g["normr"]) != A.bits(wants[k]["normr"]) or g["itn"] != 0 or g["istop"] != 0 or g["x"].any() or inv.same(g, wants[k]):
                bad.setdefault(path, []).append("%s: normr %r, the reference's %r, itn %d istop %d" % (labels[k], g["normr"], wants[k]["normr"], g["itn"], g["istop"]))
    parity_log.add("lsmr adversarial norm probe, length %d%s: %d vectors x 3 device paths, %d differ from the reference's dnrm2" %
                   (n, " (matrix without entries)" if empty else "", len(labels), sum(len(v) for v in bad.values())))
    assert not bad, {p: (len(v), v[:6]) for p, v in bad.items()}


@pytest.mark.parametrize("n", A.PROBE_LENGTHS)
def test_norm_probe(n):
    """normr of a solve that leaves before its first iteration is dnrm2 of the prescribed right-hand side: host_nrm2, k_nrm2 and the
    batch's chain (all vectors of the length in one call) return the bits of dso_lsmr, dso_dnrm2 and the NumPy twin on every
    profile, decade count and zero mask, with itn = 0, istop = 0 and x = 0"""
    assert_probe(n)


@pytest.mark.parametrize("n", A.EMPTY_LENGTHS)
def test_norm_probe_on_a_matrix_without_entries(n):
    """the same probe with nar = 0: dsa_spmv_load admits it, and both products are then the identity on their output"""
    assert_probe(n, empty=True)


@pytest.mark.parametrize("si", range(len(A.SHAPES)), ids=["%dx%d" % s for s in A.SHAPES])
def test_single_solves(si):
    """dsa_lsmr in both placements == dso_lsmr in every output bit, under each of the seven argument sets, on the shape's six
    (matrix profile, right-hand side, decades) combinations"""
    shape = A.SHAPES[si]
    O = L.oracle()
    bad, codes, nsolve = {}, set(), 0
    e = Engine(0)
    try:
        for ai, args in enumerate(A.ARGSETS):
            damp, kw = A.solve_kw(args)
            for combo in A.six_combos(si, ai):
                S = A.system(shape, *combo)
                want = inv.call_lsmr(O.dso_lsmr, S, damp, **kw)
                codes.add((want["istop"], want["itn"] >= 4))
                load(e, S)
                for dvec in (0, 1):
                    e.set_option("lsmr_device_vectors", dvec)
                    diff = inv.same(e.lsmr(S["b"], damp, **kw), want)
                    nsolve += 1
                    if diff:
                        bad[(ai + 1, combo, "device" if dvec else "host")] = (diff, want["itn"], want["istop"])
    finally:
        e.close()
    parity_log.add("lsmr adversarial single solves %d x %d: %d solves, %d differ from the oracle; stop codes after >= 4 iterations %s" %
                   (shape[0], shape[1], nsolve, len(bad), sorted(c for c, late in codes if late)))
    assert not bad, "(argument set, combination, vectors on): (fields differing, the oracle's itn, istop) %s" % bad


def batch_wants(S, sc, damp, kw):
    O = L.oracle()
    return [inv.call_lsmr(O.dso_lsmr, scaled(S, s), damp, **kw) for s in sc]


def differing(B, wants, labels):
    bad = {}
    for r, w in enumerate(wants):
        diff = inv.same(realisation(B, r), w)
        if diff:
            bad["%d (%s)" % (r, labels[r])] = (diff, "oracle itn %d istop %d, batch itn %d istop %d" % (w["itn"], w["istop"], B["itn"][r], B["istop"][r]))
    return bad


@pytest.mark.parametrize("shape", A.SHAPES, ids=lambda s: "%dx%d" % s)
def test_mixed_fate_batch(shape):
    """one resident matrix, 77 members (two lane groups) under each argument set: every member == dso_lsmr on its explicitly scaled
    system in every output bit, and the first lane group holds beta = 0, alpha = 0, an early stop and an itnlim runner in one call"""
    S = A.batch_system(shape)
    labels, sc = A.batch_members(shape)
    assert len(labels) > 64
    want_fates = {"beta = 0", "early"} if shape[0] < 4 else {"beta = 0", "alpha = 0", "early", "itnlim"}
    bad, missing, codes = {}, {}, set()
    e = Engine(0)
    try:
        load(e, S)
        for ai, args in enumerate(A.ARGSETS):
            damp, kw = A.solve_kw(args)
            B = e.lsmr_batch(S["b"], sc, damp, **kw)
            wants = batch_wants(S, sc, damp, kw)
            d = differing(B, wants, labels)
            if d:
                bad[ai + 1] = d
            if not A.fates(B["itn"], B["istop"], labels) >= want_fates:
                missing[ai + 1] = (sorted(want_fates - A.fates(B["itn"], B["istop"], labels)), B["itn"][:64].tolist())
            codes |= {int(v) for v in B["istop"]}
    finally:
        e.close()
    parity_log.add("lsmr adversarial mixed-fate batch %d x %d: %d members x %d argument sets, %d members differ from the oracle; stop codes %s" %
                   (shape[0], shape[1], len(labels), len(A.ARGSETS), sum(len(v) for v in bad.values()), sorted(codes)))
    assert not bad, "argument set: member: (fields differing, counters) %s" % bad
    assert not missing, "argument set: (fates absent from the first lane group, its itn) %s" % missing


@pytest.mark.parametrize("ai", A.ORDER_ARGSETS, ids=lambda a: "set%d" % (a + 1))
@pytest.mark.parametrize("shape", A.ORDER_SHAPES, ids=lambda s: "%dx%d" % s)
def test_batch_order_independence(shape, ai):
    """the members in reversed order give, member by member, the forward order's bytes (every member changes lane and lane group), and
    an early stopper, an itnlim runner and the alpha = 0 member give the same bytes alone (R = 1)"""
    S = A.batch_system(shape)
    labels, sc = A.batch_members(shape)
    damp, kw = A.solve_kw(A.ARGSETS[ai])
    R = len(labels)
    e = Engine(0)
    try:
        load(e, S)
        F = e.lsmr_batch(S["b"], sc, damp, **kw)
        Rv = e.lsmr_batch(S["b"], sc[::-1], damp, **kw)
        early = labels.index("one row")
        runner = int(np.flatnonzero(F["itn"] == A.ITNLIM)[0])
        alone = {r: e.lsmr_batch(S["b"], sc[r:r + 1], damp, **kw) for r in (early, runner, labels.index("empty rows"))}
    finally:
        e.close()
    assert 1 <= F["itn"][early] <= 3 and F["itn"][labels.index("empty rows")] == 0
    bad = {r: inv.same(realisation(Rv, R - 1 - r), realisation(F, r)) for r in range(R)}
    bad = {"%d (%s)" % (r, labels[r]): v for r, v in bad.items() if v}
    assert not bad, "members whose bytes change with the order: %s" % bad
    for r, B1 in alone.items():
        assert inv.same(realisation(B1, 0), realisation(F, r)) == [], (r, labels[r])
