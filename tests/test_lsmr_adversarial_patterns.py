"""The adversarial LSMR inputs of tests/lsmr_adversarial.py on the oracle alone (no device): the vectors and systems do what
test_gpu_lsmr_adversarial.py needs them to do -- the norm probe returns dnrm2 of its vector and nothing else, the NumPy twin of dnrm2
equals dso_dnrm2 on every probe vector, the iterating systems stay finite and reach the stop codes 1, 2, 3, 4, 5 and 7 after at least
four iterations, and the first lane group of every mixed-fate batch holds members of every fate.  dso_lsmr and dso_dnrm2 are pinned
to the reference's own objects by test_oracle_lsmr.py."""
import collections

import numpy as np
import pytest

import _libs as L
import inversion as inv
import lsmr_adversarial as A
from test_gpu_lsmr_batch import scaled

EST = ("normA", "condA", "normr", "normAr", "normx")


def finite(r):
    return bool(np.isfinite(r["x"]).all() and all(np.isfinite(r[k]) for k in EST))


def test_profiles_are_what_they_claim():
    """asc: every element a new maximum; desc: the first alone; saw: every batch of 64 repeats the first one's magnitudes; ties: one
    magnitude; late: the last element alone is large; all finite fp32 normals; squared ratios reach the denormal range and zero"""
    tiny = np.finfo(np.float32).tiny
    for D in A.PROBE_DECADES:
        for salt in A.PROBE_SALTS:
            for p in A.PROFILES:
                w = A.profile(p, 2305, D, salt)
                assert np.isfinite(w).all() and (np.abs(w) >= tiny).all(), (p, D)
                assert (w < 0).any() and (w > 0).any(), (p, D)
            a = np.abs(A.profile("asc", 2305, D, salt))
            assert (a[1:] > a[:-1]).all()
            d = np.abs(A.profile("desc", 2305, D, salt))
            assert (d[1:] <= d[:-1]).all()               # (an equal neighbour is no new maximum either)
            s = np.abs(A.profile("saw", 2305, D, salt))
            assert all(np.array_equal(s[k:k + 64], s[:min(64, 2305 - k)]) for k in range(64, 2305, 64))
            assert len(set(np.abs(A.profile("ties", 2305, D, salt)))) == 1
            l = np.abs(A.profile("late", 2305, D, salt))
            assert float(l[-1]) > 10.0 ** (D - 1) * float(l[:-1].max())
    for D in (30.0, 50.0):
        a = np.abs(A.profile("asc", 2305, D)).astype(np.float32)
        q = (a[:-1] / a[-1]).astype(np.float32)
        qq = q * q
        assert (qq == 0).any() and ((qq > 0) & (qq < tiny)).any(), D


@pytest.fixture(scope="module")
def probe():
    """per length: (labels, vectors, the twin's norms, new running maxima per vector)"""
    out = {}
    for n in A.PROBE_LENGTHS:
        labels, W = A.probe_vectors(n)
        out[n] = (labels, W) + A.dnrm2_twin(W)
    return out


def test_probe_returns_dnrm2_and_nothing_else(probe):
    """every probe vector: the oracle's LSMR leaves with itn = 0, istop = 0, x = 0 and a finite normr == dso_dnrm2 == the twin, bit
    for bit, and 1 / normr is finite; the same on the matrix without entries"""
    O = L.oracle()
    total = 0
    for n, (labels, W, twin, count) in probe.items():
        assert len(labels) > 64 and len(set(labels)) == len(labels)
        for k, w in enumerate(W):
            assert w.any()
            want = A.oracle_dnrm2(w)
            for empty in ((False, True) if n in A.EMPTY_LENGTHS else (False,)):
                r = inv.call_lsmr(O.dso_lsmr, A.probe_system(w, empty), 0.0)
                assert r["itn"] == 0 and r["istop"] == 0 and not r["x"].any(), (n, labels[k])
                assert np.isfinite(r["normr"]) and A.bits(r["normr"]) == A.bits(want), (n, labels[k])
            assert A.bits(twin[k]) == A.bits(want), (n, labels[k], twin[k], want)
            assert np.isfinite(np.float32(1.0) / want) and want > 0, (n, labels[k])
        total += len(labels)
    assert total > 3000


def test_probe_covers_the_branches(probe):
    """new running maxima per vector from 1 to more than 2 000 over the set; from 65 elements on (a second batch of 64 exists) every
    length has a vector with a whole zero batch; ties and saw meet `scale == |x|` (an element equal to the running maximum)"""
    counts = np.concatenate([c for _, _, _, c in probe.values()])
    assert counts.min() == 1 and counts.max() > 2000
    for n, (labels, W, _, _) in probe.items():
        if n > 64:
            assert any(A.has_zero_batch(w) for w in W), n
        for name in ("ties", "saw") if n >= 128 else ("ties",) if n > 1 else ():      # (saw: a second whole batch of 64)
            w = np.abs(next(W[k] for k, lb in enumerate(labels) if lb.startswith(name + " ") and " none " in lb))
            run = np.maximum.accumulate(w)
            assert (w[1:] == run[:-1]).any(), (n, name)


def test_twin_against_the_pinned_kinds():
    """the twin on the four kinds of vector test_oracle_lsmr.py pins dso_dnrm2 with (random, zeros inside, sorted, scaled by 1e-20)"""
    import synth
    r = synth.LCG(5)
    for n in (1, 2, 7, 64, 1000, 4097):
        X = []
        for kind in range(4):
            x = (r.uniform(n) - 0.5).astype(np.float32)
            if kind == 1: x[::3] = 0.0
            if kind == 2: x = np.sort(np.abs(x)).astype(np.float32)
            if kind == 3: x *= np.float32(1e-20)
            X.append(x)
        twin, _ = A.dnrm2_twin(np.stack(X))
        for k, x in enumerate(X):
            assert A.bits(twin[k]) == A.bits(A.oracle_dnrm2(x)), (n, k)


def test_matrix_layout():
    """sorted by row then column, the last two rows empty from m = 4 on, one entry per extra row (m > n) or column (n > m)"""
    for m, n in A.SHAPES:
        S = A.matrix(m, n, "wild", 6.0)
        nar = S["nar"]
        row, col = S["iw"][1:nar + 1].astype(np.int64), S["iw"][nar + 1:].astype(np.int64)
        assert S["iw"][0] == nar and S["iw"].size == 2 * nar + 1 and row.min() >= 1 and col.min() >= 1 and col.max() <= n
        key = row * (n + 1) + col
        assert (key[1:] > key[:-1]).all()
        assert row.max() == (m - 2 if m >= 4 else m)
        k = min(m, n)
        assert nar == max(m, n) - (2 if m >= 4 else 0)
        if n > m:
            assert (np.bincount(col - 1, minlength=n)[k:] == 1).all()
        if m > n:
            assert (np.bincount(row - 1, minlength=m)[k:row.max()] == 1).all()
        assert np.isfinite(S["rw"]).all() and (S["rw"] != 0).all()
    for si in range(len(A.SHAPES)):
        for ai in range(len(A.ARGSETS)):
            six = A.six_combos(si, ai)
            assert sorted(c[0] for c in six) == sorted(A.PROFILES) and {c[1] for c in six} == set(A.B_PROFILES) and {c[2] for c in six} == set(A.DECADES)


def test_iterating_systems_stay_finite_and_reach_the_stop_codes():
    """the full product shapes x matrix profiles x right-hand sides x decades x argument sets on the oracle: x and the five estimates
    finite everywhere, and each of the stop codes 1, 2, 3, 4, 5, 7 met after at least four iterations (0 is the probe's; 6 is outside
    the envelope).  The six combinations the device runs per (shape, argument set) reach them too."""
    O = L.oracle()
    codes, device_codes = collections.Counter(), collections.Counter()
    solves = 0
    for si, shape in enumerate(A.SHAPES):
        six = [set(A.six_combos(si, ai)) for ai in range(len(A.ARGSETS))]
        for combo in A.all_combos():
            S = A.system(shape, *combo)
            for ai, args in enumerate(A.ARGSETS):
                damp, kw = A.solve_kw(args)
                r = inv.call_lsmr(O.dso_lsmr, S, damp, **kw)
                assert finite(r), (shape, combo, ai, r)
                assert 0 <= r["itn"] <= A.ITNLIM
                solves += 1
                if r["itn"] >= 4:
                    codes[r["istop"]] += 1
                    if combo in six[ai]:
                        device_codes[r["istop"]] += 1
    print("oracle stop codes after >= 4 iterations over %d solves: %s; among the device's six per (shape, argument set): %s" %
          (solves, dict(sorted(codes.items())), dict(sorted(device_codes.items()))))
    assert solves == len(A.SHAPES) * 72 * len(A.ARGSETS)
    for code in (1, 2, 3, 4, 5, 7):
        assert codes[code] > 0, (code, dict(codes))
    for code in (1, 2, 3, 5, 7):                  # (code 4 is rare: the device meets it in the batches below)
        assert device_codes[code] > 0, (code, dict(device_codes))


@pytest.mark.parametrize("shape", A.SHAPES, ids=lambda s: "%dx%d" % s)
def test_mixed_fate_batches_on_the_oracle(shape):
    """every member of every argument set is finite on the explicitly scaled system, and the first lane group (the first 64 members)
    holds, in one call: itn = 0 by beta = 0, itn = 0 by alpha = 0, an itn in 1..3 and an itn = itnlim.  The shapes below 63 x 65 have
    no empty rows (no alpha = 0 member) and at most two unknowns (LSMR is done before itnlim): there beta = 0 and the early stop."""
    O = L.oracle()
    S = A.batch_system(shape)
    labels, sc = A.batch_members(shape)
    assert len(labels) > 64 and sc.shape == (len(labels), shape[0])
    assert {"one", "zero", "one row", "runs"} <= set(labels[:8])
    want = {"beta = 0", "early"} if shape[0] < 4 else {"beta = 0", "alpha = 0", "early", "itnlim"}
    for ai, args in enumerate(A.ARGSETS):
        damp, kw = A.solve_kw(args)
        rs = [inv.call_lsmr(O.dso_lsmr, scaled(S, s), damp, **kw) for s in sc]
        assert all(finite(r) for r in rs), (shape, ai)
        assert A.fates([r["itn"] for r in rs], [r["istop"] for r in rs], labels) >= want, (shape, ai)
        if shape[0] >= 4:
            e = rs[labels.index("empty rows")]
            assert e["itn"] == 0 and e["normr"] > 0 and e["normAr"] == 0          # beta > 0, alpha = 0
        z = rs[labels.index("zero")]
        assert z["itn"] == 0 and z["normr"] == 0
