"""Adversarial inputs for the LSMR family's ordered reductions (csrc/lsmr.hip: host_nrm2, k_nrm2, k_dot; csrc/lsmr_batch.hip:
k_pm_blockmax / k_pm_scan / k_pm_terms / k_b_chain) and for the per-member masks of batch_solve: vectors whose running maximum, ties,
underflowing ratios, zero batches and lengths are prescribed, not left to what a tomography system happens to produce.

Every value is sign_i * mant_i * 10**e_i (i = 0 .. L-1, t = i / (L-1), D decades), sign and mant in [1, 2) from synth_matrix.mix:

  asc    e = D (t - 1/2)                       every element a new running maximum (the magnitudes sorted upwards: the mantissas
                                               alone would undo a step of D / (L-1) decades)
  desc   e = D (1/2 - t)                       none after the first (sorted downwards)
  saw    e = D (((37 i) mod 64) / 63 - 1/2)    the same magnitudes in every batch of 64 (mant of i mod 64): from the second batch
                                               on the batch maximum equals the scale exactly (the reference's else branch)
  ties   e = 0, mant = 1                       all magnitudes equal, signs mixed
  wild   e = D (h(i) - 1/2)                    maxima at arbitrary places
  late   e = -D/2 + 0.3 h(i), last e = +D/2    the only large element is the last one

and two zero masks: `runs` (elements with (i div 70) even) and `gap` (elements [64, 664)).  All values are finite fp32 normals.

Test infrastructure only: used by test_lsmr_adversarial_patterns.py (oracle alone) and test_gpu_lsmr_adversarial.py (device)."""
import ctypes as C

import numpy as np

import _libs as L
from synth_matrix import mix

PROFILES = ("asc", "desc", "saw", "ties", "wild", "late")
MASKS = ("none", "runs", "gap")
PROBE_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 2305)
PROBE_DECADES = (0.5, 10.0, 30.0, 50.0)
PROBE_SALTS = (0, 1, 2, 3)                      # four draws of every (profile, decades, mask): more than 64 vectors of every length
EMPTY_LENGTHS = (1, 65, 1025)                   # the probe on a matrix without entries (nar = 0)


def profile(name, n, decades, salt=0):
    """n fp32 values of one profile"""
    i = np.arange(n, dtype=np.int64)
    t = i / float(n - 1) if n > 1 else np.zeros(n)
    sign = np.where(mix(i, 7001 + 16 * salt) < 0.5, -1.0, 1.0)
    mant = 1.0 + mix(i, 7002 + 16 * salt)
    h = mix(i, 7003 + 16 * salt)
    D = float(decades)
    if name == "asc":
        e = D * (t - 0.5)
    elif name == "desc":
        e = D * (0.5 - t)
    elif name == "saw":
        e = D * (((37 * i) % 64) / 63.0 - 0.5)
        mant = 1.0 + mix(i % 64, 7002 + 16 * salt)
    elif name == "ties":
        e = np.zeros(n)
        mant = np.ones(n)
    elif name == "wild":
        e = D * (h - 0.5)
    elif name == "late":
        e = -D / 2 + 0.3 * h
        if n:
            e[-1] = D / 2
    else:
        raise ValueError(name)
    mag = (mant * 10.0 ** e).astype(np.float32)
    if name == "asc":
        mag = np.sort(mag)
    elif name == "desc":
        mag = np.sort(mag)[::-1]
    return (sign.astype(np.float32) * mag).astype(np.float32)


def zero_mask(name, n):
    """True where the mask sets an element to zero"""
    i = np.arange(n)
    if name == "none":
        return np.zeros(n, bool)
    if name == "runs":
        return (i // 70) % 2 == 0
    if name == "gap":
        return (i >= 64) & (i < 664)
    raise ValueError(name)


def masked(x, name):
    y = x.copy()
    y[zero_mask(name, x.size)] = 0.0
    return y


def probe_vectors(n):
    """(labels, W (R, n) fp32) of the norm probe at length n: profiles x decades x masks x salts; a mask that zeroes nothing at this
    length, and every all-zero vector, is dropped (`ties` has no decades: listed once)"""
    labels, rows = [], []
    for mk in MASKS:
        if mk != "none" and not zero_mask(mk, n).any():
            continue
        for p in PROFILES:
            for D in (PROBE_DECADES if p != "ties" else PROBE_DECADES[:1]):
                for salt in PROBE_SALTS:
                    w = masked(profile(p, n, D, salt), mk)
                    if not w.any():
                        continue
                    labels.append("%s D=%g %s salt=%d" % (p, D, mk, salt))
                    rows.append(w)
    return labels, np.stack(rows)


def probe_system(w, empty=False):
    """len(w) x 1 with one stored entry (1, 1) of value 0 (or none at all), b = w: A'u = 0 exactly, so the reference leaves before its
    first iteration with itn = 0, istop = 0, x = 0 and normr = dnrm2(w)"""
    nar = 0 if empty else 1
    return dict(m=int(w.size), n=1, nar=nar, iw=np.array([nar] + [1, 1] * nar, np.int32), rw=np.zeros(nar, np.float32),
                b=np.ascontiguousarray(w, np.float32))


def dnrm2_twin(X):
    """lsmrblas.f90:247-277 in NumPy fp32 on every row of X (R, n) at once (the recurrence runs over the elements, the rows are
    independent): returns (norms (R,) fp32, how many elements of each row were a new running maximum)"""
    X = np.ascontiguousarray(X, np.float32)
    R, n = X.shape
    if n < 1:
        return np.zeros(R, np.float32), np.zeros(R, np.int64)
    A = np.abs(X)
    if n == 1:
        return A[:, 0].copy(), (A[:, 0] != 0).astype(np.int64)
    one = np.float32(1.0)
    scale, ssq, count = np.zeros(R, np.float32), np.ones(R, np.float32), np.zeros(R, np.int64)
    with np.errstate(all="ignore"):
        for i in range(n):
            a = A[:, i]
            nz = a != 0
            up = nz & (scale < a)
            dn = nz & ~up
            q = np.where(up, scale / np.where(up, a, one), a / np.where(dn, scale, one)).astype(np.float32)
            qq = q * q
            ssq = np.where(up, one + ssq * qq, np.where(dn, ssq + qq, ssq)).astype(np.float32)
            scale = np.where(up, a, scale)
            count += up
    return (scale * np.sqrt(ssq)).astype(np.float32), count


def oracle_dnrm2(x):
    O = L.oracle()
    O.dso_dnrm2.restype = C.c_float
    O.dso_dnrm2.argtypes = [C.c_int, C.c_void_p]
    x = np.ascontiguousarray(x, np.float32)
    return np.float32(O.dso_dnrm2(int(x.size), L.ptr(x)))


def has_zero_batch(w):
    """a whole batch of 64 consecutive elements from a multiple of 64 (the last one as long as the vector reaches) is zero"""
    return any(not w[k:k + 64].any() for k in range(0, w.size, 64))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- iterating systems ---------------------------------------------------------------------------------------------------------------

SHAPES = ((2, 1), (1, 2), (2, 2), (63, 65), (65, 63), (64, 64), (129, 127), (257, 255), (255, 257), (1025, 130), (130, 1025), (2049, 1023),
          (2305, 300))
B_PROFILES = ("wild", "ties", "asc", "late")
DECADES = ((2.0, 2.0), (6.0, 10.0), (10.0, 20.0))                       # (matrix, right-hand side)
ITNLIM = 40
ARGSETS = (                                                             # (damp, atol, btol, conlim, localSize)
    (0.0, 1e-6, 1e-6, 100.0, 10),
    (0.5, 0.0, 0.0, 0.0, 3),
    (0.0, 0.0, 0.0, 0.0, 0),
    (1e-3, 1e-6, 1e-6, 1e8, 10),
    (0.0, 1e-3, 1e-3, 1e30, 70),
    (0.0, 0.0, 0.0, 0.0, 2),
    (1e-4, 0.0, 0.0, 0.0, 5),
)


def solve_kw(args):
    damp, atol, btol, conlim, local_size = args
    return damp, dict(atol=atol, btol=btol, conlim=conlim, itnlim=ITNLIM, local_size=local_size)


def matrix(m, n, prof, decades, salt=0):
    """m x n COO (1-based, sorted by row then column) without a right-hand side: min(m, n) diagonal entries of profile `prof`; for m > n
    row j >= n holds one entry at column (7 j mod n) + 1, for n > m column j >= m one entry at row (5 j mod m) + 1, those values `wild`
    with half the decades; where m >= 4 the last two rows are left empty"""
    k = min(m, n)
    d = np.arange(k)
    rows, cols, vals = [d], [d], [profile(prof, k, decades, salt)]
    if m > n:
        j = np.arange(n, m)
        rows.append(j); cols.append((7 * j) % n); vals.append(profile("wild", m - n, decades / 2, salt + 5))
    elif n > m:
        j = np.arange(m, n)
        rows.append((5 * j) % m); cols.append(j); vals.append(profile("wild", n - m, decades / 2, salt + 5))
    row, col, val = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    if m >= 4:
        keep = row < m - 2
        row, col, val = row[keep], col[keep], val[keep]
    order = np.lexsort((col, row))
    row, col, val = row[order], col[order], val[order]
    nar = int(val.size)
    return dict(m=m, n=n, nar=nar, iw=np.concatenate([[nar], row + 1, col + 1]).astype(np.int32), rw=np.ascontiguousarray(val, np.float32))


def rhs(m, prof, decades, salt=0):
    """right-hand side of profile `prof`; `wild` carries the `runs` mask where m > 200"""
    b = profile(prof, m, decades, salt + 9)
    return masked(b, "runs") if prof == "wild" and m > 200 else b


def system(shape, mprof, bprof, dec, salt=0):
    S = matrix(shape[0], shape[1], mprof, dec[0], salt)
    S["b"] = rhs(shape[0], bprof, dec[1], salt)
    return S


def all_combos():
    """the full product of the oracle-only conditions: (matrix profile, b profile, decades)"""
    return [(p, bp, dec) for p in PROFILES for bp in B_PROFILES for dec in DECADES]


def six_combos(si, ai):
    """the fixed six of (shape number, argument set number) for the device: every matrix profile once, every right-hand side and every
    decade pair among them, rotated with the shape and the argument set"""
    return [(p, B_PROFILES[(k + si + ai) % 4], DECADES[(k + si + 2 * ai) % 3]) for k, p in enumerate(PROFILES)]


# ---- batches of mixed fate -----------------------------------------------------------------------------------------------------------

BATCH_DECADES = (2.0, 10.0, 20.0)
BATCH_SALTS = (0, 1, 2, 3)
ORDER_SHAPES = ((65, 63), (257, 255), (2049, 1023))
ORDER_ARGSETS = (0, 5)                          # argument sets 1 and 6


def batch_system(shape):
    """the resident system of a mixed-fate batch: `wild` over two decades, right-hand side `ties`"""
    S = matrix(shape[0], shape[1], "wild", 2.0, salt=11)
    S["b"] = profile("ties", shape[0], 0.0, salt=11)
    return S


def batch_members(shape):
    """(labels, row scales (R, m)): the special members first (all in the first lane group), then profiles x decades x salts"""
    m = shape[0]
    labels, rows = ["one"], [np.ones(m, np.float32)]
    labels.append("zero"); rows.append(np.zeros(m, np.float32))                        # beta = 0
    if m >= 4:
        s = np.zeros(m, np.float32); s[m - 2:] = (1.5, -0.75)                          # the empty rows alone: beta > 0, alpha = 0
        labels.append("empty rows"); rows.append(s)
    s = np.zeros(m, np.float32); s[0] = 1.25                                           # one data row: done after one iteration
    labels.append("one row"); rows.append(s)
    labels.append("runs"); rows.append(masked(profile("wild", m, 2.0, salt=21), "runs"))
    for p in PROFILES:
        for D in BATCH_DECADES:
            for salt in BATCH_SALTS:
                labels.append("%s D=%g salt=%d" % (p, D, salt)); rows.append(profile(p, m, D, salt=30 + salt))
    return labels, np.stack(rows)


def fates(itn, istop, labels):
    """which of the four fates the members of the first lane group (the first 64) show"""
    itn, first = np.asarray(itn)[:64], labels[:64]
    out = set()
    if "zero" in first and itn[first.index("zero")] == 0: out.add("beta = 0")
    if "empty rows" in first and itn[first.index("empty rows")] == 0: out.add("alpha = 0")
    if ((itn >= 1) & (itn <= 3)).any(): out.add("early")
    if (itn == ITNLIM).any(): out.add("itnlim")
    return out
