"""The depth inversion of the maps' 2 psi terms of one column (dsurftomo_amd/csrc/column_azimuthal.h) on the CPU through
tests/hostcheck_column_azimuthal.cpp, against the NumPy twin depth.column_azimuthal_twin: column_resolution_ref.random_column's columns of
the sizes the kernel meets (one unknown, two, a usual column, the stage's limits) with A1, A2 of a few per cent of c0 and of both signs,
some data unused in each of the three ways and by a Love mask, their Z and A NaN; the laws, bit for bit on the header; the special cases.

The tolerance is measured, not chosen, the way sections 21 and 22 do it: the twin computes every case a second time from
numpy.linalg.lstsq (g) and numpy.linalg.pinv (the measures) of the stacked [diag(a) Z; smooth L; damp I], another algorithm on the same
numbers; the largest difference between its two answers over all figures is the size of the rounding error (MEASURED in
column_azimuthal_ref.py, per size).  The header may differ from the twin by four times the largest of them.  The figure never comes from the
header under test.  In fact the twin runs the header's operations in its order and the two agree to the last bit on this compiler."""
import subprocess

import numpy as np
import pytest

from dsurftomo_amd import depth

import column_azimuthal_ref as CA
import column_resolution_ref as CR
import columns_ref
from column_azimuthal_ref import SIZES, azimuthal_column, host_one, same_bits, used_of

F = np.float32
SMOOTH, DAMP = 0.3, 0.1
SEED = 11
MEASURED, FACTOR, TOL = CA.MEASURED, CA.FACTOR, CA.TOL
FIGURES = ("gc", "gs", "chi2", "measures", "leverage")


@pytest.fixture(scope="module")
def h():
    return CA.load()


def one(h, col, smooth=SMOOTH, damp=DAMP, **kw):
    obs, a1, a2, wt, pv, Z, love, depz = col
    return host_one(h, obs, a1, a2, wt, pv, Z, love, depz, smooth, damp, **kw)


def twin_of(col, smooth=SMOOTH, damp=DAMP, **kw):
    obs, a1, a2, wt, pv, Z, love, depz = col
    return depth.column_azimuthal_twin(obs, a1, a2, wt, pv, Z, love, depz, smooth, damp, **kw)


def test_against_the_twin(h):
    """nused and flag equal; gc, gs, chi2, the measures and the leverages within FACTOR * MEASURED.  The measurement is made again and
    printed, not asserted (it is numpy's lstsq that would be tested); whether the header and the twin agree to the last bit is printed."""
    for M, K, unused, nlove in SIZES:
        col = azimuthal_column(M, K, SEED, unused, nlove)
        twin = twin_of(col)
        rmax = np.abs(twin["R"]).max()
        measured = CA.differences(twin, twin["other"], rmax)
        got = one(h, col)
        diff = CA.differences(got, twin, rmax)
        bits = all(same_bits(np.asarray(got[n], np.float64), np.asarray(twin[n], np.float64)) for n in FIGURES)
        print("M %2d K %2d: ldlt against lstsq %.3g (MEASURED %.3g; all figures: %s); header against the twin: %s; same bits: %s" %
              (M, K, max(measured.values()), MEASURED[(M, K)], " ".join("%s %.2g" % kv for kv in measured.items()), " ".join("%s %.2g" % kv for kv in diff.items()), bits))
        want = int(used_of(col[0], col[3], col[4], col[6]).sum())
        assert got["nused"] == twin["nused"] == want and 0 < want <= K - nlove and got["flag"] == twin["flag"] == 0
        assert max(diff.values()) <= TOL, diff
        assert np.abs(got["T"] - twin["T"]).max() <= TOL * np.abs(twin["T"]).max()
        assert rmax > 0.1 and all(np.isfinite(got[n]).all() for n in FIGURES)
        assert max(np.abs(got["gc"]).max(), np.abs(got["gs"]).max()) > 1e-3               # (a few per cent of anisotropy came out)


def test_swap_negate_and_zero(h):
    """swapping A1 and A2 swaps gc and gs; negating A negates g; A2 = 0 gives gs = 0.0 and chi2s = 0 -- bit for bit; the measures do not
    see A; chi2_after <= chi2_before for each component"""
    for M, K, unused, nlove in SIZES:
        obs, a1, a2, wt, pv, Z, love, depz = col = azimuthal_column(M, K, SEED, unused, nlove)
        base = one(h, col)
        swap = one(h, (obs, a2, a1, wt, pv, Z, love, depz))
        assert same_bits(swap["gc"], base["gs"]) and same_bits(swap["gs"], base["gc"]) and same_bits(swap["chi2"], base["chi2"][[1, 0, 3, 2]])
        neg = one(h, (obs, -a1, -a2, wt, pv, Z, love, depz))
        assert same_bits(neg["gc"], -base["gc"]) and same_bits(neg["gs"], -base["gs"]) and same_bits(neg["chi2"], base["chi2"])
        zero = one(h, (obs, a1, np.where(np.isnan(a2), a2, F(0.0)).astype(F), wt, pv, Z, love, depz))
        assert same_bits(zero["gc"], base["gc"]) and same_bits(zero["gs"], np.zeros(M)) and zero["chi2"][1] == 0.0 and zero["chi2"][3] == 0.0
        for other in (swap, neg, zero):
            assert same_bits(other["measures"], base["measures"]) and same_bits(other["leverage"], base["leverage"]) and other["nused"] == base["nused"]
        assert (base["chi2"][2:] <= base["chi2"][:2]).all() and (base["chi2"][:2] > 0).all()


def test_love_and_unused_slots_change_no_bit(h):
    """whatever stands at a Love slot or at an unused datum -- Z, A1, A2, and at a Love slot the weight and c0 too -- no output changes a bit;
    their leverages and rows of T are 0.0"""
    M, K, unused, nlove = SIZES[2]
    obs, a1, a2, wt, pv, Z, love, depz = col = azimuthal_column(M, K, SEED, unused, nlove)
    base = one(h, col)
    dead = ~used_of(obs, wt, pv, love)
    assert dead.sum() >= unused and love.sum() == nlove
    a1b, a2b, Zb, obsb, wtb = a1.copy(), a2.copy(), Z.copy(), obs.copy(), wt.copy()
    a1b[dead] = 7.0; a2b[dead] = -3.0; Zb[dead] = 1e30
    obsb[love] = 9.0; wtb[love] = 5.0
    got = one(h, (obsb, a1b, a2b, wtb, pv, Zb, love, depz))
    for name in FIGURES + ("T", "nused", "flag"):
        assert same_bits(np.asarray(got[name]), np.asarray(base[name])), name
    assert not base["leverage"][dead].any() and not base["T"][dead].any() and (base["leverage"][~dead] > 0).all()


def test_the_operator_is_the_resolutions(h):
    """the measures, the leverages, T, nused and flag are column_resolution.h's on S = Z and the effective weights, bit for bit; and gc is
    sum_k T_kj rhoc_k with that T, the other route through the same linear algebra, within the tolerance of the comparison"""
    hr = CR.load()
    for M, K, unused, nlove in SIZES:
        obs, a1, a2, wt, pv, Z, love, depz = col = azimuthal_column(M, K, SEED, unused, nlove)
        got = one(h, col)
        weff = CA.effective_weights(wt, love, (K,))
        res = CR.host_resolution(hr, obs[:, None], weff[:, None], pv[:, None], np.ascontiguousarray(Z.T)[:, :, None], depz, SMOOTH, DAMP)
        for name in ("measures", "leverage", "T"):
            assert same_bits(got[name], res[name][..., 0]), name
        assert got["nused"] == res["nused"][0] and got["flag"] == res["flag"][0] == 0
        used = used_of(obs, wt, pv, love)
        for g, a in ((got["gc"], a1), (got["gs"], a2)):
            rho = np.where(used, weff.astype(np.float64) * np.where(used, a, F(0.0)).astype(np.float64), 0.0)
            want = res["T"][..., 0].T @ rho
            assert np.abs(g - want).max() <= TOL * np.abs(want).max()


def test_no_data_is_flag_2_whatever_damp_is(h):
    M, K = 4, 5
    obs, a1, a2, wt, pv, Z, love, depz = azimuthal_column(M, K, 6)
    nan = np.full(K, np.nan, F)
    for damp in (0.1, 1e3):
        for w, lv in ((np.zeros(K, F), None), (wt, np.ones(K, bool))):          # no weight anywhere; every slot a Love slot
            got = host_one(h, obs, nan, nan, w, pv, np.full((K, M), np.nan), lv, depz, SMOOTH, damp, fill=9.0)
            assert got["flag"] == 2 and got["nused"] == 0
            assert all(not got[n].any() for n in FIGURES)
            twin = depth.column_azimuthal_twin(obs, nan, nan, w, pv, np.full((K, M), np.nan), lv, depz, SMOOTH, damp)
            assert twin["flag"] == 2 and not twin["gc"].any() and not twin["chi2"].any() and twin["other"] is None


def test_not_positive_definite_is_flag_1(h):
    """an N made indefinite by hand (second pivot 1 - 4), one with a zero pivot, one with a pivot that is not finite: flag 1 and every
    output 0.0; the twin agrees.  A definite one next to them is solved."""
    G = np.array([[1.0, 0.5, 0.0], [0.25, 1.0, 0.5]])
    a1, a2 = np.array([0.05, -0.02], F), np.array([-0.01, 0.04], F)
    depz = np.array([0.0, 2.0, 5.0], F)
    for N in ([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]], [[1.0, 1.0, 0.0], [1.0, 1.0, 0.0], [0.0, 0.0, 1.0]],
              [[1.0, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, 1.0]], [[np.nan, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]):
        flag, out = CA.host_finish(h, N, G, a1, a2, depz)
        assert flag == 1 and all(not v.any() for v in out.values())
        twin = depth.column_azimuthal_twin(np.ones(2, F), a1, a2, None, np.ones(2), G, None, depz, SMOOTH, DAMP, n_override=N)
        assert twin["flag"] == 1 and not twin["gc"].any() and not twin["gs"].any() and not twin["chi2"].any() and not twin["measures"].any()
    N = (G.T @ G + np.eye(3)).tolist()
    flag, out = CA.host_finish(h, N, G, a1, a2, depz)
    twin = depth.column_azimuthal_twin(np.ones(2, F), a1, a2, None, np.ones(2), G, None, depz, SMOOTH, DAMP, n_override=N)
    assert flag == 0 and twin["flag"] == 0
    for q, a in (("gc", a1), ("gs", a2)):
        assert same_bits(out[q], twin[q])
        assert np.abs(out[q] - np.linalg.solve(np.array(N), G.T @ a.astype(np.float64))).max() <= 1e-15


def test_one_unknown_and_group_slots_only(h):
    """M = 1 with several data: g = sum(g_k rho_k) / (sum(g_k^2) + damp^2) in closed form; a column whose only used data are group slots
    (the mask knows wave types, not velocity kinds): the data that stay are solved like any others"""
    obs, a1, a2, wt, pv, Z, love, depz = azimuthal_column(1, 6, 3)
    got = host_one(h, obs, a1, a2, wt, pv, Z, love, depz, SMOOTH, DAMP)
    g = wt.astype(np.float64) * Z[:, 0]
    n = float(F(DAMP)) * float(F(DAMP)) + float(g @ g)
    assert got["flag"] == 0 and got["nused"] == 6
    assert abs(got["gc"][0] - g @ (wt.astype(np.float64) * a1) / n) <= TOL * abs(got["gc"][0]) and abs(got["measures"][0, 0] - g @ g / n) <= TOL
    # K = 12 in the maps' order Rc | Rg | Lc | Lg, three periods each: the Rayleigh phase data carry no weight, the Love slots are masked
    M, K = 7, 12
    obs, a1, a2, wt, pv, Z, _, depz = azimuthal_column(M, K, 4)
    love = np.arange(K) >= 6
    wt = wt.copy(); wt[:3] = 0.0
    Z = Z.copy(); Z[:3] = np.nan; Z[6:] = np.nan
    got = host_one(h, obs, a1, a2, wt, pv, Z, love, depz, SMOOTH, DAMP)
    alone = host_one(h, obs[3:6], a1[3:6], a2[3:6], wt[3:6], pv[3:6], Z[3:6], None, depz, SMOOTH, DAMP)
    assert got["nused"] == alone["nused"] == 3 and got["flag"] == 0
    for name in ("gc", "gs", "chi2", "measures"):
        assert same_bits(got[name], alone[name]), name
    assert same_bits(got["leverage"][3:6], alone["leverage"]) and not got["leverage"][:3].any() and not got["leverage"][6:].any()


def test_a_column_among_others_and_the_mask(h):
    """columns side by side with the engine's strides: each equals the column alone; a column masked out keeps what it held; no weights: all 1"""
    M, K, n = 3, 4, 5
    cols = [azimuthal_column(M, K, 20 + c) for c in range(n)]
    stack = lambda q: np.stack([c[q] for c in cols], axis=1)
    Z = np.stack([c[5].T for c in cols], axis=2); depz = cols[0][7]
    only = np.array([1, 0, 1, 1, 0], np.uint8)
    love = np.array([False, False, False, True])
    got = CA.host_azimuthal(h, stack(0), stack(1), stack(2), stack(3), stack(4), Z, love, depz, SMOOTH, DAMP, only, fill=9.0)
    for c in range(n):
        if not only[c]:
            assert all((got[name][..., c] == 9.0).all() for name in FIGURES)
            continue
        o, a1, a2, w, p, z, _, _ = cols[c]
        alone = host_one(h, o, a1, a2, w, p, z, love, depz, SMOOTH, DAMP)
        assert all(same_bits(alone[name], got[name][..., c]) for name in FIGURES) and alone["nused"] == got["nused"][c] == 3
    nowt = CA.host_azimuthal(h, stack(0), stack(1), stack(2), None, stack(4), Z, love, depz, SMOOTH, DAMP)
    ones = CA.host_azimuthal(h, stack(0), stack(1), stack(2), np.ones_like(stack(3)), stack(4), Z, love, depz, SMOOTH, DAMP)
    assert all(same_bits(nowt[name], ones[name]) for name in FIGURES)
    assert CA.load().hca_doubles(63, 60) == CR.load().hcr_doubles(63, 60) + 2 * 63 + 2 * 60 == 10131          # 81 048 bytes of LDS


def test_azimuthal_factor_has_the_kernels_roundings():
    """Z = svs (double)(0.5f v): the product with 0.5 in fp32, the product with the kernel in fp64, the bottom depth dropped"""
    rng = np.random.default_rng(2)
    nz, K, ncol = 4, 3, 6
    svs = rng.standard_normal((nz, K, ncol))
    vels = (2.0 + 3.0 * rng.random((nz, 2, 3))).astype(F)
    Z = depth.azimuthal_factor(svs, vels)
    assert Z.shape == (nz - 1, K, ncol) and Z.dtype == np.float64
    for l in range(nz - 1):
        for c in range(ncol):
            half = F(0.5) * vels.reshape(nz, ncol)[l, c]
            assert type(half) is F and (Z[l, :, c] == svs[l, :, c] * float(half)).all()


def test_the_stand_alone_program_runs(tmp_path):
    """the same file as a program with its own main (what a sanitizer build runs): it checks the laws and the special cases itself"""
    exe = str(tmp_path / "hostcheck_column_azimuthal")
    subprocess.check_call(["g++"] + [f for f in columns_ref.FLAGS if f != "-fPIC"] + ["-DHOSTCHECK_COLUMN_AZIMUTHAL_MAIN", "-o", exe, CA.SRC, "-lm"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
