"""The depth resolution of the radial step of one column (dsurftomo_amd/csrc/column_radial_resolution.h) on the CPU
through tests/hostcheck_column_radial_resolution.cpp, against the NumPy twin depth.column_radial_resolution_twin: random well-posed columns
of the sizes the kernel meets (one depth, two, a usual column, the stage's limits), both wave types present, some data unused with NaN
kernels; the solve against the step's column_solve on 2M unknowns bit for bit; the identities of exact arithmetic; the leakage against
aniso; the radial step the resolution predicts; aniso = 0 against column_resolution.h on each model; the special cases.

The tolerance is measured, not chosen, the way section 22's is: the twin computes every case a second time from numpy.linalg.pinv of the
stacked [G^; smooth L (+) smooth L; damp I; aniso (-I | I)], another algorithm on the same numbers, and the largest difference between its
two R, relative to the largest |R| of the case, over seeds 11-13, is the size of the rounding error (MEASURED, per size).  The header may
differ from the twin by four times the largest of them -- R, R_jj, R_cross, the leverages and the traces relative to the largest |R|; m1,
m2, var, cov and vard, which carry other units, relative to their own largest value.  The figure never comes from the header under test."""
import subprocess

import numpy as np
import pytest

from dsurftomo_amd import depth

import column_radial_ref
import column_radial_resolution_ref as RR
import column_resolution_ref as CR
import columns_ref
from column_radial_resolution_ref import ANISO, DAMP, SEEDS, SIZES, SMOOTH, host_one, random_column, same_bits

F = np.float32
SEED = SEEDS[0]
MEASURED, FACTOR, TOL = RR.MEASURED, RR.FACTOR, RR.TOL        # measured on the twin alone: column_radial_resolution_ref.py


@pytest.fixture(scope="module")
def h():
    return RR.load()


def one(h, col, smooth=SMOOTH, damp=DAMP, aniso=ANISO, **kw):
    love, obs, wt, pv, S, depz, vsv, vsh = col
    return host_one(h, love, obs, wt, pv, S, depz, vsv, vsh, smooth, damp, aniso, **kw)


def used_of(col):
    love, obs, wt, pv = col[:4]
    return (wt > 0) & (obs > 0) & (pv > 0)


def leak_share(measures):
    """m1_cross / (m1_own + m1_cross) per unknown, 0 where the denominator is 0"""
    return depth.leak_share(measures[1], measures[3])


def test_against_the_twin(h):
    """nused and flag equal; measures, pair, leverage, traces and the full R within FACTOR * MEASURED.  The measurement is made again over
    the seeds and printed, not asserted (it is numpy's pinv that would be tested)."""
    for M, K, unused in SIZES:
        for seed in SEEDS:
            col = random_column(M, K, seed, unused)
            love, obs, wt, pv, S, depz = col[:6]
            twin = depth.column_radial_resolution_twin(obs, wt, pv, S, love, depz, SMOOTH, DAMP, ANISO)
            rmax = np.abs(twin["other"]["R"]).max()
            rel = np.abs(twin["R"] - twin["other"]["R"]).max() / rmax
            got = one(h, col)
            diff = RR.differences(got, twin, rmax)
            print("M %2d K %2d seed %d: ldlt against pinv %.3g (MEASURED %.3g; all figures: %s); header against the twin: %s" %
                  (M, K, seed, rel, MEASURED[(M, K)], " ".join("%s %.2g" % kv for kv in RR.differences(twin, twin["other"], rmax).items()),
                   " ".join("%s %.2g" % kv for kv in diff.items())))
            used = used_of(col)
            assert got["nused"].tolist() == twin["nused"] == [int((used & ~love).sum()), int((used & love).sum())] and got["flag"] == twin["flag"] == 0
            assert sum(twin["nused"]) == K - unused and min(twin["nused"]) >= 1
            assert max(diff.values()) <= TOL, diff
            assert np.abs(got["T"] - twin["T"]).max() <= TOL * np.abs(twin["T"]).max()
            assert np.array_equal(got["measures"][0], np.diag(got["R"]))              # R_jj and R_cross are entries of the same R, computed once
            assert np.array_equal(got["measures"][4], np.array([got["R"][(j + M) % (2 * M), j] for j in range(2 * M)]))
            assert rmax > 0.01 and np.isfinite(got["R"]).all()                               # (the case is not degenerate)


def test_solve_matches_column_solve(h):
    """row k of T is column_system.h's column_solve on 2M unknowns applied to row k of the expanded G, bit for bit; rows of unused data are 0.0"""
    for M, K, unused in SIZES:
        col = random_column(M, K, SEED, unused)
        love, obs, wt, pv, S, depz, vsv, vsh = col
        got = one(h, col)
        flag, T = RR.rows_by_column_solve(h, love, obs, wt, pv, S, vsv[:M], vsh[:M], SMOOTH, DAMP, ANISO)
        assert flag == 0 and same_bits(got["T"], T)
        used = used_of(col)
        assert not got["T"][~used].any() and np.abs(got["T"][used]).min(axis=1).max() > 0


def test_identities(h):
    """what holds in exact arithmetic, to the tolerance of the comparison: the sum of the leverages is the sum of the two traces, 0 <= h_k < 1,
    var >= 0, vard >= 0, |cov| <= sqrt(var_v var_h), vard = var_v + var_h - 2 cov, and more damping resolves less"""
    for M, K, unused in SIZES:
        col = random_column(M, K, SEED, unused)
        got = one(h, col)
        rmax = np.abs(got["R"]).max()
        used = used_of(col)
        assert abs(got["leverage"].sum() - (got["trace"][0] + got["trace"][1])) <= TOL * rmax
        assert not got["leverage"][~used].any()
        assert (got["leverage"][used] >= -TOL * rmax).all() and (got["leverage"] < 1.0).all()
        m = got["measures"]
        assert (m[5] >= 0.0).all() and (m[1] >= 0.0).all() and (m[2] >= 0.0).all() and (m[3] >= 0.0).all()
        cov, vard = got["pair"]
        var_v, var_h = m[5][:M], m[5][M:]
        vmax = m[5].max()
        assert (vard >= 0.0).all() and (np.abs(cov) <= np.sqrt(var_v * var_h) + TOL * vmax).all()
        assert np.abs(vard - (var_v + var_h - 2.0 * cov)).max() <= TOL * max(vmax, vard.max())
        lo = one(h, col, damp=0.05)
        hi = one(h, col, damp=0.5)
        assert hi["trace"].sum() < lo["trace"].sum() <= min(2 * M, K - unused) + TOL * rmax
        print("M %2d K %2d: traces %.6f + %.6f at damp 0.05, %.6f + %.6f at 0.5; R_jj in [%.3g, %.3g]" %
              (M, K, lo["trace"][0], lo["trace"][1], hi["trace"][0], hi["trace"][1], m[0].min(), m[0].max()))


def test_leak_share_is_zero_at_aniso_zero_and_grows_with_aniso(h):
    """a column with ten Rayleigh data and two Love data: without the tie nothing of a spike in one model reaches the other (m1_cross, R_cross
    and cov are 0.0 exactly); with it the Vsh block, which its own data hardly hold, takes its answer from Vsv -- the mean leak share of
    the Vsh block's spikes grows with aniso"""
    M, K = 7, 12
    love = np.zeros(K, bool); love[[3, 8]] = True
    col = random_column(M, K, SEED, 0, love)
    shares = []
    for aniso in (0.0, 0.05, 0.2, 1.0):
        got = one(h, col, aniso=aniso)
        assert got["flag"] == 0 and got["nused"].tolist() == [10, 2]
        shares.append(leak_share(got["measures"]))
        if aniso == 0.0:
            assert not got["measures"][3].any() and not got["measures"][4].any() and not got["pair"][0].any() and not shares[0].any()
            assert not got["R"][:M, M:].any() and not got["R"][M:, :M].any()
    mean_h = [float(s[M:].mean()) for s in shares]
    print("mean leak share of the Vsh block at aniso 0, 0.05, 0.2, 1: %s; of the Vsv block: %s" % (" ".join("%.4f" % v for v in mean_h), " ".join("%.4f" % float(s[:M].mean()) for s in shares)))
    assert all(b > a for a, b in zip(mean_h, mean_h[1:])) and mean_h[0] == 0.0
    assert all((s >= 0.0).all() and (s < 1.0).all() for s in shares)


def test_resolution_predicts_the_step(h):
    """equal starting models (the tie's right-hand side is zero) and obs = fl32(pv + S^ m) for a random m (2M): radial_step's unclipped delta
    is R m + T^T e with e_k = a_k (obs_k - pv_k - (S^ m)_k), the rounding of the observations to fp32, formed in fp64.  Within the tolerance
    of the comparison, relative to the larger of max |delta| and max |R| max |m| (section 22's test of the same kind)."""
    hr = column_radial_ref.load()
    for M, K, unused in SIZES:
        col = random_column(M, K, SEED, unused)
        love, obs, wt, pv, S, depz, vsv, _ = col
        used = used_of(col)
        rng = np.random.default_rng(100 + M)
        m = 0.2 * (rng.random(2 * M) - 0.5)
        Sm = np.zeros(K)
        for k in np.flatnonzero(used):
            Sm[k] = S[k] @ (m[M:] if love[k] else m[:M])
        obs2 = np.where(obs > 0, (pv + Sm).astype(F), obs).astype(F)              # (an unused datum stays unused for the same reason)
        col2 = (love, obs2, wt, pv, S, depz, vsv, vsv)
        got = one(h, col2)
        Sv, Sh = RR.split(S, love)
        start = np.asarray(vsv, F)[:, None]
        step = column_radial_ref.host_step(hr, love, obs2[:, None], wt[:, None], pv[:, None], Sv, Sh, start, start, SMOOTH, DAMP, ANISO, 1e6, -1e6, 1e6)
        assert step["flag"][0] == 0 and step["nused"][:, 0].tolist() == got["nused"].tolist()
        e = np.zeros(K)
        e[used] = wt[used].astype(np.float64) * (obs2[used].astype(np.float64) - pv[used] - Sm[used])
        want = got["R"] @ m + got["T"].T @ e
        delta = step["delta"][:, 0]
        scale = max(np.abs(delta).max(), np.abs(got["R"]).max() * np.abs(m).max())
        print("M %2d K %2d: max |delta - (R m + T^T e)| / scale = %.3g (max |delta| %.3g, max |T^T e| %.3g)" %
              (M, K, np.abs(delta - want).max() / scale, np.abs(delta).max(), np.abs(got["T"].T @ e).max()))
        assert np.abs(delta - want).max() <= TOL * scale
        assert np.abs(delta).max() > 1e-3


def test_aniso_zero_is_column_resolution_on_each_block(h):
    """aniso = 0: R_jj, m1_own, m2_own and var of the Vsv block and the Rayleigh leverages have the bits of column_resolution.h on the Vsv
    model with the Love weights zeroed, those of the Vsh block and the Love leverages the bits of column_resolution.h on the Vsh model with
    the Rayleigh weights zeroed; the own blocks of R too; m1_cross, R_cross and cov are zeros; vard = var_v + var_h to the tolerance"""
    hc = CR.load()
    for M, K, unused in SIZES:
        col = random_column(M, K, SEED, unused)
        love, obs, wt, pv, S, depz = col[:6]
        got = one(h, col, aniso=0.0)
        assert got["flag"] == 0
        Sv, Sh = RR.split(S, love)
        for q, (mine, Sq) in enumerate(((~love, Sv), (love, Sh))):
            w = np.where(mine, wt, F(0.0))
            want = CR.host_resolution(hc, obs[:, None], w[:, None], pv[:, None], Sq, depz, SMOOTH, DAMP)
            assert want["flag"][0] == 0 and want["nused"][0] == got["nused"][q] >= 1
            blk = slice(q * M, (q + 1) * M)
            for mine_q, theirs in ((0, 0), (1, 1), (2, 2), (5, 3)):
                assert same_bits(got["measures"][mine_q][blk], want["measures"][theirs][:, 0]), (M, K, q, mine_q)
            assert same_bits(got["leverage"][mine], want["leverage"][mine, 0]) and same_bits(got["R"][blk, blk], want["R"][:, :, 0])
            assert same_bits(got["trace"][q], want["trace"][0]) and same_bits(got["T"][mine][:, blk], want["T"][mine][:, :, 0])
        assert not got["measures"][3].any() and not got["measures"][4].any() and not got["pair"][0].any()
        var = got["measures"][5]
        assert np.abs(got["pair"][1] - (var[:M] + var[M:])).max() <= TOL * got["pair"][1].max()


def test_one_wave_type_without_data_still_resolves(h):
    """no Love datum used: flag 0, the Vsh block's R_jj are 0 (no datum sees it: its columns of R are 0), its trace is 0.0; what a spike in
    Vsv does to Vsh -- R_cross of the Vsv block -- is not"""
    M, K = 7, 12
    love, obs, wt, pv, S, depz, vsv, vsh = random_column(M, K, 5)
    wt = np.where(love, F(0.0), wt)
    col = (love, obs, wt, pv, np.where(love[:, None], np.nan, S), depz, vsv, vsh)
    got = one(h, col, aniso=0.5, fill=9.0)
    assert got["flag"] == 0 and got["nused"].tolist() == [6, 0]
    assert not got["measures"][0][M:].any() and got["trace"][1] == 0.0 and got["trace"][0] > 0.0 and not got["R"][:, M:].any()
    assert np.abs(got["measures"][4][:M]).max() > 0 and (got["measures"][5][M:] > 0).all() and not got["leverage"][love].any()
    twin = depth.column_radial_resolution_twin(obs, wt, pv, col[4], love, depz, SMOOTH, DAMP, 0.5)
    assert twin["flag"] == 0 and twin["nused"] == [6, 0]
    assert max(RR.differences(got, twin, np.abs(twin["R"]).max()).values()) <= TOL


def test_no_data_is_flag_2_whatever_damp_and_aniso_are(h):
    M, K = 4, 6
    love, obs, wt, pv, S, depz, vsv, vsh = random_column(M, K, 6)
    nan = np.full((K, M), np.nan)
    for damp, aniso in ((0.1, 0.0), (1e3, 0.2), (0.1, 1e3)):
        got = host_one(h, love, obs, np.zeros(K, F), pv, nan, depz, vsv, vsh, SMOOTH, damp, aniso, fill=9.0)
        assert got["flag"] == 2 and not got["nused"].any() and not got["trace"].any()
        assert not got["measures"].any() and not got["pair"].any() and not got["leverage"].any() and not got["R"].any()
        twin = depth.column_radial_resolution_twin(obs, np.zeros(K, F), pv, nan, love, depz, SMOOTH, damp, aniso)
        assert twin["flag"] == 2 and not twin["R"].any() and twin["other"] is None


def test_not_positive_definite_is_flag_1(h):
    """an N made indefinite by hand (second pivot 1 - 4), one with a zero pivot, one with a pivot that is not finite: flag 1 and every
    output 0.0; the twin agrees.  A definite one next to them is resolved."""
    G = np.array([[1.0, 0.5], [0.25, 1.0], [0.5, 0.5]])
    love = np.array([False, True, False])
    depz = np.array([0.0, 2.0, 5.0], F)
    eye = np.eye(4)
    bad = []
    for a, b, v in ((0, 1, 2.0), (0, 1, 1.0)):
        N = eye.copy(); N[a, b] = N[b, a] = v
        bad.append(N)
    N = eye.copy(); N[2, 2] = np.inf; bad.append(N)
    N = eye.copy(); N[0, 0] = np.nan; bad.append(N)
    for N in bad:
        for full in (True, False):
            flag, out = RR.host_finish(h, love, N.tolist(), G, depz, full)
            assert flag == 1 and all(not v.any() for v in out.values())
        twin = depth.column_radial_resolution_twin(np.ones(3, F), None, np.ones(3), G, love, depz, SMOOTH, DAMP, ANISO, n_override=N)
        assert twin["flag"] == 1 and not twin["R"].any() and not twin["measures"].any() and not twin["pair"].any() and not twin["leverage"].any() and not twin["trace"].any()
    Gx = depth._radial_expand(G, love)
    N = Gx.T @ Gx + eye
    flag, out = RR.host_finish(h, love, N.tolist(), G, depz)
    twin = depth.column_radial_resolution_twin(np.ones(3, F), None, np.ones(3), G, love, depz, SMOOTH, DAMP, ANISO, n_override=N)
    assert flag == 0 and twin["flag"] == 0 and np.abs(out["R"] - twin["R"]).max() <= TOL * np.abs(twin["R"]).max()
    assert np.abs(out["R"] - np.linalg.solve(N, Gx.T @ Gx)).max() <= 1e-14


def test_r_null_changes_no_other_bit(h):
    for M, K, unused in SIZES:
        col = random_column(M, K, SEED, unused)
        a = one(h, col)
        b = one(h, col, full=False)
        assert "R" not in b
        for name in ("measures", "pair", "leverage", "trace", "nused", "flag", "T"):
            assert same_bits(np.asarray(a[name]), np.asarray(b[name])), name


def test_a_column_among_others_and_the_mask(h):
    """columns side by side with the engine's strides: each equals the column alone; a column masked out keeps what it held; the work arrays
    at the limits are the 158 712 bytes the kernel asks for"""
    M, K, n = 3, 4, 5
    cols = [random_column(M, K, 20 + c) for c in range(n)]
    love, depz = cols[0][0], cols[0][5]
    obs = np.stack([c[1] for c in cols], axis=1); wt = np.stack([c[2] for c in cols], axis=1); pv = np.stack([c[3] for c in cols], axis=1)
    parts = [RR.split(c[4], love) for c in cols]
    Sv = np.concatenate([p[0] for p in parts], axis=2); Sh = np.concatenate([p[1] for p in parts], axis=2)
    vsv = np.stack([c[6] for c in cols], axis=1); vsh = np.stack([c[7] for c in cols], axis=1)
    only = np.array([1, 0, 1, 1, 0], np.uint8)
    got = RR.host_resolution(h, love, obs, wt, pv, Sv, Sh, depz, vsv, vsh, SMOOTH, DAMP, ANISO, only, fill=9.0)
    for c in range(n):
        if not only[c]:
            assert (got["measures"][:, :, c] == 9.0).all() and (got["R"][:, :, c] == 9.0).all() and (got["trace"][:, c] == 9.0).all() and (got["pair"][:, :, c] == 9.0).all()
            continue
        alone = one(h, cols[c])
        for name in ("R", "measures", "pair", "leverage", "trace"):
            assert same_bits(alone[name], got[name][..., c]), name
    nowt = RR.host_resolution(h, love, obs, None, pv, Sv, Sh, depz, vsv, vsh, SMOOTH, DAMP, ANISO)
    ones = RR.host_resolution(h, love, obs, np.ones_like(wt), pv, Sv, Sh, depz, vsv, vsh, SMOOTH, DAMP, ANISO)
    assert same_bits(nowt["R"], ones["R"]) and same_bits(nowt["leverage"], ones["leverage"])     # no weights: all 1
    assert h.hrr_doubles(63, 60) == 12279 + 7560 and h.hrr_doubles(63, 60) * 8 == 158712 <= 163840


def test_the_starting_models_do_not_enter(h):
    """vsv and vsh enter the step's right-hand side only: the resolution has the same bits whatever they are"""
    col = random_column(7, 12, SEED, 3)
    a = one(h, col)
    b = one(h, col[:6] + (col[6] * F(0.5), col[7] * F(2.0)))
    for name in ("measures", "pair", "leverage", "trace", "R", "T"):
        assert same_bits(a[name], b[name]), name


def test_the_stand_alone_program_runs(tmp_path):
    """the same file as a program with its own main (what a sanitizer build runs): it checks the special cases itself"""
    exe = str(tmp_path / "hostcheck_column_radial_resolution")
    subprocess.check_call(["g++"] + [f for f in columns_ref.FLAGS if f != "-fPIC"] + ["-DHOSTCHECK_COLUMN_RADIAL_RESOLUTION_MAIN", "-o", exe, RR.SRC, "-lm"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
