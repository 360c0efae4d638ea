"""The resolution of the laterally coupled depth step (dsurftomo_amd/csrc/column_lateral_resolution.h) on the CPU
through tests/hostcheck_column_lateral_resolution.cpp, no GPU: against the NumPy twin depth.column_lateral_resolution_twin on
tests/test_hostcheck_column_lateral.py's random grids; bit for bit against section 24's own loop with the right-hand side overwritten, and
across the member's place in the batch, the chunking and the polling; the identities between the kinds; and the step the resolution predicts.

The tolerance of the comparison with the twin is measured, not chosen, by the rule of tests/test_hostcheck_columns.py: the twin answers every
case a second time through numpy.linalg.pinv of the stacked system, and the header may differ from the twin by FACTOR times the largest
relative difference between the twin's two answers -- the vectors relative to the largest |R| of the case (MEASURED_R), each measure
relative to its own largest value of the case (MEASURED_M)."""
import subprocess

import numpy as np
import pytest

import column_lateral_ref as LR
import column_lateral_resolution_ref as RR
import column_resolution_ref as CR
import columns_ref as R
from column_lateral_resolution_ref import same_bits
from dsurftomo_amd import depth
from test_hostcheck_column_lateral import DAMP, GRIDS, LATERALS, SIZES, SMOOTH, random_grid

F = np.float32
TOL, MAXIT = 1e-12, 2000
# the largest relative differences between the twin's two answers over GRIDS x SIZES x LATERALS with seed 11, printed by
# test_members_against_the_twin (the vectors: 9 x 8, M = 1, lateral 0.05; the measures: 4 x 2, M = 7, lateral 0.05 -- a lateral moment, where
# the spike hardly leaves its column; at lateral 0.5 and 5 both stay below 1.4e-12), and the factor that covers other seeds
MEASURED_R = 6.9e-12
MEASURED_M = 8.1e-11
FACTOR = 4.0


@pytest.fixture(scope="module")
def h():
    return RR.load()


def depths(M):
    return np.cumsum(2.0 + np.arange(M + 1)).astype(F)


def members(nvx, nvy, M, rows=2):
    """every unknown as kinds 0 and 1 on the small systems; on the others the first corner's top unknown as a spike, then the centre's middle
    unknown as a spike and as a row; then one member of kind 2 and one of kind 3; the models: rows of standard normals"""
    nint = nvx * nvy
    kind, index = RR.every_unknown(nint, M)
    if nint * M > 40:
        centre = (nvy // 2) * nvx + nvx // 2
        kind, index = np.array([0, 0, 1]), np.array([0, centre * M + M // 2, centre * M + M // 2])
    models = np.random.default_rng(7).standard_normal((rows, M, nint))
    return np.r_[kind, 2, 3].astype(np.int32), np.r_[index, 0, rows - 1].astype(np.int32), models


def run(h, grid, lateral, kind, index, models=None, tol=TOL, maxit=MAXIT, poll=16, groups=0, depz=None):
    nx, ny, obs, wt, pv, S, vels = grid
    return RR.host_run(h, nx, ny, obs, wt, pv, S, depths(S.shape[0]) if depz is None else depz, SMOOTH, DAMP, lateral, kind, index, models, tol, maxit, poll, groups)


def twin(grid, lateral, kind, index, models=None, tol=TOL, maxit=MAXIT):
    nx, ny, obs, wt, pv, S, vels = grid
    return depth.column_lateral_resolution_twin(nx, ny, obs, wt, pv, S, depths(S.shape[0]), SMOOTH, DAMP, lateral, kind, index, models, tol, maxit)


def relative(a, b, kind):
    """the largest differences of two results: (the vectors of kinds 0 and 1 relative to the largest |R| of b, those of kinds 2 and 3 to their
    own largest; the measures, each relative to its largest of b)"""
    psf = kind < 2
    d = 0.0
    if psf.any():
        d = np.abs(a["full"][psf] - b["full"][psf]).max() / np.abs(b["full"][psf]).max()
    for s in np.flatnonzero(~psf):
        d = max(d, np.abs(a["full"][s] - b["full"][s]).max() / np.abs(b["full"][s]).max())
    top = np.abs(b["measures"]).max(axis=0)
    m = (np.abs(a["measures"] - b["measures"]).max(axis=0)[top > 0] / top[top > 0]).max() if (top > 0).any() else 0.0
    return float(d), float(m)


@pytest.mark.parametrize("nvx,nvy", GRIDS)
def test_members_against_the_twin(h, nvx, nvy):
    """all four kinds: itn, istop, nused and flag equal; the vectors and the measures within FACTOR * MEASURED.  The measurement is made again
    and printed, not asserted (it is numpy's pinv that would be tested).  On 9 x 8 with M = 7 at lateral 5 the spikes at the corner and at
    the centre stop at different iterations, in the header as in the twin."""
    worst = [0.0, 0.0]
    for M, K in SIZES:
        for lateral in LATERALS:
            grid = random_grid(nvx, nvy, M, K, 11)
            kind, index, models = members(nvx, nvy, M)
            want = twin(grid, lateral, kind, index, models)
            dense = dict(full=want["full_dense"], measures=want["measures_dense"])
            rel = relative(want, dense, kind)
            worst = [max(worst[0], rel[0]), max(worst[1], rel[1])]
            got = run(h, grid, lateral, kind, index, models)
            d = relative(got, dense, kind), relative(got, want, kind)
            print("%d x %d M %d K %2d lateral %4.2f: %3d members, itn %3d .. %3d; twin against dense: R %.3g measures %.3g; header against dense %.3g %.3g, against the twin %.3g %.3g"
                  % (nvx, nvy, M, K, lateral, len(kind), got["itn"].min(), got["itn"].max(), rel[0], rel[1], d[0][0], d[0][1], d[1][0], d[1][1]))
            assert np.array_equal(got["itn"], want["itn"]) and np.array_equal(got["istop"], want["istop"]) and (got["istop"] == 1).all()
            assert np.array_equal(got["nused"], want["nused"]) and np.array_equal(got["flag"], want["flag"]) and not got["flag"].any()
            assert d[1][0] <= FACTOR * MEASURED_R and d[1][1] <= FACTOR * MEASURED_M
            assert np.isfinite(got["full"]).all() and np.isfinite(got["measures"]).all() and not got["measures"][kind >= 2].any()
            if (nvx, nvy, M, lateral) == (9, 8, 7, 5.0):
                assert got["itn"][0] != got["itn"][1] and got["itn"].max() < MAXIT          # the corner's spike and the centre's stop apart
            if (nvx, nvy) == (1, 1):
                assert not got["itn"].any()
            else:
                assert got["itn"][kind == 1].min() >= 2
    print("largest twin-against-dense difference: R %.3g (MEASURED_R = %.3g), measures %.3g (MEASURED_M = %.3g)" % (worst[0], MEASURED_R, worst[1], MEASURED_M))


def test_a_member_is_section_24s_loop_with_its_right_hand_side(h):
    """x, itn, istop, rz0 and rz of a member are, bit for bit, what column_lateral.h's own loop gives with b overwritten by the member's f on
    a model without lateral differences: a given f (kind 3), and the spike's f = H e_l by the twin's chain (kind 0)"""
    for (nvx, nvy), (M, K), lateral in (((3, 3), (2, 3), 0.5), ((9, 8), (7, 12), 5.0), ((4, 2), (7, 12), 0.05), ((3, 3), (7, 12), 0.0)):
        grid = random_grid(nvx, nvy, M, K, 19)
        nx, ny, obs, wt, pv, S, vels = grid
        nint = nvx * nvy
        models = np.random.default_rng(3).standard_normal((1, M, nint))
        spike = (nint // 2) * M + M // 2
        c = (1 + (nint // 2) // nvx) * nx + 1 + (nint // 2) % nvx
        used, rho, _, G = depth._twin_data(obs[:, c], wt[:, c], pv[:, c], S[:, :, c].T)
        f0 = np.zeros((M, nint)); f0[:, nint // 2] = depth._twin_normal(G, used, rho, 0.0, 0.0)[0][:, M // 2]
        got = run(h, grid, lateral, np.array([3, 0], np.int32), np.array([0, spike], np.int32), models)
        for s, f in enumerate((models[0], f0)):
            a = RR.host_anchor(h, nx, ny, obs, wt, pv, S, SMOOTH, DAMP, lateral, f, TOL, MAXIT)
            assert same_bits(a["x"], got["full"][s]) and (a["itn"], a["istop"]) == (got["itn"][s], got["istop"][s]) == (a["itn"], 1)
            assert same_bits(np.array([a["rz0"], a["rz"]]), np.array([got["rz0"][s], got["rz"][s]]))
            assert np.abs(a["x"]).max() > 0 and (a["itn"] >= 2) == (lateral > 0)


def test_a_members_bits_are_its_own(h):
    """9 x 8, M = 2, lateral 5, every unknown as both kinds (288 members, five lane groups, the last partial) and a model: the members stop at
    different iterations, and the bits of each do not depend on the chunk size (one group against all), on how often the done flags are
    looked at (every iteration, every 16th, never), on the member's place in the batch and its neighbours there, or on the others at all"""
    grid = random_grid(9, 8, 2, 3, 41)
    kind, index = RR.every_unknown(72, 2)
    models = np.random.default_rng(5).standard_normal((1, 2, 72))
    kind = np.r_[kind, 2].astype(np.int32); index = np.r_[index, 0].astype(np.int32)
    base = run(h, grid, 5.0, kind, index, models, tol=1e-8, maxit=500)
    names = ("measures", "full", "itn", "istop", "rz0", "rz")
    assert len(np.unique(base["itn"])) >= 2 and (base["istop"] == 1).all() and base["itn"].max() < 484
    print("itn %d .. %d, %d iterations started" % (base["itn"].min(), base["itn"].max(), base["started"]))
    assert base["started"] == -(-base["itn"].max() // 16) * 16
    for poll, groups in ((16, 1), (1, 0), (0, 0), (1, 1)):
        other = run(h, grid, 5.0, kind, index, models, tol=1e-8, maxit=500, poll=poll, groups=groups)
        for name in names:
            assert same_bits(other[name], base[name]), (poll, groups, name)
        if poll == 0:
            assert other["started"] == 500
        if (poll, groups) == (1, 1):
            assert other["started"] == sum(int(base["itn"][g:g + 64].max()) for g in range(0, len(kind), 64))
    order = np.random.default_rng(9).permutation(len(kind))
    other = run(h, grid, 5.0, kind[order], index[order], models, tol=1e-8, maxit=500)
    for name in names:
        assert same_bits(other[name], base[name][order]), name
    for s in (0, 145, 288):
        alone = run(h, grid, 5.0, kind[s:s + 1], index[s:s + 1], models, tol=1e-8, maxit=500)
        for name in names:
            assert same_bits(alone[name][0], base[name][s]), (s, name)
    short = run(h, grid, 5.0, kind, index, models, tol=1e-8, maxit=int(base["itn"].min()))
    assert set(short["istop"].tolist()) == {1, 2} and (short["itn"] <= base["itn"].min()).all()
    assert same_bits(short["full"][short["istop"] == 1], base["full"][short["istop"] == 1])


def test_the_kinds_agree_and_the_measures_are_bounded(h):
    """R_jj of the spike (kind 0) and of the row (kind 1) of one unknown agree to the measured tolerance; var >= 0, 0 <= own <= m1"""
    for (nvx, nvy), lateral in (((3, 3), 0.5), ((4, 2), 5.0), ((9, 8), 0.05)):
        grid = random_grid(nvx, nvy, 2, 3, 29)
        kind, index = RR.every_unknown(nvx * nvy, 2)
        got = run(h, grid, lateral, kind, index)
        m = got["measures"]
        scale = np.abs(got["full"]).max()
        assert (np.abs(m[0::2, 0] - m[1::2, 0]) <= FACTOR * MEASURED_R * scale).all() and (m[:, 0] > 0).all()
        assert (m[:, 6] >= 0).all() and (m[1::2, 6] > 0).all() and not m[0::2, 6].any()
        assert (m[:, 5] >= 0).all() and (m[:, 5] <= m[:, 1]).all() and (m[:, 1:5] >= 0).all()


def test_a_column_without_data_and_a_flagged_column(h):
    """3 x 3, lateral 0.5.  The centre column without a used datum (its kernels NaN) takes part: a spike there has f = 0, x = 0 and itn 0,
    while its row of the averaging kernel is not zero -- it is carried by its neighbours (the largest entry is printed); the twin agrees.  A
    column whose factorisation fails (flag 1): its members give zeros, and nobody else's vector enters it."""
    grid = random_grid(3, 3, 7, 12, 5)
    nx, ny, obs, wt, pv, S, vels = grid
    centre = 2 * nx + 2
    wt[:, centre] = 0.0; S[:, :, centre] = np.nan
    kind = np.array([0, 1, 0, 1], np.int32); index = np.array([4 * 7 + 3, 4 * 7 + 3, 0, 0], np.int32)
    got, want = run(h, grid, 0.5, kind, index), twin(grid, 0.5, kind, index)
    assert got["flag"][centre] == 0 and got["nused"][centre] == 0 and np.array_equal(got["itn"], want["itn"])
    assert not got["full"][0].any() and not got["measures"][0].any() and (got["itn"][0], got["istop"][0], got["rz0"][0]) == (0, 1, 0.0)
    row = got["full"][1]
    print("the row of a carried unknown: largest entry %.3f, in its own column %.3g" % (np.abs(row).max(), np.abs(row[:, 4]).max()))
    assert np.abs(row).max() > 0.01 and not row[:, 4].any() and got["itn"][1] >= 2 and got["measures"][1, 0] == 0.0 and got["measures"][1, 5] == 0.0
    assert np.abs(got["full"] - want["full_dense"]).max() <= 2 * FACTOR * MEASURED_R * np.abs(want["full_dense"]).max()
    assert np.abs(got["full"][2][:, 4]).max() > 0                               # a neighbour's spike reaches the column without data
    grid = random_grid(3, 3, 4, 6, 9, unused=False)
    grid[5][2, 1, centre] = np.nan
    kind = np.array([0, 1, 0, 1, 2], np.int32); index = np.array([4 * 4 + 1, 4 * 4 + 1, 0, 0, 0], np.int32)
    models = np.ones((1, 4, 9))
    got = run(h, grid, 0.5, kind, index, models)
    assert got["flag"][centre] == 1 and got["flag"].sum() == 1 and not got["full"][:2].any() and not got["measures"][:2].any() and not got["itn"][:2].any()
    assert not got["full"][:, :, 4].any() and np.abs(got["full"][2:]).min(axis=(1, 2)).max() == 0 and (np.abs(got["full"][2:]).max(axis=(1, 2)) > 0).all()
    assert np.isfinite(got["full"]).all() and np.isfinite(got["measures"]).all() and (got["istop"] == 1).all()


@pytest.mark.parametrize("M,K", SIZES)
def test_lateral_zero_is_the_uncoupled_resolution(h, M, K):
    """lateral = 0: no iteration, u is zero outside its column, and the spike's vector is column j of column_resolution.h's full R to the
    measured tolerance (another chain: T^T G there, N^-1 (H e_j) here), R_jj, m1 and the depth moment with it; mx = my = 0 and own = m1"""
    grid = random_grid(3, 3, M, K, 23)
    nx, ny, obs, wt, pv, S, vels = grid
    kind, index = RR.every_unknown(9, M)
    got = run(h, grid, 0.0, kind, index)
    want = CR.host_resolution(CR.load(), obs, wt, pv, S, depths(M), SMOOTH, DAMP, R.interior(nx, ny))
    assert not got["itn"].any() and (got["istop"] == 1).all() and got["started"] == 0
    cols = [j * nx + i for j in range(1, ny - 1) for i in range(1, nx - 1)]
    tol = FACTOR * MEASURED_R * np.abs(want["R"]).max()
    bits = 0
    for s in range(len(kind)):
        b, l = divmod(int(index[s]), M)
        outside = np.delete(got["full"][s], b, axis=1)
        assert not outside.any() and got["measures"][s, 3] == 0.0 and got["measures"][s, 4] == 0.0 and got["measures"][s, 5] == got["measures"][s, 1]
        if kind[s] == 0:
            assert (np.abs(got["full"][s][:, b] - want["R"][:, l, cols[b]]) <= tol).all()
            bits += same_bits(got["full"][s][:, b], want["R"][:, l, cols[b]])
            for q, name in ((0, 0), (1, 1), (2, 2)):
                ref = want["measures"][name, l, cols[b]]
                assert abs(got["measures"][s, q] - ref) <= FACTOR * MEASURED_M * np.abs(want["measures"][name]).max()
        else:
            assert abs(got["measures"][s, 6] - want["measures"][3, l, cols[b]]) <= FACTOR * MEASURED_M * want["measures"][3].max()
    print("M %d: %d of %d spikes equal column_resolution's bits" % (M, bits, 9 * M))


def test_the_coupling_spreads_a_spike_sideways(h):
    """9 x 8, M = 7: the centre spike's lateral second moment (mx + my) / m1 is larger at lateral 5 than at 0.05, its own column's share
    own / m1 smaller"""
    grid = random_grid(9, 8, 7, 12, 11)
    kind = np.zeros(1, np.int32); index = np.array([(4 * 9 + 4) * 7 + 3], np.int32)
    weak, strong = (run(h, grid, lat, kind, index, tol=1e-8, maxit=500)["measures"][0] for lat in (0.05, 5.0))
    spread = lambda m: (m[3] + m[4]) / m[1]
    print("lateral 0.05: length %.3f cells, own share %.4f; lateral 5: length %.3f cells, own share %.4f" %
          (np.sqrt(spread(weak)), weak[5] / weak[1], np.sqrt(spread(strong)), strong[5] / strong[1]))
    assert spread(strong) > spread(weak) and strong[5] / strong[1] < weak[5] / weak[1]
    assert np.sqrt(spread(strong)) > 1.0 and np.sqrt(spread(weak)) < 0.2 and weak[5] / weak[1] > 0.95 and strong[5] / strong[1] < 0.5


def test_the_resolution_predicts_the_step(h):
    """A model without lateral differences, a perturbation m, obs = fl32(pv + S m): the unclipped step of column_lateral.h is the recovery of
    m (the member of kind 2) plus what the rounding of obs to fp32 adds, the twin's A^-1 G^T e -- to the measured tolerance"""
    hl = LR.load()
    for (nvx, nvy), (M, K), lateral in (((3, 3), (7, 12), 0.5), ((9, 8), (2, 3), 5.0), ((4, 2), (7, 12), 0.05)):
        grid = random_grid(nvx, nvy, M, K, 37)
        nx, ny, obs, wt, pv, S, vels = grid
        nint, inner = nvx * nvy, R.interior(nx, ny) == 1
        flat = np.repeat(vels[:, :1], nx * ny, axis=1)
        m = 0.05 * np.random.default_rng(2).standard_normal((1, M, nint))
        Sm = np.zeros((K, nx * ny))
        Sm[:, inner] = np.einsum("lkc,lc->kc", np.nan_to_num(S[:, :, inner]), m[0])
        obs = (pv + Sm).astype(F)
        step = LR.host_step(hl, nx, ny, obs, wt, pv, S, flat, SMOOTH, DAMP, lateral, 10.0, 0.0, 10.0, TOL, MAXIT)
        kind = np.array([2], np.int32); index = np.zeros(1, np.int32)
        got = run(h, (nx, ny, obs, wt, pv, S, flat), lateral, kind, index, m)
        tw = twin((nx, ny, obs, wt, pv, S, flat), lateral, kind, index, m)
        e = wt.astype(np.float64) * (obs.astype(np.float64) - (pv + Sm))
        predicted = got["full"][0] + tw["data_response"](e)
        scale = np.abs(step["delta"]).max()
        d = np.abs(step["delta"][:, inner] - predicted).max() / scale
        print("%d x %d M %d lateral %4.2f: the step against the recovery plus the rounding's part %.3g (the rounding's part alone %.3g)" %
              (nvx, nvy, M, lateral, d, np.abs(tw["data_response"](e)).max() / scale))
        assert step["istop"] == 1 and got["istop"][0] == 1 and d <= 2 * FACTOR * MEASURED_R and scale > 1e-3


def test_sizes(h):
    assert h.hlres_group_bytes(5, 5, 7) == 64 * ((7 * 9 * 7 + 9 + 5 * 9 + 8) * 8 + 6 * 4) and h.hlres_work_doubles(63) == 2 * 2016 + 63 + 2 * 63 * 64


def test_the_stand_alone_program_runs(tmp_path):
    """the same file as a program with its own main (what a sanitizer build runs): it checks the special cases itself"""
    exe = str(tmp_path / "hostcheck_column_lateral_resolution")
    subprocess.check_call(["g++"] + [f for f in R.FLAGS if f != "-fPIC"] + ["-DHOSTCHECK_COLUMN_LATERAL_RESOLUTION_MAIN", "-o", exe, RR.SRC, "-lm"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
