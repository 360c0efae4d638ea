"""The resolution of the period maps on the CPU: dsurftomo_amd/csrc/map_resolution.h through
tests/hostcheck_map_resolution.cpp against maps.map_resolution_twin, the panelled factorisation against the header's left-looking one,
the identities of a resolution matrix and the special cases.

The tolerance is measured, not chosen, the way sections 21 and 22 size theirs: the twin computes every system a second time from
numpy.linalg.pinv of the stacked [A_m; damp I], another algorithm on the same numbers, and the largest difference between its two answers,
every quantity on its own scale, is the size of the rounding error (map_resolution_ref.MEASURED, per size).  The header may differ from
the twin by four times the largest of them.  The figure never comes from the header under test."""
import subprocess

import numpy as np
import pytest

from dsurftomo_amd import maps

import columns_ref
import map_resolution_ref as MR
from map_resolution_ref import DAMP, SYSTEMS, TOL, same_bits

SEED = 11


@pytest.fixture(scope="module")
def h():
    return MR.load()


def twin(S, damp=DAMP, route="normal"):
    return maps.map_resolution_twin(S["nx"], S["ny"], S["nmaps"], S["nblocks"], S, S["ndata"], damp, route)


def n_m(sy):
    return sy[3] * (sy[0] - 2) * (sy[1] - 2)


@pytest.mark.parametrize("sy", SYSTEMS, ids=lambda sy: "nm%d" % n_m(sy))
def test_against_the_twin(h, sy):
    """nused and flag equal; every measure, the leverages, the traces and the R of every map within FACTOR * MEASURED.  The measurement is
    made again and printed, not asserted (it is numpy's pinv that would be tested)."""
    S = MR.system(*sy, SEED)
    a, b = twin(S), twin(S, route="pinv")
    got = MR.host_all(h, S)
    diff = MR.differences(got, a)
    routes = MR.differences(a, b)
    print("n_m %3d: the twin's two routes %.3g (MEASURED %.3g; %s); the header against the twin: %s" %
          (n_m(sy), max(routes.values()), MR.MEASURED[n_m(sy)], " ".join("%s %.2g" % kv for kv in routes.items()), " ".join("%s %.2g" % kv for kv in diff.items())))
    assert np.array_equal(got["nused"], a["nused"]) and np.array_equal(got["flag"], a["flag"])
    assert max(diff.values()) <= TOL, diff
    nmaps = sy[2]
    assert (a["flag"][:2] == 0).all() and (a["nused"][:2] > 64).all() and (a["nused"][:2] % 64 != 0).all()
    assert a["nused"].sum() == S["ndata"] - 3                                      # the three data of weight 0 are not used
    if nmaps == 3:                                                                 # the map without a datum: flag 2 and zeros
        assert got["flag"][2] == 2 and got["nused"][2] == 0
        assert not got["measures"][:, :, 2].any() and not got["trace"][:, 2].any() and not got["R"][2].any()
    assert not got["leverage"][S["datweight"] == 0].any()
    for k in range(2):                                                             # R_qq is the diagonal of the same R, computed once
        assert np.array_equal(got["measures"][0][:, k].ravel(), np.diag(got["R"][k]))
    assert np.isfinite(got["measures"]).all() and max(np.abs(R).max() for R in got["R"]) > 0.1
    if sy[3] == 1:
        assert not got["measures"][6:].any()


@pytest.mark.parametrize("sy", [s for s in SYSTEMS if n_m(s) in (63, 64, 189)], ids=lambda sy: "nm%d" % n_m(sy))
def test_the_panelled_factor_has_the_left_looking_bits(h, sy):
    """the harness's right-looking loop in panels of 64 columns (the device's order of work) against the header's map_factor: L and D
    bit for bit -- one panel short of full, one exactly full, three panels with a short last one"""
    S = MR.system(*sy, SEED)
    for k in range(2):
        flags, L1, d1, L2, d2 = MR.host_factors(h, S, k)
        assert (flags == 0).all()
        assert same_bits(L1, L2) and same_bits(d1, d2)
        assert (d1 > 0).all() and np.abs(np.tril(L1.T, -1)).max() > 0             # (entry (i, p) at [p, i]: L1.T is L)
        N = np.tril(L1.T, -1) + np.eye(d1.size)
        ref = twin_normal(S, k)
        assert np.abs((N * d1) @ N.T - ref).max() <= 1e-12 * np.abs(ref).max()


def twin_normal(S, k, damp=DAMP):
    layer = (S["nx"] - 2) * (S["ny"] - 2)
    A = np.zeros((S["m"], S["n"]))
    A[S["row"] - 1, S["col"] - 1] = S["rw"]
    cols = np.concatenate([np.arange((B * S["nmaps"] + k) * layer, (B * S["nmaps"] + k + 1) * layer) for B in range(S["nblocks"])])
    Am = A[:, cols]
    return Am.T @ Am + float(np.float32(damp)) ** 2 * np.eye(cols.size)


@pytest.mark.parametrize("sy", [SYSTEMS[0], SYSTEMS[4]], ids=lambda sy: "nm%d" % n_m(sy))
def test_identities(h, sy):
    """the trace of R is the sum of the leverages (within the tolerance of the comparison with the twin, on its scale: the largest |R|);
    R_qq and the leverages lie in [0, 1]; var shrinks when damp grows"""
    S = MR.system(*sy, SEED)
    got = MR.host_all(h, S)
    rmax = max(np.abs(R).max() for R in got["R"])
    assert abs(got["trace"].sum() - got["leverage"].sum()) <= TOL * rmax
    for k in range(S["nmaps"]):
        lev = got["leverage"][(np.arange(S["ndata"]) % S["nmaps"]) == k]
        assert abs(got["trace"][:, k].sum() - lev.sum()) <= TOL * rmax
    assert (got["measures"][0] >= 0).all() and (got["measures"][0] <= 1).all()
    assert (got["leverage"] >= 0).all() and (got["leverage"] < 1).all()
    more = MR.host_all(h, S, damp=0.5)
    ok = got["flag"] == 0
    assert (more["measures"][1][:, ok] < got["measures"][1][:, ok]).all() and (got["measures"][1][:, ok] > 0).all()


def test_a_determined_system_resolves_itself(h):
    """both weights 0, damp 0 and more rays than unknowns of full column rank: R = I within the tolerance"""
    sy = SYSTEMS[0]
    S = MR.system(*sy, SEED, weight=0.0, weight_azi=0.0)
    assert np.linalg.matrix_rank(twin_normal(S, 0, 0.0)) == n_m(sy)
    got = MR.host_all(h, S, damp=0.0)
    assert (got["flag"] == 0).all()
    for R in got["R"]:
        assert np.abs(R - np.eye(n_m(sy))).max() <= TOL
    assert np.abs(got["trace"] - n_m(sy)).max() <= TOL * n_m(sy)


def test_special_cases(h):
    """an unknown that no ray touches, with both weights 0 and damp 0, is a zero pivot: flag 1 and zeros for that map (every map here, the
    vertex is avoided in all); a row across two maps and a column stored twice in a row are refused, by the header and by the twin; a matrix
    that is not stored in row order is refused by the header (its sums run in ascending row)"""
    sy = SYSTEMS[0]
    S = MR.system(*sy, SEED, weight=0.0, weight_azi=0.0, avoid=7)
    rc, got = MR.host_resolution(h, S, damp=0.0, r_map=0)
    assert rc == 0 and (got["flag"] == 1).all() and (got["nused"] > 0).all()
    for name in ("measures", "leverage", "trace", "R"):
        assert not got[name].any(), name
    assert (twin(S, 0.0)["flag"] == 1).all()
    rc, got = MR.host_resolution(h, S, damp=DAMP, r_map=0)                         # damped, the same system is fine
    assert rc == 0 and (got["flag"] == 0).all() and got["measures"][0, 0, 0, 7] < 1e-6
    S = MR.system(*sy, SEED)
    layer = 20
    col = S["col"].copy(); col[0] += layer                                         # the first entry of datum 0 into map 1
    rc, got = MR.host_resolution(h, S, col=col)
    assert rc == 1 and (got["measures"] == 9.0).all()
    with pytest.raises(ValueError, match="two maps"):
        twin(dict(S, col=col))
    col = S["col"].copy(); col[1] = col[0]
    rc, got = MR.host_resolution(h, S, col=col)
    assert rc == 2 and (got["measures"] == 9.0).all()
    with pytest.raises(ValueError, match="twice"):
        twin(dict(S, col=col))
    order = np.arange(S["rw"].size)[::-1]                                          # stored backwards: every column's rows descend
    rc, got = MR.host_resolution(h, S, rw=S["rw"][order], row=S["row"][order], col=S["col"][order])
    assert rc == 3 and (got["measures"] == 9.0).all()


def test_the_stand_alone_program_runs(tmp_path):
    """the same file as a program with its own main (what a sanitizer build runs): it checks the special cases itself"""
    exe = str(tmp_path / "hostcheck_map_resolution")
    subprocess.check_call(["g++"] + [f for f in columns_ref.FLAGS if f != "-fPIC"] + ["-DHOSTCHECK_MAP_RESOLUTION_MAIN", "-o", exe, MR.SRC, "-lm"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
