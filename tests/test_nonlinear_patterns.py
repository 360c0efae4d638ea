"""Host-side pieces of the nonlinear judgement of trade-off and cross-validation members (dsurftomo_amd/invert.py, io.py): the numpy
restatement of dsa_forward_steps' misfit sums, the combination of the sums into the rows of the two files, the files themselves, the
refusals of the two flags, and the argument checks of dsa_forward_steps / dsa_step_models, which come before any engine exists.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import synth
from dsurftomo_amd import invert
from dsurftomo_amd import io as taipei

ERR_ARGUMENT = -2


@pytest.fixture(scope="module")
def lib():
    from dsurftomo_amd import build
    return C.CDLL(build.build())


# ---- nonlinear_measures ---------------------------------------------------------------------------------------------------------

def loop_measures(obst, dsyn, w, group, ngroups):
    """the definition, datum by datum: float32 residual and weighted residual, squares and sums in Python floats (fp64), ascending datum"""
    f = np.float32
    out = np.zeros((len(dsyn), ngroups, 2))
    for k, row in enumerate(dsyn):
        for i in range(len(obst)):
            r = f(f(obst[i]) - f(row[i]))
            wr = r if w is None else f(f(w[i]) * r)
            g = 0 if group is None else int(group[i])
            out[k, g, 0] += float(wr) * float(wr)
            out[k, g, 1] += float(r) * float(r)
    return out


def close(got, want, counts):
    """each sum within relative (N + 4) 2^-52 of the other: two fp64 summation orders of N non-negative terms"""
    for g, n in enumerate(counts):
        tol = (n + 4) * 2.0 ** -52
        assert (np.abs(got[:, g] - want[:, g]) <= tol * want[:, g]).all(), (g, got[:, g], want[:, g])


def test_nonlinear_measures_against_the_loop():
    r = np.random.default_rng(11)
    nd, K = 57, 3
    obst = (20.0 + 10.0 * r.random(nd)).astype(np.float32)
    dsyn = (obst[None, :] * (1.0 + 0.05 * (r.random((K, nd)) - 0.5))).astype(np.float32)
    w = np.where(r.random(nd) < 0.2, 0.0, r.random(nd) + 0.5).astype(np.float32)
    group = (np.arange(nd) % 3).astype(np.int32)                     # ngroups 4: group 3 is empty
    got = invert.nonlinear_measures(obst, dsyn, w, group, 4)
    assert got.shape == (K, 4, 2) and got.dtype == np.float64
    close(got, loop_measures(obst, dsyn, w, group, 4), [19, 19, 19, 0])
    assert (got[:, 3] == 0).all() and not np.signbit(got[:, 3]).any()
    assert (got[:, :3] > 0).all()
    # one group; no weights: both sums are the plain one
    one = invert.nonlinear_measures(obst, dsyn, w)
    assert one.shape == (K, 1, 2)
    close(one, loop_measures(obst, dsyn, w, None, 1), [nd])
    plain = invert.nonlinear_measures(obst, dsyn, None, group, 4)
    close(plain, loop_measures(obst, dsyn, None, group, 4), [19, 19, 19, 0])
    assert (plain[..., 0] == plain[..., 1]).all()
    # a single model as a vector; the rms of the line search is the square root of the first sum over ndata
    v = invert.nonlinear_measures(obst, dsyn[1], w)
    assert (v == one[1:2]).all()
    wr, pr = invert.line_search_scores(obst, dsyn, w)
    assert np.allclose(np.sqrt(one[:, 0, 0] / nd), wr, rtol=1e-6) and np.allclose(np.sqrt(one[:, 0, 1] / nd), pr, rtol=1e-6)
    for bad in (dict(group=group, ngroups=2), dict(group=group[:-1], ngroups=4), dict(group=-group, ngroups=4), dict(ngroups=0)):
        with pytest.raises(ValueError):
            invert.nonlinear_measures(obst, dsyn, w, **bad)


# ---- combinations ---------------------------------------------------------------------------------------------------------------

def test_tradeoff_rows_and_selection_on_hand_made_sums():
    w, d = invert.tradeoff_grid([1.0, 2.0, 4.0, 8.0], [0.5, 1.0])          # weight-major: member 2 i + j
    K, nd = 8, 4
    predicted = np.array([4.0, 16.0, 36.0, 64.0, 100.0, 144.0, 196.0, 256.0])
    meas = np.zeros((K, 1, 2))
    meas[:, 0, 0] = [64.0, 400.0, 16.0, 100.0, 36.0, 4.0, 144.0, np.nan]
    meas[:, 0, 1] = 4.0 * meas[:, 0, 0]
    fails = [0, 0, 0, 3, 0, 0, 0, 0]
    rows = invert.tradeoff_nonlinear_rows(w, d, predicted, meas, fails, nd)
    assert [tuple(r) for r in rows] == [taipei.TRADEOFF_NONLINEAR_COLUMNS] * K
    assert [r["weight"] for r in rows] == [1, 1, 2, 2, 4, 4, 8, 8] and [r["damp"] for r in rows] == [0.5, 1.0] * 4
    assert [r["predicted_rms"] for r in rows] == [1, 2, 3, 4, 5, 6, 7, 8]
    assert [r["weighted_rms"] for r in rows[:7]] == [4, 10, 2, 5, 3, 1, 6] and math.isnan(rows[7]["weighted_rms"])
    assert [r["rms"] for r in rows[:7]] == [8, 20, 4, 10, 6, 2, 12]
    assert [r["disp_failures"] for r in rows] == fails
    rough = [8.0, 8.0, 4.0, 4.0, 2.0, 2.0, 1.0, 1.0]
    picks = invert.tradeoff_nonlinear_select(rows, rough)
    assert [p["damp"] for p in picks] == [0.5, 1.0]
    assert picks[0]["best"] == 2 and picks[0]["weight"] == 2.0           # 4, 2, 3, 6 -> member 2
    assert picks[1]["best"] == 5 and picks[1]["weight"] == 4.0           # 10, 5, 1, nan -> member 5; the NaN member is never the best
    for p, idx in zip(picks, ([0, 2, 4, 6], [1, 3, 5, 7])):
        k = invert.lcurve_corner([rows[i]["weighted_rms"] for i in idx], [rough[i] for i in idx])
        assert p["corner"] == (None if k is None else idx[k])
        assert p["corner_weight"] == (None if k is None else rows[idx[k]]["weight"])
    # an L: flat misfit while the roughness falls, then a rising misfit
    L_rows = [dict(weight=float(2 ** i), damp=1.0, predicted_rms=1.0, weighted_rms=m, rms=m, disp_failures=0) for i, m in enumerate([1.0, 1.01, 1.02, 2.0, 4.0])]
    pk = invert.tradeoff_nonlinear_select(L_rows, [16.0, 8.0, 4.0, 3.9, 3.8])
    assert pk[0]["corner"] == 2 and pk[0]["corner_weight"] == 4.0 and pk[0]["best"] == 0


def test_crossval_rows_and_selection_on_hand_made_sums():
    nf, nd = 2, 8
    S = nf + 1
    w, d = invert.tradeoff_grid([1.0, 3.0], [0.5])
    meas = np.zeros((2 * S, nf, 2))
    # pair 0: member 0 holds out fold 0, member 1 fold 1, member 2 is the full one; only [member f, group f] counts as held out
    meas[0, :, 0] = [18.0, 1000.0]
    meas[1, :, 0] = [2000.0, 14.0]
    meas[2, :, 0] = [5.0, 3.0]
    meas[3, :, 0] = [50.0, 1.0]
    meas[4, :, 0] = [1.0, 22.0]
    meas[5, :, 0] = [30.0, 2.0]
    meas[..., 1] = -1.0                                                # the plain sums are not used
    fails = [1, 0, 2, 0, 0, 0]
    rows = invert.crossval_nonlinear_rows(w, d, nf, meas, fails, [0.25, 0.75], nd)
    assert [tuple(r) for r in rows] == [taipei.CROSSVAL_NONLINEAR_COLUMNS] * 2
    assert rows[0] == dict(weight=1.0, damp=0.5, heldout_rms=2.0, full_rms=1.0, cv_rms=0.25, disp_failures=3)
    assert rows[1] == dict(weight=3.0, damp=0.5, heldout_rms=3.0, full_rms=2.0, cv_rms=0.75, disp_failures=0)
    assert invert.crossval_nonlinear_select(rows) == 0
    tie = [dict(rows[0]), dict(rows[1], heldout_rms=2.0)]
    assert invert.crossval_nonlinear_select(tie) == 1                   # ties to the larger weight, as crossval_select
    assert invert.crossval_nonlinear_select([dict(rows[0], heldout_rms=float("nan"))]) is None


# ---- files ----------------------------------------------------------------------------------------------------------------------

def test_files_round_trip_bit_for_bit(tmp_path):
    r = np.random.default_rng(3)
    v = lambda: float(r.random() * 10.0 ** r.integers(-8, 8))
    rows = [dict(weight=v(), damp=v(), predicted_rms=v(), weighted_rms=v(), rms=v(), disp_failures=int(r.integers(0, 1000))) for _ in range(9)]
    rows.append(dict(weight=0.1, damp=0.0, predicted_rms=1.0 / 3.0, weighted_rms=5e-324, rms=1.7976931348623157e308, disp_failures=0))
    p = str(tmp_path / "t.dat")
    taipei.write_tradeoff_nonlinear(p, rows)
    back = taipei.read_tradeoff_nonlinear(p)
    assert back == rows
    for a, b in zip(rows, back):
        assert all(np.float64(a[k]).view(np.uint64) == np.float64(b[k]).view(np.uint64) for k in taipei.TRADEOFF_NONLINEAR_COLUMNS[:-1])
    assert open(p).readline().split() == ["#"] + list(taipei.TRADEOFF_NONLINEAR_COLUMNS)
    rows = [dict(weight=v(), damp=v(), heldout_rms=v(), full_rms=v(), cv_rms=v(), disp_failures=int(r.integers(0, 1000))) for _ in range(7)]
    p = str(tmp_path / "c.dat")
    taipei.write_crossval_nonlinear(p, rows)
    back = taipei.read_crossval_nonlinear(p)
    assert back == rows
    for a, b in zip(rows, back):
        assert all(np.float64(a[k]).view(np.uint64) == np.float64(b[k]).view(np.uint64) for k in taipei.CROSSVAL_NONLINEAR_COLUMNS[:-1])
    assert open(p).readline().split() == ["#"] + list(taipei.CROSSVAL_NONLINEAR_COLUMNS)


# ---- refusals -------------------------------------------------------------------------------------------------------------------

def test_the_flags_need_their_sweep_and_device_rows(capsys):
    invert.check_tradeoff_nonlinear(False, None, True)
    invert.check_crossval_nonlinear(False, None, True)
    invert.check_tradeoff_nonlinear(True, [1.0], False)
    invert.check_crossval_nonlinear(True, 2, False)
    with pytest.raises(ValueError, match="--tradeoff-weights"):
        invert.check_tradeoff_nonlinear(True, None, False)
    with pytest.raises(ValueError, match="--host-rows"):
        invert.check_tradeoff_nonlinear(True, [1.0], True)
    with pytest.raises(ValueError, match="--crossval"):
        invert.check_crossval_nonlinear(True, None, False)
    with pytest.raises(ValueError, match="--host-rows"):
        invert.check_crossval_nonlinear(True, 2, True)
    # run() refuses before it touches the library or the input; the command line refuses with a usage error
    with pytest.raises(ValueError, match="--tradeoff-weights"):
        invert.run("/nonexistent", tradeoff_nonlinear=True)
    with pytest.raises(ValueError, match="--crossval"):
        invert.run("/nonexistent", crossval_nonlinear=True)
    for argv in (["x", "--tradeoff-nonlinear"], ["x", "--crossval-nonlinear"], ["x", "--tradeoff-weights", "1,2", "--tradeoff-nonlinear", "--host-rows"],
                 ["x", "--crossval", "2", "--crossval-weights", "1", "--crossval-nonlinear", "--host-rows"]):
        with pytest.raises(SystemExit) as ei:
            invert.main(argv)
        assert ei.value.code == 2
        assert "nonlinear" in capsys.readouterr().err


# ---- argument checks of the two entries, before any engine ----------------------------------------------------------------------

FILL = np.float32(-7.0)


def steps_call(lib, c, **over):
    """dsa_forward_steps on the boundary case with two zero steps and every output given, one argument replaced; returns (rc, outputs)"""
    f = np.float32
    nd, n, K = c["ndata"], c["nparpi"], 2
    a = dict(nx=c["nx"], ny=c["ny"], nz=c["nz"], nmodels=K, vsf=np.ascontiguousarray(c["vels"].transpose(2, 1, 0), f), steps=np.zeros((K, n), f), alpha=None,
             minvel=2.2, maxvel=4.0, models_out=np.full((K, c["nz"], c["ny"], c["nx"]), FILL, f), dsurf=np.full((K, nd), FILL, f), ldd=nd, dicing=8,
             disp_failures=np.full(K, -7, np.int64), obst=np.ones(nd, f), datweight=np.ones(nd, f), group=np.zeros(nd, np.int32), ngroups=1,
             measures=np.full((K, 1, 2), -7.0))
    tail = list(taipei._args(c)[1])
    if "tail" in over:
        pos, val = over.pop("tail")
        tail[pos] = val
    a.update(over)
    i32 = lambda v: None if v is None else C.byref(C.c_int(int(v)))
    f32 = lambda v: None if v is None else C.byref(C.c_float(float(v)))
    p = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)
    rc = lib.dsa_forward_steps(i32(a["nx"]), i32(a["ny"]), i32(a["nz"]), i32(a["nmodels"]), p(a["vsf"]), p(a["steps"]), p(a["alpha"]), f32(a["minvel"]), f32(a["maxvel"]),
                               p(a["models_out"]), p(a["dsurf"]), i32(a["ldd"]), i32(a["dicing"]), p(a["disp_failures"]), p(a["obst"]), p(a["datweight"]), p(a["group"]),
                               i32(a["ngroups"]), p(a["measures"]), *tail)
    return rc, a


def untouched(a):
    return all(v is None or (v == -7).all() for v in (a["models_out"], a["dsurf"], a["disp_failures"], a["measures"]))


BAD = [("nmodels 0", dict(nmodels=0)), ("nmodels -1", dict(nmodels=-1)), ("nx 2", dict(nx=2)), ("ny 2", dict(ny=2)), ("nz 1", dict(nz=1)),
       ("dicing 4", dict(dicing=4)), ("dicing 0", dict(dicing=0)), ("dicing 16", dict(dicing=16)), ("ldd below ndata", dict(ldd=112)),
       ("measures without obst", dict(obst=None)), ("ngroups 0", dict(ngroups=0)), ("ngroups -3", dict(ngroups=-3)),
       ("group id at ngroups", dict(group=np.r_[np.zeros(112, np.int32), np.int32(2)], ngroups=2)),
       ("negative group id", dict(group=np.r_[np.int32(-1), np.zeros(112, np.int32)], ngroups=2)),
       ("null nx", dict(nx=None)), ("null nz", dict(nz=None)), ("null nmodels", dict(nmodels=None)), ("null vsf", dict(vsf=None)), ("null minvel", dict(minvel=None)),
       ("null maxvel", dict(maxvel=None)), ("null ldd with dsurf", dict(ldd=None)), ("null dicing", dict(dicing=None)), ("null depz", dict(tail=(15, None))),
       ("null goxdf", dict(tail=(0, None))), ("null nrcf", dict(tail=(25, None)))]


@pytest.mark.parametrize("what,over", BAD, ids=[b[0] for b in BAD])
def test_forward_steps_refuses_bad_arguments_before_the_engine(lib, what, over):
    lib.dsa_dropin_error.restype = C.c_char_p
    c = synth.boundary_case()
    assert c["ndata"] == 113 and c["nparpi"] == 360
    rc, a = steps_call(lib, c, **dict(over))
    assert rc == ERR_ARGUMENT, (what, rc, lib.dsa_dropin_error())
    assert b"dsa_forward_steps" in lib.dsa_dropin_error()
    assert untouched(a), what


def test_step_models_refuses_bad_arguments_without_an_engine(lib):
    f = np.float32
    lib.dsa_step_models.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p]
    nx, ny, nz, K = 5, 4, 3, 2
    vsf = np.full(nx * ny * nz, 3.0, f)
    steps = np.zeros(K * (nx - 2) * (ny - 2) * (nz - 1), f)
    out = np.full(K * nx * ny * nz, FILL, f)
    p = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)
    # no engine: an argument error whatever else is given (there is no GPU to make one on here); with a handle the same checks come first
    fake = C.c_void_p(0)
    for args in ((nx, ny, nz, K, vsf, steps, out), (nx, ny, nz, 0, vsf, steps, out), (2, ny, nz, K, vsf, steps, out), (nx, 2, nz, K, vsf, steps, out),
                 (nx, ny, 1, K, vsf, steps, out), (nx, ny, nz, K, None, steps, out), (nx, ny, nz, K, vsf, steps, None)):
        a = args
        assert lib.dsa_step_models(fake, a[0], a[1], a[2], a[3], p(a[4]), p(a[5]), None, 2.2, 4.0, p(a[6])) == ERR_ARGUMENT, args[:4]
    assert (out == FILL).all()
