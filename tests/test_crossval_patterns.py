"""The host side of the K-fold cross-validation (dsurftomo_amd.invert): the folds, the members' scores and the two selections, the
chunk size of the dsa_lsmr_crossval calls, the checks of --crossval* before the library is loaded and the writer of
<input>Crossval.dat.  Host code only: runs without a GPU."""
import numpy as np
import pytest

from dsurftomo_amd import invert
from dsurftomo_amd import io as taipei


@pytest.fixture(scope="module")
def case():
    return taipei.load()


def test_datum_table_is_in_data_order(case):
    """the table's coordinates give the distances of the data file in its order: the table is in the data order of dsurf"""
    c = case
    slot, src, rec = invert.datum_table(c)
    assert slot.shape == (c["ndata"],) and src.shape == rec.shape == (c["ndata"], 2) and src.dtype == np.uint32
    assert (np.diff(slot) >= 0).all() and slot.min() >= 0 and slot.max() < c["kmax"]
    s, r = src.view(np.float32), rec.view(np.float32)
    some = np.linspace(0, c["ndata"] - 1, 97).astype(int)
    dist = np.array([taipei.delsph(s[i, 0], s[i, 1], r[i, 0], r[i, 1]) for i in some], np.float32)
    assert np.array_equal(dist, c["dist"][some])


@pytest.mark.parametrize("by", ["datum", "path"])
def test_folds_are_deterministic_per_seed(case, by):
    a = invert.crossval_folds(case, 5, by, 3)
    assert a.dtype == np.int32 and a.shape == (case["ndata"],) and a.min() >= 0 and a.max() < 5
    assert np.array_equal(a, invert.crossval_folds(case, 5, by, 3))
    assert not np.array_equal(a, invert.crossval_folds(case, 5, by, 4))


@pytest.mark.parametrize("nfolds", [1, 2, 5, 7])
def test_datum_folds_differ_in_size_by_at_most_one(case, nfolds):
    f = invert.crossval_folds(case, nfolds, "datum", 1)
    cnt = np.bincount(f, minlength=nfolds)
    assert cnt.sum() == case["ndata"] and cnt.max() - cnt.min() <= 1
    assert np.array_equal(f, np.random.default_rng(1).permutation(case["ndata"]) % nfolds)


def test_path_folds_keep_a_station_pair_together(case):
    c = case
    f = invert.crossval_folds(c, 5, "path", 1)
    assert (np.bincount(f, minlength=5) > 0).all()
    _, src, rec = invert.datum_table(c)
    seen = {}
    for i in range(c["ndata"]):
        key = frozenset((tuple(src[i]), tuple(rec[i])))
        assert seen.setdefault(key, int(f[i])) == int(f[i])
    assert len(seen) < c["ndata"]                                   # (pairs recur across periods: the rule has something to keep together)
    assert len(set(seen.values())) == 5


def test_folds_reject_bad_arguments(case):
    with pytest.raises(ValueError):
        invert.crossval_folds(case, 0)
    with pytest.raises(ValueError):
        invert.crossval_folds(case, 3, "station")


def member(weight, damp, cv_rms, cv_se=0.0):
    return dict(weight=weight, damp=damp, cv_rms=cv_rms, cv_se=cv_se, train_rms=0.5 * cv_rms, misfit=1.0, rough=1.0, xnorm=1.0, itn_min=3, itn_max=9)


def test_crossval_select_minimum_and_ties():
    ms = [member(1.0, 0.5, 3.0), member(2.0, 0.5, 2.0), member(4.0, 0.5, 2.5), member(8.0, 0.5, 4.0)]
    assert invert.crossval_select(ms) == dict(best=1, one_se=1)
    # equal cv_rms: the larger weight, then the larger damp
    ms = [member(1.0, 0.5, 2.0), member(2.0, 0.5, 2.0), member(2.0, 1.5, 2.0), member(8.0, 0.5, 4.0)]
    assert invert.crossval_select(ms)["best"] == 2
    assert invert.crossval_select(ms[::-1])["best"] == 1
    ms = [member(2.0, 1.5, 2.0), member(2.0, 0.5, 2.0)]
    assert invert.crossval_select(ms) == dict(best=0, one_se=0)
    with pytest.raises(ValueError):
        invert.crossval_select([])


def test_crossval_select_one_se_moves_to_a_larger_weight():
    # cv_rms^2: 9, 4, 4.9, 5.1, 16; best = 1 with se 1: the limit is 5 -> weight 4 qualifies, weight 6 does not
    ms = [member(1.0, 0.5, 3.0), member(2.0, 0.5, 2.0, 1.0), member(4.0, 0.5, np.sqrt(4.9)), member(6.0, 0.5, np.sqrt(5.1)), member(8.0, 0.5, 4.0)]
    assert invert.crossval_select(ms) == dict(best=1, one_se=2)
    ms[1]["cv_se"] = 1.2                                            # the limit 5.2 lets weight 6 in
    assert invert.crossval_select(ms) == dict(best=1, one_se=3)
    ms[1]["cv_se"] = 0.0
    assert invert.crossval_select(ms) == dict(best=1, one_se=1)
    # among equal weights within the limit, the larger damp
    ms = [member(2.0, 0.5, 2.0, 1.0), member(4.0, 0.5, 2.1), member(4.0, 2.0, 2.2)]
    assert invert.crossval_select(ms) == dict(best=0, one_se=2)


def test_crossval_members_scores():
    """two combos x (3 folds + full) with hand-made measures: the scores from their definitions"""
    fold = np.array([0, 0, 1, 1, 1, 0, 1], np.int32)                # fold 2 is empty
    cnt = np.array([3.0, 4.0, 0.0])
    meas = np.zeros((8, 4))
    meas[:, 0] = [4.0, 3.0, 8.0, 8.0, 2.0, 1.0, 5.0, 5.0]
    meas[:3, 1] = [6.0, 2.0, 0.0]
    meas[4:7, 1] = [9.0, 12.0, 0.0]
    meas[:, 2] = np.arange(8) + 1.0
    meas[:, 3] = 2.0 * np.arange(8) + 1.0
    res = dict(weight=np.array([1.0, 2.0], np.float32), damp=np.array([0.5, 0.25], np.float32), nfolds=3, measures=meas,
               itn=np.array([5, 7, 6, 6, 9, 3, 4, 4], np.int32))
    ms = invert.crossval_members(res, fold)
    assert [m["weight"] for m in ms] == [1.0, 2.0] and [m["damp"] for m in ms] == [0.5, 0.25]
    assert ms[0]["cv_rms"] == np.sqrt(8.0 / 7.0) and ms[1]["cv_rms"] == np.sqrt(21.0 / 7.0)
    per = np.array([6.0, 2.0]) / cnt[:2]
    assert ms[0]["cv_se"] == pytest.approx(per.std(ddof=1) / np.sqrt(2.0), rel=1e-15)
    assert ms[1]["cv_se"] == 0.0                                     # 9/3 == 12/4
    assert ms[0]["train_rms"] == np.sqrt(15.0 / 14.0)                # kept 4 + 3 + 8 over 4 + 3 + 7 training rows
    assert (ms[0]["misfit"], ms[0]["rough"], ms[0]["xnorm"]) == (np.sqrt(8.0), 2.0, np.sqrt(7.0))
    assert (ms[0]["itn_min"], ms[0]["itn_max"], ms[1]["itn_min"], ms[1]["itn_max"]) == (5, 7, 3, 9)
    assert set(ms[0]) == set(invert.CROSSVAL_COLUMNS)


def crossval_bytes(m, n, nar, L, ncombo, nfolds, ndata):
    """the device buffers of a dsa_lsmr_crossval call (lsmr_batch.hip): batch_begin's for R = ncombo (nfolds + 1) members with the temporary
    R n + m + ncombo + ndata, the two coefficient copies, the measures' partials and results and the residuals (fp64)"""
    R = ncombo * (nfolds + 1)
    G = (R + 63) // 64
    Rp = 64 * G
    L = max(0, min(L, m, n))
    mx = max(m, n)
    floats = 2 * G * m * 64 + 4 * G * n * 64 + G * n * 64 * L + 12 * Rp + 3 * Rp + G * mx * 64 + G * (-(-mx // 256)) * 64 + R * n + m + ncombo + ndata
    doubles = G * (-(-m // 64)) * 64 * 3 + G * (-(-n // 1024)) * 64 + 4 * Rp + 2 * ncombo * ndata
    return 4 * floats + 8 * nar + 8 * doubles + 4


@pytest.mark.parametrize("m,n,L", [(4109, 2048, 10), (100001, 68479, 10), (3_000_000, 1_500_000, 10), (40_000_000, 20_000_000, 10), (10, 5, 10)])
@pytest.mark.parametrize("ncombo,nfolds", [(13, 5), (39, 5), (1000, 10), (3, 2)])
def test_crossval_chunk_is_a_whole_number_of_combos(m, n, L, ncombo, nfolds):
    nd = m - n
    nar = 60 * nd + 7 * n
    k = invert.crossval_chunk(m, n, nar, L, ncombo, nfolds, nd)
    assert isinstance(k, int) and 1 <= k <= ncombo and k * (nfolds + 1) <= max(4096, nfolds + 1)
    budget = 32 << 30
    if k > 1:
        assert crossval_bytes(m, n, nar, L, k, nfolds, nd) <= budget
        assert invert.crossval_bytes(m, n, nar, L, k, nfolds, nd) >= crossval_bytes(m, n, nar, L, k, nfolds, nd)
    if k < min(ncombo, 4096 // (nfolds + 1)):                        # lowered only as far as needed
        assert invert.crossval_bytes(m, n, nar, L, k + 1, nfolds, nd) > budget
    assert invert.crossval_chunk(m, n, nar, L, ncombo, nfolds, nd) == k
    assert invert.crossval_chunk(m, n, nar, L, ncombo, nfolds, nd, budget=1) == 1


def test_crossval_file_round_trips(tmp_path):
    f = np.float32
    rng = np.random.default_rng(4)
    members = [dict(weight=float(f(w)), damp=float(f(d)), cv_rms=float(rng.random() * 3), cv_se=float(rng.random() * 1e-3), train_rms=float(rng.random()),
                    misfit=float(rng.random() * 10), rough=float(rng.random() * 1e-3), xnorm=float(rng.random()), itn_min=int(rng.integers(0, 40)),
                    itn_max=int(rng.integers(40, 400)))
               for w in (0.0, 0.1, 2.0, 11.3) for d in (0.0, 1.0 / 3.0)]
    path = tmp_path / "DSurfTomo.inCrossval.dat"
    invert.write_crossval(str(path), members)
    rows = path.read_text().splitlines()
    assert len(rows) == len(members) and all(len(r.split()) == len(invert.CROSSVAL_COLUMNS) for r in rows)
    assert invert.read_crossval(str(path)) == members
    path.write_text("1 2 3\n")
    with pytest.raises(ValueError):
        invert.read_crossval(str(path))


def test_crossval_residual_file_and_slots(tmp_path):
    slot = np.array([0, 0, 2, 2, 2], np.int32)
    held = np.array([3.0, -4.0, 1.0, 2.0, -2.0])
    assert invert.crossval_by_slot(slot, held, 4) == [np.sqrt(12.5), None, np.sqrt(3.0), None]
    path = tmp_path / "r.dat"
    invert.write_crossval_residuals(str(path), slot, np.arange(5, dtype=np.float32) + 0.5, [0, 1, 0, 1, 1], np.ones(5, np.float32), held, 0.5 * held)
    rows = [r.split() for r in path.read_text().splitlines()]
    assert len(rows) == 5 and all(len(r) == 7 for r in rows)
    assert [int(r[0]) for r in rows] == [1, 2, 3, 4, 5] and [int(r[1]) for r in rows] == [1, 1, 3, 3, 3] and [int(r[3]) for r in rows] == [0, 1, 0, 1, 1]
    assert [float(r[5]) for r in rows] == held.tolist() and [float(r[6]) for r in rows] == (0.5 * held).tolist()


BAD = [dict(nfolds=1, weights=[1.0]), dict(nfolds=0, weights=[1.0]), dict(nfolds=5), dict(nfolds=5, weights=[]), dict(nfolds=5, weights=[1.0, -2.0]),
       dict(nfolds=5, weights=[1.0], damps=[]), dict(nfolds=5, weights=[1.0], damps=[float("nan")]), dict(nfolds=5, weights=[1.0], host_rows=True),
       dict(nfolds=5, weights=[1.0], iteration=0), dict(nfolds=5, weights=[1.0], iteration=3, maxiter=2), dict(nfolds=None, weights=[1.0]),
       dict(nfolds=None, damps=[1.0]), dict(nfolds=5, weights=[1.0], by="station"), dict(nfolds=5, weights=[1.0], chunk=0)]


@pytest.mark.parametrize("kw", BAD)
def test_check_crossval_rejects(kw):
    with pytest.raises(ValueError):
        invert.check_crossval(**kw)


def test_check_crossval_accepts():
    invert.check_crossval(None)
    invert.check_crossval(2, [1.0, 2.0])
    invert.check_crossval(5, [0.0], [0.0, 1.0], "path", 2, False, 2, 3)


@pytest.mark.parametrize("argv", [["--crossval", "1", "--crossval-weights", "1,2"], ["--crossval", "5"], ["--crossval", "5", "--crossval-weights", "1,2", "--host-rows"],
                                  ["--crossval", "5", "--crossval-weights", "1,-2"], ["--crossval", "5", "--crossval-weights", "1,2", "--crossval-damps", "x"],
                                  ["--crossval", "5", "--crossval-weights", "1,2", "--crossval-iter", "0"],
                                  ["--crossval", "5", "--crossval-weights", "1,2", "--crossval-iter", "3", "--maxiter", "2"],
                                  ["--crossval-weights", "1,2"], ["--crossval", "5", "--crossval-weights", "1,2", "--crossval-by", "station"]])
def test_cli_rejects_bad_crossval_arguments_before_the_library(monkeypatch, tmp_path, argv):
    def refuse():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(invert, "load_library", refuse)
    with pytest.raises(SystemExit) as exc:
        invert.main([str(tmp_path)] + argv)
    assert exc.value.code == 2


@pytest.mark.parametrize("kw", [dict(crossval=1, crossval_weights=[1.0]), dict(crossval=5), dict(crossval=5, crossval_weights=[1.0], host_rows=True),
                                dict(crossval=5, crossval_weights=[1.0], crossval_iter=0), dict(crossval=5, crossval_weights=[1.0], crossval_iter=3, maxiter=2),
                                dict(crossval_weights=[1.0])])
def test_run_rejects_bad_crossval_arguments_before_the_library(monkeypatch, tmp_path, kw):
    def refuse():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(invert, "load_library", refuse)
    with pytest.raises(ValueError):
        invert.run(str(tmp_path), **kw)


def test_help_says_why_path_folds():
    import io as _io
    from contextlib import redirect_stdout
    buf = _io.StringIO()
    with redirect_stdout(buf), pytest.raises(SystemExit):
        invert.main(["--help"])
    text = " ".join(buf.getvalue().split())
    assert "--crossval-by" in text and "correlated along period" in text
