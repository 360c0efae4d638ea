"""All analyses of dsurftomo_amd/invert.py in one run on the committed Taipei case: what no other test covers is their order in a pass and the
couplings between them (dsurftomo_amd/analyses; SOLVE_ORDER and REPORT_ORDER in invert.py).  Every K is small: only order and coupling are
under test, the numbers of each analysis have their own tests.  Three runs of two outer iterations: plain, all analyses, all but Voronoi."""
import os

import numpy as np
import pytest

from dsurftomo_amd import invert
from dsurftomo_amd import io as taipei

pytestmark = pytest.mark.gpu

# the log-line prefixes of the analyses, the longer of two that share a beginning first
PREFIXES = (" line search", " bootstrap", " checkerboard", " tradeoff nonlinear", " crossval nonlinear", " tradeoff", " crossval", " voronoi", " azimuthal")
# the analyses' lines from " 2th iteration..." to the end of the log, as the loop logged them before the analyses became modules: the reports'
# order (not the solve order), then the step after the loop
ITERATION_2 = [" line search", " bootstrap", " checkerboard", " checkerboard", " tradeoff", " tradeoff", " crossval", " crossval", " crossval",
               " tradeoff nonlinear", " tradeoff nonlinear", " crossval nonlinear", " crossval nonlinear", " voronoi", " azimuthal", " azimuthal"]
EXTRA = ["LineSearch.dat", "Std.dat", "Checker.dat.k01", "Tradeoff.dat", "TradeoffNonlinear.dat", "Crossval.dat", "CrossvalResiduals.dat",
         "CrossvalNonlinear.dat", "Voronoi.dat", "Azim.dat"]


def f32(v):
    return float(np.float32(v))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """(directory, log, history) of the plain run, the run with every analysis, and that run without the Voronoi ensemble.  The sweeps are set
    to the second (last) iteration, where the bootstrap, the checkerboard and the ensemble run: all in one pass."""
    c = taipei.load()
    w0 = float(c["weight0"])
    kw = dict(bootstrap=8, checkerboard=[(2, 2, 2)], tradeoff_weights=[f32(0.5 * w0), w0, f32(2.0 * w0)], tradeoff_nonlinear=True, tradeoff_iter=2,
              crossval=3, crossval_weights=[w0, f32(2.0 * w0)], crossval_by="path", crossval_nonlinear=True, crossval_iter=2, voronoi=(8, 50),
              line_search=[1.0], azimuthal=True)
    out = {}
    for name, options in (("plain", {}), ("all", kw), ("no_voronoi", {k: v for k, v in kw.items() if k != "voronoi"})):
        d = tmp_path_factory.mktemp(name)
        log = []
        _, hist = invert.run(taipei.HERE, maxiter=2, out_dir=str(d), log=log.append, **options)
        out[name] = (d, log, hist)
    return out


def test_the_plain_runs_files_are_unchanged(runs):
    """--line-search 1, the Voronoi ensemble without --voronoi-update and the azimuthal step apply nothing, and no analysis touches the model"""
    plain, both = runs["plain"][0], runs["all"][0]
    names = sorted(os.listdir(plain))
    assert len(names) == 5                          # residualFirst / residualLast, two .iterNNN and <input>Measure.dat
    for nm in names:
        assert (plain / nm).read_bytes() == (both / nm).read_bytes(), nm
    assert sorted(os.listdir(both)) == sorted(names + ["DSurfTomo.in" + e for e in EXTRA])
    assert sorted(os.listdir(runs["no_voronoi"][0])) == sorted(names + ["DSurfTomo.in" + e for e in EXTRA if e != "Voronoi.dat"])


def test_the_log_keeps_the_reports_order(runs):
    log = runs["all"][1]
    tail = log[log.index(" 2th iteration..."):]
    seen = [next(p for p in PREFIXES if l.startswith(p)) for l in tail if l.startswith(PREFIXES)]
    assert seen == ITERATION_2
    assert tail[-1] == "Program finishes successfully"
    # the first iteration has the line search alone; the plain run's lines are all there, in order, timings aside
    head = log[:log.index(" 2th iteration...")]
    assert [p for l in head for p in PREFIXES if l.startswith(p)] == [" line search"]
    strip = lambda lines: [l for l in lines if "(forward" not in l and not l.startswith(PREFIXES)]
    assert strip(log) == strip(runs["plain"][1])


def test_the_history_holds_every_analysis_where_it_ran(runs):
    hist = runs["all"][2]
    assert len(hist) == 3 and list(hist[2]) == ["azimuthal"]
    own = ["mean_ms", "std_ms", "rms", "dv_min", "dv_max", "itn", "istop", "nar", "m", "dws", "seconds"]
    assert list(hist[0]) == own + ["line_search"]
    assert list(hist[1]) == own + ["line_search", "bootstrap", "checkerboard", "tradeoff", "crossval", "tradeoff_nonlinear", "crossval_nonlinear", "voronoi"]
    for h, p in zip(hist[:2], runs["plain"][2]):
        assert {k: h[k] for k in own if k != "seconds"} == {k: p[k] for k in own if k != "seconds"}
    assert hist[1]["bootstrap"]["realisations"] == 8 and hist[1]["voronoi"]["realisations"] == 8 and hist[1]["tradeoff"]["realisations"] == 3
    assert hist[1]["crossval"]["realisations"] == 8 and hist[1]["crossval"]["calls"] == 1


def test_the_crossvalidations_updates_stay_resident_only_without_the_ensemble(runs):
    """one dsa_lsmr_crossval call holds both pairs; the Voronoi batch solve that follows it in the pass would overwrite the solutions that
    dsa_forward_steps(steps = NULL) reads, so with it the updates go through the host -- and give the same numbers"""
    with_v, without = runs["all"][2][1]["crossval_nonlinear"], runs["no_voronoi"][2][1]["crossval_nonlinear"]
    assert with_v["resident"] is False and without["resident"] is True
    assert "crossval_nonlinear" not in runs["all"][2][0]
    assert with_v["members"] == without["members"] and with_v["best"] == without["best"]
    assert np.array_equal(with_v["dsyn"], without["dsyn"])
