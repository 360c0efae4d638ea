"""The wiring of the depth driver on the device (dsurftomo_amd/depth.py): depth.run(**options) against the same stage
functions called by hand, in the documented order with the documented arguments, on a second fresh engine -- the two output directories
must hold the same files with the same bytes (tests/test_gpu_engine_reuse.py: the call order does not change an engine's bits, so there is
no tolerance).  The small case of the pattern tests, 6 x 5 x 3 nodes and 4 periods; the observations are the device's own curves of
columns_ref.smooth_model, written with maps.write_maps, the start is columns_ref.perturbed of it (tests/test_gpu_columns.py's loop).

The issue's third case, radial + radial_lateral + radial_resolution, is one the driver refuses (check_radial_resolution: the resolution of
the laterally coupled radial system is not computed), so it is run as its two halves: radial + radial_lateral and radial +
radial_resolution.  No new device code runs here; each case is a handful of tiny launches."""
import os

import numpy as np
import pytest

import columns_ref as R
import test_depth_patterns as T21
from dsurftomo_amd import depth, io, maps
from dsurftomo_amd.engine import Engine

pytestmark = pytest.mark.gpu

F = np.float32
NX, NY, NZ = 6, 5, 3
D = depth
LOOP = (D.DEFAULT_ITERATIONS, D.DEFAULT_SMOOTH, D.DEFAULT_DAMP, D.DEFAULT_DVMAX)
CG = (D.DEFAULT_LATERAL_TOL, D.DEFAULT_LATERAL_MAXIT)
SAMPLER = (D.DEFAULT_SAMPLE_STEP, D.DEFAULT_SAMPLE_SPREAD, D.DEFAULT_SAMPLE_WIDTH, D.DEFAULT_SAMPLE_SEED, D.DEFAULT_SAMPLE_TEMPERATURE)
quiet = lambda *_: None


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """(the case, the path of its maps file): the maps are the device's curves of the smooth truth, the case starts at the perturbed truth"""
    truth = R.smooth_model(NX, NY, NZ)
    c = dict(T21.small_case(io.load()))
    c["vels"] = np.ascontiguousarray(R.perturbed(truth).transpose(2, 1, 0))
    eng = Engine(0)
    try:
        eng.dispersion_begin(truth, c["depz"], c["minthk"], c["kmax"], c["kmax"])
        for wave, kind, t, first in depth.slot_plan(c):
            eng.dispersion_run(wave, kind, t, True, first, first)
        curves = eng.dispersion_fetch(0, c["kmax"], False, 0).astype(F)
    finally:
        eng.close()
    assert (curves[:, R.interior(NX, NY) == 1] > 0).all()
    path = str(tmp_path_factory.mktemp("maps") / "Maps.dat")
    maps.write_maps(path, c, curves, np.ones(c["kmax"] * (NX - 2) * (NY - 2), F))
    return c, path


def isotropic(eng, c, plan, obs, lateral=None):
    """the isotropic loop as run() documents it: the begin, iterate, the model; returns (iterate's result with vels, the data's sigma)"""
    eng.dispersion_begin(np.ascontiguousarray(np.asarray(c["vels"], F).transpose(2, 1, 0)), c["depz"], c["minthk"], c["kmax"], c["kmax"])
    out = depth.iterate(eng, plan, obs, None, *LOOP, float(c["minvel"]), float(c["maxvel"]), quiet, lateral, *CG)
    out["vels"] = eng.dispersion_get_model()
    return out, out["history"][-1]["rms"]


def two_files(c, out, d):
    depth.write_depth(os.path.join(d, "DSurfTomo.inDepth.dat"), c, out["vels"])
    depth.write_fit(os.path.join(d, "DSurfTomo.inDepthFit.dat"), c, out["steps"][0], out["steps"][-1])


def by_hand_resolution(eng, c, plan, obs, d):
    out, sigma = isotropic(eng, c, plan, obs)
    depth.resolve(eng, c, plan, obs, None, D.DEFAULT_SMOOTH, D.DEFAULT_DAMP, sigma, d, quiet)
    two_files(c, out, d)


def by_hand_lateral(eng, c, plan, obs, d):
    out, sigma = isotropic(eng, c, plan, obs, 0.3)
    depth.resolve_lateral(eng, c, plan, obs, None, D.DEFAULT_SMOOTH, D.DEFAULT_DAMP, 0.3, *CG, sigma, d, 2, (2, 2, 1, D.DEFAULT_CHECKER_AMP), quiet)
    two_files(c, out, d)


def by_hand_radial_lateral(eng, c, plan, obs, d):
    depth.run_radial(eng, c, plan, obs, None, *LOOP[:3], D.DEFAULT_ANISO, LOOP[3], d, quiet, 0.3, None, *CG)


def by_hand_radial_resolution(eng, c, plan, obs, d):
    out = depth.run_radial(eng, c, plan, obs, None, *LOOP[:3], D.DEFAULT_ANISO, LOOP[3], d, quiet, None, None, *CG)[0]
    depth.resolve_radial(eng, c, plan, obs, None, D.DEFAULT_SMOOTH, D.DEFAULT_DAMP, D.DEFAULT_ANISO, out["history"][-1]["rms"], d, quiet)


def by_hand_sample(eng, c, plan, obs, d):
    out, sigma = isotropic(eng, c, plan, obs)
    levels = depth.parse_quantiles(D.DEFAULT_SAMPLE_QUANTILES)
    depth.run_sample(eng, c, plan, out["vels"], obs, None, D.DEFAULT_SMOOTH, sigma, (4, 6, 2), d, *SAMPLER, quiet, 2, None, D.DEFAULT_DAMP, (4, levels, True))
    two_files(c, out, d)


CASES = {
    "resolution": (dict(resolution=True), by_hand_resolution, ("Depth", "DepthFit", "DepthResolution", "DepthLeverage")),
    "lateral_resolution": (dict(lateral=0.3, lateral_resolution=True, lateral_resolution_stride=2, lateral_checkerboard="2,2,1"), by_hand_lateral,
                           ("Depth", "DepthFit", "DepthLateralResolution", "DepthLateralChecker")),
    "radial_lateral": (dict(radial=True, radial_lateral=0.3), by_hand_radial_lateral, ("DepthRadial", "DepthRadialFit")),
    "radial_resolution": (dict(radial=True, radial_resolution=True), by_hand_radial_resolution,
                          ("DepthRadial", "DepthRadialFit", "DepthRadialResolution", "DepthRadialLeverage")),
    "sample": (dict(sample="4,6,2", sample_block=2, sample_bins=4, sample_covariance=True), by_hand_sample,
               ("Depth", "DepthFit", "DepthPosterior", "DepthPosteriorFit", "DepthPosteriorQuantiles", "DepthPosteriorMarginals", "DepthPosteriorCorrelation")),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_run_writes_what_the_stages_write_by_hand(monkeypatch, tmp_path, case, name):
    c, mpath = case
    options, by_hand, files = CASES[name]
    monkeypatch.setattr(io, "load", lambda *_: c)
    driven, manual = str(tmp_path / "run"), str(tmp_path / "hand")
    os.makedirs(driven); os.makedirs(manual)
    depth.run("case", maps_file=mpath, out_dir=driven, log=quiet, **options)
    obs = depth.maps_to_obs(maps.read_maps(mpath), c)[0]
    eng = Engine(0)
    try:
        by_hand(eng, c, depth.slot_plan(c), obs, manual)
    finally:
        eng.close()
    assert sorted(os.listdir(driven)) == sorted(os.listdir(manual)) == sorted("DSurfTomo.in%s.dat" % f for f in files)
    for f in os.listdir(driven):
        with open(os.path.join(driven, f), "rb") as a, open(os.path.join(manual, f), "rb") as b:
            assert a.read() == b.read(), "%s: %s differs between run() and the stages called by hand" % (name, f)


def test_the_issues_third_case_is_refused_whole():
    with pytest.raises(ValueError, match="--radial-resolution and --radial-lateral exclude each other"):
        depth.check_options(depth.options_over_defaults(dict(radial=True, radial_lateral=0.3, radial_resolution=True)))
