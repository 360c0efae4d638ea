"""dsa_dispersion_begin_radial and dsa_columns_step_radial (csrc/column_kernels.hip: k_column_step_radial) on the device.
The step against the CPU build of the same header (tests/hostcheck_column_radial.cpp through column_radial_ref), bit for bit: the kernel
shares column_radial.h's loops out over a wavefront, every figure is one sequential fp64 chain under -ffp-contract=off, so the lane mapping
cannot show.  The stage against plain stages holding either model; aniso = 0 against dsa_columns_step; the Gauss-Newton loop on a truth with
Vsh 6 % above Vsv next to the isotropic loop; the stage's limits once (nz = 64, K = 60: the one launch above 64 KB of LDS); the refusals.

tests/test_gpu_columns.py's cases: grid 5 x 5 (9 interior columns), three periods of each of the four wave types (K = 12: slots 0-5 Rayleigh,
6-11 Love), nz = 2, 3, 8, smooth_model and edge_model.  The inputs of the host step are the curves and kernels fetched from the device after
the runs, so the dispersion stage's own arithmetic is not under test there."""
import numpy as np
import pytest

import column_radial_ref as RR
import columns_ref as R
from column_radial_ref import same_bits
from dsurftomo_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

F = np.float32
NX, NY, K = R.NX, R.NY, R.K
NCOL = NX * NY
RING = R.interior(NX, NY) == 0
CENTRE = 2 * NX + 2
DSA_ERR_ARGUMENT, DSA_ERR_STATE = -2, -5                      # include/dsurftomo_amd.h
ARGS = (R.SMOOTH, R.DAMP, RR.ANISO, R.DVMAX, R.MINVEL, R.MAXVEL)


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def h():
    return RR.load()


@pytest.fixture(scope="module")
def hs():
    return R.load()


def runs(e, waves=R.WAVES):
    first = 0
    for wave, kind, t in waves:
        e.dispersion_run(wave, kind, t, True, first, first)
        first += len(t)


def diagnostics(e):
    """dsa_dispersion_diagnostics through the library itself: (count, first[5], period)"""
    import ctypes as C
    cnt = C.c_longlong(0); first = (C.c_int * 5)(); per = C.c_double(0.0)
    fn = e._L.dsa_dispersion_diagnostics
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert fn(e._h, C.byref(cnt), first, C.byref(per)) == 0
    return cnt.value, list(first), per.value


def above(vsv, factor=1.03):
    """Vsh = Vsv * factor above the bottom depth, equal at it"""
    vsh = np.array(vsv, F, copy=True)
    vsh[:-1] = (vsh[:-1] * F(factor)).astype(F)
    return vsh


def case(model_name, nz):
    """test_gpu_columns.py's: weights around 1, a tenth of them 0, the centre column without any"""
    depz = R.depths(nz)
    vel = (R.smooth_model if model_name == "smooth" else R.edge_model)(NX, NY, nz)
    rng = np.random.default_rng(7 + nz)
    wt = (0.5 + rng.random((K, NCOL))).astype(F)
    wt[rng.random((K, NCOL)) < 0.1] = 0.0
    wt[:, CENTRE] = 0.0
    return depz, vel, rng, wt


def against_host(h, hs, e, vsv, vsh, depz, obs, wt, args=ARGS, love=RR.LOVE, nmaps=K):
    """the device's step and the host's on the values fetched before it: every output and both stepped models, bit for bit.  Returns (the
    device's result, the stepped (vsv, vsh), the fetched pv)."""
    nz = vsv.shape[0]
    pv, svs, svp, srho = e.dispersion_fetch(0, nmaps, True, 0)
    Sv = R.host_combine(hs, vsv.reshape(nz, NCOL), depz, svs, svp, srho)
    Sh = R.host_combine(hs, vsh.reshape(nz, NCOL), depz, svs, svp, srho)
    want = RR.host_step(h, love, obs, wt, pv, Sv, Sh, vsv.reshape(nz, NCOL), vsh.reshape(nz, NCOL), *args, R.interior(NX, NY))
    got = e.columns_step_radial(obs, wt, *args)
    after = e.dispersion_get_model_radial()
    for name in ("nused", "flag", "chi2", "dv_sv", "dv_sh"):
        assert same_bits(got[name], want[name]), "%s differs from the host's (%d of %d)" % (name, int((got[name] != want[name]).sum()), got[name].size)
    assert same_bits(after[0].reshape(nz, NCOL), want["vsv"]), "the stepped Vsv differs from the host's"
    assert same_bits(after[1].reshape(nz, NCOL), want["vsh"]), "the stepped Vsh differs from the host's"
    return got, after, pv


@pytest.mark.parametrize("nz", [2, 3, 8])
@pytest.mark.parametrize("model_name", ["smooth", "edge"])
def test_step_equals_the_host_bit_for_bit(eng, h, hs, model_name, nz):
    """smooth_model with observations 2 % off its own curves, edge_model with observations far from its curves (steps clipped, values at the
    bounds) and curves without a root; Vsh 3 % above Vsv; aniso 0 and 0.2.  What stays: the ring, the bottom depth of both models, a column
    whose weights are all 0; nothing is NaN."""
    depz, vsv, rng, wt = case(model_name, nz)
    vsh = above(vsv)
    eng.dispersion_begin_radial(vsv, vsh, depz, R.MINTHK, K, K)
    runs(eng)
    pv0 = eng.dispersion_fetch(0, K, False, 0)
    if model_name == "smooth":
        obs = (pv0 * (1.0 + 0.02 * rng.standard_normal((K, NCOL)))).astype(F)
        base = (R.SMOOTH, R.DAMP, R.DVMAX, R.MINVEL, R.MAXVEL)
    else:
        obs = (2.5 + 1.5 * rng.random((K, NCOL))).astype(F)
        base = (R.SMOOTH, R.DAMP, 0.1, 2.0, 4.5)
        inner_pv = pv0[:, ~RING]
        assert (inner_pv == 0).any() and (inner_pv > 0).any(), "the edge model should lose some roots inside the ring at these periods"
    for n, aniso in enumerate((0.0, RR.ANISO)):
        if n:
            eng.dispersion_begin_radial(vsv, vsh, depz, R.MINTHK, K, K)
            runs(eng)
        args = base[:2] + (aniso,) + base[2:]
        got, after, pv = against_host(h, hs, eng, vsv, vsh, depz, obs, wt, args)
        assert same_bits(pv, pv0)
        used = (wt > 0) & (obs > 0) & (pv > 0)
        assert (got["nused"][0][~RING] == used[~RR.LOVE].sum(axis=0)[~RING]).all() and (got["nused"][1][~RING] == used[RR.LOVE].sum(axis=0)[~RING]).all()
        assert got["flag"][CENTRE] == 2 and not got["nused"][:, CENTRE].any()
        stepped = (got["flag"] == 0) & ~RING
        assert stepped.any()
        for model, before, dv in ((after[0], vsv, got["dv_sv"]), (after[1], vsh, got["dv_sh"])):
            m = model.reshape(nz, NCOL); b = before.reshape(nz, NCOL)
            assert same_bits(m[:, RING], b[:, RING]) and same_bits(m[nz - 1], b[nz - 1]) and same_bits(m[:, CENTRE], b[:, CENTRE])
            assert not dv[:, RING].any() and not dv[:, CENTRE].any()
            assert np.isfinite(m).all() and np.isfinite(dv).all()
            assert np.abs(dv[:, stepped]).max() > 0 and (np.abs(dv) <= F(args[3])).all()
            assert (m[:nz - 1][:, stepped] >= F(args[4])).all() and (m[:nz - 1][:, stepped] <= F(args[5])).all()
        assert not got["nused"][:, RING].any() and not got["chi2"][:, RING].any() and not got["flag"][RING].any() and np.isfinite(got["chi2"]).all()
        if model_name == "edge":
            assert (np.abs(got["dv_sv"]) == F(args[3])).any()                        # clipped at exactly dvmax somewhere
    # without weights: all 1
    eng.dispersion_begin_radial(vsv, vsh, depz, R.MINTHK, K, K)
    runs(eng)
    against_host(h, hs, eng, vsv, vsh, depz, obs, None, base[:2] + (RR.ANISO,) + base[2:])


@pytest.mark.parametrize("model_name,nz", [("smooth", 8), ("edge", 3)])
def test_the_stage_reads_vsh_for_love_and_vsv_for_rayleigh(eng, model_name, nz):
    """begin_radial with vsh = vsv leaves the maps, kernels and diagnostics of dispersion_begin; with vsh != vsv the Love maps and kernels
    are those of a plain stage holding vsh and the Rayleigh ones those of a plain stage holding vsv -- bit for bit"""
    depz, vsv, _, _ = case(model_name, nz)
    vsh = above(vsv, 1.05)

    def plain(vel):
        eng.dispersion_begin(vel, depz, R.MINTHK, K, K)
        runs(eng)
        return eng.dispersion_fetch(0, K, True, 0), diagnostics(eng)

    def radial(a, b):
        eng.dispersion_begin_radial(a, b, depz, R.MINTHK, K, K)
        runs(eng)
        return eng.dispersion_fetch(0, K, True, 0), diagnostics(eng), eng.dispersion_get_model_radial()

    on_v, diag_v = plain(vsv)
    on_h, _ = plain(vsh)
    same, diag_same, models = radial(vsv, vsv)
    assert all(same_bits(a, b) for a, b in zip(same, on_v)) and diag_same == diag_v
    assert same_bits(models[0], vsv) and same_bits(models[1], vsv)
    both, _, models = radial(vsv, vsh)
    assert same_bits(models[0], vsv) and same_bits(models[1], vsh)
    love = RR.LOVE
    assert same_bits(both[0][love], on_h[0][love]) and same_bits(both[0][~love], on_v[0][~love])
    for q in (1, 2, 3):
        assert same_bits(both[q][:, love], on_h[q][:, love]) and same_bits(both[q][:, ~love], on_v[q][:, ~love])
    inner = ~RING
    assert not same_bits(on_h[0][love][:, inner], on_v[0][love][:, inner])             # (the two models do differ in what Love sees)


@pytest.mark.parametrize("nz", [2, 3, 8])
def test_aniso_zero_is_columns_step_on_each_model(eng, nz):
    """aniso = 0: the Vsv block's step is dsa_columns_step on a plain stage holding vsv with the Love weights zeroed, the Vsh block's that on a
    plain stage holding vsh with the Rayleigh weights zeroed -- dv, chi2, nused and the stepped models bit for bit"""
    depz, vsv, rng, wt = case("smooth", nz)
    vsh = above(vsv)
    plain_args = (R.SMOOTH, R.DAMP, R.DVMAX, R.MINVEL, R.MAXVEL)
    love = RR.LOVE
    eng.dispersion_begin(vsv, depz, R.MINTHK, K, K)
    runs(eng)
    pv_v = eng.dispersion_fetch(0, K, False, 0)
    eng.dispersion_begin(vsh, depz, R.MINTHK, K, K)
    runs(eng)
    pv_h = eng.dispersion_fetch(0, K, False, 0)
    pv = np.where(love[:, None], pv_h, pv_v)
    obs = (pv * (1.0 + 0.02 * rng.standard_normal((K, NCOL)))).astype(F)
    want = []
    for vel, mine in ((vsv, ~love), (vsh, love)):
        eng.dispersion_begin(vel, depz, R.MINTHK, K, K)
        runs(eng)
        out = eng.columns_step(obs, np.where(mine[:, None], wt, F(0.0)), *plain_args)
        want.append((out, eng.dispersion_get_model()))
    eng.dispersion_begin_radial(vsv, vsh, depz, R.MINTHK, K, K)
    runs(eng)
    got = eng.columns_step_radial(obs, wt, R.SMOOTH, R.DAMP, 0.0, R.DVMAX, R.MINVEL, R.MAXVEL)
    after = eng.dispersion_get_model_radial()
    for q, name in enumerate(("dv_sv", "dv_sh")):
        out, model = want[q]
        assert same_bits(got[name], out["dv"]) and same_bits(after[q], model), name
        assert same_bits(got["chi2"][q], out["chi2"]) and same_bits(got["nused"][q], out["nused"])
        both = (got["nused"][0] > 0) & (got["nused"][1] > 0)
        assert both[~RING].sum() >= 8 and same_bits(got["flag"][both], out["flag"][both]) and np.abs(out["dv"]).max() > 0


@pytest.mark.parametrize("nz", [3, 8])
def test_loop_explains_the_rayleigh_love_discrepancy(eng, nz):
    """tests/test_hostcheck_column_radial.py's loop on the device's own curves: truth Vsv = smooth_model, Vsh 6 % above it at mid depth, both
    models started at perturbed(truth Vsv), four iterations.  The sum of chi2 before the last radial step is below the one before the first
    and below half of what the isotropic loop (dsa_columns_step on the same observations) has before its last step.  Measured: 9.8e-3 against
    0.675 (nz 8), 8.5e-2 against 0.294 (nz 3)."""
    depz = R.depths(nz)
    truth_v = R.smooth_model(NX, NY, nz)
    truth_h = RR.truth_vsh(truth_v)
    eng.dispersion_begin_radial(truth_v, truth_h, depz, R.MINTHK, K, K)
    runs(eng)
    obs = eng.dispersion_fetch(0, K, False, 0).astype(F)
    assert (obs[:, ~RING] > 0).all()
    start = R.perturbed(truth_v)
    eng.dispersion_begin_radial(start, start, depz, R.MINTHK, K, K)
    chi2, rms = [], []
    for it in range(R.ITERATIONS):
        runs(eng)
        got = eng.columns_step_radial(obs, None, *ARGS)
        assert not got["flag"].any()
        chi2.append(float(got["chi2"].sum()))
        rms.append(tuple(float(np.sqrt(got["chi2"][q].sum() / got["nused"][q].sum())) for q in range(2)))
    vsv, vsh = eng.dispersion_get_model_radial()
    eng.dispersion_begin(start, depz, R.MINTHK, K, K)
    iso = []
    for it in range(R.ITERATIONS):
        runs(eng)
        iso.append(float(eng.columns_step(obs, None, R.SMOOTH, R.DAMP, R.DVMAX, R.MINVEL, R.MAXVEL)["chi2"].sum()))
    xi = (vsh.reshape(nz, NCOL)[:nz - 1, ~RING].astype(np.float64) / vsv.reshape(nz, NCOL)[:nz - 1, ~RING]) ** 2
    print("nz %d: sum of chi2 before each radial step %s; before each isotropic step %s" % (nz, " ".join("%.4g" % x for x in chi2), " ".join("%.4g" % x for x in iso)))
    print("nz %d: rms (Rayleigh, Love) before each radial step %s; xi median %.4f, range %.4f to %.4f" % (nz, " ".join("(%.5f, %.5f)" % r for r in rms), np.median(xi), xi.min(), xi.max()))
    assert chi2[-1] < chi2[0]
    assert chi2[-1] < 0.5 * iso[-1]


def test_the_limits_once(eng, h, hs):
    """nz = 64 (2M = 126 unknowns), K = 60 -- test_gpu_column_resolution.py's period lists -- smooth_model on the 5 x 5 grid, Vsh 3 % above
    Vsv: the one launch that asks for more than 64 KB of LDS (98 232 bytes).  Equal to the host bit for bit, all nine interior columns
    stepped."""
    nz, nmaps = 64, 60
    waves = [(2, 0, np.linspace(3.0, 45.0, 15)), (2, 1, np.linspace(4.0, 46.0, 15)), (1, 0, np.linspace(3.0, 45.0, 15)), (1, 1, np.linspace(4.0, 46.0, 15))]
    love = np.concatenate([np.full(len(t), wave == 1) for wave, _, t in waves])
    depz = R.depths(nz)
    vsv = R.smooth_model(NX, NY, nz)
    vsh = above(vsv)
    assert h.hrad_doubles(nz - 1, nmaps) * 8 == 98232 > 64 * 1024
    eng.dispersion_begin_radial(vsv, vsh, depz, R.MINTHK, nmaps, nmaps)
    runs(eng, waves)
    pv = eng.dispersion_fetch(0, nmaps, False, 0)
    obs = np.where(pv > 0, pv * 1.01, 3.0).astype(F)
    got, after, _ = against_host(h, hs, eng, vsv, vsh, depz, obs, None, ARGS, love, nmaps)
    assert (got["flag"][~RING] == 0).all() and not got["flag"][RING].any()
    assert np.abs(got["dv_sv"][:, ~RING]).max() > 0 and np.abs(got["dv_sh"][:, ~RING]).max() > 0
    assert np.isfinite(after[0]).all() and np.isfinite(after[1]).all()
    print("nz 64, K 60: roots %d of %d, data used %d Rayleigh and %d Love, largest |dv| %.4f and %.4f km/s" %
          (int((pv[:, ~RING] > 0).sum()), 9 * nmaps, int(got["nused"][0].sum()), int(got["nused"][1].sum()), np.abs(got["dv_sv"]).max(), np.abs(got["dv_sh"]).max()))


def test_the_driver_end_to_end(eng, tmp_path):
    """depth.run_radial on the Taipei example's grid and model (18 x 18 x 9) with its 26 periods dealt out over the four wave types: the
    observations are the device's curves of a truth whose Vsh is 5 % above the input's model at mid depth; both models start as the input's.
    The Love misfit falls, Vsh rises above Vsv where the truth has it, and the two files hold the engine's models and the steps' figures."""
    from dsurftomo_amd import depth, io
    c = io.load()
    t = np.asarray(c["tRc"], np.float64)
    c = dict(c, tRc=t[:7], tRg=t[7:14], tLc=t[14:20], tLg=t[20:])
    depth.check_radial(c)
    plan = depth.slot_plan(c)
    kmax, nx, ny, nz = c["kmax"], c["nx"], c["ny"], c["nz"]
    start = np.ascontiguousarray(np.asarray(c["vels"], F).transpose(2, 1, 0))
    eng.dispersion_begin_radial(start, RR.truth_vsh(start, 0.05), c["depz"], c["minthk"], kmax, kmax)
    for wave, kind, tt, first in plan:
        eng.dispersion_run(wave, kind, tt, False, 0, first)
    obs = eng.dispersion_fetch(0, kmax).astype(F)
    lines = []
    out, path, fit = depth.run_radial(eng, c, plan, obs, None, 3, 0.2, 0.05, depth.DEFAULT_ANISO, 0.3, str(tmp_path), lines.append)
    print("\n".join(lines))
    hist = out["history"]
    assert len(hist) == 3 and hist[-1]["rms_l"] < 0.5 * hist[0]["rms_l"] and hist[-1]["chi2"] < hist[0]["chi2"]
    assert hist[0]["nused_r"] + hist[0]["nused_l"] == int((obs.reshape(kmax, ny, nx)[:, 1:-1, 1:-1] > 0).sum())
    assert out["xi"] is not None and 1.0 < out["xi"][0] < 1.1025 and any("xi" in ln and "median" in ln for ln in lines)
    rows = depth.read_radial(path)
    assert [r["vsv"] for r in rows] == out["vsv"].ravel().astype(np.float64).tolist() and [r["vsh"] for r in rows] == out["vsh"].ravel().astype(np.float64).tolist()
    rows = depth.read_radial_fit(fit)
    assert [r["nused_l"] for r in rows] == out["steps"][-1]["nused"][1].tolist() and [r["flag"] for r in rows] == out["steps"][-1]["flag"].tolist()
    assert same_bits(out["vsv"][nz - 1], start[nz - 1]) and same_bits(out["vsh"][nz - 1], start[nz - 1])


def test_refusals(eng):
    """a radial step on a plain stage; a plain step, the resolution, get_model and kernels_from_dispersion on a radial stage; a bad aniso; a
    second step without new runs -- the code of each, and the engine usable after each"""
    nz = 3
    depz, vsv, rng, wt = case("smooth", nz)
    vsh = above(vsv)
    obs = np.full((K, NCOL), 3.0, F)
    plain_args = (R.SMOOTH, R.DAMP, R.DVMAX, R.MINVEL, R.MAXVEL)

    def refused(call, match, code):
        with pytest.raises(EngineError, match=match) as exc:
            call()
        assert exc.value.code == code

    def usable():
        """a good step on the stage as the refusal left it, then the stage as it was before"""
        out = eng.columns_step_radial(obs, wt, *ARGS)
        assert (out["flag"][~RING & (wt > 0).any(axis=0)] == 0).all()
        eng.dispersion_begin_radial(vsv, vsh, depz, R.MINTHK, K, K)
        runs(eng)

    eng.dispersion_begin(vsv, depz, R.MINTHK, K, K)
    runs(eng)
    refused(lambda: eng.columns_step_radial(obs, None, *ARGS), "not radial", DSA_ERR_STATE)
    refused(lambda: eng.dispersion_get_model_radial(), "not radial", DSA_ERR_STATE)
    assert (eng.columns_step(obs, None, *plain_args)["flag"][~RING] == 0).all()    # the plain stage is as usable as before
    eng.dispersion_begin_radial(vsv, vsh, depz, R.MINTHK, K, K)
    refused(lambda: eng.columns_step_radial(obs, None, *ARGS), "has not been run", DSA_ERR_STATE)       # no runs since begin
    runs(eng)
    refused(lambda: eng.columns_step(obs, None, *plain_args), "is radial", DSA_ERR_STATE)
    usable()
    refused(lambda: eng.columns_resolution(obs, None, R.SMOOTH, R.DAMP), "is radial", DSA_ERR_STATE)
    usable()
    refused(lambda: eng.dispersion_get_model(), "is radial", DSA_ERR_STATE)
    usable()
    refused(lambda: eng.kernels_from_dispersion(), "is radial", DSA_ERR_STATE)
    usable()
    for bad in (-0.1, np.nan, np.inf):
        refused(lambda: eng.columns_step_radial(obs, None, R.SMOOTH, R.DAMP, bad, R.DVMAX, R.MINVEL, R.MAXVEL), "aniso", DSA_ERR_ARGUMENT)
    refused(lambda: eng.columns_step_radial(obs, None, R.SMOOTH, 0.0, RR.ANISO, R.DVMAX, R.MINVEL, R.MAXVEL), "damp", DSA_ERR_ARGUMENT)
    refused(lambda: eng.columns_step_radial(obs[:K - 1], None, *ARGS), "maps given", DSA_ERR_ARGUMENT)
    models = eng.dispersion_get_model_radial()
    assert same_bits(models[0], eng.dispersion_get_model_radial()[0])
    out = eng.columns_step_radial(obs, wt, *ARGS)                                  # the refusals left the runs fresh
    assert (out["flag"][~RING & (wt > 0).any(axis=0)] == 0).all()
    refused(lambda: eng.columns_step_radial(obs, wt, *ARGS), "has not been run", DSA_ERR_STATE)          # a second step without new runs
    runs(eng)
    usable()
    # either pointer of get_model_radial may be NULL, through the library itself
    import ctypes as C
    one = np.zeros((nz, NY, NX), F)
    assert eng._L.dsa_dispersion_get_model_radial(eng._h, None, one.ctypes.data_as(C.c_void_p)) == 0
    assert same_bits(one, eng.dispersion_get_model_radial()[1])
    assert eng._L.dsa_dispersion_get_model_radial(eng._h, None, None) == 0
    # any other begin ends the radial stage
    eng.dispersion_begin(vsv, depz, R.MINTHK, K, K)
    runs(eng)
    assert same_bits(eng.dispersion_get_model(), vsv)
    assert (eng.columns_step(obs, None, *plain_args)["flag"][~RING] == 0).all()
