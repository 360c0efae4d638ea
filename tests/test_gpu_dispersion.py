"""Every variant of the device dispersion stage (csrc/disp_kernels.hip k_dispersion, Engine::dispersion_run) against each
other and against the oracle's depthkernel / caldespersion (CalSurfG.f90:1-169, :2866-2927).

dispersion_run picks a variant from the input's size:
  - the layer tables of a wavefront's curves sit in LDS when rmax <= 64 sublayers (64 curves x 4 arrays x rmax x 4 B <= 64 KB),
    else in global scratch with stride nlanes;
  - in LDS, 2^gshift lanes share one curve: gshift 3 up to 4 096 curves, 2 up to 32 768, 0 beyond; 0 in global scratch.
The options disp_layers_lds (-1 auto, 0, 1) and disp_group_shift (-1 auto, 0..3) force them.  gshift only changes which lane
forms each layer matrix, not the order of the product chain (dispersion_core.h, dltar1 / dltar4), so every variant gives the
same bits.

Against the oracle the only source of difference is the device's sin / cos / exp against libm's (test_gpu_boundary.py; the CPU
build of the same code is bit-exact, test_hostcheck.py).  The roots are rounded to fp32 (surfdisp96's c is real), so:
  - every phase / group velocity equals the oracle's or lies one fp32 ulp from it, and the failed roots (0) are the same;
  - a depth kernel is (cg(+) - cg(-)) / (0.01 base_q(i)), two roots of the same size as pv, each at most one ulp off: it lies
    within 2 ulp32(pv) / (0.01 base_q(i)) of the oracle's.
"""
import ctypes as C

import numpy as np
import pytest

import _libs as L
import parity_log
from dispersion_cases import EDGE_T, NATURAL, depths, edge_model, layer_count, smooth_model      # noqa: F401
from dsurftomo_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

F = np.float32
WAVES = [(2, 0), (2, 1), (1, 0), (1, 1)]                  # Rayleigh phase / group, Love phase / group


def diagnostics(e):
    fn = e._L.dsa_dispersion_diagnostics
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    count, first, period = C.c_longlong(0), (C.c_int * 5)(), C.c_double(0.0)
    assert fn(e._h, C.byref(count), first, C.byref(period)) == 0
    return count.value, list(first), period.value


def device(e, vel, depz, minthk, iwave, igr, t, kernels, lds=-1, gshift=-1):
    e.set_option("disp_layers_lds", lds)
    e.set_option("disp_group_shift", gshift)
    e.dispersion_begin(vel, depz, minthk, len(t), len(t))
    e.dispersion_run(iwave, igr, t, kernels, 0, 0)
    out = e.dispersion_fetch(0, len(t), kernels, 0)
    return out if kernels else (out,)


def expected_variant(ncol, nz, rmax, kernels):
    """Engine::dispersion_run's automatic choice: (layer tables in LDS, gshift)"""
    nlanes = ncol * (1 + 6 * nz if kernels else 1)
    lds = rmax * 1024 <= 64 * 1024
    return lds, (0 if not lds else 3 if nlanes <= 4096 else 2 if nlanes <= 32768 else 0)


def against_oracle(dev, ref, vel, name):
    """the bounds of the module docstring; the measured differences go to the parity report"""
    pv_d, pv_o = dev[0], ref[0]
    assert ((pv_d == 0) == (pv_o == 0)).all(), "%s: failed roots differ" % name
    ulp = lambda a: np.spacing(np.abs(a).astype(F)).astype(np.float64)
    dpv = np.abs(pv_d - pv_o)
    assert (dpv <= np.maximum(ulp(pv_o), ulp(pv_d))).all(), "%s: pv off by more than one fp32 ulp: %.3g" % (name, dpv.max())
    line = "dispersion %s: %d roots (%d failed), pv differing %d (max %.3g = %.2f ulp)" % (
        name, pv_o.size, int((pv_o == 0).sum()), int((dpv > 0).sum()), dpv.max(), (dpv / np.maximum(ulp(pv_o), 1e-300)).max())
    if len(dev) > 1:
        nz = vel.shape[0]
        vs = vel.reshape(nz, -1).astype(F)
        vp, rho = L.brocher(vs)
        # ulp32 of the roots behind a kernel: pv's, 0.5 % above it (a perturbed root may sit in the next binade); where the model's
        # own root failed, the largest root of the column stands in for the perturbed ones
        top = np.where(pv_o != 0, np.abs(pv_o), np.abs(pv_o).max(axis=0)[None, :])
        u = ulp(top * 1.005)
        worst = []
        for q, (a, b, base) in enumerate(zip(dev[1:], ref[1:], (vs, vp, rho))):
            den = (F(0.01) * base).astype(np.float64)[:, None, :]                  # (nz, 1, ncol), as k_depth_kernels divides
            bound = 2.0 * u[None, :, :] / den
            d = np.abs(a - b)
            assert (d <= bound).all(), "%s: %s kernel off by %.3g (bound %.3g)" % (name, "vs vp rho".split()[q], d.max(), bound[d > bound].min())
            worst.append("%s %d differ (max %.3g, %.2f of the bound)" % ("vs vp rho".split()[q], int((d > 0).sum()), d.max(), (d / bound).max()))
        line += "; kernels: " + ", ".join(worst)
    parity_log.add(line)


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


# ---- B1: every variant on one model, bit for bit, and against the oracle ------------------------------------------------------------

VARIANTS = [(1, 0), (1, 1), (1, 2), (1, 3), (0, -1), (0, 3), (-1, -1)]      # (disp_layers_lds, disp_group_shift)


@pytest.mark.parametrize("iwave,igr", WAVES)
def test_every_variant_gives_the_same_bits(eng, iwave, igr):
    """24 columns x 12 depths (rmax 45: the tables fit LDS), depth kernels (1 752 curves), 11 periods from 0.02 s to 1 000 s,
    with the edge cases of edge_model: LDS with gshift 0, 1, 2, 3; global scratch (gshift 0, also when 3 is asked for); the
    automatic choice (LDS, gshift 3).  pv and all three kernels equal across the variants, bit for bit; then the oracle."""
    nx, ny, nz, minthk = 6, 4, 12, 3.0
    vel, depz = edge_model(nx, ny, nz), depths(nz)
    assert layer_count(depz, minthk) == 45 and expected_variant(nx * ny, nz, 45, True) == (True, 3)
    outs = [device(eng, vel, depz, minthk, iwave, igr, EDGE_T, True, lds, g) for lds, g in VARIANTS]
    for (lds, g), out in zip(VARIANTS[1:], outs[1:]):
        for q, (a, b) in enumerate(zip(out, outs[0])):
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), "lds %d gshift %d: %s differs from lds 1 gshift 0" % (lds, g, "pv vs vp rho".split()[q])
    ref = L.depthkernel("oracle", vel, depz, minthk, iwave, igr, EDGE_T)
    assert (ref[0] == 0).any() if iwave == 1 else True                          # Love: the no-contrast columns fail at long periods
    against_oracle(outs[0], ref, vel, "variants iwave %d igr %d" % (iwave, igr))


# ---- B3: natural sizes, the automatic choice ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(NATURAL))
def test_natural_sizes_against_the_oracle(eng, name):
    """no option forced: both sides of the LDS rule (rmax 64 / 65, computed with make_layer_geom's fp32 formula), more than
    32 768 curves (gshift 0), at most 4 096 (gshift 3), in between (gshift 2), nz = 64 (rmax 127, global), nper = 60"""
    nx, ny, nz, minthk, model, t, kernels, iwave, igr, rmax, variant = NATURAL[name]
    vel, depz = model(nx, ny, nz), depths(nz)
    assert layer_count(depz, minthk) == rmax and expected_variant(nx * ny, nz, rmax, kernels) == variant
    dev = device(eng, vel, depz, minthk, iwave, igr, t, kernels)
    ref = L.depthkernel("oracle", vel, depz, minthk, iwave, igr, t, kernels)
    against_oracle(dev, ref if kernels else (ref,), vel, "%s (rmax %d, %s, gshift %d)" % (name, rmax, "LDS" if variant[0] else "global", variant[1]))


# ---- B4: failure bookkeeping -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("iwave,igr", WAVES)
def test_failure_count_and_first_failure(eng, iwave, igr):
    """caldespersion (no kernels): dsa_dispersion_diagnostics counts one failure per failed curve = per oracle column with a zero
    in pv, and reports the first in the reference's call order (column by column): its column and the period of its first zero"""
    nx, ny, nz, minthk = 6, 4, 12, 3.0
    vel, depz = edge_model(nx, ny, nz), depths(nz)
    t = EDGE_T[:10]                                                             # (at 1 000 s every Love curve fails)
    ref = L.depthkernel("oracle", vel, depz, minthk, iwave, igr, t, kernels=False)
    device(eng, vel, depz, minthk, iwave, igr, t, False)
    count, first, period = diagnostics(eng)
    failed = np.flatnonzero((ref == 0).any(axis=0))
    assert failed.size > 0 and failed.size < nx * ny
    assert count == failed.size
    c0 = int(failed[0])
    k0 = int(np.flatnonzero(ref[:, c0] == 0)[0])
    assert first == [iwave, igr, c0 + 1, 0, k0 + 1] and period == t[k0]


def test_limits_are_refused_by_the_engine(eng):
    """past the limits of the layer tables and the period arrays the engine refuses the call (argument errors, no kernel
    launched), and the same engine still runs a valid call afterwards"""
    ok_vel, ok_depz = edge_model(2, 2, 7), depths(7)
    with pytest.raises(EngineError, match="bad arguments"):
        eng.dispersion_begin(edge_model(2, 2, 65), depths(65), 1.0, 1, 1)                     # nz = 65
    assert layer_count(depths(64), 3.0) > 200
    with pytest.raises(EngineError, match="exceeds 200 layers"):
        eng.dispersion_begin(edge_model(2, 2, 64), depths(64), 3.0, 1, 1)                     # 253 sublayers
    eng.dispersion_begin(ok_vel, ok_depz, 1.0, 61, 61)
    with pytest.raises(EngineError, match="bad arguments"):
        eng.dispersion_run(2, 0, np.geomspace(1.0, 100.0, 61), False, 0, 0)                     # nper = 61
    t = np.array([5.0, 20.0])
    dev = device(eng, ok_vel, ok_depz, 1.0, 2, 0, t, False)[0]
    ref = L.depthkernel("oracle", ok_vel, ok_depz, 1.0, 2, 0, t, kernels=False)
    against_oracle((dev,), (ref,), ok_vel, "after refused calls")
