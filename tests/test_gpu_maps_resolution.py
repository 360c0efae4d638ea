"""dsa_maps_resolution (csrc/map_kernels.hip) on the device against the CPU build of the same header
(tests/hostcheck_map_resolution.cpp through map_resolution_ref), bit for bit: every figure is one sequential fp64 chain under
-ffp-contract=off, without square root and with IEEE division, and the device's right-looking panels subtract the products of the header's
left-looking loop in its order -- so neither the thread mapping nor the panels can show.

The systems are map_resolution_ref.SYSTEMS through dsa_spmv_load (n_m = 20 .. 192: below, at and across the panel width) and, end to end,
the 35 x 35 fixture of tests/test_gpu_maps.py (2 maps of n_m = 1089, 576 rays) through dsa_iteration_system_maps_device."""
import time

import numpy as np
import pytest

import map_resolution_ref as MR
import synth
import test_gpu_azimuthal as TA
import test_gpu_maps as TM
from dsurftomo_amd import maps as M
from dsurftomo_amd.analyses.azimuthal import azimuthal_weights
from dsurftomo_amd.analyses.common import LSMR_ARGS
from dsurftomo_amd.engine import Engine, EngineError
from map_resolution_ref import DAMP, SYSTEMS, same_bits

pytestmark = pytest.mark.gpu

F = np.float32
SEED = 11
DSA_ERR_ARGUMENT, DSA_ERR_STATE, DSA_ERR_CAPACITY = -2, -5, -6                   # include/dsurftomo_amd.h
FIGURES = ("measures", "leverage", "trace", "nused", "flag")


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def h():
    return MR.load()


def n_m(sy):
    return sy[3] * (sy[0] - 2) * (sy[1] - 2)


def shape(S):
    return S["nx"], S["ny"], S["nmaps"], S["nblocks"], S["ndata"]


def load(e, S):
    e.spmv_load(S["m"], S["n"], S["rw"], S["row"], S["col"])


def against_host(h, e, S, damp=DAMP):
    """every output of the device, with R for each map and without, against the host's: bit for bit.  Returns the device's (r_map = -1)."""
    lean = e.maps_resolution(*shape(S), damp)
    assert "R" not in lean
    for k in range(S["nmaps"]):
        rc, want = MR.host_resolution(h, S, damp, k)
        got = e.maps_resolution(*shape(S), damp, r_map=k)
        assert rc == 0
        for name in FIGURES + ("R",):
            assert same_bits(got[name], want[name]), "%s differs from the host's (%d of %d), r_map %d" % (name, int((got[name] != want[name]).sum()), got[name].size, k)
        for name in FIGURES:
            assert same_bits(lean[name], got[name]), "%s changes when R is asked for" % name
    return lean


@pytest.mark.parametrize("sy", SYSTEMS, ids=lambda sy: "nm%d" % n_m(sy))
def test_resolution_equals_the_host_bit_for_bit(eng, h, sy):
    """1: every output and the R of every map; again under a memory budget that holds one map per group"""
    S = MR.system(*sy, SEED)
    load(eng, S)
    got = against_host(h, eng, S)
    assert (got["flag"][:2] == 0).all() and (got["trace"][:, :2] > 0).all() and np.isfinite(got["measures"]).all()
    if sy[2] == 3:
        assert got["flag"][2] == 2 and not got["measures"][:, :, 2].any()
    nm = n_m(sy)
    one = 8 * (2 * nm * nm + int(got["nused"].max()) * nm + nm)
    eng.set_memory_budget(one)
    try:
        split = eng.maps_resolution(*shape(S), DAMP, r_map=1)
    finally:
        eng.set_memory_budget(0)
    whole = eng.maps_resolution(*shape(S), DAMP, r_map=1)
    for name in FIGURES + ("R",):
        assert same_bits(split[name], whole[name]), name
        if name != "R":
            assert same_bits(split[name], got[name]), name


def test_end_to_end_on_the_35_fixture(h):
    """2: solve_rows_maps_device -> iteration_system_maps_device -> maps_resolution equals the header on the NumPy route's COO of the same
    rows, bit for bit: 2 maps of 1089 unknowns, 576 rays"""
    NX, NMAPS = TM.NX, TM.NMAPS
    e, u = TM.fresh()
    try:
        dsyn, rw, iw, col = e.solve_rows_maps(TA.capacity(u), False)
        r = synth.LCG(91)
        obst = (dsyn * (1.0 + 0.04 * (r.uniform(dsyn.size) - 0.5))).astype(F)
        threshold0, weight0, damp = F(1.2), F(2.0), 0.5
        t, nar = e.solve_rows_maps_device(False)
        D = e.iteration_system_maps_device(NX, NX, NMAPS, 1, obst, dsyn, threshold0, weight0, weight0)
        t0 = time.perf_counter()
        got = e.maps_resolution(NX, NX, NMAPS, 1, dsyn.size, damp, r_map=1)
        t1 = time.perf_counter()
        again = e.maps_resolution(NX, NX, NMAPS, 1, dsyn.size, damp, r_map=1)
        t2 = time.perf_counter()
    finally:
        e.close()
    res = (obst - dsyn).astype(F)
    dw = azimuthal_weights(res, threshold0)
    S = M.map_system(NX, NX, NMAPS, 1, rw, iw, col, res, dw, weight0, weight0)
    S.update(nx=NX, ny=NX, nmaps=NMAPS, nblocks=1, ndata=dsyn.size)
    assert D["m"] == S["m"] and D["nar"] == S["rw"].size
    t3 = time.perf_counter()
    rc, want = MR.host_resolution(h, S, damp, 1)
    t4 = time.perf_counter()
    print("35 x 35, 2 maps of 1089 unknowns, %d data (%s used): the first call %.3f s, the second %.3f s, the host %.3f s; trace %s, median R_qq %.4f, median var %.4g, largest leverage %.4f" %
          (dsyn.size, got["nused"].tolist(), t1 - t0, t2 - t1, t4 - t3, got["trace"].ravel().tolist(), float(np.median(got["measures"][0])),
           float(np.median(got["measures"][1])), float(got["leverage"].max())))
    assert rc == 0
    for name in FIGURES + ("R",):
        assert same_bits(got[name], want[name]), "%s differs from the host's (%d of %d)" % (name, int((got[name] != want[name]).sum()), got[name].size)
        assert same_bits(got[name], again[name]), name
    assert (got["flag"] == 0).all() and int(got["nused"].sum()) == int((dw > 0).sum()) > 0
    assert (got["measures"][0] > -1e-12).all() and (got["measures"][0] < 1).all() and (got["trace"] > 1).all()


def test_the_call_is_read_only(eng, h):
    """3: dsa_lsmr's x before and after the call has the same bits; a second call repeats the first, and so does a call right after a
    fresh load (it builds the contiguous copies itself)"""
    S = MR.system(*SYSTEMS[4], SEED)
    load(eng, S)
    before = eng.lsmr(S["b"], DAMP, *LSMR_ARGS)
    first = eng.maps_resolution(*shape(S), DAMP, r_map=0)
    after = eng.lsmr(S["b"], DAMP, *LSMR_ARGS)
    assert same_bits(before["x"], after["x"]) and before["itn"] == after["itn"] > 3 and before["x"].any()
    second = eng.maps_resolution(*shape(S), DAMP, r_map=0)
    for name in first:
        assert same_bits(first[name], second[name]), name
    load(eng, S)                                                                   # a fresh load: the call builds the contiguous copies itself
    third = eng.maps_resolution(*shape(S), DAMP, r_map=0)
    for name in first:
        assert same_bits(first[name], third[name]), name
    assert same_bits(eng.lsmr(S["b"], DAMP, *LSMR_ARGS)["x"], before["x"])


def test_three_spikes_of_the_iterative_route(eng):
    """4: dsa_resolution_blocks' fp32 LSMR answers to three unit spikes against the dense R columns of the same system: printed and
    recorded in DESIGN.md section 36, nothing asserted on the difference (an iterative fp32 answer)"""
    S = MR.system(*SYSTEMS[4], SEED)
    nx, ny, nmaps, nblocks, ndata = shape(S)
    layer = (nx - 2) * (ny - 2)
    load(eng, S)
    dense = eng.maps_resolution(*shape(S), DAMP, r_map=0)
    first = 20
    coords = np.random.default_rng(3).random((nmaps * layer, 3))
    it = eng.lsmr_resolution_blocks(ndata, DAMP, nblocks, (first, 3), coords, atol=1e-6, btol=1e-6, conlim=100.0, itnlim=400, local_size=10)
    cols = np.concatenate([np.arange(B * nmaps * layer, B * nmaps * layer + layer) for B in range(nblocks)])          # map 0's unknowns
    worst = 0.0
    for r in range(3):
        q = first + r                                                              # plane 0 of map 0: the local index is the column
        worst = max(worst, float(np.abs(it["x"][r][cols].astype(np.float64) - dense["R"][:, q]).max()))
    print("three spikes: largest |x_lsmr - R column| %.3g (largest |R| %.3g; itn %s, istop %s)" % (worst, np.abs(dense["R"]).max(), it["itn"].tolist(), it["istop"].tolist()))
    assert np.isfinite(worst)


def test_refusals(eng, h):
    """5: every refusal the public interface reaches, the engine usable after each"""
    S = MR.system(*SYSTEMS[0], SEED)
    nx, ny, nmaps, nblocks, ndata = shape(S)
    rc, want = MR.host_resolution(h, S, DAMP)
    codes = []

    def refused(match, code, *args, on=eng, **kw):
        with pytest.raises(EngineError, match=match) as exc:
            on.maps_resolution(*args, **kw)
        assert exc.value.code == code, exc.value
        codes.append(code)

    def usable():
        got = eng.maps_resolution(nx, ny, nmaps, nblocks, ndata, DAMP)
        for name in FIGURES:
            assert same_bits(got[name], want[name]), name

    fresh = Engine(0)
    try:
        refused("no matrix", DSA_ERR_STATE, nx, ny, nmaps, nblocks, ndata, DAMP, on=fresh)
    finally:
        fresh.close()
    load(eng, S)
    usable()
    for bad in ((2, ny, nmaps, nblocks, ndata, DAMP), (nx, 2, nmaps, nblocks, ndata, DAMP), (nx, ny, 0, nblocks, ndata, DAMP), (nx, ny, nmaps, 2, ndata, DAMP)):
        refused("nx and ny", DSA_ERR_ARGUMENT, *bad)
    refused("unknowns", DSA_ERR_ARGUMENT, nx + 1, ny, nmaps, nblocks, ndata, DAMP)
    refused("unknowns", DSA_ERR_ARGUMENT, nx, ny, nmaps, 3, ndata, DAMP)
    refused("ndata", DSA_ERR_ARGUMENT, nx, ny, nmaps, nblocks, 0, DAMP)
    refused("ndata", DSA_ERR_ARGUMENT, nx, ny, nmaps, nblocks, S["m"] + 1, DAMP)
    for bad in (-0.1, np.nan, np.inf):
        refused("damp", DSA_ERR_ARGUMENT, nx, ny, nmaps, nblocks, ndata, bad)
    refused("r_map", DSA_ERR_ARGUMENT, nx, ny, nmaps, nblocks, ndata, DAMP, r_map=nmaps)
    usable()
    # R and r_map disagreeing, and a NULL measures: through the library itself, the binding always passes them consistently
    import ctypes as C
    lib = eng._L
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    meas, R = np.zeros(9 * S["n"]), np.zeros((20, 20))
    assert lib.dsa_maps_resolution(eng._h, nx, ny, nmaps, nblocks, ndata, DAMP, -1, p(meas), None, None, None, None, p(R)) == DSA_ERR_ARGUMENT
    assert b"disagree" in lib.dsa_error_string(eng._h)
    assert lib.dsa_maps_resolution(eng._h, nx, ny, nmaps, nblocks, ndata, DAMP, 0, p(meas), None, None, None, None, None) == DSA_ERR_ARGUMENT
    assert lib.dsa_maps_resolution(eng._h, nx, ny, nmaps, nblocks, ndata, DAMP, -1, None, None, None, None, None, None) == DSA_ERR_ARGUMENT
    assert lib.dsa_maps_resolution(eng._h, nx, ny, nmaps, nblocks, ndata, DAMP, -1, p(meas), None, None, None, None, None) == 0       # only measures
    assert same_bits(meas.reshape(want["measures"].shape), want["measures"])
    usable()
    # the memory budget: below the factor and R of one map (before the device is touched), then below one map with its T
    eng.set_memory_budget(1000)
    try:
        refused("memory budget", DSA_ERR_CAPACITY, nx, ny, nmaps, nblocks, ndata, DAMP)
        eng.set_memory_budget(8 * (2 * 400 + 2 * 20) + 8)
        refused("memory budget", DSA_ERR_CAPACITY, nx, ny, nmaps, nblocks, ndata, DAMP)
    finally:
        eng.set_memory_budget(0)
    usable()
    # the structure of the rows
    col = S["col"].copy(); col[0] += 20
    eng.spmv_load(S["m"], S["n"], S["rw"], S["row"], col)
    refused("two maps", DSA_ERR_ARGUMENT, nx, ny, nmaps, nblocks, ndata, DAMP)
    col = S["col"].copy(); col[1] = col[0]
    eng.spmv_load(S["m"], S["n"], S["rw"], S["row"], col)
    refused("twice", DSA_ERR_ARGUMENT, nx, ny, nmaps, nblocks, ndata, DAMP)
    order = np.arange(S["rw"].size)[::-1]
    eng.spmv_load(S["m"], S["n"], S["rw"][order], S["row"][order], S["col"][order])
    refused("row order", DSA_ERR_ARGUMENT, nx, ny, nmaps, nblocks, ndata, DAMP)
    load(eng, S)
    usable()
    assert len(codes) == 18
