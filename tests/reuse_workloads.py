"""Workloads of tests/test_gpu_engine_reuse.py: every family of entry points of the engine as one self-contained call sequence, in two
shapes, so that any of them can follow any other on one engine.

A workload is run(name, shape, engine) -> dict[str, ndarray].  It takes an engine in an unknown state and states everything it depends on
itself: its maps, its plan, its stage (dispersion_begin*), its depth kernels, its matrix (spmv_load), the azimuthal slot mask where it emits
azimuthal rows (also when that is "all on"), keep_fields.  Options are sticky by design and not under test: an engine is handed over with
every option at its default (DEFAULTS), and a workload leaves a default only inside `options`, which puts it back.  It returns every array
the calls hand back, and asserts that the result is not vacuous (rows present, an LSMR member with itn > 3, a flagged and marched unit in
the default-mode solve, accepted and rejected proposals in the sampler).

`small` is in every dimension -- vertices of the grid, nz, maps or periods, units, members, matrix size -- at most `big` and in at least one
smaller, and its grid has another aspect; both are the smallest shapes at which the kernels still take their distinct paths (two lane
groups of 64 members in `big`, one partial group in `small`; three blocks of map unknowns against one; two models against one ...).

The inputs are built once per (name, shape) on the CPU and kept; run() makes engine calls only.  Data a step needs from the device (the
observations of an inversion step are the step's own synthetic times, perturbed by fixed factors) are computed from what the engine
returned, so they are part of what is compared.

dsa_forward_models and dsa_forward_steps exist at the drop-in level only, on the process-wide engine; `forward_models` and `forward_steps`
here are the engine-level calls those two make (dispersion_begin_models, the runs without kernels, maps_from_dispersion, the model-major
plan, solve; step_models on the solutions a trade-off batch left resident).  The drop-in entries themselves are in the boundary test.

Data and plain functions only: no pytest, no fixtures.  Nothing under dsurftomo_amd/ imports this module."""
import contextlib
import ctypes as C
import functools

import numpy as np

import _libs as L
import column_lateral_ref as IR
import column_radial_lateral_ref as LR
import column_radial_ref as RR
import columns_ref as R
import solve_units
import synth
import synth_matrix as SM
from conftest import PRODUCT_DEFAULTS
from dsurftomo_amd import maps as M, radial as RD
from dsurftomo_amd.analyses.common import LSMR_ARGS, _p, unknown_coords
from dsurftomo_amd.engine import EngineError

F = np.float32
DSA_ERR_STATE, DSA_ERR_CAPACITY = -5, -6                                                     # include/dsurftomo_amd.h

# every option a workload here may touch, at the product's default: conftest's list and the ones outside it
DEFAULTS = dict(PRODUCT_DEFAULTS, disp_layers_lds=-1, disp_group_shift=-1, lsmr_device_vectors=0, rows_on_device=0, ray_path_cap=0, ray_budget=0)

SHAPES = ("big", "small")
NAMES = ("times_default", "times_exact", "times_bundled", "rows", "rows_capacity_refused", "azimuthal_device", "maps_loop", "direct_iteration",
         "radial_direct", "radial_step_rows", "columns_plain", "columns_radial", "columns_lateral", "columns_radial_lateral", "columns_sample", "forward_models",
         "forward_steps", "lsmr_family")


@contextlib.contextmanager
def options(e, **values):
    """the options `values` for the block, their defaults afterwards -- also when the block raises"""
    try:
        for k, v in values.items():
            e.set_option(k, v)
        yield
    finally:
        for k in values:
            e.set_option(k, DEFAULTS[k])


def pack(prefix, d, out):
    """the arrays and numbers of the (nested) dict d into out under prefix.key, every one as an ndarray"""
    for k, v in d.items():
        if isinstance(v, dict):
            pack("%s.%s" % (prefix, k), v, out)
        elif v is not None:
            out["%s.%s" % (prefix, k)] = np.ascontiguousarray(v)
    return out


def factors(n, seed):
    """n fixed factors within 2 % of 1: what turns a step's synthetic times into its observations"""
    return (1.0 + 0.04 * (SM.mix(np.arange(n), seed) - 0.5)).astype(F)


# ---- travel times on given maps ------------------------------------------------------------------------------------------------------------

# Sources that meet ties, so that the default mode's census flags a unit and the march solves it again; which units are flagged depends on
# the receivers too, so sources and receivers are drawn in one fixed order.  On 257 x 121 nodes: nodes of the grid; the census flags three
# units of the `wild` medium, one of them above its threshold, which makes the map tie-prone (csrc/engine.h tie_map_strict).  On 121 x 121:
# candidates of solve_units.candidates("121") at which tests/hostcheck.cpp's worklist solve of the `wild` medium ends evaluations on a tie
# (solve_units.tie_free), as fractions of the grid; none of their ties moves a node by more than the default tie_threshold, so times_default
# counts every tie there (tie_threshold = 0).
TIED_257 = ((5.0, 7.0), (128.0, 60.0), (16.0, 24.0), (248.0, 8.0), (8.5, 16.5), (24.0, 40.5))
TIED_121 = ((0.78019, 0.50466), (0.91561, 0.86479), (0.2294, 0.8), (0.39278, 0.10382), (0.10022, 0.33463), (0.83533, 0.08642))


@functools.lru_cache(maxsize=None)
def times_case(shape, kinds, scaled=0, nsrc=12, nrec=3):
    """maps of `kinds` (or `scaled` copies of the first, 2 % apart) on 35 x 18 vertices (big) or 18 x 18 (small), dicing 8; on every map
    the first nsrc of twelve sources -- six drawn off the nodes, then the six above -- with the first nrec of their three receivers"""
    nx, ny = (35, 18) if shape == "big" else (18, 18)
    geo = (nx, ny, synth.GOXD, synth.GOZD, synth.DVD, synth.DVD, 8)
    g = L.grid(*geo)
    pv = np.stack([solve_units.medium(nx, ny, k) for k in kinds])
    if scaled:
        pv = np.stack([pv[0] * (1.0 + 0.02 * p) for p in range(scaled)])
    nmaps = pv.shape[0]
    r = synth.LCG(41 + nx + 3 * ny)
    node = lambda n: np.stack([2.4 + r.uniform(n) * (g.nnx - 5.9), 2.4 + r.uniform(n) * (g.nnz - 5.9)], axis=1)
    rad = lambda p: ((F(g.gox) + p[:, 0].astype(F) * F(g.dnx)).astype(F), (F(g.goz) + p[:, 1].astype(F) * F(g.dnz)).astype(F))
    src = np.concatenate([node(6), TIED_257 if shape == "big" else [(fx * (g.nnx - 1), fz * (g.nnz - 1)) for fx, fz in TIED_121]])
    rec = node(3 * len(src)).reshape(len(src), 3, 2)
    sx, sz = rad(src[:nsrc])
    rx, rz = rad(rec[:nsrc, :nrec].reshape(-1, 2))
    u = dict(map_index=np.repeat(np.arange(nmaps, dtype=np.int32), nsrc), scx=np.tile(sx, nmaps), scz=np.tile(sz, nmaps),
             nrec=np.full(nsrc * nmaps, nrec, np.int32), rcx=np.tile(rx, nmaps), rcz=np.tile(rz, nmaps))
    return geo, pv, u


def solve_times(e, geo, pv, u):
    nx, ny, goxd, gozd, dvxd, dvzd, gd = geo
    e.set_maps(nx, ny, goxd, gozd, dvxd, dvzd, pv, dicing=gd)
    e.keep_fields(True)
    try:
        e.plan(u["map_index"], u["scx"], u["scz"], u["nrec"], u["rcx"], u["rcz"])
        out = dict(times=e.solve())
        fl, inf = e.unit_ties()
        out.update(tie_flags=fl, tie_influence=inf)
        n = len(u["map_index"])
        for k in sorted({0, n // 2, n - 1}):
            out["field%d" % k] = e.field(k)
    finally:
        e.keep_fields(False)
    assert out["times"].size == int(u["nrec"].sum()) > 0 and np.isfinite(out["times"]).all() and (out["times"] > 0).all()
    return out


MIXED = dict(big=("wild", "rough"), small=("wild",))          # the media of times_exact: two maps, one map


def times_default(e, shape):
    """the default mode (exact_ties = 1): the fixed point, the census, the march of the flagged units of the `wild` map"""
    geo, pv, u = times_case(shape, ("wild",), nsrc=10 if shape == "big" else 7)           # (up to the last source the census flags)
    with options(e, exact_ties=1, bundle=1, tie_threshold=DEFAULTS["tie_threshold"] if shape == "big" else 0.0):
        out = solve_times(e, geo, pv, u)
    assert ((out["tie_flags"] & 3) == 3).any(), "no unit was flagged and marched: flags %s" % out["tie_flags"].tolist()
    return out


def times_exact(e, shape):
    """every unit by the literal march (exact_ties = 2), whose contract is bit-exactness: four sources on two maps, three on one"""
    geo, pv, u = times_case(shape, MIXED[shape], nsrc=4 if shape == "big" else 3)
    with options(e, exact_ties=2):
        out = solve_times(e, geo, pv, u)
        n = len(u["map_index"])
        tr, sr = e.refined(n - 1)
        out["refined_s"], out["refined_t"] = sr, np.where(sr == 0, tr, F(0))      # (the snapshot is defined on the alive set: tests/test_gpu_geometry.py)
    assert ((out["tie_flags"] & 2) != 0).all()
    return out


def times_bundled(e, shape):
    """the bundle kernel forced (bundle = 4, exact_ties = 0: tests/test_gpu_geometry.py) on four scaled smooth maps, whose fixed point is
    unique: every source's four units are one bundle, coarse and refined"""
    geo, pv, u = times_case(shape, ("smooth",), scaled=4, nsrc=6 if shape == "big" else 3, nrec=2)
    with options(e, exact_ties=0, bundle=4, bundle_refined=1):
        out = solve_times(e, geo, pv, u)
        st = e.stats()
    nsrc = len(u["map_index"]) // 4
    assert st["bundle_size"] == 4 and st["bundles"] == nsrc and st["bundled_units"] == 4 * nsrc, st
    return out


# ---- the boundary case through the dispersion stage: what dsa_calsurfg does on its engine ----------------------------------------------------

@functools.lru_cache(maxsize=None)
def boundary(shape):
    """synth.boundary_case at its defaults (12 x 11 x 5, 8 periods) or 10 x 9 x 4 with 5 periods, fewer sources and receivers; with the
    numbers of an inversion step, the drop-in's layout (dropin.hip: make_layout, clobber) and its unit lists (make_units)"""
    c = synth.boundary_case() if shape == "big" else synth.boundary_case(nx=10, ny=9, nz=4, kRc=2, kRg=1, kLc=1, kLg=1, nsrc=3, nrcf=4)
    c.update(threshold0=F(1.2), weight0=F(2.0), damp=F(0.5), minvel=F(1.5), maxvel=F(5.5))
    kRc, kRg, kLc, kLg = c["kRc"], c["kRg"], c["kLc"], c["kLg"]
    lay = dict(oRc=0, oRg=max(kRc, kRg), sRc=0, sRg=kRc, sLc=kRc + kRg, sLg=kRc + kRg + kLc)
    lay["oLc"] = lay["oRg"] + kRg
    lay["oLg"] = lay["oLc"] + max(kLc, kLg)
    lay["nmaps"] = lay["oLg"] + kLg
    c["layout"] = lay
    c["units_rows"] = dropin_units(c, lay, True)
    c["units_times"] = dropin_units(c, lay, False)
    c["model"] = np.ascontiguousarray(np.asarray(c["vels"], F).transpose(2, 1, 0))          # (nz, ny, nx), as the engine takes it
    return c


def dropin_units(c, lay, rows):
    """dropin.hip's make_units: period slot outer, the slot's sources inner; with rows a group period has two units, its times on its own
    map and its rays on the phase map of that period"""
    mp, nr, mode, slot_of, first, sx, sz, rx, rz = [], [], [], [], [], [], [], [], []
    count = 0
    for slot in range(c["kmax"]):
        for s in range(int(c["nsrcsurf1"][slot])):
            wt, gr, per, n = int(c["wavetype"][s, slot]), int(c["igrt"][s, slot]), int(c["periods"][s, slot]), int(c["nrc1"][s, slot])
            phase = (lay["oRc"] if wt == 2 else lay["oLc"]) + per - 1
            mt = phase if gr == 0 else (lay["oRg"] if wt == 2 else lay["oLg"]) + per - 1
            for ig in range(2 if rows and gr == 1 else 1):
                mp.append(mt if ig == 0 else phase); nr.append(n); slot_of.append(slot); first.append(count)
                mode.append(1 if not rows else (3 if gr == 0 else (1 if ig == 0 else 2)))
                sx.append(c["scxf"][s, slot]); sz.append(c["sczf"][s, slot])
                rx.append(c["rcxf"][:n, s, slot]); rz.append(c["rczf"][:n, s, slot])
            count += n
    assert count == c["ndata"]
    return dict(map_index=np.array(mp, np.int32), scx=np.array(sx, F), scz=np.array(sz, F), nrec=np.array(nr, np.int32), rcx=np.concatenate(rx).astype(F),
                rcz=np.concatenate(rz).astype(F), mode=np.array(mode, np.int32), sen_slot=np.array(slot_of, np.int32), data_first=np.array(first, np.int32))


def dropin_runs(e, c, kernels):
    """the dispersion runs of dsa_calsurfg (kernels) or dsa_forward_models (none): the phase velocities at the group periods go over the
    head of the phase block"""
    lay, k = c["layout"], int(bool(kernels))
    e.dispersion_run(2, 0, c["tRc"], k, lay["sRc"] * k, lay["oRc"])
    if c["kRg"]:
        e.dispersion_run(2, 1, c["tRg"], k, lay["sRg"] * k, lay["oRg"])
        e.dispersion_run(2, 0, c["tRg"], False, 0, lay["oRc"])
    e.dispersion_run(1, 0, c["tLc"], k, lay["sLc"] * k, lay["oLc"])
    if c["kLg"]:
        e.dispersion_run(1, 1, c["tLg"], k, lay["sLg"] * k, lay["oLg"])
        e.dispersion_run(1, 0, c["tLg"], False, 0, lay["oLc"])


def stage_rows(e, c):
    """dsa_calsurfg up to its solve: the plain stage on the case's model, the runs with kernels, the maps, the depth factors, the plan"""
    u = c["units_rows"]
    e.dispersion_begin(c["model"], c["depz"], c["minthk"], c["kmax"], c["layout"]["nmaps"])
    dropin_runs(e, c, True)
    e.maps_from_dispersion(c["goxd"], c["gozd"], c["dvxd"], c["dvzd"], 8)
    e.kernels_from_dispersion()
    e.keep_fields(False)
    e.plan(u["map_index"], u["scx"], u["scz"], u["nrec"], u["rcx"], u["rcz"], mode=u["mode"], sen_slot=u["sen_slot"], data_first=u["data_first"])


def capacity(c, blocks=1):
    return blocks * c["ndata"] * c["nparpi"] + 1


PATH_CAP = 4096


def rows(e, shape):
    """host rows of the isotropic kind with the rays' paths"""
    c = boundary(shape)
    stage_rows(e, c)
    with options(e, ray_path_cap=PATH_CAP):
        t, rw, iw, col = e.solve_rows(capacity(c))
        paths = e.ray_paths(PATH_CAP)
    fl, inf = e.unit_ties()
    assert rw.size > 0 and len(paths) > 0 and np.isfinite(t).all() and (t > 0).all() and 1 <= iw.min() and iw.max() <= c["ndata"]
    return dict(times=t, rw=rw, iw=iw, col=col, tie_flags=fl, tie_influence=inf, path_datum=np.array([d for d, _ in paths], np.int32),
                path_n=np.array([len(p) for _, p in paths], np.int32), path_points=np.concatenate([p for _, p in paths]))


def rows_capacity_refused(e, shape):
    """workload `rows` with room for one entry: DSA_ERR_CAPACITY after rows were emitted.  The result is the code; the point is what it leaves"""
    c = boundary(shape)
    stage_rows(e, c)
    try:
        e.solve_rows(1)
    except EngineError as exc:
        assert exc.code == DSA_ERR_CAPACITY, exc
        return dict(code=np.array([exc.code], np.int32))
    raise AssertionError("solve_rows(1) was not refused")


def spikes_of(n, count):
    """(first, count): count unit spikes in the middle of n unknowns"""
    return (n // 2 - count // 2, count)


def azimuthal_device(e, shape):
    """azimuthal rows resident (kRowsAzimuthal), the joint system (kRowsJoint), its solve and a few block PSFs.  big: Rayleigh slots only,
    as dsa_calsurfg_azimuthal sets them; small: every slot, stated"""
    c = boundary(shape)
    nx, ny, nz, dall, maxvp = c["nx"], c["ny"], c["nz"], c["ndata"], c["nparpi"]
    on = np.ones(c["kmax"], np.int32)
    if shape == "big":
        on[c["layout"]["sLc"]:] = 0
    stage_rows(e, c)
    e.set_azimuthal_slots(on)                                             # (the mask is state like the plan: whoever emits azimuthal rows states it)
    dsyn, nnz = e.solve_rows_azimuthal_device(capacity(c, 3), host_copy=False)
    obst = (dsyn * factors(dall, 91)).astype(F)
    cbst = np.zeros(dall + 3 * maxvp, F); dw = np.zeros(dall, F); norm = np.zeros(3 * maxvp, F); dws = np.zeros(6, F)
    m, nar = C.c_int(0), C.c_longlong(0)
    e._check(e._L.dsa_iteration_system_azimuthal_device(e._h, nx, ny, nz, dall, _p(obst), _p(dsyn), c["threshold0"], c["weight0"], 0.5, _p(cbst), _p(dw),
                                                        _p(norm), C.byref(m), C.byref(nar), _p(dws)))
    e._mn = (m.value, 3 * maxvp)
    sol = e.lsmr(cbst, float(c["damp"]), *LSMR_ARGS)
    psf = e.lsmr_resolution_blocks(dall, float(c["damp"]), 3, spikes_of(3 * maxvp, 5 if shape == "big" else 3), unknown_coords(c))
    assert nnz > 0 and nar.value > nnz and sol["itn"] > 3 and sol["x"][maxvp:].any() and psf["x"].any()
    out = dict(times=dsyn, nnz=np.array([nnz, nar.value, m.value]), cbst=cbst, datweight=dw, norm=norm, dws=dws)
    pack("lsmr", sol, out)
    return pack("psf", psf, out)


def maps_loop(e, shape):
    """one iteration of dsurftomo_amd.maps from --start model: map rows resident (kRowsMaps), the map system (kRowsMapSystem), LSMR, the
    update of the resident maps and the plan again.  big: three blocks of unknowns per map (c0 | A1 | A2), small: one"""
    c = boundary(shape)
    azimuthal = shape == "big"
    nx, ny = c["nx"], c["ny"]
    u = period_plan_of(shape)
    nmaps, layer = u["nmaps"], (nx - 2) * (ny - 2)
    M.start_maps(e, c, u, "model")
    e.keep_fields(False)
    M.plan_engine(e, u)
    dsyn, nnz = e.solve_rows_maps_device(azimuthal)
    obst = (dsyn * factors(dsyn.size, 92)).astype(F)
    S = e.iteration_system_maps_device(nx, ny, nmaps, 3 if azimuthal else 1, obst, dsyn, float(c["threshold0"]), float(c["weight0"]), 0.5)
    sol = e.lsmr(S["cbst"], float(c["damp"]), *LSMR_ARGS)
    e.update_maps(sol["x"][:nmaps * layer], M.DEFAULT_DVMAX, float(c["minvel"]), float(c["maxvel"]), nmaps, nx, ny)
    M.plan_engine(e, u)
    velv = e.get_maps(nmaps, nx, ny)
    assert nnz > 0 and sol["itn"] > 3 and sol["x"].any() and np.isfinite(velv).all()
    out = dict(times=dsyn, nnz=np.array([nnz]), maps=velv)
    pack("system", S, out)
    return pack("lsmr", sol, out)


@functools.lru_cache(maxsize=None)
def period_plan_of(shape):
    return M.period_plan(boundary(shape))


def direct_system(e, c, seed):
    """dsa_calsurfg with the rows left on the device (kRowsIsotropic) and dsa_iteration_system_device on them: the first half of a pass of
    invert.iteration_device, on this engine.  Returns (dsyn, obst, nnz, the system)."""
    nx, ny, nz, dall, maxvp = c["nx"], c["ny"], c["nz"], c["ndata"], c["nparpi"]
    stage_rows(e, c)
    with options(e, rows_on_device=1):
        dsyn, nnz = e.solve_rows_device()
        obst = (dsyn * factors(dall, seed)).astype(F)
        cbst = np.zeros(dall + maxvp, F); dw = np.zeros(dall, F); norm = np.zeros(maxvp, F); dws = np.zeros(2, F)
        m, nar = C.c_int(0), C.c_longlong(0)
        e._check(e._L.dsa_iteration_system_device(e._h, nx, ny, nz, dall, _p(obst), _p(dsyn), c["threshold0"], c["weight0"], _p(cbst), _p(dw), _p(norm),
                                                  C.byref(m), C.byref(nar), _p(dws)))
    e._mn = (m.value, maxvp)
    assert nnz > 0 and nar.value > nnz
    return dsyn, obst, nnz, dict(m=m.value, nar=nar.value, cbst=cbst, datweight=dw, norm=norm, dws=dws)


def direct_iteration(e, shape):
    """one pass of invert.iteration_device: device rows, the isotropic system, LSMR, the model update"""
    c = boundary(shape)
    dsyn, obst, nnz, S = direct_system(e, c, 93)
    sol = e.lsmr(S["cbst"], float(c["damp"]), *LSMR_ARGS)
    vsf = np.asfortranarray(c["vels"].copy())
    dv = sol["x"].copy()
    assert e._L.dsa_model_update(c["nx"], c["ny"], c["nz"], _p(dv), _p(vsf), c["minvel"], c["maxvel"]) == 0
    fl, inf = e.unit_ties()
    assert sol["itn"] > 3 and sol["x"].any()
    out = dict(times=dsyn, nnz=np.array([nnz]), model=np.ascontiguousarray(vsf), dv=dv, tie_flags=fl, tie_influence=inf)
    pack("system", S, out)
    return pack("lsmr", sol, out)


def above(vsv, factor=1.03):
    """Vsh = Vsv * factor above the bottom depth, equal at it"""
    vsh = np.array(vsv, F, copy=True)
    vsh[:-1] = (vsh[:-1] * F(factor)).astype(F)
    return vsh


@functools.lru_cache(maxsize=None)
def radial_plan_of(shape):
    return RD.radial_plan(boundary(shape))


def radial_direct(e, shape):
    """one pass of dsurftomo_amd.radial: the radial stage, its runs, maps and depth factors, radial rows resident (kRowsRadial), the system
    (kRowsRadialSystem), LSMR, the update of both models"""
    c, u = boundary(shape), radial_plan_of(shape)
    vsv = c["model"]
    RD.begin(e, c, u, vsv, above(vsv))
    e.keep_fields(False)
    RD.stage(e, c, u)
    dsyn, nnz = e.solve_rows_radial_device()
    obst = (dsyn * factors(dsyn.size, 94)).astype(F)
    S = e.iteration_system_radial_device(c["nx"], c["ny"], c["nz"], obst, dsyn, float(c["threshold0"]), float(c["weight0"]), 1.0, 0.3)
    sol = e.lsmr(S["cbst"], float(c["damp"]), *LSMR_ARGS)
    e.update_radial(sol["x"], RD.DEFAULT_DVMAX, float(c["minvel"]), float(c["maxvel"]))
    after = e.dispersion_get_model_radial()
    assert nnz > 0 and sol["itn"] > 3 and sol["x"][:c["nparpi"]].any() and sol["x"][c["nparpi"]:].any()
    out = dict(times=dsyn, nnz=np.array([nnz]), vsv=after[0], vsh=after[1])
    pack("system", S, out)
    return pack("lsmr", sol, out)


@functools.lru_cache(maxsize=None)
def phase_case(shape):
    """the boundary case with phase periods only, so that every map has its kernel slot and a column step can follow the rows"""
    c = synth.boundary_case(kRc=2, kRg=0, kLc=2, kLg=0) if shape == "big" else synth.boundary_case(nx=10, ny=9, nz=4, kRc=1, kRg=0, kLc=1, kLg=0, nsrc=3, nrcf=4)
    c["model"] = np.ascontiguousarray(np.asarray(c["vels"], F).transpose(2, 1, 0))
    return c, RD.radial_plan(c)


def radial_step_rows(e, shape):
    """the two-step chain on one radial stage: radial rows to the host, a radial column step on the same runs, the rows again.  The step
    changes the models, so the depth factors of the rows are no longer theirs: dsa_solve_rows_radial is refused (DSA_ERR_STATE) until the
    runs and dsa_kernels_from_dispersion_radial are repeated.  The refusal is part of the result"""
    c, u = phase_case(shape)
    assert u["nmaps"] == c["kmax"] and not u["copies"]
    vsv = c["model"]
    RD.begin(e, c, u, vsv, above(vsv))
    e.keep_fields(False)
    RD.stage(e, c, u)
    before = e.solve_rows_radial(capacity(c, 2))
    pv = e.dispersion_fetch(0, c["kmax"], False, 0)
    assert (pv > 0).all()
    step = e.columns_step_radial((pv * 1.01).astype(F), None, R.SMOOTH, R.DAMP, RR.ANISO, R.DVMAX, R.MINVEL, R.MAXVEL)
    try:
        e.solve_rows_radial(capacity(c, 2))
        code = 0
    except EngineError as exc:
        code = exc.code
    assert code == DSA_ERR_STATE, "dsa_solve_rows_radial after a step of the models, without new depth factors: %d" % code
    RD.stage(e, c, u)
    after = e.solve_rows_radial(capacity(c, 2))
    assert before[1].size > 0 and after[1].size > 0 and np.abs(step["dv_sv"]).max() > 0 and (before[0] != after[0]).any()
    out = dict(refused=np.array([code], np.int32))
    for name, r in (("before", before), ("after", after)):
        pack(name, dict(times=r[0], rw=r[1], iw=r[2], col=r[3]), out)
    return pack("step", step, out)


def forward_times(e, c, models):
    """what a pass of dsa_forward_models does on its engine: K models (K, nz, ny, nx) side by side in one stage, the runs without kernels,
    the maps, every model's copy of the unit list on its own maps (model-major), one solve.  Returns dict(times (K, ndata), failures)."""
    K, nd, nmaps = models.shape[0], c["ndata"], c["layout"]["nmaps"]
    u = c["units_times"]
    e.dispersion_begin_models(models, c["depz"], c["minthk"], nmaps)
    dropin_runs(e, c, False)
    e.maps_from_dispersion(c["goxd"], c["gozd"], c["dvxd"], c["dvzd"], 8)
    fails = e.dispersion_model_failures(K)
    tile = lambda a: np.tile(a, K)
    e.keep_fields(False)
    e.plan(np.concatenate([m * nmaps + u["map_index"] for m in range(K)]), tile(u["scx"]), tile(u["scz"]), tile(u["nrec"]), tile(u["rcx"]), tile(u["rcz"]),
           mode=tile(u["mode"]), data_first=np.concatenate([m * nd + u["data_first"] for m in range(K)]))
    t = e.solve().reshape(K, nd)
    fl, inf = e.unit_ties()
    assert t.size > 0 and np.isfinite(t).all() and (t > 0).all()
    return dict(times=t, failures=fails, tie_flags=fl, tie_influence=inf)


def forward_models(e, shape):
    """three models in one stage (big), one (small)"""
    c = boundary(shape)
    K = 3 if shape == "big" else 1
    models = np.stack([(c["model"] * F(1.0 + 0.015 * k)).astype(F) for k in range(K)])
    out = forward_times(e, c, models)
    assert K == 1 or (out["times"][0] != out["times"][K - 1]).all()
    return out


def forward_steps(e, shape):
    """the solutions a trade-off batch left resident (SpmvState::bx) become models on the device (step_models, steps = NULL), which are
    forward-modelled: the path of dsa_forward_steps behind --tradeoff-nonlinear"""
    c = boundary(shape)
    dsyn, obst, nnz, S = direct_system(e, c, 95)
    w0, damp = float(c["weight0"]), float(c["damp"])
    K = 3 if shape == "big" else 2
    T = e.lsmr_tradeoff(S["cbst"], c["ndata"], w0, [0.5 * w0, w0, 2.0 * w0][:K], [damp, damp, 2.0 * damp][:K], True, *LSMR_ARGS)
    models = e.step_models(c["vels"], None, float(c["minvel"]), float(c["maxvel"]), nmodels=K)
    assert int(T["itn"].max()) > 3 and (models[0] != models[K - 1]).any() and (models[0] != np.asarray(c["vels"], F)).any()
    out = forward_times(e, c, np.ascontiguousarray(models.transpose(0, 3, 2, 1)))
    out.update(dsyn=dsyn, models=np.ascontiguousarray(models))
    return pack("tradeoff", T, out)


# ---- the depth family ----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def column_case(shape):
    """test_gpu_columns.py's cases: 5 x 5 columns, nz = 8, columns_ref.WAVES (12 periods), the smooth model (big); 6 x 4 columns, nz = 3,
    half the periods, the edge model, which loses roots (small).  Weights around 1, a tenth of them 0, the centre column without any."""
    if shape == "big":
        nx, ny, nz, waves, model = 5, 5, 8, list(R.WAVES), R.smooth_model
    else:
        nx, ny, nz, model = 6, 4, 3, R.edge_model
        waves = [(wave, kind, t[[0, 2]] if kind == 0 else t[[1]]) for wave, kind, t in R.WAVES]
    K = sum(len(t) for _, _, t in waves)
    ncol = nx * ny
    rng = np.random.default_rng(7 + nz)
    wt = (0.5 + rng.random((K, ncol))).astype(F)
    wt[rng.random((K, ncol)) < 0.1] = 0.0
    wt[:, (ny // 2) * nx + nx // 2] = 0.0
    return dict(nx=nx, ny=ny, nz=nz, K=K, ncol=ncol, waves=waves, depz=R.depths(nz), vel=model(nx, ny, nz), wt=wt, noise=rng.standard_normal((K, ncol)),
                flat=(2.5 + 1.5 * rng.random((K, ncol))).astype(F), smooth=shape == "big")


def column_runs(e, q, kernels=True):
    first = 0
    for wave, kind, t in q["waves"]:
        e.dispersion_run(wave, kind, t, kernels, first if kernels else 0, first)
        first += len(t)


def column_obs(e, q):
    """the observations: the present curves 2 % off (the smooth model), or values far from them (the edge model)"""
    pv0 = e.dispersion_fetch(0, q["K"], False, 0)
    assert (pv0[:, R.interior(q["nx"], q["ny"]) == 1] > 0).any()
    return ((pv0 * (1.0 + 0.02 * q["noise"])).astype(F) if q["smooth"] else q["flat"]), pv0


def column_clip(q):
    return (R.DVMAX, R.MINVEL, R.MAXVEL) if q["smooth"] else (0.1, 2.0, 4.5)


def columns_plain(e, shape):
    """a plain stage, the runs with kernels, the resolution (reads only), the step, the stepped model"""
    q = column_case(shape)
    e.dispersion_begin(q["vel"], q["depz"], R.MINTHK, q["K"], q["K"])
    column_runs(e, q)
    obs, pv0 = column_obs(e, q)
    res = e.columns_resolution(obs, q["wt"], R.SMOOTH, R.DAMP, full=True)
    step = e.columns_step(obs, q["wt"], R.SMOOTH, R.DAMP, *column_clip(q))
    model = e.dispersion_get_model()
    assert np.abs(step["dv"]).max() > 0 and (step["flag"] == 0).any() and res["R"].any()
    out = dict(pv=pv0, model=model)
    pack("resolution", res, out)
    return pack("step", step, out)


def columns_radial(e, shape):
    """the same on a radial stage: Vsh 3 % above Vsv"""
    q = column_case(shape)
    e.dispersion_begin_radial(q["vel"], above(q["vel"]), q["depz"], R.MINTHK, q["K"], q["K"])
    column_runs(e, q)
    obs, pv0 = column_obs(e, q)
    res = e.columns_resolution_radial(obs, q["wt"], R.SMOOTH, R.DAMP, RR.ANISO, full=True)
    step = e.columns_step_radial(obs, q["wt"], R.SMOOTH, R.DAMP, RR.ANISO, *column_clip(q))
    vsv, vsh = e.dispersion_get_model_radial()
    assert np.abs(step["dv_sv"]).max() > 0 and np.abs(step["dv_sh"]).max() > 0 and (step["flag"] == 0).any() and res["R"].any()
    out = dict(pv=pv0, vsv=vsv, vsh=vsh)
    pack("resolution", res, out)
    return pack("step", step, out)


def lateral_members(q, count):
    """count members of the lateral resolution: spikes and rows of unknowns spread over all of them, then a test model and a right-hand side"""
    nint, Mz = (q["nx"] - 2) * (q["ny"] - 2), q["nz"] - 1
    index = (np.arange(count - 2) * 5) % (nint * Mz)
    kind = (np.arange(count - 2) % 2).astype(np.int32)
    models = np.random.default_rng(7).standard_normal((2, Mz, nint))
    return np.r_[kind, 2, 3].astype(np.int32), np.r_[index, 0, 1].astype(np.int32), models


def columns_lateral(e, shape):
    """the laterally coupled resolution -- 70 members, two lane groups, the second partial (big); 5 (small) -- and the coupled step"""
    q = column_case(shape)
    e.dispersion_begin(q["vel"], q["depz"], R.MINTHK, q["K"], q["K"])
    column_runs(e, q)
    obs, pv0 = column_obs(e, q)
    kind, index, models = lateral_members(q, 70 if shape == "big" else 5)
    res = e.columns_resolution_lateral(obs, q["wt"], R.SMOOTH, R.DAMP, IR.LATERAL, kind, index, models, IR.TOL, IR.MAXIT, full=True)
    step = e.columns_step_lateral(obs, q["wt"], R.SMOOTH, R.DAMP, IR.LATERAL, *column_clip(q), IR.TOL, IR.MAXIT)
    model = e.dispersion_get_model()
    assert np.abs(step["dv"]).max() > 0 and step["itn"] >= 1 and res["full"].any() and int(res["itn"].max()) >= 1
    out = dict(pv=pv0, model=model)
    pack("resolution", res, out)
    return pack("step", step, out)


def columns_radial_lateral(e, shape):
    """the laterally coupled step of a radial stage"""
    q = column_case(shape)
    e.dispersion_begin_radial(q["vel"], above(q["vel"]), q["depz"], R.MINTHK, q["K"], q["K"])
    column_runs(e, q)
    obs, pv0 = column_obs(e, q)
    step = e.columns_step_radial_lateral(obs, q["wt"], R.SMOOTH, R.DAMP, RR.ANISO, LR.LATERAL, LR.LATERAL_ANISO, *column_clip(q), LR.TOL, LR.MAXIT)
    vsv, vsh = e.dispersion_get_model_radial()
    assert np.abs(step["dv_sv"]).max() > 0 and np.abs(step["dv_sh"]).max() > 0 and step["itn"] >= 1
    return pack("step", step, dict(pv=pv0, vsv=vsv, vsh=vsh))


SAMPLE = dict(smooth=3.0, step=0.05, spread=0.05, width=0.4, temperature=1.0)           # tests/test_gpu_column_sample.py's PAR
SIGMA = 0.02


def columns_sample(e, shape):
    """a sample stage of 27 chains per column (big) or 3 (small): the set-up, three sweeps, the raw state and the finish.  The observations
    are the start model's own curves 2 % off, computed on a plain stage first"""
    q = column_case(shape)
    C_ = 27 if shape == "big" else 3
    e.dispersion_begin(q["vel"], q["depz"], R.MINTHK, q["K"], q["K"])
    column_runs(e, q, kernels=False)
    pv0 = e.dispersion_fetch(0, q["K"], False, 0)
    obs = np.where(pv0 > 0, pv0 * (1.0 + 0.02 * q["noise"]), q["flat"]).astype(F)
    wt = (q["wt"] / F(SIGMA)).astype(F)
    p = dict(SAMPLE) if q["smooth"] else dict(SAMPLE, temperature=2000.0, spread=0.2, step=0.2)
    e.columns_sample_begin(q["vel"], q["depz"], R.MINTHK, q["waves"], obs, wt, C_, p["smooth"], p["step"], p["spread"], p["width"], p["temperature"], R.MINVEL, R.MAXVEL,
                           2 ** 35 + 11 * q["nz"] + C_, 1)
    e.columns_sample_run(3)
    state = e.columns_sample_state()
    fetch = e.columns_sample_fetch()
    assert fetch["accepted"].sum() > 0 and fetch["rejected"].sum() > 0, "the sampler holds no accepted or no rejected proposal"
    out = dict(pv=pv0)
    pack("state", state, out)
    return pack("fetch", fetch, out)


# ---- the LSMR family on a given matrix --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def matrix_case(shape):
    """synth_matrix.system: ray-like data rows and the regularisation rows of main.f90 with weight 2.  big 300 + 288 rows over 9 x 8 x 4
    unknowns, small 120 + 90 over 6 x 5 x 3"""
    md, nvx, nvy, nl = (300, 9, 8, 4) if shape == "big" else (120, 6, 5, 3)
    S = SM.system(md, nvx, nvy, nl, seed=5 if shape == "big" else 6, long_rows=0, mean_len=12)
    m, n = S["m"], S["n"]
    b = np.zeros(m, F)
    b[:md] = (SM.mix(np.arange(md), 12) - 0.5).astype(F)
    i, j, k = np.meshgrid(np.arange(nvx), np.arange(nvy), np.arange(nl), indexing="ij")
    xyz = np.zeros((nl, nvy, nvx, 3))
    xyz[..., 0] = (24.0 - 0.05 * i).transpose(2, 1, 0); xyz[..., 1] = (121.0 + 0.05 * j).transpose(2, 1, 0); xyz[..., 2] = (4.0 * k).transpose(2, 1, 0)
    rng = np.random.default_rng(3)
    R_ = 70 if shape == "big" else 3
    K = 3 if shape == "big" else 2
    ncells = 24 if shape == "big" else 10
    return dict(S=S, m=m, n=n, nd=md, b=b, xyz=xyz.reshape(-1, 3), scales=(0.5 + rng.random((R_, m))).astype(F), x=rng.standard_normal(n).astype(F),
                y=rng.standard_normal(m).astype(F), fold=(rng.permutation(md) % 2).astype(np.int32), K=K, ncells=ncells,
                seeds=np.stack([rng.permutation(n)[:ncells] for _ in range(K)]).astype(np.int32))


def lsmr_family(e, shape):
    """spmv_load, then every solver that reads the resident matrix: spmv both ways, lsmr with its vectors on the host and on the device, a
    batch of 70 members (two lane groups; small: 3), the trade-off, the cross-validation, the Voronoi ensemble, the spike solves"""
    q = matrix_case(shape)
    S, b, nd = q["S"], q["b"], q["nd"]
    e.spmv_load(S["m"], S["n"], S["rw"], S["row"], S["col"])
    out = dict(Ax=e.spmv(1, q["x"], np.zeros(q["m"], F)), Aty=e.spmv(2, np.zeros(q["n"], F), q["y"]))
    host = e.lsmr(b, 0.5, *LSMR_ARGS)
    with options(e, lsmr_device_vectors=1):
        dev = e.lsmr(b, 0.5, *LSMR_ARGS)
    batch = e.lsmr_batch(b, q["scales"], 0.5, *LSMR_ARGS)
    K = q["K"]
    trade = e.lsmr_tradeoff(b, nd, 2.0, [1.0, 2.0, 4.0][:K], [0.5, 0.5, 1.0][:K], True, *LSMR_ARGS)
    cross = e.lsmr_crossval(b, nd, 2.0, [1.0, 2.0, 4.0][:K], [0.5, 0.5, 1.0][:K], q["fold"], 2, True, True, *LSMR_ARGS)
    vor = e.lsmr_voronoi(b, nd, q["ncells"], q["xyz"], q["seeds"], 0.5, True, True, True, *LSMR_ARGS)
    res = e.lsmr_resolution(nd, 0.5, spikes=spikes_of(q["n"], 4 if shape == "big" else 2), coords=q["xyz"], atol=LSMR_ARGS[0], btol=LSMR_ARGS[1],
                            conlim=LSMR_ARGS[2], itnlim=LSMR_ARGS[3], local_size=LSMR_ARGS[4])
    for name, r in (("lsmr", host), ("lsmr_device", dev), ("batch", batch), ("tradeoff", trade), ("crossval", cross), ("voronoi", vor), ("resolution", res)):
        assert int(np.max(r["itn"])) > 3, name
        pack(name, r, out)
    assert out["Ax"].any() and out["Aty"].any() and batch["x"].any() and vor["z"].any() and res["x"].any()
    return out


RUN = dict(times_default=times_default, times_exact=times_exact, times_bundled=times_bundled, rows=rows, rows_capacity_refused=rows_capacity_refused,
           azimuthal_device=azimuthal_device, maps_loop=maps_loop, direct_iteration=direct_iteration, radial_direct=radial_direct, radial_step_rows=radial_step_rows, columns_plain=columns_plain,
           columns_radial=columns_radial, columns_lateral=columns_lateral, columns_radial_lateral=columns_radial_lateral, columns_sample=columns_sample,
           forward_models=forward_models, forward_steps=forward_steps, lsmr_family=lsmr_family)
assert tuple(RUN) == NAMES


def run(name, shape, e):
    """workload `name` in `shape` on the engine e: dict[str, ndarray], never empty, no array empty"""
    out = RUN[name](e, shape)
    out = {k: np.ascontiguousarray(v) for k, v in out.items()}
    assert out and all(v.size > 0 for v in out.values()), [k for k, v in out.items() if v.size == 0]
    return out


def difference(got, want):
    """None where got and want hold the same arrays in every byte, shape and dtype; else (the first field that differs, elements that
    differ there, its size)"""
    if list(got) != list(want):
        return ("the fields themselves: %s" % sorted(set(got) ^ set(want)), 0, 0)
    for k, a in got.items():
        b = want[k]
        if a.shape != b.shape or a.dtype != b.dtype:
            return ("%s (%s %s, expected %s %s)" % (k, a.dtype, a.shape, b.dtype, b.shape), a.size, a.size)
        ab, bb = a.reshape(-1).view(np.uint8).reshape(a.size, -1), b.reshape(-1).view(np.uint8).reshape(b.size, -1)
        bad = (ab != bb).any(axis=1)
        if bad.any():
            return (k, int(bad.sum()), a.size)
    return None


# ---- the schedules ----------------------------------------------------------------------------------------------------------------------------

PAIRS = tuple((a, b) for i, a in enumerate(NAMES) for b in NAMES[i + 1:])


def pair_schedule(a, b):
    """test_pairs[a-b], a before b in NAMES: a.big, b.small, a.big -- a onto a smaller problem of another kind, and back onto the larger one"""
    return [(a, "big"), (b, "small"), (a, "big")]


SAME_KIND = ("big", "big", "small", "big", "small", "small")
WALK_SEED, WALK_VISITS, WALK_STEPS, WALK_SEGMENT = 20251020, 3, 150, 10


def walk_schedule():
    """a seeded walk over every (workload, shape), WALK_VISITS times each in one shuffled order, then free draws up to WALK_STEPS steps"""
    rng = np.random.default_rng(WALK_SEED)
    cells = [(n, s) for n in NAMES for s in SHAPES]
    steps = [cells[i] for i in rng.permutation(np.repeat(np.arange(len(cells)), WALK_VISITS))]
    steps += [cells[i] for i in rng.integers(0, len(cells), WALK_STEPS - len(steps))]
    return steps
