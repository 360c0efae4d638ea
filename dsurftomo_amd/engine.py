"""Python binding of the engine-level C ABI (include/dsurftomo_amd.h) via ctypes.

Plumbing only: arrays in, arrays out.  There is no CPU implementation behind this class; if the
HIP library is missing or no GPU is usable, construction raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DSA_LIB_PATH") or os.path.join(_HERE, "libdsurftomo_amd.so")   # (override: A/B builds)

STAT_NAMES = ("ms_total", "ms_fim_coarse", "ms_fim_refined", "ms_stages", "launches_fim_coarse", "units",
              "rounds_max", "evals_total", "chunk", "rescans", "freezes", "rays", "ray_steps", "rays_clamped",
              "ms_rays", "ms_rows", "nar", "ms_dispersion", "curves", "changes_total", "tie_units", "exact_units", "exact_pops", "ms_exact", "field_slots", "footprint_mb", "bundle_size", "bundles", "bundled_units", "bundle_slots", "bundle_threads", "tie_units_left", "tie_influence_max", "exact_pool", "exact_tiles", "tie_units_strict", "tie_prone_maps", "tie_units_tied", "tie_units_by_scale", "handoffs_replayed", "ray_launches")

_f32, _i32, _vp = C.c_float, C.c_int, C.c_void_p
_lib = None


class EngineError(RuntimeError):
    def __init__(self, code, text):
        super().__init__("dsurftomo_amd error %d: %s" % (code, text))
        self.code = code


def load_library():
    """Load the in-tree HIP library; raises if it has not been built (python -m dsurftomo_amd.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError("%s is missing: build it with `python -m dsurftomo_amd.build` "
                                "(there is no CPU fallback)" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    L.dsa_create.argtypes = [C.POINTER(_vp), _i32]
    L.dsa_destroy.argtypes = [_vp]
    L.dsa_destroy.restype = None
    L.dsa_set_memory_budget.argtypes = [_vp, C.c_size_t]
    L.dsa_set_option.argtypes = [_vp, C.c_char_p, C.c_double]
    L.dsa_set_maps.argtypes = [_vp, _i32, _i32, _f32, _f32, _f32, _f32, _i32, _i32, _vp]
    L.dsa_plan.argtypes = [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp]
    L.dsa_solve.argtypes = [_vp, _vp]
    L.dsa_solve_device.argtypes = [_vp, _vp]
    L.dsa_plan_units.argtypes = [_vp, _i32] + [_vp] * 9
    L.dsa_set_depth_kernels.argtypes = [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp]
    L.dsa_solve_rows.argtypes = [_vp, _vp, _vp, _vp, _vp, C.c_longlong, C.POINTER(C.c_longlong)]
    L.dsa_dispersion_begin.argtypes = [_vp, _i32, _i32, _i32, _vp, _vp, _f32, _i32, _i32]
    L.dsa_dispersion_begin_models.argtypes = [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _f32, _i32]
    L.dsa_dispersion_model_failures.argtypes = [_vp, _i32, _vp]
    L.dsa_step_models.argtypes = [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _f32, _f32, _vp]
    L.dsa_dispersion_run.argtypes = [_vp, _i32, _i32, _i32, _vp, _i32, _i32, _i32]
    L.dsa_dispersion_copy_maps.argtypes = [_vp, _i32, _i32, _i32]
    L.dsa_dispersion_fetch.argtypes = [_vp, _i32, _i32, _vp, _i32, _i32, _vp, _vp, _vp]
    L.dsa_maps_from_dispersion.argtypes = [_vp, _f32, _f32, _f32, _f32, _i32]
    L.dsa_kernels_from_dispersion.argtypes = [_vp]
    L.dsa_get_dims.argtypes = [_vp, C.POINTER(_i32), C.POINTER(_i32)]
    L.dsa_keep_fields.argtypes = [_vp, _i32]
    L.dsa_get_field.argtypes = [_vp, _i32, _vp]
    L.dsa_get_velocity.argtypes = [_vp, _i32, _vp]
    L.dsa_get_refined.argtypes = [_vp, _i32, C.POINTER(_i32), C.POINTER(_i32), _vp, _vp]
    L.dsa_get_stats.argtypes = [_vp, _vp]
    L.dsa_ray_diagnostics.argtypes = [_vp, C.POINTER(C.c_longlong), C.POINTER(_i32)]
    L.dsa_unit_ties.argtypes = [_vp, _i32, _vp, _vp]
    L.dsa_unit_rounds.argtypes = [_vp, _i32, _vp]
    if hasattr(L, "dsa_unit_tie_sums"):          # (absent from libraries of rounds 1-5: same-box A/B runs against an old build, DSA_LIB_PATH)
        L.dsa_unit_tie_sums.argtypes = [_vp, _i32, _vp, _vp, _vp]
    L.dsa_debug_counters.argtypes = [_vp, _vp]
    L.dsa_ray_paths.argtypes = [_vp, _vp, _vp, _vp]
    L.dsa_solve_rows_azimuthal.argtypes = [_vp, _vp, _vp, _vp, _vp, C.c_longlong, C.POINTER(C.c_longlong)]
    L.dsa_set_azimuthal_slots.argtypes = [_vp, _i32, _vp]
    L.dsa_ray_azimuths.argtypes = [_vp, _vp, _vp, _vp]
    L.dsa_spmv.argtypes = [_vp, _i32, _vp, _vp]
    L.dsa_debug_field.argtypes = [_vp, _i32, _i32, _vp]
    L.dsa_selfcheck_divisions.argtypes = [C.c_ulonglong, _i32, _vp, _vp]
    if hasattr(L, "dsa_selfcheck_trip"):         # (absent from older libraries: same-box A/B runs, DSA_LIB_PATH)
        L.dsa_selfcheck_trip.argtypes = [C.c_ulonglong, _i32, _vp]
    L.dsa_dropin_error.restype = C.c_char_p
    L.dsa_dropin_set_capacity.argtypes = [C.c_longlong]
    L.dsa_aprod_invalidate.argtypes = []
    _lib = declare_solvers(L)
    return L


def declare_solvers(L):
    """argtypes / restype of the dsa_lsmr* family and of what the inversion driver calls around it (the system builders, the model update,
    the drop-in engine, the error text), on any handle of the library: load_library's own, or a bare ctypes.CDLL (invert.bind).  The one
    place they are declared.  Returns L."""
    solve = [_f32] * 3 + [_i32] * 2                                   # atol, btol, conlim, itnlim, localSize
    L.dsa_error_string.argtypes = [_vp]
    L.dsa_error_string.restype = C.c_char_p
    L.dsa_dropin_engine.argtypes = []
    L.dsa_dropin_engine.restype = _vp
    L.dsa_calsurfg_azimuthal.argtypes = [_vp] * 36            # dsa_calsurfg's list: every argument by reference
    L.dsa_iteration_system.argtypes = [_i32] * 4 + [C.c_longlong] * 2 + [_vp] * 5 + [_f32] * 2 + [_vp] * 6
    L.dsa_iteration_system_device.argtypes = [_vp] + [_i32] * 4 + [_vp] * 2 + [_f32] * 2 + [_vp] * 6
    L.dsa_solve_rows_azimuthal_device.argtypes = [_vp, _vp, _vp, _vp, _vp, C.c_longlong, C.POINTER(C.c_longlong)]
    L.dsa_iteration_system_azimuthal_device.argtypes = [_vp] + [_i32] * 4 + [_vp] * 2 + [_f32] * 3 + [_vp] * 6
    L.dsa_model_update.argtypes = [_i32] * 3 + [_vp] * 2 + [_f32] * 2
    L.dsa_solve_rows_maps.argtypes = [_vp, _i32, _vp, _vp, _vp, _vp, C.c_longlong, C.POINTER(C.c_longlong)]
    L.dsa_iteration_system_maps_device.argtypes = [_vp] + [_i32] * 5 + [_vp] * 2 + [_f32] * 3 + [_vp] * 6
    L.dsa_update_maps.argtypes = [_vp, _i32, _vp] + [_f32] * 3
    L.dsa_get_maps.argtypes = [_vp, _i32, _vp]
    L.dsa_maps_resolution.argtypes = [_vp] + [_i32] * 5 + [_f32, _i32] + [_vp] * 6
    L.dsa_columns_step.argtypes = [_vp, _i32, _vp, _vp] + [_f32] * 5 + [_vp] * 4
    L.dsa_dispersion_get_model.argtypes = [_vp, _vp]
    L.dsa_columns_resolution.argtypes = [_vp, _i32, _vp, _vp] + [_f32] * 2 + [_vp] * 6
    L.dsa_columns_azimuthal.argtypes = [_vp, _i32] + [_vp] * 4 + [_f32] * 2 + [_vp] * 6
    L.dsa_dispersion_begin_radial.argtypes =[_vp, _i32, _i32, _i32, _vp, _vp, _vp, _f32, _i32, _i32]
    L.dsa_columns_step_radial.argtypes = [_vp, _i32, _vp, _vp] + [_f32] * 6 + [_vp] * 4
    L.dsa_dispersion_get_model_radial.argtypes = [_vp, _vp, _vp]
    L.dsa_columns_resolution_radial.argtypes = [_vp, _i32, _vp, _vp] + [_f32] * 3 + [_vp] * 7
    L.dsa_columns_step_lateral.argtypes = [_vp, _i32, _vp, _vp] + [_f32] * 6 + [C.c_double, _i32] + [_vp] * 5
    L.dsa_columns_step_radial_lateral.argtypes = [_vp, _i32, _vp, _vp] + [_f32] * 8 + [C.c_double, _i32] + [_vp] * 5
    L.dsa_columns_resolution_lateral.argtypes = [_vp, _i32, _vp, _vp] + [_f32] * 3 + [C.c_double, _i32, _i32, _vp, _vp, _vp, _i32] + [_vp] * 5
    L.dsa_columns_sample_begin.argtypes = [_vp] + [_i32] * 4 + [_vp, _vp, _f32, _i32] + [_vp] * 4 + [_i32, _vp, _vp] + [_f32] * 7 + [C.c_ulonglong, _i32]
    L.dsa_columns_sample_run.argtypes = [_vp, _i32]
    L.dsa_columns_sample_fetch.argtypes = [_vp] * 4
    L.dsa_columns_sample_state.argtypes = [_vp] * 15
    L.dsa_columns_sample_shape.argtypes = [_vp, _i32, _vp, _vp] + [_f32] * 2 + [_vp] * 3
    L.dsa_columns_sample_blocks.argtypes = [_vp, _i32, C.c_double]
    L.dsa_columns_sample_block_state.argtypes = [_vp] * 3
    L.dsa_columns_sample_marginals.argtypes = [_vp, _i32, _i32]
    L.dsa_columns_sample_marginals_fetch.argtypes = [_vp, _i32] + [_vp] * 4
    L.dsa_columns_sample_marginals_state.argtypes = [_vp] * 3
    L.dsa_columns_sample_radial_begin.argtypes = [_vp] + [_i32] * 4 + [_vp, _vp, _vp, _f32, _i32] + [_vp] * 4 + [_i32, _vp, _vp] + [_f32] * 8 + [C.c_ulonglong, _i32, _i32]
    L.dsa_columns_sample_radial_run.argtypes = [_vp, _i32]
    L.dsa_columns_sample_radial_fetch.argtypes = [_vp] * 4
    L.dsa_columns_sample_radial_state.argtypes = [_vp] * 25
    L.dsa_kernels_from_dispersion_radial.argtypes = [_vp]
    L.dsa_solve_rows_radial.argtypes = [_vp, _vp, _vp, _vp, _vp, C.c_longlong, C.POINTER(C.c_longlong)]
    L.dsa_iteration_system_radial_device.argtypes = [_vp] + [_i32] * 4 + [_vp] * 2 + [_f32] * 4 + [_vp] * 6
    L.dsa_update_radial.argtypes = [_vp] + [_i32] * 3 + [_vp] + [_f32] * 3
    L.dsa_spmv_load.argtypes = [_vp, _i32, _i32, C.c_longlong, _vp, _vp, _vp]
    L.dsa_lsmr.argtypes = [_vp, _vp, _f32] + solve + [_vp] * 8
    L.dsa_lsmr_batch.argtypes = [_vp, _i32, _vp, _vp, _f32] + solve + [_vp] * 4
    L.dsa_lsmr_resolution.argtypes = [_vp, _i32, _i32, _vp, _i32, _vp, _f32] + solve + [_vp] * 5
    L.dsa_resolution_blocks.argtypes = [_vp, _i32, _i32, _i32, _i32, _vp, _f32] + solve + [_vp] * 5
    L.dsa_lsmr_tradeoff.argtypes = [_vp, _i32, _i32, _vp, _f32, _vp, _vp] + solve + [_vp] * 5
    L.dsa_lsmr_crossval.argtypes = [_vp] + [_i32] * 3 + [_vp, _f32] + [_vp] * 3 + solve + [_vp] * 6
    L.dsa_lsmr_voronoi.argtypes = [_vp] + [_i32] * 3 + [_vp] * 3 + [_f32] + solve + [_vp] * 6
    return L


def _p(a):
    return a.ctypes.data_as(_vp) if a is not None and a.size else None


EST_NAMES = ("normA", "condA", "normr", "normAr", "normx")


def selfcheck_divisions(seed, millions, exponents8):
    """device self-check of the hand-expanded divisions (include/dsurftomo_amd.h: dsa_selfcheck_divisions): (fp64 pairs, fp64 quotients that
    differ from the compiler's division bitwise, fp32 pairs, fp32 quotients that differ)"""
    L = load_library()
    ex = np.ascontiguousarray(exponents8, np.int32)
    out = np.zeros(4, np.uint64)
    rc = L.dsa_selfcheck_divisions(int(seed), int(millions), _p(ex), _p(out))
    if rc != 0:
        raise EngineError("dsa_selfcheck_divisions failed (%d)" % rc)
    return tuple(int(v) for v in out)


def selfcheck_trip(seed, millions):
    """device self-check of the node trip's arithmetic helpers (include/dsurftomo_amd.h: dsa_selfcheck_trip): (square roots tried, that differ
    from sqrtf bitwise, arguments the guard left to sqrtf, minima tried, that differ)"""
    L = load_library()
    out = np.zeros(5, np.uint64)
    rc = L.dsa_selfcheck_trip(int(seed), int(millions), _p(out))
    if rc != 0:
        raise EngineError("dsa_selfcheck_trip failed (%d)" % rc)
    return tuple(int(v) for v in out)


class Engine:
    def __init__(self, device=0):
        self._L = load_library()
        h = _vp()
        rc = self._L.dsa_create(C.byref(h), int(device))
        if rc != 0:
            raise EngineError(rc, self._L.dsa_error_string(None).decode())
        self._h = h
        self.nnx = self.nnz = 0
        self._nrays = 0
        self._ndata = 0
        self._disp = (0, 0, 0)
        self._sample = (0, 0)                       # (chains, maps) of the last columns_sample_begin
        self._marginals = (0, False)                # (nbins, with_cov) of the last columns_sample_marginals since then
        self._sample_radial = (0, 0)                # (chains, maps) of the last columns_sample_radial_begin

    def close(self):
        if getattr(self, "_h", None):
            self._L.dsa_destroy(self._h)
            self._h = None

    __del__ = close

    def _check(self, rc):
        if rc != 0:
            raise EngineError(rc, self._L.dsa_error_string(self._h).decode())

    def set_memory_budget(self, nbytes):
        self._check(self._L.dsa_set_memory_budget(self._h, int(nbytes)))

    def set_option(self, name, value):
        self._check(self._L.dsa_set_option(self._h, name.encode(), float(value)))

    def set_maps(self, nx, ny, goxd, gozd, dvxd, dvzd, pv, dicing=8):
        """pv: (nmaps, nx*ny) float64, latitude index fastest inside a map."""
        pv = np.ascontiguousarray(pv, np.float64).reshape(-1, nx * ny)
        self._check(self._L.dsa_set_maps(self._h, nx, ny, goxd, gozd, dvxd, dvzd, dicing, pv.shape[0], _p(pv)))
        a, b = _i32(), _i32()
        self._check(self._L.dsa_get_dims(self._h, C.byref(a), C.byref(b)))
        self.nnx, self.nnz = a.value, b.value

    def plan(self, map_index, scx, scz, nrec, rcx, rcz, mode=None, sen_slot=None, data_first=None):
        """mode / sen_slot / data_first: optional per-unit arrays (see dsa_plan_units)"""
        map_index = np.ascontiguousarray(map_index, np.int32)
        scx = np.ascontiguousarray(scx, np.float32)
        scz = np.ascontiguousarray(scz, np.float32)
        nrec = np.ascontiguousarray(nrec, np.int32)
        rcx = np.ascontiguousarray(rcx, np.float32)
        rcz = np.ascontiguousarray(rcz, np.float32)
        n = map_index.size
        if not (scx.size == n and scz.size == n and nrec.size == n):
            raise ValueError("per-unit arrays differ in length")
        self._nrays = int(nrec.sum())
        self._nrec_of_plan = nrec
        if rcx.size != self._nrays or rcz.size != self._nrays:
            raise ValueError("receiver arrays must hold sum(nrec) entries")
        opt = [None if a is None else np.ascontiguousarray(a, np.int32) for a in (mode, sen_slot, data_first)]
        if any(a is not None and a.size != n for a in opt):
            raise ValueError("per-unit arrays differ in length")
        self._ndata = self._nrays if opt[2] is None else (int((opt[2] + nrec).max()) if n else 0)
        self._check(self._L.dsa_plan_units(self._h, n, _p(map_index), _p(scx), _p(scz), _p(nrec), _p(rcx), _p(rcz),
                                           *[None if a is None else _p(a) for a in opt]))

    def solve(self, want_times=True):
        out = np.zeros(self._ndata, np.float32) if want_times else None
        self._check(self._L.dsa_solve(self._h, _p(out) if want_times else None))
        return out

    def solve_device(self, device_ptr):
        """solve; the receiver times (ndata float32) go to `device_ptr`, memory of this engine's GPU (e.g. tensor.data_ptr())"""
        self._check(self._L.dsa_solve_device(self._h, C.c_void_p(int(device_ptr))))

    @property
    def ndata(self):
        return self._ndata

    def set_depth_kernels(self, vels, depz, sen_vs, sen_vp, sen_rho):
        """vels: (nz, ny, nx) fp32 [Fortran vels(nx,ny,nz)]; sen_*: (nz, kmax, ny*nx) fp64 [Fortran (nx*ny, kmax, nz)]"""
        vels = np.ascontiguousarray(vels, np.float32)
        depz = np.ascontiguousarray(depz, np.float32)
        sen = [np.ascontiguousarray(a, np.float64) for a in (sen_vs, sen_vp, sen_rho)]
        nz, kmax = sen[0].shape[0], sen[0].shape[1]
        self._check(self._L.dsa_set_depth_kernels(self._h, nz, kmax, _p(vels), _p(depz), *[_p(a) for a in sen]))

    def _solve_rows(self, fn, lead, capacity, host=True, null_if_empty=False):
        """one of the dsa_solve_rows* entries (fn, its arguments `lead` between the handle and the times).  host: the rows come to three
        arrays of `capacity` entries, returns (times, rw, row, col) cut to the entries written; else the three arrays are NULL (the rows stay
        on the device), returns (times, number of entries).  null_if_empty: arrays of capacity 0 are passed as NULL"""
        out = np.zeros(self._ndata, np.float32)
        nar = C.c_longlong(0)
        if not host:
            self._check(fn(self._h, *lead, _p(out), None, None, None, C.c_longlong(capacity), C.byref(nar)))
            return out, nar.value
        rw, iw, col = np.zeros(capacity, np.float32), np.zeros(capacity, np.int32), np.zeros(capacity, np.int32)
        ptr = _p if null_if_empty else (lambda a: a.ctypes.data_as(_vp))
        self._check(fn(self._h, *lead, _p(out), ptr(rw), ptr(iw), ptr(col), C.c_longlong(capacity), C.byref(nar)))
        n = nar.value
        return out, rw[:n].copy(), iw[:n].copy(), col[:n].copy()

    def solve_rows(self, capacity):
        """receiver times plus Frechet rows as COO (rw, row, col), rows / columns 1-based"""
        return self._solve_rows(self._L.dsa_solve_rows, (), capacity, null_if_empty=True)

    def solve_rows_device(self):
        """receiver times; the Frechet rows stay on the device (set_option('rows_on_device', 1) before it): returns (times, number of entries)"""
        return self._solve_rows(self._L.dsa_solve_rows, (), 1 << 62, host=False)

    def solve_rows_azimuthal(self, capacity):
        """solve_rows with the gc and gs blocks behind every ray's isotropic entries (dsa_solve_rows_azimuthal): columns
        B * maxvp + isotropic column, B = 1 (gc), 2 (gs)"""
        return self._solve_rows(self._L.dsa_solve_rows_azimuthal, (), capacity)

    def solve_rows_azimuthal_device(self, capacity, host_copy=True):
        """solve_rows_azimuthal with the rows left on the device (dsa_solve_rows_azimuthal_device), whatever the option rows_on_device says.
        host_copy: returns (times, rw, row, col), the copy bit for bit solve_rows_azimuthal's; else (times, number of entries) and no row
        leaves the device"""
        return self._solve_rows(self._L.dsa_solve_rows_azimuthal_device, (), capacity, host=host_copy)

    # ---- per-period 2-D maps -------------------------------------------------
    def solve_rows_maps(self, capacity, azimuthal=False):
        """receiver times plus the map rows as COO (rw, row, col), 1-based: columns (B * nmaps + map) * layer + vertex + 1, B = 0 (c0) and, with
        azimuthal, 1 (A1, cos 2psi) and 2 (A2, sin 2psi) (dsa_solve_rows_maps); no depth kernels needed"""
        return self._solve_rows(self._L.dsa_solve_rows_maps, (int(bool(azimuthal)),), capacity)

    def solve_rows_maps_device(self, azimuthal=False, capacity=1 << 62):
        """solve_rows_maps with the rows left on the device for iteration_system_maps_device: returns (times, number of entries)"""
        return self._solve_rows(self._L.dsa_solve_rows_maps, (int(bool(azimuthal)),), capacity, host=False)

    def _iteration_system_device(self, fn, lead, obst, dsyn, floats, n, rows_below, nblocks):
        """one of the dsa_iteration_system_*_device entries (fn, its leading integers `lead`, its floats from threshold0 on) on the rows left on
        the device, for a system of n columns, rows_below rows below the data rows and nblocks blocks of unknowns.  Returns dict(m, n, nar,
        cbst (dall + rows_below,), datweight (dall,), norm (n,), dws (nblocks, 2)); afterwards lsmr(cbst, damp) solves on the resident matrix"""
        f = np.float32
        obst = np.ascontiguousarray(obst, f); dsyn = np.ascontiguousarray(dsyn, f)
        dall = obst.size
        if dsyn.size != dall:
            raise ValueError("obst and dsyn differ in length")
        cbst = np.zeros(dall + rows_below, f); datweight = np.zeros(dall, f); norm = np.zeros(max(n, 1), f); dws = np.zeros(2 * nblocks, f)
        m, nar = C.c_int(0), C.c_longlong(0)
        self._check(fn(self._h, *[int(v) for v in lead], dall, _p(obst), _p(dsyn), *[float(v) for v in floats], cbst.ctypes.data_as(_vp),
                       datweight.ctypes.data_as(_vp), norm.ctypes.data_as(_vp), C.byref(m), C.byref(nar), dws.ctypes.data_as(_vp)))
        self._mn = (m.value, n)
        return dict(m=m.value, n=n, nar=nar.value, cbst=cbst, datweight=datweight, norm=norm[:n], dws=dws.reshape(nblocks, 2))

    def iteration_system_maps_device(self, nx, ny, nmaps, nblocks, obst, dsyn, threshold0, weight0, weight_azi=None):
        """dsa_iteration_system_maps_device on the map rows left on the device.  Returns dict(m, n, nar, cbst (m,), datweight (dall,), norm (n,),
        dws (nblocks, 2)); afterwards lsmr(cbst, damp) solves on the resident matrix"""
        n = max(int(nblocks), 0) * max(int(nmaps), 0) * max(nx - 2, 0) * max(ny - 2, 0)
        return self._iteration_system_device(self._L.dsa_iteration_system_maps_device, (nx, ny, nmaps, nblocks), obst, dsyn,
                                             (threshold0, weight0, weight0 if weight_azi is None else weight_azi), n, n, max(int(nblocks), 1))

    def update_maps(self, dv, dvmax, minvel, maxvel, nmaps, nx, ny):
        """dsa_update_maps: dv, nmaps * (nx - 2) * (ny - 2) values (the c0 block of a solution; any shape), applied to the resident vertex maps of
        an nx x ny grid; plan again afterwards.  ValueError when dv does not hold exactly that many values: the library reads that many."""
        dv = np.ascontiguousarray(dv, np.float32)
        want = int(nmaps) * (int(nx) - 2) * (int(ny) - 2)
        if dv.size != want:
            raise ValueError("update_maps: dv holds %d values, %d maps of %d x %d vertices need %d" % (dv.size, int(nmaps), nx, ny, want))
        self._check(self._L.dsa_update_maps(self._h, int(nmaps), _p(dv), float(dvmax), float(minvel), float(maxvel)))

    def get_maps(self, nmaps, nx, ny):
        """the resident fp32 vertex maps, (nmaps, nx * ny) in set_maps' layout"""
        out = np.zeros((int(nmaps), nx * ny), np.float32)
        self._check(self._L.dsa_get_maps(self._h, int(nmaps), out.ctypes.data_as(_vp)))
        return out

    def maps_resolution(self, nx, ny, nmaps, nblocks, ndata, damp, r_map=-1):
        """dsa_maps_resolution on the resident map system (iteration_system_maps_device's, or a spmv_load of one in row order): the exact
        resolution and covariance of every map from one dense fp64 factorisation per map.  Returns dict(measures (9, nblocks, nmaps, layer)
        {R_qq, var, sum R^2 over the plane, that sum weighted with dx^2 and with dy^2 in vertex units, sum R^2 over the map, R at the
        co-located unknowns of the next two planes, the covariance with the next plane's}, leverage (ndata), trace (nblocks, nmaps), nused,
        flag (nmaps), and with r_map >= 0 R (n_m, n_m) of that map)."""
        layer = (int(nx) - 2) * (int(ny) - 2)
        nm = int(nblocks) * layer
        out = dict(measures=np.zeros((9, max(int(nblocks), 1), max(int(nmaps), 1), max(layer, 1))), leverage=np.zeros(max(int(ndata), 1)),
                   trace=np.zeros((max(int(nblocks), 1), max(int(nmaps), 1))), nused=np.zeros(max(int(nmaps), 1), np.int32), flag=np.zeros(max(int(nmaps), 1), np.int32))
        if r_map >= 0:
            out["R"] = np.zeros((max(nm, 1), max(nm, 1)))
        self._check(self._L.dsa_maps_resolution(self._h, int(nx), int(ny), int(nmaps), int(nblocks), int(ndata), float(damp), int(r_map), _p(out["measures"]),
                                                _p(out["leverage"]), _p(out["trace"]), _p(out["nused"]), _p(out["flag"]), _p(out["R"]) if r_map >= 0 else None))
        return out

    def set_azimuthal_slots(self, on):
        """on: one flag per depth-kernel slot, 0 = units of that slot emit no gc / gs entries; None = every slot emits"""
        if on is None:
            self._check(self._L.dsa_set_azimuthal_slots(self._h, 0, None))
            return
        on = np.ascontiguousarray(on, np.int32)
        self._check(self._L.dsa_set_azimuthal_slots(self._h, on.size, on.ctypes.data_as(_vp)))

    def ray_azimuths(self):
        """per traced ray of the last solve_rows_azimuthal, in data order: (datum (1-based), steps, sums (R, 2) of cos 2psi and sin 2psi)"""
        nr = int(self.stats()["rays"])
        datum = np.zeros(nr, np.int32); steps = np.zeros(nr, np.int32); sums = np.zeros((nr, 2), np.float32)
        self._check(self._L.dsa_ray_azimuths(self._h, datum.ctypes.data_as(_vp), steps.ctypes.data_as(_vp), sums.ctypes.data_as(_vp)))
        return datum, steps, sums

    def ray_paths(self, cap):
        """paths of the rays traced by the last solve_rows (set_option('ray_path_cap', cap) before it): list of
        (datum, points) with points an (n, 2) array of (latitude, longitude) in degrees, receiver first, source last --
        what the reference's disabled dump writes to raypath.out (CalSurfG.f90:2276-2283)"""
        nr = int(self.stats()["rays"])
        datum = np.zeros(nr, np.int32); npts = np.zeros(nr, np.int32); pts = np.zeros((nr, cap, 2), np.float32)
        self._check(self._L.dsa_ray_paths(self._h, _p(datum), _p(npts), _p(pts)))
        if (npts > cap).any():
            raise RuntimeError("ray_paths: a ray has %d points, more than ray_path_cap = %d" % (int(npts.max()), cap))
        return [(int(datum[r]), pts[r, :npts[r]].copy()) for r in range(nr)]

    # ---- dispersion stage ------------------------------------------------------------------------
    def dispersion_begin(self, vels, depz, minthk, kmax_total, nmaps_total):
        """vels: (nz, ny, nx) fp32"""
        vels = np.ascontiguousarray(vels, np.float32)
        nz, ny, nx = vels.shape
        self._disp = (nx, ny, nz)
        self._check(self._L.dsa_dispersion_begin(self._h, nx, ny, nz, _p(vels), _p(np.ascontiguousarray(depz, np.float32)),
                                                 float(minthk), int(kmax_total), int(nmaps_total)))

    def dispersion_begin_models(self, vels, depz, minthk, nmaps_per_model):
        """vels: (nmodels, nz, ny, nx) fp32 [Fortran vels(nx,ny,nz,nmodels)]: every dispersion_run afterwards computes all models in one
        launch; the maps are model-major (global map = model * nmaps_per_model + m: dispersion_fetch, plan's map_index)"""
        vels = np.ascontiguousarray(vels, np.float32)
        nm, nz, ny, nx = vels.shape
        self._disp = (nx, ny, nz)
        self._check(self._L.dsa_dispersion_begin_models(self._h, nx, ny, nz, nm, _p(vels), _p(np.ascontiguousarray(depz, np.float32)),
                                                        float(minthk), int(nmaps_per_model)))

    def dispersion_model_failures(self, nmodels):
        """dispersion curves without a root per model since dispersion_begin / dispersion_begin_models"""
        out = np.zeros(int(nmodels), np.int64)
        self._check(self._L.dsa_dispersion_model_failures(self._h, int(nmodels), out.ctypes.data_as(_vp)))
        return out

    def step_models(self, vsf, steps, minvel, maxvel, alpha=None, nmodels=None):
        """dsa_step_models: K models from the base model vsf (nx, ny, nz) and K steps (K, (nx-2)(ny-2)(nz-1)), what K dsa_model_update calls
        leave in copies of vsf (step k scaled by float32(alpha[k]) first where alpha is given), built on the device.  steps None: the
        solutions the last batch solve left on this engine, nmodels of them.  Returns (K, nx, ny, nz) float32."""
        vsf = np.asarray(vsf, np.float32)
        nx, ny, nz = vsf.shape
        base = np.ascontiguousarray(vsf.transpose(2, 1, 0))             # C order of Fortran vsf(nx, ny, nz)
        if steps is not None:
            steps = np.ascontiguousarray(steps, np.float32).reshape(-1, (nx - 2) * (ny - 2) * (nz - 1))
            K = steps.shape[0]
        else:
            K = int(nmodels)
        if alpha is not None:
            alpha = np.ascontiguousarray(alpha, np.float32)
            if alpha.size != K:
                raise ValueError("alpha has %d values for %d models" % (alpha.size, K))
        out = np.zeros((K, nz, ny, nx), np.float32)
        self._check(self._L.dsa_step_models(self._h, nx, ny, nz, K, _p(base), _p(steps), _p(alpha), float(minvel), float(maxvel), _p(out)))
        return out.transpose(0, 3, 2, 1)

    def dispersion_run(self, iwave, igr, t, kernels, sen_slot=0, map_first=0):
        t = np.ascontiguousarray(t, np.float64)
        self._check(self._L.dsa_dispersion_run(self._h, iwave, igr, t.size, _p(t), int(bool(kernels)), sen_slot, map_first))

    def dispersion_fetch(self, map_first, nper, kernels=False, sen_slot=0):
        nx, ny, nz = self._disp
        pv = np.zeros((nper, nx * ny))
        sen = [np.zeros((nz, nper, nx * ny)) for _ in range(3)] if kernels else [None] * 3
        self._check(self._L.dsa_dispersion_fetch(self._h, map_first, nper, _p(pv), int(bool(kernels)), sen_slot,
                                                 *[None if a is None else _p(a) for a in sen]))
        return (pv, *sen) if kernels else pv

    def maps_from_dispersion(self, goxd, gozd, dvxd, dvzd, dicing=8):
        self._check(self._L.dsa_maps_from_dispersion(self._h, goxd, gozd, dvxd, dvzd, dicing))
        a, b = _i32(), _i32()
        self._check(self._L.dsa_get_dims(self._h, C.byref(a), C.byref(b)))
        self.nnx, self.nnz = a.value, b.value

    def kernels_from_dispersion(self):
        self._check(self._L.dsa_kernels_from_dispersion(self._h))

    def _columns_in(self, who, obs, wt, models=0):
        """What opens every columns_* call: obs and wt as contiguous fp32 -- ValueError (in who's name) when they differ in size or do not
        fill whole maps: the library reads nmaps * nx * ny values of each -- and, for a step of 1 or 2 models, its zeroed outputs.  Returns
        (nmaps, obs, wt, dv, nused, chi2, flag), the last four None without models."""
        nx, ny, nz = self._disp
        ncol = nx * ny
        obs = np.ascontiguousarray(obs, np.float32)
        if ncol == 0 or obs.size == 0 or obs.size % ncol:
            raise ValueError("%s: obs holds %d values, not whole maps of %d x %d" % (who, obs.size, nx, ny))
        if wt is not None:
            wt = np.ascontiguousarray(wt, np.float32)
            if wt.size != obs.size:
                raise ValueError("%s: wt holds %d values, obs %d" % (who, wt.size, obs.size))
        lead = (2,) if models == 2 else ()
        outs = (np.zeros(lead + (nz - 1, ncol), np.float32), np.zeros(lead + (ncol,), np.int32), np.zeros(lead + (ncol,)), np.zeros(ncol, np.int32)) if models else (None,) * 4
        return (obs.size // ncol, obs, wt) + outs

    def _carried(self, nused, flag):
        """the interior columns without a used datum (of any type) that were stepped all the same: nused 0, flag 0"""
        nx, ny, _ = self._disp
        inner = np.zeros((ny, nx), bool); inner[1:-1, 1:-1] = True
        return int((inner.ravel() & (nused.reshape(-1, nx * ny).sum(axis=0) == 0) & (flag == 0)).sum())

    def columns_step(self, obs, wt, smooth, damp, dvmax, minvel, maxvel):
        """dsa_columns_step on the model of dispersion_begin: obs (nmaps, ny * nx) fp32 maps in get_maps' layout, wt the same shape or None
        (all 1).  Returns dict(dv (nz - 1, ny * nx) fp32, nused (ny * nx) int32, chi2 (ny * nx) fp64, flag (ny * nx) int32).  ValueError when
        obs and wt differ in size or do not fill whole maps: the library reads nmaps * nx * ny values of each."""
        nmaps, obs, wt, dv, nused, chi2, flag = self._columns_in("columns_step", obs, wt, 1)
        self._check(self._L.dsa_columns_step(self._h, nmaps, _p(obs), _p(wt), float(smooth), float(damp), float(dvmax), float(minvel), float(maxvel), _p(dv), _p(nused),
                                             _p(chi2), _p(flag)))
        return dict(dv=dv, nused=nused, chi2=chi2, flag=flag)

    def columns_resolution(self, obs, wt, smooth, damp, full=False):
        """dsa_columns_resolution on the state columns_step needs, which it leaves as it is: obs and wt as columns_step's.  Returns
        dict(measures (4, nz - 1, ny * nx): R_jj, m1, m2, var; leverage (nmaps, ny * nx); trace (ny * nx); nused, flag (ny * nx) int32; and
        with full=True R (nz - 1, nz - 1, ny * nx), R[l, j] the response at depth l to unknown j), all fp64.  ValueError as columns_step."""
        nmaps, obs, wt = self._columns_in("columns_resolution", obs, wt)[:3]
        nx, ny, nz = self._disp
        ncol = nx * ny
        out = dict(measures=np.zeros((4, nz - 1, ncol)), leverage=np.zeros((nmaps, ncol)), trace=np.zeros(ncol), nused=np.zeros(ncol, np.int32),
                   flag=np.zeros(ncol, np.int32))
        if full:
            out["R"] = np.zeros((nz - 1, nz - 1, ncol))
        self._check(self._L.dsa_columns_resolution(self._h, nmaps, _p(obs), _p(wt), float(smooth), float(damp), _p(out["measures"]), _p(out["leverage"]),
                                                   _p(out["trace"]), _p(out["R"]) if full else None, _p(out["nused"]), _p(out["flag"])))
        return out

    def columns_azimuthal(self, obs, a1, a2, wt, smooth, damp):
        """dsa_columns_azimuthal on the state columns_resolution needs, which it leaves as it is: obs (the c0 maps) and wt as columns_step's,
        a1 and a2 (the maps' 2 psi terms) in obs's layout.  Returns dict(gc, gs (nz - 1, ny * nx); measures (4, nz - 1, ny * nx): R_jj, m1, m2,
        var, one set for both components; leverage (nmaps, ny * nx), 0 at Love and unused slots; chi2 (4, ny * nx): before c, before s, after
        c, after s; nused, flag (ny * nx) int32), all else fp64.  ValueError as columns_step, and when a1 or a2 differ from obs in size."""
        nmaps, obs, wt = self._columns_in("columns_azimuthal", obs, wt)[:3]
        a1, a2 = np.ascontiguousarray(a1, np.float32), np.ascontiguousarray(a2, np.float32)
        if a1.size != obs.size or a2.size != obs.size:
            raise ValueError("columns_azimuthal: a1 holds %d values, a2 %d, obs %d" % (a1.size, a2.size, obs.size))
        nx, ny, nz = self._disp
        ncol = nx * ny
        g = np.zeros((2, nz - 1, ncol))
        out = dict(gc=g[0], gs=g[1], measures=np.zeros((4, nz - 1, ncol)), leverage=np.zeros((nmaps, ncol)), chi2=np.zeros((4, ncol)),
                   nused=np.zeros(ncol, np.int32), flag=np.zeros(ncol, np.int32))
        self._check(self._L.dsa_columns_azimuthal(self._h, nmaps, _p(obs), _p(a1), _p(a2), _p(wt), float(smooth), float(damp), _p(g), _p(out["measures"]),
                                                  _p(out["leverage"]), _p(out["chi2"]), _p(out["nused"]), _p(out["flag"])))
        return out

    def dispersion_get_model(self):
        """the dispersion stage's resident model, (nz, ny, nx) fp32 as dispersion_begin takes it"""
        nx, ny, nz = self._disp
        out = np.zeros((nz, ny, nx), np.float32)
        self._check(self._L.dsa_dispersion_get_model(self._h, out.ctypes.data_as(_vp)))
        return out

    # ---- Monte-Carlo depth inversion ----
    def columns_sample_begin(self, vels, depz, minthk, plan, obs, wt, nchains, smooth, step, spread, width, temperature, minvel, maxvel, seed, burn):
        """dsa_columns_sample_begin: a sample stage of nchains Metropolis chains per column, started at vels (nz, ny, nx) fp32, and its set-up
        sweep.  plan: [(wave type, velocity kind, periods), ...] in slot order (further items of an entry, as depth.slot_plan's first slot,
        are ignored: the maps are cumulative); obs (nmaps, ny * nx) fp32 as columns_step's, wt the same shape (1 / sigma, 0 drops a datum) or
        None (all 1).  ValueError as columns_step's."""
        vels = np.ascontiguousarray(vels, np.float32)
        nz, ny, nx = vels.shape
        was = self._disp
        self._disp = (nx, ny, nz)
        try:
            nmaps, obs, wt = self._columns_in("columns_sample_begin", obs, wt)[:3]
        finally:
            self._disp = was                                                        # (a refused begin leaves the open stage, and its shapes, as they were)
        iwave = np.array([int(r[0]) for r in plan], np.int32); igr = np.array([int(r[1]) for r in plan], np.int32)
        nper = np.array([np.size(r[2]) for r in plan], np.int32)
        t = np.ascontiguousarray(np.concatenate([np.asarray(r[2], np.float64).ravel() for r in plan]) if len(plan) else np.zeros(0), np.float64)
        self._check(self._L.dsa_columns_sample_begin(self._h, nx, ny, nz, int(nchains), _p(vels), _p(np.ascontiguousarray(depz, np.float32)), float(minthk), len(plan),
                                                     _p(iwave), _p(igr), _p(nper), _p(t), nmaps, _p(obs), _p(wt), float(smooth), float(step), float(spread), float(width),
                                                     float(temperature), float(minvel), float(maxvel), int(seed) & 0xFFFFFFFFFFFFFFFF, int(burn)))
        self._disp = (nx, ny, nz)
        self._sample = (int(nchains), nmaps)
        self._marginals = (0, False)

    def columns_sample_run(self, nsweeps):
        """dsa_columns_sample_run: nsweeps whole sweeps of every chain on the device"""
        self._check(self._L.dsa_columns_sample_run(self._h, int(nsweeps)))

    def columns_sample_fetch(self):
        """dsa_columns_sample_fetch: the finish of the present state.  Returns dict(mean, var, W, B, best (nz - 1, ny * nx) fp64; phi_start,
        best_energy, mean_phi (ny * nx) fp64; nused, flag, accepted, rejected, out_of_box, no_root, reseeded, nkept (ny * nx) int32); without
        a kept sweep (the ring, flag 2, burn >= the sweeps run) the node figures, best_energy and mean_phi are 0."""
        nx, ny, nz = self._disp
        ncol = nx * ny
        nodes = np.zeros((5, nz - 1, ncol)); cols = np.zeros((3, ncol)); counts = np.zeros((8, ncol), np.int32)
        self._check(self._L.dsa_columns_sample_fetch(self._h, _p(nodes), _p(cols), _p(counts)))
        out = dict(zip(("mean", "var", "W", "B", "best"), nodes))
        out.update(zip(("phi_start", "best_energy", "mean_phi"), cols))
        out.update(zip(("nused", "flag", "accepted", "rejected", "out_of_box", "no_root", "reseeded", "nkept"), counts))
        return out

    def columns_sample_state(self):
        """dsa_columns_sample_state: the raw per-chain state.  Returns dict(models (nz, C, ncol) fp32; phi, psi, phisum, best_e (C, ncol);
        counters (4, C, ncol) int32: accepted, rejected, out of box, no root; S1, S2 (nz - 1, C, ncol); best_v (nz - 1, C, ncol) fp32; nkept,
        pnode, pmark, reseeded (C, ncol) int32; pold (C, ncol) fp32)."""
        nx, ny, nz = self._disp
        ncol = nx * ny
        Cn = self._sample[0]
        if Cn < 1:                                                                  # (no stage was ever begun here: the library's refusal)
            self._check(self._L.dsa_columns_sample_state(self._h, *([None] * 14)))
        f64 = lambda *shape: np.zeros(shape)
        i32 = lambda *shape: np.zeros(shape, np.int32)
        f32 = lambda *shape: np.zeros(shape, np.float32)
        out = dict(models=f32(nz, Cn, ncol), phi=f64(Cn, ncol), psi=f64(Cn, ncol), counters=i32(4, Cn, ncol), S1=f64(nz - 1, Cn, ncol), S2=f64(nz - 1, Cn, ncol),
                   phisum=f64(Cn, ncol), nkept=i32(Cn, ncol), best_e=f64(Cn, ncol), best_v=f32(nz - 1, Cn, ncol), pnode=i32(Cn, ncol), pold=f32(Cn, ncol),
                   pmark=i32(Cn, ncol), reseeded=i32(Cn, ncol))
        self._check(self._L.dsa_columns_sample_state(self._h, *[_p(a) for a in out.values()]))
        return out

    # ---- Monte-Carlo radial depth inversion ----
    RADIAL_NODE_FIGURES = ("mean_v", "var_v", "W_v", "B_v", "mean_h", "var_h", "W_h", "B_h", "mean_xi", "var_xi", "W_xi", "B_xi", "best_v", "best_h", "cov_vh", "p_pos")
    RADIAL_COLUMN_COUNTS = ("nused_r", "nused_l", "flag", "accepted", "rejected", "out_of_box", "no_root", "proposed_v", "proposed_h", "proposed_pair", "accepted_v",
                            "accepted_h", "accepted_pair", "reseeded", "nkept")

    def columns_sample_radial_begin(self, vsv, vsh, depz, minthk, plan, obs, wt, nchains, smooth, aniso, step, spread, width, temperature, minvel, maxvel, seed,
                                    burn, pairs=True):
        """dsa_columns_sample_radial_begin: a radial sample stage of nchains Metropolis chains of [Vsv ; Vsh] per column, started at vsv, vsh
        (nz, ny, nx) fp32, and its set-up sweep.  plan, obs, wt as columns_sample_begin's: a slot of a run of wave type 1 (Love) is computed
        on a chain's Vsh, every other on its Vsv.  pairs: a third of the proposals move Vsv and Vsh of one depth together.  ValueError as
        columns_step's, and when vsh differs from vsv in shape."""
        vsv = np.ascontiguousarray(vsv, np.float32)
        nz, ny, nx = vsv.shape
        if vsh is not None:
            vsh = np.ascontiguousarray(vsh, np.float32)
            if vsh.shape != vsv.shape:
                raise ValueError("columns_sample_radial_begin: vsh is %s, vsv %s" % (vsh.shape, vsv.shape))
        was = self._disp
        self._disp = (nx, ny, nz)
        try:
            nmaps, obs, wt = self._columns_in("columns_sample_radial_begin", obs, wt)[:3]
        finally:
            self._disp = was                                                        # (a refused begin leaves the open stage, and its shapes, as they were)
        iwave = np.array([int(r[0]) for r in plan], np.int32); igr = np.array([int(r[1]) for r in plan], np.int32)
        nper = np.array([np.size(r[2]) for r in plan], np.int32)
        t = np.ascontiguousarray(np.concatenate([np.asarray(r[2], np.float64).ravel() for r in plan]) if len(plan) else np.zeros(0), np.float64)
        self._check(self._L.dsa_columns_sample_radial_begin(self._h, nx, ny, nz, int(nchains), _p(vsv), _p(vsh), _p(np.ascontiguousarray(depz, np.float32)), float(minthk),
                                                            len(plan), _p(iwave), _p(igr), _p(nper), _p(t), nmaps, _p(obs), _p(wt), float(smooth), float(aniso), float(step),
                                                            float(spread), float(width), float(temperature), float(minvel), float(maxvel),
                                                            int(seed) & 0xFFFFFFFFFFFFFFFF, int(burn), int(pairs)))
        self._disp = (nx, ny, nz)
        self._sample_radial = (int(nchains), nmaps)

    def columns_sample_radial_run(self, nsweeps):
        """dsa_columns_sample_radial_run: nsweeps whole sweeps of every chain on the device"""
        self._check(self._L.dsa_columns_sample_radial_run(self._h, int(nsweeps)))

    def columns_sample_radial_fetch(self):
        """dsa_columns_sample_radial_fetch: the finish of the present state.  Returns a dict of RADIAL_NODE_FIGURES (nz - 1, ny * nx) fp64 -- mean,
        var, W, B of Vsv (_v), Vsh (_h) and xi = (Vsh / Vsv)^2 (_xi), the best model, the pooled covariance of Vsv and Vsh, the share of kept
        states with Vsh > Vsv --, phi_start, best_energy, mean_phi (ny * nx) fp64 and RADIAL_COLUMN_COUNTS (ny * nx) int32; without a kept sweep
        the node figures, best_energy and mean_phi are 0."""
        nx, ny, nz = self._disp
        ncol = nx * ny
        nodes = np.zeros((16, nz - 1, ncol)); cols = np.zeros((3, ncol)); counts = np.zeros((15, ncol), np.int32)
        self._check(self._L.dsa_columns_sample_radial_fetch(self._h, _p(nodes), _p(cols), _p(counts)))
        out = dict(zip(self.RADIAL_NODE_FIGURES, nodes))
        out.update(zip(("phi_start", "best_energy", "mean_phi"), cols))
        out.update(zip(self.RADIAL_COLUMN_COUNTS, counts))
        return out

    def columns_sample_radial_state(self):
        """dsa_columns_sample_radial_state: the raw per-chain state.  Returns dict(vsv, vsh (nz, C, ncol) fp32; phi, psi (C, ncol); counters (4, C,
        ncol), kinds (6, C, ncol) int32: proposed per kind, accepted per kind; S1v, S2v, S1h, S2h, Pvh, X1, X2 (nz - 1, C, ncol); npos (nz - 1,
        C, ncol) int32; phisum (C, ncol); nkept (C, ncol) int32; best_e (C, ncol); best_vsv, best_vsh (nz - 1, C, ncol) fp32; pnode (C, ncol)
        int32; pold_v, pold_h (C, ncol) fp32; pmark, reseeded (C, ncol) int32)."""
        nx, ny, nz = self._disp
        ncol = nx * ny
        Cn = self._sample_radial[0]
        if Cn < 1:                                                                  # (no radial stage was ever begun here: the library's refusal)
            self._check(self._L.dsa_columns_sample_radial_state(self._h, *([None] * 24)))
        f64 = lambda *shape: np.zeros(shape)
        i32 = lambda *shape: np.zeros(shape, np.int32)
        f32 = lambda *shape: np.zeros(shape, np.float32)
        M = nz - 1
        out = dict(vsv=f32(nz, Cn, ncol), vsh=f32(nz, Cn, ncol), phi=f64(Cn, ncol), psi=f64(Cn, ncol), counters=i32(4, Cn, ncol), kinds=i32(6, Cn, ncol),
                   S1v=f64(M, Cn, ncol), S2v=f64(M, Cn, ncol), S1h=f64(M, Cn, ncol), S2h=f64(M, Cn, ncol), Pvh=f64(M, Cn, ncol), X1=f64(M, Cn, ncol), X2=f64(M, Cn, ncol),
                   npos=i32(M, Cn, ncol), phisum=f64(Cn, ncol), nkept=i32(Cn, ncol), best_e=f64(Cn, ncol), best_vsv=f32(M, Cn, ncol), best_vsh=f32(M, Cn, ncol),
                   pnode=i32(Cn, ncol), pold_v=f32(Cn, ncol), pold_h=f32(Cn, ncol), pmark=i32(Cn, ncol), reseeded=i32(Cn, ncol))
        self._check(self._L.dsa_columns_sample_radial_state(self._h, *[_p(a) for a in out.values()]))
        return out

    # ---- block proposals of the sample stage ----
    def columns_sample_shape(self, obs, wt, smooth, damp):
        """dsa_columns_sample_shape on the state columns_resolution needs, which it leaves as it is: obs and wt as columns_step's.  The engine
        keeps the shape for columns_sample_blocks.  Returns dict(tri (nz (nz - 1) / 2, ny * nx): the packed lower triangle of L, N's diagonal
        on its diagonal; r (nz - 1, ny * nx) = 1 / sqrt(d), fp64; flag (ny * nx) int32).  ValueError as columns_step."""
        nmaps, obs, wt = self._columns_in("columns_sample_shape", obs, wt)[:3]
        nx, ny, nz = self._disp
        ncol = nx * ny
        out = dict(tri=np.zeros((nz * (nz - 1) // 2, ncol)), r=np.zeros((nz - 1, ncol)), flag=np.zeros(ncol, np.int32))
        self._check(self._L.dsa_columns_sample_shape(self._h, nmaps, _p(obs), _p(wt), float(smooth), float(damp), _p(out["tri"]), _p(out["r"]), _p(out["flag"])))
        return out

    def columns_sample_blocks(self, block_every, block_scale):
        """dsa_columns_sample_blocks, between columns_sample_begin and the first sweep: every block_every-th sweep proposes a block shaped by
        the held shape, scaled by block_scale; 0 switches the block sweeps off"""
        self._check(self._L.dsa_columns_sample_blocks(self._h, int(block_every), float(block_scale)))

    def columns_sample_block_state(self):
        """dsa_columns_sample_block_state: dict(pold_all (nz - 1, C, ncol) fp32, block_counters (3, C, ncol) int32: proposed, accepted, out of
        the box)"""
        nx, ny, nz = self._disp
        Cn = self._sample[0]
        if Cn < 1:                                                                  # (no stage was ever begun here: the library's refusal)
            self._check(self._L.dsa_columns_sample_block_state(self._h, None, None))
        out = dict(pold_all=np.zeros((nz - 1, Cn, nx * ny), np.float32), block_counters=np.zeros((3, Cn, nx * ny), np.int32))
        self._check(self._L.dsa_columns_sample_block_state(self._h, _p(out["pold_all"]), _p(out["block_counters"])))
        return out

    # ---- posterior marginals of the sample stage ----
    def columns_sample_marginals(self, nbins, with_cov=False):
        """dsa_columns_sample_marginals, between columns_sample_begin and the first sweep: every sweep after burn counts each chain's value
        at each depth in one of nbins (2 .. 256) equal bins of the node's box and, with_cov, adds the products of its offsets from the start;
        nbins = 0 switches them off.  The sampler's own state keeps its bits."""
        self._check(self._L.dsa_columns_sample_marginals(self._h, int(nbins), int(with_cov)))
        self._marginals = (int(nbins), bool(with_cov) and int(nbins) > 0)

    def columns_sample_marginals_fetch(self, levels=(), hist=True, cov=None):
        """dsa_columns_sample_marginals_fetch: the finish of the present counts for the probabilities levels (at most 16, each inside (0, 1)).
        Returns dict(mode (nz - 1, ny * nx), quantiles (len(levels), nz - 1, ny * nx) fp64; hist (nbins, nz - 1, ny * nx) uint32, the counts
        pooled over the chains, unless hist is false; cov (nz (nz - 1) / 2, ny * nx) fp64, the packed lower triangle of the pooled
        covariance, where cov is true -- by default where columns_sample_marginals was called with_cov).  A node without a kept sweep has
        zeros."""
        nx, ny, nz = self._disp
        ncol, M = nx * ny, nz - 1
        nbins, with_cov = self._marginals
        cov = with_cov if cov is None else bool(cov)
        lv = np.ascontiguousarray(levels, np.float64).reshape(-1)
        figures = np.zeros((1 + lv.size, M, ncol))
        out = dict(mode=figures[0], quantiles=figures[1:])
        if hist:
            out["hist"] = np.zeros((max(nbins, 0), M, ncol), np.uint32)
        if cov:
            out["cov"] = np.zeros((M * (M + 1) // 2, ncol))
        self._check(self._L.dsa_columns_sample_marginals_fetch(self._h, int(lv.size), _p(lv) if lv.size else None, _p(out["hist"]) if hist and nbins > 0 else None,
                                                              _p(figures), _p(out["cov"]) if cov else None))
        return out

    def columns_sample_marginals_state(self):
        """dsa_columns_sample_marginals_state: dict(hist (nbins, nz - 1, C, ncol) uint32; with the covariance P (nz (nz - 1) / 2, C, ncol)
        fp64: the per-chain sums of d_i d_j, whose diagonal is S2)"""
        nx, ny, nz = self._disp
        ncol, M = nx * ny, nz - 1
        Cn = self._sample[0]
        nbins, with_cov = self._marginals
        if Cn < 1 or nbins < 1:                                                     # (no stage, or the marginals are off: the library's refusal)
            self._check(self._L.dsa_columns_sample_marginals_state(self._h, None, None))
        out = dict(hist=np.zeros((nbins, M, Cn, ncol), np.uint32))
        if with_cov:
            out["P"] = np.zeros((M * (M + 1) // 2, Cn, ncol))
        self._check(self._L.dsa_columns_sample_marginals_state(self._h, _p(out["hist"]), _p(out["P"]) if with_cov else None))
        return out

    def dispersion_begin_radial(self, vsv, vsh, depz, minthk, kmax_total, nmaps_total):
        """dsa_dispersion_begin_radial: vsv and vsh (nz, ny, nx) fp32 on one set of depths; afterwards the Love runs read vsh and the Rayleigh
        runs vsv.  ValueError when the two shapes differ."""
        vsv = np.ascontiguousarray(vsv, np.float32); vsh = np.ascontiguousarray(vsh, np.float32)
        if vsv.ndim != 3 or vsv.shape != vsh.shape:
            raise ValueError("dispersion_begin_radial: vsv is %r and vsh %r, both must be (nz, ny, nx)" % (vsv.shape, vsh.shape))
        nz, ny, nx = vsv.shape
        self._disp = (nx, ny, nz)
        self._check(self._L.dsa_dispersion_begin_radial(self._h, nx, ny, nz, _p(vsv), _p(vsh), _p(np.ascontiguousarray(depz, np.float32)), float(minthk),
                                                        int(kmax_total), int(nmaps_total)))

    def columns_step_radial(self, obs, wt, smooth, damp, aniso, dvmax, minvel, maxvel):
        """dsa_columns_step_radial on the models of dispersion_begin_radial: obs and wt as columns_step's.  Returns dict(dv_sv, dv_sh (nz - 1,
        ny * nx) fp32, nused (2, ny * nx) int32 and chi2 (2, ny * nx) fp64 -- Rayleigh, then Love -- flag (ny * nx) int32).  ValueError as
        columns_step."""
        nmaps, obs, wt, dv, nused, chi2, flag = self._columns_in("columns_step_radial", obs, wt, 2)
        self._check(self._L.dsa_columns_step_radial(self._h, nmaps, _p(obs), _p(wt), float(smooth), float(damp), float(aniso), float(dvmax), float(minvel), float(maxvel),
                                                    _p(dv), _p(nused), _p(chi2), _p(flag)))
        return dict(dv_sv=dv[0], dv_sh=dv[1], nused=nused, chi2=chi2, flag=flag)

    def columns_resolution_radial(self, obs, wt, smooth, damp, aniso, full=False):
        """dsa_columns_resolution_radial on the state columns_step_radial needs, which it leaves as it is: obs and wt as columns_step's.
        Returns dict(measures (6, 2 (nz - 1), ny * nx): R_jj, m1_own, m2_own, m1_cross, R_cross, var of the Vsv block's unknowns, then the
        Vsh block's; pair (2, nz - 1, ny * nx): cov, vard; leverage (nmaps, ny * nx); trace (2, ny * nx): the Vsv block's, the Vsh block's;
        nused (2, ny * nx) and flag (ny * nx) int32; and with full=True R (2 (nz - 1), 2 (nz - 1), ny * nx), R[i, j] the response of unknown
        i to a spike in unknown j), all fp64.  ValueError as columns_step."""
        nmaps, obs, wt = self._columns_in("columns_resolution_radial", obs, wt)[:3]
        nx, ny, nz = self._disp
        ncol, n2 = nx * ny, 2 * (nz - 1)
        out = dict(measures=np.zeros((6, n2, ncol)), pair=np.zeros((2, nz - 1, ncol)), leverage=np.zeros((nmaps, ncol)), trace=np.zeros((2, ncol)),
                   nused=np.zeros((2, ncol), np.int32), flag=np.zeros(ncol, np.int32))
        if full:
            out["R"] = np.zeros((n2, n2, ncol))
        self._check(self._L.dsa_columns_resolution_radial(self._h, nmaps, _p(obs), _p(wt), float(smooth), float(damp), float(aniso), _p(out["measures"]),
                                                          _p(out["pair"]), _p(out["leverage"]), _p(out["trace"]), _p(out["nused"]), _p(out["flag"]),
                                                          _p(out["R"]) if full else None))
        return out

    def columns_step_lateral(self, obs, wt, smooth, damp, lateral, dvmax, minvel, maxvel, tol=1e-8, maxit=500):
        """dsa_columns_step_lateral on the model of dispersion_begin: columns_step with the interior columns tied to their neighbours by the
        weight lateral (0: columns_step's bits), solved by preconditioned conjugate gradients to the relative tolerance tol in at most maxit
        iterations.  Returns columns_step's dict with itn, istop (1 converged, 2 maxit), rz0, rz and carried (the interior columns without a
        used datum that were stepped all the same: nused 0, flag 0) added.  ValueError as columns_step."""
        nmaps, obs, wt, dv, nused, chi2, flag = self._columns_in("columns_step_lateral", obs, wt, 1)
        info = np.zeros(4)
        self._check(self._L.dsa_columns_step_lateral(self._h, nmaps, _p(obs), _p(wt), float(smooth), float(damp), float(lateral), float(dvmax), float(minvel),
                                                     float(maxvel), float(tol), int(maxit), _p(dv), _p(nused), _p(chi2), _p(flag), _p(info)))
        return dict(dv=dv, nused=nused, chi2=chi2, flag=flag, itn=int(info[0]), istop=int(info[1]), rz0=float(info[2]), rz=float(info[3]),
                    carried=self._carried(nused, flag))

    def columns_resolution_lateral(self, obs, wt, smooth, damp, lateral, kind, index, models=None, tol=1e-8, maxit=500, full=False):
        """dsa_columns_resolution_lateral on the state columns_step_lateral needs, which it leaves as it is: obs and wt as columns_step's.  kind
        and index (nmembers) int32: 0 the point-spread function of unknown index = b (nz - 1) + l of interior column b, 1 row index of the
        averaging kernel and its variance, 2 the recovery of row index of models, 3 that row as the right-hand side; models (rows, nz - 1,
        interior columns) fp64 or None.  Returns dict(measures (nmembers, 7): val, m1, mz, mx, my, own, var; itn, istop (nmembers) int32; rz0, rz
        (nmembers); nused, flag (ny * nx) int32; and with full=True full (nmembers, nz - 1, interior columns): u of every member).  ValueError
        as columns_step, and when kind and index differ in size or models is not (rows, nz - 1, interior columns)."""
        nmaps, obs, wt = self._columns_in("columns_resolution_lateral", obs, wt)[:3]
        nx, ny, nz = self._disp
        ncol, nint = nx * ny, (nx - 2) * (ny - 2)
        kind = np.ascontiguousarray(kind, np.int32).ravel(); index = np.ascontiguousarray(index, np.int32).ravel()
        if kind.size != index.size:
            raise ValueError("columns_resolution_lateral: kind holds %d values, index %d" % (kind.size, index.size))
        nrows = 0
        if models is not None:
            models = np.ascontiguousarray(models, np.float64)
            if models.ndim != 3 or models.shape[1:] != (nz - 1, nint):
                raise ValueError("columns_resolution_lateral: models is %r, not (rows, %d, %d)" % (models.shape, nz - 1, nint))
            nrows = models.shape[0]
        n = kind.size
        measures = np.zeros((n, 7)); info = np.zeros((n, 4))
        out = dict(measures=measures, nused=np.zeros(ncol, np.int32), flag=np.zeros(ncol, np.int32))
        if full:
            out["full"] = np.zeros((n, nz - 1, nint))
        self._check(self._L.dsa_columns_resolution_lateral(self._h, nmaps, _p(obs), _p(wt), float(smooth), float(damp), float(lateral), float(tol), int(maxit), n,
                                                           _p(kind), _p(index), _p(models), nrows, _p(measures), _p(info), _p(out["full"]) if full else None,
                                                           _p(out["nused"]), _p(out["flag"])))
        out.update(itn=info[:, 0].astype(np.int32), istop=info[:, 1].astype(np.int32), rz0=info[:, 2].copy(), rz=info[:, 3].copy())
        return out

    def columns_step_radial_lateral(self, obs, wt, smooth, damp, aniso, lateral, lateral_aniso, dvmax, minvel, maxvel, tol=1e-8, maxit=500):
        """dsa_columns_step_radial_lateral on the models of dispersion_begin_radial: columns_step_radial with the interior columns tied to their
        neighbours -- both stepped models by the weight lateral, the stepped anisotropy field Vsh - Vsv by the weight lateral_aniso (both 0:
        columns_step_radial's bits) -- solved by preconditioned conjugate gradients to the relative tolerance tol in at most maxit iterations.
        Returns columns_step_radial's dict with itn, istop (1 converged, 2 maxit), rz0, rz and carried (the interior columns without a used
        datum of either type that were stepped all the same: nused 0 0, flag 0) added.  ValueError as columns_step."""
        nmaps, obs, wt, dv, nused, chi2, flag = self._columns_in("columns_step_radial_lateral", obs, wt, 2)
        info = np.zeros(4)
        self._check(self._L.dsa_columns_step_radial_lateral(self._h, nmaps, _p(obs), _p(wt), float(smooth), float(damp), float(aniso), float(lateral), float(lateral_aniso),
                                                            float(dvmax), float(minvel), float(maxvel), float(tol), int(maxit), _p(dv), _p(nused), _p(chi2), _p(flag),
                                                            _p(info)))
        return dict(dv_sv=dv[0], dv_sh=dv[1], nused=nused, chi2=chi2, flag=flag, itn=int(info[0]), istop=int(info[1]), rz0=float(info[2]), rz=float(info[3]),
                    carried=self._carried(nused, flag))

    def dispersion_get_model_radial(self):
        """the radial stage's two resident models, (vsv, vsh), each (nz, ny, nx) fp32"""
        nx, ny, nz = self._disp
        vsv = np.zeros((nz, ny, nx), np.float32); vsh = np.zeros((nz, ny, nx), np.float32)
        self._check(self._L.dsa_dispersion_get_model_radial(self._h, vsv.ctypes.data_as(_vp), vsh.ctypes.data_as(_vp)))
        return vsv, vsh

    # ---- radial anisotropy in the direct inversion --------------------------
    def kernels_from_dispersion_radial(self):
        """dsa_kernels_from_dispersion_radial: the depth factors of the Frechet rows on a radial stage, every slot from the model of its
        wave type; every slot must carry kernels of the present models"""
        self._check(self._L.dsa_kernels_from_dispersion_radial(self._h))

    def solve_rows_radial(self, capacity):
        """solve_rows with the columns of the units on Love slots moved into the Vsh block (dsa_solve_rows_radial): column
        B * maxvp + isotropic column, B = 0 (Vsv, Rayleigh), 1 (Vsh, Love); returns (times, rw, row, col)"""
        return self._solve_rows(self._L.dsa_solve_rows_radial, (), capacity)

    def solve_rows_radial_device(self, capacity=1 << 62):
        """solve_rows_radial with the rows left on the device for iteration_system_radial_device: returns (times, number of entries)"""
        return self._solve_rows(self._L.dsa_solve_rows_radial, (), capacity, host=False)

    def iteration_system_radial_device(self, nx, ny, nz, obst, dsyn, threshold0, weight0, weight_h=None, aniso=0.0):
        """dsa_iteration_system_radial_device on the radial rows left on the device.  Returns dict(m, n, nar, cbst (m,), datweight (dall,),
        norm (n,), dws (2, 2)); afterwards lsmr(cbst, damp) solves on the resident matrix"""
        maxvp = max(nx - 2, 0) * max(ny - 2, 0) * max(nz - 1, 0)
        return self._iteration_system_device(self._L.dsa_iteration_system_radial_device, (nx, ny, nz), obst, dsyn,
                                             (threshold0, weight0, weight0 if weight_h is None else weight_h, aniso), 2 * maxvp, 3 * maxvp, 2)

    def update_radial(self, dv, dvmax, minvel, maxvel):
        """dsa_update_radial: dv, 2 (nx - 2)(ny - 2)(nz - 1) values (the Vsv block then the Vsh block of a solution; any shape), applied to the
        two resident models of dispersion_begin_radial; the runs and kernels_from_dispersion_radial again afterwards.  ValueError when dv
        does not hold exactly that many values: the library reads that many."""
        nx, ny, nz = self._disp
        dv = np.ascontiguousarray(dv, np.float32)
        want = 2 * max(nx - 2, 0) * max(ny - 2, 0) * max(nz - 1, 0)
        if dv.size != want:
            raise ValueError("update_radial: dv holds %d values, two models of %d x %d x %d nodes need %d" % (dv.size, nx, ny, nz, want))
        self._check(self._L.dsa_update_radial(self._h, nx, ny, nz, _p(dv), float(dvmax), float(minvel), float(maxvel)))

    # ---- matrix-vector products of the inversion step (reference aprod) ---------------------------
    def spmv_load(self, m, n, rw, row, col):
        """COO matrix with 1-based row / col indices"""
        rw = np.ascontiguousarray(rw, np.float32)
        row = np.ascontiguousarray(row, np.int32)
        col = np.ascontiguousarray(col, np.int32)
        self._mn = (int(m), int(n))
        self._check(self._L.dsa_spmv_load(self._h, int(m), int(n), rw.size, _p(rw), _p(row), _p(col)))

    def spmv(self, mode, x, y):
        """mode 1: returns y + A x; mode 2: returns x + A^T y (fp32, the reference's accumulation order)"""
        x = np.array(x, np.float32, copy=True)
        y = np.array(y, np.float32, copy=True)
        assert x.size == self._mn[1] and y.size == self._mn[0]
        self._check(self._L.dsa_spmv(self._h, int(mode), _p(x), _p(y)))
        return y if mode == 1 else x

    def lsmr(self, b, damp, atol=1e-6, btol=1e-6, conlim=100.0, itnlim=400, local_size=10):
        """LSMR (reference lsmrModule.f90:36, arguments of main.f90:470-489) on the matrix of the last spmv_load;
        returns dict(x, istop, itn, normA, condA, normr, normAr, normx)"""
        b = np.ascontiguousarray(b, np.float32)
        assert b.size == self._mn[0]
        x = np.zeros(self._mn[1], np.float32)
        ii = [C.c_int(-1), C.c_int(-1)]
        ff = [C.c_float(0.0) for _ in range(5)]
        self._check(self._L.dsa_lsmr(self._h, _p(b), damp, atol, btol, conlim, int(itnlim), int(local_size), _p(x),
                                     *[C.byref(v) for v in ii], *[C.byref(v) for v in ff]))
        return dict(x=x, istop=ii[0].value, itn=ii[1].value, **{k: np.float32(v.value) for k, v in zip(EST_NAMES, ff)})

    def _batch(self, fn, R, head, solve, **out):
        """One call of a batch entry point: fn(handle, *head, atol, btol, conlim, itnlim, localSize, *out, istop, itn, est) for R solves,
        arrays passed by pointer and None as NULL.  Returns dict(**out, istop=(R,), itn=(R,), one (R,) array per name of EST_NAMES)."""
        ptr = lambda a: _p(a) if isinstance(a, np.ndarray) else a
        istop, itn, est = np.zeros(R, np.int32), np.zeros(R, np.int32), np.zeros((R, 5), np.float32)
        atol, btol, conlim, itnlim, local_size = solve
        self._check(fn(self._h, *map(ptr, head), atol, btol, conlim, int(itnlim), int(local_size), *map(ptr, out.values()), ptr(istop), ptr(itn), ptr(est)))
        return dict(**out, istop=istop, itn=itn, **{k: est[:, j].copy() for j, k in enumerate(EST_NAMES)})

    def lsmr_batch(self, b, row_scale, damp, atol=1e-6, btol=1e-6, conlim=100.0, itnlim=400, local_size=10):
        """R LSMR solves on the matrix of the last spmv_load: realisation r with its rows scaled by row_scale[r] (shape (R, m)),
        each bit-identical to lsmr() on that explicitly scaled system.  Returns dict(x=(R, n), istop=(R,), itn=(R,), normA=(R,), condA,
        normr, normAr, normx)"""
        b = np.ascontiguousarray(b, np.float32)
        s = np.ascontiguousarray(row_scale, np.float32)
        m, n = self._mn
        assert b.size == m and s.ndim == 2 and s.shape[1] == m
        R = s.shape[0]
        x = np.zeros((R, n), np.float32)
        return self._batch(self._L.dsa_lsmr_batch, R, (R, b, s, damp), (atol, btol, conlim, itnlim, local_size), x=x)

    def lsmr_resolution(self, ndata, damp, models=None, spikes=None, coords=None, want_x=True, atol=1e-6, btol=1e-6, conlim=100.0, itnlim=400,
                        local_size=10):
        """R LSMR solves on the matrix of the last spmv_load whose right-hand sides the device forms from test models: A m_r on the
        rows below ndata, 0 from ndata up; each bit-identical to lsmr() on that right-hand side.  models: (R, n) host models, or
        spikes = (first, R): the unit spikes at unknowns first .. first + R - 1; with spikes, coords ((n, 3) latitude, longitude,
        depth) adds the PSF measures.  Returns dict(x=(R, n) or None when not want_x, psf=(R, 4) or None, istop=(R,), itn=(R,),
        normA=(R,), condA, normr, normAr, normx)"""
        m, n = self._mn
        mod = None if models is None else np.ascontiguousarray(models, np.float32)
        if mod is not None:
            assert mod.ndim == 2 and mod.shape[1] == n
            first, R = 0, mod.shape[0]
        else:
            first, R = int(spikes[0]), int(spikes[1])
        xyz = None if coords is None else np.ascontiguousarray(coords, np.float64)
        x = np.zeros((R, n), np.float32) if want_x else None
        psf = np.zeros((R, 4)) if xyz is not None else None
        return self._batch(self._L.dsa_lsmr_resolution, R, (R, int(ndata), mod, first, xyz, damp), (atol, btol, conlim, itnlim, local_size), x=x, psf=psf)

    def lsmr_resolution_blocks(self, ndata, damp, nblocks, spikes, coords, want_x=True, atol=1e-6, btol=1e-6, conlim=100.0, itnlim=400, local_size=10):
        """lsmr_resolution's spike solves with the PSF measures per parameter block (dsa_resolution_blocks): the n unknowns are nblocks
        blocks of n / nblocks cells, coords ((n / nblocks, 3) latitude, longitude, depth) per cell, spikes = (first, R).  Returns
        dict(x=(R, n) or None when not want_x, psf=(R, nblocks, 4) {x_r at the spike's cell in block B, sum x^2, sum x^2 dh^2, sum x^2 dz^2
        over block B}, istop=(R,), itn=(R,), normA=(R,), condA, normr, normAr, normx)"""
        m, n = self._mn
        first, R = int(spikes[0]), int(spikes[1])
        xyz = None if coords is None else np.ascontiguousarray(coords, np.float64)
        x = np.zeros((R, n), np.float32) if want_x else None
        psf = np.zeros((R, max(int(nblocks), 1), 4))
        return self._batch(self._L.dsa_resolution_blocks, R, (R, int(ndata), int(nblocks), first, xyz, damp), (atol, btol, conlim, itnlim, local_size), x=x, psf=psf)

    def lsmr_tradeoff(self, b, ndata, weight0, weights, damps, want_x=True, atol=1e-6, btol=1e-6, conlim=100.0, itnlim=400, local_size=10):
        """K LSMR solves on the matrix of the last spmv_load, whose rows from ndata up are regularisation rows built with weight0:
        member k on the system with those rows rebuilt with weights[k] (entries fl(c * weights[k]), c their integer coefficient) and
        damping damps[k], each bit-identical to lsmr(b, damps[k]) on that system.  Returns dict(x=(K, n) or None when not want_x,
        measures=(K, 3) float64 {sum of squared data residuals, sum of squared C x (unweighted roughness), sum of x^2}, istop=(K,),
        itn=(K,), normA=(K,), condA, normr, normAr, normx)"""
        b = np.ascontiguousarray(b, np.float32)
        w = np.ascontiguousarray(weights, np.float32).ravel()
        d = np.ascontiguousarray(damps, np.float32).ravel()
        m, n = self._mn
        assert b.size == m and w.size == d.size
        K = w.size
        x = np.zeros((K, n), np.float32) if want_x else None
        meas = np.zeros((K, 3))
        return self._batch(self._L.dsa_lsmr_tradeoff, K, (K, int(ndata), b, weight0, w, d), (atol, btol, conlim, itnlim, local_size), x=x, measures=meas)

    def lsmr_crossval(self, b, ndata, weight0, weights, damps, fold, nfolds, want_x=True, want_resid=True, atol=1e-6, btol=1e-6, conlim=100.0,
                      itnlim=400, local_size=10):
        """K-fold cross-validation of the combos (weights[q], damps[q]) on the matrix of the last spmv_load (rows from ndata up built with
        weight0, as for lsmr_tradeoff): K = ncombo * (nfolds + 1) solves, member q * (nfolds + 1) + f without the data rows i with
        fold[i] == f (f == nfolds: with all of them), each bit-identical to lsmr() on the system with those rows zeroed and the
        regularisation rows rebuilt with weights[q].  Returns dict(x=(K, n) or None when not want_x, measures=(K, 4) float64 {kept misfit,
        held-out misfit, unweighted roughness, sum of x^2 (sums of squares)}, resid=(ncombo, 2, ndata) float64 {held-out, full-fit residual
        of every datum} or None when not want_resid, istop=(K,), itn=(K,), normA=(K,), condA, normr, normAr, normx)"""
        b = np.ascontiguousarray(b, np.float32)
        w = np.ascontiguousarray(weights, np.float32).ravel()
        d = np.ascontiguousarray(damps, np.float32).ravel()
        fo = np.ascontiguousarray(fold, np.int32).ravel()
        m, n = self._mn
        assert b.size == m and w.size == d.size and fo.size >= min(max(int(ndata), 0), m)
        nc, nd = w.size, max(int(ndata), 0)
        K = nc * (max(int(nfolds), 0) + 1)
        x = np.zeros((K, n), np.float32) if want_x else None
        meas = np.zeros((K, 4))
        resid = np.zeros((nc, 2, nd)) if want_resid else None
        return self._batch(self._L.dsa_lsmr_crossval, K, (nc, int(nfolds), int(ndata), b, weight0, w, d, fo), (atol, btol, conlim, itnlim, local_size),
                           x=x, measures=meas, resid=resid)

    def lsmr_voronoi(self, b, ndata, ncells, xyz, seeds, damp, want_z=True, want_cell=True, want_stats=True, atol=1e-6, btol=1e-6, conlim=100.0,
                     itnlim=400, local_size=10):
        """K LSMR solves on random Voronoi projections of the data rows (rows below ndata) of the matrix of the last spmv_load: member k
        on M_k, those rows with every column j relabelled cell_k(j), the nearest (fp64 squared distance between rows of xyz (n, 3),
        lowest index on ties) of its seeds[k] (seeds: (K, ncells) 0-based unknowns); each bit-identical to lsmr(b[:ndata], damp) after
        spmv_load(ndata, ncells, M_k).  Returns dict(z=(K, ncells) or None, cell=(K, n) int32 or None, stats=(2, n) float64 {mean, sample
        standard deviation over the members of z_k[cell_k(j)]} or None, istop=(K,), itn=(K,), normA=(K,), condA, normr, normAr, normx)"""
        b = np.ascontiguousarray(b, np.float32)
        m, n = self._mn
        pts = np.ascontiguousarray(xyz, np.float64)
        sd = np.ascontiguousarray(seeds, np.int32)
        assert b.size >= min(int(ndata), m) and pts.shape == (n, 3) and sd.ndim == 2
        K = sd.shape[0]
        assert ncells < 1 or sd.shape[1] == ncells
        z = np.zeros((K, max(int(ncells), 0)), np.float32) if want_z else None
        cell = np.zeros((K, n), np.int32) if want_cell else None
        stats = np.zeros((2, n)) if want_stats else None
        return self._batch(self._L.dsa_lsmr_voronoi, K, (K, int(ndata), int(ncells), b, pts, sd, damp), (atol, btol, conlim, itnlim, local_size),
                           z=z, cell=cell, stats=stats)

    def traveltimes(self, map_index, scx, scz, nrec, rcx, rcz):
        self.plan(map_index, scx, scz, nrec, rcx, rcz)
        return self.solve()

    def keep_fields(self, on):
        """keep every planned unit's fields resident after a solve (field / refined of any unit); plan fails when they do not fit one chunk"""
        self._check(self._L.dsa_keep_fields(self._h, int(bool(on))))

    def ray_diagnostics(self):
        """rays of the last solve_rows clamped at the model edge (reference rbint) and the planned unit of the first of them (-1: none)"""
        n, u = C.c_longlong(0), _i32(0)
        self._check(self._L.dsa_ray_diagnostics(self._h, C.byref(n), C.byref(u)))
        return n.value, u.value

    def field(self, unit):
        """coarse travel-time field of a unit of the last chunk, indexed [ix, iz]"""
        out = np.zeros((self.nnx, self.nnz), np.float32)
        self._check(self._L.dsa_get_field(self._h, int(unit), _p(out)))
        return out

    def velocity(self, m):
        out = np.zeros((self.nnx, self.nnz), np.float32)
        self._check(self._L.dsa_get_velocity(self._h, int(m), _p(out)))
        return out

    def refined(self, unit):
        t = np.zeros(129 * 129, np.float32)
        s = np.zeros(129 * 129, np.int8)
        a, b = _i32(), _i32()
        self._check(self._L.dsa_get_refined(self._h, int(unit), C.byref(a), C.byref(b), _p(t), _p(s)))
        n = a.value * b.value
        return t[:n].reshape(a.value, b.value).copy(), s[:n].reshape(a.value, b.value).copy()

    def debug_field(self, unit, which):
        """raw device state of a resident unit (see dsa_debug_field); coarse fields come back [ix, iz]"""
        out = np.zeros((self.nnx, self.nnz) if which < 2 else (129 * 129,), np.float32)
        self._check(self._L.dsa_debug_field(self._h, int(unit), int(which), _p(out)))
        return out

    def debug_counters(self):
        out = np.zeros(24, np.float64)
        self._check(self._L.dsa_debug_counters(self._h, _p(out)))
        return out

    def unit_ties(self):
        """per unit of the last solve: flags (bit 0 met an exact tie, bit 1 solved by the literal march) and the largest tie influence (s)"""
        n = len(self._nrec_of_plan)
        fl = np.zeros(n, np.int32); inf = np.zeros(n, np.float32)
        self._check(self._L.dsa_unit_ties(self._h, n, _p(fl), _p(inf)))
        return fl, inf

    def unit_tie_sums(self):
        """per unit of the last solve: ties with an influence, the sum of their influences (s), cycles frozen by the unit or its bundle"""
        n = len(self._nrec_of_plan)
        cnt = np.zeros(n, np.int32); sm = np.zeros(n, np.float32); fr = np.zeros(n, np.int32)
        self._check(self._L.dsa_unit_tie_sums(self._h, n, _p(cnt), _p(sm), _p(fr)))
        return cnt, sm, fr

    def unit_rounds(self):
        """rounds of each unit's coarse solve in the last solve"""
        n = len(self._nrec_of_plan)
        r = np.zeros(n, np.int32)
        self._check(self._L.dsa_unit_rounds(self._h, n, _p(r)))
        return r

    def stats(self):
        out = np.zeros(64, np.float64)
        self._check(self._L.dsa_get_stats(self._h, _p(out)))
        d = dict(zip(STAT_NAMES, out[:len(STAT_NAMES)].tolist()))
        d["phase_ticks"] = out[len(STAT_NAMES):len(STAT_NAMES) + 8].tolist()
        return d
