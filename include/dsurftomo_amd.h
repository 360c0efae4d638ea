/* dsurftomo_amd -- C ABI of the MI355X forward-modelling engine for DSurfTomo's CalSurfG path.
 *
 * Plain C, pointers and sizes only.  Two levels:
 *
 *   (1) Drop-in level: dsa_calsurfg / dsa_synthetic take exactly the argument lists of the
 *       reference's Fortran subroutines CalSurfG (reference src/CalSurfG.f90:939-943, argument
 *       declarations :987-1002) and synthetic (:2412-2415, :2460-2472): every argument by
 *       pointer, arrays column-major, 1-based indices in iw/col.  The Fortran shim
 *       dsurftomo_amd/fortran/calsurfg_shim.f90 exports the link symbols `calsurfg_` and
 *       `synthetic_` that the reference's main program imports (main.f90:355-359, :338-342) and
 *       forwards to these two functions.  See INTEGRATION.md.
 *
 *   (2) Engine level (own design): an explicit context, phase-velocity maps given per period
 *       slot (this is what the benchmark and the parity tests at synthetic sizes use: "identical
 *       grids" by construction), and batched (period, source) units.
 *
 * All functions return 0 on success or a negative dsa_status; dsa_error_string() gives the text.
 * Where the reference prints a message and STOPs (source or receiver outside the model,
 * CalSurfG.f90:1214-1220, :1686-1692, :1898-1904) the engine returns DSA_ERR_OUTSIDE and the shim
 * prints the reference's message and stops the program, so callers see the same behaviour.
 * There is no CPU fallback: without a usable GPU every entry point fails with DSA_ERR_DEVICE.
 */
#ifndef DSURFTOMO_AMD_H
#define DSURFTOMO_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dsa_engine dsa_engine;

enum dsa_status {
    DSA_OK = 0,
    DSA_ERR_DEVICE = -1,     /* no GPU / HIP runtime error */
    DSA_ERR_ARGUMENT = -2,
    DSA_ERR_OUTSIDE = -3,    /* a source or receiver lies outside the model */
    DSA_ERR_INTERNAL = -4,   /* a device-side guard fired (window / tree overflow, no convergence) */
    DSA_ERR_STATE = -5,      /* call order (e.g. solve before plan) */
    DSA_ERR_CAPACITY = -6    /* an output array is too small (the reference: stop 'increase sparsity fraction') */
};

/* ---- context ------------------------------------------------------------------------------- */
int dsa_create(dsa_engine** out, int device_index);
void dsa_destroy(dsa_engine* e);
const char* dsa_error_string(const dsa_engine* e);   /* e may be NULL: last creation error */
/* memory the engine may use for per-source fields (bytes, 0 = default: 60 % of free HBM, at most 150 GB) */
int dsa_set_memory_budget(dsa_engine* e, size_t bytes);

/* Options (dsa_set_option; every value is a double).  Defaults in [brackets]; DSA_ERR_ARGUMENT for an unknown name or a value out of range.
 *
 *   tie handling (see dsa_unit_ties below)
 *     exact_ties               [1]     0 fixed point only | 1 fixed point + tie census + the reference's march for the flagged units | 2 the march for every unit
 *     tie_threshold            [2e-5]  seconds: the influence on its node's value a tie must have to flag its unit; 0 = any tie
 *     tie_detect               [1]     exact_ties = 0 runs the census too and reports what it would have flagged (DSA_STAT_TIE_UNITS, dsa_unit_ties); 0 = off
 *     tie_map_strict           [1]     on a map where some unit holds a tie above tie_threshold, every unit holding a tie with any influence is flagged; 0 = the per-unit rule alone
 *     tie_scale_guard          [1]     a unit that holds a tie and whose travel times lie outside the envelope in which the fixed point's tie errors were measured to stay
 *                                      within tie_tolerance (26 ulps of the time on grids up to 1025 nodes per side, growing with the grid beyond) is flagged; 0 = off
 *     tie_tolerance            [1e-4]  seconds: the bar that envelope is held to (a lower value marches more units)
 *     handoff_replay           [1]     a unit in which a node ranks equal with the one that ended the refined stage, and the choice changes what the coarse grid receives, has its
 *                                      refined box (<= 129^2 nodes) marched literally and is handed off from that (up to 256 units a launch); 0 = such a unit is flagged (marched whole)
 *     tie_sum_threshold        [0]     seconds: a unit whose ties' influences add up to more than this is flagged; 0 = off (measured: separates nothing, see dsa_unit_tie_sums)
 *     tie_count_threshold      [0]     a unit holding more ties with an influence than this is flagged; 0 = off
 *     tie_frozen_bundles       [0]     1 = every member of a bundle that froze a cycle is flagged (a unit-by-unit solve that froze one always is)
 *     exact_lds_slots          [0]     tree slots kept in LDS per marching unit, 63 .. 4975 (made odd); 0 = what lets every wavefront of a batch be resident
 *     exact_heap_blocked       [1]     the march's tree beyond its LDS part stored in blocks of three levels: 0 never | 1 batches that fill the chip (>= 12 wavefronts per CU) | 2 whenever the LDS part is whole levels
 *     exact_pool               [0]     units marching at a time, up to 65535; 0 = by free memory, at most exact_pool_max
 *     exact_pool_max           [16384] 4 .. 32768
 *     exact_tiles              [0]     times-only calls: 0 = the march keeps pooled 8x8-node tiles per unit instead of whole fields when whole fields would bound the
 *                                      units marching side by side (4097^2: 3 MB per unit instead of 67) | 1 always | -1 never
 *     exact_tile_cap           [0]     tiles per marching unit, 64 .. 65000; 0 = 8 (tiles per grid side, both sides added)
 *
 *   fixed-point solve, unit by unit (csrc/fim_kernel.hip)
 *     window_cells             [1.25]  causal window in cell travel times
 *     fim_threads              [0]     workgroup size 128 | 256 | 512 | 1024; 0 = by grid size (128 up to 700 nodes per side, 256 up to 1500, 512 up to 3000, 1024 beyond)
 *     fim_sorted               [1]     refined boxes: 1 tile masks walked in record order | 0 lists in activation order (same fixed point)
 *     fim_lds_pad              [0]     extra dynamic LDS bytes per workgroup (limits the workgroups resident per CU; experiments)
 *     list_cap, ready_cap      [0]     active-list sizes of the list variant; 0 = from the grid, else at least 512 / 256
 *     field_pool               [0]     coarse field slots: 0 = four times the workgroups the GPU holds (a call with more units recycles them: a workgroup
 *                                      claims a free slot by compare-and-swap, resets it, solves, writes its unit's receiver times, frees it) | -1 one per
 *                                      unit | n > 0.  Fields stay readable (dsa_get_field) only when the call's units fit the slots; calls that need the
 *                                      fields afterwards (rows, exact_ties = 2, keep_fields) never recycle
 *     exc_log2cap              [0]     log2 of the exception table's entries, 6 .. 24; 0 = from the grid (the table grows by itself when it overflows)
 *     max_chunk                [0]     cap on units resident per launch; 0 = memory budget only
 *
 *   bundles: the periods of one source solved by one workgroup under one shared round schedule (csrc/bundle_kernel.hip).  Same travel times as unit by
 *   unit -- the fixed point does not depend on the schedule; a field with exact ties has two self-consistent states there and the two solves can settle
 *   differently (measured: identical on the headline and checkerboard media, 4 of 262 144 times apart by up to 4.2e-5 s on unrelated random maps)
 *     bundle                   [1]     1 automatic: 16 / 8 / 4 members, whichever the launch-time model promises most for the call's sources and periods,
 *                                      on grids of at least 120 nodes per side (below 400: only launches of at least 384 bundles of 8 or 16) | 0 off | 4, 8, 16
 *     bundle_window_cells      [0]     causal window of the bundles; 0 = 0.6 (768 threads wide: 1.0 for bundles of 16, 1.75 for bundles of 8 or 4)
 *     bundle_threads           [0]     256 | 512 | 768; 0 = 256 (three workgroups per CU), 768 beyond 1500 nodes per side and for launches of at most 256 bundles
 *     bundle_members_per_lane  [0]     4 | 2; 0 = four for bundles of 16, two for bundles of 8 / 4 in launches of more than 512
 *     bundle_pool              [0]     bundle field slots; 0 = the bundles resident at a time and an eighth more, within the memory budget
 *     bundle_tail              [1]     a launch of 768 .. 1500 bundles, the ones beyond the first generation (768 = three workgroups per CU): 1 whole and 768 threads
 *                                      wide on a second stream, a CU each, when there are at most 256 of them | 0 cut in halves (256 threads; also beyond 256)
 *     bundle_refined           [1]     the 129^2 refined boxes of bundled units in bundles too, in launches of at least 128 bundles | 0 unit by unit | 2 always
 *     bundle_max_rounds        [0]     round limit of a bundle; 0 = the solver's own.  A bundle that hits it sends its chunk to the unit-by-unit solve (tests)
 *     bundle_far_all           [0]     1 = every node trip fetches all four outer neighbours (round 4's loads; A/B switch)
 *
 *   rays, rows, dispersion, inversion step
 *     ray_budget               [0]     bytes of per-ray vertex slabs per launch of the tracer; 0 = a third of free HBM, up to 40 GB
 *     ray_lanes                [0]     lanes that trace a ray together: 0 = by the size of the launch (4 up to 81 920 rays, else 1) | 1 | 4 (same rows)
 *     ray_path_cap             [0]     points kept per traced ray for dsa_ray_paths
 *     rows_on_device           [0]     1 = dsa_solve_rows leaves the COO rows on the device (dsa_iteration_system_device, dsa_lsmr)
 *     disp_layers_lds          [-1]    layer tables of the dispersion kernel: 1 LDS | 0 global scratch | -1 LDS when they fit
 *     disp_group_shift         [-1]    lanes per dispersion curve = 2^shift, 0 .. 3; -1 = 8 lanes up to 4096 curves, 4 up to 32768, else 1
 *     forward_models_chunk     [0]     dsa_forward_models: models per pass; 0 = as many as the memory budget holds maps for (same results)
 *     forward_models_order     [0]     dsa_forward_models: unit order, 0 model-major | 1 period-major (A/B switch; same results under exact_ties = 2)
 *     disp_failure_log         [0]     keep the first N curves without a root in the reference's call order (dsa_dispersion_failure)
 *     lsmr_device_vectors      [0]     dsa_lsmr: 0 ordered reductions on the host | 1 all vectors on the device (same results)
 *
 * Grid size limit: the coarse solve keeps one bit per 8x8-node tile in LDS (36 KB): up to about 4340 nodes per side (nx <= 545 at dicing 8);
 * dsa_plan returns DSA_ERR_ARGUMENT beyond. */
int dsa_set_option(dsa_engine* e, const char* name, double value);

/* ---- engine level --------------------------------------------------------------------------- */
/* Grid of reference CalSurfG.f90:1032-1065 (dicing 8) / :2487-2520 (dicing 5) and `nmaps`
 * velocity maps pv[m][nx*ny] (fp64, latitude index fastest: pv[(jj-1)*nx + ii - 1], the layout
 * of the reference's pvRc etc.).  Runs the dicing kernel once per map (the reference repeats it
 * per source, :1186). */
int dsa_set_maps(dsa_engine* e, int nx, int ny, float goxd, float gozd, float dvxd, float dvzd,
                 int dicing, int nmaps, const double* pv);

/* Describe the (map, source) units and their receivers (colatitude / longitude in radians, the
 * convention of scxf/sczf/rcxf/rczf).  Receivers of unit u are rcx[first .. first+nrec[u]) with
 * first = sum of nrec over earlier units.  Host-side preparation and upload only. */
int dsa_plan(dsa_engine* e, int nunits, const int* map_index, const float* scx, const float* scz,
             const int* nrec, const float* rcx, const float* rcz);

/* Same with per-unit extras (any may be NULL): mode[u] bit 0 = produce receiver times, bit 1 = trace
 * rays / emit Frechet rows (default both); sen_slot[u] = period slot of the depth kernels used
 * by unit u's rows; data_first[u] = 0-based index of the datum of unit u's first receiver
 * (default: running receiver count).  Group-velocity data take two units with the same
 * data_first: times on the group-velocity map, rays on the phase-velocity map
 * (reference CalSurfG.f90:1166-1183, :1360-1376). */
int dsa_plan_units(dsa_engine* e, int nunits, const int* map_index, const float* scx, const float* scz,
                   const int* nrec, const float* rcx, const float* rcz, const int* mode,
                   const int* sen_slot, const int* data_first);

/* Depth kernels for the Frechet rows, in the reference's layout: vels(nx,ny,nz) fp32,
 * depz(nz), sen_*(nx*ny, kmax, nz) fp64 (CalSurfG.f90:1005-1016).  Uploaded and folded with the
 * Brocher chain-rule factors (:1385-1423) once. */
int dsa_set_depth_kernels(dsa_engine* e, int nz, int kmax, const float* vels, const float* depz,
                          const double* sen_vs, const double* sen_vp, const double* sen_rho);

/* Dispersion stage on the device (reference depthkernel CalSurfG.f90:1-169 / caldespersion
 * :2866-2927 over surfdisp96.f): spherical earth, fundamental mode.
 *   begin: the Vs model vels(nx,ny,nz), depths depz(nz), sublayering minthk; room for
 *          `nmaps_total` phase/group-velocity maps and `kmax_total` depth-kernel slots.
 *   run:   one wave type (iwave 1 Love / 2 Rayleigh, igr 0 phase / 1 group) at periods t[nper]:
 *          maps [map_first, map_first+nper) and, if with_kernels, slots [sen_slot, sen_slot+nper).
 *   copy_maps: duplicate maps inside the store (the reference overwrites the head of pvRc / pvLc
 *          with the phase velocities at the group periods, CalSurfG.f90:1110, :1128).
 *   fetch: host copies in the reference's layouts pv(nx*ny, nper), sen_*(nx*ny, nper, nz).
 *   maps_from_dispersion / kernels_from_dispersion: hand the resident results to the solve
 *          (same effect as dsa_set_maps / dsa_set_depth_kernels, no host round trip). */
int dsa_dispersion_begin(dsa_engine* e, int nx, int ny, int nz, const float* vels, const float* depz,
                         float minthk, int kmax_total, int nmaps_total);
int dsa_dispersion_run(dsa_engine* e, int iwave, int igr, int nper, const double* t, int with_kernels,
                       int sen_slot, int map_first);
int dsa_dispersion_copy_maps(dsa_engine* e, int from, int to, int n);
int dsa_dispersion_fetch(dsa_engine* e, int map_first, int nper, double* pv, int with_kernels,
                         int sen_slot, double* sen_vs, double* sen_vp, double* sen_rho);
int dsa_maps_from_dispersion(dsa_engine* e, float goxd, float gozd, float dvxd, float dvzd, int dicing);
int dsa_kernels_from_dispersion(dsa_engine* e);

/* The dispersion stage with a model dimension: `nmodels` Vs models vels(nx,ny,nz,nmodels), model slowest, on one set of depths.
 *   begin_models: room for nmaps_per_model maps per model.  The store is model-major: global map = model * nmaps_per_model + m.
 *   dsa_dispersion_run(iwave, igr, nper, t, 0, 0, map_first) afterwards computes the curves of ALL models in one launch (the models
 *          are further columns of the kernel: the lanes-per-curve choice of option disp_group_shift is made on nx*ny*nmodels curves)
 *          and writes maps [model * nmaps_per_model + map_first, .. + nper) of every model.
 *   dsa_dispersion_fetch / dsa_dispersion_copy_maps take global map indices; dsa_maps_from_dispersion hands all
 *          nmodels * nmaps_per_model maps to the solve (dsa_plan_units' map_index is the global one).
 * Model k's maps are bit-identical to dsa_dispersion_begin + run + fetch on model k alone, whatever the group width.  nmodels = 1 IS
 * dsa_dispersion_begin with kmax_total = nmaps_total = nmaps_per_model, depth kernels included.  Depth kernels exist for one model only:
 * with_kernels = 1 (run or fetch) with nmodels > 1 returns DSA_ERR_ARGUMENT, dsa_kernels_from_dispersion DSA_ERR_STATE.
 * dsa_dispersion_diagnostics counts over all models, its column field being model * nx*ny + column (1-based);
 * model_failures: curves without a root per model since begin (nmodels must be the begin's). */
int dsa_dispersion_begin_models(dsa_engine* e, int nx, int ny, int nz, int nmodels, const float* vels, const float* depz,
                                float minthk, int nmaps_per_model);
int dsa_dispersion_model_failures(const dsa_engine* e, int nmodels, long long* count);

/* Solve every planned unit: eikonal field per unit, then receiver times into dsurf (host,
 * one float per datum, unit-major order == the reference's (knumi, srcnum, istep) order). */
int dsa_solve(dsa_engine* e, float* dsurf);

/* dsa_solve with the receiver times left on the device: d_dsurf is a DEVICE pointer (memory of the engine's GPU, one float per
 * datum).  For the multi-GPU path: the rank's slice goes into the RCCL all-gather straight from HBM (bench.py, sharding.py). */
int dsa_solve_device(dsa_engine* e, void* d_dsurf);

/* dsa_solve plus rays and Frechet rows (reference rpaths + row loop, CalSurfG.f90:1377-1432):
 * COO triplets in the reference's order -- rw[k] value, iw[k] 1-based row (datum), col[k]
 * 1-based column (k-1)*nvx*nvz + (jj-1)*nvx + kk -- *nar entries, at most `capacity`. */
int dsa_solve_rows(dsa_engine* e, float* dsurf, float* rw, int* iw, int* col, long long capacity,
                   long long* nar);

/* Ray paths (the reference's disabled raypath.out dump, CalSurfG.f90:2276-2283, read by its
 * scripts/plotpath.py): with dsa_set_option(e, "ray_path_cap", C) the next dsa_solve_rows keeps up to C points per traced
 * ray.  For the R traced rays (DSA_STAT_RAYS) in data order: datum[R] 1-based row, npts[R] points of the ray (may exceed
 * C), latlon[R * C * 2] (latitude, longitude) in degrees: receiver first, source last. */
int dsa_ray_paths(dsa_engine* e, int* datum, int* npts, float* latlon);

/* ---- azimuthal anisotropy: 2psi Frechet rows traced with the rays (extension; Liu et al. 2019) ----
 * c(psi) = c0 + A1 cos 2psi + A2 sin 2psi, psi the azimuth of propagation clockwise from north, A1 = int (Vs/2)(dc/dVs)(Gc/L) dz and A2
 * likewise with Gs/L; the unknowns gc = Gc/L and gs = Gs/L live on the isotropic unknowns' grid.
 * dsa_solve_rows_azimuthal is dsa_solve_rows with two more blocks of columns: every gradient step of a ray's back-trace has
 * cos 2psi = (dtx^2 - dtz^2)/q and sin 2psi = -2 dtx dtz/q of its travel-time gradient (dtx south, dtz east, q = dtx^2 + dtz^2; both 0
 * unless q is finite and positive), and every contribution r1 to a vertex sum of the isotropic kernel fdm also goes, times those, into
 * fdm_c and fdm_s (fp32, r1*c2 + acc, the isotropic sum's order).  Per ray, in data order: the isotropic entries exactly as dsa_solve_rows
 * writes them, then block gc, then block gs, each over the vertices the isotropic row lists, layers outer:
 *   val = (float)(Sazi * (double)f), Sazi = sen_vs * (double)(0.5f * vels) of the layer and column, f = fdm_c (gc) or fdm_s (gs),
 *   kept when |val| > 1e-4, col = B*maxvp + k*nvx*nvz + (jj-1)*nvx + kk with B = 1 (gc), 2 (gs), maxvp = nvx*nvz*(nz-1).
 * dsurf and every statistic are dsa_solve_rows'.  Host COO only (dsa_solve_rows_azimuthal_device leaves the rows on the device):
 * DSA_ERR_STATE with option rows_on_device, DSA_ERR_ARGUMENT for a null
 * array or when 3*maxvp does not fit an int, DSA_ERR_CAPACITY as dsa_solve_rows.  Calls that never ask for it use no memory for it. */
int dsa_solve_rows_azimuthal(dsa_engine* e, float* dsurf, float* rw, int* iw, int* col, long long capacity,
                             long long* nar);
/* dsa_solve_rows_azimuthal with its rows left on the device: the COO is written behind the engine's resident rows exactly
 * as dsa_solve_rows writes it under option rows_on_device, whatever that option says, and the option is left as it was found.  rw / iw /
 * col are all given -- they then receive a copy, bit for bit dsa_solve_rows_azimuthal's, as are dsurf, *nar and every statistic -- or all
 * NULL: nothing of 12 bytes per entry leaves the device.  Afterwards dsa_iteration_system_azimuthal_device builds the joint system on
 * these rows; dsa_iteration_system_device refuses them (DSA_ERR_STATE).  Errors: DSA_ERR_ARGUMENT (a null e / nar, only some of rw / iw /
 * col given, 3*maxvp beyond an int), DSA_ERR_STATE (no plan, no depth kernels, several engines sharing the call), DSA_ERR_CAPACITY. */
int dsa_solve_rows_azimuthal_device(dsa_engine* e, float* dsurf, float* rw, int* iw, int* col, long long capacity,
                                    long long* nar);
/* on[kmax] (kmax = the depth kernels' slot count, checked by the next azimuthal solve): 0 = units of that depth-kernel slot (sen_slot of
 * dsa_plan_units) emit no gc / gs entries -- Love periods, for which the 2psi terms above do not hold.  on = NULL: every slot emits. */
int dsa_set_azimuthal_slots(dsa_engine* e, int kmax, const int* on);
/* For the R traced rays (DSA_STAT_RAYS) of the last dsa_solve_rows_azimuthal, in data order: datum[R] 1-based row, nsteps[R] gradient
 * steps taken, sums[2 R] the sequential fp32 sums of cos 2psi and of sin 2psi over them (sums / nsteps = the ray's mean 2psi direction).
 * DSA_ERR_STATE before an azimuthal solve of the current plan. */
int dsa_ray_azimuths(dsa_engine* e, int* datum, int* nsteps, float* sums);

/* ---- next to the path: the matrix-vector products of the inversion step (reference aprod.f90:7-60) ----
 * load: COO matrix (rw[k], 1-based row[k] <= m, col[k] <= n), kept on the device in row-major and
 * column-major order; spmv mode 1: y += A x, mode 2: x += A^T y on host vectors x[n], y[m].
 * Every output element adds its entries in storage order in fp32, like the reference's loop. */
int dsa_spmv_load(dsa_engine* e, int m, int n, long long nar, const float* rw, const int* row, const int* col);
int dsa_spmv(dsa_engine* e, int mode, float* x, float* y);

/* LSMR of the inversion step (reference lsmrModule.f90:36-750, single precision as shipped, called at main.f90:487) on
 * the matrix of the last dsa_spmv_load, all vectors resident on the device.  b[m] right-hand side (host, not
 * modified), x[n] solution (host, out); the other arguments and results are the reference's (damp, atol, btol,
 * conlim, itnlim, localSize -> istop, itn, normA, condA, normr, normAr, normx).  Sums run in the reference's order:
 * results are bit-identical to the reference's LSMR. */
int dsa_lsmr(dsa_engine* e, const float* b, float damp, float atol, float btol, float conlim, int itnlim,
             int localSize, float* x, int* istop, int* itn, float* normA, float* condA, float* normr,
             float* normAr, float* normx);

/* nreal LSMR solves on the matrix of the last dsa_spmv_load / dsa_iteration_system_device.  Realisation r solves
 * min || diag(s_r) (A x - b) ||^2 + damp^2 ||x||^2 with s_r = row_scale[r*m .. r*m+m-1] (host, not modified) and the
 * shared right-hand side b[m].  x: nreal*n (realisation-major), istop/itn: nreal, est: 5*nreal (normA condA normr
 * normAr normx per realisation).  Realisation r is bit-identical to dsa_lsmr on the explicitly scaled system
 * (entries fl(a*s_r[row]), right-hand side fl(b*s_r)).  The resident matrix and dsa_lsmr are left as they were.
 * Errors: DSA_ERR_ARGUMENT (nreal < 1, a null pointer), DSA_ERR_STATE (no matrix), DSA_ERR_DEVICE. */
int dsa_lsmr_batch(dsa_engine* e, int nreal, const float* b, const float* row_scale, float damp, float atol, float btol,
                   float conlim, int itnlim, int localSize, float* x, int* istop, int* itn, float* est);

/* Linearised resolution tests: nreal LSMR solves on the (m x n) matrix of the last dsa_spmv_load /
 * dsa_iteration_system_device, realisation r with the right-hand side of a test model m_r formed on the device:
 * b_r[i] = (A m_r)[i] for the data rows i < ndata (the bits of dsa_spmv mode 1 with x = m_r, y = 0), +0 for the rows
 * from ndata up.  models: nreal*n host array (realisation-major), or NULL: m_r = the unit spike at unknown spike_first + r
 * (made on the device; the spike range must lie in [0, n)).  Realisation r is bit-identical (x, istop, itn, est as in
 * dsa_lsmr_batch) to dsa_lsmr on b_r; a zero b_r gives x = 0, itn 0, istop 0.  x (nreal*n) may be NULL: then nothing of
 * size n*nreal leaves the device.  psf (spikes only, 4*nreal, may be NULL) needs coords (3*n: latitude deg, longitude
 * deg, depth km per unknown): psf[4r..4r+3] = {R_jj = x_r[j], sum x^2, sum x^2 dh^2, sum x^2 dz^2} over the unknowns of
 * x_r, j = spike_first + r, dh the great-circle distance in km (haversine, radius 6371 km) and dz the depth difference
 * from unknown j; fp64 in a fixed order (repeated calls give the same bits).  The resident matrix, dsa_lsmr and
 * dsa_lsmr_batch are left as they were.  Errors: DSA_ERR_ARGUMENT (nreal < 1, ndata outside [1, m], a spike range
 * outside [0, n), psf without spikes or coords, a null istop / itn / est), DSA_ERR_STATE (no matrix), DSA_ERR_DEVICE. */
int dsa_lsmr_resolution(dsa_engine* e, int nreal, int ndata, const float* models, int spike_first, const double* coords,
                        float damp, float atol, float btol, float conlim, int itnlim, int localSize, float* x, double* psf,
                        int* istop, int* itn, float* est);

/* dsa_lsmr_resolution's spike solves with the PSF measures taken per parameter block: the n unknowns are read as
 * nblocks blocks of nb = n / nblocks cells each on one grid of cells (the joint system: Vs | gc | gs, nblocks = 3); coords holds 3*nb
 * doubles, (latitude deg, longitude deg, depth km) per cell.  x, istop, itn, est are dsa_lsmr_resolution's for the same spikes, bit for
 * bit.  For spike r at unknown j = spike_first + r, cell cj = j mod nb, and every block B:
 *   psf[(r*nblocks + B)*4 + 0]      = x_r[B*nb + cj]: R_jj in the spike's own block, the co-located leakage in the others;
 *   psf[(r*nblocks + B)*4 + 1 .. 3] = sum x^2, sum x^2 dh^2, sum x^2 dz^2 over the unknowns of block B, dh and dz measured from cell
 *                                     cj to the unknown's cell as in dsa_lsmr_resolution.
 * fp64 in a fixed order (repeated calls give the same bits): a block is cut into chunks of 1024 cells, a chunk's four runs of 256
 * consecutive cells are summed in order and added as ((w0 + w1) + w2) + w3, the chunks are added in order.  With nblocks = 1 psf is
 * dsa_lsmr_resolution's, bit for bit.  x (nreal*n) may be NULL: then nothing of size n*nreal leaves the device.  The resident matrix and
 * the other solvers are left as they were.  Errors: DSA_ERR_ARGUMENT (nreal < 1, ndata outside [1, m], nblocks < 1 or not a divisor of
 * n, a spike range outside [0, n), a null coords / psf / istop / itn / est), DSA_ERR_STATE (no matrix), DSA_ERR_DEVICE. */
int dsa_resolution_blocks(dsa_engine* e, int nreal, int ndata, int nblocks, int spike_first, const double* coords,
                               float damp, float atol, float btol, float conlim, int itnlim, int localSize, float* x,
                               double* psf, int* istop, int* itn, float* est);

/* Regularisation trade-off sweep: nreal LSMR solves on the (m x n) matrix of the last dsa_spmv_load /
 * dsa_iteration_system_device, whose rows below ndata are data rows and whose rows from ndata up are regularisation rows
 * built with weight0 (every entry fl(c*weight0), c a non-zero integer, |c| <= 64).  Member k solves the system that keeps
 * the data rows and gives every regularisation entry the value fl(c*weight[k]) -- what dsa_iteration_system(_device)
 * builds with weight[k] in place of weight0 -- with damping damp[k] and the shared right-hand side b[m]; it is
 * bit-identical (x, istop, itn, est as in dsa_lsmr_batch) to dsa_lsmr(b, damp[k], ...) on that system.  weight[k] = 0
 * and damp[k] = 0 are valid.  x (nreal*n) may be NULL: then nothing of size n*nreal leaves the device.  measures
 * (3*nreal, may be NULL): measures[3k..3k+2] = {sum over i < ndata of (b_i - (A x_k)_i)^2, sum over i >= ndata of
 * ((C x_k)_i)^2, sum of x_k[j]^2}, C the integer coefficients (free of the weight: comparable across members); fp64,
 * every row's sum over its entries in storage order, in a fixed order (repeated calls give the same bits).  The resident
 * matrix, dsa_lsmr, dsa_lsmr_batch and dsa_lsmr_resolution are left as they were.  Errors: DSA_ERR_ARGUMENT (nreal < 1,
 * ndata outside [1, m], a null b / weight / damp / istop / itn / est, weight0 not finite or not > 0, a negative or
 * non-finite weight[k] or damp[k], a regularisation entry that is not fl(c*weight0)), DSA_ERR_STATE (no matrix),
 * DSA_ERR_DEVICE. */
int dsa_lsmr_tradeoff(dsa_engine* e, int nreal, int ndata, const float* b, float weight0, const float* weight,
                      const float* damp, float atol, float btol, float conlim, int itnlim, int localSize, float* x,
                      double* measures, int* istop, int* itn, float* est);

/* K-fold cross-validation of (weight, damp) pairs: ncombo*(nfolds+1) LSMR solves on the (m x n) matrix of the last dsa_spmv_load /
 * dsa_iteration_system_device, rows and weight0 as for dsa_lsmr_tradeoff.  fold[i] in [0, nfolds) is the fold of datum i < ndata.
 * With S = nfolds + 1 and nreal = ncombo*S, member k = q*S + f (f < nfolds) holds out fold f with (weight[q], damp[q]); member
 * q*S + nfolds holds out nothing (the full member of combo q).  Member k is bit-identical (x, istop, itn, est as in dsa_lsmr_batch)
 * to dsa_lsmr(b_k, damp[q], ...) on the explicitly written system: every data row i with entries fl(a*s) and right-hand side
 * fl(b_i*s), s = 0 where fold[i] = f and 1 otherwise; every regularisation entry fl(c*weight[q]) with its b_i unscaled.  A zeroed
 * row gives LSMR what deleting it gives, so the member is the cross-validation solve itself.  A member whose masked right-hand
 * side is all zero returns x = 0, itn 0, istop 0; a fold id no datum has makes its member equal to the full one; nfolds = 1 is
 * valid.  x (nreal*n) may be NULL: then nothing of size n*nreal leaves the device.  measures (4*nreal, may be NULL):
 * measures[4k..4k+3] = {sum over the kept data rows of (b_i - (A x_k)_i)^2, the same over the held-out rows, sum over i >= ndata
 * of ((C x_k)_i)^2, sum of x_k[j]^2}, A and b unscaled, C the integer coefficients; fp64 in the fixed order of
 * dsa_lsmr_tradeoff's measures, so a full member's kept sum, roughness and size have the bits of that call's measures for the same
 * (weight, damp), and its held-out sum is +0.  resid (2*ncombo*ndata, may be NULL): resid[(2q)*ndata + i] = b_i - (A x_h)_i with
 * h = q*S + fold[i], the residual of datum i in the member that held it out; resid[(2q+1)*ndata + i] the same in the full member
 * (the values the measures square).  The resident matrix and the five other solvers are left as they were.  Errors:
 * DSA_ERR_ARGUMENT (ncombo or nfolds < 1, more than 64*65535 members, ndata outside [1, m], a null b / weight / damp / fold /
 * istop / itn / est, a resid whose 2*ncombo*ndata overflows, weight0 not finite or not > 0, a negative or non-finite weight[q] or
 * damp[q], a fold id outside [0, nfolds), a regularisation entry that is not fl(c*weight0)), DSA_ERR_STATE (no matrix),
 * DSA_ERR_DEVICE. */
int dsa_lsmr_crossval(dsa_engine* e, int ncombo, int nfolds, int ndata, const float* b, float weight0, const float* weight,
                      const float* damp, const int* fold, float atol, float btol, float conlim, int itnlim, int localSize,
                      float* x, double* measures, double* resid, int* istop, int* itn, float* est);

/* Poisson-Voronoi subspace ensemble: nreal LSMR solves on random Voronoi projections of the data rows of the (m x n) matrix
 * of the last dsa_spmv_load / dsa_iteration_system_device.  Rows below ndata are the data rows; the rows from ndata up (the
 * smoothing rows) take no part.  Tessellation: xyz holds 3*n doubles, one Cartesian point per unknown (the host chooses the
 * metric); seeds holds nreal*ncells 0-based unknown indices, member-major, distinct within a member; cell_k(j) is the index
 * s in [0, ncells) that minimises d2 = ((xj-xs)*(xj-xs) + (yj-ys)*(yj-ys)) + (zj-zs)*(zj-zs), evaluated in fp64 in exactly
 * that association without contraction, ties to the lowest s (only exactly rounded basic operations: a numpy restatement
 * gives the same integers).  Member k's system M_k lists the data rows row by row (rows ascending, each row's entries in the
 * resident storage order) with every column index j replaced by cell_k(j), duplicates not merged: ncells unknowns,
 * right-hand side b[0..ndata), damping damp.  z[k*ncells ..], istop[k], itn[k], est[5k..] are bit-identical to dsa_lsmr after
 * dsa_spmv_load(ndata, ncells, M_k), with localVecs = min(localSize, ndata, ncells); a cell no data entry touches gets z = 0.
 * z (nreal*ncells) and cell (nreal*n ints: cell_k(j) at cell[k*n + j]) may be NULL.  stats (2*n doubles, may be NULL):
 * stats[j] = the ensemble mean and stats[n + j] = the sample standard deviation of x_k[j] = z_k[cell_k(j)] over the members;
 * all sums fp64 over k = 0 .. nreal-1 in order, mean = sum / nreal, std = sqrt(sum (x - mean)^2 / (nreal - 1)), 0 for
 * nreal = 1 (repeated calls give the same bits).  With z and cell NULL nothing of size nreal*n or nreal*ncells leaves the
 * device.  The resident matrix, dsa_lsmr, dsa_lsmr_batch, dsa_lsmr_resolution and dsa_lsmr_tradeoff are left as they were.
 * Errors: DSA_ERR_ARGUMENT (nreal < 1, ndata outside [1, m], ncells outside [1, n] or above 2^24, a null b / xyz / seeds /
 * istop / itn / est, a seed outside [0, n), a non-finite damp or coordinate, data rows of more than 2^25 - 1 entries),
 * DSA_ERR_STATE (no matrix), DSA_ERR_DEVICE.  After a failure the engine is as it was. */
int dsa_lsmr_voronoi(dsa_engine* e, int nreal, int ndata, int ncells, const float* b, const double* xyz, const int* seeds,
                     float damp, float atol, float btol, float conlim, int itnlim, int localSize, float* z, int* cell,
                     double* stats, int* istop, int* itn, float* est);

/* One outer iteration's host glue (reference main.f90:361-466 and :520-535; plain host code, no device):
 * iteration_system: residual cbst = obst - dsyn, percentile weights (getpercentile.f90), rows scaled by their weights,
 *   DWS norm[maxvp] with dws = {max, mean}, regularisation rows appended.  In/out rw, col (capacity entries) and iw
 *   (2*capacity + 1: iw[0] = final nar, then rows, then columns -- the layout aprod / LSMR take); cbst has dall + maxvp
 *   values, *m_out = dall + maxvp rows.
 * model_update: dv clipped to +-0.5, vsf(nx, ny, nz) += dv on the interior, clipped to [minvel, maxvel]. */
int dsa_iteration_system(int nx, int ny, int nz, int dall, long long nar_in, long long capacity, float* rw, int* iw,
                         int* col, const float* obst, const float* dsyn, float threshold0, float weight0, float* cbst,
                         float* datweight, float* norm, int* m_out, long long* nar_out, float* dws);
int dsa_model_update(int nx, int ny, int nz, float* dv, float* vsf, float minvel, float maxvel);
/* model_update for nmodels steps at once, on the device, without touching its inputs: models_out (nmodels * nx*ny*nz floats, model
 * slowest) receives what nmodels dsa_model_update calls leave in copies of vsf, given steps[k n .. (k+1) n) (n = (nx-2)(ny-2)(nz-1)),
 * scaled by alpha[k] first (one rounded product) where alpha is not NULL -- bit for bit, a NaN step giving a NaN node.  steps == NULL:
 * the solutions the last batch solve left on e (see dsa_forward_steps, whose models these are; DSA_ERR_STATE where it has none that fit).
 * DSA_ERR_ARGUMENT: a null e / vsf / models_out, nmodels < 1, nx or ny < 3, nz < 2. */
int dsa_step_models(dsa_engine* e, int nx, int ny, int nz, int nmodels, const float* vsf, const float* steps, const float* alpha,
                    float minvel, float maxvel, float* models_out);
/* The same system built where the rows are: on the COO rows that dsa_solve_rows (option rows_on_device) or dsa_calsurfg
 * (called with null rw / iw / col) left on the device.  Weights, regularisation rows, DWS and both orderings of the matrix
 * are made on the device; the matrix (12 bytes per entry) never crosses PCIe (reference: main.f90:349-359 -> :361-466 ->
 * :487-489 all on host arrays).  cbst has dall + maxvp elements; afterwards dsa_lsmr(e, cbst, ...) solves on that matrix.
 * Bit-identical to dsa_iteration_system + dsa_spmv_load. */
int dsa_iteration_system_device(dsa_engine* e, int nx, int ny, int nz, int dall, const float* obst, const float* dsyn,
                                float threshold0, float weight0, float* cbst, float* datweight, float* norm, int* m_out,
                                long long* nar_out, float* dws);

/* The joint Vs | gc | gs system of the azimuthal step built on the azimuthal rows that
 * dsa_solve_rows_azimuthal_device, or dsa_calsurfg_azimuthal called with null rw / iw / col, left on the device.  datweight[dall]: the
 * reference's 0/1 percentile weights of the residuals obst - dsyn; cbst[i] = fl((obst[i] - dsyn[i]) * datweight[i]) (under a zero
 * weight a zero with the residual's sign, as the host route's product leaves it); every data entry scaled by its datum's weight, and below the dall data rows the first-difference Laplacian rows of the three blocks, written by a kernel: block
 * B = 0 (Vs), 1 (gc), 2 (gs) has rows dall + B*maxvp + index and columns B*maxvp + ..., 2 w on the block's faces, 6 w and six -w
 * inside, w = weight0 on Vs and weight_azi on gc and gs, each value one rounded product.  m = *m_out = dall + 3*maxvp rows,
 * n = 3*maxvp columns; cbst has dall + 3*maxvp elements (0 from dall up).  norm[3*maxvp]: per column the sequential fp32 sum of |entry|
 * over its data entries in storage order; dws[6]: {max, mean} of norm per block.  Afterwards dsa_lsmr(e, cbst, ...) and every batched
 * solver run on that matrix (dsa_lsmr_tradeoff / _crossval when weight_azi = weight0: one weight per call).  Bit-identical -- matrix
 * in both orderings, cbst, datweight -- to the host route: dsa_calsurfg_azimuthal with arrays, the same weights, the same rows in the
 * order data, Vs, gc, gs through dsa_spmv_load.  Every argument is checked before the device is touched.  Errors: DSA_ERR_ARGUMENT (a
 * null pointer, nx or ny < 3, nz < 2, dall < 1, too few data for the quartile rule, dall + 3*maxvp beyond an int, a weight0 or
 * weight_azi that is negative or not finite), DSA_ERR_STATE (no azimuthal rows on the device: none at all, isotropic ones, or a joint
 * system already built from them), DSA_ERR_CAPACITY (more than 2^31-1 entries), DSA_ERR_DEVICE. */
int dsa_iteration_system_azimuthal_device(dsa_engine* e, int nx, int ny, int nz, int dall, const float* obst, const float* dsyn,
                                          float threshold0, float weight0, float weight_azi, float* cbst, float* datweight,
                                          float* norm, int* m_out, long long* nar_out, float* dws);

/* ---- per-period 2-D maps on the bent rays.  layer = (nx-2)*(ny-2), nmaps = the maps of dsa_set_maps. ----
 *
 * dsa_solve_rows_maps: dsa_solve, and every unit whose mode has bit 1 traces its rays; the ray of datum d of a unit on map m adds, for
 * block B = 0 (the map value c0; azimuthal = 1: also 1 = A1 with the cos 2psi slab and 2 = A2 with the sin 2psi slab, rays traced as by
 * dsa_solve_rows_azimuthal) and every vertex i (0-based, the isotropic list: |fdm| >= 1e-4 on the isotropic slab, latitude index
 * fastest) whose slab element f has |f| > 1e-4, the entry rw = f, iw = d + 1, col = (B*nmaps + m)*layer + i + 1; within a ray B outer,
 * vertices inner; rays in data order.  These are dsa_solve_rows' / dsa_solve_rows_azimuthal's entries under a depth factor of exactly 1
 * on one layer, with every map in columns of its own.  No depth kernels are needed.  rw, iw, col: host arrays of `capacity` entries, or
 * all three NULL: the rows stay on the device for dsa_iteration_system_maps_device (the option rows_on_device is not consulted and left
 * as it is).  dsa_ray_azimuths works after an azimuthal call.  Errors: DSA_ERR_ARGUMENT (azimuthal not 0 / 1, only some of the three
 * arrays, more than 2^31-1 columns), DSA_ERR_STATE (no maps, no plan, several engines sharing the call), DSA_ERR_CAPACITY. */
int dsa_solve_rows_maps(dsa_engine* e, int azimuthal, float* dsurf, float* rw, int* iw, int* col, long long capacity, long long* nar);

/* The regularised system of the map rows left on the device (nblocks = 1 after azimuthal = 0, 3 after azimuthal = 1): datweight, cbst and
 * the scaling of the data entries exactly as dsa_iteration_system_azimuthal_device; n = nblocks*nmaps*layer columns, m = dall + n rows,
 * cbst has m elements (0 from dall up).  Unknown `index` (0-based, column order) has the row dall + index: on the edge of its plane -- one
 * (block, map) pair of (nx-2) x (ny-2) unknowns -- the entry {index, 2 w}, inside {index, 4 w} and -w at -1, +1, -(nx-2), +(nx-2), in
 * that order: the reference's rule without the depth axis; planes never couple.  w = weight0 on block 0, weight_azi on blocks 1 and 2,
 * each value one rounded product.  norm[n]: per column the sequential fp32 sum of |entry| over its data entries in storage order;
 * dws[2*nblocks]: {max, mean} of norm per block.  Afterwards dsa_lsmr(e, cbst, ...) and the batch solvers run on that matrix.  Every
 * argument is checked before the device is touched.  Errors: DSA_ERR_ARGUMENT (a null pointer, nx or ny < 3, nmaps < 1, nblocks not 1 /
 * 3, dall < 1, too few data for the quartile rule, dall + n beyond an int, a weight that is negative or not finite, nx / ny / nmaps
 * other than the rows'), DSA_ERR_STATE (the resident rows are not map rows of this nblocks, or a system was already built from them),
 * DSA_ERR_CAPACITY (more than 2^31-1 entries), DSA_ERR_DEVICE. */
int dsa_iteration_system_maps_device(dsa_engine* e, int nx, int ny, int nmaps, int nblocks, int dall, const float* obst, const float* dsyn,
                                     float threshold0, float weight0, float weight_azi, float* cbst, float* datweight, float* norm,
                                     int* m_out, long long* nar_out, float* dws);

/* dsa_update_maps: the resident fp32 vertex maps updated on the device.  dv: nmaps*layer floats, the c0 block of a solution (required:
 * dsa_lsmr returns its solution to the host, a NULL dv is DSA_ERR_ARGUMENT).  Interior vertex i of map m becomes
 * v + clamp(dv, -dvmax, dvmax), then clamped to [minvel, maxvel], plain fp32 in dsa_model_update's order of operations; the outer ring
 * of vertices keeps its values.  Then everything dsa_set_maps derives from the vertex values is made again and the plan is dropped (plan
 * again): the engine is in the state dsa_set_maps leaves with pv = (double) of the same fp32 values, bit for bit.
 * dsa_get_maps: the resident vertex maps, nmaps*nx*ny floats in dsa_set_maps' layout.
 * Errors: DSA_ERR_STATE (no maps), DSA_ERR_ARGUMENT (nmaps is not the engine's, dvmax not finite or <= 0, minvel > maxvel, a null pointer). */
int dsa_update_maps(dsa_engine* e, int nmaps, const float* dv, float dvmax, float minvel, float maxvel);
int dsa_get_maps(dsa_engine* e, int nmaps, float* velv);

/* dsa_maps_resolution: how well every value of the period maps is known (extension).  The resident matrix is a map system
 * of nblocks*nmaps planes of layer = (nx-2)*(ny-2) unknowns with ndata data rows on top: dsa_iteration_system_maps_device's, or a
 * dsa_spmv_load of one in row order.  Maps never couple, so the normal matrix A^T A + damp^2 I is one dense block of n_m = nblocks*layer
 * unknowns per map; each block is factored exactly (fp64 L D L^T, csrc/map_resolution.h) and solved for every used datum of the map, which
 * gives the generalised inverse T, the resolution matrix R = T^T G and the covariance for unit data variance, T^T T.  A row belongs to the map that
 * all of its entries lie in; a data row is used iff an entry of it is not zero (the builder scales unweighted rows to zero).
 *   measures  9*n doubles, (measure, unknown in column order); for local unknown q of plane B: 0 R_qq; 1 var_q = sum_d t_dq^2; 2 the sum
 *             of R_lq^2 over the l of plane B; 3, 4 that sum weighted with the squared vertex distance in x and in y; 5 the sum of R_lq^2 over
 *             the whole map; 6, 7 R at the co-located unknowns of planes (B+1) and (B+2) mod nblocks; 8 sum_d t_dq t_dq' with q' the
 *             co-located unknown of plane (B+1) mod nblocks.  6, 7, 8 are 0 for nblocks = 1.
 *   leverage  NULL, or ndata: h_d = g_d . t_d, 0 for a datum that is not used
 *   trace     NULL, or nblocks*nmaps: the sum of R_qq per plane, (block, map)
 *   nused     NULL, or nmaps: used data per map
 *   flag      NULL, or nmaps: 0; 1 a pivot that is not finite or <= 0; 2 no used datum.  Every output of a flagged map is 0.
 *   R         NULL with r_map = -1, or the n_m*n_m doubles of map r_map's R, R_lq at l*n_m + q
 * Maps are processed in groups whose factor, R and T (8*(2 n_m^2 + K_m n_m) bytes per map of K_m used data) fit dsa_set_memory_budget,
 * or half of the free memory, at most 16 GiB, where none is set.  The call is read-only on the resident matrix and on every solver's
 * state: dsa_lsmr and the batch solvers give the bits they gave without it, the solutions a batch solve left stay valid.
 * Errors: DSA_ERR_ARGUMENT (a NULL e / measures, nx or ny < 3, nmaps < 1, nblocks not 1 or 3, n other than nblocks*nmaps*layer, ndata
 * outside [1, m], damp negative or not finite, r_map outside -1 .. nmaps-1, R and r_map disagreeing), DSA_ERR_STATE (no resident matrix,
 * or the radial system), DSA_ERR_CAPACITY (the factor and R of one map alone exceed a set budget): all found before the device is touched.
 * Then, found by a pass over the matrix before anything is factored: DSA_ERR_ARGUMENT (a row with entries in two maps; a row that stores a
 * column twice; a column whose rows do not ascend, i.e. a matrix that was not loaded in row order), DSA_ERR_CAPACITY (one map with its T
 * does not fit).  DSA_ERR_DEVICE.  The engine stays usable after every refusal. */
int dsa_maps_resolution(dsa_engine* e, int nx, int ny, int nmaps, int nblocks, int ndata, float damp, int r_map, double* measures,
                        double* leverage, double* trace, int* nused, int* flag, double* R);

/* dsa_columns_step: the depth inversion of the period maps, one Gauss-Newton step of every interior column's Vs(z) on the device (extension;
 * DESIGN.md 21).  The dispersion stage holds one model, as many maps as kernel slots (nmaps == nmaps_total == kmax_total of
 * dsa_dispersion_begin, at most 60), and every map k and kernel slot k has been written by a dsa_dispersion_run with_kernels = 1 (sen_slot ==
 * map_first) since dsa_dispersion_begin or since the last step.  obs: the maps, nmaps*nx*ny floats in dsa_get_maps' layout; wt: as many
 * weights, or NULL for 1.  Datum k of a column is used iff wt > 0, obs > 0 and the column's own curve pv > 0 (0: no root).  Per column, with
 * M = nz-1 unknowns (the bottom depth is kept), S = d c / d Vs of dsa_kernels_from_dispersion's rule, a = (double)wt, g = a S,
 * rho = a ((double)obs - pv):  (G^T G + smooth^2 L^T L + damp^2 I) delta = G^T rho,  L the first-difference Laplacian (-1, 2, -1) closed by
 * the rows (1, -1) and (-1, 1), solved by an L D L^T factorisation without square roots, everything fp64 and every sum sequential; then in fp32
 * s = (float)delta clipped to +-dvmax, v = v + s clamped to [minvel, maxvel], dsa_model_update's comparisons.  The model is stepped where it
 * lies: the next dsa_dispersion_run works on it.  The outer ring of columns keeps its values.
 *   dv     (nz-1)*nx*ny floats, depth slowest like the model: the clipped step, 0 where the column was left alone
 *   nused  nx*ny: data used;  chi2  nx*ny: sum of rho^2 before the step;  flag  nx*ny: 0 stepped (or ring), 1 a pivot of the
 *          factorisation was not finite or <= 0 (column left alone), 2 no datum used (column left alone).  Any of the four may be NULL.
 * The step clears the marks of all maps and slots: a second step without new runs is DSA_ERR_STATE.
 * Errors, all found before the device is touched: DSA_ERR_STATE (no dispersion stage, several models, maps != slots, a map or slot not run
 * with kernels since begin / the last step, or map k and slot k written by different runs), DSA_ERR_ARGUMENT (nmaps is not the stage's, a
 * grid without interior columns, obs NULL or not finite, a wt negative or not finite, damp <= 0, smooth < 0, dvmax <= 0, minvel > maxvel).
 * dsa_dispersion_get_model: the stage's resident model, nx*ny*nz floats in dsa_dispersion_begin's layout (DSA_ERR_STATE without a stage or
 * with several models). */
int dsa_columns_step(dsa_engine* e, int nmaps, const float* obs, const float* wt, float smooth, float damp, float dvmax, float minvel,
                     float maxvel, float* dv, int* nused, double* chi2, int* flag);
int dsa_dispersion_get_model(dsa_engine* e, float* vels);

/* dsa_columns_resolution: how far the depth step's answer can be trusted, per interior column, from the regularised normal matrix the step
 * factors (extension).  The state and obs, wt, smooth, damp are dsa_columns_step's, with its rules and refusals; of obs only
 * the sign is used (which data count).  Per column, with the definitions above, N = G^T G + smooth^2 L^T L + damp^2 I = L D L^T:
 * T (nmaps x M) has in row k the solution of N t = g_k for a used datum (the step's substitutions, one solve per datum) and zeros for any
 * other; R = T^T G is the model resolution matrix, its column j the point-spread function of unknown j.  Everything fp64, every sum
 * sequential from 0.0 over the used data ascending.
 *   measures  4*(nz-1)*nx*ny doubles, (measure, depth, column): R_jj;  m1 = sum_l R_lj^2;  m2 = sum_l R_lj^2 (depz_l - depz_j)^2 -- the
 *             vertical length of the PSF is sqrt(m2 / m1);  var_j = sum_k T_kj^2, the variance of unknown j for unit variance of the
 *             weighted data (the diagonal of N^-1 G^T G N^-1)
 *   leverage  nmaps*nx*ny: h_k = sum_l g_kl T_kl, the diagonal of the data resolution matrix; 0 for a datum not used
 *   trace     nx*ny: sum_j R_jj (= sum_k h_k in exact arithmetic);  nused, flag  nx*ny: as dsa_columns_step's
 *   R         NULL, or (nz-1)*(nz-1)*nx*ny doubles: R_lj at (l*(nz-1) + j)*nx*ny + column.  NULL skips the store and changes no other bit.
 * A column with flag 1 or 2 and the outer ring of columns have 0.0 everywhere.  R is not symmetric: R_jj may leave [0, 1].
 * Nothing is changed: the model, the marks of the maps and slots and the Frechet rows' sensitivities stay, so a dsa_columns_step after
 * the call gives the bits it would have given without it; after a step the call is DSA_ERR_STATE until the runs are repeated.
 * Errors, all but the last found before the device is touched: DSA_ERR_STATE and DSA_ERR_ARGUMENT as dsa_columns_step, in its order;
 * DSA_ERR_ARGUMENT for a NULL measures, leverage, trace, nused or flag; DSA_ERR_DEVICE when a column's work arrays (about 77 KB at
 * nz = 64 with 60 maps) exceed the LDS a block of the device may have or the device refuses that size. */
int dsa_columns_resolution(dsa_engine* e, int nmaps, const float* obs, const float* wt, float smooth, float damp, double* measures,
                           double* leverage, double* trace, double* R, int* nused, int* flag);

/* dsa_columns_azimuthal: the depth inversion of the maps' 2 psi terms, gc(z) = Gc/L and gs(z) = Gs/L of every interior column from the
 * A1(T), A2(T) of c(psi) = c0 + A1 cos 2 psi + A2 sin 2 psi that the map step leaves per period (extension).  The state and obs
 * (the c0 maps), wt, smooth, damp are dsa_columns_resolution's, with its rules and refusals; a1, a2: obs's layout and type.  Slot k is a
 * Rayleigh slot iff it was run with iwave != 1 (phase and group); a Love slot is a slot of weight 0.  Datum k of a column is used iff slot k
 * is a Rayleigh slot and dsa_columns_step would use it (wt > 0, obs > 0, pv > 0); the a1, a2 of any other datum are not read.  Per column,
 * with M = nz-1 unknowns per component, Z_kl = sen_vs_kl (double)(0.5f v_l) the depth factor of the gc / gs entries of dsa_solve_rows_azimuthal (only
 * the Vs kernel), a = (double)wt, g_kl = a Z_kl, rhoc = a (double)a1, rhos = a (double)a2:
 *   (G^T G + smooth^2 L^T L + damp^2 I) gc = G^T rhoc,  the same matrix for gs and rhos,
 * one L D L^T factorisation and the step's substitutions for both; everything fp64, every sum sequential from 0.0 over the used data ascending.
 *   g         2*(nz-1)*nx*ny doubles: gc, then gs, each (depth, column).  Required.
 *   measures  NULL, or 4*(nz-1)*nx*ny doubles as dsa_columns_resolution's (R_jj, m1, m2, var) of this operator: gc and gs share it, so one
 *             set serves both; var_j is the variance of gc_j and of gs_j for unit variance of the weighted a1 and a2, which are uncorrelated
 *   leverage  NULL, or nmaps*nx*ny: h_k as dsa_columns_resolution's; 0 for a datum not used and for a Love slot
 *   chi2      NULL, or 4*nx*ny: sum rhoc^2, sum rhos^2 before, then sum (rhoc - G gc)^2, sum (rhos - G gs)^2 after
 *   nused, flag  nx*ny, required: as dsa_columns_step's (flag 1: a pivot not finite or <= 0; flag 2: no datum used)
 * A column with flag 1 or 2 and the outer ring of columns have 0.0 everywhere.  No root and no atan2 is taken: strength and fast axis are
 * the caller's.  Nothing is changed: the model, the marks of the maps and slots and the Frechet rows' sensitivities stay, so a
 * dsa_columns_step after the call gives the bits it would have given without it.
 * Errors, all but the last found before the device is touched: DSA_ERR_STATE and DSA_ERR_ARGUMENT as dsa_columns_resolution, in its order
 * (a radial stage, several models and an open sample stage are DSA_ERR_STATE); then DSA_ERR_ARGUMENT for a NULL or not finite a1 / a2 and
 * for a NULL g, nused or flag; DSA_ERR_STATE where no slot is a Rayleigh slot; DSA_ERR_DEVICE when a column's work arrays (about 79 KB at
 * nz = 64 with 60 maps) exceed the LDS a block of the device may have or the device refuses that size. */
int dsa_columns_azimuthal(dsa_engine* e, int nmaps, const float* obs, const float* a1, const float* a2, const float* wt, float smooth, float damp,
                          double* g, double* measures, double* leverage, double* chi2, int* nused, int* flag);

/* Radial anisotropy in the depth inversion (extension): Rayleigh waves see Vsv, Love waves see Vsh.
 * dsa_dispersion_begin_radial: dsa_dispersion_begin with two models vsv and vsh (each in its layout) on one set of depths.  The stage stays a
 * one-model stage -- depth kernels allowed, every size and limit dsa_dispersion_begin's -- that keeps Vsh resident beside Vsv: afterwards
 * dsa_dispersion_run reads Vsh when iwave == 1 (Love) and Vsv when iwave == 2 (Rayleigh), for the curves, the depth kernels and the replay of a
 * logged failure.  With vsh == vsv every map, kernel, mark and diagnostic is dsa_dispersion_begin's, bit for bit.  Any other begin ends the
 * radial stage.  dsa_maps_from_dispersion, dsa_dispersion_fetch, dsa_dispersion_copy_maps and dsa_dispersion_diagnostics work as on any stage;
 * dsa_columns_step, dsa_columns_resolution, dsa_dispersion_get_model and dsa_kernels_from_dispersion (whose combined sensitivities assume one
 * model for all slots) are DSA_ERR_STATE on a radial stage.
 * dsa_columns_step_radial: dsa_columns_step on a radial stage, with its state and argument rules, messages and order, and aniso finite and
 * >= 0 (DSA_ERR_ARGUMENT); DSA_ERR_STATE on a stage that is not radial.  Slot k is a Love slot iff it was run with iwave == 1.  Per column,
 * 2M unknowns x = [dVsv ; dVsh], M = nz-1: g_kl = a_k S_kl with S of dsa_kernels_from_dispersion's rule on the model the slot was run on; a
 * Rayleigh datum touches only the Vsv block and a Love datum only the Vsh block (the cross sensitivities are neglected).  Minimised:
 * |G x - rho|^2 + smooth^2 (|L x_v|^2 + |L x_h|^2) + damp^2 |x|^2 + aniso^2 |(vsh + x_h) - (vsv + x_v)|^2, by the step's L D L^T on the packed
 * 2M x 2M normal matrix, fp64, every sum sequential; both models are clipped and stepped as dsa_columns_step steps one, where they lie.  At
 * aniso = 0 each block's step has the bits of dsa_columns_step on that model with the other wave type's weights 0.
 *   dv     2*(nz-1)*nx*ny floats: the Vsv block, then the Vsh block, each as dsa_columns_step's
 *   nused, chi2  2*nx*ny: the Rayleigh data's, then the Love data's;  flag  nx*ny: 1 as dsa_columns_step's, 2 no datum of either type used
 *          (whatever damp and aniso are); a column with one type unused still steps.  Any of the four may be NULL.
 * Everything is checked before the device is touched, except DSA_ERR_DEVICE: a column's work arrays (98 232 bytes at nz = 64 with 60 maps)
 * exceed the LDS a block of the device may have, or the device refuses that size.
 * dsa_dispersion_get_model_radial: the two resident models; either pointer may be NULL.  DSA_ERR_STATE on a stage that is not radial. */
int dsa_dispersion_begin_radial(dsa_engine* e, int nx, int ny, int nz, const float* vsv, const float* vsh, const float* depz, float minthk,
                                int kmax_total, int nmaps_total);
int dsa_columns_step_radial(dsa_engine* e, int nmaps, const float* obs, const float* wt, float smooth, float damp, float aniso, float dvmax,
                            float minvel, float maxvel, float* dv, int* nused, double* chi2, int* flag);
int dsa_dispersion_get_model_radial(dsa_engine* e, float* vsv, float* vsh);

/* dsa_columns_step_lateral: dsa_columns_step with neighbouring columns coupled (extension).  The state, obs, wt, smooth, damp,
 * dvmax, minvel, maxvel and the outputs dv, nused, chi2, flag are dsa_columns_step's, with its rules, messages and order of refusals.  The step
 * of all interior columns together minimises
 *   sum_c [ |G_c x_c - rho_c|^2 + smooth^2 |L x_c|^2 + damp^2 |x_c|^2 ] + lateral^2 sum_edges |(v_c + x_c) - (v_c' + x_c')|^2
 * over the edges between interior columns at +-1 and +-nx that both take part: the roughness of the stepped model, so that iterations
 * converge to a laterally smooth model.  A column takes part if the factorisation of its own normal matrix succeeds (flag 1 otherwise: left
 * alone, no edge touches it); with lateral > 0 a column without a used datum takes part too (nused 0, flag 0) and is carried by its
 * neighbours.  The outer ring is never an unknown and never a neighbour.  The normal equations are solved by conjugate gradients
 * preconditioned with the columns' own factors, from x0 = the preconditioner applied to the right-hand side, until r^T z <= tol^2 rz0
 * (rz0 = that right-hand side's own r^T z) or maxit iterations; fp64, every sum in a fixed order (csrc/column_lateral.h), so the result has
 * one value whatever computes it.  lateral = 0 is no iteration: every output and the stepped model are dsa_columns_step's bit for bit,
 * flag 2 for a column without a used datum included.
 *   info   4 doubles: the iterations done, istop (1: the criterion was met, 2: maxit), rz0, the last r^T z
 * Afterwards as dsa_columns_step: the marks are cleared, the ring and the bottom depth are kept.
 * Errors, all found before the device is touched: DSA_ERR_STATE and DSA_ERR_ARGUMENT as dsa_columns_step, in its order (a radial stage is
 * DSA_ERR_STATE); then DSA_ERR_ARGUMENT: lateral not finite or < 0, tol not finite or <= 0, maxit < 1; DSA_ERR_CAPACITY: the loop's
 * workspace (two triangles and eight vectors per interior column) exceeds dsa_set_memory_budget, where one is set -- the workspace alone
 * is held against the whole budget, not against what the budget leaves beside the engine's other buffers. */
int dsa_columns_step_lateral(dsa_engine* e, int nmaps, const float* obs, const float* wt, float smooth, float damp, float lateral, float dvmax,
                             float minvel, float maxvel, double tol, int maxit, float* dv, int* nused, double* chi2, int* flag, double* info);

/* dsa_columns_resolution_lateral: how far the laterally coupled step's answer can be trusted (extension).  The state, obs, wt,
 * smooth, damp, lateral, tol and maxit are dsa_columns_step_lateral's, with its rules, messages and order of refusals.  With A the coupled
 * normal matrix of that step and H = blockdiag(G_c^T G_c), each of the nmembers members is one solve A x = f by that step's preconditioned
 * conjugate gradients (its arithmetic, criterion and istop), with its own iteration count:
 *   kind 0  the point-spread function of unknown index = b*(nz-1) + l (b the interior column (bj*(nx-2) + bi), l the depth): f = H e_index
 *   kind 1  row index of R = A^-1 H: f = e_index, u = H x; var = x^T u, the variance of that unknown for unit variance of the weighted data
 *   kind 2  the recovery of a test model: f = H m, m row index of models
 *   kind 3  f = row index of models
 *   models  nrows*(nz-1)*(nx-2)*(ny-2) doubles, depth slowest within a row; may be NULL when no member is of kind 2 or 3
 *   measures  nmembers*7: R_jj (the vector's own entry), m1 = sum u^2, mz = sum u^2 dz^2 (km^2), mx, my = sum u^2 di^2, dj^2 (cells^2), own =
 *          the part of m1 in the unknown's own column, var; zeros for kinds 2 and 3.  u = x for kinds 0, 2, 3
 *   info   nmembers*4: the iterations done, istop, rz0, the last r^T z of each member
 *   full   NULL, or nmembers*(nz-1)*(nx-2)*(ny-2) doubles: u of every member, depth slowest
 *   nused, flag  nx*ny, as dsa_columns_step_lateral's
 * An entry of f in a column that takes no part is 0.0; lateral = 0 is no iteration.  fp64, every sum in a fixed order
 * (csrc/column_lateral_resolution.h): a member's result has one value whatever its place in the batch and however the batch is cut into
 * chunks.  The stage is read only, as dsa_columns_resolution's.
 * Errors, all found before the device is touched: as dsa_columns_step_lateral without dvmax, minvel, maxvel, in its order; then
 * DSA_ERR_ARGUMENT: nmembers < 1, a required pointer NULL, a kind outside 0 .. 3, an index out of range, models NULL or not finite where a
 * member needs it; DSA_ERR_CAPACITY: not even one group of 64 members fits the smaller of dsa_set_memory_budget (where one is set) and
 * 1 GiB.  DSA_ERR_DEVICE: the batched kernels' LDS (97 272 bytes at nz = 64) is refused, before anything is launched. */
int dsa_columns_resolution_lateral(dsa_engine* e, int nmaps, const float* obs, const float* wt, float smooth, float damp, float lateral, double tol,
                                   int maxit, int nmembers, const int* kind, const int* index, const double* models, int nrows, double* measures,
                                   double* info, double* full, int* nused, int* flag);

/* dsa_columns_sample_*: Monte-Carlo depth inversion, nchains Metropolis chains of Vs(z) per interior column kept on the device (extension;
 * DESIGN.md 29; the arithmetic is csrc/column_sample.h).
 * dsa_columns_sample_begin opens a dispersion stage of nchains models (dsa_dispersion_begin_models' stage, kmax = nmaps) whose models are the
 * chains, and runs the set-up sweep.  vels, depz, minthk: the start model, dsa_dispersion_begin's; the plan of the runs: nruns entries iwave,
 * igr, nper and all periods one run after the other -- run r writes the maps [sum of the nper before it, + nper[r]), which must add up to
 * nmaps (1 .. 60); obs, wt: nmaps*nx*ny floats as dsa_columns_step's, wt = 1 / sigma of a datum, 0 to drop it, or NULL (all 1).  smooth: the
 * weight of dsa_columns_step's depth Laplacian in the prior psi = smooth^2 |L v|^2; a chain samples exp(-(phi + psi) / (2 temperature)), phi
 * the sum of the squared weighted residuals of the used data, inside the box [max(minvel, v0 - width), min(maxvel, v0 + width)] per node.
 * step: half width of the uniform single-node proposal in km/s; spread: half width of the uniform scatter of chains 1 .. nchains-1 about
 * the start (chain 0 starts at it); seed: of the counter-based generator; burn: sweeps before the moments are taken.  A datum is used where
 * wt > 0, obs > 0 and the start model's curve has a root; a column without one gets flag 2 and is never moved, like the outer ring.
 * dsa_columns_sample_run: nsweeps whole sweeps -- the proposals, one times-only dispersion run per plan entry, the Metropolis tests and the
 * running moments, all on the device; n calls with 1 leave the bits one call with n leaves.
 * dsa_columns_sample_fetch: the finish of the present state, which it leaves as it is.
 *   nodes   5*(nz-1)*nx*ny doubles, (figure, depth, column): the pooled posterior mean, the pooled variance, the mean within-chain variance
 *           W, the variance B of the chain means (/ (nchains - 1); 0 for one chain), the best model -- sd = sqrt(var) and the convergence
 *           figure sqrt((W (n-1)/n + B) / W) are the caller's to take
 *   cols    3*nx*ny doubles: phi of the start, the best phi + psi, the mean kept phi
 *   counts  8*nx*ny ints: nused, flag, accepted, rejected, out of box, no root (summed over the chains; the last two are among the
 *           rejected), the chains put back to the start at the set-up, the sweeps kept n
 *   without a kept sweep (the ring, flag 2, burn >= the sweeps run) nodes and the last two of cols are 0
 * dsa_columns_sample_state: the raw state for tests, every pointer may be NULL: models nz*nchains*nx*ny (depth, chain, column); phi, psi,
 * phisum, nkept, best_e, pnode, pold, pmark (-1 idle, 1 out of box, 2 accepted, 3 rejected, 4 no root), reseeded: nchains*nx*ny (chain,
 * column); counters 4*nchains*nx*ny (accepted, rejected, out of box, no root); S1, S2, best_v (nz-1)*nchains*nx*ny.
 * While the stage is open dsa_columns_step*, dsa_columns_resolution*, dsa_dispersion_get_model and dsa_dispersion_failure return
 * DSA_ERR_STATE (no host copy of the chains exists); dsa_dispersion_fetch works on global maps (chain * nmaps + map), the failure counts stay
 * right; any dsa_dispersion_begin* ends the stage.
 * Errors of begin, all found before the device is touched (a stage that was open stays as it was): DSA_ERR_ARGUMENT: nchains < 1, nx or ny
 * < 3, nz outside 2 .. 64, nchains*nx*ny or nchains*nmaps beyond 2^31 - 1, a NULL vels / depz / obs / plan, a plan entry with iwave outside
 * 1, 2 or nper outside 1 .. 60, periods that do not add up to nmaps, obs or the model not finite, wt negative or not finite, step <= 0,
 * spread < 0, width <= 0, temperature <= 0, smooth < 0 (or any of them not finite), minvel > maxvel, burn < 0.  run, fetch, state without
 * an open stage: DSA_ERR_STATE; nsweeps < 0 and a NULL output of fetch: DSA_ERR_ARGUMENT. */
int dsa_columns_sample_begin(dsa_engine* e, int nx, int ny, int nz, int nchains, const float* vels, const float* depz, float minthk, int nruns,
                             const int* iwave, const int* igr, const int* nper, const double* periods, int nmaps, const float* obs, const float* wt,
                             float smooth, float step, float spread, float width, float temperature, float minvel, float maxvel,
                             unsigned long long seed, int burn);
int dsa_columns_sample_run(dsa_engine* e, int nsweeps);
int dsa_columns_sample_fetch(dsa_engine* e, double* nodes, double* cols, int* counts);
int dsa_columns_sample_state(dsa_engine* e, float* models, double* phi, double* psi, int* counters, double* S1, double* S2, double* phisum, int* nkept,
                             double* best_e, float* best_v, int* pnode, float* pold, int* pmark, int* reseeded);

/* Block proposals of the sample stage, shaped by each column's linearised posterior (extension; csrc/column_sample.h).
 * dsa_columns_sample_shape: the state, nmaps, obs, wt, smooth, damp and the refusals are dsa_columns_resolution's, in its order: a
 * single-model stage whose maps and kernel slots were all run with kernels.  Per interior column the normal matrix dsa_columns_step
 * assembles, N = G^T G + smooth^2 L^T L + damp^2 I, is factored as L D L^T on the device; the model is not stepped and the stage is left as
 * it is (a dsa_columns_step after the call gives the bits it would have given).  tri: (nz-1)*nz/2*nx*ny doubles, (entry, column), the packed
 * lower triangle row by row -- entry i (i + 1) / 2 + j is L_ij for j < i and N_ii for j = i; r: (nz-1)*nx*ny doubles, r_l = 1 / sqrt(d_l);
 * flag: nx*ny ints, dsa_columns_step's (2: no used datum, 1: a pivot not positive; tri and r are then 0, as on the outer ring).  Each of the
 * three may be NULL.  The engine holds the shape, with nx, ny, nz, until the next call or dsa_destroy; no other call reads it.
 * dsa_columns_sample_blocks, between dsa_columns_sample_begin and the first sweep: sweep s >= 1 is a block sweep iff block_every > 0 and
 * s % block_every == 0.  In one, a chain of a column with shape flag 0 proposes v' = v + (float)(block_scale delta) on all nz-1 nodes, L^T
 * delta = y, y_l = (2 u_l - 1) r_l, u_l draw 3 + l of the sweep -- a symmetric proposal of covariance block_scale^2 N^-1 / 3; outside the
 * box of any node nothing is written; the Metropolis test is the single-node one and a rejection restores every node.  A chain of a flagged
 * column makes the single-node proposal.  block_every = 0: off (the default of every dsa_columns_sample_begin).  DSA_ERR_STATE: no open
 * sample stage, a sweep already run, no held shape of the stage's nx, ny, nz; DSA_ERR_ARGUMENT: block_every < 0, block_scale not finite or
 * <= 0; the stage stays as it was.
 * dsa_columns_sample_block_state: the raw block state for tests, each pointer may be NULL: pold_all (nz-1)*nchains*nx*ny floats (depth,
 * chain, column), the values the last block proposal of a chain replaced; counters 3*nchains*nx*ny ints: block proposals made, accepted,
 * out of the box (each also counted by dsa_columns_sample_state's counters).  Zeros while block sweeps are off. */
int dsa_columns_sample_shape(dsa_engine* e, int nmaps, const float* obs, const float* wt, float smooth, float damp, double* tri, double* r, int* flag);
int dsa_columns_sample_blocks(dsa_engine* e, int block_every, double block_scale);
int dsa_columns_sample_block_state(dsa_engine* e, float* pold_all, int* counters);

/* Posterior marginals of the sample stage: per-node histograms, mode and quantiles, and the covariance between the depths of a column
 * (extension; csrc/column_sample.h).  They only observe: with them on, every array of dsa_columns_sample_state,
 * dsa_columns_sample_block_state and dsa_columns_sample_fetch has the bits it has with them off.
 * dsa_columns_sample_marginals, between dsa_columns_sample_begin and the first sweep (before or after dsa_columns_sample_blocks): nbins = 0
 * is off (the default of every dsa_columns_sample_begin); nbins = 2 .. 256 cuts the box [lo, hi] of every node (dsa_columns_sample_begin's)
 * into nbins equal bins.  In every sweep after burn, where the moments are taken, a chain's value v at a depth counts in bin
 * min(nbins - 1, max(0, (int)(((double)v - lo) / (hi - lo) * nbins))) -- bin 0 in a box without width; chain 0 starts at the unclipped
 * start, so a value outside its box is possible and counts in an end bin.  with_cov = 1 also adds d_i d_j, d = v - start, for every pair
 * of depths j <= i of the chain.  The counts and sums are cleared; the buffers come out of the memory budget before anything changes.
 * DSA_ERR_STATE: no open sample stage, a sweep already run; DSA_ERR_ARGUMENT: nbins < 0, 1 or > 256, with_cov not 0 or 1; the stage stays
 * as it was.
 * dsa_columns_sample_marginals_fetch: the finish of the present counts; the state is left as it is and the sweeps may go on.  levels:
 * nlevels (0 .. 16) probabilities, each finite and inside (0, 1).  hist (may be NULL): nbins*(nz-1)*nx*ny unsigned, (bin, depth, column),
 * the counts summed over the chains.  figures (required): (1+nlevels)*(nz-1)*nx*ny doubles, (figure, depth, column): the mode -- the centre
 * lo + (b + 0.5) (hi - lo) / nbins of the first fullest pooled bin b -- then the quantile of every level p: with N the pooled total and
 * target = p N, at the first bin b (ascending) that is not empty and whose cumulated count reaches target, lo + (b + (target - cum) / h_b)
 * (hi - lo) / nbins, cum the count below the bin (linear inside a bin).  cov (may be NULL; needs with_cov): (nz-1)*nz/2*nx*ny doubles,
 * (entry, column), entry i (i + 1) / 2 + j, j <= i: sum over the chains of the products / (nkept nchains) - pm_i pm_j, pm the pooled mean
 * of d; its diagonal has the bits of dsa_columns_sample_fetch's variance.  A node without a kept sweep (the outer ring, flag 2, burn >=
 * the sweeps run) has zeros everywhere.  DSA_ERR_STATE: no open sample stage, the marginals are off, cov without with_cov;
 * DSA_ERR_ARGUMENT: nlevels outside 0 .. 16, a level not finite or outside (0, 1), figures NULL.
 * dsa_columns_sample_marginals_state: the raw per-chain state for tests, each pointer may be NULL: hist nbins*(nz-1)*nchains*nx*ny unsigned,
 * (bin, depth, chain, column); P (nz-1)*nz/2*nchains*nx*ny doubles, (entry, chain, column) (needs with_cov), whose diagonal has the bits of
 * dsa_columns_sample_state's S2.  DSA_ERR_STATE as the fetch. */
int dsa_columns_sample_marginals(dsa_engine* e, int nbins, int with_cov);
int dsa_columns_sample_marginals_fetch(dsa_engine* e, int nlevels, const double* levels, unsigned* hist, double* figures, double* cov);
int dsa_columns_sample_marginals_state(dsa_engine* e, unsigned* hist, double* P);

/* dsa_columns_sample_radial_*: Monte-Carlo radial depth inversion, nchains Metropolis chains of [Vsv ; Vsh] per interior column kept on the
 * device (extension; the arithmetic is csrc/column_sample_radial.h).
 * dsa_columns_sample_radial_begin opens a radial dispersion stage of nchains models -- a Rayleigh run (iwave 2) reads a chain's Vsv, a Love
 * run (iwave 1) its Vsh -- and runs the set-up sweep.  vsv, vsh: the start models (nz*nx*ny floats each, Vsv > 0); depz, minthk, the plan,
 * nmaps, obs, wt, smooth, step, spread, width, temperature, seed, burn: dsa_columns_sample_begin's.  A chain samples exp(-(phi + psi) / (2
 * temperature)) with psi = smooth^2 (|L vsv|^2 + |L vsh|^2) + aniso^2 |vsh - vsv|^2 inside a box per model and node, [max(minvel, v0 - width),
 * min(maxvel, v0 + width)] about the model's own start; minvel > 0.  A proposal moves one Vsv node, one Vsh node or, with pairs = 1, the Vsv
 * and the Vsh of one depth together by the same amount (a third of the proposals each).  A datum is used as in dsa_columns_sample_begin; a
 * column without a used datum of either type gets flag 2 and is never moved, a column with one type missing samples.
 * dsa_columns_sample_radial_run: nsweeps whole sweeps; n calls with 1 leave the bits one call with n leaves.
 * dsa_columns_sample_radial_fetch: the finish of the present state, which it leaves as it is.
 *   nodes   16*(nz-1)*nx*ny doubles, (figure, depth, column): the pooled mean, the pooled variance, W and B (dsa_columns_sample_fetch's) of
 *           Vsv, then of Vsh, then of xi = (Vsh / Vsv)^2; the best model's Vsv and Vsh; the pooled covariance of Vsv and Vsh; the share of
 *           the kept states with Vsh > Vsv
 *   cols    3*nx*ny doubles: phi of the start, the best phi + psi, the mean kept phi
 *   counts  15*nx*ny ints: nused (Rayleigh), nused (Love), flag, accepted, rejected, out of box, no root, proposed per kind (Vsv, Vsh,
 *           pair), accepted per kind, the chains put back to the start at the set-up, the sweeps kept n
 *   without a kept sweep nodes and the last two of cols are 0
 * dsa_columns_sample_radial_state: the raw state for tests, every pointer may be NULL: vsv, vsh nz*nchains*nx*ny (depth, chain, column); phi,
 * psi, phisum, nkept, best_e, pnode (kind * (nz-1) + depth), pold_v, pold_h, pmark, reseeded: nchains*nx*ny; counters 4*nchains*nx*ny; kinds
 * 6*nchains*nx*ny; S1v, S2v, S1h, S2h, Pvh, X1, X2, npos (int), best_vsv, best_vsh (nz-1)*nchains*nx*ny.
 * While the stage is open everything an open dsa_columns_sample_begin stage refuses returns DSA_ERR_STATE, and so do
 * dsa_dispersion_get_model_radial, dsa_kernels_from_dispersion_radial, dsa_solve_rows_radial, dsa_update_radial and every
 * dsa_columns_sample_* entry above.  Leaving the stage: only a dsa_dispersion_begin* (dsa_dispersion_begin, _begin_models, _begin_radial)
 * or another dsa_columns_sample_radial_begin ends it.  dsa_columns_sample_begin does not: on an open radial stage it is refused like the
 * other isotropic entries, before its arguments are looked at and with the radial stage left as it was, so that a caller who mixes the two
 * families up loses no chains; call dsa_dispersion_begin first, then dsa_columns_sample_begin -- the isotropic stage that follows has a
 * fresh engine's bits.  run, fetch and state return DSA_ERR_STATE without an open radial stage (an open dsa_columns_sample_begin stage
 * is none).
 * Errors of begin, all found before the device is touched (a stage that was open stays as it was): dsa_columns_sample_begin's, and
 * DSA_ERR_ARGUMENT: a NULL vsh, vsh not finite, vsv not > 0, aniso < 0 or not finite, minvel <= 0, pairs outside 0, 1. */
int dsa_columns_sample_radial_begin(dsa_engine* e, int nx, int ny, int nz, int nchains, const float* vsv, const float* vsh, const float* depz, float minthk,
                                    int nruns, const int* iwave, const int* igr, const int* nper, const double* periods, int nmaps, const float* obs,
                                    const float* wt, float smooth, float aniso, float step, float spread, float width, float temperature, float minvel,
                                    float maxvel, unsigned long long seed, int burn, int pairs);
int dsa_columns_sample_radial_run(dsa_engine* e, int nsweeps);
int dsa_columns_sample_radial_fetch(dsa_engine* e, double* nodes, double* cols, int* counts);
int dsa_columns_sample_radial_state(dsa_engine* e, float* vsv, float* vsh, double* phi, double* psi, int* counters, int* kinds, double* S1v, double* S2v,
                                    double* S1h, double* S2h, double* Pvh, double* X1, double* X2, int* npos, double* phisum, int* nkept, double* best_e,
                                    float* best_vsv, float* best_vsh, int* pnode, float* pold_v, float* pold_h, int* pmark, int* reseeded);

/* dsa_columns_step_radial_lateral: dsa_columns_step_radial with neighbouring columns coupled (extension).  The state, obs, wt,
 * smooth, damp, aniso, dvmax, minvel, maxvel and the outputs dv, nused, chi2, flag are dsa_columns_step_radial's, with its rules and order of
 * refusals (a stage that is not radial is DSA_ERR_STATE).  The step of all interior columns together minimises the sum of
 * dsa_columns_step_radial's objectives of the columns, plus, over the edges of dsa_columns_step_lateral,
 *   lateral^2 sum_edges [ |(vsv_c + xv_c) - (vsv_c' + xv_c')|^2 + |(vsh_c + xh_c) - (vsh_c' + xh_c')|^2 ]
 *   + lateral_aniso^2 sum_edges |(a_c + u_c) - (a_c' + u_c')|^2,   a = vsh - vsv, u = xh - xv:
 * the roughness of the two stepped models, and the roughness of the stepped anisotropy field Vsh - Vsv by a weight of its own, so that xi
 * can be smoothed more strongly than the velocities.  Edges exist iff lateral > 0 or lateral_aniso > 0.  A column takes part as in
 * dsa_columns_step_lateral: flag 1 is left alone and no edge touches it; with edges a column without a used datum of either type takes part
 * (nused 0 0, flag 0) and both its models are carried by its neighbours.  Solved by dsa_columns_step_lateral's preconditioned conjugate
 * gradients with the columns' own 2(nz-1) x 2(nz-1) factors, tol, maxit and info as there; fp64, every sum in a fixed order
 * (csrc/column_radial_lateral.h).  lateral = 0 and lateral_aniso = 0 is no iteration: every output and both stepped models are
 * dsa_columns_step_radial's bit for bit, flag 2 included, and info[3] is the residual of that direct solve.
 * Afterwards as dsa_columns_step_radial: both models stepped where they lie, the marks cleared, the ring and the bottom depth kept.
 * Errors, all found before the device is touched: as dsa_columns_step_radial, in its order; then DSA_ERR_ARGUMENT: lateral or lateral_aniso not
 * finite or < 0, tol not finite or <= 0, maxit < 1; DSA_ERR_CAPACITY: the loop's workspace exceeds dsa_set_memory_budget, held against it as
 * dsa_columns_step_lateral's.  DSA_ERR_DEVICE as dsa_columns_step_radial (the set-up needs its LDS), before anything is launched. */
int dsa_columns_step_radial_lateral(dsa_engine* e, int nmaps, const float* obs, const float* wt, float smooth, float damp, float aniso, float lateral,
                                    float lateral_aniso, float dvmax, float minvel, float maxvel, double tol, int maxit, float* dv, int* nused,
                                    double* chi2, int* flag, double* info);

/* dsa_columns_resolution_radial: how far the radial step's answer can be trusted, per interior column, from the 2M x 2M normal matrix
 * dsa_columns_step_radial factors (extension).  The state and obs, wt, smooth, damp, aniso are dsa_columns_step_radial's, with
 * its rules, messages and order of refusals; of obs only the sign is used.  Per column, M = nz-1, unknown i < M in the Vsv block and i >= M in
 * the Vsh block at depth i mod M: T (nmaps x 2M) has in row k the solution of N t = g^_k for a used datum (g_k in the block of its wave type,
 * 0 elsewhere; the step's substitutions) and zeros for any other; R = T^T G^, its column j the answer to a spike in unknown j.  Everything
 * fp64, every sum sequential from 0.0 over the used data ascending (csrc/column_radial_resolution.h).
 *   measures  6*2(nz-1)*nx*ny doubles, (measure, unknown, column): R_jj;  m1_own = sum R_ij^2 over i in j's block;  m2_own = sum R_ij^2
 *             (depz_i - depz_j)^2 over that block -- the vertical length of the PSF is sqrt(m2_own / m1_own);  m1_cross = sum R_ij^2 over the
 *             other block, the energy a spike in j leaks into the other model;  R_cross, the entry of column j at the co-located unknown of
 *             the other block;  var_j = sum_k T_kj^2
 *   pair      2*(nz-1)*nx*ny: cov_l = sum_k T_kl T_k,M+l;  vard_l = sum_k (T_k,M+l - T_kl)^2, the variance of dVsh - dVsv at depth l -- both
 *             for unit variance of the weighted data
 *   leverage  nmaps*nx*ny: h_k = sum_l g_kl T_k,l in the datum's own block; 0 for a datum not used
 *   trace     2*nx*ny: sum_j R_jj over the Vsv block, then over the Vsh block;  nused 2*nx*ny, flag nx*ny: as dsa_columns_step_radial's
 *   R         NULL, or 2(nz-1)*2(nz-1)*nx*ny doubles: R_ij at (i*2(nz-1) + j)*nx*ny + column.  NULL skips the store and changes no other bit.
 * A column with flag 1 or 2 and the outer ring of columns have 0.0 everywhere; a column with one wave type unused still resolves.  At
 * aniso = 0 the own-block measures, var and the leverages of each block have the bits of dsa_columns_resolution on that model with the other
 * wave type's weights 0, and m1_cross, R_cross and cov are zeros.
 * Nothing is changed: both models, the marks and the Frechet rows' sensitivities stay, so a dsa_columns_step_radial after the call gives the
 * bits it would have given without it; after a step the call is DSA_ERR_STATE until the runs are repeated.
 * Errors, all but the last found before the device is touched: as dsa_columns_step_radial, in its order (DSA_ERR_STATE on a stage that is not
 * radial); DSA_ERR_ARGUMENT for a NULL measures, pair, leverage, trace, nused or flag; DSA_ERR_DEVICE when a column's work arrays (158 712
 * bytes at nz = 64 with 60 maps) exceed the LDS a block of the device may have or the device refuses that size. */
int dsa_columns_resolution_radial(dsa_engine* e, int nmaps, const float* obs, const float* wt, float smooth, float damp, float aniso,
                                  double* measures, double* pair, double* leverage, double* trace, int* nused, int* flag, double* R);

/* Radial anisotropy in the direct 3-D inversion (extension): a radial stage (dsa_dispersion_begin_radial) through the whole
 * direct loop on the device.  Rayleigh data touch only Vsv, Love data only Vsh; the cross sensitivities are neglected; each period's rays
 * are traced through the map of the model of its wave type.  n = 2*maxvp unknowns, maxvp = (nx-2)(ny-2)(nz-1): the Vsv block, then Vsh.
 *
 * dsa_kernels_from_dispersion_radial: dsa_kernels_from_dispersion for a radial stage.  The depth factor of slot s is
 * dsa_kernels_from_dispersion's rule on Vsh where the slot was run with iwave == 1 (Love) and on Vsv otherwise, bit for bit; a per-slot
 * block table (0 Vsv, 1 Vsh) stays on the device.  DSA_ERR_STATE: no stage, a stage that is not radial, or one of the kmax_total slots
 * without a fresh mark of a dsa_dispersion_run with kernels.  Afterwards dsa_solve_rows works on these factors, columns unshifted.
 *
 * dsa_solve_rows_radial: dsa_solve_rows whose entries of a unit on a Love slot have their column shifted by maxvp -- column
 * B*maxvp + k*layer + i + 1, B the block of the unit's sen_slot -- entries, order, values and the |val| > 1e-4 rule unchanged.  rw / iw /
 * col are all given (host COO) or all NULL: the rows stay on the device for dsa_iteration_system_radial_device, whatever the option
 * rows_on_device says, which is left as found.  DSA_ERR_ARGUMENT: only some of the three arrays, or 2*maxvp beyond an int; DSA_ERR_STATE:
 * no plan, no radial depth factors of the present models, or several engines sharing the call; DSA_ERR_CAPACITY as dsa_solve_rows.
 *
 * dsa_iteration_system_radial_device: the joint system on the rows dsa_solve_rows_radial left on the device.  The data rows, datweight and
 * cbst[0 .. dall) exactly as dsa_iteration_system_azimuthal_device.  Below them (csrc/radial_system.h): the Laplacian rows of block 0
 * weighted weight0 at rows dall + index, those of block 1 weighted weight_h at rows dall + maxvp + index, and maxvp tie rows at
 * dall + 2*maxvp + index with the two entries { column index + 1, 0.0f - aniso }, { column maxvp + index + 1, aniso } and the right-hand
 * side cbst = 0.0f - aniso * (vsh - vsv) (fp32) at the unknown's node of the resident models: the tie penalises the anisotropy of the
 * stepped model.  The tie rows are always present: m = dall + 3*maxvp, n = 2*maxvp.  norm[2*maxvp] and dws[4] = { max, mean } per block
 * as the azimuthal builder's.  Every argument is checked before the device is touched.  DSA_ERR_ARGUMENT: a NULL, bad dimensions, or
 * weight0, weight_h or aniso negative or not finite; DSA_ERR_STATE: no radial rows resident, or a system already built from them;
 * DSA_ERR_CAPACITY as the azimuthal builder.  dsa_lsmr, dsa_lsmr_batch, dsa_lsmr_resolution and dsa_resolution_blocks (nblocks = 2) run
 * on the system; dsa_lsmr_tradeoff and dsa_lsmr_crossval, which would rescale the tie rows too, are DSA_ERR_STATE on it.
 *
 * dsa_update_radial: dv[2*maxvp], the Vsv block then the Vsh block, applied to the two resident models where they lie, with
 * dsa_model_update's comparisons and dvmax in place of 0.5; the ring and the bottom depth stay.  The marks are cleared and the radial
 * depth factors are stale afterwards: dsa_solve_rows_radial is DSA_ERR_STATE until the runs and dsa_kernels_from_dispersion_radial have
 * been repeated.  DSA_ERR_STATE on a stage that is not radial; DSA_ERR_ARGUMENT: dimensions other than the stage's, a NULL dv, dvmax not
 * finite or <= 0, minvel > maxvel. */
int dsa_kernels_from_dispersion_radial(dsa_engine* e);
int dsa_solve_rows_radial(dsa_engine* e, float* dsurf, float* rw, int* iw, int* col, long long capacity, long long* nar);
int dsa_iteration_system_radial_device(dsa_engine* e, int nx, int ny, int nz, int dall, const float* obst, const float* dsyn, float threshold0,
                                       float weight0, float weight_h, float aniso, float* cbst, float* datweight, float* norm, int* m_out,
                                       long long* nar_out, float* dws);
int dsa_update_radial(dsa_engine* e, int nx, int ny, int nz, const float* dv, float dvmax, float minvel, float maxvel);

/* copy one unit's coarse travel-time field (nnz, nnx column-major) back; valid after dsa_solve
 * for units of the last chunk only unless keep_fields was requested */
int dsa_get_dims(const dsa_engine* e, int* nnx, int* nnz);
int dsa_keep_fields(dsa_engine* e, int on);
int dsa_get_field(dsa_engine* e, int unit, float* ttn);
int dsa_get_velocity(dsa_engine* e, int map, float* veln);
/* refined snapshot of a unit: ttnr (rnz, rnx) and status (-1 far, 0 alive, 1 close) */
int dsa_get_refined(dsa_engine* e, int unit, int* rnx, int* rnz, float* ttnr, int8_t* status);

/* raw state of a resident unit for diagnostics: which = 0 coarse T (sign bit = pinned), 1 coarse
 * tau (sign bit = queued), 2 refined T, 3 refined tau (rnx*rnz floats, leading dimension rnz) */
int dsa_debug_field(dsa_engine* e, int unit, int which, float* out);

/* Non-fatal diagnostics of the boundary (SURVEY.md 8b "Error convention").
 * dispersion: curves of the dispersion runs since dsa_dispersion_begin that ended with the reference's "improper initial value in
 *   disper - no zero found" (surfdisp96.f:308-339; the rest of such a curve is zero, :342-348): their number, the first one in call
 *   order as first[5] = { iwave (1 Love, 2 Rayleigh), igr, column (1-based, (jj-1)*nx+ii), perturbation (0 = the model itself, else
 *   1 + 6 depth + 2 parameter + sign of the depth-kernel differences), period index k }, and that period.
 * rays: traced rays of the last dsa_solve_rows that were clamped at the model boundary (reference rbint, CalSurfG.f90:2082-2101,
 *   reported by the note of :1447-1454), and the planned unit of the first of them (-1: none). */
int dsa_dispersion_diagnostics(const dsa_engine* e, long long* count, int* first, double* period);
/* The failing curves one by one (reference surfdisp96.f:308-339 writes its block, with the call's layer table, once per failing
 * surfdisp96 call).  Option "disp_failure_log" = N > 0 keeps the first N of them in the reference's single-thread call order (wave type
 * by wave type; column by column, the model itself, then its depth-kernel perturbations: CalSurfG.f90:44-150); dsa_dispersion_failure
 * replays curve `index` (0-based) on the host and returns what the block prints: info[8] = { ifunc (1 L, 2 R), igr, column
 * (jj-1)*nx+ii, perturbation, k, ie (periods of the call; is = 1), mmax, failures logged }, vals[4] = { t(k), cc, cm, c1 },
 * table[800] = d, a, b, rho of the flattened layers (200 each, mmax used), c[60] = the roots of the periods before k (the reference
 * also prints c(k), an element it never assigned: 0 here).  DSA_ERR_ARGUMENT beyond the logged ones. */
int dsa_dispersion_failure(const dsa_engine* e, int index, int* info, double* vals, float* table, double* c);
int dsa_ray_diagnostics(const dsa_engine* e, long long* clamped, int* first_unit);

/* Exact time ties (DESIGN.md "Ties").  The fixed-point solve lands on the reference's Fast-Marching travel times except downstream of bit-equal
 * times of two neighbouring narrow-band nodes, where the reference's own answer depends on the layout of its binary tree (CalSurfG.f90:417-485,
 * :768-921).  Option "exact_ties":
 *   1 (default)  fixed point, then a census of the converged fields.  A node holds a tie when a near neighbour's ACCEPTANCE time equals its value bit for
 *                bit (for all but ~0.02 % of the nodes that is the neighbour's value), or -- round 6 -- when an exceptional outer node was accepted at
 *                the very clock of the neighbour taken in last, or when a node of the refined box ranks equal with the node that ended the refined
 *                stage (the hand-off's probe); the tie's influence is what deciding it the other way changes at the node.  Flagged and solved again by
 *                the reference's march itself (four units per wavefront; field, refined snapshot and receiver times then the reference's bit for bit):
 *                  - a unit holding a tie whose influence exceeds "tie_threshold";
 *                  - "tie_map_strict" (on): on a map where some unit holds such a tie -- a tie-prone medium: sharp contrasts, second-order stencils
 *                    switching along ridges, where a one-ulp difference grows downstream -- every unit holding a tie with ANY influence;
 *                  - (a tie at the hand-off that changes what the coarse grid receives -- a difference of first order, not an ulp -- is not flagged but
 *                    resolved: the refined box is marched literally and handed off again, "handoff_replay"; only a full list of such units, 256 a launch,
 *                    flags the rest; where the refined box's slowness does not vary along x -- a 1-D model: the two choices are mirror images -- it counts);
 *                  - a unit whose band march could not leave its tree a heap, or whose bundle froze a cycle ("tie_frozen_bundles");
 *                  - "tie_scale_guard" (on): a unit holding a tie whose times lie outside the MEASURED ENVELOPE.  Downstream of one-ulp ties the fixed
 *                    point's field differs from the reference's by a number of ulps of the travel time that grows with the grid -- at a receiver at
 *                    most 26 ulps on grids up to 1025 nodes per side in 2.2 M fuzzed units (9.92e-5 s), 36 and 27 ulps in two units of the next 0.7 M (1.37e-4 s, 1.03e-4 s: at 1025^2 with
 *                    times of 32-64 s about one unit in 400 000 ends beyond the bar -- the tolerance is statistical there; lower "tie_tolerance" for a margin), 35 at 2049^2, 110 at 4097^2 -- so against the absolute bar
 *                    ("tie_tolerance", 1e-4 s) it is the size of the times that decides: a unit whose farthest receiver (great-circle distance x the
 *                    map's mean slowness) lies at 64 s or beyond on grids up to 1025^2 -- 32 s at 2049^2, 16 s at 4097^2 -- is marched.
 *                What stays with the fixed point: units without a tie (measured: bit-identical to the reference but for 5 of 83 000 such units, off by an
 *                ulp at a receiver: DESIGN.md "Ties", known residuals), and -- on maps where no tie reaches the threshold -- units holding ties of an
 *                ulp or two: within 1e-4 s of the reference BY MEASUREMENT (about 450 000 smooth-medium units x 32 receivers: worst 5.7e-6 s at 121^2-193^2,
 *                9.5e-5 s at 1025^2 with times of 32-64 s: the envelope the scale guard above holds the call to), not by
 *                construction (DSA_STAT_TIE_UNITS_TIED counts them, the
 *                shim says so once per call).  No rule on a unit's own ties -- largest, summed, counted influence -- separates the rare unit that ends
 *                beyond 1e-4 s from the thousands that do not (profiles/r06_tie_rule_scan_*.log).
 *                Cost: a few per cent where nothing is flagged; a flagged unit costs one march (sequential accepts, ~2.3 us each: 35 ms at 121^2,
 *                2.4 s at 1025^2, a minute at 4097^2 -- the same for one unit or thousands side by side): a tie-prone medium runs at the march's rate;
 *   2            every unit by the march (the guarantee; ~2 000 solves/s at 1025^2 with 16 000 units in flight, ~50 at 4097^2);
 *   0            the fixed point alone; the census still runs ("tie_detect") and DSA_STAT_TIE_UNITS / DSA_STAT_TIE_UNITS_LEFT / dsa_unit_ties say
 *                which units a default call would have marched.
 * The march's tree holds at most 65 534 nodes per unit (16-bit slots): a narrow band longer than that returns DSA_ERR_INTERNAL (grids beyond ~8000
 * nodes per side; the grid size limit above is lower).
 * dsa_unit_ties: per planned unit of the last solve, flags (bit 0: holds a tie above the threshold, bit 1: solved by the march) and the largest
 * tie influence in seconds (either array may be NULL). */
int dsa_unit_ties(const dsa_engine* e, int nunits, int* flags, float* influence);
/* (round 6) what else the census keeps per planned unit of the last solve: how many of the unit's ties have an influence at all, the sum of those
 * influences in seconds (sub-threshold ties add up along a front: options tie_sum_threshold / tie_count_threshold flag by them), and the cycles
 * the unit -- or, for a bundled unit, its bundle -- froze (option tie_frozen_bundles).  Any array may be NULL. */
int dsa_unit_tie_sums(const dsa_engine* e, int nunits, int* count, float* sum, int* frozen);
/* rounds the coarse fixed-point solve of each planned unit took in the last dsa_solve (a bundled unit: its bundle's) */
int dsa_unit_rounds(const dsa_engine* e, int nunits, int* rounds);

/* Device self-check, on no product path (tests/test_gpu_boundary.py): the hand-expanded divisions of the dispersion and ray kernels
 * (dispersion_core.h: recip_of / div_by; ray_core.h: recipf_of / divf_by) against the compiler's IEEE division on `millions` x 1e6 random operand
 * pairs per precision, five numerators per denominator, zeros / infinities / NaN among the numerators.  exponents8: unbiased binary exponent
 * ranges {numerator lo, hi, denominator lo, hi} for fp64, then for fp32.  out4: fp64 pairs, fp64 quotients that differ bitwise, fp32 pairs, fp32
 * quotients that differ.  Needs no engine; uses the current device. */
int dsa_selfcheck_divisions(unsigned long long seed, int millions, const int* exponents8, unsigned long long* out4);
/* device self-check of the bundled node trip's arithmetic helpers (csrc/eikonal_core.h: sqrt_nonneg, min_canon, min3_sel) against their plain forms,
   `millions` * 1e6 operands each: out5 = { square roots tried, that differ from sqrtf bitwise, arguments the helper's guard left to sqrtf,
   minima tried, that differ } */
int dsa_selfcheck_trip(unsigned long long seed, int millions, unsigned long long* out5);

/* probe builds only (-DDSA_LEDGER, tools/isa_ledger.py): trip counters of the coarse solve's phases, summed over the units of the last solve */
int dsa_debug_counters(const dsa_engine* e, double* out24);

/* counters of the last dsa_solve: see DSA_STAT_* */
enum { DSA_STAT_MS_TOTAL = 0, DSA_STAT_MS_FIM_COARSE, DSA_STAT_MS_FIM_REFINED, DSA_STAT_MS_STAGES,
       DSA_STAT_LAUNCHES_FIM_COARSE, DSA_STAT_UNITS, DSA_STAT_ROUNDS_MAX, DSA_STAT_EVALS_TOTAL,
       DSA_STAT_CHUNK, DSA_STAT_RESCANS, DSA_STAT_FREEZES, DSA_STAT_RAYS, DSA_STAT_RAY_STEPS,
       DSA_STAT_RAYS_CLAMPED, DSA_STAT_MS_RAYS, DSA_STAT_MS_ROWS, DSA_STAT_NAR, DSA_STAT_MS_DISPERSION,
       DSA_STAT_CURVES, DSA_STAT_CHANGES_TOTAL, DSA_STAT_TIE_UNITS, DSA_STAT_EXACT_UNITS, DSA_STAT_EXACT_POPS,
       DSA_STAT_MS_EXACT, DSA_STAT_FIELD_SLOTS, DSA_STAT_FOOTPRINT_MB, DSA_STAT_BUNDLE_SIZE, DSA_STAT_BUNDLES,
       DSA_STAT_BUNDLED_UNITS, DSA_STAT_BUNDLE_SLOTS, DSA_STAT_BUNDLE_THREADS,
       DSA_STAT_TIE_UNITS_LEFT,       /* units the tie detector flagged (DSA_STAT_TIE_UNITS, filled in every mode) that stayed with the fixed point: exact_ties = 0 */
       DSA_STAT_TIE_INFLUENCE_MAX,    /* largest tie influence met (seconds) */
       DSA_STAT_EXACT_POOL,           /* units the last march held side by side */
       DSA_STAT_EXACT_TILES,          /* > 0: it marched in pooled tiles, that many 8x8-node tiles per unit */
       DSA_STAT_TIE_UNITS_STRICT,     /* (round 6) of DSA_STAT_TIE_UNITS: flagged only because their map is tie-prone (option tie_map_strict) */
       DSA_STAT_TIE_PRONE_MAPS,       /* maps on which some unit held a tie above tie_threshold, summed over the call's launches */
       DSA_STAT_TIE_UNITS_TIED,       /* units that stayed with the fixed point although the census found a tie with an influence in them: their times are the
                                         reference's to ~1e-4 s statistically, not by construction (DESIGN.md "Ties") */
       DSA_STAT_TIE_UNITS_BY_SCALE,   /* of DSA_STAT_TIE_UNITS: flagged because they hold a tie and their travel times lie outside the envelope in which the
                                         fixed point's tie errors were measured to stay within the tolerance (option tie_scale_guard) */
       DSA_STAT_HANDOFFS_REPLAYED,    /* units whose refined box was marched literally behind the hand-off's probe (a node ranking equal with the one that ended the refined
                                         stage changed what the coarse grid receives: the reference's own tree decides; option handoff_replay) */
       DSA_STAT_RAY_LAUNCHES,         /* launches of the ray kernel (option ray_budget bounds the rays of one) */
       DSA_STAT_COUNT };
int dsa_get_stats(const dsa_engine* e, double* out /* DSA_STAT_COUNT + 8: counters, then 8 phase-clock sums (probe builds) */);

/* ---- drop-in level -------------------------------------------------------------------------- */
int dsa_calsurfg(const int* nx, const int* ny, const int* nz, const int* nparpi, const float* vels,
                 int* iw, float* rw, int* col, float* dsurf,
                 const float* goxdf, const float* gozdf, const float* dvxdf, const float* dvzdf,
                 const int* kmaxRc, const int* kmaxRg, const int* kmaxLc, const int* kmaxLg,
                 const double* tRc, const double* tRg, const double* tLc, const double* tLg,
                 const int* wavetype, const int* igrt, const int* periods, const float* depz,
                 const float* minthk, const float* scxf, const float* sczf, const float* rcxf,
                 const float* rczf, const int* nrc1, const int* nsrcsurf1, const int* kmax,
                 const int* nsrcsurf, const int* nrcf, int* nar);

int dsa_synthetic(const int* nx, const int* ny, const int* nz, const int* nparpi, const float* vels,
                  float* obst,
                  const float* goxdf, const float* gozdf, const float* dvxdf, const float* dvzdf,
                  const int* kmaxRc, const int* kmaxRg, const int* kmaxLc, const int* kmaxLg,
                  const double* tRc, const double* tRg, const double* tLc, const double* tLg,
                  const int* wavetype, const int* igrt, const int* periods, const float* depz,
                  const float* minthk, const float* scxf, const float* sczf, const float* rcxf,
                  const float* rczf, const int* nrc1, const int* nsrcsurf1, const int* kmax,
                  const int* nsrcsurf, const int* nrcf, const float* noiselevel);

/* dsa_calsurfg with the azimuthal blocks of dsa_solve_rows_azimuthal (extension): the same argument list and conventions --
 * iw(1) = nar on return, the rows behind it, the capacity of dsa_dropin_set_capacity (state it for 3 nparpi columns per datum).  The
 * Rayleigh depth-kernel slots (phase and group periods) emit gc / gs entries, the Love slots none.  The isotropic entries, dsurf and the
 * diagnostics afterwards are dsa_calsurfg's; columns run to 3*nparpi.  rw / iw / col are host arrays, or NULL together: the rows then
 * stay on the drop-in engine (dsa_solve_rows_azimuthal_device), as dsa_calsurfg's do, for dsa_iteration_system_azimuthal_device on
 * dsa_dropin_engine(); iw(1) is then not written.  Only some of the three NULL: DSA_ERR_ARGUMENT.  DSA_ERR_STATE: more than one
 * engine in the pool (DSA_DEVICES): the azimuthal call is not sharded over GPUs. */
int dsa_calsurfg_azimuthal(const int* nx, const int* ny, const int* nz, const int* nparpi, const float* vels,
                           int* iw, float* rw, int* col, float* dsurf,
                           const float* goxdf, const float* gozdf, const float* dvxdf, const float* dvzdf,
                           const int* kmaxRc, const int* kmaxRg, const int* kmaxLc, const int* kmaxLg,
                           const double* tRc, const double* tRg, const double* tLc, const double* tLg,
                           const int* wavetype, const int* igrt, const int* periods, const float* depz,
                           const float* minthk, const float* scxf, const float* sczf, const float* rcxf,
                           const float* rczf, const int* nrc1, const int* nsrcsurf1, const int* kmax,
                           const int* nsrcsurf, const int* nrcf, int* nar);

/* Forward-model `nmodels` Vs models vels(nx,ny,nz,nmodels), model slowest, in ONE call: times only, no rays, no rows (extension; the
 * reference has no such entry).  goxdf .. nrcf are the arguments of dsa_synthetic between obst and noiselevel, with the same meaning.
 * Column k of dsurf(ldd, nmodels) receives model k's receiver times in the reference's data order; rows beyond the data are left alone.
 *   dicing = 8: the times dsa_calsurfg returns in dsurf for that model (CalSurfG's grid, the phase velocities at the group periods
 *               written over the head of the phase-velocity maps as there);
 *   dicing = 5: the times dsa_synthetic returns with noiselevel 0.
 * Under exact_ties = 2 column k is bit-identical to the single-model call; in the default mode every time is within tie_tolerance
 * (1e-4 s) of it -- the units of a source bundle across models, so a unit's fixed point may run beside other members than alone.
 * All models go through the dispersion stage in one launch per wave type (dsa_dispersion_begin_models) and through the eikonal solves
 * as one unit list, model-major (option forward_models_order).  When the maps of all models do not fit the memory budget the models
 * are processed in passes (option forward_models_chunk; the results do not depend on the split; the pass that holds model 0 runs last).
 * disp_failures (may be NULL) receives the curves without a root per model.  dsa_dropin_tie_diagnostics / _tie_census afterwards sum
 * over all units of the call, dsa_dropin_velocity_maps serves model 0's maps, dsa_dropin_diagnostics the dispersion counts over all
 * models (no rays: rbint_notes 0).
 * DSA_ERR_ARGUMENT: nmodels < 1, ldd below the number of data, dicing not 5 or 8, a null pointer.  DSA_ERR_STATE: more than one engine
 * in the pool (DSA_DEVICES): models are not sharded over GPUs.  After a failure the engine is as usable as after a failed dsa_synthetic. */
int dsa_forward_models(const int* nx, const int* ny, const int* nz, const int* nmodels, const float* vels,
                       float* dsurf, const int* ldd, const int* dicing, long long* disp_failures,
                       const float* goxdf, const float* gozdf, const float* dvxdf, const float* dvzdf,
                       const int* kmaxRc, const int* kmaxRg, const int* kmaxLc, const int* kmaxLg,
                       const double* tRc, const double* tRg, const double* tLc, const double* tLg,
                       const int* wavetype, const int* igrt, const int* periods, const float* depz,
                       const float* minthk, const float* scxf, const float* sczf, const float* rcxf,
                       const float* rczf, const int* nrc1, const int* nsrcsurf1, const int* kmax,
                       const int* nsrcsurf, const int* nrcf);

/* Forward-model `nmodels` models that are built ON THE DEVICE from one base model vsf(nx,ny,nz) and `nmodels` steps, and judge them where
 * their times are (extension).  goxdf .. nrcf as in dsa_forward_models.  Member k's model is dsa_model_update's on a copy:
 * for unknown j = (l (ny-2) + jj)(nx-2) + i, s = steps[k n + j] (n = (nx-2)(ny-2)(nz-1)), s = fl(alpha[k] s) where alpha is not NULL, s
 * clipped to +-0.5, v = vsf(i+1, jj+1, l) + s clipped to [minvel, maxvel], with dsa_model_update's comparisons (a NaN step gives a NaN
 * node); the outer ring in x and y and the bottom layer keep the base value.  No input is modified.
 *   steps == NULL: the steps are the solutions the last batch solve on the drop-in engine (dsa_dropin_engine) left on the device --
 *     dsa_lsmr_batch, _resolution, _tradeoff or _crossval, also when called with x = NULL.  DSA_ERR_STATE unless such solutions are
 *     resident (no batch yet; the matrix was loaded or edited since; the last batch was dsa_lsmr_voronoi's, whose solutions are in cell
 *     space), nmodels equals their number and n the matrix's column count.
 *   models_out (may be NULL): the models, nmodels * nx*ny*nz floats, model slowest -- bit-identical to nmodels dsa_model_update calls.
 *   dsurf(ldd, nmodels) (may be NULL, ldd is ignored then): as dsa_forward_models'; bit-identical to it on those models under
 *     exact_ties = 2, within tie_tolerance in the default mode.  With dsurf NULL nothing of size nmodels * ndata leaves the device.
 *   disp_failures (may be NULL): curves without a root per model.
 *   measures (may be NULL; needs obst): measures[(k ngroups + g) 2 + {0, 1}] = { sum (double)wr^2, sum (double)r^2 } over the data i of
 *     group g, r = fl(obst[i] - t_k[i]), wr = fl(datweight[i] r) (datweight NULL: w = 1).  group[i] in [0, ngroups) (NULL: one group;
 *     ngroups NULL: 1); an empty group gives +0.  fp64 sums in an order fixed by the datum index: the same bits on every call, for either
 *     forward_models_order and any forward_models_chunk.
 * Passes, unit orders, the dispersion sequence and the diagnostics afterwards are dsa_forward_models'.
 * DSA_ERR_ARGUMENT (checked before the engine is created): a null required pointer, nmodels < 1, nx or ny < 3, nz < 2, dicing not 5 or
 * 8, ldd below the number of data when dsurf is given, measures without obst, ngroups < 1, a group id out of range.  DSA_ERR_STATE: as
 * above, or more than one engine (DSA_DEVICES).  After a failure the engine is as usable as after a failed dsa_forward_models. */
int dsa_forward_steps(const int* nx, const int* ny, const int* nz, const int* nmodels, const float* vsf,
                      const float* steps, const float* alpha, const float* minvel, const float* maxvel,
                      float* models_out, float* dsurf, const int* ldd, const int* dicing, long long* disp_failures,
                      const float* obst, const float* datweight, const int* group, const int* ngroups, double* measures,
                      const float* goxdf, const float* gozdf, const float* dvxdf, const float* dvzdf,
                      const int* kmaxRc, const int* kmaxRg, const int* kmaxLc, const int* kmaxLg,
                      const double* tRc, const double* tRg, const double* tLc, const double* tLg,
                      const int* wavetype, const int* igrt, const int* periods, const float* depz,
                      const float* minthk, const float* scxf, const float* sczf, const float* rcxf,
                      const float* rczf, const int* nrc1, const int* nsrcsurf1, const int* kmax,
                      const int* nsrcsurf, const int* nrcf);

/* Capacity (entries) of the rw / iw(2:) / col arrays handed to dsa_calsurfg from now on.  The reference's interface
 * (CalSurfG.f90:939-943) does not carry it -- main.f90:287 sizes the arrays as spfra*dall*nx*ny*nz and only checks
 * afterwards (main.f90:467); with it dsa_calsurfg returns DSA_ERR_CAPACITY instead of writing past the arrays.
 * 0 = not stated (then DSA_MAXNAR from the environment, else unlimited). */
int dsa_dropin_set_capacity(long long maxnar);

/* the reference's aprod (aprod.f90:7-60: mode 1 y += A x, mode 2 x += A^T y; iw = [nar, rows, cols]) on the
 * device; the matrix is uploaded when first seen (dsurftomo_amd/fortran/aprod_shim.f90 exports `aprod_`) */
int dsa_aprod(const int* mode, const int* m, const int* n, float* x, float* y, const int* leniw,
              const int* lenrw, const int* iw, const float* rw);
/* Contract of the device copy behind dsa_aprod: the matrix is uploaded when its address, size or a sample of its
 * entries changes, and whenever a new LSMR solve starts (two mode-2 products in a row: lsmrModule.f90:390 opens a
 * solve with mode 2 and :497 ends every iteration with it) -- which covers the reference's main program, that rebuilds
 * rw / iw in place before each solve (main.f90:361-466).  Any other in-place edit must be announced with this call. */
int dsa_aprod_invalidate(void);

/* the reference's LSMR with its own argument list (lsmrModule.f90:36-39: every argument by reference; iw = [nar,
 * rows, cols], nout ignored) on the device; dsurftomo_amd/fortran/lsmr_shim.f90 exports module lsmrModule with it */
int dsa_lsmr_dropin(const int* m, const int* n, const int* leniw, const int* lenrw, const int* iw, const float* rw,
                    const float* b, const float* damp, const float* atol, const float* btol, const float* conlim,
                    const int* itnlim, const int* localSize, const int* nout, float* x, int* istop, int* itn,
                    float* normA, float* condA, float* normr, float* normAr, float* normx);

/* pv(nx*ny, kmaxXX) of the last drop-in call: which = 0 Rc, 1 Rg, 2 Lc, 3 Lg (what the reference's synthetic
 * writes to velmap2d*.dat, CalSurfG.f90:2559-2617) */
int dsa_dropin_velocity_maps(const int* which, double* pv);

/* Non-fatal diagnostics of the last dsa_calsurfg call, for the caller to print where the reference prints them:
 *   rbint_notes: how many times the reference would have written its six-line boundary note to unit 6 -- once after every
 *     (period, source) iteration from the first one with a clamped ray on (rbint is set once and tested inside the source loop,
 *     CalSurfG.f90:1088, :1447-1454); 0 = no ray touched the boundary;
 *   disp_count / disp_first[5] / disp_period: see dsa_dispersion_diagnostics (the reference writes its block to unit 66).
 * The C level prints nothing itself; dsurftomo_amd/fortran/calsurfg_shim.f90 writes the reference's texts. */
int dsa_dropin_diagnostics(int* rbint_notes, long long* disp_count, int* disp_first, double* disp_period);
/* Tie census of the last dsa_calsurfg / dsa_synthetic call (see dsa_unit_ties): units holding an exact time tie whose influence exceeds the
 * threshold; how many of them stayed with the fixed point (exact_ties = 0 -- their times may differ from the reference's Fast Marching by more
 * than 1e-4 s; the shim writes one line about it to unit 6) and how many were solved again by the reference's march (exact_ties = 1, the default);
 * the largest influence met, in seconds.  Any pointer may be NULL. */
int dsa_dropin_tie_diagnostics(long long* flagged_units, long long* left_to_fixed_point, long long* marched_units, float* largest_influence);
/* (round 6) the same call's units that stayed with the fixed point although the census found a tie with a (sub-threshold) influence in them -- within 1e-4 s
 * of the reference by measurement, not by construction: the shim writes one line about them unless DSA_TIE_NOTE=0 --, the maps found tie-prone (a unit on
 * them holds a tie above the threshold; summed over the call's launches) and the units marched because of their map (option tie_map_strict). */
int dsa_dropin_tie_census(long long* tied_units_left, long long* tie_prone_maps, long long* flagged_by_map);
/* dsa_dispersion_failure of the last dsa_calsurfg call (environment DSA_DISP_FAILURE_LOG = N switches the log on): the shim then writes
 * the reference's unit-66 block once per failing surfdisp96 call, layer table included */
int dsa_dropin_dispersion_failure(int index, int* info, double* vals, float* table, double* c);

/* text of the last error of the process-wide engine used by the drop-in level */
const char* dsa_dropin_error(void);
/* that engine (created on first use; null if no GPU), for engine-level calls that continue a drop-in call on the device */
dsa_engine* dsa_dropin_engine(void);

#ifdef __cplusplus
}
#endif
#endif
