// Engine state behind the opaque dsa_engine handle.
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "bundle_plan.h"
#include "host_geometry.h"
#include "kernels.h"

namespace dsa {

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// A DevBuf that frees itself: every buffer the engine owns (nothing to list in ~Engine).  The plain DevBuf stays for the ones that
// are copied as values and released by hand (spmv_state.h).
template <class T>
struct OwnedBuf : DevBuf<T> {
    OwnedBuf() = default;
    OwnedBuf(const OwnedBuf&) = delete;
    OwnedBuf& operator=(const OwnedBuf&) = delete;
    ~OwnedBuf() { this->release(); }
};

struct SpmvState;

// Defaults of the tie handling (round 5; DESIGN.md "Modes").  exact_ties = 1: the fixed point, a census of its exact ties, and the units
// that hold a tie whose influence on its node exceeds tie_threshold solved again by the reference's march itself.  Where nothing is flagged
// the census costs a few per cent of the solve; a flagged unit costs a march -- one unit's accepts are sequential, 2.3 us each: 35 ms at
// 121^2, 2.4 s at 1025^2, whatever the number of units marching beside it.  tie_threshold 2e-5 s: below it the ties of a smooth medium
// (one ulp of a 100 s travel time is 7.6e-6 s) would flag half of the headline's units for differences that stay inside 1e-4 s
// (profiles/r05_ties_headline.log); it is a heuristic, not a bound -- the guarantee is exact_ties = 2.  exact_ties = 0 opts out
// (DSA_EXACT_TIES=0 for an unchanged Fortran host); the census still runs (tie_detect) and the call reports what it would have flagged.
constexpr int kDefaultExactTies = 1;
constexpr float kDefaultTieThreshold = 2.0e-5f;
// (round 6) the census keeps the SUM and the COUNT of a unit's tie influences beside the largest one; the defaults of the rule that uses them
// are set from the scans under profiles/r06_tie_*: 0 = that part of the rule is off
constexpr float kDefaultTieSumThreshold = 0.0f;
constexpr int kDefaultTieCountThreshold = 0;
constexpr int kDefaultTieFrozenBundles = 0;
// the shortest lists dsa_set_option accepts for the list variant of the solve (k_fim: the refined boxes, kRefMax nodes per side): one layer of the
// longest front a box holds -- its perimeter -- per list, half of it in the ready list (both colours)
constexpr int kMinListCap = 4 * (kRefMax - 1), kMinReadyCap = 2 * (kRefMax - 1);
constexpr int kDefaultTieMapStrict = 1;
constexpr int kHandoffReplayCap = 256;       // units of a launch whose refined box the hand-off may march literally (the rest of such units are flagged: the whole unit marched)
constexpr float kTieUlpsAt1025 = 26.0f;      // what a receiver time of the fixed point differs by from the reference's downstream of one-ulp ties, at most, in ulps, on grids up to 1025 nodes per side (measured: 26 = 9.92e-5 s at 32-64 s, the worst of the first 2.2 M fuzzed units; two units of the next 0.7 M reached 36 and 27: not a bound; Engine::tie_verdicts)
// Rays of a launch up to which four lanes trace a ray together (ray_kernels.hip: launch_rays; profiles/r05_ab_rays.log)
constexpr int kRayGroupMax = 81920;

struct Engine {
    int device = 0;
    std::string arch;
    hipStream_t stream = nullptr;
    hipEvent_t events[8] = {};
    std::string error;
    int status = 0;

    // model
    GridDesc g{};
    int nmaps = 0;
    size_t nfield = 0;         // nodes of the coarse grid
    size_t nrec_c = 0;         // records of its tiled storage (padded to whole tiles)
    bool have_maps = false;
    float dpl = 0.0f;          // minimum cell width (km)
    float hmin_slow = 0.0f;    // smallest slowness of the maps (window scale)
    OwnedBuf<float> velv, veln, slow, risti_c, cbasis, rbasis;

    // plan
    bool planned = false;
    bool keep_fields = false;
    std::vector<SourceDesc> h_src;
    std::vector<float> h_risti_r;
    std::vector<RayDesc> h_rays;
    size_t mem_budget = 0;
    size_t per_unit_bytes = 0;
    int chunk = 0;
    int max_chunk = 0;
    float window_cells = 1.25f;        // causal window of the coarse solve in cell travel times (measured optimum 1.0-1.5)
    int list_cap = 0, ready_cap = 0;   // 0 = derive from the grid; else at least kMinListCap / kMinReadyCap (dsa_set_option)
    int last_chunk_first = -1, last_chunk_n = 0;
    bool fields_resident = false;      // the last chunk's coarse fields are still in their slots (not so after a launch that recycled them)

    OwnedBuf<SourceDesc> src;
    OwnedBuf<RayDesc> rays;
    OwnedBuf<float> out;
    OwnedBuf<int32_t> err;
    OwnedBuf<float> slow_r, Tfin_r, risti_r, vcorner;
    OwnedBuf<Rec> F_r, W_c;            // refined records; records of the coarse march windows
    OwnedBuf<float> T_c;               // compact coarse fields (eikonal_core.h)
    OwnedBuf<unsigned long long> exc_c;  // their exception tables
    int exc_log2cap = 0;
    int exc_log2cap_opt = 0;           // option exc_log2cap: initial table size (0 = from the grid); the table grows by itself when it overflows
    int grown_nnx = 0, grown_nnz = 0;
    int exc_log2cap_grown = 0;         // ... and the size it grew to is kept for the later plans of this grid (an inversion solves the same geometry every iteration)
    OwnedBuf<int> seed_r, nseed_r, seed_c, nseed_c, lists, launch_rank;
    // field slots of the coarse solve (kernels.h: FimEnds): T_c, exc_c and lists_c hold `pool_slots` slots; a launch with more units than
    // slots recycles them (only when nobody needs the fields afterwards: no rows, no exact mode, no keep_fields)
    OwnedBuf<int> lists_c, pool_gen;
    OwnedBuf<int32_t> replay_list;     // (round 6) units whose refined box is marched literally behind the hand-off's probe: [0] count, [1 ..] units (kernels.h launch_handoff)
    OwnedBuf<unsigned char> replay_scratch;
    int handoff_replay = 1;            // option handoff_replay: 1 = as above; 0 = a hand-off tie that changes what the coarse grid receives flags the unit (the whole unit marched)
    OwnedBuf<FimEnds> ends_c;
    size_t lists_c_stride = 0;
    int pool_slots = 0;
    int field_pool_opt = 0;            // option field_pool: 0 = automatic (four times the workgroups the chip holds), -1 = one slot per unit, > 0 = that many slots
    size_t per_slot_bytes = 0;
    size_t plan_budget = 0;            // bytes plan() worked with (solve() grows the slot pool inside it when a call needs every field afterwards)
    std::vector<int> h_launch_rank;
    // bundles (bundle_kernel.hip, kernels.h: FimBundle): the units of one source -- its periods -- solved by one workgroup under one shared
    // round schedule.  Option `bundle`: 0 = off, 1 = automatic (default: 16, 8 or 4 members by the sources' unit counts and the memory),
    // 4 / 8 / 16 = that many members per bundle.  Default mode only (the tie detector and the literal march work per unit).
    int bundle_opt = 1;
    int ray_lanes_opt = 0;             // option ray_lanes: lanes per ray of the back-trace, 0 = automatic (4 for launches of up to kRayGroupMax rays, else 1), 1, 4
    float bundle_window_opt = 0.0f;    // option bundle_window_cells: causal window of the bundles, 0 = automatic (bundle_window(): 0.6 cells -- a round's fixed costs are shared by the members, so fewer evaluations per round pay; 1.25 for small wide launches)
    int bundle_G_now = 0;              // members per bundle of the current solve
                                       // (measured at 1025^2, 16 members: 0.4 / 0.5 / 0.6 / 0.8 / 1.25 cells -> 24.4 / 24.6 / 24.4 / 23.9 / 22.7 k solves/s)
    int bundle_threads_opt = 0;        // option bundle_threads: workgroup size of the bundle kernel (0 = automatic: 256; 768 beyond 1500 nodes per side and for small launches)
    int bundle_max_rounds = 0;         // option bundle_max_rounds (tests): > 0 = round limit of the bundles; a bundle that hits it sends its chunk to the unit-by-unit solve
    int bundle_mpl = 0;                // option bundle_members_per_lane: 0 = automatic (bundle_mpl_of), 4, or 2
    bool bundle_wide = false;          // this call's bundles run 768 threads wide on a small grid (choose_bundle_size: a CU per bundle)
    int bundle_mpl_now = 4, bundle_mpl_b = 2;      // ... what the current launch uses (whole bundles; the halved last ones)
    int bundle_threads_b = 256;                    // workgroup size of the second group of a launch (plan_bundles)
    int bundle_tail_opt = 1;                       // option bundle_tail: what a launch of 768 .. 1500 bundles does with the ones beyond the first generation: 1 (default) = whole and 768 threads wide when they are at most 256 (a CU each), 0 = cut in halves (256 threads; also beyond 256)
    int bundle_far_all = 0;                        // option bundle_far_all (A/B): 1 = every node trip fetches all four outer neighbours (round 4's loads)
    int bundles_a = 0, bundles_b = 0, bundle_Gb = 0;      // the launch's bundles: whole ones, and (plan_bundles) the last ones cut in halves of bundle_Gb members on a second stream
    hipStream_t stream2 = nullptr;
    hipEvent_t ev_b0 = nullptr, ev_b1 = nullptr;
    hipError_t make_stream2();
    // Round 5: the REFINED boxes of bundled units are solved in bundles too (option bundle_refined, default on): the same member lists as the
    // coarse bundles, fields of the 129^2 box (1.3 MB per bundle), the members' own refined slowness member-minor, the converged members written back
    // into their (T, tau) records for the hand-off (kernels.h: FimEnds::Fpin, launch_bundle_*).  The unit-by-unit refined solves took 29 ms of the
    // headline step: 5 times the coarse bundles' cost per evaluation.
    int bundle_refined_opt = 1;
    bool refined_bundles_failed = false;      // a refined bundle ran out of rounds / table space: unit by unit until the maps change
    bool refined_bundles_now = false;
    std::vector<FimBundle> h_bundles_r;
    OwnedBuf<FimBundle> bundles_r_d;
    OwnedBuf<FimEnds> ends_r;
    OwnedBuf<float> Br_pool, slowIr;
    OwnedBuf<unsigned long long> exc_br;
    OwnedBuf<int> lists_br, cand_br;
    size_t slowIr_off_b = 0;                   // floats from slowIr to the second group's block
    int bundle_pool_opt = 0;           // option bundle_pool: bundle field slots (0 = up to 1024; fewer than the bundles of a launch: recycled like the unit slots)
    OwnedBuf<float> slowI, B_pool;     // member-minor slowness of all maps; bundle field slots
    bool slowI_ready = false;
    bool bundles_failed = false;       // a bundle of the current maps ran out of rounds: the automatic mode stays unit by unit until the maps change
    OwnedBuf<unsigned long long> exc_b;  // exception tables of the bundle slots
    OwnedBuf<int> lists_b, bpool_gen, member_flag, cand_b;    // (cand_b: tie candidates per bundle slot, kernels.h FimBundle::cand)
    OwnedBuf<FimBundle> bundles_d;
    std::vector<FimBundle> h_bundles;
    std::vector<int> h_member_flag;
    int bundle_slots = 0;
    size_t solve_stage_bytes() const;
    hipError_t bundle_room(size_t* room) const;
    bool grow_unit_pool();
    void release_march_pool();
    bool march_pool_kept = false, released_bundles_for_march = false;      // (exact_ties = 1: the marching pool stays allocated between calls when the device has room, run_exact)
    int bundle_threads() const;
    BundleOptions bundle_options() const;
    float bundle_window() const;
    float bundle_window_tail() const;
    int choose_bundle_size(int step, long* solo_units = nullptr);
    int plan_bundles(int first, int n, int G, int* nsolo, int* nbundles);
    size_t lists_stride = 0;
    int fim_threads = 0;               // workgroup size of the solve kernel; 0 = by grid size (launch_shape)
    int fim_lds_pad = 0;               // dynamic LDS bytes per workgroup of the solve kernel (occupancy limiter)
    int fim_sorted = 1;                // 1: k_fim_sorted (tile masks, record-order sweep), 0: k_fim (lists); same fixed point
    // exact mode (exact_kernel.hip): 0 off; 1 = units whose fixed-point solve met an exact time tie (or froze a cycle) are solved
    // again by the literal Fast Marching; 2 = every unit by the literal Fast Marching only
    int exact_ties = kDefaultExactTies;
    float tie_threshold = kDefaultTieThreshold;     // a tie counts when taking the tied neighbour in moves the node's value by more than this (s); 0 = any tie
    int tie_list_opt = 1;              // option tie_list: 1 = the bundles mark tie candidates as they iterate and the census looks at those only; 0 = the census sweeps the converged field (A/B; also the fallback of a list that overflows)
    int tie_detect = 1;                // option tie_detect: exact_ties = 0 runs the detector too and reports the units it would have flagged (no second solve)
    int exact_lds_slots = 0;           // tree slots kept in LDS per marching unit (8 bytes each, made odd); 0 = by the number of units marching (.. 4799)
    int exact_heap_blocked = 1;        // option exact_heap_blocked: the march's tree beyond its LDS part in blocks of three levels (exact_kernel.hip: xg_gi): 0 never, 1 batches that fill the chip, 2 whenever the LDS part is whole levels
    int exact_pool = 0;                // units marching at a time (0 = by free memory, at most exact_pool_max)
    size_t exact_pool_max = 16384;     // option exact_pool_max: four units per wavefront, sixteen wavefronts per CU (measured at 1025^2: 10 240 units 1 500, 12 288 1 600, 16 384 1 700 solves/s)
    OwnedBuf<unsigned> X_pool;                   // per marching unit: one packed word per node of the whole grid (exact_kernel.hip)
    OwnedBuf<unsigned long long> X_heap;         // ... and the tree slots beyond the LDS part
    // pooled tiles of a times-only march on a large grid (kernels.h XTiles; run_exact)
    OwnedBuf<unsigned short> X_tt, X_free;
    OwnedBuf<unsigned> X_tp, X_ring, X_pins;
    int exact_tiles_opt = 0, exact_tile_cap = 0;
    bool marched_in_tiles = false;
    OwnedBuf<int> x_units, x_nstart;
    OwnedBuf<unsigned long long> x_starts;       // the coarse stage's starting tree per marching unit (kernels.h: exact_start_bytes)
    OwnedBuf<int32_t> xinfo, tieinfo;
    std::vector<unsigned char> h_unit_flags;     // per planned unit after a solve: bit 0 tie met, bit 1 solved by the exact mode
    std::vector<int> h_unit_rounds;               // rounds of the unit's coarse solve (of its bundle's, for a bundled unit)
    std::vector<float> h_unit_tie;               // largest tie influence of the unit (s)
    std::vector<float> h_unit_tie_sum;           // (round 6) sum of the influences of the unit's ties (s) ...
    std::vector<int> h_unit_tie_count;           // ... and how many had one; cycles the unit (its bundle) froze
    std::vector<int> h_unit_froze;
    float tie_sum_threshold = kDefaultTieSumThreshold;      // option tie_sum_threshold: a unit whose ties' influences add up to more than this (s) is flagged; 0 = off
    int tie_count_threshold = kDefaultTieCountThreshold;    // option tie_count_threshold: ... or that holds more ties with an influence than this; 0 = off
    int tie_frozen_bundles = kDefaultTieFrozenBundles;      // option tie_frozen_bundles: 1 = every member of a bundle that froze a cycle is flagged
    int bundle_order_opt = 0;          // option bundle_order: 0 = the first generation's bundles longest first | 1 = bundles of similar length on one CU (plan_bundles)
    int tie_scale_guard = 1;           // option tie_scale_guard: units whose time scale lies outside the measured envelope of the fixed point's tie errors are marched when they hold a tie (Engine::tie_verdicts)
    float tie_tolerance = 1.0e-4f;     // option tie_tolerance: the bar the envelope is held against (s)
    std::vector<float> h_unit_reach_km;                    // per planned unit: great-circle distance to its farthest receiver (plan)
    std::vector<float> map_mean_slow;                      // per map: mean slowness of its vertices (set_maps)
    void mean_slowness_of_maps(const float* hv, size_t nv, int nm);
    int tie_map_strict = kDefaultTieMapStrict;              // option tie_map_strict: on a map where some unit holds a tie above tie_threshold, every unit holding a tie with any influence is flagged
    int tie_verdict(int unit, const int32_t* tie_words, const int32_t* info16, bool member);
    std::vector<char> tie_verdicts(int first, int n, const int32_t* tie_words, const int32_t* info16, bool bundled);
    int run_exact(int first, int n, const std::vector<int>& local_units, bool receivers, bool compact, bool may_pool_tiles = false);
    OwnedBuf<int8_t> S_r, cinit;
    OwnedBuf<int16_t> rst, cst;
    OwnedBuf<int32_t> heap, flags, info;
    OwnedBuf<FimProblem> prob_r, prob_c;
    OwnedBuf<unsigned long long> clocks;
    double phase_ticks[kClockSlots] = {};

    // Frechet rows: depth-kernel factor S (ray_kernels.hip) and per-launch ray scratch
    bool have_sens = false;
    int sens_nz = 0, sens_kmax = 0;
    OwnedBuf<double> Srow, sen_vs, sen_vp, sen_rho;
    OwnedBuf<float> vels_d;
    std::vector<int> h_trace;          // ids of the rays to trace (flag kRayPath), ascending
    size_t ndata = 0;                  // data (travel times / rows) addressed by the planned rays
    size_t ray_budget = 0;             // bytes for ray slabs per launch (0 = default)
    OwnedBuf<int> trace_ids, vlist, nvv, counts, coo_col, coo_iw;
    OwnedBuf<long long> offsets;
    OwnedBuf<float> slabs, coo_rw;
    OwnedBuf<int32_t> rayinfo;
    int ray_path_cap = 0;              // > 0: keep up to that many points of every traced ray (dsa_ray_paths)
    OwnedBuf<float> paths;             // [traced ray][point][colatitude, longitude]
    OwnedBuf<int> path_n;              // points of every traced ray
    // azimuthal rows (dsa_solve_rows_azimuthal): a ray keeps three slabs [iso | c | s], its row the isotropic block and
    // the gc and gs blocks behind it.  Nothing here is allocated before the first azimuthal solve.
    bool azi_now = false;              // the running solve is an azimuthal one (trace_chunk)
    bool sazi_ready = false;           // Sazi is that of the current depth kernels
    OwnedBuf<double> Sazi;             // depth factor of the gc / gs entries (ray_kernels.hip: k_sen_azimuthal)
    std::vector<unsigned char> h_azi_slot_on;      // dsa_set_azimuthal_slots: per depth-kernel slot, 0 = no gc / gs entries; empty = all on
    OwnedBuf<unsigned char> azi_slot_on;
    bool have_azi = false;             // the last azimuthal solve of this plan succeeded: the sums below are its rays'
    std::vector<float> h_azi_sums;     // per traced ray of the plan (position in h_trace, like the path store): sum of cos 2psi, of sin 2psi over its steps
    std::vector<int> h_azi_steps;      // ... and its steps
    // device_rows: the rows stay behind G_rw / G_row / G_col whatever the option rows_on_device says (dsa_solve_rows_azimuthal_device)
    int solve_azimuthal(float* dsurf, float* rw, int* iw, int* col, long long cap, long long* nar, bool device_rows = false);
    // map rows (dsa_solve_rows_maps): the running solve emits rows whose columns are (block, map, vertex) and needs no
    // depth kernels; with azimuthal = 1 it is an azimuthal solve too (azi_now: three slabs per ray, the sums of dsa_ray_azimuths)
    bool maps_now = false;
    int solve_maps(int azimuthal, float* dsurf, float* rw, int* iw, int* col, long long cap, long long* nar);
    int update_maps(int nm, const float* dv, float dvmax, float minvel, float maxvel);
    int get_maps(int nm, float* out_v);

    // dispersion stage (disp_kernels.hip): Vs model -> pv maps + depth kernels, all resident
    bool disp_ready = false;
    int disp_nx = 0, disp_ny = 0, disp_nz = 0, disp_kmax_total = 0, disp_nmaps = 0;
    // model dimension (dsa_dispersion_begin_models): disp_nmodels Vs models share one launch per dispersion_run.  The models sit side by side as
    // columns -- vels_d / h_vels are (depth, model, column), a curve is model * ncol + column -- so k_dispersion runs unchanged on
    // ncol * nmodels columns; the map store is model-major, disp_nmaps maps per model (global map = model * disp_nmaps + m)
    int disp_nmodels = 1;
    std::vector<long long> disp_model_fail;      // curves without a root per model since begin (dsa_dispersion_model_failures)
    int forward_models_chunk = 0;                // option forward_models_chunk: models per pass of dsa_forward_models, 0 = from the memory budget
    int forward_models_order = 0;                // option forward_models_order: unit order of dsa_forward_models, 0 = model-major (default), 1 = period-major (A/B)
    // dsa_forward_steps / dsa_step_models (step_kernels.hip): the base model, the steps of a pass and their factors; the receiver times of a
    // pass, what they are compared with (obst, then datweight) and per datum { first datum, receiver count } of its unit, then its group;
    // the misfit sums of a pass
    OwnedBuf<float> fs_vsf, fs_steps, fs_alpha, fs_models, fs_times, fs_obs;
    OwnedBuf<int> fs_idx;
    OwnedBuf<double> fs_meas;
    std::vector<float> h_depz;
    LayerGeom h_geom{};
    OwnedBuf<LayerGeom> geom;
    OwnedBuf<double> pvstore, curves, tper;
    OwnedBuf<float> disp_ws;
    OwnedBuf<unsigned long long> disp_diag;
    // non-fatal diagnostics of the boundary since dispersion_begin / the last plan (dsa_dispersion_diagnostics, dsa_ray_diagnostics)
    long long disp_fail_count = 0;     // dispersion curves that ended with "no zero found" (surfdisp96.f:308-339)
    int disp_fail_first[5] = {};       // first of them in call order: iwave, igr, column (1-based), perturbation (0 = the model itself), period index k
    double disp_fail_period = 0.0;
    // option disp_failure_log: keep up to that many of the curves without a root, in the reference's call order (column, then
    // perturbation, wave type by wave type), so that a host can print the reference's unit-66 block per failing surfdisp96 call
    // (dsa_dispersion_failure replays the curve on the host for the numbers and the layer table)
    int disp_failure_log = 0;
    struct DispFailRec { int iwave, igr, nper, column, pert, k; double t[60]; };
    std::vector<DispFailRec> disp_failures;
    std::vector<float> h_vels;         // the model of dsa_dispersion_begin (ncol * nz): the replay's input
    OwnedBuf<unsigned long long> disp_fail_list;
    int dispersion_failure(int index, int* info, double* vals, float* table, double* c) const;
    long long rays_clamped = 0;        // traced rays that were clamped at the model boundary (reference rbint, CalSurfG.f90:2082-2101)
    int first_clamped_unit = -1;       // planned unit of the first of them
    int disp_group_shift = -1;         // lanes per Rayleigh curve = 2^shift; -1 = by the number of curves, 0 = one lane per curve
    int disp_layers_lds = -1;          // layer tables of k_dispersion: 1 LDS, 0 global scratch, -1 LDS when they fit
    // depth step of the columns (dsa_columns_step, column_kernels.hip).  One mark per map and per kernel slot: what a
    // dispersion_run with kernels wrote there (wave type, velocity kind, period) and whether it is of the present model -- set by the run,
    // cleared by dispersion_commit, by the step and, for a map, by whatever else writes it.  The step needs map k and slot k fresh and alike.
    struct DispMark { bool fresh = false; int iwave = 0, igr = 0; double t = 0.0; };
    std::vector<DispMark> disp_map_mark, disp_slot_mark;
    OwnedBuf<double> col_S, col_chi2;  // the combined sensitivities of all slots (M, K, ncol); the step's outputs
    OwnedBuf<float> col_obs, col_wt, col_dv;
    OwnedBuf<int> col_nused, col_flag;
    int columns_step(int nmaps_in, const float* obs, const float* wt, float smooth, float damp, float dvmax, float minvel, float maxvel, float* dv, int* nused,
                     double* chi2, int* flag);
    // what dsa_columns_step and dsa_columns_resolution share (who: the caller's name in the messages): the state and the arguments both have,
    // in the step's order of refusals; step: also dvmax, minvel, maxvel; radial: the kind of stage the caller works on (the other kind is refused)
    int columns_front(const char* who, int nmaps_in, const float* obs, const float* wt, float smooth, float damp, bool step, float dvmax, float minvel, float maxvel,
                      bool radial = false);
    // the named steps the five columns_* calls share (engine.hip, below columns_front): one argument check, the coupled steps' checks, the
    // Love mask, stage-in for 1 or 2 models (step: with the step's zeroed outputs), the LDS refusal, the coupled loop, a step's stage-out
    int columns_weight(const char* who, const char* name, float v);
    int columns_coupled_front(const char* who, int blocks, float lateral, float lateral_aniso, double tol, int maxit);
    unsigned long long columns_love() const;
    int columns_stage_in(int models, const float* obs, const float* wt, bool step);
    int columns_lds_refusal(const char* who, int rc, int unknowns, size_t lds, int limit);
    int columns_coupled_loop(const CoupledSystem& s, double tol, int maxit, float dvmax, float minvel, float maxvel);
    int columns_stage_out(int models, float* dv, int* nused, double* chi2, int* flag, const CoupledSystem* s, double* info);
    // depth resolution of the columns (dsa_columns_resolution, k_column_resolution): reads what the step reads, changes nothing
    OwnedBuf<double> col_meas, col_lev, col_trace, col_R;
    OwnedBuf<float> col_depz;
    int columns_resolution(int nmaps_in, const float* obs, const float* wt, float smooth, float damp, double* measures, double* leverage, double* trace, double* R,
                           int* nused, int* flag);
    // depth inversion of the maps' 2 psi terms (dsa_columns_azimuthal, k_column_azimuthal): reads what the step reads
    // and the call's own depth factors col_Z (k_sen_azimuthal's rule; Sazi and Srow are not written), changes nothing.  col_wt gets the
    // effective weights (0 at a Love slot); col_meas, col_lev and col_depz are shared with the plain resolution.
    OwnedBuf<double> col_Z, col_g, col_chi4;
    OwnedBuf<float> col_a1, col_a2;
    int columns_azimuthal(int nmaps_in, const float* obs, const float* a1, const float* a2, const float* wt, float smooth, float damp, double* g, double* measures,
                          double* leverage, double* chi2, int* nused, int* flag);
    int dispersion_get_model(float* vels);
    // radially anisotropic stage and step (dsa_dispersion_begin_radial, dsa_columns_step_radial, k_column_step_radial): a
    // one-model stage in every other sense that keeps a second resident model -- vels_d / h_vels hold Vsv, which the Rayleigh runs read, vsh_d /
    // h_vsh hold Vsh, which the Love runs read.  Set by dispersion_begin_radial, cleared by every other begin (dispersion_setup).
    bool disp_radial = false;
    OwnedBuf<float> vsh_d;
    std::vector<float> h_vsh;
    OwnedBuf<double> col_Sh;           // the combined sensitivities on the Vsh model (col_S: on the Vsv model)
    int dispersion_begin_radial(int nx, int ny, int nz, const float* vsv, const float* vsh, const float* depz, float minthk, int kmax_total, int nmaps_total);
    int columns_step_radial(int nmaps_in, const float* obs, const float* wt, float smooth, float damp, float aniso, float dvmax, float minvel, float maxvel,
                            float* dv, int* nused, double* chi2, int* flag);
    int dispersion_get_model_radial(float* vsv, float* vsh);
    // depth resolution of the radial step (dsa_columns_resolution_radial, k_column_resolution_radial): reads what
    // dsa_columns_step_radial reads, changes nothing; col_meas, col_lev, col_trace and col_R are shared with the plain resolution
    OwnedBuf<double> col_pair;
    int columns_resolution_radial(int nmaps_in, const float* obs, const float* wt, float smooth, float damp, float aniso, double* measures, double* pair,
                                  double* leverage, double* trace, int* nused, int* flag, double* R);
    // laterally coupled step (dsa_columns_step_lateral, k_lateral_*): dsa_columns_step's state, arguments and outputs; the
    // workspace of the conjugate-gradient loop is kept allocated between calls; no call reads what an earlier one left in it.  The host looks at
    // the loop's done flag every lateral_poll iterations.
    OwnedBuf<double> col_lat;
    static constexpr int lateral_poll = 16;
    int columns_step_lateral(int nmaps_in, const float* obs, const float* wt, float smooth, float damp, float lateral, float dvmax, float minvel, float maxvel,
                             double tol, int maxit, float* dv, int* nused, double* chi2, int* flag, double* info);
    // laterally coupled radial step (dsa_columns_step_radial_lateral, k_radial_lateral_setup / _start, then k_lateral_*):
    // dsa_columns_step_radial's state, arguments and outputs, the loop, the poll and the workspace (2 (nz - 1) unknowns per column) of the lateral step
    int columns_step_radial_lateral(int nmaps_in, const float* obs, const float* wt, float smooth, float damp, float aniso, float lateral, float lateral_aniso,
                                    float dvmax, float minvel, float maxvel, double tol, int maxit, float* dv, int* nused, double* chi2, int* flag, double* info);
    // resolution of the laterally coupled step (dsa_columns_resolution_lateral, k_latres_*): reads what
    // dsa_columns_step_lateral reads, changes nothing.  col_lat holds the set-up, col_latH the columns' G^T G, col_latB one chunk of members,
    // col_latM the test models.  A chunk is at most latres_default_cap bytes, or the memory budget where that is smaller.
    OwnedBuf<double> col_latH, col_latB, col_latM;
    static constexpr size_t latres_default_cap = (size_t)1 << 30;
    int columns_resolution_lateral(int nmaps_in, const float* obs, const float* wt, float smooth, float damp, float lateral, double tol, int maxit, int nmembers,
                                   const int* kind, const int* index, const double* models, int nrows, double* measures, double* info, double* full, int* nused,
                                   int* flag);

    // Monte-Carlo depth inversion (dsa_columns_sample_*, k_sample_*): a stage of sample_chains models whose model store
    // (vels_d) holds the chains; everything a sweep reads or writes stays on the device, the host keeps the plan of the runs, the parameters
    // and the number of the last sweep.  sample_open: set by columns_sample_begin, cleared by every dispersion_setup; while it is set the
    // column steps, the resolutions, dispersion_get_model and dispersion_failure are refused.  obs and wt lie in col_obs / col_wt.
    bool sample_open = false, sample_has_wt = false;
    int sample_sweep = 0, sample_burn = 0;
    unsigned long long sample_seed = 0ull;
    double sample_lam2 = 0.0, sample_step = 0.0, sample_spread = 0.0, sample_two_t = 0.0;
    float sample_width = 0.0f, sample_minvel = 0.0f, sample_maxvel = 0.0f;
    struct SampleRun { int iwave, igr, first; std::vector<double> t; };
    std::vector<SampleRun> sample_plan;
    OwnedBuf<float> smp_v0, smp_bestv, smp_pold;
    OwnedBuf<double> smp_phi, smp_psi, smp_S1, smp_S2, smp_phisum, smp_beste, smp_phi0, smp_nodes, smp_cols;
    OwnedBuf<int> smp_cnt, smp_nkept, smp_pnode, smp_pmark, smp_reseed, smp_nused, smp_flag, smp_counts;
    OwnedBuf<unsigned long long> smp_used;
    int columns_sample_begin(int nx, int ny, int nz, int nchains, const float* vels, const float* depz, float minthk, int nruns, const int* iwave, const int* igr,
                             const int* nper, const double* periods, int nmaps_in, const float* obs, const float* wt, float smooth, float step, float spread,
                             float width, float temperature, float minvel, float maxvel, unsigned long long seed, int burn);
    int columns_sample_run(int nsweeps);
    int columns_sample_fetch(double* nodes, double* cols, int* counts);
    int columns_sample_state(float* models, double* phi, double* psi, int* counters, double* S1, double* S2, double* phisum, int* nkept, double* best_e, float* best_v,
                             int* pnode, float* pold, int* pmark, int* reseeded);
    int sample_refused(const char* who);
    // block proposals of the sample stage (dsa_columns_sample_shape, dsa_columns_sample_blocks, dsa_columns_sample_block_state; k_sample_shape,
    // k_sample_*_block).  The shape (blk_tri, blk_r, blk_flag) is built on a single-model stage with columns_resolution's
    // state, held with its dimensions until the next shape call, and read by no other call; sample_block_every > 0 (set by
    // columns_sample_blocks on an open sample stage before its first sweep, cleared by every columns_sample_begin) makes every
    // sample_block_every-th sweep a block sweep.
    bool blk_held = false;
    int blk_nx = 0, blk_ny = 0, blk_nz = 0, sample_block_every = 0;
    double sample_block_scale = 0.0;
    OwnedBuf<double> blk_tri, blk_r;
    OwnedBuf<int> blk_flag, blk_nused, blk_cnt;
    OwnedBuf<float> blk_pold;
    int columns_sample_shape(int nmaps_in, const float* obs, const float* wt, float smooth, float damp, double* tri, double* r, int* flag);
    int columns_sample_blocks(int block_every, double block_scale);
    int columns_sample_block_state(float* pold_all, int* counters);
    // posterior marginals of the sample stage (dsa_columns_sample_marginals, _marginals_fetch, _marginals_state; k_sample_hist, k_sample_cov,
    // k_sample_marginal_finish).  sample_nbins > 0 (set by columns_sample_marginals on an open sample stage before its
    // first sweep, cleared by every columns_sample_begin) makes every sweep after burn count the chains' states in mrg_hist and, with
    // sample_cov, add their products to mrg_P; nothing else of the stage is written.
    int sample_nbins = 0;
    bool sample_cov = false;
    OwnedBuf<unsigned> mrg_hist, mrg_pooled;
    OwnedBuf<double> mrg_P, mrg_fig, mrg_covout;
    int columns_sample_marginals(int nbins, int with_cov);
    int columns_sample_marginals_fetch(int nlevels, const double* levels, unsigned* hist, double* figures, double* cov);
    int columns_sample_marginals_state(unsigned* hist, double* P);
    // Monte-Carlo radial depth inversion (dsa_columns_sample_radial_*, k_sample_radial_*): a radial stage of nchains
    // models -- vels_d holds the chains' Vsv, vsh_d their Vsh, dispersion_run picks by wave type -- with the sample stage's plan, parameters
    // and rules.  sample_radial: set beside sample_open by columns_sample_radial_begin, cleared with it by every dispersion_setup; while it is
    // set everything a sample stage refuses is refused, and so are the isotropic dsa_columns_sample_* entries, dsa_dispersion_get_model_radial
    // and the radial depth-kernel and row entries.  The per-chain figures that have the isotropic stage's shape lie in its buffers (smp_*).
    bool sample_radial = false;
    int sample_pairs = 0;
    unsigned long long sample_love = 0ull;
    double sample_gam2 = 0.0;
    OwnedBuf<float> smr_v0h, smr_bestvh, smr_poldh;
    OwnedBuf<double> smr_S1h, smr_S2h, smr_Pvh, smr_X1, smr_X2, smr_nodes;
    OwnedBuf<int> smr_kcnt, smr_npos, smr_nusedl, smr_counts;
    int columns_sample_radial_begin(int nx, int ny, int nz, int nchains, const float* vsv, const float* vsh, const float* depz, float minthk, int nruns,
                                    const int* iwave, const int* igr, const int* nper, const double* periods, int nmaps_in, const float* obs, const float* wt,
                                    float smooth, float aniso, float step, float spread, float width, float temperature, float minvel, float maxvel,
                                    unsigned long long seed, int burn, int pairs);
    int columns_sample_radial_run(int nsweeps);
    int columns_sample_radial_fetch(double* nodes, double* cols, int* counts);
    int columns_sample_radial_state(float* vsv, float* vsh, double* phi, double* psi, int* counters, int* kinds, double* S1v, double* S2v, double* S1h, double* S2h,
                                    double* Pvh, double* X1, double* X2, int* npos, double* phisum, int* nkept, double* best_e, float* best_vsv, float* best_vsh,
                                    int* pnode, float* pold_v, float* pold_h, int* pmark, int* reseeded);
    int sample_radial_refused(const char* who);      // the entry `who` is an isotropic sample stage's: refused on a radial one

    // radial anisotropy in the direct inversion (dsa_kernels_from_dispersion_radial, dsa_solve_rows_radial, dsa_update_radial; DESIGN.md
    // section 28).  radial_sens: Srow holds the depth factors of every slot on the model of its wave type (k_sen_combine_radial) and
    // radial_block the slots' blocks (0 Vsv, 1 Vsh), both of the present models -- cleared by whatever changes the models, the marks or Srow.
    // radial_now: the running solve emits radial rows (trace_chunk)
    bool radial_sens = false, radial_now = false;
    OwnedBuf<unsigned char> radial_block;
    int kernels_from_dispersion_radial();
    int solve_radial(float* dsurf, float* rw, int* iw, int* col, long long cap, long long* nar);
    int update_radial(int nx, int ny, int nz, const float* dv, float dvmax, float minvel, float maxvel);

    // optional growing host destination of the COO rows (used when several engines share one call)
    std::vector<float>* grow_rw = nullptr;
    std::vector<int>* grow_iw = nullptr;
    std::vector<int>* grow_col = nullptr;

    // COO rows kept on the device across the chunks of a solve (rows_on_device): what dsa_iteration_system_device and LSMR
    // work on without the matrix ever visiting the host (reference: rw / iw / col of main.f90:349-359, 487-489)
    bool rows_on_device = false;
    OwnedBuf<float> G_rw;
    OwnedBuf<int> G_row, G_col;        // 1-based datum (row) and model parameter (column)
    long long G_nar = 0;
    // what the G_nar resident entries are: set by the launch that writes them, cleared wherever G_nar is reset.  The four entries of
    // iteration.hip check it, each taking its own kind of rows only, and its one builder (build_resident_system) commits G_nar and the kind
    // an entry names.  dsa_iteration_system_device takes isotropic rows (or none) and leaves the kind as it is;
    // dsa_iteration_system_azimuthal_device takes kRowsAzimuthal and leaves kRowsJoint (its system, Laplacian rows included: not rows to
    // build from again).
    // kRowsMaps: map rows (dsa_solve_rows_maps) of G_map_blocks blocks on G_map_nmaps maps of an nx x ny vertex grid; only
    // dsa_iteration_system_maps_device takes them, and leaves kRowsMapSystem
    // kRowsRadial: radial rows (dsa_solve_rows_radial) of a Vsv and a Vsh block; only dsa_iteration_system_radial_device
    // takes them, and leaves kRowsRadialSystem
    enum RowsKind { kRowsNone, kRowsIsotropic, kRowsAzimuthal, kRowsJoint, kRowsMaps, kRowsMapSystem, kRowsRadial, kRowsRadialSystem };
    RowsKind G_kind = kRowsNone;
    int G_map_blocks = 0, G_map_nmaps = 0, G_map_nx = 0, G_map_ny = 0;
    template <class T> int ensure_keep(DevBuf<T>& b, size_t n, size_t used);

    bool spmv_attr_set = false;        // LDS attribute of the blocked SpmV kernels set on this engine's device
    SpmvState* spmv = nullptr;         // device copy of a COO matrix for dsa_spmv (spmv.hip)
    int lsmr_device_vectors = 0;       // dsa_lsmr: 1 = vectors and ordered reductions on the device, 0 = on the host (lsmr.hip)

    double stats[DSA_STAT_COUNT + 2] = {};

    ~Engine();
    void fail(int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
    template <class T> int ensure(DevBuf<T>& b, size_t n);
    int init(int device_index);
    int set_maps(int nx, int ny, float goxd, float gozd, float dvxd, float dvzd, int dicing, int nm, const double* pv);
    int plan(int nunits, const int* map_index, const float* scx, const float* scz, const int* nrec, const float* rcx, const float* rcz,
             const int* mode, const int* sen_slot, const int* data_first);
    int set_sensitivity(int nz, int kmax, const float* vels, const float* depz, const double* svs, const double* svp, const double* srho, bool on_device);
    int finish_maps(int nm);
    int dispersion_begin(int nx, int ny, int nz, const float* vels, const float* depz, float minthk, int kmax_total, int nmaps_total, int nmodels = 1);
    // the two halves of dispersion_begin, for models that are built on the device: setup sizes and clears the stage for nmodels models and
    // leaves vels_d (depth, model, column) to be written on the stream; commit declares it written (host_copy: h_vels fetched from it)
    int dispersion_setup(int nx, int ny, int nz, const float* depz, float minthk, int kmax_total, int nmaps_total, int nmodels);
    int dispersion_commit(bool host_copy);
    // steps of a device-built model: d_steps (the pass's, member-major) or, null, the resident batch solutions after resident_steps_check
    int resident_steps_check(const char* who, int nmodels, int n);
    int step_models(int nx, int ny, int nz, int nmodels, const float* vsf, const float* steps, const float* alpha, float minvel, float maxvel, float* models_out);
    int dispersion_run(int iwave, int igr, int nper, const double* t, int with_kernels, int sen_slot, int map_first);
    int dispersion_copy_map(int from, int to, int n);
    int dispersion_fetch(int map_first, int nper, double* pv, int with_kernels, int sen_slot, double* svs, double* svp, double* srho);
    int maps_from_dispersion(float goxd, float gozd, float dvxd, float dvzd, int dicing);
    int kernels_from_dispersion();
    int solve(float* dsurf, float* rw, int* iw, int* col, long long cap, long long* nar);
    int trace_chunk(int first_unit, int n, float* rw, int* iw, int* col, long long cap, long long* nar);
    BatchPtrs batch() const;
    FimLaunch launch_shape(int nnx, int nnz) const;
    FimLaunch shape_c{}, shape_r{};    // launch shapes fixed by plan(): lists_stride is sized from them, solve() must use the same
    void launch_srtimes_chunk(int r0, int nr, int first_unit);
    int get_field(int unit, float* ttn);
    int fetch_tiled(const Rec* dev, int nnx, int nnz, int which, float* out);
    int fetch_compact(int slot, int which, float* out);
    int get_refined(int unit, int* rnx, int* rnz, float* ttnr, int8_t* st);
    int get_velocity(int map, float* out_v);
};

}  // namespace dsa
