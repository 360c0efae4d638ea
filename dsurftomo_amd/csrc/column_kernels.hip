// k_column_step: the depth step of every interior column of the resident model, one wavefront per column.  The
// arithmetic is column_system.h's, shared out over the 64 lanes; a block is one wavefront, so the barrier between the phases costs one
// instruction.  The work arrays lie in LDS, sized by the launch for the case's (M, K): K * M doubles of weighted sensitivities, the packed
// triangle of N (then L), and five short vectors -- 2.5 KB for the Taipei example (M = 8, K = 26: a CU's 160 KB hold more blocks than its
// wave slots), 49 KB at the stage's limits (M = 63, K = 60: three columns per CU, where the triangle alone is 16 KB).
// k_column_resolution, below it: the depth resolution of the same columns on the same factor, the same launch shape.
// k_column_azimuthal: gc(z), gs(z) from the maps' 2 psi terms on that factor, the same launch shape.
// k_column_step_radial: the step on two models, Vsv and Vsh, 2M unknowns per column, the same launch shape.
// k_column_resolution_radial: the resolution of that step's 2M unknowns, a block of two wavefronts per column.
// k_lateral_* (DESIGN.md section 24): the laterally coupled step, a preconditioned conjugate-gradient loop of small launches of that shape.
// the same loop and kernels on the radial step's 2M unknowns per column; only k_radial_lateral_setup and
// k_radial_lateral_start are that system's own.
// k_latres_* (DESIGN.md section 27): the resolution of the laterally coupled step, a batch of section 24's solves, one lane per member.
// k_sample_* (DESIGN.md section 29): the Metropolis chains of the Monte-Carlo depth inversion, one thread per (column, chain).
// k_sample_shape, k_sample_propose_block, k_sample_accept_block: the columns' shapes and the block sweeps.
// k_sample_hist, k_sample_cov, k_sample_marginal_finish: the posterior marginals, one thread per counter or sum.
// k_sample_radial_* (DESIGN.md section 37): the Metropolis chains of [Vsv ; Vsh] of the Monte-Carlo radial depth inversion.
#include "kernels.h"
#include "column_system.h"
#include "column_resolution.h"
#include "column_azimuthal.h"
#include "column_radial.h"
#include "column_radial_resolution.h"
#include "column_lateral.h"
#include "column_radial_lateral.h"
#include "column_lateral_resolution.h"
#include "column_sample.h"
#include "column_sample_radial.h"

namespace dsa {

namespace {

struct BlockBarrier {
    __device__ __forceinline__ void operator()() const { __syncthreads(); }
};

// block b is interior column (i, j) = (1 + b % nvx, 1 + b / nvx): column c = j * nx + i of the (nz, ny, nx) model, or -1 for a block past
// the interior
__device__ __forceinline__ long long block_column(int nx, int ny)
{
    const int nvx = nx - 2;
    const int bj = (int)blockIdx.x / nvx, bi = (int)blockIdx.x - bj * nvx;
    return bj >= ny - 2 ? -1 : (long long)(bj + 1) * nx + (bi + 1);
}

// what ColumnIn and RadialIn share, for column c: obs / wt: (K, ncol) fp32; pv: (K, ncol); the strides of S (M, K, ncol)
template <class In>
__device__ __forceinline__ void column_in(In& in, int M, int K, long long c, long long ncol, const float* obs, const float* wt, const double* pv)
{
    in.M = M; in.K = K;
    in.obs = obs + c; in.obs_stride = ncol;
    in.wt = wt ? wt + c : nullptr; in.wt_stride = ncol;
    in.pv = pv + c; in.pv_stride = ncol;
    in.s_lstride = (long long)K * ncol; in.s_kstride = ncol;
}

// dv: (M, ncol); nused / chi2 / flag: (ncol).  The ring's outputs are the caller's zeros.
__global__ void __launch_bounds__(64) k_column_step(int nx, int ny, int nz, int K, const float* __restrict__ obs, const float* __restrict__ wt,
                                                   const double* __restrict__ pv, const double* __restrict__ S, float smooth, float damp, float dvmax,
                                                   float minvel, float maxvel, float* __restrict__ vels, float* __restrict__ dv, int* __restrict__ nused,
                                                   double* __restrict__ chi2, int* __restrict__ flag)
{
    extern __shared__ double column_lds[];
    const int M = nz - 1;
    const long long ncol = (long long)nx * ny, c = block_column(nx, ny);
    if (c < 0) return;
    ColumnIn in;
    column_in(in, M, K, c, ncol, obs, wt, pv);
    in.S = S + c;
    const ColumnWork w = column_work(column_lds, M, K);
    int n = 0;
    double x2 = 0.0;
    const int f = column_step(in, smooth, damp, dvmax, minvel, maxvel, w, vels + c, ncol, dv + c, ncol, &n, &x2, (int)threadIdx.x, 64, BlockBarrier());
    if (threadIdx.x == 0) { nused[c] = n; chi2[c] = x2; flag[c] = f; }
}

// k_column_resolution: column_resolution.h on every interior column, the launch shape and the column of a block as
// above.  The work arrays of the step and T lie in dynamic LDS: column_resolution_doubles(M, K) doubles -- 4.1 KB for the Taipei example
// (M = 8, K = 26), 77.2 KB at the stage's limits (M = 63, K = 60: two columns per CU), which the launcher has to ask for.  depz: the nz
// depths of the model; measures: (4, M, ncol); leverage: (K, ncol); trace / nused / flag: (ncol); R: null or (M, M, ncol).
__global__ void __launch_bounds__(64) k_column_resolution(int nx, int ny, int nz, int K, const float* __restrict__ obs, const float* __restrict__ wt,
                                                         const double* __restrict__ pv, const double* __restrict__ S, const float* __restrict__ depz,
                                                         float smooth, float damp, double* __restrict__ measures, double* __restrict__ leverage,
                                                         double* __restrict__ trace, double* __restrict__ R, int* __restrict__ nused, int* __restrict__ flag)
{
    extern __shared__ double column_lds[];
    const int M = nz - 1;
    const long long ncol = (long long)nx * ny, c = block_column(nx, ny);
    if (c < 0) return;
    ColumnIn in;
    column_in(in, M, K, c, ncol, obs, wt, pv);
    in.S = S + c;
    ColumnResOut out;
    out.measures = measures + c; out.m_qstride = (long long)M * ncol; out.m_jstride = ncol;
    out.leverage = leverage + c; out.h_stride = ncol;
    out.R = R ? R + c : nullptr; out.r_stride = ncol;
    const ColumnWork w = column_work(column_lds, M, K);
    int n = 0;
    double tr = 0.0;
    const int f = column_resolution(in, depz, smooth, damp, w, column_resolution_t(column_lds, M, K), out, &tr, &n, (int)threadIdx.x, 64, BlockBarrier());
    if (threadIdx.x == 0) { nused[c] = n; trace[c] = tr; flag[c] = f; }
}

// k_column_azimuthal: column_azimuthal.h on every interior column, the launch shape and the column of a block as
// above.  The work arrays of the resolution, the two right-hand sides and the two rho vectors lie in dynamic LDS:
// column_azimuthal_doubles(M, K) doubles -- 4.6 KB for the Taipei example (M = 8, K = 26), 81 048 B at the stage's limits (M = 63, K = 60),
// which the launcher has to ask for.  wt: the effective weights, 0 at a Love slot; Z: (M, K, ncol), launch_sen_azimuthal's; a1 / a2: (K, ncol)
// fp32; g: (2, M, ncol), gc then gs; measures: (4, M, ncol); leverage: (K, ncol); chi2: (4, ncol); nused / flag: (ncol).
__global__ void __launch_bounds__(64) k_column_azimuthal(int nx, int ny, int nz, int K, const float* __restrict__ obs, const float* __restrict__ wt,
                                                        const double* __restrict__ pv, const double* __restrict__ Z, const float* __restrict__ a1,
                                                        const float* __restrict__ a2, const float* __restrict__ depz, float smooth, float damp,
                                                        double* __restrict__ g, double* __restrict__ measures, double* __restrict__ leverage,
                                                        double* __restrict__ chi2, int* __restrict__ nused, int* __restrict__ flag)
{
    extern __shared__ double column_lds[];
    const int M = nz - 1;
    const long long ncol = (long long)nx * ny, c = block_column(nx, ny);
    if (c < 0) return;
    ColumnAziIn in;
    column_in(in.col, M, K, c, ncol, obs, wt, pv);
    in.col.S = Z + c;
    in.a1 = a1 + c; in.a2 = a2 + c; in.a_stride = ncol;
    ColumnAziOut out;
    out.g = g + c; out.g_qstride = (long long)M * ncol; out.g_lstride = ncol;
    out.chi2 = chi2 + c; out.chi2_stride = ncol;
    out.res.measures = measures + c; out.res.m_qstride = (long long)M * ncol; out.res.m_jstride = ncol;
    out.res.leverage = leverage + c; out.res.h_stride = ncol;
    out.res.R = nullptr; out.res.r_stride = 0;
    int n = 0;
    const int f = column_azimuthal(in, depz, smooth, damp, column_azimuthal_work(column_lds, M, K), out, &n, (int)threadIdx.x, 64, BlockBarrier());
    if (threadIdx.x == 0) { nused[c] = n; flag[c] = f; }
}

// k_column_step_radial: column_radial.h on every interior column of the two resident models, the launch shape and the
// column of a block as above.  The work arrays lie in dynamic LDS: radial_work_doubles(M, K) doubles -- 5.1 KB for K = 26 on M = 8, 98 232 B
// at the stage's limits (M = 63, K = 60: one column per CU), which the launcher has to ask for.  love: bit k set where slot k is a Love slot.
// Sv / Sh: (M, K, ncol), k_sen_combine's rule on the Vsv and on the Vsh model; dv: (2, M, ncol), the Vsv block then the Vsh block; nused /
// chi2: (2, ncol), Rayleigh then Love; flag: (ncol).
__global__ void __launch_bounds__(64) k_column_step_radial(int nx, int ny, int nz, int K, unsigned long long love, const float* __restrict__ obs,
                                                          const float* __restrict__ wt, const double* __restrict__ pv, const double* __restrict__ Sv,
                                                          const double* __restrict__ Sh, float smooth, float damp, float aniso, float dvmax, float minvel,
                                                          float maxvel, float* __restrict__ vsv, float* __restrict__ vsh, float* __restrict__ dv,
                                                          int* __restrict__ nused, double* __restrict__ chi2, int* __restrict__ flag)
{
    extern __shared__ double column_lds[];
    const int M = nz - 1;
    const long long ncol = (long long)nx * ny, c = block_column(nx, ny);
    if (c < 0) return;
    RadialIn in;
    column_in(in, M, K, c, ncol, obs, wt, pv);
    in.love = love; in.Sv = Sv + c; in.Sh = Sh + c;
    const ColumnWork w = radial_work(column_lds, M, K);
    int n[2] = { 0, 0 };
    double x2[2] = { 0.0, 0.0 };
    const int f = radial_step(in, smooth, damp, aniso, dvmax, minvel, maxvel, w, vsv + c, vsh + c, ncol, dv + c, dv + (long long)M * ncol + c, ncol, n, x2,
                              (int)threadIdx.x, 64, BlockBarrier());
    if (threadIdx.x == 0) { nused[c] = n[0]; nused[ncol + c] = n[1]; chi2[c] = x2[0]; chi2[ncol + c] = x2[1]; flag[c] = f; }
}

// k_column_resolution_radial: column_radial_resolution.h on every interior column of the two resident models, one
// block of two wavefronts per column (the header's nlanes: 2M reaches 126, one lane per unknown in the reductions; the K solves run on the
// first K lanes).  The work arrays of the radial step and T (2M x K) lie in dynamic LDS and nowhere else: 6.7 KB for K = 26 on M = 8,
// 158 712 B at the stage's limits (M = 63, K = 60) of the 163 840 B a workgroup may have, which the launcher has to ask for.
// measures: (6, 2M, ncol); pair: (2, M, ncol); leverage: (K, ncol); trace / nused: (2, ncol); flag: (ncol); R: null or (2M, 2M, ncol).
#ifndef DSA_RADIAL_RESOLUTION_LANES
#define DSA_RADIAL_RESOLUTION_LANES 128          // 64 or 128: both were timed (section 26)
#endif
constexpr int kRadialResolutionLanes = DSA_RADIAL_RESOLUTION_LANES;

__global__ void __launch_bounds__(kRadialResolutionLanes)
k_column_resolution_radial(int nx, int ny, int nz, int K, unsigned long long love, const float* __restrict__ obs, const float* __restrict__ wt,
                           const double* __restrict__ pv, const double* __restrict__ Sv, const double* __restrict__ Sh, const float* __restrict__ depz,
                           const float* __restrict__ vsv, const float* __restrict__ vsh, float smooth, float damp, float aniso, double* __restrict__ measures,
                           double* __restrict__ pair, double* __restrict__ leverage, double* __restrict__ trace, double* __restrict__ R, int* __restrict__ nused,
                           int* __restrict__ flag)
{
    extern __shared__ double column_lds[];
    const int M = nz - 1;
    const long long ncol = (long long)nx * ny, c = block_column(nx, ny);
    if (c < 0) return;
    RadialIn in;
    column_in(in, M, K, c, ncol, obs, wt, pv);
    in.love = love; in.Sv = Sv + c; in.Sh = Sh + c;
    RadialResOut out;
    out.measures = measures + c; out.m_qstride = 2ll * M * ncol; out.m_jstride = ncol;
    out.pair = pair + c; out.p_qstride = (long long)M * ncol; out.p_lstride = ncol;
    out.leverage = leverage + c; out.h_stride = ncol;
    out.R = R ? R + c : nullptr; out.r_stride = ncol;
    const ColumnWork w = radial_work(column_lds, M, K);
    int n[2] = { 0, 0 };
    double tr[2] = { 0.0, 0.0 };
    const int f = radial_resolution(in, depz, smooth, damp, aniso, vsv + c, vsh + c, ncol, w, radial_resolution_t(column_lds, M, K), out, tr, n, (int)threadIdx.x,
                                    (int)blockDim.x, BlockBarrier());
    if (threadIdx.x == 0) { nused[c] = n[0]; nused[ncol + c] = n[1]; trace[c] = tr[0]; trace[ncol + c] = tr[1]; flag[c] = f; }
}

// The laterally coupled steps (DESIGN.md sections 24 and 25): column_lateral.h's conjugate gradients on every interior column, the launch
// shape as above -- block b is interior column b of the header.  A system is passed to its kernels by value: LateralWs (section 24), or
// RadialLateralWs (section 25: 2M unknowns per column) -- views of lateral_ws_doubles doubles in global memory, where N, the factor, the
// vectors, the columns' dot products, the scalars and the done flag lie between the launches.  No kernel waits for another block: what a
// column needs of its neighbours was written by an earlier launch.
// k_lateral_setup: assemble and factor in LDS (k_column_step's arrays), N, the factor and b to the workspace; nused / chi2 / flag: (ncol).
__global__ void __launch_bounds__(64) k_lateral_setup(int nx, int ny, int nz, int K, const float* __restrict__ obs, const float* __restrict__ wt,
                                                     const double* __restrict__ pv, const double* __restrict__ S, float smooth, float damp, LateralWs ws,
                                                     int* __restrict__ nused, double* __restrict__ chi2, int* __restrict__ flag)
{
    extern __shared__ double column_lds[];
    const int M = nz - 1;
    const long long ncol = (long long)nx * ny, c = block_column(nx, ny);
    if (c < 0) return;
    ColumnIn in;
    column_in(in, M, K, c, ncol, obs, wt, pv);
    in.S = S + c;
    int n = 0;
    double x2 = 0.0;
    const int f = lateral_setup(in, smooth, damp, column_work(column_lds, M, K), ws, (int)blockIdx.x, &n, &x2, (int)threadIdx.x, 64, BlockBarrier());
    if (threadIdx.x == 0) { nused[c] = n; chi2[c] = x2; flag[c] = f; }
}

// k_radial_lateral_setup: radial_assemble and the factorisation in LDS (k_column_step_radial's arrays and sizes), N, the factor and b to the
// workspace; Sv / Sh, love, nused / chi2 (2, ncol), flag (ncol) as k_column_step_radial's.
__global__ void __launch_bounds__(64) k_radial_lateral_setup(int nx, int ny, int nz, int K, unsigned long long love, const float* __restrict__ obs,
                                                            const float* __restrict__ wt, const double* __restrict__ pv, const double* __restrict__ Sv,
                                                            const double* __restrict__ Sh, float smooth, float damp, float aniso, const float* __restrict__ vsv,
                                                            const float* __restrict__ vsh, RadialLateralWs rl, int* __restrict__ nused,
                                                            double* __restrict__ chi2, int* __restrict__ flag)
{
    extern __shared__ double column_lds[];
    const int M = nz - 1;
    const long long ncol = (long long)nx * ny, c = block_column(nx, ny);
    if (c < 0) return;
    RadialIn in;
    column_in(in, M, K, c, ncol, obs, wt, pv);
    in.love = love; in.Sv = Sv + c; in.Sh = Sh + c;
    int n[2] = { 0, 0 };
    double x2[2] = { 0.0, 0.0 };
    const int f = radial_lateral_setup(in, smooth, damp, aniso, vsv + c, vsh + c, ncol, radial_work(column_lds, M, K), rl, (int)blockIdx.x, n, x2, (int)threadIdx.x,
                                       64, BlockBarrier());
    if (threadIdx.x == 0) { nused[c] = n[0]; nused[ncol + c] = n[1]; chi2[c] = x2[0]; chi2[ncol + c] = x2[1]; flag[c] = f; }
}

__device__ __forceinline__ bool past_interior(const LateralWs& ws) { return (int)blockIdx.x >= ws.nvx * ws.nvy; }
__device__ __forceinline__ long long model_columns(const LateralWs& ws) { return (long long)(ws.nvx + 2) * (ws.nvy + 2); }

// the right-hand side with the edges' part, x0 and the columns' figures of rz0: each system's own
__global__ void __launch_bounds__(64) k_lateral_start(LateralWs ws, const float* __restrict__ vels)
{
    if (past_interior(ws)) return;
    lateral_start(ws, (int)blockIdx.x, vels, model_columns(ws), (int)threadIdx.x, 64, BlockBarrier());
}

__global__ void __launch_bounds__(64) k_radial_lateral_start(RadialLateralWs rl, const float* __restrict__ vsv, const float* __restrict__ vsh)
{
    if (past_interior(rl.ws)) return;
    radial_lateral_start(rl, (int)blockIdx.x, vsv, vsh, model_columns(rl.ws), (int)threadIdx.x, 64, BlockBarrier());
}

// r0, z0 and the columns' figures of the first rz, with the system's operator
template <class Sys>
__global__ void __launch_bounds__(64) k_lateral_residual(Sys sys)
{
    if (past_interior(lateral_view(sys))) return;
    lateral_residual(sys, (int)blockIdx.x, (int)threadIdx.x, 64, BlockBarrier());
}

// the two kernels of an iteration: the new direction and q = A p, with the system's operator; the update of x and r, z = M^-1 r, the same
// for every system.  Both return at once when done is set.
template <class Sys>
__global__ void __launch_bounds__(64) k_lateral_direction(Sys sys)
{
    if (past_interior(lateral_view(sys))) return;
    lateral_direction(sys, (int)blockIdx.x, (int)threadIdx.x, 64, BlockBarrier());
}

__global__ void __launch_bounds__(64) k_lateral_update(LateralWs ws)
{
    if (past_interior(ws)) return;
    lateral_update(ws, (int)blockIdx.x, (int)threadIdx.x, 64, BlockBarrier());
}

// the global sums, one wavefront: lane t is chain t; lane 0 adds the chains and sets the scalars
__global__ void __launch_bounds__(64) k_lateral_reduce(LateralWs ws, int what, double tol, int maxit)
{
    __shared__ double chains[kLateralChains];
    lateral_reduce(ws, what, tol, maxit, chains, (int)threadIdx.x, 64, BlockBarrier());
}

// the clipped steps and the stepped model(s): one block of ws.M rows of vels0 and dv (M, ncol), or two of Mb = ws.M / 2 rows, vels0's and
// vels1's, dv (2, Mb, ncol)
__global__ void __launch_bounds__(64) k_lateral_finish(LateralWs ws, int Mb, float dvmax, float minvel, float maxvel, float* __restrict__ vels0,
                                                      float* __restrict__ vels1, float* __restrict__ dv)
{
    if (past_interior(ws)) return;
    const long long ncol = model_columns(ws);
    lateral_finish_blocks(ws, (int)blockIdx.x, Mb, dvmax, minvel, maxvel, vels0, vels1, ncol, dv, dv + (long long)Mb * ncol, ncol, (int)threadIdx.x, 64);
}

// The resolution of the laterally coupled step: column_lateral_resolution.h's batch of members.  Block (b, g) is one
// wavefront: interior column b, the 64 members of lane group g, lane = member.  N_b, the factor and d_b (or H_b) are staged in LDS and read as
// broadcasts; every lane runs its member's chains on its own operand vectors in LDS (element l of lane t at l * 64 + t: consecutive doubles
// across the lanes, every bank once); the member vectors in global memory are member-fastest, so a wavefront's loads and stores of one
// element are 512 contiguous bytes.  latres_work_doubles(M) doubles of dynamic LDS: 8.8 KB at M = 8, 97 272 B at M = 63, which the launcher
// has to ask for.  No kernel waits for another block: what a column needs of its neighbours was written by an earlier launch.
// k_latres_gram: H_b = G_b^T G_b of every active column, after k_lateral_setup, in k_column_step's work arrays.
__global__ void __launch_bounds__(64) k_latres_gram(int nx, int ny, int nz, int K, const float* __restrict__ obs, const float* __restrict__ wt,
                                                   const double* __restrict__ pv, const double* __restrict__ S, LateralWs ws, double* __restrict__ H)
{
    extern __shared__ double column_lds[];
    const int M = nz - 1;
    const long long ncol = (long long)nx * ny, c = block_column(nx, ny);
    if (c < 0) return;
    ColumnIn in;
    column_in(in, M, K, c, ncol, obs, wt, pv);
    in.S = S + c;
    latres_gram(in, column_work(column_lds, M, K), ws, (int)blockIdx.x, H, (int)threadIdx.x, 64, BlockBarrier());
}

__device__ __forceinline__ bool latres_past(const LatResBatch& B)
{
    return (int)blockIdx.x >= B.ws.nvx * B.ws.nvy || ((int)blockIdx.y + 1) * kLatResGroup > B.Sc;
}

// phase: 0 the right-hand sides, 1 x0 and the figures of rz0, 2 r0, z0 and the figures of the first rz, 3 and 4 the two halves of an
// iteration, 5 u and the figures of the measures
template <int Phase>
__global__ void __launch_bounds__(64) k_latres_phase(LatResBatch B)
{
    extern __shared__ double column_lds[];
    if (latres_past(B)) return;
    const LatResWork w = latres_work(column_lds, B.ws.M);
    const int b = (int)blockIdx.x, g = (int)blockIdx.y, lane = (int)threadIdx.x;
    if (Phase == 0) latres_form(B, b, g, w, lane, 64, BlockBarrier());
    else if (Phase == 1) latres_start(B, b, g, w, lane, 64, BlockBarrier());
    else if (Phase == 2) latres_residual(B, b, g, w, lane, 64, BlockBarrier());
    else if (Phase == 3) latres_direction(B, b, g, w, lane, 64, BlockBarrier());
    else if (Phase == 4) latres_update(B, b, g, w, lane, 64, BlockBarrier());
    else latres_measure(B, b, g, w, lane, 64, BlockBarrier());
}

// the global sums and the scalars, one lane per member over coalesced reads of the columns' figures
__global__ void __launch_bounds__(64) k_latres_reduce(LatResBatch B, int what, double tol, int maxit)
{
    if (((int)blockIdx.x + 1) * kLatResGroup > B.Sc) return;
    latres_reduce(B, (int)blockIdx.x, what, tol, maxit, (int)threadIdx.x, 64);
}

__global__ void __launch_bounds__(64) k_latres_measures(LatResBatch B, double* __restrict__ measures)
{
    if (((int)blockIdx.x + 1) * kLatResGroup > B.Sc) return;
    latres_measures(B, (int)blockIdx.x, measures, (int)threadIdx.x, 64);
}

// The Monte-Carlo depth inversion: column_sample.h on every (column, chain) of a sample stage, thread t = chain *
// ncol + column -- the column is the fastest index of the model store (depth, chain, column) and of the map store (chain, map, column), so
// a wavefront's loads and stores of one depth or one map are consecutive.  The view is passed by value.  No thread reads what another one
// writes in the same launch: the used mask, the flag and chain 0's figures a chain needs were written by an earlier launch or are computed
// again by the chain itself.  No LDS, no atomics.
constexpr int kSampleBlock = 256;

__device__ __forceinline__ bool sample_thread(const SampleView& S, long long* c, int* q)
{
    const long long t = (long long)blockIdx.x * kSampleBlock + threadIdx.x;
    if (t >= S.ncol * S.C) return false;
    *q = (int)(t / S.ncol);
    *c = t - (long long)*q * S.ncol;
    return true;
}

// phase 0: the chains' start models and the cleared state, before the set-up's dispersion runs; phase 1: the used mask, phi, psi and the
// chains put back, after them
__global__ void __launch_bounds__(kSampleBlock) k_sample_setup(SampleView S, int phase)
{
    long long c; int q;
    if (!sample_thread(S, &c, &q)) return;
    if (phase == 0) sample_setup_models(S, c, q);
    else sample_setup_state(S, c, q);
}

__global__ void __launch_bounds__(kSampleBlock) k_sample_propose(SampleView S, int sweep)
{
    long long c; int q;
    if (!sample_thread(S, &c, &q)) return;
    sample_propose(S, c, q, sweep);
}

__global__ void __launch_bounds__(kSampleBlock) k_sample_accept(SampleView S, int sweep)
{
    long long c; int q;
    if (!sample_thread(S, &c, &q)) return;
    sample_accept(S, c, q, sweep);
}

// The block sweeps: the two kernels above with a SampleBlockView beside the view, launched in place of them in a
// block sweep and in no other, so that the kernels above stay what they were.  A chain of a column whose shape is flagged takes the
// single-node path inside them.  The block proposal keeps its M steps in a thread's own array (63 doubles: 512 bytes of scratch); all chains of a
// column read the same L and r.
__global__ void __launch_bounds__(kSampleBlock) k_sample_propose_block(SampleView S, SampleBlockView B, int sweep)
{
    long long c; int q;
    if (!sample_thread(S, &c, &q)) return;
    sample_propose_block(S, B, c, q, sweep);
}

__global__ void __launch_bounds__(kSampleBlock) k_sample_accept_block(SampleView S, SampleBlockView B, int sweep)
{
    long long c; int q;
    if (!sample_thread(S, &c, &q)) return;
    sample_accept_block(S, B, c, q, sweep);
}

// k_sample_shape: the shape of every interior column for the block proposals, k_column_step's launch shape and LDS work arrays: assemble
// and factor, then the packed triangle (T, ncol), r (M, ncol) and the flag (ncol) to global memory, column fastest.  The model is not
// touched.  The ring's and a flagged column's tri and r are the caller's zeros.
__global__ void __launch_bounds__(64) k_sample_shape(int nx, int ny, int nz, int K, const float* __restrict__ obs, const float* __restrict__ wt,
                                                    const double* __restrict__ pv, const double* __restrict__ S, float smooth, float damp,
                                                    double* __restrict__ tri, double* __restrict__ r, int* __restrict__ nused, int* __restrict__ flag)
{
    extern __shared__ double column_lds[];
    const int M = nz - 1;
    const long long ncol = (long long)nx * ny, c = block_column(nx, ny);
    if (c < 0) return;
    ColumnIn in;
    column_in(in, M, K, c, ncol, obs, wt, pv);
    in.S = S + c;
    int n = 0;
    const int f = sample_shape(in, smooth, damp, column_work(column_lds, M, K), tri + c, r + c, ncol, &n, (int)threadIdx.x, 64, BlockBarrier());
    if (threadIdx.x == 0) { nused[c] = n; flag[c] = f; }
}

// one thread per (column, depth): t = depth * ncol + column.  nodes (5, M, ncol), cols (3, ncol), counts (8, ncol)
__global__ void __launch_bounds__(kSampleBlock) k_sample_finish(SampleView S, double* __restrict__ nodes, double* __restrict__ cols, int* __restrict__ counts)
{
    const long long t = (long long)blockIdx.x * kSampleBlock + threadIdx.x;
    if (t >= S.ncol * (S.nz - 1)) return;
    const int l = (int)(t / S.ncol);
    sample_finish(S, t - (long long)l * S.ncol, l, nodes, cols, counts);
}

// The Monte-Carlo radial depth inversion: column_sample_radial.h on every (column, chain) of a radial sample stage,
// k_sample_*'s mapping (thread t = chain * ncol + column, the column fastest in both model stores and in the map store) and rules: the view
// by value, no thread reads what another writes in the same launch, no LDS, no atomics.
__device__ __forceinline__ bool sample_radial_thread(const SampleRadialView& S, long long* c, int* q)
{
    const long long t = (long long)blockIdx.x * kSampleBlock + threadIdx.x;
    if (t >= S.ncol * S.C) return false;
    *q = (int)(t / S.ncol);
    *c = t - (long long)*q * S.ncol;
    return true;
}

// phase 0: both stores of every chain and the cleared state, before the set-up's dispersion runs; phase 1: the used mask, phi, psi and the
// chains put back, after them
__global__ void __launch_bounds__(kSampleBlock) k_sample_radial_setup(SampleRadialView S, int phase)
{
    long long c; int q;
    if (!sample_radial_thread(S, &c, &q)) return;
    if (phase == 0) sample_radial_setup_models(S, c, q);
    else sample_radial_setup_state(S, c, q);
}

__global__ void __launch_bounds__(kSampleBlock) k_sample_radial_propose(SampleRadialView S, int sweep)
{
    long long c; int q;
    if (!sample_radial_thread(S, &c, &q)) return;
    sample_radial_propose(S, c, q, sweep);
}

__global__ void __launch_bounds__(kSampleBlock) k_sample_radial_accept(SampleRadialView S, int sweep)
{
    long long c; int q;
    if (!sample_radial_thread(S, &c, &q)) return;
    sample_radial_accept(S, c, q, sweep);
}

// one thread per (column, depth): t = depth * ncol + column.  nodes (16, M, ncol), cols (3, ncol), counts (15, ncol)
__global__ void __launch_bounds__(kSampleBlock) k_sample_radial_finish(SampleRadialView S, double* __restrict__ nodes, double* __restrict__ cols,
                                                                       int* __restrict__ counts)
{
    const long long t = (long long)blockIdx.x * kSampleBlock + threadIdx.x;
    if (t >= S.ncol * (S.nz - 1)) return;
    const int l = (int)(t / S.ncol);
    sample_radial_finish(S, t - (long long)l * S.ncol, l, nodes, cols, counts);
}

// The posterior marginals, launched after the Metropolis test of a kept sweep while they are switched on.  Thread t =
// (row * C + chain) * ncol + column, row a depth (k_sample_hist) or a packed triangle entry (k_sample_cov): the column is the fastest
// index, so a wavefront's reads of v and v0 and its read-modify-write of P are consecutive; the counters of one depth and chain lie nbins
// planes apart and a wavefront touches as many of them as its values have bins.  Every counter and every sum has one thread: no atomics,
// no LDS.
__device__ __forceinline__ bool marginal_thread(const SampleView& S, int rows, long long* c, int* q, int* row)
{
    const long long t = (long long)blockIdx.x * kSampleBlock + threadIdx.x, cc = S.ncol * S.C;
    if (t >= cc * rows) return false;
    *row = (int)(t / cc);
    const long long r = t - (long long)*row * cc;
    *q = (int)(r / S.ncol);
    *c = r - (long long)*q * S.ncol;
    return true;
}

__global__ void __launch_bounds__(kSampleBlock) k_sample_hist(SampleView S, SampleMarginalView G, int sweep)
{
    long long c; int q, l;
    if (!marginal_thread(S, S.nz - 1, &c, &q, &l)) return;
    sample_marginal_hist(S, G, c, q, l, sweep);
}

__global__ void __launch_bounds__(kSampleBlock) k_sample_cov(SampleView S, SampleMarginalView G, int sweep)
{
    long long c; int q, e;
    if (!marginal_thread(S, column_tri_size(S.nz - 1), &c, &q, &e)) return;
    sample_marginal_cov(S, G, c, q, e, sweep);
}

// one thread per (column, row): t = row * ncol + column, rows = M (or the triangle's size where cov is asked for).  A row below M is a
// depth: its pooled counts (nbins, M, ncol), mode and quantiles (1 + nlevels, M, ncol); every row is a triangle entry of cov (tri, ncol)
__global__ void __launch_bounds__(kSampleBlock) k_sample_marginal_finish(SampleView S, SampleMarginalView G, SampleLevels lv, int rows, unsigned* __restrict__ pooled,
                                                                         double* __restrict__ figures, double* __restrict__ cov)
{
    const long long t = (long long)blockIdx.x * kSampleBlock + threadIdx.x;
    if (t >= S.ncol * rows) return;
    const int row = (int)(t / S.ncol);
    const long long c = t - (long long)row * S.ncol;
    if (row < S.nz - 1) sample_marginal_finish(S, G, c, row, lv.n, lv.p, pooled, figures);
    if (cov) sample_marginal_cov_finish(S, G, c, row, cov);
}

}  // namespace

void launch_column_step(int nx, int ny, int nz, int K, const float* d_obs, const float* d_wt, const double* d_pv, const double* d_S, float smooth, float damp,
                        float dvmax, float minvel, float maxvel, float* d_vels, float* d_dv, int* d_nused, double* d_chi2, int* d_flag, hipStream_t stream)
{
    if (nx < 3 || ny < 3 || nz < 2 || K < 1) return;
    const size_t lds = column_work_doubles(nz - 1, K) * sizeof(double);
    hipLaunchKernelGGL(k_column_step, dim3((unsigned)((nx - 2) * (ny - 2))), dim3(64), lds, stream, nx, ny, nz, K, d_obs, d_wt, d_pv, d_S, smooth, damp, dvmax,
                       minvel, maxvel, d_vels, d_dv, d_nused, d_chi2, d_flag);
}

// The dynamic-LDS rule of a kernel whose work arrays may pass the 64 KB a block gets without asking (the attribute is per device: set every
// time).  0: launch; 1: the case needs more than a block of this device may have (*limit_out); 2: the device refused the attribute
static int column_lds_opt_in(int device, const void* kernel, size_t lds, int* limit_out)
{
    if (lds <= 64 * 1024) return 0;
    int limit = 0;
    if (hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess) limit = 0;
    if (limit_out) *limit_out = limit;
    if (lds > (size_t)limit) return 1;
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        (void)hipGetLastError();
        return 2;
    }
    return 0;
}

size_t column_resolution_lds_bytes(int nz, int K) { return column_resolution_doubles(nz - 1, K) * sizeof(double); }

// column_lds_opt_in's return values: nothing is launched unless 0
int launch_column_resolution(int device, int nx, int ny, int nz, int K, const float* d_obs, const float* d_wt, const double* d_pv, const double* d_S,
                             const float* d_depz, float smooth, float damp, double* d_measures, double* d_leverage, double* d_trace, double* d_R, int* d_nused,
                             int* d_flag, hipStream_t stream, int* limit_out)
{
    if (nx < 3 || ny < 3 || nz < 2 || K < 1) return 0;
    const size_t lds = column_resolution_lds_bytes(nz, K);
    if (int rc = column_lds_opt_in(device, reinterpret_cast<const void*>(&k_column_resolution), lds, limit_out)) return rc;
    hipLaunchKernelGGL(k_column_resolution, dim3((unsigned)((nx - 2) * (ny - 2))), dim3(64), lds, stream, nx, ny, nz, K, d_obs, d_wt, d_pv, d_S, d_depz, smooth,
                       damp, d_measures, d_leverage, d_trace, d_R, d_nused, d_flag);
    return 0;
}

size_t column_azimuthal_lds_bytes(int nz, int K) { return column_azimuthal_doubles(nz - 1, K) * sizeof(double); }

// column_lds_opt_in's return values: nothing is launched unless 0
int launch_column_azimuthal(int device, int nx, int ny, int nz, int K, const float* d_obs, const float* d_wt, const double* d_pv, const double* d_Z,
                            const float* d_a1, const float* d_a2, const float* d_depz, float smooth, float damp, double* d_g, double* d_measures,
                            double* d_leverage, double* d_chi2, int* d_nused, int* d_flag, hipStream_t stream, int* limit_out)
{
    if (nx < 3 || ny < 3 || nz < 2 || K < 1) return 0;
    const size_t lds = column_azimuthal_lds_bytes(nz, K);
    if (int rc = column_lds_opt_in(device, reinterpret_cast<const void*>(&k_column_azimuthal), lds, limit_out)) return rc;
    hipLaunchKernelGGL(k_column_azimuthal, dim3((unsigned)((nx - 2) * (ny - 2))), dim3(64), lds, stream, nx, ny, nz, K, d_obs, d_wt, d_pv, d_Z, d_a1, d_a2, d_depz,
                       smooth, damp, d_g, d_measures, d_leverage, d_chi2, d_nused, d_flag);
    return 0;
}

size_t column_radial_lds_bytes(int nz, int K) { return radial_work_doubles(nz - 1, K) * sizeof(double); }

int launch_column_step_radial(int device, int nx, int ny, int nz, int K, unsigned long long love, const float* d_obs, const float* d_wt, const double* d_pv,
                              const double* d_Sv, const double* d_Sh, float smooth, float damp, float aniso, float dvmax, float minvel, float maxvel, float* d_vsv,
                              float* d_vsh, float* d_dv, int* d_nused, double* d_chi2, int* d_flag, hipStream_t stream, int* limit_out)
{
    if (nx < 3 || ny < 3 || nz < 2 || K < 1) return 0;
    const size_t lds = column_radial_lds_bytes(nz, K);
    if (int rc = column_lds_opt_in(device, reinterpret_cast<const void*>(&k_column_step_radial), lds, limit_out)) return rc;
    hipLaunchKernelGGL(k_column_step_radial, dim3((unsigned)((nx - 2) * (ny - 2))), dim3(64), lds, stream, nx, ny, nz, K, love, d_obs, d_wt, d_pv, d_Sv, d_Sh,
                       smooth, damp, aniso, dvmax, minvel, maxvel, d_vsv, d_vsh, d_dv, d_nused, d_chi2, d_flag);
    return 0;
}

size_t column_radial_resolution_lds_bytes(int nz, int K) { return radial_resolution_doubles(nz - 1, K) * sizeof(double); }

// column_lds_opt_in's return values: nothing is launched unless 0
int launch_column_resolution_radial(int device, int nx, int ny, int nz, int K, unsigned long long love, const float* d_obs, const float* d_wt, const double* d_pv,
                                    const double* d_Sv, const double* d_Sh, const float* d_depz, const float* d_vsv, const float* d_vsh, float smooth, float damp,
                                    float aniso, double* d_measures, double* d_pair, double* d_leverage, double* d_trace, double* d_R, int* d_nused, int* d_flag,
                                    hipStream_t stream, int* limit_out)
{
    if (nx < 3 || ny < 3 || nz < 2 || K < 1) return 0;
    const size_t lds = column_radial_resolution_lds_bytes(nz, K);
    if (int rc = column_lds_opt_in(device, reinterpret_cast<const void*>(&k_column_resolution_radial), lds, limit_out)) return rc;
    hipLaunchKernelGGL(k_column_resolution_radial, dim3((unsigned)((nx - 2) * (ny - 2))), dim3(kRadialResolutionLanes), lds, stream, nx, ny, nz, K, love, d_obs,
                       d_wt, d_pv, d_Sv, d_Sh, d_depz, d_vsv, d_vsh, smooth, damp, aniso, d_measures, d_pair, d_leverage, d_trace, d_R, d_nused, d_flag);
    return 0;
}

// ---- the coupled systems: the views of a CoupledSystem, the set-up of each, and one copy of the loop's launch sequences ----

static dim3 coupled_grid(const CoupledSystem& s) { return dim3((unsigned)((s.nx - 2) * (s.ny - 2))); }
static bool coupled_empty(const CoupledSystem& s) { return s.nx < 3 || s.ny < 3 || s.nz < 2; }
static LateralWs coupled_iso(const CoupledSystem& s) { return lateral_ws(s.d_ws, s.nx - 2, s.ny - 2, s.nz - 1, s.lateral); }
static RadialLateralWs coupled_radial(const CoupledSystem& s) { return radial_lateral_ws(s.d_ws, s.nx - 2, s.ny - 2, s.nz - 1, s.lateral, s.lateral_aniso); }
// what the kernels that are the same for every system run on
static LateralWs coupled_view(const CoupledSystem& s) { return s.blocks == 2 ? coupled_radial(s).ws : coupled_iso(s); }

size_t coupled_ws_bytes(int blocks, int nx, int ny, int nz) { return lateral_ws_doubles(nx - 2, ny - 2, blocks * (nz - 1)) * sizeof(double); }
bool coupled_edges(const CoupledSystem& s) { return coupled_view(s).edges != 0; }
const int* coupled_ints(const CoupledSystem& s) { return coupled_view(s).ic; }
const double* coupled_scalars(const CoupledSystem& s) { return coupled_view(s).sc; }

static void launch_reduce(const CoupledSystem& s, int what, double tol, int maxit, hipStream_t stream)
{
    hipLaunchKernelGGL(k_lateral_reduce, dim3(1), dim3(64), 0, stream, coupled_view(s), what, tol, maxit);
}

void launch_lateral_setup(const CoupledSystem& s, int K, const float* d_obs, const float* d_wt, const double* d_pv, const double* d_S, float smooth, float damp,
                          double tol, const float* d_vels, int* d_nused, double* d_chi2, int* d_flag, hipStream_t stream)
{
    if (coupled_empty(s) || K < 1) return;
    const size_t lds = column_work_doubles(s.nz - 1, K) * sizeof(double);
    hipLaunchKernelGGL(k_lateral_setup, coupled_grid(s), dim3(64), lds, stream, s.nx, s.ny, s.nz, K, d_obs, d_wt, d_pv, d_S, smooth, damp, coupled_iso(s), d_nused,
                       d_chi2, d_flag);
    hipLaunchKernelGGL(k_lateral_start, coupled_grid(s), dim3(64), 0, stream, coupled_iso(s), d_vels);
    launch_reduce(s, kLatSumRz0, tol, 0, stream);
}

// column_lds_opt_in's return values for the set-up kernel: nothing is launched unless 0
int launch_radial_lateral_setup(int device, const CoupledSystem& s, int K, unsigned long long love, const float* d_obs, const float* d_wt, const double* d_pv,
                                const double* d_Sv, const double* d_Sh, float smooth, float damp, float aniso, double tol, const float* d_vsv, const float* d_vsh,
                                int* d_nused, double* d_chi2, int* d_flag, hipStream_t stream, int* limit_out)
{
    if (coupled_empty(s) || K < 1) return 0;
    const size_t lds = column_radial_lds_bytes(s.nz, K);
    if (int rc = column_lds_opt_in(device, reinterpret_cast<const void*>(&k_radial_lateral_setup), lds, limit_out)) return rc;
    hipLaunchKernelGGL(k_radial_lateral_setup, coupled_grid(s), dim3(64), lds, stream, s.nx, s.ny, s.nz, K, love, d_obs, d_wt, d_pv, d_Sv, d_Sh, smooth, damp, aniso,
                       d_vsv, d_vsh, coupled_radial(s), d_nused, d_chi2, d_flag);
    hipLaunchKernelGGL(k_radial_lateral_start, coupled_grid(s), dim3(64), 0, stream, coupled_radial(s), d_vsv, d_vsh);
    launch_reduce(s, kLatSumRz0, tol, 0, stream);
    return 0;
}

template <class Sys>
static void coupled_first(const CoupledSystem& s, const Sys& sys, double tol, int maxit, hipStream_t stream)
{
    hipLaunchKernelGGL(k_lateral_residual<Sys>, coupled_grid(s), dim3(64), 0, stream, sys);
    launch_reduce(s, kLatSumFirst, tol, maxit, stream);
}

template <class Sys>
static void coupled_iteration(const CoupledSystem& s, const Sys& sys, double tol, int maxit, hipStream_t stream)
{
    hipLaunchKernelGGL(k_lateral_direction<Sys>, coupled_grid(s), dim3(64), 0, stream, sys);
    launch_reduce(s, kLatSumPq, tol, maxit, stream);
    hipLaunchKernelGGL(k_lateral_update, coupled_grid(s), dim3(64), 0, stream, coupled_view(s));
    launch_reduce(s, kLatSumRz, tol, maxit, stream);
}

void launch_coupled_first(const CoupledSystem& s, double tol, int maxit, hipStream_t stream)
{
    if (coupled_empty(s)) return;
    if (s.blocks == 2) coupled_first(s, coupled_radial(s), tol, maxit, stream);
    else coupled_first(s, coupled_iso(s), tol, maxit, stream);
}

void launch_coupled_iteration(const CoupledSystem& s, double tol, int maxit, hipStream_t stream)
{
    if (coupled_empty(s)) return;
    if (s.blocks == 2) coupled_iteration(s, coupled_radial(s), tol, maxit, stream);
    else coupled_iteration(s, coupled_iso(s), tol, maxit, stream);
}

void launch_coupled_finish(const CoupledSystem& s, float dvmax, float minvel, float maxvel, float* d_vels0, float* d_vels1, float* d_dv, hipStream_t stream)
{
    if (coupled_empty(s)) return;
    hipLaunchKernelGGL(k_lateral_finish, coupled_grid(s), dim3(64), 0, stream, coupled_view(s), s.nz - 1, dvmax, minvel, maxvel, d_vels0, d_vels1, d_dv);
}

// ---- the resolution of the laterally coupled step ----

size_t latres_lds_bytes(int nz) { return latres_work_doubles(nz - 1) * sizeof(double); }
size_t latres_gram_bytes(int nx, int ny, int nz) { return (size_t)(nx - 2) * (ny - 2) * column_tri_size(nz - 1) * sizeof(double); }
size_t latres_bytes_per_member(int nx, int ny, int nz) { return latres_member_bytes(nx - 2, ny - 2, nz - 1); }
size_t latres_chunk_bytes(int nx, int ny, int nz, int Sc) { return latres_batch_doubles(nx - 2, ny - 2, nz - 1, Sc) * sizeof(double); }

static LatResBatch latres_view(const LatResSystem& r)
{
    return latres_batch(coupled_iso(r.s), r.d_H, r.d_depz, r.d_models, r.d_batch, r.Sc);
}
static dim3 latres_grid(const LatResSystem& r) { return dim3((unsigned)((r.s.nx - 2) * (r.s.ny - 2)), (unsigned)(r.Sc / kLatResGroup)); }

int* latres_ints(const LatResSystem& r) { return latres_view(r).ic; }
int* latres_kinds(const LatResSystem& r) { return latres_view(r).kind; }
const double* latres_scalars(const LatResSystem& r) { return latres_view(r).sc; }
const double* latres_u(const LatResSystem& r) { return latres_view(r).q; }

// column_lds_opt_in's return values for the six kernels of a phase: nothing may be launched unless 0
int latres_prepare(int device, int nz, int* limit_out)
{
    const size_t lds = latres_lds_bytes(nz);
    const void* kernels[6] = { reinterpret_cast<const void*>(&k_latres_phase<0>), reinterpret_cast<const void*>(&k_latres_phase<1>),
                               reinterpret_cast<const void*>(&k_latres_phase<2>), reinterpret_cast<const void*>(&k_latres_phase<3>),
                               reinterpret_cast<const void*>(&k_latres_phase<4>), reinterpret_cast<const void*>(&k_latres_phase<5>) };
    for (const void* k : kernels)
        if (int rc = column_lds_opt_in(device, k, lds, limit_out)) return rc;
    return 0;
}

// section 24's set-up kernel as it is, then H
void launch_latres_setup(const CoupledSystem& s, int K, const float* d_obs, const float* d_wt, const double* d_pv, const double* d_S, float smooth, float damp,
                         double* d_H, int* d_nused, double* d_chi2, int* d_flag, hipStream_t stream)
{
    if (coupled_empty(s) || K < 1) return;
    const size_t lds = column_work_doubles(s.nz - 1, K) * sizeof(double);
    hipLaunchKernelGGL(k_lateral_setup, coupled_grid(s), dim3(64), lds, stream, s.nx, s.ny, s.nz, K, d_obs, d_wt, d_pv, d_S, smooth, damp, coupled_iso(s), d_nused,
                       d_chi2, d_flag);
    hipLaunchKernelGGL(k_latres_gram, coupled_grid(s), dim3(64), lds, stream, s.nx, s.ny, s.nz, K, d_obs, d_wt, d_pv, d_S, coupled_iso(s), d_H);
}

template <int Phase>
static void latres_phase(const LatResSystem& r, hipStream_t stream)
{
    hipLaunchKernelGGL(k_latres_phase<Phase>, latres_grid(r), dim3(64), latres_lds_bytes(r.s.nz), stream, latres_view(r));
}
static void latres_sums(const LatResSystem& r, int what, double tol, int maxit, hipStream_t stream)
{
    hipLaunchKernelGGL(k_latres_reduce, dim3((unsigned)(r.Sc / kLatResGroup)), dim3(64), 0, stream, latres_view(r), what, tol, maxit);
}

// the right-hand sides, x0, the first residual and the criterion at iteration 0 (five launches)
void launch_latres_first(const LatResSystem& r, double tol, int maxit, hipStream_t stream)
{
    if (coupled_empty(r.s)) return;
    latres_phase<0>(r, stream);
    latres_phase<1>(r, stream);
    latres_sums(r, kLatSumRz0, tol, maxit, stream);
    latres_phase<2>(r, stream);
    latres_sums(r, kLatSumFirst, tol, maxit, stream);
}

// one iteration of every member that is not done: four launches
void launch_latres_iteration(const LatResSystem& r, double tol, int maxit, hipStream_t stream)
{
    if (coupled_empty(r.s)) return;
    latres_phase<3>(r, stream);
    latres_sums(r, kLatSumPq, tol, maxit, stream);
    latres_phase<4>(r, stream);
    latres_sums(r, kLatSumRz, tol, maxit, stream);
}

// u and the measures (Sc, 7)
void launch_latres_measures(const LatResSystem& r, double* d_measures, hipStream_t stream)
{
    if (coupled_empty(r.s)) return;
    latres_phase<5>(r, stream);
    hipLaunchKernelGGL(k_latres_measures, dim3((unsigned)(r.Sc / kLatResGroup)), dim3(64), 0, stream, latres_view(r), d_measures);
}

// ---- the Monte-Carlo depth inversion ----

static dim3 sample_grid(long long n) { return dim3((unsigned)((n + kSampleBlock - 1) / kSampleBlock)); }
static bool sample_empty(const SampleView& S) { return S.ncol < 1 || S.C < 1 || S.nz < 2; }

void launch_sample_setup(const SampleView& S, int phase, hipStream_t stream)
{
    if (sample_empty(S)) return;
    hipLaunchKernelGGL(k_sample_setup, sample_grid(S.ncol * S.C), dim3(kSampleBlock), 0, stream, S, phase);
}

void launch_sample_propose(const SampleView& S, int sweep, hipStream_t stream)
{
    if (sample_empty(S)) return;
    hipLaunchKernelGGL(k_sample_propose, sample_grid(S.ncol * S.C), dim3(kSampleBlock), 0, stream, S, sweep);
}

void launch_sample_accept(const SampleView& S, int sweep, hipStream_t stream)
{
    if (sample_empty(S)) return;
    hipLaunchKernelGGL(k_sample_accept, sample_grid(S.ncol * S.C), dim3(kSampleBlock), 0, stream, S, sweep);
}

void launch_sample_propose_block(const SampleView& S, const SampleBlockView& B, int sweep, hipStream_t stream)
{
    if (sample_empty(S)) return;
    hipLaunchKernelGGL(k_sample_propose_block, sample_grid(S.ncol * S.C), dim3(kSampleBlock), 0, stream, S, B, sweep);
}

void launch_sample_accept_block(const SampleView& S, const SampleBlockView& B, int sweep, hipStream_t stream)
{
    if (sample_empty(S)) return;
    hipLaunchKernelGGL(k_sample_accept_block, sample_grid(S.ncol * S.C), dim3(kSampleBlock), 0, stream, S, B, sweep);
}

void launch_sample_shape(int nx, int ny, int nz, int K, const float* d_obs, const float* d_wt, const double* d_pv, const double* d_S, float smooth, float damp,
                         double* d_tri, double* d_r, int* d_nused, int* d_flag, hipStream_t stream)
{
    if (nx < 3 || ny < 3 || nz < 2 || K < 1) return;
    const size_t lds = column_work_doubles(nz - 1, K) * sizeof(double);
    hipLaunchKernelGGL(k_sample_shape, dim3((unsigned)((nx - 2) * (ny - 2))), dim3(64), lds, stream, nx, ny, nz, K, d_obs, d_wt, d_pv, d_S, smooth, damp, d_tri, d_r,
                       d_nused, d_flag);
}

void launch_sample_marginals(const SampleView& S, const SampleMarginalView& G, int sweep, hipStream_t stream)
{
    if (sample_empty(S) || sweep <= S.burn) return;
    const long long cc = S.ncol * S.C;
    hipLaunchKernelGGL(k_sample_hist, sample_grid(cc * (S.nz - 1)), dim3(kSampleBlock), 0, stream, S, G, sweep);
    if (G.P) hipLaunchKernelGGL(k_sample_cov, sample_grid(cc * column_tri_size(S.nz - 1)), dim3(kSampleBlock), 0, stream, S, G, sweep);
}

void launch_sample_marginal_finish(const SampleView& S, const SampleMarginalView& G, const SampleLevels& levels, unsigned* d_pooled, double* d_figures, double* d_cov,
                                   hipStream_t stream)
{
    if (sample_empty(S)) return;
    const int rows = d_cov ? column_tri_size(S.nz - 1) : S.nz - 1;
    hipLaunchKernelGGL(k_sample_marginal_finish, sample_grid(S.ncol * rows), dim3(kSampleBlock), 0, stream, S, G, levels, rows, d_pooled, d_figures, d_cov);
}

void launch_sample_finish(const SampleView& S, double* d_nodes, double* d_cols, int* d_counts, hipStream_t stream)
{
    if (sample_empty(S)) return;
    hipLaunchKernelGGL(k_sample_finish, sample_grid(S.ncol * (S.nz - 1)), dim3(kSampleBlock), 0, stream, S, d_nodes, d_cols, d_counts);
}

static bool sample_radial_empty(const SampleRadialView& S) { return S.ncol < 1 || S.C < 1 || S.nz < 2; }

void launch_sample_radial_setup(const SampleRadialView& S, int phase, hipStream_t stream)
{
    if (sample_radial_empty(S)) return;
    hipLaunchKernelGGL(k_sample_radial_setup, sample_grid(S.ncol * S.C), dim3(kSampleBlock), 0, stream, S, phase);
}

void launch_sample_radial_propose(const SampleRadialView& S, int sweep, hipStream_t stream)
{
    if (sample_radial_empty(S)) return;
    hipLaunchKernelGGL(k_sample_radial_propose, sample_grid(S.ncol * S.C), dim3(kSampleBlock), 0, stream, S, sweep);
}

void launch_sample_radial_accept(const SampleRadialView& S, int sweep, hipStream_t stream)
{
    if (sample_radial_empty(S)) return;
    hipLaunchKernelGGL(k_sample_radial_accept, sample_grid(S.ncol * S.C), dim3(kSampleBlock), 0, stream, S, sweep);
}

void launch_sample_radial_finish(const SampleRadialView& S, double* d_nodes, double* d_cols, int* d_counts, hipStream_t stream)
{
    if (sample_radial_empty(S)) return;
    hipLaunchKernelGGL(k_sample_radial_finish, sample_grid(S.ncol * (S.nz - 1)), dim3(kSampleBlock), 0, stream, S, d_nodes, d_cols, d_counts);
}

}  // namespace dsa
