// k_column_step: the depth step of every interior column of the resident model, one wavefront per column.  The
// arithmetic is column_system.h's, shared out over the 64 lanes; a block is one wavefront, so the barrier between the phases costs one
// instruction.  The work arrays lie in LDS, sized by the launch for the case's (M, K): K * M doubles of weighted sensitivities, the packed
// triangle of N (then L), and five short vectors -- 2.5 KB for the Taipei example (M = 8, K = 26: a CU's 160 KB hold more blocks than its
// wave slots), 49 KB at the stage's limits (M = 63, K = 60: three columns per CU, where the triangle alone is 16 KB).
// k_column_resolution, below it: the depth resolution of the same columns on the same factor, the same launch shape.
// k_column_step_radial: the step on two models, Vsv and Vsh, 2M unknowns per column, the same launch shape.
// k_lateral_* (DESIGN.md section 24): the laterally coupled step, a preconditioned conjugate-gradient loop of small launches of that shape.
// k_radial_lateral_* (DESIGN.md section 25), last: that loop on the radial step's 2M unknowns per column, with k_lateral_update and k_lateral_reduce as they are.
#include "kernels.h"
#include "column_system.h"
#include "column_resolution.h"
#include "column_radial.h"
#include "column_lateral.h"
#include "column_radial_lateral.h"

namespace dsa {

namespace {

struct BlockBarrier {
    __device__ __forceinline__ void operator()() const { __syncthreads(); }
};

// block b is interior column (i, j) = (1 + b % nvx, 1 + b / nvx), column c = j * nx + i of the (nz, ny, nx) model.  obs / wt: (K, ncol)
// fp32; pv: (K, ncol); S: (M, K, ncol); dv: (M, ncol); nused / chi2 / flag: (ncol).  The ring's outputs are the caller's zeros.
__global__ void __launch_bounds__(64) k_column_step(int nx, int ny, int nz, int K, const float* __restrict__ obs, const float* __restrict__ wt,
                                                   const double* __restrict__ pv, const double* __restrict__ S, float smooth, float damp, float dvmax,
                                                   float minvel, float maxvel, float* __restrict__ vels, float* __restrict__ dv, int* __restrict__ nused,
                                                   double* __restrict__ chi2, int* __restrict__ flag)
{
    extern __shared__ double column_lds[];
    const int nvx = nx - 2, M = nz - 1;
    const long long ncol = (long long)nx * ny;
    const int bj = (int)blockIdx.x / nvx, bi = (int)blockIdx.x - bj * nvx;
    if (bj >= ny - 2) return;
    const long long c = (long long)(bj + 1) * nx + (bi + 1);
    ColumnIn in;
    in.M = M; in.K = K;
    in.obs = obs + c; in.obs_stride = ncol;
    in.wt = wt ? wt + c : nullptr; in.wt_stride = ncol;
    in.pv = pv + c; in.pv_stride = ncol;
    in.S = S + c; in.s_lstride = (long long)K * ncol; in.s_kstride = ncol;
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
    const int nvx = nx - 2, M = nz - 1;
    const long long ncol = (long long)nx * ny;
    const int bj = (int)blockIdx.x / nvx, bi = (int)blockIdx.x - bj * nvx;
    if (bj >= ny - 2) return;
    const long long c = (long long)(bj + 1) * nx + (bi + 1);
    ColumnIn in;
    in.M = M; in.K = K;
    in.obs = obs + c; in.obs_stride = ncol;
    in.wt = wt ? wt + c : nullptr; in.wt_stride = ncol;
    in.pv = pv + c; in.pv_stride = ncol;
    in.S = S + c; in.s_lstride = (long long)K * ncol; in.s_kstride = ncol;
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
    const int nvx = nx - 2, M = nz - 1;
    const long long ncol = (long long)nx * ny;
    const int bj = (int)blockIdx.x / nvx, bi = (int)blockIdx.x - bj * nvx;
    if (bj >= ny - 2) return;
    const long long c = (long long)(bj + 1) * nx + (bi + 1);
    RadialIn in;
    in.M = M; in.K = K; in.love = love;
    in.obs = obs + c; in.obs_stride = ncol;
    in.wt = wt ? wt + c : nullptr; in.wt_stride = ncol;
    in.pv = pv + c; in.pv_stride = ncol;
    in.Sv = Sv + c; in.Sh = Sh + c; in.s_lstride = (long long)K * ncol; in.s_kstride = ncol;
    const ColumnWork w = radial_work(column_lds, M, K);
    int n[2] = { 0, 0 };
    double x2[2] = { 0.0, 0.0 };
    const int f = radial_step(in, smooth, damp, aniso, dvmax, minvel, maxvel, w, vsv + c, vsh + c, ncol, dv + c, dv + (long long)M * ncol + c, ncol, n, x2,
                              (int)threadIdx.x, 64, BlockBarrier());
    if (threadIdx.x == 0) { nused[c] = n[0]; nused[ncol + c] = n[1]; chi2[c] = x2[0]; chi2[ncol + c] = x2[1]; flag[c] = f; }
}

// The laterally coupled step: column_lateral.h on every interior column, the launch shape and the column of a block as
// above -- block b is interior column b of the header.  ws: lateral_ws_doubles(nvx, nvy, M) doubles in global memory, where N, the factor,
// the vectors, the columns' dot products, the scalars and the done flag lie between the launches.  No kernel waits for another block: what
// a column needs of its neighbours was written by an earlier launch.
// k_lateral_setup: assemble and factor in LDS (k_column_step's arrays), N, the factor and b to the workspace; nused / chi2 / flag: (ncol).
__global__ void __launch_bounds__(64) k_lateral_setup(int nx, int ny, int nz, int K, const float* __restrict__ obs, const float* __restrict__ wt,
                                                     const double* __restrict__ pv, const double* __restrict__ S, float smooth, float damp, float lateral,
                                                     double* __restrict__ ws_base, int* __restrict__ nused, double* __restrict__ chi2, int* __restrict__ flag)
{
    extern __shared__ double column_lds[];
    const int nvx = nx - 2, M = nz - 1;
    const long long ncol = (long long)nx * ny;
    const int bj = (int)blockIdx.x / nvx, bi = (int)blockIdx.x - bj * nvx;
    if (bj >= ny - 2) return;
    const long long c = (long long)(bj + 1) * nx + (bi + 1);
    ColumnIn in;
    in.M = M; in.K = K;
    in.obs = obs + c; in.obs_stride = ncol;
    in.wt = wt ? wt + c : nullptr; in.wt_stride = ncol;
    in.pv = pv + c; in.pv_stride = ncol;
    in.S = S + c; in.s_lstride = (long long)K * ncol; in.s_kstride = ncol;
    const ColumnWork w = column_work(column_lds, M, K);
    const LateralWs ws = lateral_ws(ws_base, nvx, ny - 2, M, lateral);
    int n = 0;
    double x2 = 0.0;
    const int f = lateral_setup(in, smooth, damp, w, ws, (int)blockIdx.x, &n, &x2, (int)threadIdx.x, 64, BlockBarrier());
    if (threadIdx.x == 0) { nused[c] = n; chi2[c] = x2; flag[c] = f; }
}

// the right-hand side with the edges' part, x0 and the columns' figures of rz0
__global__ void __launch_bounds__(64) k_lateral_start(int nvx, int nvy, int M, float lateral, double* __restrict__ ws_base, const float* __restrict__ vels)
{
    if ((int)blockIdx.x >= nvx * nvy) return;
    lateral_start(lateral_ws(ws_base, nvx, nvy, M, lateral), (int)blockIdx.x, vels, (long long)(nvx + 2) * (nvy + 2), (int)threadIdx.x, 64, BlockBarrier());
}

// r0, z0 and the columns' figures of the first rz
__global__ void __launch_bounds__(64) k_lateral_residual(int nvx, int nvy, int M, float lateral, double* __restrict__ ws_base)
{
    if ((int)blockIdx.x >= nvx * nvy) return;
    lateral_residual(lateral_ws(ws_base, nvx, nvy, M, lateral), (int)blockIdx.x, (int)threadIdx.x, 64, BlockBarrier());
}

// the two kernels of an iteration: the new direction and q = A p; the update of x and r, z = M^-1 r.  Both return at once when done is set.
__global__ void __launch_bounds__(64) k_lateral_direction(int nvx, int nvy, int M, float lateral, double* __restrict__ ws_base)
{
    if ((int)blockIdx.x >= nvx * nvy) return;
    lateral_direction(lateral_ws(ws_base, nvx, nvy, M, lateral), (int)blockIdx.x, (int)threadIdx.x, 64, BlockBarrier());
}

__global__ void __launch_bounds__(64) k_lateral_update(int nvx, int nvy, int M, float lateral, double* __restrict__ ws_base)
{
    if ((int)blockIdx.x >= nvx * nvy) return;
    lateral_update(lateral_ws(ws_base, nvx, nvy, M, lateral), (int)blockIdx.x, (int)threadIdx.x, 64, BlockBarrier());
}

// the global sums, one wavefront: lane t is chain t; lane 0 adds the chains and sets the scalars
__global__ void __launch_bounds__(64) k_lateral_reduce(int nvx, int nvy, int M, float lateral, double* __restrict__ ws_base, int what, double tol, int maxit)
{
    __shared__ double chains[kLateralChains];
    lateral_reduce(lateral_ws(ws_base, nvx, nvy, M, lateral), what, tol, maxit, chains, (int)threadIdx.x, 64, BlockBarrier());
}

// the clipped steps and the stepped model; dv: (M, ncol)
__global__ void __launch_bounds__(64) k_lateral_finish(int nvx, int nvy, int M, float lateral, double* __restrict__ ws_base, float dvmax, float minvel, float maxvel,
                                                      float* __restrict__ vels, float* __restrict__ dv)
{
    if ((int)blockIdx.x >= nvx * nvy) return;
    const long long ncol = (long long)(nvx + 2) * (nvy + 2);
    lateral_finish(lateral_ws(ws_base, nvx, nvy, M, lateral), (int)blockIdx.x, dvmax, minvel, maxvel, vels, ncol, dv, ncol, (int)threadIdx.x, 64);
}

// The laterally coupled radial step: column_radial_lateral.h on every interior column, block b interior column b.  ws:
// radial_lateral_ws_doubles(nvx, nvy, M) doubles in global memory -- column_lateral.h's workspace of 2M unknowns per column, on which
// k_lateral_update and k_lateral_reduce run as they are.  No kernel waits for another block.
// k_radial_lateral_setup: radial_assemble and the factorisation in LDS (k_column_step_radial's arrays and sizes), N, the factor and b to the
// workspace; Sv / Sh, love, nused / chi2 (2, ncol), flag (ncol) as k_column_step_radial's.
__global__ void __launch_bounds__(64) k_radial_lateral_setup(int nx, int ny, int nz, int K, unsigned long long love, const float* __restrict__ obs,
                                                            const float* __restrict__ wt, const double* __restrict__ pv, const double* __restrict__ Sv,
                                                            const double* __restrict__ Sh, float smooth, float damp, float aniso, float lateral,
                                                            float lateral_aniso, const float* __restrict__ vsv, const float* __restrict__ vsh,
                                                            double* __restrict__ ws_base, int* __restrict__ nused, double* __restrict__ chi2,
                                                            int* __restrict__ flag)
{
    extern __shared__ double column_lds[];
    const int nvx = nx - 2, M = nz - 1;
    const long long ncol = (long long)nx * ny;
    const int bj = (int)blockIdx.x / nvx, bi = (int)blockIdx.x - bj * nvx;
    if (bj >= ny - 2) return;
    const long long c = (long long)(bj + 1) * nx + (bi + 1);
    RadialIn in;
    in.M = M; in.K = K; in.love = love;
    in.obs = obs + c; in.obs_stride = ncol;
    in.wt = wt ? wt + c : nullptr; in.wt_stride = ncol;
    in.pv = pv + c; in.pv_stride = ncol;
    in.Sv = Sv + c; in.Sh = Sh + c; in.s_lstride = (long long)K * ncol; in.s_kstride = ncol;
    const ColumnWork w = radial_work(column_lds, M, K);
    const RadialLateralWs rl = radial_lateral_ws(ws_base, nvx, ny - 2, M, lateral, lateral_aniso);
    int n[2] = { 0, 0 };
    double x2[2] = { 0.0, 0.0 };
    const int f = radial_lateral_setup(in, smooth, damp, aniso, vsv + c, vsh + c, ncol, w, rl, (int)blockIdx.x, n, x2, (int)threadIdx.x, 64, BlockBarrier());
    if (threadIdx.x == 0) { nused[c] = n[0]; nused[ncol + c] = n[1]; chi2[c] = x2[0]; chi2[ncol + c] = x2[1]; flag[c] = f; }
}

// the right-hand side with the edges' parts, x0 and the columns' figures of rz0
__global__ void __launch_bounds__(64) k_radial_lateral_start(int nvx, int nvy, int M, float lateral, float lateral_aniso, double* __restrict__ ws_base,
                                                            const float* __restrict__ vsv, const float* __restrict__ vsh)
{
    if ((int)blockIdx.x >= nvx * nvy) return;
    radial_lateral_start(radial_lateral_ws(ws_base, nvx, nvy, M, lateral, lateral_aniso), (int)blockIdx.x, vsv, vsh, (long long)(nvx + 2) * (nvy + 2),
                         (int)threadIdx.x, 64, BlockBarrier());
}

// r0, z0 and the columns' figures of the first rz
__global__ void __launch_bounds__(64) k_radial_lateral_residual(int nvx, int nvy, int M, float lateral, float lateral_aniso, double* __restrict__ ws_base)
{
    if ((int)blockIdx.x >= nvx * nvy) return;
    radial_lateral_residual(radial_lateral_ws(ws_base, nvx, nvy, M, lateral, lateral_aniso), (int)blockIdx.x, (int)threadIdx.x, 64, BlockBarrier());
}

// the first kernel of an iteration: the new direction and q = A p; returns at once when done is set.  The second is k_lateral_update.
__global__ void __launch_bounds__(64) k_radial_lateral_direction(int nvx, int nvy, int M, float lateral, float lateral_aniso, double* __restrict__ ws_base)
{
    if ((int)blockIdx.x >= nvx * nvy) return;
    radial_lateral_direction(radial_lateral_ws(ws_base, nvx, nvy, M, lateral, lateral_aniso), (int)blockIdx.x, (int)threadIdx.x, 64, BlockBarrier());
}

// the clipped steps and the two stepped models; dv: (2, M, ncol)
__global__ void __launch_bounds__(64) k_radial_lateral_finish(int nvx, int nvy, int M, float lateral, float lateral_aniso, double* __restrict__ ws_base,
                                                             float dvmax, float minvel, float maxvel, float* __restrict__ vsv, float* __restrict__ vsh,
                                                             float* __restrict__ dv)
{
    if ((int)blockIdx.x >= nvx * nvy) return;
    const long long ncol = (long long)(nvx + 2) * (nvy + 2);
    radial_lateral_finish(radial_lateral_ws(ws_base, nvx, nvy, M, lateral, lateral_aniso), (int)blockIdx.x, dvmax, minvel, maxvel, vsv, vsh, ncol, dv,
                          dv + (long long)M * ncol, ncol, (int)threadIdx.x, 64);
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

size_t column_resolution_lds_bytes(int nz, int K) { return column_resolution_doubles(nz - 1, K) * sizeof(double); }

// 0: launched; 1: the case needs more dynamic LDS than a block of this device may have (*limit_out); 2: the device refused the attribute
int launch_column_resolution(int device, int nx, int ny, int nz, int K, const float* d_obs, const float* d_wt, const double* d_pv, const double* d_S,
                             const float* d_depz, float smooth, float damp, double* d_measures, double* d_leverage, double* d_trace, double* d_R, int* d_nused,
                             int* d_flag, hipStream_t stream, int* limit_out)
{
    if (nx < 3 || ny < 3 || nz < 2 || K < 1) return 0;
    const size_t lds = column_resolution_lds_bytes(nz, K);
    if (lds > 64 * 1024) {          // (above what a block gets without asking; the attribute is per device: set every time)
        int limit = 0;
        if (hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess) limit = 0;
        if (limit_out) *limit_out = limit;
        if (lds > (size_t)limit) return 1;
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_column_resolution), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
            (void)hipGetLastError();
            return 2;
        }
    }
    hipLaunchKernelGGL(k_column_resolution, dim3((unsigned)((nx - 2) * (ny - 2))), dim3(64), lds, stream, nx, ny, nz, K, d_obs, d_wt, d_pv, d_S, d_depz, smooth,
                       damp, d_measures, d_leverage, d_trace, d_R, d_nused, d_flag);
    return 0;
}

size_t column_radial_lds_bytes(int nz, int K) { return radial_work_doubles(nz - 1, K) * sizeof(double); }

// launch_column_resolution's rule for the LDS and its return values
int launch_column_step_radial(int device, int nx, int ny, int nz, int K, unsigned long long love, const float* d_obs, const float* d_wt, const double* d_pv,
                              const double* d_Sv, const double* d_Sh, float smooth, float damp, float aniso, float dvmax, float minvel, float maxvel, float* d_vsv,
                              float* d_vsh, float* d_dv, int* d_nused, double* d_chi2, int* d_flag, hipStream_t stream, int* limit_out)
{
    if (nx < 3 || ny < 3 || nz < 2 || K < 1) return 0;
    const size_t lds = column_radial_lds_bytes(nz, K);
    if (lds > 64 * 1024) {
        int limit = 0;
        if (hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess) limit = 0;
        if (limit_out) *limit_out = limit;
        if (lds > (size_t)limit) return 1;
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_column_step_radial), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
            (void)hipGetLastError();
            return 2;
        }
    }
    hipLaunchKernelGGL(k_column_step_radial, dim3((unsigned)((nx - 2) * (ny - 2))), dim3(64), lds, stream, nx, ny, nz, K, love, d_obs, d_wt, d_pv, d_Sv, d_Sh,
                       smooth, damp, aniso, dvmax, minvel, maxvel, d_vsv, d_vsh, d_dv, d_nused, d_chi2, d_flag);
    return 0;
}

size_t column_lateral_ws_bytes(int nx, int ny, int nz) { return lateral_ws_doubles(nx - 2, ny - 2, nz - 1) * sizeof(double); }

void launch_lateral_setup(int nx, int ny, int nz, int K, const float* d_obs, const float* d_wt, const double* d_pv, const double* d_S, float smooth, float damp,
                          float lateral, double tol, double* d_ws, const float* d_vels, int* d_nused, double* d_chi2, int* d_flag, hipStream_t stream)
{
    if (nx < 3 || ny < 3 || nz < 2 || K < 1) return;
    const dim3 grid((unsigned)((nx - 2) * (ny - 2)));
    const size_t lds = column_work_doubles(nz - 1, K) * sizeof(double);
    hipLaunchKernelGGL(k_lateral_setup, grid, dim3(64), lds, stream, nx, ny, nz, K, d_obs, d_wt, d_pv, d_S, smooth, damp, lateral, d_ws, d_nused, d_chi2, d_flag);
    hipLaunchKernelGGL(k_lateral_start, grid, dim3(64), 0, stream, nx - 2, ny - 2, nz - 1, lateral, d_ws, d_vels);
    hipLaunchKernelGGL(k_lateral_reduce, dim3(1), dim3(64), 0, stream, nx - 2, ny - 2, nz - 1, lateral, d_ws, (int)kLatSumRz0, tol, 0);
}

void launch_lateral_first(int nx, int ny, int nz, float lateral, double* d_ws, double tol, int maxit, hipStream_t stream)
{
    if (nx < 3 || ny < 3 || nz < 2) return;
    hipLaunchKernelGGL(k_lateral_residual, dim3((unsigned)((nx - 2) * (ny - 2))), dim3(64), 0, stream, nx - 2, ny - 2, nz - 1, lateral, d_ws);
    hipLaunchKernelGGL(k_lateral_reduce, dim3(1), dim3(64), 0, stream, nx - 2, ny - 2, nz - 1, lateral, d_ws, (int)kLatSumFirst, tol, maxit);
}

void launch_lateral_iteration(int nx, int ny, int nz, float lateral, double* d_ws, double tol, int maxit, hipStream_t stream)
{
    if (nx < 3 || ny < 3 || nz < 2) return;
    const dim3 grid((unsigned)((nx - 2) * (ny - 2)));
    hipLaunchKernelGGL(k_lateral_direction, grid, dim3(64), 0, stream, nx - 2, ny - 2, nz - 1, lateral, d_ws);
    hipLaunchKernelGGL(k_lateral_reduce, dim3(1), dim3(64), 0, stream, nx - 2, ny - 2, nz - 1, lateral, d_ws, (int)kLatSumPq, tol, maxit);
    hipLaunchKernelGGL(k_lateral_update, grid, dim3(64), 0, stream, nx - 2, ny - 2, nz - 1, lateral, d_ws);
    hipLaunchKernelGGL(k_lateral_reduce, dim3(1), dim3(64), 0, stream, nx - 2, ny - 2, nz - 1, lateral, d_ws, (int)kLatSumRz, tol, maxit);
}

void launch_lateral_finish(int nx, int ny, int nz, float lateral, double* d_ws, float dvmax, float minvel, float maxvel, float* d_vels, float* d_dv, hipStream_t stream)
{
    if (nx < 3 || ny < 3 || nz < 2) return;
    hipLaunchKernelGGL(k_lateral_finish, dim3((unsigned)((nx - 2) * (ny - 2))), dim3(64), 0, stream, nx - 2, ny - 2, nz - 1, lateral, d_ws, dvmax, minvel, maxvel,
                       d_vels, d_dv);
}

// where the done flag, the count and the stop code (3 ints) and the scalars lie in the workspace, for the host's copies
const int* column_lateral_ints(double* d_ws, int nx, int ny, int nz) { return lateral_ws(d_ws, nx - 2, ny - 2, nz - 1, 0.0f).ic; }
const double* column_lateral_scalars(double* d_ws, int nx, int ny, int nz) { return lateral_ws(d_ws, nx - 2, ny - 2, nz - 1, 0.0f).sc; }

size_t column_radial_lateral_ws_bytes(int nx, int ny, int nz) { return radial_lateral_ws_doubles(nx - 2, ny - 2, nz - 1) * sizeof(double); }

namespace {
// what k_lateral_update and k_lateral_reduce get as their `lateral`: they ask it only whether there are edges
float radial_lateral_edges(float lateral, float lateral_aniso) { return (lateral > 0.0f || lateral_aniso > 0.0f) ? 1.0f : 0.0f; }
}

// launch_column_step_radial's rule for the LDS of the set-up kernel and its return values; nothing is launched unless 0 is returned
int launch_radial_lateral_setup(int device, int nx, int ny, int nz, int K, unsigned long long love, const float* d_obs, const float* d_wt, const double* d_pv,
                                const double* d_Sv, const double* d_Sh, float smooth, float damp, float aniso, float lateral, float lateral_aniso, double tol,
                                double* d_ws, const float* d_vsv, const float* d_vsh, int* d_nused, double* d_chi2, int* d_flag, hipStream_t stream, int* limit_out)
{
    if (nx < 3 || ny < 3 || nz < 2 || K < 1) return 0;
    const size_t lds = column_radial_lds_bytes(nz, K);
    int limit = 0;
    if (hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess) limit = 0;
    if (limit_out) *limit_out = limit;
    if (lds > (size_t)limit) return 1;
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(&k_radial_lateral_setup), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        (void)hipGetLastError();
        return 2;
    }
    const dim3 grid((unsigned)((nx - 2) * (ny - 2)));
    hipLaunchKernelGGL(k_radial_lateral_setup, grid, dim3(64), lds, stream, nx, ny, nz, K, love, d_obs, d_wt, d_pv, d_Sv, d_Sh, smooth, damp, aniso, lateral,
                       lateral_aniso, d_vsv, d_vsh, d_ws, d_nused, d_chi2, d_flag);
    hipLaunchKernelGGL(k_radial_lateral_start, grid, dim3(64), 0, stream, nx - 2, ny - 2, nz - 1, lateral, lateral_aniso, d_ws, d_vsv, d_vsh);
    hipLaunchKernelGGL(k_lateral_reduce, dim3(1), dim3(64), 0, stream, nx - 2, ny - 2, 2 * (nz - 1), radial_lateral_edges(lateral, lateral_aniso), d_ws,
                       (int)kLatSumRz0, tol, 0);
    return 0;
}

void launch_radial_lateral_first(int nx, int ny, int nz, float lateral, float lateral_aniso, double* d_ws, double tol, int maxit, hipStream_t stream)
{
    if (nx < 3 || ny < 3 || nz < 2) return;
    hipLaunchKernelGGL(k_radial_lateral_residual, dim3((unsigned)((nx - 2) * (ny - 2))), dim3(64), 0, stream, nx - 2, ny - 2, nz - 1, lateral, lateral_aniso, d_ws);
    hipLaunchKernelGGL(k_lateral_reduce, dim3(1), dim3(64), 0, stream, nx - 2, ny - 2, 2 * (nz - 1), radial_lateral_edges(lateral, lateral_aniso), d_ws,
                       (int)kLatSumFirst, tol, maxit);
}

void launch_radial_lateral_iteration(int nx, int ny, int nz, float lateral, float lateral_aniso, double* d_ws, double tol, int maxit, hipStream_t stream)
{
    if (nx < 3 || ny < 3 || nz < 2) return;
    const dim3 grid((unsigned)((nx - 2) * (ny - 2)));
    const float edges = radial_lateral_edges(lateral, lateral_aniso);
    hipLaunchKernelGGL(k_radial_lateral_direction, grid, dim3(64), 0, stream, nx - 2, ny - 2, nz - 1, lateral, lateral_aniso, d_ws);
    hipLaunchKernelGGL(k_lateral_reduce, dim3(1), dim3(64), 0, stream, nx - 2, ny - 2, 2 * (nz - 1), edges, d_ws, (int)kLatSumPq, tol, maxit);
    hipLaunchKernelGGL(k_lateral_update, grid, dim3(64), 0, stream, nx - 2, ny - 2, 2 * (nz - 1), edges, d_ws);
    hipLaunchKernelGGL(k_lateral_reduce, dim3(1), dim3(64), 0, stream, nx - 2, ny - 2, 2 * (nz - 1), edges, d_ws, (int)kLatSumRz, tol, maxit);
}

void launch_radial_lateral_finish(int nx, int ny, int nz, float lateral, float lateral_aniso, double* d_ws, float dvmax, float minvel, float maxvel, float* d_vsv,
                                  float* d_vsh, float* d_dv, hipStream_t stream)
{
    if (nx < 3 || ny < 3 || nz < 2) return;
    hipLaunchKernelGGL(k_radial_lateral_finish, dim3((unsigned)((nx - 2) * (ny - 2))), dim3(64), 0, stream, nx - 2, ny - 2, nz - 1, lateral, lateral_aniso, d_ws,
                       dvmax, minvel, maxvel, d_vsv, d_vsh, d_dv);
}

const int* column_radial_lateral_ints(double* d_ws, int nx, int ny, int nz) { return radial_lateral_ws(d_ws, nx - 2, ny - 2, nz - 1, 0.0f, 0.0f).ws.ic; }
const double* column_radial_lateral_scalars(double* d_ws, int nx, int ny, int nz) { return radial_lateral_ws(d_ws, nx - 2, ny - 2, nz - 1, 0.0f, 0.0f).ws.sc; }

}  // namespace dsa
