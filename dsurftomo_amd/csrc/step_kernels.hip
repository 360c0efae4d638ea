// The two device ends of dsa_forward_steps: K Vs models from a base model and K steps, written where the dispersion
// stage reads its columns, and the travel-time misfit sums of K models from the receiver times a solve left in HBM.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"

namespace dsa {

// One thread per node of every model of a pass.  Node (ix, jy, kd) of model m0 + m is the base node, plus -- inside the outer ring in x and
// y and above the bottom layer -- the clipped step of unknown j = (kd (ny-2) + jy-1)(nx-2) + ix-1, clipped to [minvel, maxvel]: the
// arithmetic and the comparisons of dsa_model_update (iteration.hip; main.f90:520-535), one rounding per operation.  A NaN step fails
// every comparison and gives a NaN node, as there.  steps: member-major (local member m of the pass at m n), or null for the solutions
// of the last batch solve (bx: element j of realisation r at ((r / 64) n + j) 64 + r % 64, r = m0 + m).  alpha: per global member, or null.
// out[kd sd + m sm + column]: sd = nm ncol, sm = ncol is the dispersion stage's (depth, model, column); sd = ncol, sm = nz ncol is model slowest.
__global__ void k_step_models(int nx, int ny, int nz, int nm, int m0, const float* __restrict__ vsf, const float* __restrict__ steps,
                              const float* __restrict__ bx, int n, const float* __restrict__ alpha, float minvel, float maxvel,
                              float* __restrict__ out, size_t sd, size_t sm)
{
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t ncol = (size_t)nx * ny, per_model = ncol * nz;
    if (id >= per_model * nm) return;
    const int m = (int)(id / per_model);
    const size_t node = id - (size_t)m * per_model;
    const int kd = (int)(node / ncol);
    const size_t c = node - (size_t)kd * ncol;
    const int jy = (int)(c / nx), ix = (int)(c - (size_t)jy * nx);
    float v = vsf[node];
    if (ix >= 1 && ix <= nx - 2 && jy >= 1 && jy <= ny - 2 && kd < nz - 1) {
        const size_t j = ((size_t)kd * (ny - 2) + (jy - 1)) * (nx - 2) + (ix - 1);
        const int r = m0 + m;
        float s = steps ? steps[(size_t)m * n + j] : bx[((size_t)(r >> 6) * n + j) * 64 + (r & 63)];
        if (alpha) s = __fmul_rn(alpha[r], s);
        if (s >= 0.500f) s = 0.500f;
        if (s <= -0.500f) s = -0.500f;
        v = __fadd_rn(v, s);
        if (v < minvel) v = minvel;
        if (v > maxvel) v = maxvel;
    }
    out[(size_t)kd * sd + (size_t)m * sm + c] = v;
}

void launch_step_models(int nx, int ny, int nz, int nm, int m0, const float* d_vsf, const float* d_steps, const float* d_bx, int n, const float* d_alpha,
                        float minvel, float maxvel, float* d_out, size_t stride_depth, size_t stride_model, hipStream_t stream)
{
    const size_t total = (size_t)nx * ny * nz * nm;
    if (total == 0) return;
    hipLaunchKernelGGL(k_step_models, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, nx, ny, nz, nm, m0, d_vsf, d_steps, d_bx, n, d_alpha, minvel, maxvel,
                       d_out, stride_depth, stride_model);
}

// One block per (model of the pass, group): { sum (double)wr^2, sum (double)r^2 } over the data of the group, r = fl(obst - t), wr = fl(w r).
// The order of the additions is a function of the datum index alone -- thread t adds the data t, t + 256, ... in ascending order, then the
// 256 partial sums meet in a fixed tree -- so the sums do not depend on where a unit's times sit in the solve's output: model-major
// (order 0) datum i of model m is at m nd + i, period-major (order 1) at nm first[i] + m count[i] + (i - first[i]), first / count being
// the first datum and the receiver count of the datum's unit.
__global__ __launch_bounds__(256) void k_misfit_sums(const float* __restrict__ times, int order, int nm, int nd, const int* __restrict__ first,
                                                     const int* __restrict__ count, const float* __restrict__ obst, const float* __restrict__ w,
                                                     const int* __restrict__ group, int ngroups, double* __restrict__ measures)
{
    __shared__ double s_w[256], s_r[256];
    const int m = blockIdx.x, t = threadIdx.x;
    for (int g = blockIdx.y; g < ngroups; g += gridDim.y) {
        double aw = 0.0, ar = 0.0;
        for (int i = t; i < nd; i += 256) {
            if (group && group[i] != g) continue;
            const size_t pos = order == 0 ? (size_t)m * nd + i : (size_t)nm * first[i] + (size_t)m * count[i] + (size_t)(i - first[i]);
            const float r = __fsub_rn(obst[i], times[pos]);
            const float wr = w ? __fmul_rn(w[i], r) : r;
            aw = __dadd_rn(aw, __dmul_rn((double)wr, (double)wr));
            ar = __dadd_rn(ar, __dmul_rn((double)r, (double)r));
        }
        s_w[t] = aw; s_r[t] = ar;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (t < o) { s_w[t] = __dadd_rn(s_w[t], s_w[t + o]); s_r[t] = __dadd_rn(s_r[t], s_r[t + o]); }
            __syncthreads();
        }
        if (t == 0) { measures[((size_t)m * ngroups + g) * 2] = s_w[0]; measures[((size_t)m * ngroups + g) * 2 + 1] = s_r[0]; }
        __syncthreads();
    }
}

void launch_misfit_sums(const float* d_times, int order, int nm, int nd, const int* d_first, const int* d_count, const float* d_obst, const float* d_w,
                        const int* d_group, int ngroups, double* d_measures, hipStream_t stream)
{
    if (nm < 1 || ngroups < 1) return;
    hipLaunchKernelGGL(k_misfit_sums, dim3((unsigned)nm, (unsigned)std::min(ngroups, 65535)), dim3(256), 0, stream, d_times, order, nm, nd, d_first, d_count, d_obst, d_w,
                       d_group, ngroups, d_measures);
}

}  // namespace dsa
