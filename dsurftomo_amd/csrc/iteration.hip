// Host side of one outer iteration around the device calls: what the reference's main program
// does between CalSurfG and LSMR (main.f90:361-466) and after LSMR (main.f90:520-535).  Plain host code with the
// reference's fp32 arithmetic, so that an iteration driven through this library (dsurftomo_amd/invert.py) produces the
// reference's numbers; O(nar) work, no device involved.  The four *_device entries do the same step where the rows are: each checks its
// arguments and the kind of the resident rows, makes the right-hand side, and describes its system to the one builder
// (build_resident_system), which does everything that touches the device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/dsurftomo_amd.h"
#include "engine.h"
#include "joint_system.h"
#include "map_system.h"
#include "radial_system.h"
#include "spmv_state.h"

namespace dsa {
int spmv_load_from_device(Engine* e, int m, int n, long long nar, const float* d_rw, const int* d_row, const int* d_col, long long nar_data);
void spmv_abs_column_sums(Engine* e, float* d_out);
}

namespace {

// cbst = obst - dsyn (main.f90:361-363); data outside [q25, q75] * threshold0 get weight 0 and residual 0 (:366-372);
// q25 / q75: elements int(0.25 N) and int(0.75 N) of the sorted residuals (getpercentile.f90:27-30)
int residual_weights(int dall, const float* obst, const float* dsyn, float threshold0, float* cbst, float* datweight)
{
    for (int i = 0; i < dall; ++i) cbst[i] = obst[i] - dsyn[i];
    float q25, q75;
    {
        std::vector<float> ra(cbst, cbst + dall);
        const int i25 = (int)(0.25f * (float)dall), i75 = (int)(0.75f * (float)dall);          // 1-based ranks
        if (i25 < 1 || i75 < 1) return DSA_ERR_ARGUMENT;
        std::nth_element(ra.begin(), ra.begin() + (i75 - 1), ra.end());
        q75 = ra[i75 - 1];
        if (i25 < i75) std::nth_element(ra.begin(), ra.begin() + (i25 - 1), ra.begin() + (i75 - 1));
        q25 = ra[i25 - 1];
    }
    const float lo = q25 * threshold0, hi = q75 * threshold0;
    for (int i = 0; i < dall; ++i) {
        const bool out = cbst[i] < lo || cbst[i] > hi;
        datweight[i] = out ? 0.0f : 1.0f;
        if (out) cbst[i] = 0.0f;
    }
    return 0;
}

// The right-hand side of the three block systems (joint, maps, radial): residual_weights, then the host route's product
// fl(residual * weight) -- under a zero weight a zero with the residual's sign, where residual_weights alone leaves +0 -- and `zeros`
// zero elements below the dall data rows.
int block_rhs(int dall, const float* obst, const float* dsyn, float threshold0, long long zeros, float* cbst, float* datweight)
{
    const int rc = residual_weights(dall, obst, dsyn, threshold0, cbst, datweight);
    if (rc != 0) return rc;
    for (int i = 0; i < dall; ++i) cbst[i] = (obst[i] - dsyn[i]) * datweight[i];
    for (long long i = 0; i < zeros; ++i) cbst[dall + i] = 0.0f;
    return 0;
}

// DWS block by block (main.f90:386-392): dws[2 B], dws[2 B + 1] = {max, mean} of block B's per_block elements of norm; the sum is
// sequential in fp32
void block_max_mean(const float* norm, int nblocks, long long per_block, float* dws)
{
    for (int B = 0; B < nblocks; ++B) {
        const float* nb = norm + (size_t)B * (size_t)per_block;
        float total = 0.0f, top = 0.0f;
        for (long long i = 0; i < per_block; ++i) { total = total + nb[i]; if (nb[i] > top) top = nb[i]; }
        dws[2 * B] = top; dws[2 * B + 1] = total / (float)per_block;
    }
}

long long regularisation_entries(int nvx, int nvz, int nl)
{
    const long long maxvp = (long long)nvx * nvz * nl;
    long long interior = 0;
    if (nvx > 2 && nvz > 2 && nl > 2) interior = (long long)(nvx - 2) * (nvz - 2) * (nl - 2);
    return 7 * interior + (maxvp - interior);
}

// first-difference Laplacian rows, one per model parameter in (k, j, i) order: 2 w on the model's faces, 6 w and six -w
// inside (main.f90:420-457); row numbers continue behind the dall data rows; returns the entries written
long long regularisation_rows(int nvx, int nvz, int nl, float weight0, int dall, float* rw, int* row_out, int* col)
{
    long long nar = 0;
    int row = dall;
    const int plane = nvz * nvx;
    for (int k = 1; k <= nl; ++k)
        for (int j = 1; j <= nvz; ++j)
            for (int i = 1; i <= nvx; ++i) {
                ++row;
                const int here = (k - 1) * plane + (j - 1) * nvx + i;
                const bool face = i == 1 || i == nvx || j == 1 || j == nvz || k == 1 || k == nl;
                if (face) {
                    col[nar] = here; rw[nar] = 2.0f * weight0; row_out[nar] = row;
                    nar += 1;
                } else {
                    const int nb[7] = { here, here - 1, here + 1, here - nvx, here + nvx, here - plane, here + plane };
                    for (int q = 0; q < 7; ++q) {
                        col[nar + q] = nb[q];
                        rw[nar + q] = q == 0 ? 6.0f * weight0 : -1.0f * weight0;
                        row_out[nar + q] = row;
                    }
                    nar += 7;
                }
            }
    return nar;
}

// rw[k] *= w[row[k] - 1] (main.f90:379)
__global__ void k_scale_rows(long long nar, float* __restrict__ rw, const int* __restrict__ row, const float* __restrict__ w)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nar) return;
    rw[k] = rw[k] * w[row[k] - 1];
}

// The Laplacian rows of the joint system's three blocks (joint_system.h), written where the data rows are: thread t = (block B, unknown
// `index`) writes its 1 or 7 entries at first + B * per_block + joint_first_entry(index) -- row dall + B maxvp + index + 1, column
// B maxvp + the block's column, value (float)c * w in one rounded product, w = weight0 on block 0 and weight_azi on blocks 1 and 2.
__global__ __launch_bounds__(256) void k_laplacian_blocks(int nvx, int nvz, int nl, int dall, long long first, long long per_block, float weight0,
                                                          float weight_azi, float* __restrict__ rw, int* __restrict__ row, int* __restrict__ col)
{
    const long long maxvp = (long long)nvx * nvz * nl;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 3 * maxvp) return;
    const int B = (int)(t / maxvp);
    const long long index = t - B * maxvp;
    const float w = B == 0 ? weight0 : weight_azi;
    const long long at = first + B * per_block + dsa::joint_first_entry(nvx, nvz, nl, index);
    const int count = dsa::joint_row_entries(nvx, nvz, nl, index);
    for (int q = 0; q < count; ++q) {
        long long c1;
        int coef;
        dsa::joint_entry(nvx, nvz, nl, index, q, &c1, &coef);
        rw[at + q] = (float)coef * w;
        row[at + q] = (int)(dall + t + 1);
        col[at + q] = (int)(B * maxvp + c1);
    }
}

// The Laplacian rows of the map system (map_system.h), written where the data rows are: thread t = unknown `index` in column order writes
// its 1 or 5 entries at first + map_first_entry(index) -- row dall + index + 1, value (float)c * w in one rounded product, w = weight0 on
// the planes of block 0 (the first nmaps planes) and weight_azi on the others.
__global__ __launch_bounds__(256) void k_laplacian_maps(int nvx, int nvz, int nmaps, long long n, int dall, long long first, float weight0, float weight_azi,
                                                        float* __restrict__ rw, int* __restrict__ row, int* __restrict__ col)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const long long plane = t / ((long long)nvx * nvz);
    const float w = plane < nmaps ? weight0 : weight_azi;
    const long long at = first + dsa::map_first_entry(nvx, nvz, t);
    const int count = dsa::map_row_entries(nvx, nvz, t);
    for (int q = 0; q < count; ++q) {
        long long c1;
        int coef;
        dsa::map_entry(nvx, nvz, t, q, &c1, &coef);
        rw[at + q] = (float)coef * w;
        row[at + q] = (int)(dall + t + 1);
        col[at + q] = (int)c1;
    }
}

// The rows below the data rows of the radial system (radial_system.h), written where the data rows are: thread t = (part, unknown `index`),
// part 0 and 1 the Laplacian rows of the Vsv and Vsh blocks, part 2 the tie rows; every position, row, column and value is that header's.
__global__ __launch_bounds__(256) void k_radial_system(int nvx, int nvz, int nl, int dall, long long first, float weight0, float weight_h, float aniso,
                                                       float* __restrict__ rw, int* __restrict__ row, int* __restrict__ col)
{
    const long long maxvp = (long long)nvx * nvz * nl;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 3 * maxvp) return;
    const int part = (int)(t / maxvp);
    const long long index = t - part * maxvp;
    const long long at = first + dsa::radial_first_entry(nvx, nvz, nl, part, index);
    const int count = dsa::radial_row_entries(nvx, nvz, nl, part, index);
    const int r = (int)dsa::radial_row(nvx, nvz, nl, dall, part, index);
    for (int q = 0; q < count; ++q) {
        long long c1;
        int coef;
        dsa::radial_entry(nvx, nvz, nl, part, index, q, &c1, &coef);
        rw[at + q] = dsa::radial_value(part, coef, weight0, weight_h, aniso);
        row[at + q] = r;
        col[at + q] = (int)c1;
    }
}

// What an entry asks build_resident_system to build on the nar_in resident entries, after its own checks
struct ResidentSystem {
    const char* who;                   // the entry's name in messages
    int dall;                          // data rows
    long long n, below;                // columns; rows below the data rows: m = dall + below
    long long nar_in, appended;        // resident entries; entries of the rows below, written behind them
    int nblocks;                       // dws: {max, mean} of norm over nblocks blocks ...
    long long per_block;               // ... of per_block unknowns
    dsa::Engine::RowsKind kind;        // what the entries are afterwards (the isotropic entry: what it found)
    bool commit_before_load;           // G_nar / G_kind are set before the load (a later failure leaves a system) or after the column sums
    bool radial;                       // the loaded matrix is a radial system (spmv_state.h)
};

#define IT_TRY(call) do { if ((call) != hipSuccess) { e->fail(DSA_ERR_DEVICE, "%s: %s failed", s.who, #call); return DSA_ERR_DEVICE; } } while (0)

// Everything the four device entries do on the device: the data rows scaled by the 0/1 weights (rw[k] *= datweight[row[k] - 1], one fp32
// multiply per entry), the rows below them written at entry nar_in by append(nar_in) -- a copy of host-built rows or one kernel launch, which
// returns its hipError_t --, both orderings of the matrix built where the entries are (spmv_load_from_device, nar_data = nar_in), norm[n] =
// per column the sum of |entry| over the DATA entries, which lead every column in storage order (main.f90:378-392), and dws from it.
template <class Append>
int build_resident_system(dsa::Engine* e, const ResidentSystem& s, const float* datweight, float* norm, int* m_out, long long* nar_out, float* dws,
                          Append append)
{
    IT_TRY(hipSetDevice(e->device));
    const long long nar = s.nar_in + s.appended;
    const size_t used = (size_t)s.nar_in;
    dsa::OwnedBuf<float> d_w, d_norm;
    if (e->ensure(d_w, (size_t)s.dall) || e->ensure(d_norm, (size_t)s.n) ||
        e->ensure_keep(e->G_rw, (size_t)nar, used) || e->ensure_keep(e->G_row, (size_t)nar, used) || e->ensure_keep(e->G_col, (size_t)nar, used)) return e->status;
    IT_TRY(hipMemcpyAsync(d_w.p, datweight, (size_t)s.dall * 4, hipMemcpyHostToDevice, e->stream));
    IT_TRY(hipMemsetAsync(d_norm.p, 0, (size_t)s.n * 4, e->stream));
    if (s.nar_in > 0)
        hipLaunchKernelGGL(k_scale_rows, dim3((unsigned)((s.nar_in + 255) / 256)), dim3(256), 0, e->stream, s.nar_in, e->G_rw.p, e->G_row.p, d_w.p);
    IT_TRY(append(s.nar_in));
    IT_TRY(hipStreamSynchronize(e->stream));
    const int m = s.dall + (int)s.below;
    if (s.commit_before_load) { e->G_nar = nar; e->G_kind = s.kind; }
    { const int rc = dsa::spmv_load_from_device(e, m, (int)s.n, nar, e->G_rw.p, e->G_row.p, e->G_col.p, s.nar_in); if (rc != 0) return rc; }
    if (s.radial) e->spmv->radial = true;
    dsa::spmv_abs_column_sums(e, d_norm.p);
    IT_TRY(hipMemcpyAsync(norm, d_norm.p, (size_t)s.n * 4, hipMemcpyDeviceToHost, e->stream));
    IT_TRY(hipStreamSynchronize(e->stream));
    IT_TRY(hipGetLastError());
    block_max_mean(norm, s.nblocks, s.per_block, dws);
    if (!s.commit_before_load) { e->G_nar = nar; e->G_kind = s.kind; }
    *m_out = m;
    *nar_out = nar;
    return 0;
}

#undef IT_TRY

}  // namespace

extern "C" {

// cbst = obst - dsyn; data outside [q25, q75] * threshold0 get weight 0 (q25 / q75: elements int(0.25 N) and int(0.75 N)
// of the sorted residuals, getpercentile.f90:27-30); rows scaled by their weights; DWS = column sums of |G|;
// first-difference Laplacian rows appended below the data rows (2 w on the model's faces, 6 w and six -w inside).
int dsa_iteration_system(int nx, int ny, int nz, int dall, long long nar_in, long long capacity, float* rw, int* iw, int* col,
                         const float* obst, const float* dsyn, float threshold0, float weight0, float* cbst,
                         float* datweight, float* norm, int* m_out, long long* nar_out, float* dws)
{
    if (nx < 3 || ny < 3 || nz < 2 || dall < 1 || nar_in < 0 || !rw || !iw || !col || !obst || !dsyn || !cbst || !datweight || !norm ||
        !m_out || !nar_out || !dws) return DSA_ERR_ARGUMENT;
    const int nvx = nx - 2, nvz = ny - 2, nl = nz - 1;
    const long long maxvp = (long long)nvx * nvz * nl;
    { const int rc = residual_weights(dall, obst, dsyn, threshold0, cbst, datweight); if (rc != 0) return rc; }   // :361-372
    std::fill(norm, norm + maxvp, 0.0f);
    for (long long k = 0; k < nar_in; ++k) {                                                   // :378-385
        rw[k] = rw[k] * datweight[iw[1 + k] - 1];
        norm[col[k] - 1] = norm[col[k] - 1] + std::fabs(rw[k]);
    }
    block_max_mean(norm, 1, maxvp, dws);                                                       // :386-392

    // regularisation rows, one per model parameter in (k, j, i) order (:420-457)
    const long long nar_out_ = nar_in + regularisation_entries(nvx, nvz, nl);
    if (nar_out_ > capacity) return DSA_ERR_CAPACITY;                                          // the reference: stop 'increase sparsity fraction'
    for (long long i = 0; i < maxvp; ++i) cbst[dall + i] = 0.0f;
    const long long nar = nar_in + regularisation_rows(nvx, nvz, nl, weight0, dall, rw + nar_in, iw + 1 + nar_in, col + nar_in);
    const int row = dall + (int)maxvp;
    *m_out = row;
    iw[0] = (int)nar;                                                                          // :461-464
    for (long long k = 0; k < nar; ++k) iw[1 + nar + k] = col[k];
    *nar_out = nar;
    return 0;
}

// The same step on the rows that dsa_calsurfg / dsa_solve_rows left on the device (option rows_on_device, or dsa_calsurfg
// called with null rw / iw / col): the weights are applied, the regularisation rows appended and both orderings of the
// matrix built where the rows are, so the 12 bytes per entry never cross PCIe (main.f90:349-359 hands them to the host,
// :361-466 rebuilds them there, :487-489 gives them to LSMR).  Afterwards dsa_lsmr solves on that matrix.  Same bits as
// dsa_iteration_system followed by dsa_spmv_load: the scaling is one fp32 multiply per entry, the DWS column sums add
// |entry| in storage order.
int dsa_iteration_system_device(dsa_engine* h, int nx, int ny, int nz, int dall, const float* obst, const float* dsyn, float threshold0,
                                float weight0, float* cbst, float* datweight, float* norm, int* m_out, long long* nar_out, float* dws)
{
    if (!h) return DSA_ERR_ARGUMENT;
    dsa::Engine* e = reinterpret_cast<dsa::Engine*>(h);
    if (nx < 3 || ny < 3 || nz < 2 || dall < 1 || !obst || !dsyn || !cbst || !datweight || !norm || !m_out || !nar_out || !dws) { e->fail(DSA_ERR_ARGUMENT, "iteration_system_device: bad arguments"); return DSA_ERR_ARGUMENT; }
    // (radial rows are resident whatever the option rows_on_device says: dsa_solve_rows_radial leaves them without it)
    if (e->G_kind == dsa::Engine::kRowsRadial || e->G_kind == dsa::Engine::kRowsRadialSystem) { e->fail(DSA_ERR_STATE, "iteration_system_device: the rows on the device are radial rows (a Vsv and a Vsh block of columns): dsa_iteration_system_radial_device builds their system"); return DSA_ERR_STATE; }
    if (!e->rows_on_device || (e->G_nar > 0 && !e->G_rw.p)) { e->fail(DSA_ERR_STATE, "iteration_system_device: no rows on the device (option rows_on_device + dsa_solve_rows, or dsa_calsurfg with null arrays)"); return DSA_ERR_STATE; }
    if (e->G_kind == dsa::Engine::kRowsAzimuthal || e->G_kind == dsa::Engine::kRowsJoint) { e->fail(DSA_ERR_STATE, "iteration_system_device: the rows on the device are azimuthal rows (three blocks of columns): dsa_iteration_system_azimuthal_device builds their system"); return DSA_ERR_STATE; }
    if (e->G_kind == dsa::Engine::kRowsMaps || e->G_kind == dsa::Engine::kRowsMapSystem) { e->fail(DSA_ERR_STATE, "iteration_system_device: the rows on the device are map rows (columns per period): dsa_iteration_system_maps_device builds their system"); return DSA_ERR_STATE; }
    const int nvx = nx - 2, nvz = ny - 2, nl = nz - 1;
    const long long maxvp = (long long)nvx * nvz * nl, nar_in = e->G_nar;
    { const int rc = residual_weights(dall, obst, dsyn, threshold0, cbst, datweight); if (rc != 0) { e->fail(rc, "iteration_system_device: too few data"); return rc; } }
    for (long long i = 0; i < maxvp; ++i) cbst[dall + i] = 0.0f;
    const long long nreg = regularisation_entries(nvx, nvz, nl);
    if (nar_in + nreg > 0x7fffffffll) { e->fail(DSA_ERR_CAPACITY, "iteration_system_device: more than 2^31-1 matrix entries"); return DSA_ERR_CAPACITY; }
    std::vector<float> hrw((size_t)nreg);
    std::vector<int> hrow((size_t)nreg), hcol((size_t)nreg);
    regularisation_rows(nvx, nvz, nl, weight0, dall, hrw.data(), hrow.data(), hcol.data());
    // (the kind of the entries stays what it was found to be: isotropic rows, or none where no ray left an entry)
    const ResidentSystem s = { "iteration_system_device", dall, maxvp, maxvp, nar_in, nreg, 1, maxvp, e->G_kind, false, false };
    return build_resident_system(e, s, datweight, norm, m_out, nar_out, dws, [&](long long first) {
        hipError_t rc = hipMemcpyAsync(e->G_rw.p + first, hrw.data(), (size_t)nreg * 4, hipMemcpyHostToDevice, e->stream);
        if (rc == hipSuccess) rc = hipMemcpyAsync(e->G_row.p + first, hrow.data(), (size_t)nreg * 4, hipMemcpyHostToDevice, e->stream);
        if (rc == hipSuccess) rc = hipMemcpyAsync(e->G_col.p + first, hcol.data(), (size_t)nreg * 4, hipMemcpyHostToDevice, e->stream);
        return rc;
    });
}

// The joint Vs | gc | gs system of the azimuthal step built where dsa_solve_rows_azimuthal_device, or
// dsa_calsurfg_azimuthal called with null rw / iw / col, left its rows: the data rows scaled by the 0/1 weights (block_rhs,
// build_resident_system), and below the dall data rows the Laplacian rows of the three blocks, written by
// k_laplacian_blocks -- block B's rows dall + B maxvp + index, columns B maxvp + ..., weight0 on Vs and weight_azi on gc and gs.
// m = dall + 3 maxvp, n = 3 maxvp.  Same bits as analyses/azimuthal.py's azimuthal_weights + azimuthal_system + dsa_spmv_load on the
// host rows of the same call; norm[3 maxvp] adds |entry| over a column's data entries in storage order, dws[2 B], dws[2 B + 1] are
// block B's {max, mean} of it (main.f90:386-392).  Every argument is checked before the device is touched.
int dsa_iteration_system_azimuthal_device(dsa_engine* h, int nx, int ny, int nz, int dall, const float* obst, const float* dsyn, float threshold0,
                                          float weight0, float weight_azi, float* cbst, float* datweight, float* norm, int* m_out, long long* nar_out,
                                          float* dws)
{
    if (!h) return DSA_ERR_ARGUMENT;
    dsa::Engine* e = reinterpret_cast<dsa::Engine*>(h);
    if (nx < 3 || ny < 3 || nz < 2 || dall < 1 || !obst || !dsyn || !cbst || !datweight || !norm || !m_out || !nar_out || !dws) { e->fail(DSA_ERR_ARGUMENT, "iteration_system_azimuthal_device: bad arguments"); return DSA_ERR_ARGUMENT; }
    if (!std::isfinite(weight0) || weight0 < 0.0f || !std::isfinite(weight_azi) || weight_azi < 0.0f) {
        e->fail(DSA_ERR_ARGUMENT, "iteration_system_azimuthal_device: weight0 %g and weight_azi %g must be finite and >= 0", (double)weight0, (double)weight_azi);
        return DSA_ERR_ARGUMENT;
    }
    const int nvx = nx - 2, nvz = ny - 2, nl = nz - 1;
    const long long maxvp = (long long)nvx * nvz * nl;
    if (3 * maxvp + dall > 0x7fffffffll) { e->fail(DSA_ERR_ARGUMENT, "iteration_system_azimuthal_device: %lld rows do not fit an int", 3 * maxvp + dall); return DSA_ERR_ARGUMENT; }
    if (e->G_kind != dsa::Engine::kRowsAzimuthal || e->G_nar < 1 || !e->G_rw.p) {
        e->fail(DSA_ERR_STATE, "iteration_system_azimuthal_device: %s (dsa_solve_rows_azimuthal_device, or dsa_calsurfg_azimuthal with null arrays, first)",
                e->G_kind == dsa::Engine::kRowsIsotropic ? "the rows on the device are isotropic rows" :
                e->G_kind == dsa::Engine::kRowsJoint ? "the rows on the device are a joint system already" : "no azimuthal rows on the device");
        return DSA_ERR_STATE;
    }
    const long long nar_in = e->G_nar, per_block = dsa::joint_block_entries(nvx, nvz, nl);
    if (nar_in + 3 * per_block > 0x7fffffffll) { e->fail(DSA_ERR_CAPACITY, "iteration_system_azimuthal_device: more than 2^31-1 matrix entries"); return DSA_ERR_CAPACITY; }
    { const int rc = block_rhs(dall, obst, dsyn, threshold0, 3 * maxvp, cbst, datweight); if (rc != 0) { e->fail(rc, "iteration_system_azimuthal_device: too few data"); return rc; } }
    const ResidentSystem s = { "iteration_system_azimuthal_device", dall, 3 * maxvp, 3 * maxvp, nar_in, 3 * per_block, 3, maxvp, dsa::Engine::kRowsJoint, false, false };
    return build_resident_system(e, s, datweight, norm, m_out, nar_out, dws, [&](long long first) {
        hipLaunchKernelGGL(k_laplacian_blocks, dim3((unsigned)((3 * maxvp + 255) / 256)), dim3(256), 0, e->stream, nvx, nvz, nl, dall, first, per_block, weight0,
                           weight_azi, e->G_rw.p, e->G_row.p, e->G_col.p);
        return hipGetLastError();
    });
}

// The per-period map system built where dsa_solve_rows_maps left its rows on the device: the data rows scaled by the
// 0/1 weights and the right-hand side fl(residual * weight) (block_rhs, build_resident_system: the same code as for the joint system),
// and below the dall data rows one 2-D Laplacian row per unknown (k_laplacian_maps: map_system.h), weight0 on the planes of block 0 and
// weight_azi on those of blocks 1 and 2.  n = nblocks nmaps layer columns, m = dall + n rows.  norm[n] adds |entry| over a column's data
// entries in storage order; dws[2 B], dws[2 B + 1] are block B's {max, mean} of it.  Every argument is checked before the device is touched.
int dsa_iteration_system_maps_device(dsa_engine* h, int nx, int ny, int nmaps, int nblocks, int dall, const float* obst, const float* dsyn, float threshold0,
                                     float weight0, float weight_azi, float* cbst, float* datweight, float* norm, int* m_out, long long* nar_out, float* dws)
{
    if (!h) return DSA_ERR_ARGUMENT;
    dsa::Engine* e = reinterpret_cast<dsa::Engine*>(h);
    if (nx < 3 || ny < 3 || nmaps < 1 || (nblocks != 1 && nblocks != 3) || dall < 1 || !obst || !dsyn || !cbst || !datweight || !norm || !m_out || !nar_out || !dws) { e->fail(DSA_ERR_ARGUMENT, "iteration_system_maps_device: bad arguments"); return DSA_ERR_ARGUMENT; }
    if (!std::isfinite(weight0) || weight0 < 0.0f || !std::isfinite(weight_azi) || weight_azi < 0.0f) {
        e->fail(DSA_ERR_ARGUMENT, "iteration_system_maps_device: weight0 %g and weight_azi %g must be finite and >= 0", (double)weight0, (double)weight_azi);
        return DSA_ERR_ARGUMENT;
    }
    const int nvx = nx - 2, nvz = ny - 2;
    const long long layer = (long long)nvx * nvz, n = (long long)nblocks * nmaps * layer;
    if (n + dall > 0x7fffffffll) { e->fail(DSA_ERR_ARGUMENT, "iteration_system_maps_device: %lld rows do not fit an int", n + dall); return DSA_ERR_ARGUMENT; }
    if (e->G_kind != dsa::Engine::kRowsMaps || e->G_map_blocks != nblocks || e->G_nar < 1 || !e->G_rw.p) {
        e->fail(DSA_ERR_STATE, "iteration_system_maps_device: %s (dsa_solve_rows_maps with azimuthal = %d first)",
                e->G_kind == dsa::Engine::kRowsMapSystem ? "the rows on the device are a map system already" :
                e->G_kind == dsa::Engine::kRowsMaps ? "the map rows on the device have another number of blocks" : "no map rows on the device", nblocks == 3 ? 1 : 0);
        return DSA_ERR_STATE;
    }
    if (e->G_map_nx != nx || e->G_map_ny != ny || e->G_map_nmaps != nmaps) {
        e->fail(DSA_ERR_ARGUMENT, "iteration_system_maps_device: nx %d ny %d nmaps %d, the map rows on the device were made with %d %d %d", nx, ny, nmaps, e->G_map_nx, e->G_map_ny, e->G_map_nmaps);
        return DSA_ERR_ARGUMENT;
    }
    const long long nar_in = e->G_nar, nreg = (long long)nblocks * nmaps * dsa::map_plane_entries(nvx, nvz);
    if (nar_in + nreg > 0x7fffffffll) { e->fail(DSA_ERR_CAPACITY, "iteration_system_maps_device: more than 2^31-1 matrix entries"); return DSA_ERR_CAPACITY; }
    { const int rc = block_rhs(dall, obst, dsyn, threshold0, n, cbst, datweight); if (rc != 0) { e->fail(rc, "iteration_system_maps_device: too few data"); return rc; } }
    // (once the rows below are written the resident entries are a system, not rows to build from again -- also when a later step fails)
    const ResidentSystem s = { "iteration_system_maps_device", dall, n, n, nar_in, nreg, nblocks, nmaps * layer, dsa::Engine::kRowsMapSystem, true, false };
    return build_resident_system(e, s, datweight, norm, m_out, nar_out, dws, [&](long long first) {
        hipLaunchKernelGGL(k_laplacian_maps, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, nvx, nvz, nmaps, n, dall, first, weight0, weight_azi,
                           e->G_rw.p, e->G_row.p, e->G_col.p);
        return hipGetLastError();
    });
}

// The radial Vsv | Vsh system of the direct inversion built where dsa_solve_rows_radial left its rows: the data rows
// scaled and the right-hand side fl(residual * weight) made by the same code as for the joint system (block_rhs, build_resident_system), and
// below the dall data rows what k_radial_system writes by radial_system.h -- the Laplacian rows of the Vsv block (weight0) and of the Vsh
// block (weight_h), then maxvp tie rows {-aniso, +aniso} whose right-hand side is 0.0f - aniso * (vsh - vsv) at the unknown's node of the
// resident models (their host copies, which every call that changes the models refreshes).  m = dall + 3 maxvp, n = 2 maxvp, the tie rows
// also at aniso = 0.  norm[2 maxvp] adds |entry| over a column's data entries in storage order; dws[2 B], dws[2 B + 1] are block B's
// {max, mean} of it.  Every argument is checked before the device is touched.
int dsa_iteration_system_radial_device(dsa_engine* h, int nx, int ny, int nz, int dall, const float* obst, const float* dsyn, float threshold0,
                                       float weight0, float weight_h, float aniso, float* cbst, float* datweight, float* norm, int* m_out,
                                       long long* nar_out, float* dws)
{
    if (!h) return DSA_ERR_ARGUMENT;
    dsa::Engine* e = reinterpret_cast<dsa::Engine*>(h);
    if (nx < 3 || ny < 3 || nz < 2 || dall < 1 || !obst || !dsyn || !cbst || !datweight || !norm || !m_out || !nar_out || !dws) { e->fail(DSA_ERR_ARGUMENT, "iteration_system_radial_device: bad arguments"); return DSA_ERR_ARGUMENT; }
    if (!std::isfinite(weight0) || weight0 < 0.0f || !std::isfinite(weight_h) || weight_h < 0.0f || !std::isfinite(aniso) || aniso < 0.0f) {
        e->fail(DSA_ERR_ARGUMENT, "iteration_system_radial_device: weight0 %g, weight_h %g and aniso %g must be finite and >= 0", (double)weight0, (double)weight_h, (double)aniso);
        return DSA_ERR_ARGUMENT;
    }
    const int nvx = nx - 2, nvz = ny - 2, nl = nz - 1;
    const long long maxvp = (long long)nvx * nvz * nl;
    if (dsa::radial_rows(nvx, nvz, nl, dall) > 0x7fffffffll) { e->fail(DSA_ERR_ARGUMENT, "iteration_system_radial_device: %lld rows do not fit an int", dsa::radial_rows(nvx, nvz, nl, dall)); return DSA_ERR_ARGUMENT; }
    if (e->G_kind != dsa::Engine::kRowsRadial || e->G_nar < 1 || !e->G_rw.p) {
        e->fail(DSA_ERR_STATE, "iteration_system_radial_device: %s (dsa_solve_rows_radial with null arrays first)",
                e->G_kind == dsa::Engine::kRowsRadialSystem ? "the rows on the device are a radial system already" :
                e->G_kind == dsa::Engine::kRowsNone ? "no radial rows on the device" : "the rows on the device are not radial rows");
        return DSA_ERR_STATE;
    }
    if (!e->disp_ready || !e->disp_radial) { e->fail(DSA_ERR_STATE, "iteration_system_radial_device: no radial stage holds the models of the tie rows (dsa_dispersion_begin_radial first)"); return DSA_ERR_STATE; }
    if (e->disp_nx != nx || e->disp_ny != ny || e->disp_nz != nz) {
        e->fail(DSA_ERR_ARGUMENT, "iteration_system_radial_device: nx %d ny %d nz %d, the radial stage holds %d %d %d", nx, ny, nz, e->disp_nx, e->disp_ny, e->disp_nz);
        return DSA_ERR_ARGUMENT;
    }
    const size_t nn = (size_t)nx * ny * nz;
    if (e->h_vels.size() != nn || e->h_vsh.size() != nn) { e->fail(DSA_ERR_STATE, "iteration_system_radial_device: the radial stage's host copies of the models are missing"); return DSA_ERR_STATE; }
    const long long nar_in = e->G_nar, nreg = dsa::radial_entries(nvx, nvz, nl);
    if (nar_in + nreg > 0x7fffffffll) { e->fail(DSA_ERR_CAPACITY, "iteration_system_radial_device: more than 2^31-1 matrix entries"); return DSA_ERR_CAPACITY; }
    { const int rc = block_rhs(dall, obst, dsyn, threshold0, 2 * maxvp, cbst, datweight); if (rc != 0) { e->fail(rc, "iteration_system_radial_device: too few data"); return rc; } }
    for (long long i = 0; i < maxvp; ++i) {
        const size_t node = (size_t)dsa::radial_node(nvx, nvz, i);
        const float d = e->h_vsh[node] - e->h_vels[node];
        cbst[dall + 2 * maxvp + i] = 0.0f - aniso * d;
    }
    // (once the rows below are written the resident entries are a system, not rows to build from again -- also when a later step fails)
    const ResidentSystem s = { "iteration_system_radial_device", dall, dsa::radial_columns(nvx, nvz, nl), dsa::radial_rows(nvx, nvz, nl, dall) - dall, nar_in, nreg,
                               2, maxvp, dsa::Engine::kRowsRadialSystem, true, true };
    return build_resident_system(e, s, datweight, norm, m_out, nar_out, dws, [&](long long first) {
        hipLaunchKernelGGL(k_radial_system, dim3((unsigned)((3 * maxvp + 255) / 256)), dim3(256), 0, e->stream, nvx, nvz, nl, dall, first, weight0, weight_h, aniso,
                           e->G_rw.p, e->G_row.p, e->G_col.p);
        return hipGetLastError();
    });
}

// main.f90:520-535: the update is clipped to +-0.5 km/s, the model to [minvel, maxvel]; vsf(nx, ny, nz) column-major
int dsa_model_update(int nx, int ny, int nz, float* dv, float* vsf, float minvel, float maxvel)
{
    if (nx < 3 || ny < 3 || nz < 2 || !dv || !vsf) return DSA_ERR_ARGUMENT;
    const int nvx = nx - 2, nvz = ny - 2;
    for (int k = 0; k < nz - 1; ++k)
        for (int j = 0; j < nvz; ++j)
            for (int i = 0; i < nvx; ++i) {
                float& d = dv[((size_t)k * nvz + j) * nvx + i];
                if (d >= 0.500f) d = 0.500f;
                if (d <= -0.500f) d = -0.500f;
                float& v = vsf[((size_t)k * ny + (j + 1)) * nx + (i + 1)];
                v = v + d;
                if (v < minvel) v = minvel;
                if (v > maxvel) v = maxvel;
            }
    return 0;
}

}  // extern "C"
