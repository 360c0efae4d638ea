// The exact resolution and covariance of the period maps: section 22's method one level up.  The map system of
// section 20 never couples two periods, so its normal matrix is block diagonal, one dense block per map, small enough to factor exactly.
//
// Input: the resident (m x n) matrix as a row CSR (rptr, rval, ridx) and a column CSC (cptr, cval, cidx: the rows of a column's entries),
// 0-based, every segment in storage order, with (nx, ny, nmaps, nblocks, ndata, damp).
//
//   layer    (nx-2)(ny-2).  Unknown (B nmaps + m) layer + i belongs to map m: local index q = B layer + i, plane B, vertex (i mod (nx-2),
//            i div (nx-2)).  n_m = nblocks layer unknowns per map.
//   owner    a row belongs to map m iff every stored entry of it lies in map m's unknowns; a row with entries in two maps is refused, a
//            row without entries belongs to no map.  A column's rows must ascend strictly: an equal pair is a row that stores the column
//            twice (refused), a descending pair a matrix that was not loaded in row order (refused: the sums below run in ascending row).
//   used     a data row (index < ndata) is used iff at least one of its entries is non-zero
//   N        lower triangle, N_pq = sum_r (double)a_rp (double)a_rq over the rows r that store both columns, r ascending, from 0.0 (the
//            other rows of the map would add an exact zero); then + (double)damp (double)damp on the diagonal
//   factor   N = L D L^T by column_factor's operations in its order: v_p = L_jp d_p, s -= L_ip v_p for p ascending, s / d_j.  A pivot that
//            is not finite or <= 0: flag 1.  A map without a used datum: flag 2, not factored.  In both every output of the map is 0.
//   T        for every used datum d of the map t_d solves N t = g_d, g_d the row as doubles, by column_solve's substitutions: element i of
//            the forward pass loses L_ip t_p for p ascending, then / d_i, then i descending loses L_pi t_p for p ascending
//   R        R_lq = sum_d t_dl g_dq over the used d that store column q, d ascending, from 0.0
//   measures per unknown (local q = B layer + i), sums over l ascending in local index, from 0.0:
//            0  R_qq                                   1  var_q = sum_d t_dq t_dq over ALL used d of the map, ascending (diag T^T T)
//            2  sum_{l in plane B} R_lq^2              3, 4  the same sum weighted with (i_l - i_q)^2 and with (j_l - j_q)^2 (vertex units)
//            5  sum_{l in the map} R_lq^2              6, 7  R_lq at l = the co-located unknown of planes (B+1), (B+2) mod nblocks
//            8  sum_d t_dq t_dq', q' the co-located unknown of plane (B+1) mod nblocks, over all used d; 6, 7, 8 are 0 for nblocks = 1
//   leverage h_d = sum_q g_dq t_dq over the stored entries of row d in storage order; 0 for a datum that is not used
//   trace    per (plane, map): sum of R_qq over the plane's unknowns, ascending
//
// column_system.h's contract: __host__ __device__, fp64 under -ffp-contract=off, no libm, no square root, IEEE division, every figure one
// sequential chain of its own -- so whatever thread computes a figure, it has one value.  map_kernels.hip calls these functions for
// every figure but the factor: map_factor below is column_factor's left-looking loop, the kernels run a right-looking panel update.  Both
// subtract the SAME products L_ip (L_jp d_p) from entry (i, j) in the SAME order (p ascending) before the one division: a right-looking
// update only interrupts the chain between two panels and stores the partial sum, which is exact.  They are bit-identical by
// construction; tests/hostcheck_map_resolution.cpp holds a panelled host loop that shows it.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define DSA_MR __host__ __device__ __forceinline__
#else
#define DSA_MR static inline
#endif

namespace dsa {

constexpr int kMapPanel = 64;          // columns per panel of the device factorisation
constexpr int kMapMeasures = 9;

enum { kMapOk = 0, kMapNotPositive = 1, kMapNoData = 2 };
enum { kMapRowNone = -1, kMapRowTwoMaps = -2 };
enum { kMapColumnOk = 0, kMapColumnTwice = 1, kMapColumnOrder = 2 };

struct MapShape {
    int nx, ny, nmaps, nblocks, layer, nm, n;
};

DSA_MR MapShape map_shape(int nx, int ny, int nmaps, int nblocks)
{
    MapShape S;
    S.nx = nx; S.ny = ny; S.nmaps = nmaps; S.nblocks = nblocks;
    S.layer = (nx - 2) * (ny - 2);
    S.nm = nblocks * S.layer;
    S.n = S.nm * nmaps;
    return S;
}

// column c: its map; *q gets the local index
DSA_MR int map_of_column(const MapShape& S, int c, int* q)
{
    const int plane = c / S.layer;
    *q = (plane / S.nmaps) * S.layer + (c - plane * S.layer);
    return plane % S.nmaps;
}

DSA_MR int map_column(const MapShape& S, int m, int q)
{
    const int B = q / S.layer;
    return (B * S.nmaps + m) * S.layer + (q - B * S.layer);
}

// the owner of row r (a map, kMapRowNone or kMapRowTwoMaps) and whether it is a used datum
DSA_MR int map_row_owner(const MapShape& S, int ndata, int r, const long long* rptr, const float* rval, const int* ridx, int* used)
{
    int owner = kMapRowNone, q;
    bool nonzero = false;
    for (long long e = rptr[r]; e < rptr[r + 1]; ++e) {
        const int m = map_of_column(S, ridx[e], &q);
        if (owner == kMapRowNone) owner = m;
        else if (owner != m) owner = kMapRowTwoMaps;
        if (owner == kMapRowTwoMaps) break;
        if (rval[e] != 0.0f) nonzero = true;
    }
    *used = owner >= 0 && r < ndata && nonzero;
    return owner;
}

// the rows of column c ascend strictly
DSA_MR int map_column_check(int c, const long long* cptr, const int* cidx)
{
    int bad = kMapColumnOk;
    for (long long e = cptr[c] + 1; e < cptr[c + 1]; ++e) {
        if (cidx[e] == cidx[e - 1] && bad == kMapColumnOk) bad = kMapColumnTwice;
        if (cidx[e] < cidx[e - 1]) bad = kMapColumnOrder;
    }
    return bad;
}

// N_ip of map m (i >= p, local indices), damp2 on the diagonal
DSA_MR double map_normal_entry(const MapShape& S, int m, int i, int p, double damp2, const long long* rptr, const float* rval, const int* ridx,
                               const long long* cptr, const float* cval, const int* cidx)
{
    const int gi = map_column(S, m, i), gp = map_column(S, m, p);
    double s = 0.0;
    for (long long e = cptr[gp]; e < cptr[gp + 1]; ++e) {
        const int r = cidx[e];
        for (long long f = rptr[r]; f < rptr[r + 1]; ++f)
            if (ridx[f] == gi) { s += (double)cval[e] * (double)rval[f]; break; }
    }
    if (i == p) s = s + damp2;
    return s;
}

// N = L D L^T in place, left-looking (column_factor's loop): L holds N's lower triangle, entry (i, p) at p nm + i; on return L below the
// diagonal, d the pivots.  v: nm doubles of work.  Returns the flag.
DSA_MR int map_factor(int nm, double* L, double* d, double* v)
{
    for (int j = 0; j < nm; ++j) {
        for (int p = 0; p < j; ++p) v[p] = L[(size_t)p * nm + j] * d[p];
        double dj = L[(size_t)j * nm + j];
        for (int p = 0; p < j; ++p) dj -= L[(size_t)p * nm + j] * v[p];
        if (!(isfinite(dj) && dj > 0.0)) return kMapNotPositive;
        d[j] = dj;
        for (int i = j + 1; i < nm; ++i) {
            double s = L[(size_t)j * nm + i];
            for (int p = 0; p < j; ++p) s -= L[(size_t)p * nm + i] * v[p];
            L[(size_t)j * nm + i] = s / dj;
        }
    }
    return kMapOk;
}

// t of the used datum in row r of map m, element i at T[i Kp + k] (datum-fastest: the lanes of a wavefront run the solves of 64 data
// side by side, read the same entry of the factor and consecutive doubles of T)
DSA_MR void map_solve_datum(const MapShape& S, int r, const long long* rptr, const float* rval, const int* ridx, const double* L, const double* d,
                            double* T, long long Kp, int k)
{
    const int nm = S.nm;
    int q;
    for (int i = 0; i < nm; ++i) T[i * Kp + k] = 0.0;
    for (long long e = rptr[r]; e < rptr[r + 1]; ++e) {
        (void)map_of_column(S, ridx[e], &q);
        T[q * Kp + k] = (double)rval[e];
    }
    for (int i = 1; i < nm; ++i) {
        double s = T[i * Kp + k];
        for (int p = 0; p < i; ++p) s -= L[(size_t)p * nm + i] * T[p * Kp + k];
        T[i * Kp + k] = s;
    }
    for (int i = 0; i < nm; ++i) T[i * Kp + k] = T[i * Kp + k] / d[i];
    for (int i = nm - 2; i >= 0; --i) {
        double s = T[i * Kp + k];
        const double* col = L + (size_t)i * nm;
        for (int p = i + 1; p < nm; ++p) s -= col[p] * T[p * Kp + k];
        T[i * Kp + k] = s;
    }
}

// R_lq of map m.  kidx: per row, the place of a used datum in its map's T, or -1.
DSA_MR double map_r_entry(const MapShape& S, int m, int l, int q, int ndata, const long long* cptr, const float* cval, const int* cidx, const int* kidx,
                          const double* T, long long Kp)
{
    const int gq = map_column(S, m, q);
    double r = 0.0;
    for (long long e = cptr[gq]; e < cptr[gq + 1]; ++e) {
        const int row = cidx[e];
        if (row >= ndata) break;                                      // (the rows ascend)
        const int k = kidx[row];
        if (k >= 0) r += T[l * Kp + k] * (double)cval[e];
    }
    return r;
}

// measures 0, 2 .. 7 of local unknown q from column q of R (R_lq at R[l nm + q]); out[1] and out[8] are left alone
DSA_MR void map_moments(const MapShape& S, int q, const double* R, double* out)
{
    const int nm = S.nm, layer = S.layer, nvx = S.nx - 2;
    const int B = q / layer, iq = q - B * layer;
    const double xq = (double)(iq % nvx), yq = (double)(iq / nvx);
    double m2 = 0.0, m3 = 0.0, m4 = 0.0, m5 = 0.0;
    for (int l = 0; l < nm; ++l) {
        const double r = R[(size_t)l * nm + q], r2 = r * r;
        m5 += r2;
        if (l / layer == B) {
            const int il = l - B * layer;
            const double dx = (double)(il % nvx) - xq, dy = (double)(il / nvx) - yq;
            m2 += r2;
            m3 += r2 * (dx * dx);
            m4 += r2 * (dy * dy);
        }
    }
    out[0] = R[(size_t)q * nm + q];
    out[2] = m2; out[3] = m3; out[4] = m4; out[5] = m5;
    out[6] = S.nblocks == 1 ? 0.0 : R[(size_t)(((B + 1) % S.nblocks) * layer + iq) * nm + q];
    out[7] = S.nblocks == 1 ? 0.0 : R[(size_t)(((B + 2) % S.nblocks) * layer + iq) * nm + q];
}

// sum_d t_dq t_dq' over the K used data of the map: q' = q is measure 1, the co-located unknown of the next plane measure 8
DSA_MR double map_covariance(int q, int qp, int K, const double* T, long long Kp)
{
    double s = 0.0;
    for (int k = 0; k < K; ++k) s += T[q * Kp + k] * T[qp * Kp + k];
    return s;
}

DSA_MR int map_next_plane(const MapShape& S, int q)
{
    const int B = q / S.layer;
    return ((B + 1) % S.nblocks) * S.layer + (q - B * S.layer);
}

DSA_MR double map_leverage(const MapShape& S, int r, const long long* rptr, const float* rval, const int* ridx, const double* T, long long Kp, int k)
{
    double h = 0.0;
    int q;
    for (long long e = rptr[r]; e < rptr[r + 1]; ++e) {
        (void)map_of_column(S, ridx[e], &q);
        h += (double)rval[e] * T[q * Kp + k];
    }
    return h;
}

// the trace of plane B of map m from measure 0 (measures: (measure, unknown in column order))
DSA_MR double map_trace(const MapShape& S, int m, int B, const double* measures)
{
    const double* r = measures + (size_t)(B * S.nmaps + m) * S.layer;
    double t = 0.0;
    for (int i = 0; i < S.layer; ++i) t += r[i];
    return t;
}

}  // namespace dsa
