// Where the first-difference Laplacian rows of the joint Vs | gc | gs system lie (iteration.hip: k_laplacian_blocks):
// one row per unknown of a block of nvx * nvz * nl unknowns in (k, j, i) order, i fastest -- one entry 2 w on the block's faces, seven
// inside (6 w, then -w on -1, +1, -nvx, +nvx, -plane, +plane), the rows of main.f90:420-457.  Integer arithmetic only, every rule once,
// __host__ __device__: the kernel calls these functions, and tests/hostcheck_joint.cpp runs them on a CPU against the Python loop
// (analyses/azimuthal.py: laplacian_rows).  The isotropic builder's regularisation_rows / regularisation_entries are not touched.
#pragma once

#if defined(__HIPCC__)
#define DSA_JS __host__ __device__ __forceinline__
#else
#define DSA_JS static inline
#endif

namespace dsa {

DSA_JS long long joint_clamp(long long v, long long hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// 1-based (i, j, k) of the 0-based unknown `index` of a block
DSA_JS void joint_ijk(int nvx, int nvz, long long index, int* i, int* j, int* k)
{
    const long long plane = (long long)nvx * nvz;
    *k = (int)(index / plane) + 1;
    const long long r = index % plane;
    *j = (int)(r / nvx) + 1;
    *i = (int)(r % nvx) + 1;
}

DSA_JS bool joint_interior(int nvx, int nvz, int nl, int i, int j, int k)
{
    return i > 1 && i < nvx && j > 1 && j < nvz && k > 1 && k < nl;
}

// entries of one block: 7 per interior unknown, 1 per unknown on a face
DSA_JS long long joint_block_entries(int nvx, int nvz, int nl)
{
    const long long ni = nvx > 2 ? nvx - 2 : 0, nj = nvz > 2 ? nvz - 2 : 0, nk = nl > 2 ? nl - 2 : 0;
    return (long long)nvx * nvz * nl + 6 * (ni * nj * nk);
}

// position, within its block's entries, of the first entry of the 0-based unknown `index`: one entry per unknown before it and six more
// per interior one, of which there are  clamp(k-2, nk) ni nj + [2 <= k <= nl-1] (clamp(j-2, nj) ni + [2 <= j <= nvz-1] clamp(i-2, ni))
DSA_JS long long joint_first_entry(int nvx, int nvz, int nl, long long index)
{
    const long long ni = nvx > 2 ? nvx - 2 : 0, nj = nvz > 2 ? nvz - 2 : 0, nk = nl > 2 ? nl - 2 : 0;
    int i, j, k;
    joint_ijk(nvx, nvz, index, &i, &j, &k);
    long long before = joint_clamp(k - 2, nk) * ni * nj;
    if (k >= 2 && k <= nl - 1) {
        before += joint_clamp(j - 2, nj) * ni;
        if (j >= 2 && j <= nvz - 1) before += joint_clamp(i - 2, ni);
    }
    return index + 6 * before;
}

// entries of the row of unknown `index`: 1 or 7
DSA_JS int joint_row_entries(int nvx, int nvz, int nl, long long index)
{
    int i, j, k;
    joint_ijk(nvx, nvz, index, &i, &j, &k);
    return joint_interior(nvx, nvz, nl, i, j, k) ? 7 : 1;
}

// entry q of that row: its 1-based column within the block and its integer coefficient c (the stored value is the one rounded product
// (float)c * w): face {here, 2}; inside q = 0 {here, 6}, q = 1 .. 6 {here -1, +1, -nvx, +nvx, -plane, +plane; -1}
DSA_JS void joint_entry(int nvx, int nvz, int nl, long long index, int q, long long* col, int* coef)
{
    int i, j, k;
    joint_ijk(nvx, nvz, index, &i, &j, &k);
    const long long here = index + 1, plane = (long long)nvx * nvz;
    if (!joint_interior(nvx, nvz, nl, i, j, k)) { *col = here; *coef = 2; return; }
    const long long step = q == 0 ? 0 : (q <= 2 ? 1 : (q <= 4 ? (long long)nvx : plane));
    *col = q == 0 ? here : ((q & 1) ? here - step : here + step);
    *coef = q == 0 ? 6 : -1;
}

}  // namespace dsa
