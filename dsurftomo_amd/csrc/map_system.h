// Where the first-difference Laplacian rows of the per-period map system lie (iteration.hip: k_laplacian_maps): the
// unknowns are `planes` planes of nvx * nvz vertices, i fastest, one plane per (block, map) pair; one row per unknown in column order -- one
// entry 2 w on its plane's edge, five inside (4 w, then -w on -1, +1, -nvx, +nvx), the rows of main.f90:421-457 without the depth axis.
// Planes never couple.  Integer arithmetic only, every rule once, __host__ __device__: the kernel calls these functions, and
// tests/hostcheck_maps.cpp runs them on a CPU against the Python loop (maps.py: laplacian_rows_2d).
#pragma once

#if defined(__HIPCC__)
#define DSA_MS __host__ __device__ __forceinline__
#else
#define DSA_MS static inline
#endif

namespace dsa {

DSA_MS long long map_clamp(long long v, long long hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// plane and 1-based (i, j) of the 0-based unknown `index`
DSA_MS void map_pij(int nvx, int nvz, long long index, long long* p, int* i, int* j)
{
    const long long layer = (long long)nvx * nvz;
    *p = index / layer;
    const long long r = index % layer;
    *j = (int)(r / nvx) + 1;
    *i = (int)(r % nvx) + 1;
}

DSA_MS bool map_interior(int nvx, int nvz, int i, int j) { return i > 1 && i < nvx && j > 1 && j < nvz; }

// entries of one plane: 5 per interior unknown, 1 per unknown on the edge
DSA_MS long long map_plane_entries(int nvx, int nvz)
{
    const long long ni = nvx > 2 ? nvx - 2 : 0, nj = nvz > 2 ? nvz - 2 : 0;
    return (long long)nvx * nvz + 4 * (ni * nj);
}

// position, within the regularisation entries, of the first entry of the 0-based unknown `index`: one entry per unknown before it and four
// more per interior one, of which there are  p ni nj + clamp(j-2, nj) ni + [2 <= j <= nvz-1] clamp(i-2, ni)
DSA_MS long long map_first_entry(int nvx, int nvz, long long index)
{
    const long long ni = nvx > 2 ? nvx - 2 : 0, nj = nvz > 2 ? nvz - 2 : 0;
    long long p;
    int i, j;
    map_pij(nvx, nvz, index, &p, &i, &j);
    long long before = p * ni * nj + map_clamp(j - 2, nj) * ni;
    if (j >= 2 && j <= nvz - 1) before += map_clamp(i - 2, ni);
    return index + 4 * before;
}

// entries of the row of unknown `index`: 1 or 5
DSA_MS int map_row_entries(int nvx, int nvz, long long index)
{
    long long p;
    int i, j;
    map_pij(nvx, nvz, index, &p, &i, &j);
    return map_interior(nvx, nvz, i, j) ? 5 : 1;
}

// entry q of that row: its 1-based column and its integer coefficient c (the stored value is the one rounded product (float)c * w):
// edge {here, 2}; inside q = 0 {here, 4}, q = 1 .. 4 {here -1, +1, -nvx, +nvx; -1}
DSA_MS void map_entry(int nvx, int nvz, long long index, int q, long long* col, int* coef)
{
    long long p;
    int i, j;
    map_pij(nvx, nvz, index, &p, &i, &j);
    const long long here = index + 1;
    if (!map_interior(nvx, nvz, i, j)) { *col = here; *coef = 2; return; }
    const long long step = q == 0 ? 0 : (q <= 2 ? 1 : (long long)nvx);
    *col = q == 0 ? here : ((q & 1) ? here - step : here + step);
    *coef = q == 0 ? 4 : -1;
}

}  // namespace dsa
