// Where the rows below the data rows of the radial Vsv | Vsh system lie (iteration.hip: k_radial_system): two blocks
// of maxvp = nvx * nvz * nl unknowns in joint_system.h's order.  Part 0: the Laplacian rows of block 0 (Vsv), part 1: those of block 1
// (Vsh), both by joint_system.h's rule, which is called here and not repeated; part 2: maxvp tie rows with two entries each,
// {index + 1, -1} and {maxvp + index + 1, +1}, whose stored values are 0.0f - aniso and aniso.  Integer arithmetic, every rule once,
// __host__ __device__: the kernel calls these functions, and tests/hostcheck_radial_system.cpp runs them on a CPU against the Python twin
// (dsurftomo_amd/radial.py: radial_system).  radial_value is the one place where an entry's fp32 value is formed: a single operation.
#pragma once

#include "joint_system.h"

namespace dsa {

// entries below the data rows: both Laplacian blocks, then two per tie row
DSA_JS long long radial_entries(int nvx, int nvz, int nl)
{
    return 2 * joint_block_entries(nvx, nvz, nl) + 2 * ((long long)nvx * nvz * nl);
}

// rows of the system (dall data rows, 3 maxvp below them) and its columns
DSA_JS long long radial_rows(int nvx, int nvz, int nl, long long dall) { return dall + 3 * ((long long)nvx * nvz * nl); }
DSA_JS long long radial_columns(int nvx, int nvz, int nl) { return 2 * ((long long)nvx * nvz * nl); }

// entries of row `index` of part `part` (0, 1: Laplacian rows, 1 or 7; 2: a tie row, 2)
DSA_JS int radial_row_entries(int nvx, int nvz, int nl, int part, long long index)
{
    return part == 2 ? 2 : joint_row_entries(nvx, nvz, nl, index);
}

// position of that row's first entry, counted from the first entry below the data entries
DSA_JS long long radial_first_entry(int nvx, int nvz, int nl, int part, long long index)
{
    const long long per_block = joint_block_entries(nvx, nvz, nl);
    return part == 2 ? 2 * per_block + 2 * index : part * per_block + joint_first_entry(nvx, nvz, nl, index);
}

// 1-based row of the system
DSA_JS long long radial_row(int nvx, int nvz, int nl, long long dall, int part, long long index)
{
    return dall + part * ((long long)nvx * nvz * nl) + index + 1;
}

// entry q of that row: its 1-based column of the system and its integer coefficient (Laplacian: joint_entry's in the part's block; tie:
// q = 0 {index + 1, -1}, q = 1 {maxvp + index + 1, +1})
DSA_JS void radial_entry(int nvx, int nvz, int nl, int part, long long index, int q, long long* col, int* coef)
{
    const long long maxvp = (long long)nvx * nvz * nl;
    if (part == 2) { *col = q * maxvp + index + 1; *coef = q == 0 ? -1 : 1; return; }
    long long c1;
    joint_entry(nvx, nvz, nl, index, q, &c1, coef);
    *col = part * maxvp + c1;
}

// the stored value: the one rounded product (float)c * w on a Laplacian row, w = weight0 on part 0 and weight_h on part 1; on a tie row
// 0.0f - aniso under coefficient -1 and aniso under +1
DSA_JS float radial_value(int part, int coef, float weight0, float weight_h, float aniso)
{
    if (part == 2) return coef < 0 ? 0.0f - aniso : aniso;
    return (float)coef * (part == 0 ? weight0 : weight_h);
}

// 0-based node, in a model (nz, ny, nx) with nx = nvx + 2 and ny = nvz + 2, of the unknown `index` of a block: dsa_model_update's
DSA_JS long long radial_node(int nvx, int nvz, long long index)
{
    int i, j, k;
    joint_ijk(nvx, nvz, index, &i, &j, &k);
    return ((long long)(k - 1) * (nvz + 2) + j) * (nvx + 2) + i;
}

}  // namespace dsa
