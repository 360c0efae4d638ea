// TEST HARNESS (not product): the placement rules of dsurftomo_amd/csrc/joint_system.h behind a C interface, for
// tests/test_hostcheck_joint.py.  Integer arithmetic and one fp32 product per entry; a library of its own so that the other harnesses stay
// as they are.
#include "../dsurftomo_amd/csrc/joint_system.h"

using namespace dsa;

extern "C" {

long long hcj_block_entries(int nvx, int nvz, int nl) { return joint_block_entries(nvx, nvz, nl); }

// One block the way k_laplacian_blocks writes it (iteration.hip), unknown by unknown in any order -- here the last first, so that nothing
// leans on the order: first[index], count[index], and the entries at first[index] + q: value (float)c * w, row row0 + index + 1, column
// col0 + the block's column.  Entries outside [0, cap) are counted and not written.  Returns that count.
long long hcj_block(int nvx, int nvz, int nl, float w, int row0, int col0, long long cap, long long* first, int* count, float* rw, int* row, int* col)
{
    const long long maxvp = (long long)nvx * nvz * nl;
    long long outside = 0;
    for (long long index = maxvp - 1; index >= 0; --index) {
        const long long at = joint_first_entry(nvx, nvz, nl, index);
        const int cnt = joint_row_entries(nvx, nvz, nl, index);
        first[index] = at; count[index] = cnt;
        for (int q = 0; q < cnt; ++q) {
            long long c1;
            int coef;
            joint_entry(nvx, nvz, nl, index, q, &c1, &coef);
            if (at + q < 0 || at + q >= cap) { ++outside; continue; }
            rw[at + q] = (float)coef * w;
            row[at + q] = (int)(row0 + index + 1);
            col[at + q] = (int)(col0 + c1);
        }
    }
    return outside;
}

}  // extern "C"
