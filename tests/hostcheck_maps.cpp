// TEST HARNESS (not product): the placement rules of dsurftomo_amd/csrc/map_system.h behind a C interface, for
// tests/test_hostcheck_maps.py.  Integer arithmetic and one fp32 product per entry; a library of its own so that the other harnesses stay
// as they are.
#include "../dsurftomo_amd/csrc/map_system.h"

using namespace dsa;

extern "C" {

long long hcm_plane_entries(int nvx, int nvz) { return map_plane_entries(nvx, nvz); }

// The regularisation rows of `planes` planes the way k_laplacian_maps writes them (iteration.hip), unknown by unknown in any order -- here
// the last first, so that nothing leans on the order: first[index], count[index], and the entries at first[index] + q: value (float)c * w
// with w = w0 on the first planes0 planes and wa on the others, row row0 + index + 1, column the unknown's.  Entries outside [0, cap) are
// counted and not written.  Returns that count.
long long hcm_rows(int nvx, int nvz, int planes, int planes0, float w0, float wa, int row0, long long cap, long long* first, int* count, float* rw, int* row,
                   int* col)
{
    const long long layer = (long long)nvx * nvz, n = layer * planes;
    long long outside = 0;
    for (long long index = n - 1; index >= 0; --index) {
        const float w = index / layer < planes0 ? w0 : wa;
        const long long at = map_first_entry(nvx, nvz, index);
        const int cnt = map_row_entries(nvx, nvz, index);
        first[index] = at; count[index] = cnt;
        for (int q = 0; q < cnt; ++q) {
            long long c1;
            int coef;
            map_entry(nvx, nvz, index, q, &c1, &coef);
            if (at + q < 0 || at + q >= cap) { ++outside; continue; }
            rw[at + q] = (float)coef * w;
            row[at + q] = (int)(row0 + index + 1);
            col[at + q] = (int)c1;
        }
    }
    return outside;
}

}  // extern "C"
