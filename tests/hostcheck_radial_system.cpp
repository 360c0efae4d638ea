// TEST HARNESS (not product): the placement rules of dsurftomo_amd/csrc/radial_system.h behind a C interface, for
// tests/test_hostcheck_radial_system.py.  Integer arithmetic and one fp32 operation per entry; a library of its own so that the other
// harnesses stay as they are.  With -DHOSTCHECK_RADIAL_SYSTEM_MAIN the file is a stand-alone program that writes the rows of made-up
// grids into arrays of exactly their size and checks that every entry is written once and lies in the system (what a sanitizer build runs).
#include "../dsurftomo_amd/csrc/radial_system.h"

using namespace dsa;

extern "C" {

long long hcr_entries(int nvx, int nvz, int nl) { return radial_entries(nvx, nvz, nl); }
long long hcr_rows(int nvx, int nvz, int nl, long long dall) { return radial_rows(nvx, nvz, nl, dall); }
long long hcr_columns(int nvx, int nvz, int nl) { return radial_columns(nvx, nvz, nl); }
long long hcr_node(int nvx, int nvz, long long index) { return radial_node(nvx, nvz, index); }

// Everything below the data rows the way k_radial_system writes it (iteration.hip), thread by thread in any order -- here the last first, so
// that nothing leans on the order: the entries of thread t = (part, index) at radial_first_entry + q.  hits[p] counts the writes to position
// p.  Entries outside [0, cap) are counted and not written.  Returns that count.
long long hcr_system(int nvx, int nvz, int nl, int dall, float weight0, float weight_h, float aniso, long long cap, float* rw, int* row, int* col, int* hits)
{
    const long long maxvp = (long long)nvx * nvz * nl;
    long long outside = 0;
    for (long long t = 3 * maxvp - 1; t >= 0; --t) {
        const int part = (int)(t / maxvp);
        const long long index = t - part * maxvp;
        const long long at = radial_first_entry(nvx, nvz, nl, part, index);
        const int cnt = radial_row_entries(nvx, nvz, nl, part, index);
        for (int q = 0; q < cnt; ++q) {
            long long c1;
            int coef;
            radial_entry(nvx, nvz, nl, part, index, q, &c1, &coef);
            if (at + q < 0 || at + q >= cap) { ++outside; continue; }
            rw[at + q] = radial_value(part, coef, weight0, weight_h, aniso);
            row[at + q] = (int)radial_row(nvx, nvz, nl, dall, part, index);
            col[at + q] = (int)c1;
            hits[at + q] += 1;
        }
    }
    return outside;
}

}  // extern "C"

#ifdef HOSTCHECK_RADIAL_SYSTEM_MAIN
#include <cstdio>
#include <vector>

int main()
{
    const int grids[][3] = { { 1, 1, 1 }, { 2, 2, 2 }, { 3, 3, 3 }, { 8, 7, 3 }, { 4, 5, 1 }, { 5, 4, 2 }, { 6, 3, 5 }, { 3, 9, 5 } };
    for (const auto& g : grids)
        for (float aniso : { 0.0f, 0.3f }) {
            const int nvx = g[0], nvz = g[1], nl = g[2], dall = 17;
            const long long n = hcr_entries(nvx, nvz, nl), maxvp = (long long)nvx * nvz * nl;
            std::vector<float> rw((size_t)n);
            std::vector<int> row((size_t)n), col((size_t)n), hits((size_t)n, 0);
            if (hcr_system(nvx, nvz, nl, dall, 2.0f, 0.7f, aniso, n, rw.data(), row.data(), col.data(), hits.data()) != 0) { std::printf("%d %d %d: entries outside\n", nvx, nvz, nl); return 1; }
            for (long long p = 0; p < n; ++p)
                if (hits[(size_t)p] != 1 || row[(size_t)p] <= dall || row[(size_t)p] > hcr_rows(nvx, nvz, nl, dall) || col[(size_t)p] < 1 || col[(size_t)p] > hcr_columns(nvx, nvz, nl)) {
                    std::printf("%d %d %d: entry %lld written %d times, row %d column %d\n", nvx, nvz, nl, p, hits[(size_t)p], row[(size_t)p], col[(size_t)p]);
                    return 1;
                }
            for (long long i = 0; i < maxvp; ++i)
                if (hcr_node(nvx, nvz, i) < 0 || hcr_node(nvx, nvz, i) >= (long long)(nvx + 2) * (nvz + 2) * nl) { std::printf("%d %d %d: node of %lld outside the model\n", nvx, nvz, nl, i); return 1; }
        }
    std::printf("ok\n");
    return 0;
}
#endif
