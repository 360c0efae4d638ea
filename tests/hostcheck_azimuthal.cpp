// TEST HARNESS (not product): trace_ray<., true> (dsurftomo_amd/csrc/ray_core.h), the azimuthal back-trace, on the CPU -- the host twin of
// k_rays<., true>.  Fields in the oracle's format, as tests/hostcheck.cpp's hc_trace_ray takes them; a library of its own so that the
// isotropic harness stays as it is.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../dsurftomo_amd/csrc/host_geometry.h"
#include "../dsurftomo_amd/csrc/ray_core.h"

using namespace dsa;

extern "C" {

// ttn / veln x-major (nnz fastest), refined snapshot ttnr / nstsr x-major with leading dimension rnz.  fdm3 comes back as three slabs
// [iso | c | s], each in the oracle's layout fdm[vx * (nvz+2) + vz]; sums[2] = sums of cos 2psi and sin 2psi over the steps.
// lanes = 1, or 4: the four lanes' traces one after the other on the one slab triple (a slab row has one owner); the sums, the flag and
// the steps must then be the same from every lane (return -3 otherwise).
int hca_trace_ray(int nx, int ny, float goxd, float gozd, float dvxd, float dvzd, int gd, const float* veln, const float* ttn,
                  const float* ttnr, const int* nstsr, float sx, float sz, float rx, float rz, float* fdm3, int* flags, int* nsteps,
                  float* sums, int lanes)
{
    GridDesc g; make_grid(g, nx, ny, goxd, gozd, dvxd, dvzd, gd);
    SourceDesc s;
    if (make_source(g, sx, sz, s) != 0) return -2;
    std::vector<float> F((size_t)g.nbx * g.nbz * kTileRecs, kInf);          // compact coarse field: one float per node, tiled
    for (int ix = 0; ix < g.nnx; ++ix)
        for (int iz = 0; iz < g.nnz; ++iz) F[rec_index(g.nbz, iz, ix)] = ttn[(size_t)ix * g.nnz + iz];
    std::vector<int8_t> S((size_t)s.rnx * s.rnz);
    for (size_t k = 0; k < S.size(); ++k) S[k] = (int8_t)(nstsr[k] > 0 ? 1 : (nstsr[k] < 0 ? -1 : 0));
    const size_t slab_len = (size_t)(g.nvx + 2) * (g.nvz + 2);
    std::vector<float> slab(3 * slab_len, 0.0f);
    RayFields f{ F.data(), veln, ttnr, S.data() };
    int rc = 0;
    if (lanes == 1) {
        *flags = 0;
        rc = trace_ray<1, true>(g, s, f, rx, rz, min_cell_km(g), slab.data(), flags, nsteps, nullptr, 0, sums);
    } else {
        int fl0 = 0, st0 = 0;
        float sm0[2] = { 0.0f, 0.0f };
        for (int sub = 3; sub >= 0; --sub) {
            *flags = 0;
            sums[0] = sums[1] = 0.0f;
            rc = trace_ray<4, true>(g, s, f, rx, rz, min_cell_km(g), slab.data(), flags, nsteps, nullptr, sub, sums);
            if (sub == 3) { fl0 = *flags; st0 = *nsteps; std::memcpy(sm0, sums, 8); }
            else if (fl0 != *flags || st0 != *nsteps || std::memcmp(sm0, sums, 8) != 0) return -3;
        }
    }
    for (int b = 0; b < 3; ++b)
        for (int vx = 0; vx < g.nvx + 2; ++vx)
            for (int vz = 0; vz < g.nvz + 2; ++vz)
                fdm3[b * slab_len + (size_t)vx * (g.nvz + 2) + vz] = slab[b * slab_len + (size_t)vz * (g.nvx + 2) + vx];
    return rc;
}

}  // extern "C"
