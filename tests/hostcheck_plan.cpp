// TEST HARNESS (not product): the bundle planning rules of dsurftomo_amd/csrc/bundle_plan.h behind a C interface, for
// tests/test_hostcheck_plan.py.  Host arithmetic only; a library of its own so that the other harnesses stay as they are.
#include <cstdint>
#include <vector>

#include "../dsurftomo_amd/csrc/bundle_plan.h"

using namespace dsa;

namespace {

// opt: bundle, bundle_members_per_lane, bundle_tail, bundle_order, threads (Engine::bundle_threads()), option bundle_threads is 0
BundleOptions options(const int* opt)
{
    BundleOptions o;
    o.bundle = opt[0]; o.mpl = opt[1]; o.tail = opt[2]; o.order = opt[3]; o.threads = opt[4]; o.threads_auto = opt[5] != 0;
    return o;
}

}  // namespace

extern "C" {

int hcp_bundle_log2(int G) { return bundle_log2(G); }

long long hcp_slot_bytes(int G, long long nrec_c, int exc_log2cap, long long lists_c_stride, int bstride)
{
    return (long long)bundle_slot_bytes(G, (size_t)nrec_c, exc_log2cap, (size_t)lists_c_stride, bstride);
}

// 1 when source a orders before source b
int hcp_source_before(float ax, float az, float bx, float bz) { return source_key(ax, az) < source_key(bx, bz); }

float hcp_farness(int nnx, int nnz, float gox, float goz, float dnx, float dnz, float scx, float scz)
{
    GridDesc g{}; g.nnx = nnx; g.nnz = nnz; g.gox = gox; g.goz = goz; g.dnx = dnx; g.dnz = dnz;
    SourceDesc s{}; s.scx = scx; s.scz = scz;
    return farness(g, s);
}

// out: bundles, covered
void hcp_census(const int* counts, int nsrc, int G, long long* out)
{
    const Census s = bundle_census(std::vector<int>(counts, counts + nsrc), G);
    out[0] = s.bundles; out[1] = s.covered;
}

// The layout of one launch of n units.  member_flag, launch_rank, bundle_of (the unit's bundle in launch order, the tail's behind the
// whole ones; -1 solo) and place_of (its place in that bundle's member list): n each.
// scal: bundles_a, bundles_b, bundle_Gb, mpl_now, mpl_b, threads_b, nsolo
void hcp_layout(int nnx, int nnz, float gox, float goz, float dnx, float dnz, int n, const float* scx, const float* scz, int G, const int* opt,
                int* member_flag, int* launch_rank, int* bundle_of, int* place_of, int* scal)
{
    GridDesc g{}; g.nnx = nnx; g.nnz = nnz; g.gox = gox; g.goz = goz; g.dnx = dnx; g.dnz = dnz;
    std::vector<SourceDesc> src((size_t)n, SourceDesc{});
    for (int u = 0; u < n; ++u) { src[(size_t)u].scx = scx[u]; src[(size_t)u].scz = scz[u]; }
    const BundleLayout L = plan_layout(src.data(), n, g, G, options(opt));
    for (int u = 0; u < n; ++u) { member_flag[u] = L.member_flag[(size_t)u]; launch_rank[u] = L.launch_rank[(size_t)u]; bundle_of[u] = -1; place_of[u] = -1; }
    int k = 0;
    for (const auto* grp : { &L.whole, &L.tail })
        for (const std::vector<int>& mem : *grp) {
            for (size_t m = 0; m < mem.size(); ++m) { bundle_of[mem[m]] = k; place_of[mem[m]] = (int)m; }
            ++k;
        }
    const int s[7] = { L.bundles_a, L.bundles_b, L.bundle_Gb, L.mpl_now, L.mpl_b, L.threads_b, L.nsolo };
    for (int q = 0; q < 7; ++q) scal[q] = s[q];
    if ((int)L.whole.size() != L.bundles_a || (int)L.tail.size() != L.bundles_b) scal[0] = -1;
}

// dims: nnx, nnz, nmaps, exc_log2cap, step, bstride, bundles_failed.  out: G, wide, solo_units
void hcp_choose(const int* counts, int nsrc, const int* dims, long long nrec_c, long long lists_c_stride, long long room, const int* opt, long long* out)
{
    SizeInputs in;
    in.nnx = dims[0]; in.nnz = dims[1]; in.nmaps = dims[2]; in.exc_log2cap = dims[3]; in.step = dims[4]; in.bstride = dims[5]; in.bundles_failed = dims[6] != 0;
    in.nrec_c = (size_t)nrec_c; in.lists_c_stride = (size_t)lists_c_stride; in.room = (size_t)room;
    const SizeChoice c = choose_bundle_size(std::vector<int>(counts, counts + nsrc), in, options(opt));
    out[0] = c.G; out[1] = c.wide; out[2] = c.solo_units;
}

// lay: bundles_a, bundles_b, G, bundle_Gb, mpl_now, mpl_b, threads_a, threads_b.  groups: per group G, count, slots, xlog, b_stride, b_off,
// exc_off, slot0.  totals: floats of the fields, exception entries, slots, bytes of the slot that found no room (0: none)
void hcp_slots(const int* lay, long long nrec_c, int exc_log2cap, long long lists_c_stride, int bstride, int bundle_pool, long long room,
               long long* groups, long long* totals)
{
    BundleLayout L;
    L.bundles_a = lay[0]; L.bundles_b = lay[1]; L.bundle_Gb = lay[3]; L.mpl_now = lay[4]; L.mpl_b = lay[5]; L.threads_b = lay[7];
    const SlotPlan sp = size_bundle_slots(L, lay[2], lay[6], (size_t)nrec_c, exc_log2cap, (size_t)lists_c_stride, bstride, bundle_pool, (size_t)room);
    for (int q = 0; q < 2; ++q) {
        const SlotGroup& r = sp.gr[q];
        const long long v[8] = { r.G, r.count, r.slots, r.xlog, (long long)r.b_stride, (long long)r.b_off, (long long)r.exc_off, (long long)r.slot0 };
        for (int k = 0; k < 8; ++k) groups[q * 8 + k] = v[k];
    }
    totals[0] = (long long)sp.b_total; totals[1] = (long long)sp.exc_total; totals[2] = (long long)sp.slots_total; totals[3] = (long long)sp.no_room_for;
}

}  // extern "C"
