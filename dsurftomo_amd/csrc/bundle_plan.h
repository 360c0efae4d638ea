// How a launch is bundled (bundle_kernel.hip: the units of one source -- its periods -- side by side in one workgroup): which units share
// a bundle, which bundles run wide or are cut in halves, the launch order, the members per bundle of a call and the field slots.  Host
// arithmetic only, every rule once: the engine gathers the inputs (the memory included), calls these functions, then allocates and uploads.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "source_stage.h"

namespace dsa {

// A source is its coordinates bit for bit.  The pair's order is the order of the sources wherever they are walked (ties of the stable sorts below).
using SourceKey = std::pair<uint32_t, uint32_t>;
inline SourceKey source_key(float scx, float scz)
{
    uint32_t a, b;
    std::memcpy(&a, &scx, 4); std::memcpy(&b, &scz, 4);
    return { a, b };
}

// Launch order: a launch ends with its slowest workgroups, and the rounds of a solve grow with the distance from the source to the
// farthest corner of the grid, so the units with the longest fronts get the lowest workgroup numbers (dispatched first) and the short
// ones fill the tail.  The sort key: minus that distance squared, in nodes.
inline float farness(const GridDesc& g, const SourceDesc& sd)
{
    const float fx = (sd.scx - g.gox) / g.dnx, fz = (sd.scz - g.goz) / g.dnz;
    const float dx = std::max(fx, (float)(g.nnx - 1) - fx), dz = std::max(fz, (float)(g.nnz - 1) - fz);
    return -(dx * dx + dz * dz);
}

inline int bundle_log2(int G) { return G == 16 ? 4 : G == 8 ? 3 : 2; }

// floats of a bundle's field: G members per record (bstride = DSA_BSTRIDE apart) and the shared record behind them
inline size_t bundle_field_floats(int G, size_t nrec, int bstride) { return (size_t)(G * bstride + 1) * nrec; }

// bytes of a bundle field slot: the field, its exception table, its tile records
inline size_t bundle_slot_bytes(int G, size_t nrec_c, int exc_log2cap, size_t lists_c_stride, int bstride)
{
    return bundle_field_floats(G, nrec_c, bstride) * 4 + ((size_t)8 << (exc_log2cap + bundle_log2(G))) + lists_c_stride * 4;
}

// What the bundle field slots take of the room the engine finds for them (Engine::bundle_room)
constexpr double kBundleShare = 0.7;
inline size_t bundle_share(size_t room) { return (size_t)(kBundleShare * (double)room); }

// The options of a call that decide its bundles (engine.h: bundle_opt, bundle_mpl, bundle_tail_opt, bundle_order_opt), and `threads`:
// what Engine::bundle_threads() returns; threads_auto: option bundle_threads is 0
struct BundleOptions {
    int bundle = 1, mpl = 0, tail = 1, order = 0;
    int threads = 256;
    bool threads_auto = true;
};

// bundles the chip holds at a time: one workgroup of 512 threads per CU, two of 256 (four members per lane: 204 VGPRs) or three (two
// members per lane: 168 VGPRs, round 4)
inline size_t bundles_resident(int G, int mpl, int threads)
{
#ifdef DSA_BUNDLE_WAVES          // (probe builds: bundle_kernel.hip compiled for that many waves per SIMD whatever the members per lane)
    if (threads == 256) return (size_t)256 * DSA_BUNDLE_WAVES;
#endif
    // (bundle_kernel.hip: DSA_BUNDLE_OCC -- three workgroups of 256 threads per CU with two members per lane and for bundles of 16)
    return (size_t)256 * (threads >= 512 ? 1 : (mpl == 2 || G == 16) ? 3 : 2);
}

// Members per lane of a launch of nb bundles of G: the option, or 16 members four per lane; 8 and 4 members two per lane (three workgroups
// per CU) when the launch holds more than the 512 bundles that two per CU take, else four
inline int bundle_mpl_of(const BundleOptions& o, int G, long nb)
{
    if (o.mpl) return o.mpl;
    if (o.threads != 256 || G == 16) return 4;
    return nb > 512 ? 2 : 4;
}

// The c units of a source under bundle size G: c / G whole bundles and one more of the remainder -- unless that is a single unit, which stays solo
struct SourcePieces { int whole, rest; };
inline SourcePieces source_pieces(int c, int G) { return { c / G, c % G >= 2 ? c % G : 0 }; }

struct Census { long bundles = 0, covered = 0; };
inline Census bundle_census(const std::vector<int>& counts, int G)
{
    Census s;
    for (int c : counts) { const SourcePieces p = source_pieces(c, G); s.bundles += p.whole + (p.rest > 0); s.covered += (long)p.whole * G + p.rest; }
    return s;
}

// units per source of a unit list, sources in key order
inline std::vector<int> source_unit_counts(const SourceDesc* src, size_t n)
{
    std::map<SourceKey, int> count;
    for (size_t u = 0; u < n; ++u) ++count[source_key(src[u].scx, src[u].scz)];
    std::vector<int> c;
    for (const auto& kv : count) c.push_back(kv.second);
    return c;
}

// ---- the layout of one launch ---------------------------------------------------------------------
// Units are chunk-local.  Solo units keep the launch ranks 0 .. nsolo-1 (and the field slots those select), longest fronts first; the
// members of the bundles follow, bundle by bundle: the whole bundles (longest first), then the tail.
struct BundleLayout {
    std::vector<std::vector<int>> whole, tail;      // member lists of the first group and of the second (its own stream)
    int bundles_a = 0, bundles_b = 0, bundle_Gb = 0;
    int mpl_now = 4, mpl_b = 2, threads_b = 256;    // members per lane of the two groups, workgroup size of the second
    std::vector<int> member_flag;                   // 0 solo, 1 member, 2 member of a wide tail bundle (its own causal window)
    std::vector<int> launch_rank;
    int nsolo = 0;
};

// G = 0: no bundles, the ranks of a unit-by-unit launch.
inline BundleLayout plan_layout(const SourceDesc* src, int n, const GridDesc& g, int G, const BundleOptions& o)
{
    BundleLayout L;
    L.member_flag.assign((size_t)n, 0);
    L.launch_rank.assign((size_t)n, 0);
    L.threads_b = o.threads;
    L.mpl_b = o.mpl ? o.mpl : 2;
    struct Piece { float far; std::vector<int> mem; };
    std::vector<Piece> pieces, tail;
    if (G > 0) {
        std::map<SourceKey, std::vector<int>> groups;
        for (int u = 0; u < n; ++u) groups[source_key(src[u].scx, src[u].scz)].push_back(u);
        for (const auto& kv : groups) {
            const std::vector<int>& v = kv.second;
            const SourcePieces p = source_pieces((int)v.size(), G);
            for (int k = 0; k < p.whole + (p.rest > 0); ++k) {
                const auto at = v.begin() + (long)k * G;
                pieces.push_back({ farness(g, src[*at]), std::vector<int>(at, at + (k < p.whole ? G : p.rest)) });
                for (int u : pieces.back().mem) L.member_flag[(size_t)u] = 1;
            }
        }
        std::stable_sort(pieces.begin(), pieces.end(), [](const Piece& x, const Piece& y) { return x.far < y.far; });
    }
    std::vector<std::pair<float, int>> solo;
    for (int u = 0; u < n; ++u) if (!L.member_flag[(size_t)u]) solo.push_back({ farness(g, src[u]), u });
    std::stable_sort(solo.begin(), solo.end());
    L.nsolo = (int)solo.size();
    for (int r = 0; r < L.nsolo; ++r) L.launch_rank[(size_t)solo[(size_t)r].second] = r;
    const int nb = (int)pieces.size();
    L.bundles_a = nb;
    if (nb == 0) return L;
    // Members per lane and workgroups per CU (round 4, profiles/r04_bundle_occupancy.log; bundle_mpl_of, bundle_kernel.hip: DSA_BUNDLE_OCC):
    // bundles of 16 run three workgroups per CU (768 resident), bundles of 8 / 4 too when the launch has more than 512 of them.  A bundle
    // takes longer with two neighbours on its CU than with one (768 bundles of 16: 241 ms; 500: 210; 250: 190), but a CU finishes more of
    // them per second.  The catch is a last generation that is nearly empty -- 1 000 bundles = 768 + 232 -- so, automatic mode, between 768
    // and 1 500 bundles: the first 768 (the longest) as they are and the REST CUT IN HALVES -- bundles of G / 2, two members per lane, on a
    // second stream, which fill the CUs the first launch frees one by one (1 000 sources x 16 periods: 383 ms against ~430 uncut).
    const int res3 = 768;
    L.mpl_now = bundle_mpl_of(o, G, nb);
    const bool second = o.mpl == 0 && o.threads == 256 && o.bundle == 1 && G >= 8 && nb > res3 && nb < 1500;
    if (second && o.tail == 1 && nb - res3 <= 256) {
        // Round 5, option bundle_tail = 1: the bundles beyond the first generation stay WHOLE and run 768 threads wide on the second stream, a CU
        // each as the first generation's workgroups leave (a bundle of 16 alone on a CU: 106 ms wide against 190 with 256 threads)
        tail.assign(pieces.begin() + res3, pieces.end());
        pieces.resize((size_t)res3);
        for (const Piece& pc : tail) for (int u : pc.mem) L.member_flag[(size_t)u] = 2;      // (their own causal window: bundle_window_tail)
        L.bundle_Gb = G;
        L.mpl_b = 4; L.threads_b = 768;
    } else if (second) {
        std::vector<Piece> keep(pieces.begin(), pieces.begin() + res3);
        for (size_t k = (size_t)res3; k < pieces.size(); ++k) {
            const std::vector<int>& v = pieces[k].mem;
            if ((int)v.size() >= G / 2 + 2) {
                tail.push_back({ pieces[k].far, std::vector<int>(v.begin(), v.begin() + G / 2) });
                tail.push_back({ pieces[k].far, std::vector<int>(v.begin() + G / 2, v.end()) });
            } else keep.push_back(pieces[k]);
        }
        pieces.swap(keep);
        L.bundle_Gb = G / 2;
    }
    L.bundles_a = (int)pieces.size(); L.bundles_b = (int)tail.size();
    if (o.order == 1 && L.bundles_b > 0 && L.threads_b == 768 && (int)pieces.size() == res3) {
        // Round 6, option bundle_order (A/B switch, default 0; other values change nothing): which bundles share a CU.  If the first generation's 768
        // workgroups went out round robin -- k, k + 256 and k + 512 on one CU -- "longest first" would give every CU a long, a middle and a short
        // bundle, and the wide tail, whose workgroups need whole CUs, could only start when the generation is all but over; position p holding rank
        // 3 (p mod 256) + p / 256 would then put bundles of similar length on one CU.  Measured (profiles/r06_ab_bundle_order.log): 350.4 ms against
        // 342.0 -- the dispatcher fills a CU with CONSECUTIVE workgroups, "longest first" already is the grouped order (the rocprof trace shows the
        // tail starting with the generation and ending 84 ms after it), and the permutation un-groups it.
        std::vector<Piece> perm((size_t)res3);
        const int ncu = res3 / 3;
        for (int p = 0; p < res3; ++p) perm[(size_t)p] = pieces[(size_t)(3 * (p % ncu) + p / ncu)];
        pieces.swap(perm);
    }
    int rank = L.nsolo;
    for (std::vector<Piece>* grp : { &pieces, &tail })
        for (Piece& pc : *grp) {
            for (int u : pc.mem) L.launch_rank[(size_t)u] = rank++;
            (grp == &pieces ? L.whole : L.tail).push_back(std::move(pc.mem));
        }
    return L;
}

// ---- the choice of size -----------------------------------------------------------------------------
// bundles are an option of the call, and the automatic mode stays unit by unit after a bundle of the current maps ran out of rounds
inline bool bundles_possible(const BundleOptions& o, bool bundles_failed) { return o.bundle != 0 && !(bundles_failed && o.bundle == 1); }

struct SizeInputs {
    int nnx = 0, nnz = 0, nmaps = 0, exc_log2cap = 0;
    size_t nrec_c = 0, lists_c_stride = 0;
    int step = 0, bstride = 1;     // units per launch; DSA_BSTRIDE
    size_t room = 0;               // bytes the bundle slots may share (Engine::bundle_room)
    bool bundles_failed = false;
};
struct SizeChoice { int G; bool wide; long solo_units; };

// Members per bundle for a call: the option, or (automatic) the largest of 16 / 8 / 4 that still gives the chip enough workgroups
// and whose field slots fit the memory; 0 = no bundles.  `counts`: units per source.  wide: the bundles run 768 threads wide on a
// small launch (a CU per bundle).  solo_units: the units that stay outside bundles.  (o.threads: Engine::bundle_threads() of a call that is not wide.)
inline SizeChoice choose_bundle_size(const std::vector<int>& counts, const SizeInputs& in, const BundleOptions& o)
{
    long total = 0;
    for (int c : counts) total += c;
    SizeChoice pick = { 0, false, total };
    if (!bundles_possible(o, in.bundles_failed) || total == 0) return pick;
    const size_t nrec_c = in.nrec_c;
    auto fits = [&](int G) {
        if ((unsigned long long)nrec_c * (unsigned long long)G * 4ull * (unsigned long long)in.bstride >= (1ull << 32)) return false;          // 32-bit byte offsets inside a bundle field
        if (nrec_c >= ((size_t)1 << 27)) return false;                                                          // (record indices share the ready-list word with the far-load code, and -- shifted by four -- the tie candidates' word with a flag bit)
        if ((unsigned long long)nrec_c * (unsigned long long)G >= (1ull << 30)) return false;                // exception keys
        if ((unsigned long long)nrec_c * (unsigned long long)in.nmaps * 4ull >= (1ull << 32)) return false;      // ... and inside the member-minor slowness
        const long nb = std::min<long>(bundle_census(counts, G).bundles, (long)in.step);
        const size_t want = (size_t)std::min<long>(std::max<long>(nb, 1), (long)(bundles_resident(G, bundle_mpl_of(o, G, nb), o.threads) * 9 / 8));      // (bundles resident at a time, and a few more)
        return want * bundle_slot_bytes(G, nrec_c, in.exc_log2cap, in.lists_c_stride, in.bstride) + (size_t)in.nmaps * nrec_c * 4 < bundle_share(in.room);      // (what size_bundle_slots allows itself)
    };
    if (o.bundle == 4 || o.bundle == 8 || o.bundle == 16) {
        const Census s = bundle_census(counts, o.bundle);
        if (fits(o.bundle) && s.bundles > 0) pick = { o.bundle, false, total - s.covered };
        return pick;
    }
    // automatic: a bundle is one workgroup where its members would have been G, so it pays only while the bundles still fill the chip.
    // The best of the estimates below wins: a launch-time model from times measured at 1025^2 (only the ratios decide; they hold from 129^2
    // to 4097^2: profiles/r03_bundle_sizes.log, r04_bundle_occupancy.log).  Beyond 1500 nodes per side the bundle kernel runs wide (768
    // threads, one workgroup per CU: a third as many bundles fill the chip); round 3's table of rates serves there.
    // Grid size: round 3 kept grids below 400 nodes per side unit by unit.  With round 4's kernel the bundles win there too when the call
    // has the sources (16 periods x 1000 sources: 385^2 66 k -> 141 k solves/s, 257^2 119 k -> 200 k, 129^2 232 k -> 288 k; 200 sources at
    // 257^2: 101 k -> 116 k; profiles/r04_bundle_occupancy.log), so the floor is 120 nodes per side.
    if (std::min(in.nnx, in.nnz) < 120) return pick;
    // ... but only for launches that fill the chip: below 400 nodes per side a solve is a few hundred short rounds, many unit-by-unit
    // workgroups share a CU, and a handful of bundles -- the Taipei example: 34 bundles for 449 units at 137^2 -- take longer than the
    // units by themselves (coarse solves 2.9 -> 7.0 ms); there a size needs 384 bundles of at least 8 members and the wide variant stays off
    const bool small_grid = std::min(in.nnx, in.nnz) < 400;
    const double n_units = (double)std::min<size_t>((size_t)total, (size_t)in.step);
    const double solo_rate = 10.0 * std::min(1.0, n_units / 1100.0);          // k solves/s
    double best = solo_rate * 1.05;
    const int sizes[3] = { 16, 8, 4 };
    // Round 4 (256-thread kernel): a launch's time from the measured time of ONE bundle at one / two / three workgroups per CU at 1025^2 (ms;
    // the ratios hold at other sizes: only ratios decide) -- a bundle takes what its rounds take, whatever shares the chip with it, so a
    // launch of nb <= 768 bundles takes one bundle's time at that occupancy, a longer one whole generations plus a last partial one that
    // costs at least 45 % of a generation (profiles/r04_bundle_occupancy.log); between 768 and 1 500 bundles plan_layout cuts the last
    // ones in halves (1 000 bundles of 16: 383 ms)
    const double t_one[3][3] = { { 189.5, 210.0, 241.0 }, { 130.8, 151.7, 187.2 }, { 104.8, 125.4, 164.3 } };
    const double rate512[3] = { 24.5, 20.4, 15.5 };                             // (large grids, one wide workgroup per CU: round 3's table; only the ratios decide)
    const double t_wide[3] = { 106.0, 77.0, 69.0 };                             // (768 threads at 1025^2, a CU per bundle: ms of one bundle of 16 / 8 / 4)
    for (int k = 0; k < 3; ++k) {
        const int G = sizes[k];
        const Census s = bundle_census(counts, G);
        long nb = s.bundles;
        const long covered = s.covered;
        if (nb == 0 || !fits(G)) continue;
        nb = std::min<long>(nb, (long)in.step);
        if (small_grid && (nb < 384 || G < 8)) continue;      // (bundles of 4 lose there: 100 sources x 16 at 257^2 73 k against 93 k unit by unit)
        const double frac = (double)covered / (double)total;                         // units that end up in bundles ...
        const double fill = (double)covered / ((double)nb * G);                       // ... and how full the bundles are
        double est;
        if (o.threads >= 512) est = frac * rate512[k] * fill * std::min(1.0, (double)nb / 280.0) + (1.0 - frac) * solo_rate;
        else {
            const double occ = (double)nb / 256.0;
            double ms;
            if (occ <= 1.0) ms = t_one[k][0];
            else if (occ <= 2.0) ms = t_one[k][0] + (t_one[k][1] - t_one[k][0]) * (occ - 1.0);
            else if (occ <= 3.0) ms = t_one[k][1] + (t_one[k][2] - t_one[k][1]) * (occ - 2.0);
            else {
                const double gens = std::floor((double)nb / 768.0), rem = (double)nb / 768.0 - gens;
                ms = t_one[k][2] * (gens + (rem > 0.0 ? 0.45 + 0.55 * rem : 0.0));
                if (G >= 8 && nb > 768 && nb < 1500) ms *= 0.98;                    // (the halved last bundles)
                // (round 5) at most 256 bundles beyond the first generation: whole, 768 threads wide, a CU each as the first generation leaves
                // (1 000 bundles of 16: 325 ms against 368 with halves, profiles/r05_ab_bundle_kernel.log)
                if (o.tail == 1 && G >= 8 && o.mpl == 0 && nb > 768 && nb <= 1024) ms = t_one[k][2] + 0.8 * (t_wide[k] + 12.0 * (double)(nb - 768) / 256.0);
            }
            // k solves/s (= units per ms) of the whole launch: the bundles in `ms` (a little less when they are not full: idle member lanes save no trips), the rest unit by unit behind them
            const double units_s = n_units * (1.0 - frac);
            est = n_units / (ms * (0.65 + 0.35 * fill) + units_s / std::max(solo_rate, 1e-9));
        }
        bool wide = false;
        if (o.threads_auto && o.threads == 256 && nb <= 256 && !small_grid) {
            // ... or a CU per bundle, 768 threads wide (one bundle's time at that width, nearly flat in the number of bundles)
            const double ms_w = t_wide[k] + 12.0 * (double)nb / 256.0;
            const double est_w = n_units / (ms_w * (0.65 + 0.35 * fill) + n_units * (1.0 - frac) / std::max(solo_rate, 1e-9));
            if (est_w > est) { est = est_w; wide = true; }
        }
        if (est > best) { best = est; pick = { G, wide, total - covered }; }
    }
    return pick;
}

// ---- field-slot sizing --------------------------------------------------------------------------------
// Field slots per group of bundles: one per bundle, or -- more bundles than the chip holds at a time -- as many as can be resident and a
// few more (option bundle_pool: that many); a bundle claims a free one when it starts (FimBundle::slot_busy).  Two groups halve the room.
struct SlotGroup { int G = 0, count = 0, slots = 0, xlog = 0; size_t b_stride = 0, b_off = 0, exc_off = 0, slot0 = 0; };
struct SlotPlan {
    SlotGroup gr[2];
    size_t b_total = 0, exc_total = 0, slots_total = 0;      // floats of all fields, exception entries, slots
    size_t no_room_for = 0;                                  // != 0: the room does not hold one slot of that many bytes
};

// threads_a: the first group's workgroup size (Engine::bundle_threads()); `room` as in SizeInputs
inline SlotPlan size_bundle_slots(const BundleLayout& L, int G, int threads_a, size_t nrec_c, int exc_log2cap, size_t lists_c_stride, int bstride,
                                  int bundle_pool_opt, size_t room)
{
    SlotPlan sp;
    sp.gr[0].G = G; sp.gr[0].count = L.bundles_a;
    sp.gr[1].G = L.bundle_Gb; sp.gr[1].count = L.bundles_b;
    for (int q = 0; q < 2; ++q) {
        SlotGroup& r = sp.gr[q];
        if (r.count == 0) continue;
        r.xlog = exc_log2cap + bundle_log2(r.G);
        r.b_stride = bundle_field_floats(r.G, nrec_c, bstride);
        const size_t slot_b = bundle_slot_bytes(r.G, nrec_c, exc_log2cap, lists_c_stride, bstride);
        const size_t fit = bundle_share(room) / slot_b / (L.bundles_b ? 2 : 1);
        if (fit < 1) { sp.no_room_for = slot_b; return sp; }
        const size_t resident = bundles_resident(r.G, q == 0 ? L.mpl_now : L.mpl_b, q == 0 ? threads_a : L.threads_b);
        r.slots = (int)std::min<size_t>({ (size_t)r.count, (size_t)(bundle_pool_opt > 0 ? bundle_pool_opt : (int)(resident + resident / 8)), fit });
        r.b_off = sp.b_total; r.exc_off = sp.exc_total; r.slot0 = sp.slots_total;
        sp.b_total += (size_t)r.slots * r.b_stride; sp.exc_total += (size_t)r.slots << r.xlog; sp.slots_total += (size_t)r.slots;
    }
    return sp;
}

}  // namespace dsa
