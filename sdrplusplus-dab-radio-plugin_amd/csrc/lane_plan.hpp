// lane_plan.hpp -- what a launch of the lane Viterbi (viterbi_lane_kernels.hip) decides on the host before it touches the
// device, stated once: where an item's soft bits come from, whether it can take the fused forward pass, how much scratch a
// list needs, and the entries of one launch.  Plain C++ on values -- no HIP runtime call, no pointer is followed -- so the
// API layer (dabgpu_decode_api.hip) asks the same questions the launcher does, and tools/lane_plan_check.hip runs all of
// it under the host sanitizers.  Internal to libdabgpu.
#pragma once
#include <algorithm>
#include <vector>

#include "soft_source.hpp"

namespace dabk {

// does the traceback's output tile ([64][words | 1] dwords) fit into LDS?
__host__ __device__ __forceinline__ bool lane_tile_fits(int nsteps) {
    return size_t(64) * size_t(((nsteps - 6) >> 5) | 1) * 4 <= size_t(150) * 1024;
}

// One entry of a launch, as lane_forward_grouped_kernel / lane_traceback_grouped_kernel take it by value.
struct LaneEntry {
    SoftSrc src;
    const int32_t *desc, *tiles;
    const uint8_t *prbs;
    uint8_t *out;
    uint8_t *crc_ok;          // FIC entry: CRC flag per FIB; nullptr otherwise
    uint2 *dec;
    int nsteps, n_codewords, first_group, groups;
};

inline SoftSrc lane_item_src(const LaneItem &it) {
    const int n = int(it.codewords());
    if (it.kind == LaneItem::FIC) return make_fic_src(it.args.soft, it.args.soft_stride, n);
    if (it.kind == LaneItem::PLAIN) return make_plain_src(it.args.soft, it.code.n_punct, n);
    return make_msc_src(it.args);
}

// every row of the source starts on a 16-byte boundary: the kernels stage it with 16-byte loads
inline bool lane_src_vec16(const SoftSrc &s) {
    return ((reinterpret_cast<uintptr_t>(s.soft) | s.stride | size_t(s.base_off) | size_t(s.per_cif)) & 15) == 0;
}

// Can the item take the fused forward pass (no lane_prep_kernel)?  Whole groups of 64 codewords inside a stream (a source
// that is one stream has no boundary to straddle), 16-byte aligned soft bits, stride and start bit, 16-byte aligned history
// rows, a 4-byte aligned output, the fused tables, a length the lane kernels take.
inline bool lane_item_fusable(const LaneItem &it) {
    const SoftSrc s = lane_item_src(it);
    const bool one_stream = size_t(s.cifs_per_stream) > it.codewords();
    return (one_stream || s.cifs_per_stream % 64 == 0) && lane_src_vec16(s) &&
           (!s.hist || ((reinterpret_cast<uintptr_t>(s.hist) | size_t(s.nbits)) & 15) == 0) &&
           (reinterpret_cast<uintptr_t>(it.args.out) & 3) == 0 && it.tables.fused_desc && it.tables.fused_tiles &&
           lane_supported(it.code.nsteps);
}

inline size_t lane_item_groups(const LaneItem &it) { return (it.codewords() + 63) / 64; }

// Scratch of one item: the survivor words, 8 bytes per codeword-step; an item that goes through lane_prep_kernel
// (`unfused`, or not fusable) also the depunctured soft words in front of them, 4 more.
inline size_t lane_item_scratch_bytes(const LaneItem &it, bool unfused) {
    return lane_item_groups(it) * 64 * size_t(it.code.nsteps) * ((unfused || !lane_item_fusable(it)) ? 12 : 8);
}
inline size_t lane_scratch_bytes(const LaneItem *items, int n, bool unfused) {
    size_t total = 512;
    for (int i = 0; i < n; i++) total += lane_item_scratch_bytes(items[i], unfused);
    return total;
}

// The entries of ONE launch over items[0..n), in dispatch order.
struct LanePlan {
    std::vector<LaneEntry> e;
    std::vector<int> item;    // entry k decodes items[item[k]]
    bool fused;               // every entry takes the fused forward pass
    int total_groups;
    int tile_nwords;          // output words of the longest codeword whose traceback tile fits into LDS (0: none does)
    int prio_nsteps;          // forward waves of entries at least this long get the issue slots first (0: nobody)
    char *scratch_end;        // first byte behind the entries' slices of the scratch
};

// longest_first: workgroups start in grid order, so the longest codewords go first and the short ones fill the end of the
//   launch (a long wave started last would run on alone).  Every entry works on buffers of its own: the order changes no result.
// scratch: where the first entry's slice begins (an entry that is not fused keeps its soft words in front of its survivors).
// resident_groups: how many forward waves the chip holds at once (two per SIMD).  Codeword lengths differ between entries;
//   when the whole launch is resident the longest entry's waves would run alone, at a single wave's issue rate, for the end
//   of the launch, so they get the issue slots first.  Launches with more waves than the chip holds balance themselves by
//   dispatch order, and there a priority only hurt: prio_nsteps is 0 for them.
inline void plan_lane_launch(const LaneItem *items, int n, bool unfused, bool longest_first, char *scratch, int resident_groups,
                             LanePlan &plan) {
    plan.e.assign(size_t(n), LaneEntry{});
    plan.item.resize(size_t(n));
    for (int i = 0; i < n; i++) plan.item[size_t(i)] = i;
    if (longest_first)
        std::stable_sort(plan.item.begin(), plan.item.end(), [&](int a, int b) { return items[a].code.nsteps > items[b].code.nsteps; });
    plan.fused = !unfused;
    plan.total_groups = plan.tile_nwords = 0;
    int longest = 0, shortest = 0x7fffffff;
    for (int k = 0; k < n; k++) {
        const LaneItem &it = items[plan.item[size_t(k)]];
        LaneEntry &e = plan.e[size_t(k)];
        const bool fused = !unfused && lane_item_fusable(it);
        plan.fused = plan.fused && fused;
        e.src = lane_item_src(it);
        e.desc = it.tables.fused_desc;
        e.tiles = it.tables.fused_tiles;
        e.prbs = it.code.prbs_bytes;
        e.out = it.args.out;
        e.crc_ok = it.kind == LaneItem::FIC ? it.crc_ok : nullptr;
        e.nsteps = it.code.nsteps;
        e.n_codewords = int(it.codewords());
        e.first_group = plan.total_groups;
        e.groups = int(lane_item_groups(it));
        const size_t words = size_t(e.groups) * 64 * size_t(e.nsteps);
        e.dec = reinterpret_cast<uint2 *>(scratch + (fused ? 0 : words * 4));
        scratch += words * (fused ? 8 : 12);
        plan.total_groups += e.groups;
        if (lane_tile_fits(e.nsteps)) plan.tile_nwords = std::max(plan.tile_nwords, (e.nsteps - 6) >> 5);
        longest = std::max(longest, e.nsteps);
        shortest = std::min(shortest, e.nsteps);
    }
    plan.prio_nsteps = (plan.total_groups <= resident_groups && longest > shortest) ? longest : 0;
    plan.scratch_end = scratch;
}

}  // namespace dabk
