// lane_plan_check.hip -- the lane decoder's host-side planning (csrc/lane_plan.hpp: source form, fusable predicate, scratch
// size, entry builder) run on its own, for the host sanitizers.  No device is touched and no pointer is followed: the
// buffers are made-up addresses.  Build and run (from the repository root):
//   hipcc -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -Isdrplusplus-dab-radio-plugin_amd/csrc tools/lane_plan_check.hip -o /tmp/lane_plan_check && /tmp/lane_plan_check
// It walks the item lists the GPU tests send (tests/test_gpu_lane.py, tests/test_ensembles.py, tests/test_long_codewords.py):
// the empty list, one entry, 16, 17 and 33 entries in packs of 16 and through the table, plain codewords and the FIC at the
// group edges, aligned and not, a sub-channel with history in whole groups and not, and a codeword whose traceback tile does
// not fit into LDS -- and checks what the launcher relies on.
#include <cstdio>
#include <cstdlib>

#include "lane_plan.hpp"

using namespace dabk;

namespace {

int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) { std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

template <class T>
T *fake(uintptr_t a) { return reinterpret_cast<T *>(a); }

constexpr uintptr_t SOFT = 0x7f0000000000u, OUT = 0x7f1000000000u, HIST = 0x7f2000000000u, SCRATCH = 0x7f4000000000u;
constexpr int PACK = 16, RESIDENT = 2 * 4 * 256;

LaneItem item(LaneItem::Kind kind, int nsteps, int n_punct) {
    LaneItem it{};
    it.kind = kind;
    it.code.nsteps = nsteps;
    it.code.n_punct = n_punct;
    it.tables = LaneTables{fake<const int32_t>(0x1000), fake<const int32_t>(0x2000), fake<const int32_t>(0x3000)};
    it.args.out = fake<uint8_t>(OUT);
    return it;
}
LaneItem plain(int nsteps, int n_punct, int n, uintptr_t soft = SOFT) {
    LaneItem it = item(LaneItem::PLAIN, nsteps, n_punct);
    it.args.soft = fake<const int8_t>(soft);
    it.n_plain = n;
    return it;
}
LaneItem fic(int n_frames, size_t stride, uintptr_t soft = SOFT) {
    LaneItem it = item(LaneItem::FIC, 774, 2304);
    it.args.soft = fake<const int8_t>(soft);
    it.args.soft_stride = stride;
    it.args.n_streams = 1;
    it.args.frames_per_stream = n_frames;
    it.crc_ok = fake<uint8_t>(OUT + 0x100000);
    return it;
}
LaneItem sub(int nsteps, int start_cu, int length_cu, int n_streams, int frames, bool history, int k = 0) {
    LaneItem it = item(LaneItem::SUBCHANNEL, nsteps, length_cu * 64);
    it.args = MscArgs{fake<const int8_t>(SOFT), 230400, n_streams, frames, start_cu * 64, length_cu * 64,
                      history ? fake<const int8_t>(HIST + uintptr_t(k) * 0x100000) : nullptr,
                      history ? fake<int8_t>(HIST + 0x80000000u + uintptr_t(k) * 0x100000) : nullptr, fake<uint8_t>(OUT + uintptr_t(k) * 0x1000000)};
    return it;
}

// the launcher's walk over a list: packs of 16 by value, or the whole list through the table
void walk(const std::vector<LaneItem> &items, bool unfused, bool by_table, bool want_fused) {
    const int n = int(items.size());
    const size_t need = lane_scratch_bytes(items.data(), n, unfused);
    char *const base = fake<char>(SCRATCH);
    char *scratch = base;
    LanePlan plan;
    const int per_launch = by_table ? std::max(n, 1) : PACK;
    for (int i0 = 0; i0 < n; i0 += per_launch) {
        const int m = std::min(per_launch, n - i0);
        plan_lane_launch(items.data() + i0, m, unfused, by_table, scratch, RESIDENT, plan);
        CHECK(int(plan.e.size()) == m && int(plan.item.size()) == m);
        CHECK(plan.fused == want_fused);
        int groups = 0, longest = 0, shortest = 0x7fffffff, nwords = 0;
        std::vector<bool> seen(size_t(m), false);
        char *p = scratch;
        for (int k = 0; k < m; k++) {
            const LaneEntry &e = plan.e[size_t(k)];
            CHECK(plan.item[size_t(k)] >= 0 && plan.item[size_t(k)] < m && !seen[size_t(plan.item[size_t(k)])]);
            seen[size_t(plan.item[size_t(k)])] = true;
            const LaneItem &it = items[size_t(i0 + plan.item[size_t(k)])];
            CHECK(e.nsteps == it.code.nsteps && e.n_codewords == int(it.codewords()) && e.out == it.args.out);
            CHECK(e.groups == (e.n_codewords + 63) / 64 && e.first_group == groups);
            CHECK((e.crc_ok != nullptr) == (it.kind == LaneItem::FIC));
            CHECK((e.src.d_force == 15) == (it.kind != LaneItem::SUBCHANNEL));
            if (by_table && k > 0) CHECK(plan.e[size_t(k - 1)].nsteps >= e.nsteps);
            if (!by_table) CHECK(plan.item[size_t(k)] == k);
            // the entry's slice: [soft words |] survivors, inside the scratch, behind the entry before it
            const bool fused = !unfused && lane_item_fusable(it);
            const size_t words = size_t(e.groups) * 64 * size_t(e.nsteps);
            CHECK(reinterpret_cast<char *>(e.dec) == p + (fused ? 0 : words * 4));
            p = reinterpret_cast<char *>(e.dec) + words * 8;
            CHECK(p <= base + need);
            CHECK((reinterpret_cast<uintptr_t>(e.dec) & 7) == 0);
            groups += e.groups;
            longest = std::max(longest, e.nsteps);
            shortest = std::min(shortest, e.nsteps);
            if (lane_tile_fits(e.nsteps)) nwords = std::max(nwords, (e.nsteps - 6) >> 5);
        }
        CHECK(plan.scratch_end == p && plan.total_groups == groups && plan.tile_nwords == nwords);
        CHECK(size_t(64) * size_t(plan.tile_nwords | 1) * 4 <= size_t(160) * 1024);
        CHECK(plan.prio_nsteps == ((groups <= RESIDENT && longest > shortest) ? longest : 0));
        scratch = plan.scratch_end;
    }
    CHECK(scratch + 512 == base + need);
}

}  // namespace

int main() {
    walk({}, false, false, true);
    walk({}, false, true, true);
    // plain codewords, nsteps 198: 784 of 792 mother bits kept (fused), unpunctured (792 is no multiple of 16: prep)
    for (int n : {1, 3, 63, 64, 65, 130}) {
        walk({plain(198, 784, n)}, false, false, true);
        walk({plain(198, 792, n)}, false, false, false);
        walk({plain(198, 784, n)}, true, false, false);
        walk({plain(198, 784, n, SOFT + 1)}, false, false, false);
        // 8 bytes per codeword-step fused, 12 through the prep kernel
        const LaneItem fused = plain(198, 784, n), prep = plain(198, 792, n);
        CHECK(lane_scratch_bytes(&fused, 1, false) == size_t((n + 63) / 64) * 64 * 198 * 8 + 512);
        CHECK(lane_scratch_bytes(&prep, 1, false) == size_t((n + 63) / 64) * 64 * 198 * 12 + 512);
    }
    // the FIC alone
    for (int f : {1, 15, 16, 17}) {
        walk({fic(f, 230400)}, false, false, true);
        walk({fic(f, 9216)}, false, false, true);
        walk({fic(f, 230400, SOFT + 1)}, false, false, false);
        walk({fic(f, 9217)}, false, false, false);
    }
    {   // make_plain_src and make_fic_src are the frame form of contiguous rows
        const SoftSrc s = lane_item_src(plain(198, 792, 130));
        CHECK(s.stride == 4 * 792 && s.per_cif == 792 && s.base_off == 0 && s.nbits == 792 && s.d_force == 15 && !s.hist &&
              s.cifs_per_stream == 130 + 128);
        const SoftSrc f = lane_item_src(fic(17, 9216));
        CHECK(f.stride == 9216 && f.per_cif == 2304 && f.cifs_per_stream == 68 + 128 && f.d_force == 15);
    }
    // one sub-channel, 3 streams with history: whole groups (16 frames) fused, 6 frames through the prep kernel
    walk({sub(1542, 0, 48, 3, 16, true)}, false, false, true);
    walk({sub(1542, 0, 48, 3, 6, true)}, false, false, false);
    walk({sub(1542, 0, 48, 3, 16, true)}, true, false, false);
    {   // each alignment rule on its own
        LaneItem it = sub(1542, 0, 48, 3, 16, true);
        CHECK(lane_item_fusable(it));
        LaneItem a = it; a.args.hist_in = fake<const int8_t>(HIST + 8);
        LaneItem b = it; b.args.out = fake<uint8_t>(OUT + 2);
        LaneItem c = it; c.tables.fused_tiles = nullptr;
        LaneItem d = it; d.args.soft_stride = 230408;
        LaneItem e = it; e.code.nsteps = 1540;
        LaneItem f = it; f.args.start_bit = 8;
        CHECK(!lane_item_fusable(a) && !lane_item_fusable(b) && !lane_item_fusable(c) && !lane_item_fusable(d) && !lane_item_fusable(e) &&
              !lane_item_fusable(f));
    }
    // grouped lists: FIC + sub-channels of different lengths, 2 / 16 / 17 / 30 + 1 / 33 entries, by value and by table
    const int lengths[4] = {1542, 774, 3078, 582};
    for (int n : {2, 16, 17, 31, 33})
        for (bool by_table : {false, true}) {
            std::vector<LaneItem> items{fic(16, 230400)};
            for (int k = 1; k < n; k++) items.push_back(sub(lengths[k & 3], 16 * (k % 50), 16, by_table ? 1 : 2, 16, (k & 1) != 0, k));
            walk(items, false, by_table, true);
        }
    // a launch larger than the chip holds gets no priority; a codeword whose tile does not fit writes directly
    walk({fic(16384, 230400), sub(1542, 0, 48, 1, 16384, false)}, false, false, true);
    CHECK(lane_tile_fits(3078) && !lane_tile_fits(43782) && lane_supported(43782));
    walk({sub(43782, 0, 864, 1, 16, false)}, false, false, true);
    walk({sub(43782, 0, 864, 1, 3, false)}, false, false, false);
    walk({fic(16, 230400), sub(43782, 0, 864, 1, 16, false)}, false, true, true);
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("lane plan ok\n");
    return 0;
}
