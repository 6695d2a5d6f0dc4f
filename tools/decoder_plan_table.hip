// decoder_plan_table.hip -- every path-selection decision of the channel decoder (csrc/wave_plan.hpp, csrc/lane_plan.hpp)
// as a table, for every legal sub-channel length and for plain codeword lengths.  No device is touched.  Build and run
// (from the repository root), as tools/lane_plan_check.hip:
//   hipcc -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -Isdrplusplus-dab-radio-plugin_amd/csrc tools/decoder_plan_table.hip -o /tmp/decoder_plan_table && /tmp/decoder_plan_table
// Lines (tests/test_decoder_seams.py reads them and takes every threshold from them):
//   const NAME VALUE
//   dab   BITRATE NSTEPS PATH WAVES LDS SEG_CYCLES N_LANES GROUP GROUP_LDS LANE TILE_LDS     nsteps = 24 b + 6, b = 8 .. 1728 by 8
//   plain 0       NSTEPS ...the same...                                                       nsteps = 38 .. 20 000 by 2
// PATH is what a call takes that leaves the choice to the library at a small batch: rot (viterbi_rot_kernel), wave
// (viterbi_wave_kernel), lane_tile / lane_direct (the lane kernels, traceback through an LDS tile or with direct stores)
// or refused.  WAVES and LDS: codewords per workgroup and dynamic LDS of launch_wave before balanced_lds_bytes (0: the
// wave kernels do not take the length).  SEG_CYCLES, N_LANES: rot_layout (0 for other kernels).  GROUP, GROUP_LDS: the
// small-batch grouped launch takes the length, and its LDS.  LANE: the lane kernels take the length when forced; TILE_LDS:
// the traceback's dynamic LDS for this length alone (0: direct stores).
// The last line is "decoder plan ok" unless a check of the layouts failed.
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

void row(const char *kind, int bitrate, int nsteps) {
    const WaveLaunchPlan p = plan_wave_launch(nsteps);
    const bool lane = lane_supported(nsteps), tile = lane && lane_tile_fits(nsteps);
    const char *path = p.ok ? (p.rot ? "rot" : "wave") : !lane ? "refused" : tile ? "lane_tile" : "lane_direct";
    RotLayout L{};
    if (p.ok && p.rot) {
        L = rot_layout(nsteps);
        const int groups = (nsteps - 6) / 6;
        // the traceback: every phase cycle has a lane, the survivor slots (skewed) end below the decoded bits, the
        // regions follow each other inside the slab, the position table holds the mother bits
        CHECK(L.n_lanes >= 1 && L.n_lanes <= 64 && L.n_lanes * L.seg_cycles >= groups && (L.n_lanes - 1) * L.seg_cycles < groups);
        CHECK(8 * (nsteps + (nsteps - 7) / L.seg_steps) <= L.out6_off);
        CHECK(L.mother_off + 4 * nsteps <= L.out6_off && L.out6_off + groups <= L.zero_off && L.zero_off + 64 <= L.total);
        CHECK(L.total <= p.lds_per_wave && 4 * nsteps <= 65536);
    }
    if (p.ok) CHECK(p.waves >= 1 && p.lds == size_t(p.lds_per_wave) * size_t(p.waves) && p.lds <= size_t(160) * 1024);
    if (p.ok && !p.rot) CHECK(viterbi_wave_lds_bytes(nsteps) <= size_t(p.lds_per_wave) && ((4 * nsteps + 15) & ~15) + 8 * nsteps <= p.lds_per_wave);
    const bool group = wave_group_supported(nsteps);
    if (group) CHECK(p.ok && p.rot && wave_group_lds_bytes(nsteps) == size_t(p.lds_per_wave));
    const size_t tile_lds = tile ? size_t(64) * size_t(((nsteps - 6) >> 5) | 1) * 4 : 0;
    CHECK(tile_lds <= size_t(160) * 1024);
    std::printf("%s %d %d %s %d %zu %d %d %d %zu %d %zu\n", kind, bitrate, nsteps, path, p.ok ? p.waves : 0, p.ok ? p.lds : size_t(0),
                L.seg_cycles, L.n_lanes, int(group), group ? wave_group_lds_bytes(nsteps) : size_t(0), int(lane), tile_lds);
}

}  // namespace

int main() {
    std::printf("const WAVES_PER_WG %d\n", WAVES_PER_WG);
    std::printf("const WAVE_GROUP_MAX %d\n", WAVE_GROUP_MAX);
    std::printf("const HIST_BLOCKS %d\n", HIST_BLOCKS);
    {   // the largest history ring (bytes) that rides in the grouped launch: the rule is one threshold
        size_t lo = 1, hi = size_t(1) << 40;
        CHECK(!wave_history_rides(0) && wave_history_rides(lo) && !wave_history_rides(hi));
        while (hi - lo > 1) {
            const size_t mid = lo + (hi - lo) / 2;
            (wave_history_rides(mid) ? lo : hi) = mid;
        }
        std::printf("const RIDE_MAX_BYTES %zu\n", lo);
    }
    for (int b = 8; b <= 1728; b += 8) row("dab", b, 24 * b + 6);
    for (int n = 38; n <= 20000; n += 2) row("plain", 0, n);
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("decoder plan ok\n");
    return 0;
}
