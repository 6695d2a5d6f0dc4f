// wave_plan.hpp -- what a launch of the wave-per-codeword Viterbi (viterbi_kernels.hip) decides on the host before it
// touches the device, stated once: which lengths the kernels take, the rot kernel's LDS slab, how many codewords share a
// workgroup, which lengths the small-batch grouped launch takes and whether its history rings ride along.  Plain C++ on
// values -- no HIP runtime call, no pointer; the HIP header is there for rot_layout's __host__ __device__ alone -- so that tools/decoder_plan_table.hip prints every decision for every legal
// length under the host sanitizers, and tests/test_decoder_seams.py puts a test on either side of every switch-over.
// Internal to libdabgpu.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace dabk {

constexpr int WAVES_PER_WG = 4;

// ---- large-batch variant: one codeword per lane (viterbi_lane_kernels.hip, lane_plan.hpp) ----
// Whole phase cycles and whole 32-bit output words; any length (a codeword whose output tile does not fit into LDS
// writes its words directly, lane_traceback_body).
inline bool lane_supported(int nsteps) { return nsteps >= 38 && nsteps % 6 == 0 && ((nsteps - 6) & 31) == 0; }

// LDS bytes one codeword needs in the first (fallback) wave-per-codeword kernel
inline size_t viterbi_wave_lds_bytes(int nsteps) { return size_t(nsteps) * 12 + 64; }
// largest trellis the wave-per-codeword kernels take: it must fit one CU's 160 KB of LDS (8 B/step for DAB codeword
// lengths) and its mother-bit positions 16 bits (CodeTables::mother_pos) -- about 680 kbit/s.  Longer codewords go to
// the lane kernels, which keep survivors in HBM.
inline bool viterbi_fits(int nsteps) {
    const bool rot = nsteps >= 102 && (nsteps - 6) % 96 == 0;
    return 4 * size_t(nsteps) <= 65535 && (rot ? size_t(nsteps) * 8 + 4096 : viterbi_wave_lds_bytes(nsteps)) <= 160 * 1024;
}

// The per-wave LDS slab of the rot kernel (host and device agree through this one function).
//   survivors: one 8-byte slot per trellis step t (bit l = lane l's r of the step: flip bit q or not), at slot t + (t - 6) / seg_steps
//              for t >= 6 -- one slot of skew per traceback segment, so that the lanes of the traceback, each reading
//              its own segment, spread over the LDS banks (segments are 12..48 slots long: unskewed, 8- to 16-way conflicts)
//   mother:    the depunctured codeword, consumed from a region that starts half-way up the survivors' final extent: a
//              survivor row is only written after the codeword bytes it overlaps have been read (4 B/step consumed vs
//              8 B/step produced); the skew slots are added to the offset
//   out6:      the decoded bits, six per byte;  zero: six all-zero slots (what the traceback reads above the last step:
//              nothing flips)
struct RotLayout {
    int seg_cycles;       // six-step phase cycles per traceback lane
    int seg_steps;        // = 6 * seg_cycles
    int n_lanes;          // lanes that own a segment
    int mother_off, mother_bytes, out6_off, zero_off, total;
};
__host__ __device__ inline RotLayout rot_layout(int nsteps) {
    RotLayout L;
    const int groups = (nsteps - 6) / 6;
    L.seg_cycles = (groups + 63) / 64;
    L.seg_steps = 6 * L.seg_cycles;
    L.n_lanes = (groups + L.seg_cycles - 1) / L.seg_cycles;
    const int skew_slots = (nsteps - 6) / L.seg_steps + 2;
    L.mother_off = 128 * ((nsteps - 6) / 32 + 1) + ((8 * skew_slots + 255) & ~255);
    L.mother_bytes = (4 * nsteps + 255) & ~255;
    L.out6_off = L.mother_off + L.mother_bytes;
    L.zero_off = L.out6_off + ((groups + 255) & ~255);
    L.total = L.zero_off + 256;                                   // (the survivors end below out6_off)
    return L;
}

inline size_t viterbi_rot_lds_bytes(int nsteps) { return size_t(rot_layout(nsteps).total); }

// the rot kernel's lengths: 96 k + 6 steps (every DAB codeword: FIC 768 + 6, EEP 192 n + 6); other lengths use kernel 1
inline bool wave_rot_length(int nsteps) {
    return nsteps >= 102 && (nsteps - 6) % 96 == 0 && viterbi_rot_lds_bytes(nsteps) <= 160 * 1024;
}

// One launch of launch_wave: the kernel, the LDS slab of a wave, the codewords (waves) of a workgroup and the dynamic
// LDS of a workgroup before balanced_lds_bytes pads it.  ok = false: the wave kernels do not take the length.
struct WaveLaunchPlan {
    bool ok, rot;
    int lds_per_wave, waves;
    size_t lds;
};
inline WaveLaunchPlan plan_wave_launch(int nsteps) {
    WaveLaunchPlan p{false, false, 0, 0, 0};
    if (!viterbi_fits(nsteps)) return p;                          // longer codewords: lane kernels only
    p.rot = wave_rot_length(nsteps);
    const size_t per_wave = p.rot ? viterbi_rot_lds_bytes(nsteps) : viterbi_wave_lds_bytes(nsteps);
    p.lds_per_wave = int((per_wave + 255) & ~size_t(255));
    // 4 waves per workgroup normally; long codewords (high bit rates) need more LDS per wave -> fewer waves
    p.waves = WAVES_PER_WG;
    while (p.waves > 1 && size_t(p.lds_per_wave) * p.waves > 160 * 1024) p.waves >>= 1;
    p.lds = size_t(p.lds_per_wave) * p.waves;
    p.ok = p.lds <= 160 * 1024;
    return p;
}

// ---- the small-batch grouped launch (viterbi_rot_grouped_kernel): one wavefront = one workgroup per codeword ----
constexpr int WAVE_GROUP_MAX = 24;    // entries per launch, by value in the kernel arguments; longer lists are chunked
constexpr int HIST_BLOCKS = 32;       // workgroups per entry that write its history ring, behind the decoding ones

// the rot kernel's lengths that the wave kernels hold at all (every DAB profile up to 680 kbit/s)
inline bool wave_group_supported(int nsteps) { return wave_rot_length(nsteps) && viterbi_fits(nsteps); }
// dynamic LDS of the grouped launch: the slab of its longest codeword
inline size_t wave_group_lds_bytes(int nsteps) { return (viterbi_rot_lds_bytes(nsteps) + 255) & ~size_t(255); }
// small rings (the plugin's one stream) ride in the decoding launch; large ones keep a launch of their own, whose
// 256-thread workgroups move bytes faster than 64-thread ones sharing CUs with the decoder.  hist_items: the largest
// ring of the launch, n_streams x 15 x nbits bytes.
inline bool wave_history_rides(size_t hist_items) { return hist_items > 0 && hist_items <= size_t(1) << 20; }
// `n_waves` codewords whose longest takes `max_nsteps` steps are all resident at once on `n_cu` compute units
inline bool wave_group_fits_one_round(int max_nsteps, long n_waves, unsigned n_cu) {
    const size_t lds = wave_group_lds_bytes(max_nsteps);
    return n_waves >= 0 && size_t(n_waves) <= size_t(n_cu) * (size_t(160 * 1024) / lds);
}

}  // namespace dabk
