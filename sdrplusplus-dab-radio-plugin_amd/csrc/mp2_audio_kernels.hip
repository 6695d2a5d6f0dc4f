// mp2_audio_kernels.hip -- checked layer-II frames to sub-band samples and audio levels (dabgpu_mp2_subbands_dev; contract
// and code: include/dabgpu_mp2_audio.h, shared with the host twin and the host mirror).
//
// Two launches behind the follow call, for all entries and all rows of a batch.
//   mp2_audio_zero_kernel  a lane per entry clears the entry's counters.
//   mp2_audio_kernel       workgroup (entry, chunk) of four waves, ONE WAVE PER FRAME (a lane per frame would diverge on
//                          every bit field).  Rows, rate and phase come from the record the follow call wrote, the held
//                          half of a 24 kHz frame from the carry record it read.  The wave brings its frame into LDS as
//                          big-endian words (16-byte loads where the frame lies on 16 bytes).  A lane is a cell:
//                          lane = 32 ch + sb, so a channel's 32 sub-band values of one t are one 128-byte store.  The
//                          allocation position is a closed form of (table, bound); the SCFSI position a ballot and two
//                          popcounts in stream order; the scale-factor position and the position within a granule two
//                          scans over the sub-bands (a granule has the same size twelve times).  Every lane then reads
//                          its own <= 48 bits a granule from LDS -- both lanes of a shared cell the same bits.  Power and
//                          peak are reduced per 32-lane half in a fixed order; the counters of the call are integer
//                          atomics, one per frame: no float atomics, so a call's results are reproducible.
#include <hip/hip_runtime.h>

#include "../../include/dabgpu_mp2_audio.h"
#include "kernels.hpp"

namespace dabk {
namespace {

namespace mp2 = dabgpu_mp2;

constexpr int AUDIO_WAVES = 4;                      // frames per workgroup: one per wave
constexpr int AUDIO_MAX_BYTES = 1152;               // the longest frame: 384 kbit/s at 48 kHz (24 kHz ends at 6 * 160)
constexpr int AUDIO_LDS_WORDS = AUDIO_MAX_BYTES / 4 + 4;   // the bit reader takes the word behind the one it starts in

static_assert(sizeof(SuperframeStatus) == 64 && sizeof(mp2::Result) == 64 && sizeof(mp2::Level) == 32 && sizeof(mp2::AudioResult) == 32,
              "records of the ABI");
static_assert(mp2::FRAME_VALUES % 4 == 0 && mp2::SUBBANDS == 32, "a channel's sub-bands are half a wave");

__device__ __forceinline__ uint32_t load_word(const uint8_t *p) {
    if ((reinterpret_cast<uintptr_t>(p) & 3) == 0) return *reinterpret_cast<const uint32_t *>(p);
    return uint32_t(p[0]) | (uint32_t(p[1]) << 8) | (uint32_t(p[2]) << 16) | (uint32_t(p[3]) << 24);
}

// one logical frame of n bytes (a multiple of 8) into LDS as big-endian words, by the whole wave
__device__ __forceinline__ void load_frame(uint32_t *dst, const uint8_t *src, int n, int lane) {
    int done = 0;
    if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {
        for (int i = lane; i < n / 16; i += 64) {
            const uint4 v = reinterpret_cast<const uint4 *>(src)[i];
            dst[4 * i] = __builtin_bswap32(v.x); dst[4 * i + 1] = __builtin_bswap32(v.y);
            dst[4 * i + 2] = __builtin_bswap32(v.z); dst[4 * i + 3] = __builtin_bswap32(v.w);
        }
        done = n / 16 * 4;
    }
    for (int i = done + lane; i < n / 4; i += 64) dst[i] = __builtin_bswap32(load_word(src + 4 * i));
}

// n (1 .. 16) bits at bit position pos of the frame in LDS
__device__ __forceinline__ uint32_t lds_bits(const uint32_t *w, int pos, int n) {
    const int i = pos >> 5;
    const uint64_t x = (uint64_t(w[i]) << 32) | w[i + 1];
    return uint32_t(x >> (64 - (pos & 31) - n)) & ((1u << n) - 1);
}

// inclusive sum over the sub-bands 0 .. sb of a 32-lane half
__device__ __forceinline__ int scan_subbands(int v, int sb) {
#pragma unroll
    for (int d = 1; d < 32; d <<= 1) {
        const int y = __shfl_up(v, d, 32);
        if (sb >= d) v += y;
    }
    return v;
}

__global__ __launch_bounds__(64) void mp2_audio_zero_kernel(const Mp2AudioEntry *table, int n_entries) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_entries) return;
    int32_t *a = reinterpret_cast<int32_t *>(table[i].audio);
#pragma unroll
    for (int w = 0; w < 8; w++) a[w] = 0;
}

__global__ __launch_bounds__(64 * AUDIO_WAVES) void mp2_audio_kernel(const Mp2AudioEntry *table, int chunks, int n_cifs) {
    __shared__ __attribute__((aligned(16))) uint32_t words[AUDIO_WAVES][AUDIO_LDS_WORDS];
    const int ei = blockIdx.x / unsigned(chunks), k0 = int(blockIdx.x % unsigned(chunks)) * AUDIO_WAVES;
    const Mp2AudioEntry e = table[ei];
    const mp2::Result *res = reinterpret_cast<const mp2::Result *>(e.result);
    const int id = res->id, phase = res->phase;
    if ((id != 0 && id != 1) || (phase != 0 && phase != 1)) return;     // no rate: no rows (the whole workgroup)
    mp2::Carry cy = {0, 0, 0};
    if (e.carry_in) {
        const int4 h = *reinterpret_cast<const int4 *>(e.carry_in);
        cy = mp2::read_carry(h.x, h.y, h.z, h.w);
    }
    const int B = e.bitrate, lf = 3 * B, per = id == 1 ? 1 : 2, L = per * lf;
    // (what the follow call wrote never names a row beyond the frames of its call)
    const int frames = min(res->frames, (cy.held + n_cifs - phase) / per);
    if (k0 >= frames) return;                                           // (the whole workgroup, before the barrier)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, k = k0 + wave;
    const bool live = k < frames;
    uint32_t *w = words[wave];
    bool good = false;
    if (live) {
        good = reinterpret_cast<const int32_t *>(e.status)[size_t(k) * 16 + 4] == 1 && L <= AUDIO_MAX_BYTES;
        if (good)
            for (int part = 0; part < per; part++) {
                const int i = phase + per * k + part;
                const uint8_t *src = i < cy.held ? reinterpret_cast<const uint8_t *>(e.carry_in) + mp2::CARRY_HEADER
                                                 : reinterpret_cast<const uint8_t *>(e.in) + size_t(i - cy.held) * e.in_stride;
                load_frame(w + part * (lf / 4), src, lf, lane);
            }
    }
    __syncthreads();
    if (!live) return;

    mp2::Level *level = reinterpret_cast<mp2::Level *>(e.levels) + k;
    float *out = e.subbands ? reinterpret_cast<float *>(e.subbands) + size_t(k) * mp2::FRAME_VALUES : nullptr;
    mp2::AudioResult *audio = reinterpret_cast<mp2::AudioResult *>(e.audio);
    // a frame that is not decoded: its record, zeros for its values, its counter
    auto undecoded = [&](int kind) {
        if (out)
            for (int i = lane; i < mp2::FRAME_VALUES / 4; i += 64) reinterpret_cast<float4 *>(out)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (lane == 0) {
            int32_t *lv = reinterpret_cast<int32_t *>(level);
            lv[0] = kind;
#pragma unroll
            for (int q = 1; q < 8; q++) lv[q] = 0;
            atomicAdd(kind == mp2::AUDIO_OVERRUN ? &audio->overrun : &audio->not_good, 1);
        }
    };
    if (!good || mp2::header_id(w[0], B) != id) return undecoded(mp2::AUDIO_NOT_GOOD);

    const mp2::Shape s = mp2::frame_shape(w[0], id, B);
    const int limit = mp2::audio_limit(L, s.c);
    const int ch = lane >> 5, sb = lane & 31;
    int n = 0;                                                          // the cell's class; 0: not active
    if (sb < s.t.sblimit && ch < s.channels) {
        const int a = int(lds_bits(w, mp2::alloc_position(s, sb, ch), mp2::nbal(s.t, sb)));
        if (a) n = mp2::levels(s.t, sb, a);
    }
    const bool active = n != 0;
    // SCFSI: two bits per active cell in stream order (sb-major, ch-minor)
    const uint64_t m = __ballot(active);
    const uint32_t m0 = uint32_t(m), m1 = uint32_t(m >> 32), below = (1u << sb) - 1;
    const int before = __popc(m0 & (ch ? below | (1u << sb) : below)) + __popc(m1 & below);
    const int cells = __popcll(m);
    int pos = mp2::alloc_position(s, s.t.sblimit, 0);
    if (pos + 2 * cells > limit) return undecoded(mp2::AUDIO_OVERRUN);
    const int scfsi = active ? int(lds_bits(w, pos + 2 * before, 2)) : 0;
    pos += 2 * cells;
    // scale factors: the indices sent, in stream order
    const int sent = active ? mp2::scf_sent(scfsi) : 0;
    const int sent_other = __shfl_xor(sent, 32);
    const int sent_through = scan_subbands(sent + sent_other, sb);
    const int sent_all = __shfl(sent_through, 31, 32);
    if (pos + 6 * sent_all > limit) return undecoded(mp2::AUDIO_OVERRUN);
    const int first = pos + 6 * (sent_through - sent - sent_other + (ch ? sent_other : 0));
    const int i0 = sent > 0 ? int(lds_bits(w, first, 6)) : 63, i1 = sent > 1 ? int(lds_bits(w, first + 6, 6)) : 63,
              i2 = sent > 2 ? int(lds_bits(w, first + 12, 6)) : 63;
    int scf63 = (sent > 0 && i0 == 63) + (sent > 1 && i1 == 63) + (sent > 2 && i2 == 63);
    auto index_of = [&](int j) { return j == 0 ? i0 : j == 1 ? i1 : i2; };
    const float f0 = mp2::scale_factor(index_of(mp2::scf_of_part(scfsi, 0))), f1 = mp2::scale_factor(index_of(mp2::scf_of_part(scfsi, 1))),
                f2 = mp2::scale_factor(index_of(mp2::scf_of_part(scfsi, 2)));
    pos += 6 * sent_all;
    // samples: the fields of a granule in stream order; a shared field belongs to channel 0's lane and is read by both
    const bool own = ch == 0 || sb < s.bound;
    const int width = active && own ? mp2::field_bits(n) : 0;
    const int width_other = __shfl_xor(width, 32);
    const int width_through = scan_subbands(width + width_other, sb);
    const int granule = __shfl(width_through, 31, 32);
    if (pos + mp2::GRANULES * granule > limit) return undecoded(mp2::AUDIO_OVERRUN);
    const int offset = width_through - width - width_other + (ch && own ? width_other : 0);
    const bool is_grouped = mp2::grouped(n);
    const int b = active ? (is_grouped ? mp2::code_bits(n) : mp2::sample_bits(n)) : 1;
    const float r = active ? mp2::recip(n) : 0.0f;
    float power = 0.0f, peak = 0.0f;
    for (int g = 0; g < mp2::GRANULES; g++) {
        const float f = g < 4 ? f0 : g < 8 ? f1 : f2;
        float x[3] = {0.0f, 0.0f, 0.0f};
        if (active) {
            const int p = pos + g * granule + offset;
            uint32_t smp[3];
            if (is_grouped) {
                mp2::group_split(lds_bits(w, p, b), n, smp);
            } else {
#pragma unroll
                for (int q = 0; q < 3; q++) smp[q] = lds_bits(w, p + q * b, b);
            }
#pragma unroll
            for (int q = 0; q < 3; q++) x[q] = mp2::value(smp[q], n, r, f);
        }
#pragma unroll
        for (int q = 0; q < 3; q++) {
            if (out) out[(ch * mp2::SAMPLES + 3 * g + q) * mp2::SUBBANDS + sb] = x[q];
            power += x[q] * x[q];
            peak = fmaxf(peak, fabsf(x[q]));
        }
    }
#pragma unroll
    for (int d = 16; d > 0; d >>= 1) {
        power += __shfl_xor(power, d);
        peak = fmaxf(peak, __shfl_xor(peak, d));
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) scf63 += __shfl_xor(scf63, d);
    const float power1 = __shfl(power, 32), peak1 = __shfl(peak, 32);
    if (lane == 0) {
        int32_t *lv = reinterpret_cast<int32_t *>(level);
        lv[0] = mp2::AUDIO_DECODED; lv[1] = s.channels; lv[2] = cells; lv[3] = scf63;
        lv[4] = __float_as_int(power); lv[5] = __float_as_int(power1); lv[6] = __float_as_int(peak); lv[7] = __float_as_int(peak1);
        atomicAdd(&audio->decoded, 1);
        if (power + power1 == 0.0f) atomicAdd(&audio->silent, 1);
    }
}

}  // namespace

size_t mp2_audio_table_bytes(int n_entries) { return size_t(n_entries) * sizeof(Mp2AudioEntry); }

hipError_t launch_mp2_subbands(const Mp2AudioEntry *entries, int n_entries, int n_cifs, void *d_table, size_t table_bytes, hipStream_t stream) {
    if (n_entries <= 0) return hipSuccess;
    if (n_cifs < 0 || !d_table || table_bytes < mp2_audio_table_bytes(n_entries) || (reinterpret_cast<uintptr_t>(d_table) & 15))
        return hipErrorInvalidValue;
    for (int i = 0; i < n_entries; i++)
        if (!mp2::bitrate_ok(entries[i].bitrate)) return hipErrorInvalidValue;
    const int chunks = (n_cifs + 1 + AUDIO_WAVES - 1) / AUDIO_WAVES;
    if (size_t(n_entries) * size_t(chunks) > size_t(0x7fffffff) || n_cifs > (1 << 28)) return hipErrorInvalidValue;
    // (pageable memory: the copy has left `entries` when the call returns)
    hipError_t err = hipMemcpyAsync(d_table, entries, size_t(n_entries) * sizeof(Mp2AudioEntry), hipMemcpyHostToDevice, stream);
    if (err != hipSuccess) return err;
    const Mp2AudioEntry *table = static_cast<const Mp2AudioEntry *>(d_table);
    hipLaunchKernelGGL(mp2_audio_zero_kernel, dim3(unsigned((n_entries + 63) / 64)), dim3(64), 0, stream, table, n_entries);
    hipLaunchKernelGGL(mp2_audio_kernel, dim3(unsigned(n_entries) * unsigned(chunks)), dim3(64 * AUDIO_WAVES), 0, stream, table, chunks, n_cifs);
    return hipGetLastError();
}

}  // namespace dabk
