// soft_source.hpp -- where a codeword's punctured soft bits come from: one source struct (SoftSrc) that states the frame
// layout of the FIC, the time de-interleaver's mapping of an MSC sub-channel including the carried history, and contiguous
// plain codewords, with one maker for each.  One statement for every kernel that
// reads codewords out of demodulated frames -- the lane Viterbi (viterbi_lane_kernels.hip) and the channel-BER count
// (quality_kernels.hip), which must read each soft byte from exactly where the decoder read it.  Internal to libdabgpu.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "dab_tables.hpp"
#include "kernels.hpp"

namespace dabk {

// time de-interleaver: punctured bit i of a logical frame is delayed by bitrev4(i mod 16) CIFs (ETSI EN 300 401 clause
// 12); the codeword completed by CIF t reads bit i from CIF t - 15 + tdi_delay(i)
__host__ __device__ inline int tdi_delay(int i) {
#if defined(__HIP_DEVICE_COMPILE__)
    return int(__brev(unsigned(i) & 15u) >> 28);
#else
    const unsigned b = unsigned(i) & 15u;
    return int(((b & 1u) << 3) | ((b & 2u) << 1) | ((b & 4u) >> 1) | ((b & 8u) >> 3));
#endif
}

// The one source form: codeword g lies at row(g), four to a "frame" `stride` bytes long, `per_cif` apart inside it;
// consecutive codeword indices are consecutive CIFs of a stream of cifs_per_stream.  PRE = how many earlier codewords a
// codeword draws from (the time de-interleaver reads CIFs t-15..t of its own stream).  Sources without interleaving -- the
// FIC, plain codewords -- say so with d_force = 15: every bit "delay 15" = the codeword's own row, never a history row.
struct SoftSrc {
    static constexpr int PRE = 15;
    const int8_t *soft;
    size_t stride;
    const int8_t *hist;
    int cifs_per_stream;
    int base_off;             // first byte of the codeword's part in CIF 0 of a frame (FIC: 0; MSC: 9216 + 64*start CU)
    int per_cif;              // distance between the four codewords of a frame (FIC group: 2304; CIF: 55296)
    int nbits;
    int d_force;              // -1: time de-interleaver delays from the descriptor table; 15: no interleaving
    __device__ __forceinline__ const int8_t *row(int g) const {
        return soft + size_t(g >> 2) * stride + base_off + size_t(g & 3) * per_cif;
    }
};
__host__ __device__ inline SoftSrc make_msc_src(const MscArgs &a) {
    return SoftSrc{a.soft, a.soft_stride, a.hist_in, a.frames_per_stream * dab::NB_CIFS, dab::NB_FIC_BITS + a.start_bit,
                   dab::NB_CIF_BITS, a.nbits, -1};
}
// the FIC of n_codewords / 4 frames: four 2304-bit groups per frame, all of it one "stream"
__host__ __device__ inline SoftSrc make_fic_src(const int8_t *soft, size_t stride, int n_codewords) {
    return SoftSrc{soft, stride, nullptr, n_codewords + 128, 0, dab::NB_FIC_GROUP_BITS, dab::NB_FIC_GROUP_BITS, 15};
}
// contiguous punctured codewords, n_punct bytes each: "frames" of four
__host__ __device__ inline SoftSrc make_plain_src(const int8_t *punct, int n_punct, int n_codewords) {
    return SoftSrc{punct, size_t(4) * size_t(n_punct), nullptr, n_codewords + 128, 0, n_punct, n_punct, 15};
}

// The FIC and plain codewords as sources of their own, without the 15 rows of look-back (PRE = 0, every bit in the
// codeword's own row): what the forward pass of a SINGLE such item stages (lane_forward_fused_kernel).  In SoftSrc form
// it stages 79 rows a group for 64 -- measured 1.2 % (FIC) and 1.6 % (plain) of the call at 65 536 codewords,
// profiles/lane_one_path.txt.  Nothing else uses them: lists, the prep kernel and the BER count take SoftSrc.
struct LSrcFic {
    static constexpr int PRE = 0, d_force = 0;
    const int8_t *soft;
    size_t stride;
    __device__ __forceinline__ const int8_t *row(int g) const {
        return soft + size_t(g >> 2) * stride + size_t(g & 3) * dab::NB_FIC_GROUP_BITS;
    }
};
struct LSrcPlain {
    static constexpr int PRE = 0, d_force = 0;
    const int8_t *punct;
    int n_punct;
    __device__ __forceinline__ const int8_t *row(int g) const { return punct + size_t(g) * n_punct; }
};

// soft byte of punctured bit `idx` of codeword g, read where the decoder reads it: CIF g - 15 + delay of the codeword's
// own stream, or the carried history for CIFs before the stream's first (0 = erased when there is none)
__device__ __forceinline__ int soft_at(const SoftSrc &s, int g, int idx) {
    const int d = s.d_force >= 0 ? s.d_force : tdi_delay(idx);
    const int stream = g / s.cifs_per_stream;
    const int t = g - stream * s.cifs_per_stream;
    if (t + d >= 15) return s.row(g - 15 + d)[idx];
    return s.hist ? int(s.hist[(size_t(stream) * 15 + t + d) * s.nbits + idx]) : 0;
}

}  // namespace dabk
