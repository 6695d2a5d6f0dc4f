// quality_kernels.hip -- reception quality from what the front end and the decoder already left on the device:
//
//   MER   the modulation error ratio of the differential constellation, from the soft bits.  The quantiser (ofdm_kernels.hip,
//         A6) divides both components of a carrier by the larger one, so a carrier that is not erased is (+-127, +-s) or
//         (+-s, +-127), s = trunc(127 min/max): the pair keeps exactly the phase of the differential symbol, whose ideal
//         points lie on the diagonals.  With a = |re|, b = |im| the signal term is (a + b)^2 and the error term (a - b)^2;
//         for a small phase error e their ratio is ~1/e^2.  Both are summed as integers (exact, independent of the launch).
//   BER   channel bit errors before the Viterbi decoder: the decoded bytes are scrambled again, re-encoded with the mother
//         code and punctured as the profile says, and every kept bit is compared with the hard decision of the soft byte
//         the decoder read for it (soft_source.hpp: the same FIC layout, time de-interleaver and carried history).
//
// Both kernels stream what they read once and keep nothing in LDS.
#include <algorithm>

#include "mem_stream.hpp"
#include "kernels.hpp"
#include "dab_tables.hpp"
#include "soft_source.hpp"

namespace dabk {

using namespace dab;

namespace {

// |x| of the four signed bytes of a word, as unsigned bytes 0..128 (no carry crosses a byte: ~x + 1 <= 128)
__device__ __forceinline__ unsigned abs_bytes(unsigned x) {
    const unsigned m = (x >> 7) & 0x01010101u;
    return (x ^ (m * 0xFFu)) + m;
}

// number of bytes of v that are not zero
__device__ __forceinline__ unsigned nonzero_bytes(unsigned v) {
    return unsigned(__popc((((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v) & 0x80808080u));
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---------------------------------------------------------------------------------------------------------
// MER: one wave per frame.  A work item is 16 carriers of one symbol: a 16-byte load from each half of the symbol's soft
// bits.  Per four carriers: (a+b)^2 + (a-b)^2 = 2(a^2 + b^2) and (a+b)^2 - (a-b)^2 = 4ab, so three byte dot products
// (a.a, b.b, a.b) carry both sums.  Per lane at most 113 items x 16 carriers x 2 x 128^2 < 2^32.
// ---------------------------------------------------------------------------------------------------------
constexpr int MER_CHUNKS = NB_CARRIERS / 16;      // 96 work items per symbol

__global__ __launch_bounds__(256) void mer_kernel(const int8_t *soft, size_t stride, int n_frames, int first_symbol,
                                                  int n_symbols, MerSums *out) {
    const int lane = threadIdx.x & 63;
    const int f = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (f >= n_frames) return;
    const int8_t *base = soft + size_t(f) * stride + size_t(first_symbol) * NB_SYM_BITS;
    const int items = n_symbols * MER_CHUNKS;
    unsigned sq = 0, ab = 0, nz = 0;
#pragma unroll 2
    for (int i = lane; i < items; i += 64) {
        const int s = i / MER_CHUNKS, c = i - s * MER_CHUNKS;
        const int8_t *p = base + size_t(s) * NB_SYM_BITS + 16 * c;
        const uint4 re = ld_stream(reinterpret_cast<const uint4 *>(p));
        const uint4 im = ld_stream(reinterpret_cast<const uint4 *>(p + NB_CARRIERS));
        const unsigned rw[4] = {re.x, re.y, re.z, re.w}, iw[4] = {im.x, im.y, im.z, im.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned a = abs_bytes(rw[k]), b = abs_bytes(iw[k]);
            sq = __builtin_amdgcn_udot4(a, a, sq, false);
            sq = __builtin_amdgcn_udot4(b, b, sq, false);
            ab = __builtin_amdgcn_udot4(a, b, ab, false);
            nz += nonzero_bytes(a | b);
        }
    }
    const uint64_t tsq = wave_sum(uint64_t(sq)), tab = wave_sum(uint64_t(ab));
    const unsigned tnz = wave_sum(nz);
    if (lane == 0) {
        MerSums r;
        r.signal = tsq + 2 * tab;
        r.error = tsq - 2 * tab;
        r.carriers = int32_t(tnz);
        r.reserved = 0;
        out[f] = r;
    }
}

// ---------------------------------------------------------------------------------------------------------
// Channel BER: one wave per codeword, a lane per trellis step (t = lane, lane + 64, ...).  The mother code is feed-forward:
// step t's four output bits depend on the input window u[t-6..t] alone (bits outside 0 .. nsteps-7 are zero: start state
// and tail), which two bytes of the re-scrambled output always hold.  The FIC and every sub-channel of a call go into ONE
// launch: the entry table travels by value in the kernel arguments (as the lane decoder's LaneEntryPack).
// ---------------------------------------------------------------------------------------------------------
constexpr int BER_GROUP_MAX = 16;
struct BerEntry {
    SoftSrc src;
    const int32_t *punct_idx;
    const uint8_t *prbs;
    const uint8_t *dec;        // decoded bytes, codeword g at dec + g*nbytes
    uint2 *counts;             // [n_codewords] {errors, bits}
    int nsteps, nbytes, first_wave, n_codewords;
};
struct BerPack {
    int n;
    int total_waves;
    BerEntry e[BER_GROUP_MAX];
};

// polynomials {0133, 0171, 0145, 0133} (ETSI EN 300 401 clause 11.1.1) as masks whose bit k taps u[t-k]
constexpr unsigned POLY0 = 109, POLY1 = 79, POLY2 = 83, POLY3 = 109;

__device__ __forceinline__ unsigned parity7(unsigned x) { return unsigned(__popc(x)) & 1u; }

__global__ __launch_bounds__(256) void channel_ber_kernel(const BerPack pack) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (wave >= pack.total_waves) return;
    int ei = 0;
    while (ei + 1 < pack.n && wave >= pack.e[ei + 1].first_wave) ei++;
    const BerEntry &en = pack.e[ei];
    const SoftSrc src = en.src;
    const int g = wave - en.first_wave;
    const int nbytes = en.nbytes;
    const uint8_t *dec = en.dec + size_t(g) * nbytes;
    // input byte j of the encoder (decoded byte re-scrambled); 0 outside the codeword's information bits
    auto in_byte = [&](int j) -> unsigned {
        return (j >= 0 && j < nbytes) ? unsigned(dec[j] ^ en.prbs[j]) : 0u;
    };
    unsigned errors = 0, bits = 0;
    for (int t = lane; t < en.nsteps; t += 64) {
        const int j0 = ((t + 2) >> 3) - 1;                     // byte of u[t-6] (floor((t-6)/8))
        const unsigned v = (in_byte(j0) << 8) | in_byte(j0 + 1);
        const unsigned w = (v >> (15 - (t - 8 * j0))) & 0x7Fu;  // bit k = u[t-k]
        const unsigned cb[4] = {parity7(w & POLY0), parity7(w & POLY1), parity7(w & POLY2), parity7(w & POLY3)};
        const int4 pi = *reinterpret_cast<const int4 *>(en.punct_idx + 4 * t);
        const int idx[4] = {pi.x, pi.y, pi.z, pi.w};
#pragma unroll
        for (int m = 0; m < 4; m++) {
            if (idx[m] < 0) continue;                          // punctured away
            const int sv = soft_at(src, g, idx[m]);
            if (sv == 0) continue;                             // erased: no decision
            bits++;
            errors += unsigned(sv > 0) ^ cb[m];                // +127 = logical 1
        }
    }
    errors = wave_sum(errors);
    bits = wave_sum(bits);
    if (lane == 0) en.counts[g] = make_uint2(errors, bits);
}

}  // namespace

hipError_t launch_mer(const int8_t *soft, size_t stride, int n_frames, int first_symbol, int n_symbols, MerSums *out,
                      hipStream_t s) {
    if (n_frames <= 0) return hipSuccess;
    if (((reinterpret_cast<uintptr_t>(soft) | stride) & 15) || first_symbol < 0 || n_symbols <= 0 ||
        first_symbol + n_symbols > NB_DATA_SYMBOLS)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(mer_kernel, dim3(unsigned((n_frames + 3) / 4)), dim3(256), 0, s, soft, stride, n_frames, first_symbol,
                       n_symbols, out);
    return hipGetLastError();
}

int ber_group_max() { return BER_GROUP_MAX; }

hipError_t launch_channel_ber(const BerItem *items, int n, hipStream_t s) {
    for (int i0 = 0; i0 < n; i0 += BER_GROUP_MAX) {
        BerPack pack{};
        for (int i = i0; i < std::min(n, i0 + BER_GROUP_MAX); i++) {
            const BerItem &it = items[i];
            const MscArgs &a = it.args;
            const int n_cw = a.n_streams * a.frames_per_stream * NB_CIFS;
            if (n_cw <= 0) continue;
            if (!it.punct_idx || !it.prbs_bytes || !a.out || !it.counts || it.nsteps < 7 ||
                (reinterpret_cast<uintptr_t>(it.punct_idx) & 15) || (reinterpret_cast<uintptr_t>(it.counts) & 7))
                return hipErrorInvalidValue;
            BerEntry &e = pack.e[pack.n++];
            e.src = it.is_fic ? make_fic_src(a.soft, a.soft_stride, n_cw) : make_msc_src(a);
            e.punct_idx = it.punct_idx;
            e.prbs = it.prbs_bytes;
            e.dec = a.out;
            e.counts = reinterpret_cast<uint2 *>(it.counts);
            e.nsteps = it.nsteps;
            e.nbytes = (it.nsteps - 6) / 8;
            e.first_wave = pack.total_waves;
            e.n_codewords = n_cw;
            pack.total_waves += n_cw;
        }
        if (pack.total_waves == 0) continue;
        hipLaunchKernelGGL(channel_ber_kernel, dim3(unsigned((pack.total_waves + 3) / 4)), dim3(256), 0, s, pack);
    }
    return hipGetLastError();
}

}  // namespace dabk
