// eti_cif.hpp -- what the ETI(NI) writer (eti_kernels.hip) and the EDI writer (edi_kernels.hip) decide about one output
// CIF, once: the FIC delay of 15 CIFs and the history record, warm-up, the CIF count from the anchor pre-pass, the ERR /
// STAT byte and the flags of dabgpu_eti_status -- and the CRC-16 arithmetic both fold their frames with.
#ifndef DABK_ETI_CIF_HPP
#define DABK_ETI_CIF_HPP

#include "kernels.hpp"

namespace dabk {

constexpr uint32_t ETI_POLY = 0x11021u;
constexpr int ETI_FLAG_WARMUP = 1, ETI_FLAG_FIB_CRC = 2, ETI_FLAG_NO_ANCHOR = 4, ETI_FLAG_COUNT_MISMATCH = 8;

// a(x) b(x) mod P, b's lowest `bits` bits
__device__ __forceinline__ uint32_t eti_gf_mul(uint32_t a, uint32_t b, int bits) {
    uint32_t r = 0;
#pragma unroll
    for (int i = bits - 1; i >= 0; i--) {
        r <<= 1;
        if (r & 0x10000u) r ^= ETI_POLY;
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}

// entry `byte` of the CRC's byte table
__device__ __forceinline__ uint16_t eti_crc_table_entry(int byte) {
    uint32_t r = uint32_t(byte) << 8;
#pragma unroll
    for (int i = 0; i < 8; i++) r = (r & 0x8000u) ? ((r << 1) ^ ETI_POLY) : (r << 1);
    return uint16_t(r);
}

// the count a valid first FIB that begins with FIG 0/0 carries, or -1 (w0 / w1: its first two little-endian words)
__device__ __forceinline__ int eti_fig0_0_count(uint32_t w0, uint32_t w1, int crc_ok) {
    const int upper = int(w1 & 0x1fu), lower = int((w1 >> 8) & 0xffu);
    if (!crc_ok || (w0 & 0xffffu) != 0x0005u || upper >= 20 || lower >= 250) return -1;
    return upper * 250 + lower;
}

__device__ __forceinline__ int eti_history_valid(const EtiHistory *h) {
    if (!h) return 0;
    const int v = h->valid;
    return v < 0 ? 0 : v > ETI_FIC_DELAY ? ETI_FIC_DELAY : v;
}

// output CIF t of stream s of a call of n_cif CIFs
struct EtiCif {
    const uint8_t *fic;        // its 96 FIC bytes (4-byte aligned), nullptr = a warm-up CIF: zeros
    uint32_t fib_ok;           // bit j = FIB j passed its CRC
    uint32_t flags;            // ETI_FLAG_*
    uint32_t err;              // the ERR byte of ETI(NI), STAT of EDI
    int count;                 // 0 .. 4999
};

// base: what eti_anchor_kernel left per stream (count of the call's first CIF | no-anchor << 16)
__device__ __forceinline__ EtiCif eti_cif(const uint8_t *fib, const uint8_t *crc_ok, const EtiHistory *history_in, const int32_t *base_of,
                                          int s, int t, int n_cif) {
    const int c = t - ETI_FIC_DELAY;
    const EtiHistory *hin = history_in ? history_in + s : nullptr;
    const bool warm = c < 0 && t < ETI_FIC_DELAY - eti_history_valid(hin);
    const uint8_t *fic = c >= 0 ? fib + (size_t(s) * n_cif + c) * ETI_FIC_BYTES : warm ? nullptr : hin->fib[t];
    const uint8_t *ok = c >= 0 ? crc_ok + (size_t(s) * n_cif + c) * 3 : warm ? nullptr : hin->crc_ok[t];
    const int base = base_of[s];
    EtiCif r;
    r.fic = fic;
    r.fib_ok = 0;
    r.count = ((base & 0xffff) + t + ETI_CIF_COUNTS - ETI_FIC_DELAY) % ETI_CIF_COUNTS;
    int own = -1;
    if (!warm) {
        const uint32_t *w = reinterpret_cast<const uint32_t *>(fic);
        r.fib_ok = (ok[0] ? 1u : 0u) | (ok[1] ? 2u : 0u) | (ok[2] ? 4u : 0u);
        own = eti_fig0_0_count(w[0], w[1], int(r.fib_ok & 1u));
    }
    r.flags = (warm ? ETI_FLAG_WARMUP : r.fib_ok != 7u ? ETI_FLAG_FIB_CRC : 0) | ((base >> 16) & 1 ? ETI_FLAG_NO_ANCHOR : 0) |
              (own >= 0 && own != r.count ? ETI_FLAG_COUNT_MISMATCH : 0);
    r.err = warm ? 0x00u : r.fib_ok == 7u ? 0xFFu : 0xE1u;
    return r;
}

}  // namespace dabk
#endif
