// wave_copy.hpp -- a block of bytes from one place in global memory to another by a whole wave64 (mot_kernels.hip: a
// closed segment to its place in the arena, a completed object into its slot).
//
// Device code under hipcc; plain inline C++ under a host compiler, where tests/wave_copy_exhaustive.cpp and
// tests/mot_order_census.cpp call it for lane = 0 .. 63 in turn: the lanes of one copy do not depend on each other (no
// overlap, no lane reads what another wrote), so that is the wave, exactly.
#ifndef DABK_WAVE_COPY_HPP
#define DABK_WAVE_COPY_HPP

#include <stdint.h>

#if defined(__HIPCC__)
#define DABK_WAVE_COPY_FN __host__ __device__ __forceinline__
#else
#define DABK_WAVE_COPY_FN inline
#endif

namespace dabk {

#if !defined(__HIPCC__)
struct alignas(16) uint4 {                // HIP's 16-byte vector, for a host compiler
    uint32_t x, y, z, w;
};
#endif

// len bytes from src to dst (global memory, no overlap) by the whole wave: 16-byte accesses where both run on the same
// 16-byte phase, 4-byte ones where on the same 4-byte phase, else a byte a lane -- coalesced either way
template <class W> DABK_WAVE_COPY_FN void wave_copy_as(uint8_t *dst, const uint8_t *src, int len, int lane) {
    constexpr int B = int(sizeof(W));
    int head = int((B - (reinterpret_cast<uintptr_t>(dst) & (B - 1))) & (B - 1));
    head = head < len ? head : len;
    if (lane < head) dst[lane] = src[lane];
    const int words = (len - head) / B;
    const W *s = reinterpret_cast<const W *>(src + head);
    W *d = reinterpret_cast<W *>(dst + head);
    for (int i = lane; i < words; i += 64) d[i] = s[i];
    const int done = head + words * B;
    if (done + lane < len) dst[done + lane] = src[done + lane];       // (fewer than B <= 16 bytes are left)
}
DABK_WAVE_COPY_FN void wave_copy(uint8_t *dst, const uint8_t *src, int len, int lane) {
    const unsigned phase = unsigned(reinterpret_cast<uintptr_t>(dst) ^ reinterpret_cast<uintptr_t>(src));
    if (!(phase & 15)) wave_copy_as<uint4>(dst, src, len, lane);
    else if (!(phase & 3)) wave_copy_as<uint32_t>(dst, src, len, lane);
    else
        for (int i = lane; i < len; i += 64) dst[i] = src[i];
}

}  // namespace dabk
#endif
