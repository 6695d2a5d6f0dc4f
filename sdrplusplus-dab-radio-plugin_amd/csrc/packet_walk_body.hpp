// packet_walk_body.hpp -- the walk launch of the packet-mode calls: one wave per entry, a template over its sink.  The wave
// sums the scan records' counters (a lane per frame), finds the frames with followed packets by ballot, and per followed
// packet stages its header and useful bytes into LDS, lane 0 runs the sink's control over LDS and leaves copy orders, and all
// 64 lanes execute them.  packet_kernels.hip instantiates it for dabgpu_packet_slides_dev (SlidesWalk),
// packet_carousel_kernels.hip for dabgpu_packet_carousel_dev (CarouselWalk).
#ifndef DABK_PACKET_WALK_BODY_HPP
#define DABK_PACKET_WALK_BODY_HPP

#include <hip/hip_runtime.h>

#include "../../include/dabgpu_mot_carousel.h"
#include "kernels.hpp"
#include "wave_copy.hpp"

namespace dabk {
namespace {

namespace mot = dabgpu_mot;
namespace pkt = dabgpu_packet;
namespace car = dabgpu_carousel;

// the orders of one control step, by the whole wave; each complete before the next begins
__device__ __forceinline__ void execute_orders(const mot::Orders &ord, const uint8_t *bytes, uint8_t *arena, uint8_t *out,
                                               uint8_t *directory, int lane) {
    const int n_orders = ord.n;
    for (int j = 0; j < n_orders; j++) {
        const mot::Order o = ord.o[j];
        if (o.kind == pkt::ORDER_PACKET) {
            for (int b = lane; b < o.len; b += 64) arena[o.dst + b] = bytes[o.src + b];
        } else if (o.kind == mot::ORDER_MOVE) {
            wave_copy(arena + o.dst, arena + o.src, o.len, lane);
        } else if (o.kind == mot::ORDER_SLIDE || o.kind == car::ORDER_OBJECT) {
            wave_copy(out + o.dst, arena + o.src, o.len, lane);
        } else if (o.kind == car::ORDER_DIRECTORY) {
            wave_copy(directory + o.dst, arena + o.src, o.len, lane);
        } else if (lane < mot::RECORD_BYTES / 4) {
            reinterpret_cast<int32_t *>(out + o.dst)[lane] = ord.record[o.src][lane];
        }
        __syncthreads();                                               // the next order, or the next walk, may read this one's bytes
    }
}

template <class K>
__global__ __launch_bounds__(64) void packet_walk_kernel(const PacketEntry *table, const CarouselExtra *extras, int n_cifs) {
    __shared__ typename K::State st;
    __shared__ typename K::Counters c;
    __shared__ mot::Orders ord;
    __shared__ __attribute__((aligned(16))) uint8_t bytes[pkt::MAX_PACKET_BYTES];
    const PacketEntry e = table[blockIdx.x];
    const CarouselExtra *extra = extras ? extras + blockIdx.x : nullptr;
    K sink(e, extra);
    const int lane = threadIdx.x, S = e.s, rw = packet_record_words(S);
    constexpr int STATE_WORDS = int(sizeof(typename K::State) / 16), COUNTER_WORDS = int(sizeof(typename K::Counters) / 4);
    for (int w = lane; w < STATE_WORDS; w += 64)
        reinterpret_cast<uint4 *>(&st)[w] = e.state_in ? reinterpret_cast<const uint4 *>(e.state_in)[w] : make_uint4(0u, 0u, 0u, 0u);
    for (int w = lane; w < COUNTER_WORDS; w += 64) reinterpret_cast<int32_t *>(&c)[w] = 0;
    __syncthreads();
    const uint32_t *records = reinterpret_cast<const uint32_t *>(e.records);
    // the scan's counters, a lane per frame
    int followed = 0, fec = 0, bad = 0, padding = 0, other = 0;
    for (int k = lane; k < n_cifs; k += 64) {
        const uint32_t n = records[size_t(k) * rw], w = records[size_t(k) * rw + 1];
        followed += int(n);
        fec += int(w & 0xFF);
        bad += int((w >> 8) & 0xFF);
        padding += int((w >> 16) & 0xFF);
        other += int(w >> 24);
    }
    for (int off = 1; off < 64; off <<= 1) {
        followed += __shfl_xor(followed, off);
        fec += __shfl_xor(fec, off);
        bad += __shfl_xor(bad, off);
        padding += __shfl_xor(padding, off);
        other += __shfl_xor(other, off);
    }
    if (lane == 0) {
        sink.sanitize(st);
        pkt::Counters &h = K::head(c);
        h.cifs = n_cifs;
        h.slots = n_cifs * S;
        h.slots_bad = bad;
        h.packets_fec = fec;
        h.packets_padding = padding;
        h.packets_other = other;
        h.packets_followed = followed;
    }
    uint8_t *arena = reinterpret_cast<uint8_t *>(e.arena), *out = reinterpret_cast<uint8_t *>(e.slides);
    uint8_t *directory = K::directory(extra);
    for (int k0 = 0; k0 < n_cifs; k0 += 64) {
        const int mine = k0 + lane;
        uint64_t busy = __ballot(mine < n_cifs && records[size_t(mine < n_cifs ? mine : 0) * rw] != 0);
        while (busy) {
            const int k = k0 + __ffsll(static_cast<unsigned long long>(busy)) - 1;
            busy &= busy - 1;
            const uint32_t *rec = records + size_t(k) * rw;
            const int n = int(rec[0]) < S ? int(rec[0]) : S;
            const uint8_t *frame = reinterpret_cast<const uint8_t *>(e.in) + size_t(k) * e.in_stride;
            for (int i = 0; i < n; i++) {
                const uint32_t w = rec[4 + i];
                int pos = int(w & 0xFF), L = int((w >> 8) & 0xFF);
                // (what the scan wrote; held inside the frame whatever the record says)
                L = L < 1 ? 1 : L > 4 ? 4 : L;
                L = L > S ? S : L;
                pos = pos + L > S ? S - L : pos;
                const uint8_t *src = frame + pkt::SLOT_BYTES * pos;
                __syncthreads();                                       // (the packet before has been read)
                if (lane < 3) bytes[lane] = src[lane];
                __syncthreads();
                const int need = pkt::packet_read_bytes(L, bytes[2]);
                for (int b = 3 + lane; b < need; b += 64) bytes[b] = src[b];
                __syncthreads();
                if (lane == 0) sink.follow(st, c, ord, bytes, L, k, pos);
                __syncthreads();
                execute_orders(ord, bytes, arena, out, directory, lane);
                sink.behind(st, c, ord, bytes, arena, out, directory, lane);
            }
        }
    }
    __syncthreads();
    if (lane == 0) K::finish(st, c);
    __syncthreads();
    for (int w = lane; w < STATE_WORDS; w += 64) reinterpret_cast<uint4 *>(e.state_out)[w] = reinterpret_cast<const uint4 *>(&st)[w];
    for (int w = lane; w < COUNTER_WORDS; w += 64) reinterpret_cast<int32_t *>(e.result)[w] = reinterpret_cast<const int32_t *>(&c)[w];
}

}  // namespace
}  // namespace dabk
#endif
