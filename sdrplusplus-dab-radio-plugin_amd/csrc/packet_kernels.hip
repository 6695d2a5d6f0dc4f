// packet_kernels.hip -- packet-mode MOT services to slides (dabgpu_packet_slides_dev; contract and code:
// include/dabgpu_packet_walk.h, shared with the host twin; from the closed data group on: include/dabgpu_mot_walk.h).
//
// Scan: one lane per 24-byte slot, a wave64 takes 64 / S whole frames of S slots.  Each frame's bytes go into LDS by 16-byte
// loads (the frame sits in LDS at its own 16-byte phase, so an aligned load is an aligned store; the ragged first and last
// word go by bytes).  Every lane takes its slot for the start of a packet and computes length, address and the CRC verdict
// (crc16_step over LDS bytes, no table).  A lane stride of 24 bytes is 6 dwords: within a group of 32 lanes the byte reads
// meet 16 banks, a 2-way conflict.  It is accepted: the CRC step is six ALU operations to one LDS byte, the conflict hides
// behind them, and a swizzle would cost the 16-byte stores.  The first lane of each frame then resolves the chain from the
// verdicts in at most S steps (next = pos + (good ? L : 1)) and writes the frame's scan record: counters and the followed
// packets.  No atomics: the walk launch sums the records.
//
// Walk: one wave per entry, shaped like mot_slides_kernel.  The wave sums the records' counters (a lane per frame), finds the
// frames with followed packets by ballot, and per followed packet stages its header and useful bytes into LDS, lane 0 runs
// steps a .. g and close_group() over LDS and leaves copy orders, and all 64 lanes execute them.  Work is proportional to the
// followed packets.
#include <hip/hip_runtime.h>

#include "../../include/dabgpu_packet_walk.h"
#include "kernels.hpp"
#include "wave_copy.hpp"

namespace dabk {
namespace {

namespace mot = dabgpu_mot;
namespace pkt = dabgpu_packet;

static_assert(sizeof(pkt::State) % 16 == 0 && sizeof(pkt::Counters) % 4 == 0, "copied by words");

// a frame's room in LDS: its 24 S bytes at the phase (0 .. 15) its global address has, in whole 16-byte words
__device__ __forceinline__ int frame_room(int s) { return ((pkt::SLOT_BYTES * s + 15) & ~15) + 16; }
// 64 / S frames of frame_room(S) bytes: at most 1536 + 31 * 64 / S
constexpr int SCAN_LDS_BYTES = 3584;

__global__ __launch_bounds__(64) void packet_scan_kernel(const PacketEntry *table, int n_cifs, unsigned blocks_per_entry) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[SCAN_LDS_BYTES];
    __shared__ uint32_t verdicts[64];
    const unsigned entry = blockIdx.x / blocks_per_entry, block = blockIdx.x - entry * blocks_per_entry;
    const PacketEntry e = table[entry];
    const int lane = threadIdx.x, S = e.s, F = 64 / S;
    const int64_t f0 = int64_t(block) * F;
    if (f0 >= n_cifs) return;                                          // (an entry of larger S has more blocks than this one)
    const int nf = n_cifs - f0 < F ? int(n_cifs - f0) : F;
    const int room = frame_room(S), words = room / 16, bytes = pkt::SLOT_BYTES * S;
    const uint8_t *in = reinterpret_cast<const uint8_t *>(e.in) + size_t(f0) * e.in_stride;
    for (int idx = lane; idx < nf * words; idx += 64) {
        const int f = idx / words, w = idx - f * words;
        const uint8_t *src = in + size_t(f) * e.in_stride;
        const int a = int(reinterpret_cast<uintptr_t>(src) & 15), lo = 16 * w;   // the frame is [a, a + bytes) of its room
        uint8_t *dst = lds + f * room;
        const uint8_t *base = src - a;
        if (lo >= a && lo + 16 <= a + bytes) {
            *reinterpret_cast<uint4 *>(dst + lo) = *reinterpret_cast<const uint4 *>(base + lo);
        } else {
            const int b0 = lo > a ? lo : a, b1 = lo + 16 < a + bytes ? lo + 16 : a + bytes;
            for (int b = b0; b < b1; b++) dst[b] = base[b];
        }
    }
    __syncthreads();
    const int f = lane / S, pos = lane - f * S;
    const uint8_t *frame = nullptr;
    if (f < nf) {
        const int a = int(reinterpret_cast<uintptr_t>(in + size_t(f) * e.in_stride) & 15);
        frame = lds + f * room + a;
        verdicts[lane] = pkt::slot_verdict(frame, S, pos, e.fec);
    }
    __syncthreads();
    if (f < nf && pos == 0) {
        uint32_t *rec = reinterpret_cast<uint32_t *>(e.records) + size_t(f0 + f) * packet_record_words(S);
        pkt::FrameTally t = {};
        const uint32_t *v = verdicts + lane;
        uint32_t *list = rec + 4;
        pkt::resolve_chain(
            S, e.address, t, [&](int p) { return v[p]; },
            [&](int p, int L) {
                const uint8_t *h = frame + pkt::SLOT_BYTES * p;
                *list++ = uint32_t(p) | (uint32_t(L) << 8) | (uint32_t(h[0]) << 16) | (uint32_t(h[2]) << 24);
            });
        rec[0] = uint32_t(t.followed);
        rec[1] = uint32_t(t.fec) | (uint32_t(t.bad) << 8) | (uint32_t(t.padding) << 16) | (uint32_t(t.other) << 24);
        rec[2] = 0;
        rec[3] = 0;
    }
}

__global__ __launch_bounds__(64) void packet_walk_kernel(const PacketEntry *table, int n_cifs) {
    __shared__ pkt::State st;
    __shared__ pkt::Counters c;
    __shared__ mot::Orders ord;
    __shared__ __attribute__((aligned(16))) uint8_t bytes[pkt::MAX_PACKET_BYTES];
    const PacketEntry e = table[blockIdx.x];
    const int lane = threadIdx.x, S = e.s, rw = packet_record_words(S);
    constexpr int STATE_WORDS = int(sizeof(pkt::State) / 16);
    if (lane < STATE_WORDS)
        reinterpret_cast<uint4 *>(&st)[lane] = e.state_in ? reinterpret_cast<const uint4 *>(e.state_in)[lane] : make_uint4(0u, 0u, 0u, 0u);
    if (lane < int(sizeof(pkt::Counters) / 4)) reinterpret_cast<int32_t *>(&c)[lane] = 0;
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
        pkt::sanitize(st, e.body_capacity);
        c.cifs = n_cifs;
        c.slots = n_cifs * S;
        c.slots_bad = bad;
        c.packets_fec = fec;
        c.packets_padding = padding;
        c.packets_other = other;
        c.packets_followed = followed;
    }
    uint8_t *arena = reinterpret_cast<uint8_t *>(e.arena), *slides = reinterpret_cast<uint8_t *>(e.slides);
    mot::Call call;
    call.body_capacity = e.body_capacity;
    call.max_slides = e.max_slides;
    call.slide_stride = e.slide_stride;
    for (int k0 = 0; k0 < n_cifs; k0 += 64) {
        const int mine = k0 + lane;
        uint64_t busy = __ballot(mine < n_cifs && records[size_t(mine < n_cifs ? mine : 0) * rw] != 0);
        while (busy) {
            const int k = k0 + __ffsll(static_cast<unsigned long long>(busy)) - 1;
            busy &= busy - 1;
            const uint32_t *rec = records + size_t(k) * rw;
            const int n = int(rec[0]) < S ? int(rec[0]) : S;
            const uint8_t *frame = reinterpret_cast<const uint8_t *>(e.in) + size_t(k) * e.in_stride;
            call.superframe = k;
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
                if (lane == 0) {
                    call.au = pos;
                    pkt::follow_packet(st, c, ord, call, bytes, L);
                }
                __syncthreads();
                const int n_orders = ord.n;
                for (int j = 0; j < n_orders; j++) {
                    const mot::Order o = ord.o[j];
                    if (o.kind == pkt::ORDER_PACKET) {
                        for (int b = lane; b < o.len; b += 64) arena[o.dst + b] = bytes[o.src + b];
                    } else if (o.kind == mot::ORDER_MOVE) {
                        wave_copy(arena + o.dst, arena + o.src, o.len, lane);
                    } else if (o.kind == mot::ORDER_SLIDE) {
                        wave_copy(slides + o.dst, arena + o.src, o.len, lane);
                    } else if (lane < mot::RECORD_BYTES / 4) {
                        reinterpret_cast<int32_t *>(slides + o.dst)[lane] = ord.record[o.src][lane];
                    }
                    __syncthreads();                                   // the next order, or the next walk, may read this one's bytes
                }
            }
        }
    }
    __syncthreads();
    if (lane < STATE_WORDS) reinterpret_cast<uint4 *>(e.state_out)[lane] = reinterpret_cast<const uint4 *>(&st)[lane];
    if (lane < int(sizeof(pkt::Counters) / 4))
        reinterpret_cast<int32_t *>(e.result)[lane] = reinterpret_cast<const int32_t *>(&c)[lane];
}

size_t records_bytes(const PacketEntry &e, int n_cifs) { return size_t(n_cifs) * size_t(packet_record_words(e.s)) * 4; }
size_t table_part(int n_entries) { return size_t(n_entries) * sizeof(PacketEntry); }
unsigned blocks_per_entry(const PacketEntry *entries, int n_entries, int n_cifs) {
    unsigned most = 0;
    for (int i = 0; i < n_entries; i++) {
        const int F = 64 / entries[i].s;
        const unsigned blocks = unsigned((n_cifs + F - 1) / F);
        most = blocks > most ? blocks : most;
    }
    return most;
}

}  // namespace

size_t packet_table_bytes(const PacketEntry *entries, int n_entries, int n_cifs) {
    size_t bytes = table_part(n_entries);
    for (int i = 0; i < n_entries; i++) bytes += records_bytes(entries[i], n_cifs);
    return bytes;
}

uint64_t packet_scan_blocks(const PacketEntry *entries, int n_entries, int n_cifs) {
    return uint64_t(n_entries) * blocks_per_entry(entries, n_entries, n_cifs);
}

hipError_t launch_packet_slides(PacketEntry *entries, int n_entries, int n_cifs, void *d_table, size_t table_bytes, hipStream_t stream) {
    if (n_entries <= 0) return hipSuccess;
    if (!d_table || n_cifs < 0 || n_cifs > pkt::MAX_N_CIFS || (reinterpret_cast<uintptr_t>(d_table) & 15)) return hipErrorInvalidValue;
    for (int i = 0; i < n_entries; i++) {
        const PacketEntry &e = entries[i];
        if (e.s < 1 || e.s > pkt::MAX_SLOTS || e.in_stride < uint64_t(pkt::SLOT_BYTES) * e.s || e.max_slides < 0 || e.body_capacity < 0 ||
            e.body_capacity > mot::BODY_CAP_MAX || (e.max_slides > 0 && uint64_t(e.max_slides) * e.slide_stride >= (uint64_t(1) << 31)))
            return hipErrorInvalidValue;
    }
    if (table_bytes < packet_table_bytes(entries, n_entries, n_cifs)) return hipErrorInvalidValue;
    const uint64_t blocks = packet_scan_blocks(entries, n_entries, n_cifs);
    if (blocks >= (uint64_t(1) << 31)) return hipErrorInvalidValue;
    size_t at = table_part(n_entries);
    for (int i = 0; i < n_entries; i++) {
        entries[i].records = uint64_t(reinterpret_cast<uintptr_t>(d_table)) + at;
        at += records_bytes(entries[i], n_cifs);
    }
    // (pageable memory: the copy has left `entries` when the call returns)
    hipError_t err = hipMemcpyAsync(d_table, entries, table_part(n_entries), hipMemcpyHostToDevice, stream);
    if (err != hipSuccess) return err;
    const PacketEntry *table = static_cast<const PacketEntry *>(d_table);
    if (blocks > 0) {
        hipLaunchKernelGGL(packet_scan_kernel, dim3(unsigned(blocks)), dim3(64), 0, stream, table, n_cifs,
                           blocks_per_entry(entries, n_entries, n_cifs));
        err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    hipLaunchKernelGGL(packet_walk_kernel, dim3(unsigned(n_entries)), dim3(64), 0, stream, table, n_cifs);
    return hipGetLastError();
}

}  // namespace dabk
