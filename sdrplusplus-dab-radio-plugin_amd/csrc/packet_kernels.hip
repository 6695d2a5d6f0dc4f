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
//
// The walk's body is a template over its sink (packet_walk_body.hpp): SlidesWalk here is dabgpu_packet_slides_dev (header
// mode: a closed group goes to the slideshow call's own code); dabgpu_packet_carousel_dev's sink and its instantiation are
// packet_carousel_kernels.hip.  The scan is the same launch for both.
#include "packet_walk_body.hpp"

namespace dabk {
namespace {

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

// header mode: dabgpu_packet_walk.h's follow_packet, nothing behind its orders
struct SlidesWalk {
    using State = pkt::State;
    using Counters = pkt::Counters;
    mot::Call call;
    __device__ __forceinline__ SlidesWalk(const PacketEntry &e, const CarouselExtra *) {
        call.body_capacity = e.body_capacity;
        call.max_slides = e.max_slides;
        call.slide_stride = e.slide_stride;
    }
    __device__ __forceinline__ static uint8_t *directory(const CarouselExtra *) { return nullptr; }
    __device__ __forceinline__ static pkt::Counters &head(Counters &c) { return c; }
    __device__ __forceinline__ void sanitize(State &st) const { pkt::sanitize(st, call.body_capacity); }
    __device__ __forceinline__ void follow(State &st, Counters &c, mot::Orders &ord, const uint8_t *bytes, int L, int k, int pos) {
        call.superframe = k;
        call.au = pos;
        pkt::follow_packet(st, c, ord, call, bytes, L);
    }
    __device__ __forceinline__ void behind(State &, Counters &, mot::Orders &, const uint8_t *, uint8_t *, uint8_t *, uint8_t *, int) {}
    __device__ __forceinline__ static void finish(const State &, Counters &) {}
};

size_t records_bytes(const PacketEntry &e, int n_cifs) { return size_t(n_cifs) * size_t(packet_record_words(e.s)) * 4; }
size_t table_part(int n_entries, bool carousel) {
    return size_t(n_entries) * (sizeof(PacketEntry) + (carousel ? sizeof(CarouselExtra) : 0));
}
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

size_t packet_table_bytes(const PacketEntry *entries, int n_entries, int n_cifs, bool carousel) {
    size_t bytes = table_part(n_entries, carousel);
    for (int i = 0; i < n_entries; i++) bytes += records_bytes(entries[i], n_cifs);
    return bytes;
}

uint64_t packet_scan_blocks(const PacketEntry *entries, int n_entries, int n_cifs) {
    return uint64_t(n_entries) * blocks_per_entry(entries, n_entries, n_cifs);
}

hipError_t launch_packet_scan(const PacketEntry *d_table, const PacketEntry *entries, int n_entries, int n_cifs, hipStream_t stream) {
    const uint64_t blocks = packet_scan_blocks(entries, n_entries, n_cifs);
    if (blocks >= (uint64_t(1) << 31)) return hipErrorInvalidValue;
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(packet_scan_kernel, dim3(unsigned(blocks)), dim3(64), 0, stream, d_table, n_cifs,
                       blocks_per_entry(entries, n_entries, n_cifs));
    return hipGetLastError();
}

hipError_t launch_packet_walk(PacketEntry *entries, const CarouselExtra *extras, int n_entries, int n_cifs, void *d_table,
                              size_t table_bytes, hipStream_t stream) {
    const bool carousel = extras != nullptr;
    if (n_entries <= 0) return hipSuccess;
    if (!d_table || n_cifs < 0 || n_cifs > pkt::MAX_N_CIFS || (reinterpret_cast<uintptr_t>(d_table) & 15)) return hipErrorInvalidValue;
    for (int i = 0; i < n_entries; i++) {
        const PacketEntry &e = entries[i];
        if (e.s < 1 || e.s > pkt::MAX_SLOTS || e.in_stride < uint64_t(pkt::SLOT_BYTES) * e.s || e.max_slides < 0 || e.body_capacity < 0 ||
            e.body_capacity > mot::BODY_CAP_MAX || (e.max_slides > 0 && uint64_t(e.max_slides) * e.slide_stride >= (uint64_t(1) << 31)))
            return hipErrorInvalidValue;
        if (carousel && (!extras[i].directory || !car::sizes_ok(extras[i].directory_capacity, extras[i].assemblies, e.body_capacity)))
            return hipErrorInvalidValue;
    }
    if (table_bytes < packet_table_bytes(entries, n_entries, n_cifs, carousel)) return hipErrorInvalidValue;
    const uint64_t blocks = packet_scan_blocks(entries, n_entries, n_cifs);
    if (blocks >= (uint64_t(1) << 31)) return hipErrorInvalidValue;
    size_t at = table_part(n_entries, carousel);
    for (int i = 0; i < n_entries; i++) {
        entries[i].records = uint64_t(reinterpret_cast<uintptr_t>(d_table)) + at;
        at += records_bytes(entries[i], n_cifs);
    }
    // (pageable memory: the copy has left `entries` when the call returns)
    const size_t entries_bytes = size_t(n_entries) * sizeof(PacketEntry);
    hipError_t err = hipMemcpyAsync(d_table, entries, entries_bytes, hipMemcpyHostToDevice, stream);
    if (err != hipSuccess) return err;
    const PacketEntry *table = static_cast<const PacketEntry *>(d_table);
    const CarouselExtra *d_extras = nullptr;
    if (carousel) {
        void *at_extras = static_cast<uint8_t *>(d_table) + entries_bytes;
        err = hipMemcpyAsync(at_extras, extras, size_t(n_entries) * sizeof(CarouselExtra), hipMemcpyHostToDevice, stream);
        if (err != hipSuccess) return err;
        d_extras = static_cast<const CarouselExtra *>(at_extras);
    }
    if (blocks > 0) {
        hipLaunchKernelGGL(packet_scan_kernel, dim3(unsigned(blocks)), dim3(64), 0, stream, table, n_cifs,
                           blocks_per_entry(entries, n_entries, n_cifs));
        err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    if (carousel) return launch_carousel_walk(table, d_extras, n_entries, n_cifs, stream);
    hipLaunchKernelGGL(packet_walk_kernel<SlidesWalk>, dim3(unsigned(n_entries)), dim3(64), 0, stream, table, d_extras, n_cifs);
    return hipGetLastError();
}

}  // namespace dabk
