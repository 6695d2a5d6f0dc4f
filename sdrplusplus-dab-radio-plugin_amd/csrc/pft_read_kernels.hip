// pft_read_kernels.hip -- PF fragment byte streams put back together into AF packets (include/dabgpu.h, "EDI PFT layer"; the
// contract and every scalar step: include/dabgpu_pft.h).  Per entry S = the state's tail + the new bytes.
//
// pft_read_check_kernel   the parallel part of the walk: a lane per byte position, 4096 positions per workgroup, an entry per
//                         grid row.  Every position is judged by the header's position_status (the HCRC covers at most 18
//                         bytes).  A wave owns the 64-position words of the two bitmaps it leaves -- `good` (T of the
//                         contract) and `stop` (an incomplete fragment or a cut header: the walk ends there) -- and writes
//                         every one of them: no clearing pass, no atomics.
// pft_read_walk_kernel    a wave per entry walks the bitmaps (the next set bit by ballot and find-first over 64 words at a
//                         time).  The two open groups live in LDS: heads and 2 x 10496 buffer bytes.  Per taken fragment lane
//                         0 runs the header's scalar steps (horizon, late run, join) on the LDS record and all 64 lanes move
//                         the payload; when a group closes, a lane per chunk counts its erased positions (a step per missing fragment), lane 0 makes the
//                         record, and all lanes move the packet out (a complete group: no RS arithmetic) or, for a group to be
//                         filled, its received map and fragments into the entry's arena.  Records, offsets and counters follow
//                         from the walk's own order: no scan, no atomics.  The serial part is one step per fragment.
// pft_read_fill_kernel    a workgroup per emitted record (a grid row per entry, strided over its records).  A group to be
//                         filled is de-interleaved from the arena into LDS; a wave per chunk finds the erased positions by
//                         ballot against the received map, computes a syndrome per lane, the erasure locator by 48 shifted
//                         multiply-adds across lanes, the evaluator and Forney's values a coefficient / a position per lane,
//                         and holds the filled chunk to all 48 syndromes; the packet then leaves LDS for the output.  Every
//                         emitted packet has its AF header judged and its CRC folded a chunk of bytes per lane.
#include "kernels.hpp"

#include <algorithm>

#include "../../include/dabgpu_pft.h"

namespace dabk {

namespace {

namespace pf = dabgpu_pft;

constexpr int CHECK_WG = 256;
constexpr int FILL_WG = 256;
constexpr int FILL_WAVES = FILL_WG / 64;
constexpr uint32_t POLY = 0x11021u;
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint32_t NO_ARENA = 0xFFFFFFFFu;
static_assert(PFT_READ_SPAN % CHECK_WG == 0 && CHECK_WG % 64 == 0, "a wave owns whole bitmap words");
static_assert(PFT_READ_MAX_TAIL == pf::MAX_TAIL && PFT_READ_MAX_BLOCK == pf::MAX_BLOCK, "kernels.hpp sizes the scratch with these");

__device__ const pf::Gf GF_TABLES = pf::make_gf();

// S of an entry in global memory: the tail of the state record, then the new bytes
struct StreamBytes {
    const uint8_t *tail, *fresh;
    uint32_t t;                                // tail length
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return i < t ? tail[i] : fresh[i - t]; }
};
struct StreamAt {
    StreamBytes s;
    uint32_t q;
    __device__ __forceinline__ uint32_t operator()(int i) const { return s(q + uint32_t(i)); }
};
struct LdsBytes {
    const uint8_t *p;
    __device__ __forceinline__ uint32_t operator()(int i) const { return p[i]; }
};

__device__ __forceinline__ StreamBytes stream_of(const PftReadEntry &e) {
    StreamBytes s;
    const uint8_t *in = reinterpret_cast<const uint8_t *>(uintptr_t(e.state_in));
    s.tail = in ? in + pf::STATE_TAIL_AT : nullptr;
    s.t = in ? pf::clamp_tail(reinterpret_cast<const pf::Head *>(in)->tail_bytes) : 0u;
    s.fresh = reinterpret_cast<const uint8_t *>(uintptr_t(e.bytes));
    return s;
}

__global__ __launch_bounds__(CHECK_WG) void pft_read_check_kernel(const PftReadEntry *entries) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const PftReadEntry &e = entries[blockIdx.y];
    const StreamBytes S = stream_of(e);
    const uint32_t len = S.t + uint32_t(e.n_bytes);
    const uint32_t b0 = blockIdx.x * uint32_t(PFT_READ_SPAN);
    unsigned long long *good = reinterpret_cast<unsigned long long *>(uintptr_t(e.good));
    unsigned long long *stop = reinterpret_cast<unsigned long long *>(uintptr_t(e.stop));
    for (int it = 0; it < PFT_READ_SPAN / CHECK_WG; it++) {
        const uint32_t q0 = b0 + uint32_t(it * CHECK_WG + wave * 64), q = q0 + uint32_t(lane);
        if (q0 >= len) break;                                                  // (uniform in the wave; words at and above len are not read)
        int status = 0;
        if (q < len) {
            pf::FragHeader h;
            status = pf::position_status(StreamAt{S, q}, min(len - q, uint32_t(pf::MAX_TAIL) + 1u), h);
        }
        const unsigned long long t_word = __ballot(status == 2), s_word = __ballot(status == 1);
        if (lane == 0) {
            good[q0 / 64u] = t_word;
            stop[q0 / 64u] = s_word;
        }
    }
}

// the smallest set bit at or above `from` in the first `words` words, or NONE
__device__ __forceinline__ uint32_t next_bit(const unsigned long long *bitmap, uint32_t words, uint32_t from, int lane) {
    const uint32_t w0 = from >> 6;
    for (uint32_t base = w0; base < words; base += 64) {
        const uint32_t w = base + uint32_t(lane);
        unsigned long long v = w < words ? bitmap[w] : 0ull;
        if (w == w0) v &= ~0ull << (from & 63u);
        const unsigned long long any = __ballot(v != 0ull);
        if (any) {
            const int first = __ffsll(any) - 1;
            const uint32_t lo = uint32_t(__shfl(int(uint32_t(v)), first, 64)), hi = uint32_t(__shfl(int(uint32_t(v >> 32)), first, 64));
            const int bit = lo ? __ffs(int(lo)) - 1 : 32 + __ffs(int(hi)) - 1;
            return (base + uint32_t(first)) * 64u + uint32_t(bit);
        }
    }
    return NONE;
}

// what the walk's wave keeps in LDS
struct WalkLds {
    __attribute__((aligned(16))) uint8_t buf[2][pf::MAX_BLOCK];
    pf::Walk w;
    int32_t n_close, close_slot[2], next;
    pf::Move mv;
    int32_t kind;                              // of the group being closed: pf::CloseKind
    uint32_t offset, length, arena_at;         // its place in the output; in the arena (NO_ARENA: no room, never reached)
    uint32_t arena_used;
};

__device__ __forceinline__ void zero_buffer(WalkLds &sh, int slot, int lane) {
    uint4 *b = reinterpret_cast<uint4 *>(sh.buf[slot]);
    for (int i = lane; i < pf::MAX_BLOCK / 16; i += 64) b[i] = make_uint4(0u, 0u, 0u, 0u);
}

// a complete group's packet, out of its buffer into the output: whole words between the unaligned ends
__device__ __forceinline__ void move_packet_out(const WalkLds &sh, int slot, uint8_t *out, uint32_t offset, uint32_t length, int lane) {
    const pf::GroupHead &g = sh.w.g[slot];
    const uint8_t *buf = sh.buf[slot];
    const uint32_t end = offset + length, F = g.fcount, s = g.s;
    if (g.fec) {
        // packet byte t lies in fragment t % F at t / F: the pair is carried along, not divided out per byte
        const uint32_t a0 = (offset & ~3u) + 4u * uint32_t(lane);
        uint32_t t = a0 >= offset ? a0 - offset : 0u;                          // (the first word's bytes in front of the packet are passed over)
        uint32_t fr = t % F, at = t / F;
        const uint32_t df = 256u % F, da = 256u / F;
        for (uint32_t a = a0; a < end; a += 256u) {
            uint32_t v = 0, fb = fr, ab = at;
            const bool whole = a >= offset && a + 4u <= end;
            for (uint32_t b = 0; b < 4u; b++) {
                if (a + b < offset || a + b >= end) continue;
                const uint32_t x = buf[fb * s + ab];
                if (whole) v |= x << (8u * b);
                else out[a + b] = uint8_t(x);
                if (++fb == F) {
                    fb = 0;
                    ab++;
                }
            }
            if (whole) *reinterpret_cast<uint32_t *>(out + a) = v;
            // 256 bytes on (the first word may have begun inside: its t was 0, not a - offset)
            const uint32_t step = a >= offset ? 256u : 256u - (offset - a);
            if (step == 256u) {
                fr += df;
                at += da;
                if (fr >= F) {
                    fr -= F;
                    at++;
                }
            } else {
                t = step;
                fr = t % F;
                at = t / F;
            }
        }
        return;
    }
    const uint32_t body = (F - 1u) * s, last_at = uint32_t(pf::MAX_BLOCK) - g.last_len;
    for (uint32_t a = (offset & ~3u) + 4u * uint32_t(lane); a < end; a += 256u) {
        uint32_t v = 0;
        const bool whole = a >= offset && a + 4u <= end;
        for (uint32_t b = 0; b < 4u; b++) {
            if (a + b < offset || a + b >= end) continue;
            const uint32_t t = a + b - offset, x = buf[t < body ? t : last_at + (t - body)];
            if (whole) v |= x << (8u * b);
            else out[a + b] = uint8_t(x);
        }
        if (whole) *reinterpret_cast<uint32_t *>(out + a) = v;
    }
}

// closing the group of `slot`, which holds a fragment (contract: "Closing a group")
__device__ __forceinline__ void close_group(WalkLds &sh, const PftReadEntry &e, int slot, uint32_t extra, bool advance, int lane) {
    const pf::GroupHead &g = sh.w.g[slot];
    int er = 0;
    if (g.fec && g.received < g.fcount && lane < int(g.chunks)) er = pf::chunk_erasures(g, lane);
    int worst = er, erased = er;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        worst = max(worst, __shfl_xor(worst, d, 64));
        erased += __shfl_xor(erased, d, 64);
    }
    const int with = __popcll(__ballot(er > 0));
    if (lane == 0) {
        pf::Record r;
        const int kind = pf::close_record(sh.w, slot, worst, with, erased, extra, r);
        uint32_t arena_at = NO_ARENA;
        if (kind == pf::CLOSE_FILL) {
            const uint32_t item = 32u + uint32_t(g.received) * g.s;
            if (sh.arena_used + item <= e.arena_bytes) {
                arena_at = sh.arena_used;
                sh.arena_used += item;
            }
        }
        // (records <= max_records and the packet fits always: both are sized by what S and the carried groups can hold; the
        // tests only keep a table this code did not fill from writing outside the outputs.  A packet that did not fit, or a
        // group to fill without room in the arena, would leave as a LOST record of no bytes, its reserved words zero)
        const bool fits = uint64_t(r.offset) + r.length <= pf::read_out_bytes(uint32_t(e.n_bytes)) && (kind != pf::CLOSE_FILL || arena_at != NO_ARENA);
        if (!fits) {
            r.flags = uint16_t((r.flags & ~uint32_t(pf::FLAG_RECOVERED)) | pf::FLAG_LOST);
            r.length = 0;
        }
        if (sh.w.c.records <= e.max_records) {
            pf::Record *out = reinterpret_cast<pf::Record *>(uintptr_t(e.records)) + (sh.w.c.records - 1u);
            out->offset = r.offset;
            out->length = r.length;
            out->pseq = r.pseq;
            out->fcount = r.fcount;
            out->received = r.received;
            out->plen = r.plen;
            out->rs_k = r.rs_k;
            out->rs_z = r.rs_z;
            out->chunks = r.chunks;
            out->max_erasures = r.max_erasures;
            out->flags = r.flags;
            out->source = r.source;
            out->dest = r.dest;
            out->reserved_a = fits && kind == pf::CLOSE_FILL ? arena_at : 0u;  // (the fill launch reads it, then writes 0, on every path)
            out->reserved_b = 0;
        }
        sh.kind = fits ? kind : int(pf::CLOSE_LOST);
        sh.offset = r.offset;
        sh.length = r.length;
        sh.arena_at = arena_at;
    }
    __syncthreads();
    if (sh.kind == pf::CLOSE_COPY) {
        move_packet_out(sh, slot, reinterpret_cast<uint8_t *>(uintptr_t(e.out)), sh.offset, sh.length, lane);
    } else if (sh.kind == pf::CLOSE_FILL && sh.arena_at != NO_ARENA) {
        uint8_t *item = reinterpret_cast<uint8_t *>(uintptr_t(e.arena)) + sh.arena_at;
        if (lane < 32) item[lane] = uint8_t(g.map[lane >> 3] >> (8 * (lane & 7)));
        const uint32_t s = g.s;
        uint32_t rank = 0;
        for (uint32_t f = 0; f < g.fcount; f++) {
            if (!pf::held(g, f)) continue;
            for (uint32_t i = uint32_t(lane); i < s; i += 64) item[32u + rank * s + i] = sh.buf[slot][f * s + i];
            rank++;
        }
    }
    __syncthreads();
    zero_buffer(sh, slot, lane);
    if (lane == 0) pf::close_done(sh.w, slot, advance);
    __syncthreads();
}

__global__ __launch_bounds__(64) void pft_read_walk_kernel(const PftReadEntry *entries) {
    __shared__ WalkLds sh;
    const int lane = threadIdx.x;
    const PftReadEntry &e = entries[blockIdx.x];
    const StreamBytes S = stream_of(e);
    const uint32_t len = S.t + uint32_t(e.n_bytes), words = (len + 63u) / 64u;
    const unsigned long long *good = reinterpret_cast<const unsigned long long *>(uintptr_t(e.good));
    const unsigned long long *stop = reinterpret_cast<const unsigned long long *>(uintptr_t(e.stop));
    const uint8_t *state_in = reinterpret_cast<const uint8_t *>(uintptr_t(e.state_in));
    uint8_t *state_out = reinterpret_cast<uint8_t *>(uintptr_t(e.state_out));
    pf::Head in{};
    if (state_in) in = *reinterpret_cast<const pf::Head *>(state_in);
    // the carried groups: heads, held to what this code writes, then the buffers of those that stay
    if (lane < 2 * pf::GROUP_HEAD_BYTES / 4) {
        const int j = lane / (pf::GROUP_HEAD_BYTES / 4), w = lane % (pf::GROUP_HEAD_BYTES / 4);
        reinterpret_cast<uint32_t *>(&sh.w.g[j])[w] =
            state_in ? reinterpret_cast<const uint32_t *>(state_in + pf::STATE_GROUPS_AT + j * pf::GROUP_BYTES)[w] : 0u;
    }
    __syncthreads();
    if (lane == 0) {
        pf::walk_begin(sh.w, in);
        for (int j = 0; j < 2; j++) pf::sanitize(sh.w.g[j], j, sh.w.have_horizon != 0, sh.w.horizon);
        sh.arena_used = 0;
    }
    __syncthreads();
    for (int j = 0; j < 2; j++) {
        const bool keep = state_in && sh.w.g[j].kind == pf::GROUP_OPEN;
        const uint4 *src = reinterpret_cast<const uint4 *>(state_in + pf::STATE_GROUPS_AT + j * pf::GROUP_BYTES + pf::GROUP_HEAD_BYTES);
        uint4 *dst = reinterpret_cast<uint4 *>(sh.buf[j]);
        for (int i = lane; i < pf::MAX_BLOCK / 16; i += 64) dst[i] = keep ? src[i] : make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();
    bool in_skip = in.in_skip != 0;
    uint32_t p = 0, skipped = 0, resyncs = 0;
    for (;;) {
        if (!(p < len && ((good[p >> 6] >> (p & 63u)) & 1ull))) {
            const uint32_t qt = next_bit(good, words, p, lane), qs = next_bit(stop, words, p, lane);
            const uint32_t q = min(min(qt, qs), len);
            if (q > p) {
                skipped += q - p;
                in_skip = true;
                p = q;
            }
            if (p >= len || qs <= qt) break;
        }
        if (in_skip) {
            resyncs++;
            in_skip = false;
        }
        // (the check launch has held this position to T: the header is read again, bounded all the same)
        pf::FragHeader h;
        if (!pf::header_ok(StreamAt{S, p}, min(len - p, 64u), h) || p + h.header_bytes + h.plen > len) break;
        if (lane == 0) sh.n_close = pf::before_join(sh.w, h, sh.close_slot);
        __syncthreads();
        const int n_close = sh.n_close;
        if (n_close >= 0) {
            for (int i = 0; i < n_close; i++) close_group(sh, e, sh.close_slot[i], 0u, false, lane);
            if (lane == 0) sh.mv = pf::join(sh.w, h);
            __syncthreads();
            const int slot = sh.mv.slot;
            const uint32_t at = sh.mv.at, n = sh.mv.n;
            if (sh.mv.clear) zero_buffer(sh, slot, lane);
            if (n && at + n <= uint32_t(pf::MAX_BLOCK)) {
                const uint32_t from = p + h.header_bytes;
                for (uint32_t i = uint32_t(lane); i < n; i += 64) sh.buf[slot][at + i] = uint8_t(S(from + i));
            }
            for (;;) {
                __syncthreads();
                if (lane == 0) sh.next = pf::next_complete(sh.w);
                __syncthreads();
                const int next = sh.next;
                if (next < 0) break;
                close_group(sh, e, next, 0u, true, lane);
            }
        } else {
            __syncthreads();                                                   // (n_close is read before the next fragment writes it)
        }
        p += h.header_bytes + h.plen;
    }
    if (e.flags & int32_t(pf::READ_FLUSH)) {
        __syncthreads();
        if (lane == 0) sh.n_close = pf::flush_list(sh.w, sh.close_slot);
        __syncthreads();
        const int n_close = sh.n_close;
        for (int i = 0; i < n_close; i++) close_group(sh, e, sh.close_slot[i], pf::FLAG_FLUSHED, false, lane);
    }
    __syncthreads();
    if (lane == 0) {
        sh.w.c.skipped = skipped;
        sh.w.c.resyncs = resyncs;
        sh.w.c.tail_bytes = len - p;
        const pf::Result &c = sh.w.c;
        // (field by field: a copy of the whole record may be kept in scratch memory)
        pf::Result *out = reinterpret_cast<pf::Result *>(uintptr_t(e.result));
        out->records = c.records;
        out->packets = c.packets;
        out->lost = c.lost;
        out->recovered = c.recovered;
        out->fragments = c.fragments;
        out->duplicates = c.duplicates;
        out->mismatched = c.mismatched;
        out->late = c.late;
        out->unsupported = c.unsupported;
        out->missing = c.missing;
        out->skipped = c.skipped;
        out->resyncs = c.resyncs;
        out->out_bytes = c.out_bytes;
        out->tail_bytes = c.tail_bytes;
        out->chunks_filled = c.chunks_filled;
        out->bytes_filled = c.bytes_filled;
        *reinterpret_cast<pf::Head *>(state_out) = pf::next_head(in, sh.w, in_skip);
    }
    // the open groups: heads and buffers, as whole words
    if (lane < 2 * pf::GROUP_HEAD_BYTES / 4) {
        const int j = lane / (pf::GROUP_HEAD_BYTES / 4), w = lane % (pf::GROUP_HEAD_BYTES / 4);
        reinterpret_cast<uint32_t *>(state_out + pf::STATE_GROUPS_AT + j * pf::GROUP_BYTES)[w] = reinterpret_cast<const uint32_t *>(&sh.w.g[j])[w];
    }
    for (int j = 0; j < 2; j++) {
        uint4 *dst = reinterpret_cast<uint4 *>(state_out + pf::STATE_GROUPS_AT + j * pf::GROUP_BYTES + pf::GROUP_HEAD_BYTES);
        const uint4 *src = reinterpret_cast<const uint4 *>(sh.buf[j]);
        for (int i = lane; i < pf::MAX_BLOCK / 16; i += 64) dst[i] = src[i];
    }
    // the new tail: S[p ..), zeros behind it, as whole words
    uint32_t *tail = reinterpret_cast<uint32_t *>(state_out + pf::STATE_TAIL_AT);
    const uint32_t kept = len - p;
    for (uint32_t w = uint32_t(lane); w < uint32_t(pf::STATE_TAIL_ROOM / 4); w += 64) {
        uint32_t v = 0;
        for (uint32_t b = 0; b < 4; b++)
            if (4 * w + b < kept) v |= S(p + 4 * w + b) << (8 * b);
        tail[w] = v;
    }
}

// ---- the fill launch -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t gf_mul16(uint32_t a, uint32_t b) {
    uint32_t r = 0;
    for (int i = 15; i >= 0; i--) {
        r <<= 1;
        if (r & 0x10000u) r ^= POLY;
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}
__device__ __forceinline__ uint32_t gf_xpow(uint32_t n) {
    uint32_t r = 1, sq = 2;
    for (; n; n >>= 1) {
        if (n & 1u) r = gf_mul16(r, sq);
        sq = gf_mul16(sq, sq);
    }
    return r;
}
// v alpha^e, 0 <= e < 255
__device__ __forceinline__ uint32_t mul_exp(const pf::Gf &g, uint32_t v, uint32_t e) { return v ? g.exp[g.log[v] + e] : 0u; }

// what a wave keeps of the chunk it fills
struct ChunkLds {
    uint8_t pos[pf::PARITY], xlog[pf::PARITY], syn[pf::PARITY], gamma[64], omega[pf::PARITY], y[pf::PARITY];
};

__global__ __launch_bounds__(FILL_WG) void pft_read_fill_kernel(const PftReadEntry *entries) {
    __shared__ pf::Gf g;
    __shared__ __attribute__((aligned(16))) uint8_t s_blk[pf::MAX_BLOCK];
    __shared__ uint16_t s_tab[256];
    __shared__ uint8_t s_rank[pf::MAX_FRAGMENTS];
    __shared__ unsigned long long s_map[4];
    __shared__ ChunkLds s_chunk[FILL_WAVES];
    __shared__ uint32_t s_crc[FILL_WAVES];
    __shared__ int s_bad;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 192) reinterpret_cast<uint32_t *>(&g)[tid] = reinterpret_cast<const uint32_t *>(&GF_TABLES)[tid];
    {
        uint32_t r = uint32_t(tid) << 8;
#pragma unroll
        for (int i = 0; i < 8; i++) r = (r & 0x8000u) ? ((r << 1) ^ POLY) & 0xffffu : (r << 1);
        s_tab[tid] = uint16_t(r);
    }
    const PftReadEntry &e = entries[blockIdx.y];
    const uint32_t n_records = min(reinterpret_cast<const pf::Result *>(uintptr_t(e.result))->records, e.max_records);
    uint8_t *out = reinterpret_cast<uint8_t *>(uintptr_t(e.out));
    const uint64_t out_room = pf::read_out_bytes(uint32_t(e.n_bytes));
    ChunkLds &ck = s_chunk[wave];
    for (uint32_t r = blockIdx.x; r < n_records; r += gridDim.x) {
        pf::Record *rec = reinterpret_cast<pf::Record *>(uintptr_t(e.records)) + r;
        const uint32_t offset = rec->offset, l = rec->length, flags = rec->flags, arena_at = rec->reserved_a;
        if (l == 0u || l > uint32_t(pf::MAX_BLOCK) || uint64_t(offset) + l > out_room) {               // LOST (the rest: never)
            if (tid == 0 && arena_at) rec->reserved_a = 0;
            continue;
        }
        __syncthreads();                                                       // the tables; the record before this one is done with
        if (tid == 0) s_bad = 0;
        const bool fill = (flags & pf::FLAG_RECOVERED) != 0u;
        if (!fill) {
            for (uint32_t t = uint32_t(tid); t < l; t += FILL_WG) s_blk[t] = out[offset + t];
        } else {
            const uint32_t F = rec->fcount, s = rec->plen, k = rec->rs_k, c = rec->chunks, n = k + uint32_t(pf::PARITY), B = c * n;
            const uint32_t held_n = rec->received;
            // (a record the walk made: F s <= MAX_BLOCK, c = F s / n; held to that all the same)
            const bool sound = arena_at != NO_ARENA && F >= 1u && F <= uint32_t(pf::MAX_FRAGMENTS) && k >= 1u && k <= uint32_t(pf::RS_K) && F * s <= uint32_t(pf::MAX_BLOCK) &&
                               B <= F * s && l <= c * k && uint64_t(arena_at) + 32u + uint64_t(held_n) * s <= e.arena_bytes;
            if (!sound) {                                                      // (never: the record leaves without AF_OK, its reserved word zero)
                if (tid == 0) rec->reserved_a = 0;
                continue;
            }
            const uint8_t *item = reinterpret_cast<const uint8_t *>(uintptr_t(e.arena)) + arena_at;
            if (tid < 4) {
                unsigned long long v = 0;
                for (int b = 0; b < 8; b++) v |= (unsigned long long)(item[8 * tid + b]) << (8 * b);
                s_map[tid] = v;
            }
            __syncthreads();
            {
                // the rank of fragment tid among the held ones
                uint32_t rank = 0;
                for (int w = 0; w < 4; w++) {
                    const unsigned long long m = s_map[w];
                    if (tid >= 64 * (w + 1)) rank += uint32_t(__popcll(m));
                    else if (tid > 64 * w) rank += uint32_t(__popcll(m & ((1ull << (tid - 64 * w)) - 1ull)));
                }
                s_rank[tid] = uint8_t(min(rank, held_n ? held_n - 1u : 0u));
            }
            __syncthreads();
            {
                // block byte idx lies in fragment idx % F at idx / F
                uint32_t fr = uint32_t(tid) % F, at = uint32_t(tid) / F;
                const uint32_t df = uint32_t(FILL_WG) % F, da = uint32_t(FILL_WG) / F;
                for (uint32_t idx = uint32_t(tid); idx < B; idx += FILL_WG) {
                    const bool have = (s_map[fr >> 6] >> (fr & 63u)) & 1ull;
                    s_blk[idx] = have ? item[32u + uint32_t(s_rank[fr]) * s + at] : uint8_t(0);
                    fr += df;
                    at += da;
                    if (fr >= F) {
                        fr -= F;
                        at++;
                    }
                }
            }
            __syncthreads();
            // a wave per chunk, every wave the same number of rounds
            for (uint32_t i0 = 0; i0 < c; i0 += FILL_WAVES) {
                const uint32_t i = i0 + uint32_t(wave);
                const bool active = i < c;
                int ne = 0;
                if (active) {
                    for (uint32_t j0 = 0; j0 < n; j0 += 64) {
                        const uint32_t j = j0 + uint32_t(lane);
                        bool er = false;
                        if (j < n) {
                            const uint32_t f = uint32_t(pf::block_index(int(c), int(k), int(i), int(j))) % F;
                            er = !((s_map[f >> 6] >> (f & 63u)) & 1ull);
                        }
                        const unsigned long long b = __ballot(er);
                        const int at = ne + __popcll(b & ((1ull << lane) - 1ull));
                        if (er && at < pf::PARITY) ck.pos[at] = uint8_t(j);
                        ne += __popcll(b);
                    }
                }
                const bool work = active && ne > 0 && ne <= pf::PARITY;         // (more than 48: the walk holds such a group LOST)
                const uint32_t e_n = uint32_t(ne);
                __syncthreads();
                if (work) {
                    if (lane < pf::PARITY) {
                        // syndrome `lane`: the codeword at alpha^(FIRST_ROOT + lane), erased positions read as zero
                        const uint32_t root = uint32_t(pf::FIRST_ROOT + lane) % 255u;
                        uint32_t acc = 0;
                        for (uint32_t j = 0; j < k; j++) acc = mul_exp(g, acc, root) ^ s_blk[i * k + j];
                        for (uint32_t j = 0; j < uint32_t(pf::PARITY); j++) acc = mul_exp(g, acc, root) ^ s_blk[c * k + uint32_t(pf::PARITY) * i + j];
                        ck.syn[lane] = uint8_t(acc);
                    }
                    if (uint32_t(lane) < e_n) ck.xlog[lane] = uint8_t(n - 1u - ck.pos[lane]);
                }
                __syncthreads();
                if (work) {
                    // the locator prod (1 + X_u x): lane j holds the coefficient of x^j
                    uint32_t gam = lane == 0 ? 1u : 0u;
                    for (uint32_t u = 0; u < e_n; u++) {
                        uint32_t prev = uint32_t(__shfl_up(int(gam), 1, 64));
                        if (lane == 0) prev = 0;
                        gam ^= mul_exp(g, prev, ck.xlog[u]);
                    }
                    ck.gamma[lane] = uint8_t(gam);
                }
                __syncthreads();
                if (work && uint32_t(lane) < e_n) {
                    // the evaluator: syndromes 1 .. e times the locator, modulo x^e
                    uint32_t om = 0;
                    for (int q = 0; q <= lane; q++) om ^= pf::gmul(g, ck.syn[q], ck.gamma[lane - q]);
                    ck.omega[lane] = uint8_t(om);
                }
                __syncthreads();
                if (work && uint32_t(lane) < e_n) {
                    // Forney: the value at this lane's position
                    const uint32_t x = ck.xlog[lane], xinv = (255u - x) % 255u;
                    uint32_t num = 0, den = 1;
                    for (int q = int(e_n) - 1; q >= 0; q--) num = mul_exp(g, num, xinv) ^ ck.omega[q];
                    for (uint32_t v = 0; v < e_n; v++)
                        if (v != uint32_t(lane)) den = pf::gmul(g, den, 1u ^ g.exp[(uint32_t(ck.xlog[v]) + xinv) % 255u]);
                    const uint32_t y = pf::gdiv(g, num, mul_exp(g, den, x * uint32_t(pf::FIRST_ROOT) % 255u));
                    ck.y[lane] = uint8_t(y);
                    s_blk[pf::block_index(int(c), int(k), int(i), int(ck.pos[lane]))] = uint8_t(y);
                }
                __syncthreads();
                if (work) {
                    // all 48 syndromes of the filled chunk
                    uint32_t after = 0;
                    if (lane < pf::PARITY) {
                        after = ck.syn[lane];
                        for (uint32_t v = 0; v < e_n; v++) after ^= mul_exp(g, ck.y[v], uint32_t(ck.xlog[v]) * uint32_t(pf::FIRST_ROOT + lane) % 255u);
                    }
                    if (__ballot(after != 0u) && lane == 0) s_bad = 1;
                }
                __syncthreads();
            }
            for (uint32_t t = uint32_t(tid); t < l; t += FILL_WG) out[offset + t] = s_blk[t];
        }
        __syncthreads();
        // AF_OK: the header, 12 + LEN == l, and the CRC over the l - 2 bytes in front of it: zero bytes in front up to 256
        // equal chunks, a chunk per lane, each chunk's way to the end x^(8 n) mod P
        int total = 0;
        bool af = l >= uint32_t(dabgpu_edi::AF_OVERHEAD) && l <= uint32_t(pf::MAX_PACKET) && dabgpu_edi::header_ok(LdsBytes{s_blk}, total) &&
                  uint32_t(total) == l;
        if (af) {
            const uint32_t L = l - 2u, cb = (L + uint32_t(FILL_WG) - 1u) / uint32_t(FILL_WG), lead = uint32_t(FILL_WG) * cb - L;
            uint32_t crc = 0;
            for (uint32_t j = 0; j < cb; j++) {
                const uint32_t m = uint32_t(tid) * cb + j;
                if (m >= lead) crc = ((crc << 8) & 0xffffu) ^ s_tab[(crc >> 8) ^ s_blk[m - lead]];
            }
            uint32_t sum = gf_mul16(crc, gf_xpow(8u * cb * uint32_t(FILL_WG - 1 - tid)));
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) sum ^= uint32_t(__shfl_xor(int(sum), d, 64));
            if (lane == 0) s_crc[wave] = sum;
            __syncthreads();
            sum = s_crc[0] ^ s_crc[1] ^ s_crc[2] ^ s_crc[3];
            sum = (sum ^ gf_mul16(0xFFFFu, gf_xpow(8u * L)) ^ 0xffffu) & 0xffffu;
            af = sum == ((uint32_t(s_blk[L]) << 8) | s_blk[L + 1u]);
        }
        if (tid == 0) {
            rec->flags = uint16_t(flags | (s_bad ? uint32_t(pf::FLAG_INCONSISTENT) : 0u) | (af ? uint32_t(pf::FLAG_AF_OK) : 0u));
            rec->reserved_a = 0;
        }
    }
}

}  // namespace

hipError_t launch_pft_read(PftReadEntry *entries, int n_entries, void *d_table, hipStream_t s) {
    if (n_entries <= 0) return hipSuccess;
    if (!d_table || (reinterpret_cast<uintptr_t>(d_table) & 15) || n_entries > PFT_READ_MAX_ENTRIES) return hipErrorInvalidValue;
    const size_t entry_bytes = (size_t(n_entries) * sizeof(PftReadEntry) + 15) / 16 * 16;
    size_t at = entry_bytes, spans = 0;
    uint32_t most_records = 0;
    for (int i = 0; i < n_entries; i++) {
        PftReadEntry &e = entries[i];
        if (e.n_bytes < 0 || e.max_records < 1) return hipErrorInvalidValue;
        e.good = uint64_t(reinterpret_cast<uintptr_t>(d_table)) + at;
        e.stop = e.good + uint64_t(pft_read_bitmap_words(e.n_bytes)) * 8u;
        e.arena = e.good + (2 * pft_read_bitmap_words(e.n_bytes) * 8 + 15) / 16 * 16;
        e.arena_bytes = uint32_t(std::min<size_t>(pft_read_arena_bytes(e.n_bytes), 0xFFFFFFF0u));
        at += pft_read_scratch_bytes(e.n_bytes);
        spans = std::max(spans, (pft_read_positions(e.n_bytes) + PFT_READ_SPAN - 1) / PFT_READ_SPAN);
        most_records = std::max(most_records, e.max_records);
    }
    if (spans >= (size_t(1) << 31)) return hipErrorInvalidValue;
    // (pageable memory: the copy has left the host array when the call returns)
    hipError_t err = hipMemcpyAsync(d_table, entries, size_t(n_entries) * sizeof(PftReadEntry), hipMemcpyHostToDevice, s);
    if (err != hipSuccess) return err;
    const PftReadEntry *d_entries = static_cast<const PftReadEntry *>(d_table);
    hipLaunchKernelGGL(pft_read_check_kernel, dim3(unsigned(spans), unsigned(n_entries)), dim3(CHECK_WG), 0, s, d_entries);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    hipLaunchKernelGGL(pft_read_walk_kernel, dim3(unsigned(n_entries)), dim3(64), 0, s, d_entries);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    // the fill launch: about 4096 workgroups in all, each striding over its entry's records
    const unsigned per_entry = unsigned(std::min<size_t>(std::max<size_t>(4096 / size_t(n_entries), 1), most_records));
    hipLaunchKernelGGL(pft_read_fill_kernel, dim3(per_entry, unsigned(n_entries)), dim3(FILL_WG), 0, s, d_entries);
    return hipGetLastError();
}

}  // namespace dabk
