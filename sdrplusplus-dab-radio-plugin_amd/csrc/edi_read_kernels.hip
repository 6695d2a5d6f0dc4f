// edi_read_kernels.hip -- AF packet byte streams read back into FIBs, CRC flags and logical frames (include/dabgpu.h, "EDI
// input"; the contract and every check: include/dabgpu_edi.h).  Per entry S = the state's tail + the new bytes.
//
// edi_read_check_kernel   the parallel part: a lane per byte position, 4096 positions per workgroup, an entry per grid row.
//                         Every position is tested for a plausible header (H).  The rare hits are visited one after the
//                         other by their wave: a packet that lies inside S has its CRC folded a chunk of bytes per lane from
//                         a zero start, the chunk's way to the packet's end x^(8 n) mod P worked out on the spot (lengths
//                         vary), the 64 products added by six cross-lane exchanges.  A wave owns the 64-position words
//                         of the two bitmaps it leaves -- `good` (C of the contract) and `open` (H holds, the packet is
//                         incomplete) -- and writes every one of them: no clearing pass, no atomics.  Hits lie at least
//                         10 bytes apart, so a hostile stream costs at most n / 10 CRCs of at most 8 KB each.
// edi_read_walk_kernel    a wave per entry walks `good`: the next good position above a damaged stretch by ballot and
//                         find-first over 64 bitmap words at a time.  Each CRC-good packet comes into LDS; its TAG item
//                         chain is short and serial -- one lane runs the header's parse over LDS and leaves the fields
//                         record there -- and all 64 lanes then do the plan comparison, the FIB CRCs and the moves out.
//                         Rows, counters, status, result and the new state follow from the walk's own order: no scan, no
//                         atomics.  The serial part is one step per packet.
#include "kernels.hpp"

#include <algorithm>

#include "../../include/dabgpu_edi.h"

namespace dabk {

namespace {

namespace ed = dabgpu_edi;

constexpr int CHECK_WG = 256;
constexpr uint32_t POLY = 0x11021u;
constexpr uint32_t NONE = 0xFFFFFFFFu;
static_assert(EDI_READ_SPAN % CHECK_WG == 0 && CHECK_WG % 64 == 0, "a wave owns whole bitmap words");

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
struct LdsPacket {
    const uint8_t *p;
    __device__ __forceinline__ uint32_t operator()(int i) const { return p[i]; }
};

__device__ __forceinline__ StreamBytes stream_of(const EdiReadEntry &e) {
    StreamBytes s;
    const uint8_t *in = reinterpret_cast<const uint8_t *>(uintptr_t(e.state_in));
    s.tail = in ? in + ed::STATE_HEAD_BYTES : nullptr;
    s.t = in ? ed::clamp_tail(reinterpret_cast<const ed::Head *>(in)->tail_bytes) : 0u;
    s.fresh = reinterpret_cast<const uint8_t *>(uintptr_t(e.bytes));
    return s;
}

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

__global__ __launch_bounds__(CHECK_WG) void edi_read_check_kernel(const EdiReadEntry *entries) {
    __shared__ uint16_t s_tab[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    {
        uint32_t r = uint32_t(tid) << 8;
#pragma unroll
        for (int i = 0; i < 8; i++) r = (r & 0x8000u) ? ((r << 1) ^ POLY) & 0xffffu : (r << 1);
        s_tab[tid] = uint16_t(r);
    }
    __syncthreads();
    const EdiReadEntry &e = entries[blockIdx.y];
    const StreamBytes S = stream_of(e);
    const uint32_t len = S.t + uint32_t(e.n_bytes);
    const uint32_t b0 = blockIdx.x * uint32_t(EDI_READ_SPAN);
    unsigned long long *good = reinterpret_cast<unsigned long long *>(uintptr_t(e.good));
    unsigned long long *open = reinterpret_cast<unsigned long long *>(uintptr_t(e.open));
    for (int it = 0; it < EDI_READ_SPAN / CHECK_WG; it++) {
        const uint32_t q0 = b0 + uint32_t(it * CHECK_WG + wave * 64), q = q0 + uint32_t(lane);
        if (q0 >= len) break;                                                  // (uniform in the wave; words at and above len are not read)
        int total = 0;
        const bool hit = q + uint32_t(ed::AF_HEADER_BYTES) <= len && ed::header_ok(StreamAt{S, q}, total);
        unsigned long long hits = __ballot(hit), c_word = 0ull, i_word = 0ull;
        while (hits) {
            const int b = __ffsll(hits) - 1;
            hits &= hits - 1ull;
            const uint32_t qb = q0 + uint32_t(b), tb = uint32_t(__shfl(total, b, 64));
            if (qb + tb > len) {
                i_word |= 1ull << b;
                continue;
            }
            // the CRC over the L bytes in front of it: zero bytes in front up to 64 equal chunks, a chunk per lane
            const uint32_t L = tb - 2u, cb = (L + 63u) / 64u, lead = 64u * cb - L;
            uint32_t crc = 0;
            for (uint32_t j = 0; j < cb; j++) {
                const uint32_t m = uint32_t(lane) * cb + j;
                if (m >= lead) crc = ((crc << 8) & 0xffffu) ^ s_tab[(crc >> 8) ^ S(qb + m - lead)];
            }
            uint32_t sum = gf_mul16(crc, gf_xpow(8u * cb * uint32_t(63 - lane)));
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) sum ^= uint32_t(__shfl_xor(int(sum), d, 64));
            sum = (sum ^ gf_mul16(0xFFFFu, gf_xpow(8u * L)) ^ 0xffffu) & 0xffffu;
            if (sum == ((S(qb + L) << 8) | S(qb + L + 1u))) c_word |= 1ull << b;
        }
        if (lane == 0) {
            good[q0 / 64u] = c_word;
            open[q0 / 64u] = i_word;
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

__global__ __launch_bounds__(64) void edi_read_walk_kernel(const EdiReadEntry *entries) {
    __shared__ __attribute__((aligned(16))) uint8_t s_pkt[ed::MAX_PACKET];
    __shared__ ed::Fields s_f;
    __shared__ int s_verdict;
    const int lane = threadIdx.x;
    const EdiReadEntry &e = entries[blockIdx.x];
    const StreamBytes S = stream_of(e);
    const uint32_t len = S.t + uint32_t(e.n_bytes), words = (len + 63u) / 64u;
    const unsigned long long *good = reinterpret_cast<const unsigned long long *>(uintptr_t(e.good));
    const unsigned long long *open = reinterpret_cast<const unsigned long long *>(uintptr_t(e.open));
    ed::Head in{};
    if (e.state_in) in = *reinterpret_cast<const ed::Head *>(uintptr_t(e.state_in));
    ed::Carry k = ed::carry_of(in);
    ed::Result c{};
    const LdsPacket F{s_pkt};
    uint32_t p = 0, r = 0;
    for (;;) {
        if (!(p < len && ((good[p >> 6] >> (p & 63u)) & 1ull))) {
            const uint32_t q = next_bit(good, words, p + 1u, lane);
            if (q == NONE) {
                uint32_t t = next_bit(open, words, p, lane);
                if (t == NONE) t = len >= 9u && len - 9u > p ? len - 9u : p;
                if (t > p) {
                    c.skipped += t - p;
                    k.in_skip = true;
                }
                p = t;
                break;
            }
            c.skipped += q - p;
            p = q;
            k.in_skip = true;
        }
        if (k.in_skip) {
            c.resyncs++;
            k.in_skip = false;
        }
        // (the check launch has held this packet to its header and its CRC: LEN is read, bounded all the same)
        const uint32_t claimed = 12u + ((S(p + 2u) << 24) | (S(p + 3u) << 16) | (S(p + 4u) << 8) | S(p + 5u));
        const uint32_t total = min(min(claimed, uint32_t(ed::MAX_PACKET)), len - p);
        __syncthreads();                                                       // the packet before this one is done with
        for (uint32_t i = uint32_t(lane); i < total; i += 64) s_pkt[i] = uint8_t(S(p + i));
        __syncthreads();
        if (lane == 0) s_verdict = total >= uint32_t(ed::AF_OVERHEAD) ? ed::parse(F, int(total), s_f) : int(ed::BAD_TAGS);
        __syncthreads();
        const uint32_t seq = (uint32_t(s_pkt[6]) << 8) | s_pkt[7];
        const bool seq_break = k.have_seq && seq != ((k.last_seq + 1u) & 0xFFFFu);
        k.have_seq = true;
        k.last_seq = seq;
        const int verdict = s_verdict;
        bool row = false;
        if (verdict == ed::BAD_TAGS) {
            c.bad_tags++;
        } else if (verdict == ed::NOT_DETI) {
            c.not_deti++;
        } else if (e.has_plan) {
            bool differs = s_f.n_est != e.nst;
            if (!differs && lane < e.nst) {
                const uint8_t *stc = e.stc + 4 * lane;
                differs = s_f.sstc[lane][0] != stc[0] || s_f.sstc[lane][1] != stc[1] || (s_f.sstc[lane][2] & 0xFCu) != (stc[2] & 0xFCu) ||
                          int(s_f.stl[lane]) != (((stc[2] & 3) << 8) | stc[3]);
            }
            if (__ballot(differs)) c.other_plan++;
            else row = true;
        } else {
            row = true;
        }
        // (r < max_rows always: max_rows counts the smallest packets that give a row into |S|, as the host call's outputs
        // are sized; the test only keeps a table this code did not fill from writing outside them)
        if (row && r < uint32_t(e.max_rows)) {
            const bool ficf = s_f.ficf != 0;
            const int fic_at = ficf ? s_f.fic_at : 0;
            uint32_t ok = 0;
            if (ficf && lane < 3) ok = ed::fib_crc_ok(F, fic_at, lane);
            const uint32_t fib_ok = uint32_t(__ballot(ok != 0)) & 7u;
            const auto word_at = [&](int at) -> uint32_t {
                return uint32_t(s_pkt[at]) | (uint32_t(s_pkt[at + 1]) << 8) | (uint32_t(s_pkt[at + 2]) << 16) | (uint32_t(s_pkt[at + 3]) << 24);
            };
            uint32_t *fib_out = reinterpret_cast<uint32_t *>(uintptr_t(e.fib) + size_t(r) * ed::FIC_BYTES);
            if (lane < ed::FIC_BYTES / 4) fib_out[lane] = ficf ? word_at(fic_at + 4 * lane) : 0u;
            if (lane < 3) reinterpret_cast<uint8_t *>(uintptr_t(e.crc_ok))[size_t(r) * 3 + lane] = uint8_t(ok);
            if (e.has_plan) {
                for (int n = 0; n < e.nst; n++) {
                    if (!e.out[n]) continue;
                    const int nb = 8 * int(s_f.stl[n]), at = s_f.data_at[n];
                    uint32_t *dst = reinterpret_cast<uint32_t *>(uintptr_t(e.out[n]) + size_t(r) * size_t(nb));
                    for (int w = lane; w < nb / 4; w += 64) dst[w] = word_at(at + 4 * w);
                }
            }
            const ed::Status st = ed::make_status(p, int(total), s_f, fib_ok, seq_break, k);
            if (lane == 0) reinterpret_cast<ed::Status *>(uintptr_t(e.status))[r] = st;
            ed::count_row(c, st);
            k.have_prev = true;
            k.last_dlfc = uint32_t(s_f.dlfc);
            r++;
        }
        p += total;
    }
    c.tail_bytes = len - p;
    if (lane == 0) {
        // (field by field: a copy of the whole record keeps its reserved words in scratch memory)
        ed::Result *out = reinterpret_cast<ed::Result *>(uintptr_t(e.result));
        out->rows = c.rows;
        out->not_deti = c.not_deti;
        out->bad_tags = c.bad_tags;
        out->other_plan = c.other_plan;
        out->skipped = c.skipped;
        out->resyncs = c.resyncs;
        out->gap_sum = c.gap_sum;
        out->fib_errors = c.fib_errors;
        out->tail_bytes = c.tail_bytes;
        out->reserved_a = out->reserved_b = out->reserved_c = 0;
        *reinterpret_cast<ed::Head *>(uintptr_t(e.state_out)) = ed::next_head(in, c, k);
    }
    // the new tail: S[p ..), zeros behind it, as whole words
    uint32_t *tail = reinterpret_cast<uint32_t *>(uintptr_t(e.state_out) + ed::STATE_HEAD_BYTES);
    const uint32_t held = len - p;
    for (uint32_t w = uint32_t(lane); w < uint32_t(ed::MAX_PACKET / 4); w += 64) {
        uint32_t v = 0;
        for (uint32_t b = 0; b < 4; b++)
            if (4 * w + b < held) v |= S(p + 4 * w + b) << (8 * b);
        tail[w] = v;
    }
}

}  // namespace

hipError_t launch_edi_read(EdiReadEntry *entries, int n_entries, void *d_table, hipStream_t s) {
    if (n_entries <= 0) return hipSuccess;
    if (!d_table || (reinterpret_cast<uintptr_t>(d_table) & 15) || n_entries > EDI_READ_MAX_ENTRIES) return hipErrorInvalidValue;
    const size_t entry_bytes = (size_t(n_entries) * sizeof(EdiReadEntry) + 15) / 16 * 16;
    size_t at = entry_bytes, spans = 0;
    for (int i = 0; i < n_entries; i++) {
        EdiReadEntry &e = entries[i];
        if (e.n_bytes < 0 || e.max_rows < 1 || e.nst < 0 || e.nst > ETI_MAX_STREAMS) return hipErrorInvalidValue;
        e.good = uint64_t(reinterpret_cast<uintptr_t>(d_table)) + at;
        e.open = e.good + uint64_t(edi_read_bitmap_words(e.n_bytes)) * 8u;
        at += edi_read_scratch_bytes(e.n_bytes);
        spans = std::max(spans, (edi_read_positions(e.n_bytes) + EDI_READ_SPAN - 1) / EDI_READ_SPAN);
    }
    if (spans >= (size_t(1) << 31)) return hipErrorInvalidValue;
    // (pageable memory: the copy has left the host array when the call returns)
    hipError_t err = hipMemcpyAsync(d_table, entries, size_t(n_entries) * sizeof(EdiReadEntry), hipMemcpyHostToDevice, s);
    if (err != hipSuccess) return err;
    const EdiReadEntry *d_entries = static_cast<const EdiReadEntry *>(d_table);
    hipLaunchKernelGGL(edi_read_check_kernel, dim3(unsigned(spans), unsigned(n_entries)), dim3(CHECK_WG), 0, s, d_entries);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    hipLaunchKernelGGL(edi_read_walk_kernel, dim3(unsigned(n_entries)), dim3(64), 0, s, d_entries);
    return hipGetLastError();
}

}  // namespace dabk
