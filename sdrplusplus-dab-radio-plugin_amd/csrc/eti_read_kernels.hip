// eti_read_kernels.hip -- ETI(NI) byte streams read back into FIBs, CRC flags and logical frames (include/dabgpu.h,
// "ETI(NI) input"; the contract and every check: include/dabgpu_eti_read.h).  Per entry S = the state's tail + the new bytes.
//
// eti_read_scan_kernel    a lane per byte position, 8192 positions per workgroup.  The span of S comes into LDS with aligned
//                         16-byte loads -- the tail's part and the new bytes' part each on its own 16-byte phase, so the two
//                         meet in LDS -- and every position is tested for FSYNC, its parity against FCT and FCT < 250.  The rare
//                         hits run the header checks and the header CRC on the staged bytes (a header's length is staged
//                         behind the span).  A ballot per wave leaves the
//                         candidate bitmap, every word of it written (no clearing pass).
// eti_read_chain_kernel   a wave per entry resolves the walk from the bitmap: the 64 frame positions ahead are looked at
//                         together (a lane each), so the serial part is one step per run of up to 64 good frames; after
//                         damage the smallest candidate above p by ballot and find-first over 64 bitmap words at a time.
//                         Writes the row list and the new state's tail.
// eti_read_row_kernel     a wave per row.  The frame comes into LDS from its byte offset (on the source's 16-byte phase),
//                         the data CRC is folded chunk per lane with the x^(8n) mod P constants of the entry table (or, for a
//                         frame of another length than the plan's, worked out here), then the three FIB CRCs, the plan
//                         comparison, the status and the moves out.
// eti_read_finish_kernel  a wave per entry adds the rows' counters up (no atomics) and writes the result and the state's head.
#include "kernels.hpp"

#include <vector>

#include "../../include/dabgpu_eti_read.h"

namespace dabk {

namespace {

namespace er = dabgpu_eti_read;

static_assert(er::FRAME_BYTES == ETI_FRAME_BYTES && er::MAX_STREAMS == ETI_MAX_STREAMS && er::FIC_BYTES == ETI_FIC_BYTES, "one frame");

constexpr int SCAN_WG = 256;
constexpr int SCAN_AHEAD = 288;                // bytes staged behind a span: the header of its last position
constexpr int SCAN_LDS_A = ETI_FRAME_BYTES + 16;   // the tail's part (the tail lies inside the first span)
constexpr int SCAN_LDS_B = ETI_READ_SCAN_SPAN + SCAN_AHEAD + 16;
static_assert(SCAN_AHEAD >= er::MAX_HEADER_BYTES + 4 && SCAN_AHEAD % 16 == 0, "a header behind the span's last position");
static_assert(ETI_READ_SCAN_SPAN >= ETI_FRAME_BYTES && ETI_READ_SCAN_SPAN % SCAN_WG == 0, "the tail lies inside the first span");
constexpr int ROW_WG = 64 * ETI_READ_ROW_WAVES;
constexpr int ROW_LDS = ETI_FRAME_BYTES + 32;
constexpr uint32_t POLY = 0x11021u;

// S of an entry in global memory: the tail of the state record, then the new bytes
struct StreamBytes {
    const uint8_t *tail, *fresh;
    uint32_t t;                                // tail length
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return i < t ? tail[i] : fresh[i - t]; }
};
struct LdsFrame {
    const uint8_t *p;
    __device__ __forceinline__ uint32_t operator()(int i) const { return p[i]; }
};

__device__ __forceinline__ StreamBytes stream_of(const EtiReadEntry &e) {
    StreamBytes s;
    const uint8_t *in = reinterpret_cast<const uint8_t *>(uintptr_t(e.state_in));
    s.tail = in ? in + er::STATE_HEAD_BYTES : nullptr;
    s.t = in ? er::clamp_tail(reinterpret_cast<const er::Head *>(in)->tail_bytes) : 0u;
    s.fresh = reinterpret_cast<const uint8_t *>(uintptr_t(e.bytes));
    return s;
}

// the last entry whose base is at or below g (bases ascend, base[0] = 0), found by the whole wave: the packed bases come in
// coalesced loads that do not depend on each other, and the entry is one less than the number of bases at or below g
__device__ __forceinline__ int entry_of(const uint32_t *base, int n_entries, uint32_t g, int lane) {
    int count = 0;
    for (int i0 = 0; i0 < n_entries; i0 += 64) {
        const int i = i0 + lane;
        count += __popcll(__ballot(i < n_entries && base[i] <= g));
    }
    return count - 1;
}
__device__ __forceinline__ const uint32_t *packed_bases(const EtiReadEntry *entries, int n_entries) {
    return reinterpret_cast<const uint32_t *>(entries + n_entries);         // scan_base [n_entries], then row_base [n_entries]
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

__global__ __launch_bounds__(SCAN_WG) void eti_read_scan_kernel(const EtiReadEntry *entries, int n_entries) {
    __shared__ __attribute__((aligned(16))) uint8_t s_a[SCAN_LDS_A];
    __shared__ __attribute__((aligned(16))) uint8_t s_b[SCAN_LDS_B];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ei = entry_of(packed_bases(entries, n_entries), n_entries, blockIdx.x, lane);
    const EtiReadEntry &e = entries[ei];
    const StreamBytes S = stream_of(e);
    const uint32_t n = uint32_t(e.n_bytes), len = S.t + n;
    const uint32_t b0 = (blockIdx.x - e.scan_base) * uint32_t(ETI_READ_SCAN_SPAN);
    const uint32_t limit = len >= uint32_t(ETI_FRAME_BYTES) ? len - uint32_t(ETI_FRAME_BYTES) + 1u : 0u;   // positions below it are judged
    const uint32_t end = min(b0 + uint32_t(ETI_READ_SCAN_SPAN + SCAN_AHEAD), len);                             // bytes [b0, end) are staged
    // the tail's part: S[i] at s_a[i - b0] (the record holds 6144 tail bytes, so whole 16-byte loads stay inside it)
    if (b0 < S.t) {
        const uint32_t stop = min(S.t, end);
        for (uint32_t c = b0 / 16u + uint32_t(tid); c * 16u < stop; c += SCAN_WG)
            reinterpret_cast<uint4 *>(s_a)[c - b0 / 16u] = reinterpret_cast<const uint4 *>(S.tail)[c];
    }
    // the new bytes' part: new byte j at s_b[j - jb]; whole 16-byte loads where they end inside the n bytes, bytes behind
    uint32_t jb = 0;
    if (end > S.t) {
        const uint32_t j0 = max(b0, S.t) - S.t, j1 = end - S.t;
        jb = j0 & ~15u;
        const uint32_t whole = min(j1, n & ~15u);
        for (uint32_t c = jb / 16u + uint32_t(tid); c * 16u < whole; c += SCAN_WG)
            reinterpret_cast<uint4 *>(s_b)[c - jb / 16u] = reinterpret_cast<const uint4 *>(S.fresh)[c];
        for (uint32_t j = max(jb, n & ~15u) + uint32_t(tid); j < j1; j += SCAN_WG) s_b[j - jb] = S.fresh[j];
    }
    __syncthreads();
    const uint32_t a_off = b0, b_off = S.t + jb;
    const auto at = [&](uint32_t i) -> uint32_t { return i < S.t ? s_a[i - a_off] : s_b[i - b_off]; };
    unsigned long long *bitmap = reinterpret_cast<unsigned long long *>(uintptr_t(e.bitmap));
    for (int it = 0; it < ETI_READ_SCAN_SPAN / SCAN_WG; it++) {
        const uint32_t q0 = b0 + uint32_t(it * SCAN_WG + wave * 64), q = q0 + uint32_t(lane);
        if (q0 / 64u >= uint32_t(e.bitmap_words)) break;                       // (uniform in the wave)
        bool cand = false;
        // (one byte decides for 254 positions of 256; the other three are looked at behind it)
        const uint32_t b1 = q < limit ? at(q + 1) : 0u;
        if ((b1 == 0x07u || b1 == 0xF8u) && er::sync_ok(b1, at(q + 2), at(q + 3), at(q + 4))) {
            // (the header of the last position of the span still lies in LDS: the span is staged with a header's length behind it)
            er::Fields f;
            cand = er::header_verdict([&](int i) -> uint32_t { return at(q + uint32_t(i)); }, f) == er::TAKEN;
        }
        const unsigned long long word = __ballot(cand);
        if (lane == 0) bitmap[q0 / 64u] = word;
    }
}

// the smallest candidate at or above `from` (bits at and above the judged limit are zero), or 0xFFFFFFFF
__device__ __forceinline__ uint32_t next_candidate(const unsigned long long *bitmap, uint32_t words, uint32_t from, int lane) {
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
    return 0xFFFFFFFFu;
}

__global__ __launch_bounds__(64) void eti_read_chain_kernel(const EtiReadEntry *entries) {
    const int lane = threadIdx.x;
    const EtiReadEntry &e = entries[blockIdx.x];
    const StreamBytes S = stream_of(e);
    const uint32_t len = S.t + uint32_t(e.n_bytes), words = uint32_t(e.bitmap_words);
    const unsigned long long *bitmap = reinterpret_cast<const unsigned long long *>(uintptr_t(e.bitmap));
    uint32_t *list = reinterpret_cast<uint32_t *>(uintptr_t(e.rows));
    uint32_t p = 0, r = 0, skipped = 0, resyncs = 0;
    while (p + uint32_t(ETI_FRAME_BYTES) <= len) {
        // the next 64 frame positions at once: lane k looks at p + 6144 k, and the run of candidates from lane 0 on is as
        // many steps of the walk (an undamaged stream takes 64 rows per dependent load, not one)
        const uint32_t mine = p + uint32_t(lane) * uint32_t(ETI_FRAME_BYTES);
        const bool cand = mine + uint32_t(ETI_FRAME_BYTES) <= len && ((bitmap[mine >> 6] >> (mine & 63u)) & 1ull);
        const unsigned long long run = ~__ballot(cand);
        const uint32_t n = run ? uint32_t(__ffsll(run) - 1) : 64u;
        if (n) {
            if (uint32_t(lane) < n && r + uint32_t(lane) < uint32_t(e.max_frames)) list[ETI_READ_LIST_HEAD + r + uint32_t(lane)] = mine;
            r += n;
            p += n * uint32_t(ETI_FRAME_BYTES);
            continue;
        }
        const uint32_t q = next_candidate(bitmap, words, p + 1, lane);
        if (q != 0xFFFFFFFFu) {
            skipped += q - p;
            resyncs++;
            p = q;
        } else {
            const uint32_t stop = len - uint32_t(er::MAX_TAIL);
            if (stop > p) {
                skipped += stop - p;
                p = stop;
            }
            break;
        }
    }
    if (lane == 0) {
        list[0] = min(r, uint32_t(e.max_frames));
        list[1] = p;
        list[2] = skipped;
        list[3] = resyncs;
    }
    // the new tail: S[p ..), zeros behind it, as whole words
    uint32_t *tail = reinterpret_cast<uint32_t *>(uintptr_t(e.state_out) + er::STATE_HEAD_BYTES);
    const uint32_t held = len - p;
    for (uint32_t w = uint32_t(lane); w < uint32_t(ETI_FRAME_BYTES / 4); w += 64) {
        uint32_t v = 0;
        for (uint32_t b = 0; b < 4; b++)
            if (4 * w + b < held) v |= S(p + 4 * w + b) << (8 * b);
        tail[w] = v;
    }
}

__global__ __launch_bounds__(ROW_WG) void eti_read_row_kernel(const EtiReadEntry *entries, int n_entries, uint32_t total) {
    __shared__ __attribute__((aligned(16))) uint8_t s_frame[ETI_READ_ROW_WAVES][ROW_LDS];
    __shared__ uint16_t s_tab[4][256];                                         // s_tab[k][i] = i x^(16 + 8 k) mod P
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    {
        uint32_t r = uint32_t(tid) << 8;
#pragma unroll
        for (int k = 0; k < 4; k++) {
#pragma unroll
            for (int i = 0; i < 8; i++) r = (r & 0x8000u) ? ((r << 1) ^ POLY) & 0xffffu : (r << 1);
            s_tab[k][tid] = uint16_t(r);
        }
    }
    const uint32_t g = blockIdx.x * uint32_t(ETI_READ_ROW_WAVES) + uint32_t(wave);
    const int ei = entry_of(packed_bases(entries, n_entries) + n_entries, n_entries, min(g, total - 1u), lane);
    const EtiReadEntry &e = entries[ei];
    const uint32_t *list = reinterpret_cast<const uint32_t *>(uintptr_t(e.rows));
    const uint32_t r = g - e.row_base;
    const bool live = g < total && r < list[0];
    const StreamBytes S = stream_of(e);
    uint8_t *W = s_frame[wave];
    uint32_t p = 0, ph = 0, length = 0;
    if (live) {
        p = list[ETI_READ_LIST_HEAD + r];
        // bytes before the padding: 4 FL + 16 (the position is a candidate: no more than 6144)
        length = min(4u * (((S(p + 6) & 7u) << 8) | S(p + 7)) + 16u, uint32_t(ETI_FRAME_BYTES));
        // frame byte i lies at W[ph + i]; the new bytes' part keeps the phase it has in global memory
        const uint32_t i0 = p < S.t ? min(S.t - p, length) : 0u;               // frame bytes that come from the tail
        const uint32_t j0 = p < S.t ? 0u : p - S.t;                            // the first new byte of the frame
        ph = (j0 - i0) & 15u;
        for (uint32_t i = uint32_t(lane); i < i0; i += 64) W[ph + i] = S.tail[p + i];
        if (length > i0) {
            const uint32_t n = uint32_t(e.n_bytes), j1 = j0 + (length - i0), jb = j0 & ~15u;
            const uint32_t lds0 = ph + i0 - (j0 - jb);                        // where new byte jb lies: a multiple of 16
            const uint32_t whole = min((j1 + 15u) & ~15u, n & ~15u);
            for (uint32_t c = jb / 16u + uint32_t(lane); c * 16u < whole; c += 64)
                *reinterpret_cast<uint4 *>(W + lds0 + (c * 16u - jb)) = reinterpret_cast<const uint4 *>(S.fresh)[c];
            for (uint32_t j = max(jb, n & ~15u) + uint32_t(lane); j < j1; j += 64) W[lds0 + (j - jb)] = S.fresh[j];
        }
    }
    __syncthreads();
    if (!live) return;
    const LdsFrame F{W + ph};
    // (a candidate: the scan has held the header to its CRC, so the fields are read, not judged again; the bounds that keep
    // every access below inside the frame's LDS are checked all the same, and a header that broke them gives a row of zeros)
    er::Fields f{};
    er::candidate_fields(F, f);
    int verdict = er::TAKEN;
    if (f.nst > ETI_MAX_STREAMS || f.data_bytes < ETI_FIC_BYTES || f.fic_offset + f.data_bytes + 8 > int(length)) {
        f.data_bytes = 0;
        verdict = er::BAD_HEADER;
    }
    // the data CRC: FIC + streams, zero words in front up to 64 equal chunks, a chunk per lane from a zero start
    const int n_words = f.data_bytes / 4;
    const bool planned = e.has_plan && f.data_bytes == e.data_bytes;
    const int cw = planned ? e.chunk_words : (n_words + 63) / 64;
    const int lead = 64 * cw - n_words;
    uint32_t crc = 0;
    for (int j = 0; j < cw; j++) {
        const int m = lane * cw + j - lead;
        if (m >= 0) {
            // four bytes a step: the register's two bytes meet the first two, and the four look-ups do not wait for each other
            const uint8_t *d = W + ph + f.fic_offset + 4 * m;
            crc = uint32_t(s_tab[3][(crc >> 8) ^ d[0]]) ^ s_tab[2][(crc & 0xffu) ^ d[1]] ^ s_tab[1][d[2]] ^ s_tab[0][d[3]];
        }
    }
    const uint32_t shift = planned ? uint32_t(e.lane_shift[lane]) : gf_xpow(32u * uint32_t(cw) * uint32_t(63 - lane));
    const uint32_t init = planned ? uint32_t(e.data_init) : gf_mul16(0xFFFFu, gf_xpow(8u * uint32_t(f.data_bytes)));
    uint32_t sum = gf_mul16(crc, shift);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum ^= uint32_t(__shfl_xor(int(sum), d, 64));
    sum = (sum ^ init ^ 0xffffu) & 0xffffu;
    const int eof = f.fic_offset + f.data_bytes;
    if (verdict == er::TAKEN && sum != ((F(eof) << 8) | F(eof + 1))) verdict = er::BAD_DATA_CRC;
    if (verdict == er::TAKEN && e.has_plan) {
        bool differs = f.nst != e.nst || f.fl != e.fl;
        if (!differs)
            for (int i = lane; i < 4 * f.nst; i += 64) differs = differs || F(8 + i) != e.stc[i];
        if (__ballot(differs)) verdict = er::OTHER_PLAN;
    }
    const bool taken = verdict == er::TAKEN;
    // the three FIB CRCs, a FIB per lane
    uint32_t ok = 0;
    if (taken && lane < 3) ok = er::fib_crc_ok(F, f, lane);
    const uint32_t fib_ok = uint32_t(__ballot(ok != 0)) & 7u;
    // out: the FIC, the flags, the wanted streams (or zeros)
    const uint8_t *fic = W + ph + f.fic_offset;
    const auto word_at = [&](const uint8_t *b) -> uint32_t { return taken ? uint32_t(b[0]) | (uint32_t(b[1]) << 8) | (uint32_t(b[2]) << 16) | (uint32_t(b[3]) << 24) : 0u; };
    uint32_t *fib_out = reinterpret_cast<uint32_t *>(uintptr_t(e.fib) + size_t(r) * ETI_FIC_BYTES);
    if (lane < ETI_FIC_BYTES / 4) fib_out[lane] = word_at(fic + 4 * lane);
    if (lane < 3) reinterpret_cast<uint8_t *>(uintptr_t(e.crc_ok))[size_t(r) * 3 + lane] = uint8_t(ok);
    if (e.has_plan) {
        for (int k = 0; k < e.nst; k++) {
            if (!e.out[k]) continue;
            const int nb = e.nbytes[k];
            uint32_t *dst = reinterpret_cast<uint32_t *>(uintptr_t(e.out[k]) + size_t(r) * size_t(nb));
            const uint8_t *src = fic + ETI_FIC_BYTES + e.offset[k];
            for (int w = lane; w < nb / 4; w += 64) dst[w] = word_at(src + 4 * w);
        }
    }
    if (lane == 0) {
        bool have;
        uint32_t fct, fp;
        if (r > 0) {
            const uint32_t before = list[ETI_READ_LIST_HEAD + r - 1];
            have = true;
            fct = S(before + 4);
            fp = S(before + 6) >> 5;
        } else {
            const er::Head *in = reinterpret_cast<const er::Head *>(uintptr_t(e.state_in));
            have = in && in->have_prev != 0;
            fct = in ? in->last_fct : 0;
            fp = in ? in->last_fp : 0;
        }
        reinterpret_cast<er::Status *>(uintptr_t(e.status))[r] = er::make_status(p, verdict, f, fib_ok, have, fct, fp);
    }
}

__global__ __launch_bounds__(64) void eti_read_finish_kernel(const EtiReadEntry *entries) {
    const int lane = threadIdx.x;
    const EtiReadEntry &e = entries[blockIdx.x];
    const uint32_t *list = reinterpret_cast<const uint32_t *>(uintptr_t(e.rows));
    const er::Status *status = reinterpret_cast<const er::Status *>(uintptr_t(e.status));
    const uint32_t rows = list[0];
    er::Result c{};
    for (uint32_t r = uint32_t(lane); r < rows; r += 64) er::count_row(c, status[r]);
    uint32_t *sums[] = {&c.rows, &c.taken, &c.bad_data_crc, &c.other_plan, &c.gap_sum, &c.fib_errors};
    for (uint32_t *v : sums)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) *v += uint32_t(__shfl_xor(int(*v), d, 64));
    if (lane != 0) return;
    const StreamBytes S = stream_of(e);
    c.skipped = list[2];
    c.resyncs = list[3];
    c.tail_bytes = S.t + uint32_t(e.n_bytes) - list[1];
    *reinterpret_cast<er::Result *>(uintptr_t(e.result)) = c;
    er::Head in{};
    if (e.state_in) in = *reinterpret_cast<const er::Head *>(uintptr_t(e.state_in));
    uint32_t fct = 0, fp = 0;
    if (rows) {
        fct = status[rows - 1].fct;
        fp = status[rows - 1].fp;
    }
    *reinterpret_cast<er::Head *>(uintptr_t(e.state_out)) = er::next_head(in, c, rows != 0, fct, fp);
}

}  // namespace

hipError_t launch_eti_read(EtiReadEntry *entries, int n_entries, void *d_table, hipStream_t s) {
    if (n_entries <= 0) return hipSuccess;
    if (!d_table || (reinterpret_cast<uintptr_t>(d_table) & 15)) return hipErrorInvalidValue;
    const size_t entry_bytes = size_t(n_entries) * sizeof(EtiReadEntry), table_bytes = entry_bytes + eti_read_bases_bytes(n_entries);
    std::vector<uint32_t> bases(eti_read_bases_bytes(n_entries) / 4, 0u);
    size_t at = table_bytes;
    uint64_t scan_blocks = 0, row_waves = 0;
    for (int i = 0; i < n_entries; i++) {
        EtiReadEntry &e = entries[i];
        if (e.n_bytes < 0 || e.max_frames != (e.n_bytes + 6143) / 6144) return hipErrorInvalidValue;
        e.bitmap_words = (e.n_bytes + 63) / 64;
        e.bitmap = uint64_t(reinterpret_cast<uintptr_t>(d_table)) + at;
        e.rows = e.bitmap + uint64_t(e.bitmap_words) * 8u;
        at += eti_read_scratch_bytes(e.n_bytes);
        e.scan_base = bases[size_t(i)] = uint32_t(scan_blocks);
        e.row_base = bases[size_t(n_entries) + size_t(i)] = uint32_t(row_waves);
        scan_blocks += uint64_t((e.n_bytes + ETI_READ_SCAN_SPAN - 1) / ETI_READ_SCAN_SPAN);
        row_waves += uint64_t(e.max_frames);
        if (scan_blocks >= (uint64_t(1) << 31) || row_waves >= (uint64_t(1) << 31)) return hipErrorInvalidValue;
    }
    // (pageable memory: the copy has left the host array when the call returns)
    hipError_t err = hipMemcpyAsync(d_table, entries, entry_bytes, hipMemcpyHostToDevice, s);
    if (err != hipSuccess) return err;
    err = hipMemcpyAsync(static_cast<uint8_t *>(d_table) + entry_bytes, bases.data(), bases.size() * 4, hipMemcpyHostToDevice, s);
    if (err != hipSuccess) return err;
    const EtiReadEntry *d_entries = static_cast<const EtiReadEntry *>(d_table);
    if (scan_blocks) {
        hipLaunchKernelGGL(eti_read_scan_kernel, dim3(unsigned(scan_blocks)), dim3(SCAN_WG), 0, s, d_entries, n_entries);
        if ((err = hipGetLastError()) != hipSuccess) return err;
    }
    hipLaunchKernelGGL(eti_read_chain_kernel, dim3(unsigned(n_entries)), dim3(64), 0, s, d_entries);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    if (row_waves) {
        const unsigned blocks = unsigned((row_waves + ETI_READ_ROW_WAVES - 1) / ETI_READ_ROW_WAVES);
        hipLaunchKernelGGL(eti_read_row_kernel, dim3(blocks), dim3(ROW_WG), 0, s, d_entries, n_entries, uint32_t(row_waves));
        if ((err = hipGetLastError()) != hipSuccess) return err;
    }
    hipLaunchKernelGGL(eti_read_finish_kernel, dim3(unsigned(n_entries)), dim3(64), 0, s, d_entries);
    return hipGetLastError();
}

}  // namespace dabk
