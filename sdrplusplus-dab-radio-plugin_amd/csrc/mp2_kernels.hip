// mp2_kernels.hip -- following DAB (MPEG layer II) sub-channels to checked frames and PAD rows (dabgpu_mp2_follow_dev;
// contract and code: include/dabgpu_mp2_frame.h, shared with the host twin and the host mirror).
//
// Two launches for all entries and all frames of a batch.
//   mp2_rate_kernel   one wave64 per entry: a lane per logical frame reads the four header bytes, ballots count the valid
//                     ID = 1 headers and the valid ID = 0 headers by residue, every lane then knows rate and phase; the
//                     wave writes the plan (behind the table), both result records and the whole carry record.
//   mp2_frame_kernel  workgroup (entry, chunk) of one wave: a lane per frame brings the frame's first 48 bytes into LDS
//                     (16-byte loads where the frame lies on 16 bytes) and runs the header check and the ISO CRC over them
//                     -- the bit reader indexes LDS, never a local array; the allocation widths are comparisons against
//                     packed constants -- then the whole wave lifts the PAD of the chunk's frames into their rows, a
//                     4-byte store a lane, and writes the status rows 16 words a frame.  The three counters of a chunk go
//                     into the result record as one atomic add each.
#include <hip/hip_runtime.h>

#include "../../include/dabgpu_mp2_frame.h"
#include "kernels.hpp"

namespace dabk {
namespace {

namespace mp2 = dabgpu_mp2;

constexpr int MP2_CHUNK = 64;                       // frames per workgroup of the frame kernel: one per lane
constexpr int MP2_FRONT_WORDS = mp2::FRONT_BYTES / 4;
constexpr int MP2_FRONT_STRIDE = MP2_FRONT_WORDS + 1;   // 13 words a lane: odd, so the lanes' rows start on different banks
constexpr int MP2_ROW_WORDS = mp2::ROW_BYTES / 4;

static_assert(sizeof(SuperframeStatus) == 64 && sizeof(FollowResult) == 32 && sizeof(mp2::Result) == 64, "records of the ABI");
static_assert(MP2_ROW_WORDS <= 64 && mp2::ROW_BYTES % 4 == 0, "a row is one 4-byte store a lane");

// logical frame i of F: the held frame of the carry record, then the new ones
__device__ __forceinline__ const uint8_t *mp2_frame(const Mp2Entry &e, int held, int i) {
    return i < held ? reinterpret_cast<const uint8_t *>(e.carry_in) + mp2::CARRY_HEADER
                    : reinterpret_cast<const uint8_t *>(e.in) + size_t(i - held) * e.in_stride;
}

__device__ __forceinline__ uint32_t load_word(const uint8_t *p) {
    if ((reinterpret_cast<uintptr_t>(p) & 3) == 0) return *reinterpret_cast<const uint32_t *>(p);
    return uint32_t(p[0]) | (uint32_t(p[1]) << 8) | (uint32_t(p[2]) << 16) | (uint32_t(p[3]) << 24);
}

__device__ __forceinline__ mp2::Carry mp2_carry(const Mp2Entry &e) {
    if (!e.carry_in) return mp2::Carry{0, 0, 0};
    const int4 h = *reinterpret_cast<const int4 *>(e.carry_in);
    return mp2::read_carry(h.x, h.y, h.z, h.w);
}

__global__ __launch_bounds__(64) void mp2_rate_kernel(const Mp2Entry *table, Mp2Plan *plan, int n_cifs) {
    const Mp2Entry e = table[blockIdx.x];
    const int lane = threadIdx.x, B = e.bitrate, lf = 3 * B;
    const mp2::Carry cy = mp2_carry(e);
    const int T = cy.held + n_cifs;
    int hits1 = 0, v0 = 0, v1 = 0;
    // (index << 2) | mode of the lane's first valid header of either ID; i0 is a multiple of 64, so a lane's frames all
    // have the lane's parity
    int first1 = 0x7fffffff, first0 = 0x7fffffff;
    for (int i0 = 0; i0 < T; i0 += 64) {
        const int i = i0 + lane;
        int id = -1;
        if (i < T) {
            const uint32_t h = __builtin_bswap32(load_word(mp2_frame(e, cy.held, i)));
            id = mp2::header_id(h, B);
            const int key = (i << 2) | mp2::header_mode(h);
            if (id == 1 && key < first1) first1 = key;
            if (id == 0 && key < first0) first0 = key;
        }
        hits1 += __popcll(__ballot(id == 1));
        v0 += __popcll(__ballot(id == 0 && !(i & 1)));
        v1 += __popcll(__ballot(id == 0 && (i & 1)));
    }
    const mp2::Plan p = mp2::decide(cy, T, hits1, v0, v1);
    int key = p.rate == mp2::RATE_48K ? first1 : p.rate == mp2::RATE_24K && (lane & 1) == p.phase ? first0 : 0x7fffffff;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) key = min(key, __shfl_xor(key, d));
    // the carry record, whole: header, the held frame, zeros behind it
    uint8_t *co = reinterpret_cast<uint8_t *>(e.carry_out);
    const int body = mp2::carry_bytes(B) - mp2::CARRY_HEADER;          // a multiple of 8, as lf is
    if (p.kept) {
        const uint8_t *src = mp2_frame(e, cy.held, p.first_kept);
        if ((reinterpret_cast<uintptr_t>(src) & 7) == 0) {
            for (int i = lane; i < lf / 8; i += 64)
                reinterpret_cast<uint2 *>(co + mp2::CARRY_HEADER)[i] = reinterpret_cast<const uint2 *>(src)[i];
        } else {
            for (int i = lane; i < lf; i += 64) co[mp2::CARRY_HEADER + i] = src[i];
        }
    }
    for (int i = p.kept * lf / 8 + lane; i < body / 8; i += 64)
        reinterpret_cast<uint2 *>(co + mp2::CARRY_HEADER)[i] = make_uint2(0u, 0u);
    if (lane == 0) {
        *reinterpret_cast<int4 *>(co) = make_int4(p.synced, p.kept, p.synced ? p.rate : 0, mp2::CARRY_MAGIC);
        Mp2Plan pl;
        pl.rate = p.rate; pl.phase = p.phase; pl.n_rows = p.n_rows; pl.held = cy.held;
        plan[blockIdx.x] = pl;
        FollowResult r;
        r.n_superframes = p.n_rows; r.phase = p.phase; r.synced = p.synced; r.dropped = p.dropped;
        r.raw_hits = hits1 + v0 + v1; r.held = p.kept;
        r.reserved[0] = r.reserved[1] = 0;
        *reinterpret_cast<FollowResult *>(e.follow) = r;
        *reinterpret_cast<mp2::Result *>(e.result) = mp2::plan_result(p, B, hits1 + v0 + v1, key == 0x7fffffff ? -1 : key & 3);
    }
}

// bytes of a frame's front that lie in LDS
struct LdsBytes {
    const uint8_t *p;
    __device__ uint8_t operator()(int i) const { return p[i]; }
};

__global__ __launch_bounds__(MP2_CHUNK) void mp2_frame_kernel(const Mp2Entry *table, const Mp2Plan *plan, int chunks) {
    __shared__ __attribute__((aligned(16))) uint32_t front[MP2_CHUNK * MP2_FRONT_STRIDE];
    __shared__ int slot_x[MP2_CHUNK], slot_c[MP2_CHUNK];
    const int ei = blockIdx.x / unsigned(chunks), k0 = int(blockIdx.x % unsigned(chunks)) * MP2_CHUNK;
    const Mp2Plan pl = plan[ei];
    if (k0 >= pl.n_rows) return;                                       // (the whole workgroup, before any barrier)
    const Mp2Entry e = table[ei];
    const int lane = threadIdx.x, B = e.bitrate, lf = 3 * B;
    const int per = mp2::slot_frames(pl.rate), L = per * lf, want_id = pl.rate == mp2::RATE_48K ? 1 : 0;
    const int n = min(MP2_CHUNK, pl.n_rows - k0);
    auto slot = [&](int k) {
        mp2::TwoPart tp;
        const int i = pl.phase + per * k;
        tp.a = mp2_frame(e, pl.held, i);
        tp.b = per == 2 ? mp2_frame(e, pl.held, i + 1) : tp.a + lf;
        tp.split = lf;
        return tp;
    };
    int kind = -1;
    if (lane < n) {
        const mp2::TwoPart tp = slot(k0 + lane);
        uint32_t *mine = front + lane * MP2_FRONT_STRIDE;
        if (lf >= mp2::FRONT_BYTES && (reinterpret_cast<uintptr_t>(tp.a) & 15) == 0) {
#pragma unroll
            for (int q = 0; q < MP2_FRONT_WORDS / 4; q++) {
                const uint4 v = reinterpret_cast<const uint4 *>(tp.a)[q];
                mine[4 * q] = v.x; mine[4 * q + 1] = v.y; mine[4 * q + 2] = v.z; mine[4 * q + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int w = 0; w < MP2_FRONT_WORDS; w++) {
                const int off = 4 * w;                                 // (lf is a multiple of 8: a word lies in one part)
                mine[w] = off + 4 <= L ? load_word(off < lf ? tp.a + off : tp.b + (off - lf)) : 0u;
            }
        }
        // (a lane reads back only what it wrote itself: no barrier)
        int c = 0;
        kind = mp2::parse_frame(LdsBytes{reinterpret_cast<const uint8_t *>(mine)}, min(L, mp2::FRONT_BYTES), B, want_id, &c);
        slot_x[lane] = kind == mp2::FRAME_GOOD ? mp2::xpad_bytes(L, c) : -1;
        slot_c[lane] = c;
    }
    const int n_header = __popcll(__ballot(kind == mp2::FRAME_HEADER_ERROR));
    const int n_no_crc = __popcll(__ballot(kind == mp2::FRAME_NO_CRC));
    const int n_failed = __popcll(__ballot(kind == mp2::FRAME_CRC_FAILED));
    if (lane == 0) {
        mp2::Result *r = reinterpret_cast<mp2::Result *>(e.result);
        if (n_header) atomicAdd(&r->header_errors, n_header);
        if (n_no_crc) atomicAdd(&r->frames_no_crc, n_no_crc);
        if (n_failed) atomicAdd(&r->crc_failed, n_failed);
    }
    __syncthreads();
    uint8_t *rows = reinterpret_cast<uint8_t *>(e.rows) + size_t(k0) * mp2::ROW_BYTES;
    const bool word_rows = (e.rows & 3) == 0;                          // (220 is a multiple of 4: all rows or none)
    for (int r = 0; r < n && lane < MP2_ROW_WORDS; r++) {
        const int x = slot_x[r], c = slot_c[r];
        uint32_t v = 0;
        if (x >= 0 && 4 * lane < x + 4) {
            const mp2::TwoPart tp = slot(k0 + r);
#pragma unroll
            for (int b = 0; b < 4; b++) v |= uint32_t(mp2::row_byte(tp, L, c, x, 4 * lane + b)) << (8 * b);
        }
        uint8_t *dst = rows + size_t(r) * mp2::ROW_BYTES + 4 * lane;
        if (word_rows) {
            *reinterpret_cast<uint32_t *>(dst) = v;
        } else {
            dst[0] = uint8_t(v); dst[1] = uint8_t(v >> 8); dst[2] = uint8_t(v >> 16); dst[3] = uint8_t(v >> 24);
        }
    }
    int32_t *status = reinterpret_cast<int32_t *>(e.status) + size_t(k0) * 16;
    for (int i = lane; i < n * 16; i += 64) status[i] = mp2::status_word(i & 15, slot_x[i >> 4]);
}

}  // namespace

size_t mp2_table_bytes(int n_entries) { return size_t(n_entries) * (sizeof(Mp2Entry) + sizeof(Mp2Plan)); }

hipError_t launch_mp2_follow(const Mp2Entry *entries, int n_entries, int n_cifs, void *d_table, size_t table_bytes, hipStream_t stream) {
    if (n_entries <= 0) return hipSuccess;
    if (n_cifs < 0 || !d_table || table_bytes < mp2_table_bytes(n_entries) || (reinterpret_cast<uintptr_t>(d_table) & 15))
        return hipErrorInvalidValue;
    for (int i = 0; i < n_entries; i++)
        if (!mp2::bitrate_ok(entries[i].bitrate)) return hipErrorInvalidValue;
    const int chunks = (n_cifs + 1 + MP2_CHUNK - 1) / MP2_CHUNK;
    if (size_t(n_entries) * size_t(chunks) > size_t(0x7fffffff) || n_cifs > (1 << 28)) return hipErrorInvalidValue;
    // (pageable memory: the copy has left `entries` when the call returns)
    hipError_t err = hipMemcpyAsync(d_table, entries, size_t(n_entries) * sizeof(Mp2Entry), hipMemcpyHostToDevice, stream);
    if (err != hipSuccess) return err;
    const Mp2Entry *table = static_cast<const Mp2Entry *>(d_table);
    Mp2Plan *plan = reinterpret_cast<Mp2Plan *>(static_cast<char *>(d_table) + size_t(n_entries) * sizeof(Mp2Entry));
    hipLaunchKernelGGL(mp2_rate_kernel, dim3(unsigned(n_entries)), dim3(64), 0, stream, table, plan, n_cifs);
    hipLaunchKernelGGL(mp2_frame_kernel, dim3(unsigned(n_entries) * unsigned(chunks)), dim3(MP2_CHUNK), 0, stream, table, plan, chunks);
    return hipGetLastError();
}

}  // namespace dabk
