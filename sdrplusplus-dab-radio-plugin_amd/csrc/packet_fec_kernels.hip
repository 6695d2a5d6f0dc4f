// packet_fec_kernels.hip -- RS(204,188) correction of the FEC frames of packet-mode sub-channels (dabgpu_packet_fec_dev;
// contract and code: include/dabgpu_packet_fec.h, shared with the host twin and the host mirror).
//
// The window of an entry is its D carried frames followed by the call's n frames.  Four launches on the caller's stream, no
// host synchronisation, no global atomics; what one launch leaves for the next lies behind the entry table in the stage area.
//
// Move: a wave takes 64 / S whole frames of the window and copies each to where it goes -- the first n to d_out, the last D
// into the new state record -- by wave_copy (16-byte accesses where source and destination share a phase, else 4-byte, else
// a byte a lane; d_in and d_out may lie on any byte).  A fresh start has no carried frames: padding packets are written.  A
// lane per slot of a new frame writes its mark, from the bytes as received.
//
// Accept: one wave per entry.  A lane per new slot counts the nine marks that would end a frame there; the candidates of 64
// slots come out as one ballot and lane 0 resolves the accept chain in order (dabgpu_packet_fec::judge).  The list of accepted
// frames and the call's counters go to the stage area, the new record's head to d_state_out.
//
// Correct: one workgroup of 192 lanes per accepted frame (the grid is sized for the most there can be; the rest exit).  The
// 2472 bytes go into LDS as they lie in the stream.  Lane t takes bytes t, t + 192, ... of the data table and byte t of the
// RS data table: 192 = 16 x 12, so a lane stays in row t mod 12, and neighbouring lanes read neighbouring bytes -- four lanes
// to a bank, the same dword, a broadcast: no conflict.  (A lane per row walking its row would read at a stride of 12 bytes =
// 3 dwords: twelve lanes, no conflict either, but 204 dependent steps on 12 of 192 lanes.)  Each byte costs one log look-up
// and 16 independent exp look-ups (dabgpu_packet_fec::syndrome_add; a Horner chain would be 16 x 204 dependent three-look-up
// multiplications a row -- dabplus_kernels.hip, rs_syndromes, records what that cost there).  The 16 partial sums of a row
// meet through LDS.  Rows whose syndromes are not all zero: Berlekamp-Massey on one lane a row (its arrays in LDS, indexed by
// variables), the 204 positions of the Chien search on the row's 16 lanes with Forney's value at each root, then one lane a
// row holds the pattern to the definition and writes the corrected data bytes to where the move launch put them.
//
// Tally: one wave per entry sums the frames' counts into the result record.
//
// The GF tables come from a constexpr table, copied into LDS by all lanes, as in dabplus_kernels.hip.  That file keeps its own
// copy of the table and of gmul / gdiv: sharing them through a header would have meant rebuilding its code object.
#include <hip/hip_runtime.h>

#include "../../include/dabgpu_packet_fec.h"
#include "kernels.hpp"
#include "wave_copy.hpp"

namespace dabk {
namespace {

namespace fec = dabgpu_packet_fec;

__device__ const fec::Gf GF_TABLES = fec::make_gf();

constexpr int CORRECT_LANES = 192;        // 16 lanes a row
constexpr int ACCEPT_HEAD_WORDS = 16;     // count, 3 x 0, the call's Counters (12 words); then the accepted ends
constexpr int COUNT_WORDS = 8;            // a frame's FrameCounts, 3 x 0
static_assert(sizeof(fec::Counters) == 48 && sizeof(fec::FrameCounts) == 20 && CORRECT_LANES == fec::ROWS * fec::T2, "records of the stage area");

// the head of the entry's state record into LDS (zeros when there is none); a barrier is left to the caller
__device__ __forceinline__ void load_head(const PacketFecEntry &e, fec::Head &h, int lane) {
    if (lane < fec::HEAD_BYTES / 16)
        reinterpret_cast<uint4 *>(&h)[lane] = e.state_in ? reinterpret_cast<const uint4 *>(e.state_in)[lane] : make_uint4(0u, 0u, 0u, 0u);
}

// where frame wf of the window goes: the first n_cifs to d_out, the rest into the new state record
__device__ __forceinline__ uint8_t *window_frame(const PacketFecEntry &e, int n_cifs, int wf) {
    return wf < n_cifs ? reinterpret_cast<uint8_t *>(e.out) + uint64_t(wf) * e.out_stride
                       : reinterpret_cast<uint8_t *>(e.state_out) + fec::HEAD_BYTES + size_t(wf - n_cifs) * size_t(fec::SLOT_BYTES * e.s);
}

__global__ __launch_bounds__(64) void packet_fec_move_kernel(const PacketFecEntry *table, int n_cifs, unsigned blocks_per_entry) {
    __shared__ fec::Head h;
    const unsigned entry = blockIdx.x / blocks_per_entry, block = blockIdx.x - entry * blocks_per_entry;
    const PacketFecEntry e = table[entry];
    const int lane = threadIdx.x, S = e.s, D = fec::delay(S), fb = fec::SLOT_BYTES * S, F = 64 / S;
    const int total = D + n_cifs;
    const int64_t f0 = int64_t(block) * F;
    if (f0 >= total) return;                                           // (an entry of larger S has fewer blocks than the grid)
    load_head(e, h, lane);
    __syncthreads();
    const bool fresh = !fec::head_ok(h, S);
    uint8_t *marks = reinterpret_cast<uint8_t *>(e.marks);
    if (block == 0) {
        if (lane < 8) marks[lane] = fresh ? fec::MARK_NONE : h.tail[lane];
        const int used = fec::HEAD_BYTES + D * fb;                     // (the record's size is rounded up to 16)
        if (used + lane < fec::state_bytes(S)) reinterpret_cast<uint8_t *>(e.state_out)[used + lane] = 0;
    }
    const int nf = total - f0 < F ? int(total - f0) : F;
    for (int k = 0; k < nf; k++) {
        const int wf = int(f0) + k;
        uint8_t *dst = window_frame(e, n_cifs, wf);
        if (wf >= D) {
            const uint8_t *src = reinterpret_cast<const uint8_t *>(e.in) + uint64_t(wf - D) * e.in_stride;
            wave_copy(dst, src, fb, lane);
            if (lane < S) marks[8 + size_t(wf - D) * S + lane] = fec::mark_of(src[fec::SLOT_BYTES * lane], src[fec::SLOT_BYTES * lane + 1]);
        } else if (fresh) {
            for (int i = lane; i < fb; i += 64) dst[i] = fec::padding_byte(i % fec::SLOT_BYTES);
        } else {
            wave_copy(dst, reinterpret_cast<const uint8_t *>(e.state_in) + fec::HEAD_BYTES + size_t(wf) * fb, fb, lane);
        }
    }
}

__global__ __launch_bounds__(64) void packet_fec_accept_kernel(const PacketFecEntry *table, int n_cifs) {
    __shared__ fec::Head h;
    __shared__ fec::Counters c;
    __shared__ int n_accepted;
    const PacketFecEntry e = table[blockIdx.x];
    const int lane = threadIdx.x, S = e.s;
    load_head(e, h, lane);
    __syncthreads();
    if (lane == 0) {
        if (!fec::head_ok(h, S)) fec::head_fresh(h, S);
        c = fec::Counters{};
        c.cifs = n_cifs;
        c.slots = n_cifs * S;
        n_accepted = 0;
    }
    __syncthreads();
    const uint8_t *m = reinterpret_cast<const uint8_t *>(e.marks) + 8;  // m[j]: the mark of new slot j, j >= -8
    uint32_t *acc = reinterpret_cast<uint32_t *>(e.accepted);
    const int slots = n_cifs * S;
    const int64_t g0 = h.frames_seen * S;                              // the slot number of new slot 0
    int n_marks = 0;
    for (int base = 0; base < slots; base += 64) {
        const int j = base + lane;
        const bool valid = j < slots;
        const bool is_mark = valid && m[j] != fec::MARK_NONE;
        const bool ends = valid && fec::ends_here([&](int64_t jj) { return m[jj]; }, j);
        n_marks += __popcll(__ballot(is_mark));
        uint64_t bits = __ballot(ends);
        if (lane == 0) {
            while (bits) {
                const int j0 = base + __ffsll(static_cast<unsigned long long>(bits)) - 1;
                bits &= bits - 1;
                if (fec::judge(h, c, g0 + j0) != fec::ACCEPTED) continue;
                if (n_accepted < e.max_frames) acc[ACCEPT_HEAD_WORDS + n_accepted++] = uint32_t(j0);
            }
        }
    }
    if (lane == 0) {
        uint8_t tail[8];
#pragma unroll
        for (int i = 0; i < 8; i++) tail[i] = m[slots - 8 + i];
#pragma unroll
        for (int i = 0; i < 8; i++) h.tail[i] = tail[i];
        h.frames_seen += n_cifs;
        c.marks = n_marks;
    }
    __syncthreads();
    if (lane < fec::HEAD_BYTES / 16) reinterpret_cast<uint4 *>(e.state_out)[lane] = reinterpret_cast<const uint4 *>(&h)[lane];
    if (lane < 4) acc[lane] = lane == 0 ? uint32_t(n_accepted) : 0u;
    if (lane < int(sizeof(fec::Counters) / 4)) acc[4 + lane] = reinterpret_cast<const uint32_t *>(&c)[lane];
}

__global__ __launch_bounds__(CORRECT_LANES) void packet_fec_correct_kernel(const PacketFecEntry *table, int n_cifs, unsigned frames_per_entry) {
    __shared__ fec::Gf g;
    __shared__ __attribute__((aligned(16))) uint8_t fr[(fec::FRAME_BYTES + 15) & ~15];
    __shared__ uint8_t part[fec::T2][CORRECT_LANES];
    __shared__ fec::RowWork work[fec::ROWS];
    __shared__ fec::FrameCounts counts[fec::ROWS];
    __shared__ uint8_t todo[fec::ROWS];                                // 0: a codeword, 1: a locator to search, 2: beyond the bound
    const unsigned entry = blockIdx.x / frames_per_entry, k = blockIdx.x - entry * frames_per_entry;
    const PacketFecEntry e = table[entry];
    const uint32_t *acc = reinterpret_cast<const uint32_t *>(e.accepted);
    const unsigned n_accepted = acc[0] < unsigned(e.max_frames) ? acc[0] : unsigned(e.max_frames);
    if (k >= n_accepted) return;
    const int t = threadIdx.x, S = e.s, D = fec::delay(S), slots = n_cifs * S;
    const uint32_t j0 = acc[ACCEPT_HEAD_WORDS + k];
    // (what the accept launch wrote; held inside the window whatever the record says)
    if (j0 >= uint32_t(slots) || D * S + int(j0) < fec::FRAME_SLOTS - 1) return;
    const int first = D * S + int(j0) - (fec::FRAME_SLOTS - 1);        // the frame's first slot, counted from the window's
    auto slot = [&](int i) {
        const int w = first + i, wf = w / S;
        return window_frame(e, n_cifs, wf) + fec::SLOT_BYTES * (w - wf * S);
    };
    reinterpret_cast<uint32_t *>(&g)[t] = reinterpret_cast<const uint32_t *>(&GF_TABLES)[t];
    if (((e.out | e.out_stride | e.state_out) & 3) == 0) {
        for (int idx = t; idx < fec::FRAME_SLOTS * 6; idx += CORRECT_LANES) {
            const int i = idx / 6, w = idx - 6 * i;
            reinterpret_cast<uint32_t *>(fr)[idx] = reinterpret_cast<const uint32_t *>(slot(i))[w];
        }
    } else {
        for (int idx = t; idx < fec::FRAME_BYTES; idx += CORRECT_LANES) {
            const int i = idx / fec::SLOT_BYTES;
            fr[idx] = slot(i)[idx - fec::SLOT_BYTES * i];
        }
    }
    __syncthreads();
    const int r = t % fec::ROWS, q = t / fec::ROWS;                    // this lane's row, and which of the row's 16 lanes it is
    {
        unsigned sy[fec::T2];
#pragma unroll
        for (int i = 0; i < fec::T2; i++) sy[i] = 0;
        for (int b = t; b < fec::DATA_BYTES; b += CORRECT_LANES) fec::syndrome_add(g, fr[b], b / fec::ROWS, sy);
        fec::syndrome_add(g, fr[fec::frame_index(r, fec::K + q)], fec::K + q, sy);
#pragma unroll
        for (int i = 0; i < fec::T2; i++) part[i][t] = uint8_t(sy[i]);
    }
    __syncthreads();
    {
        unsigned x = 0;                                                // syndrome q of row r
        for (int i = 0; i < fec::T2; i++) x ^= part[q][r + fec::ROWS * i];
        work[r].syn[q] = uint8_t(x);
    }
    __syncthreads();
    if (t < fec::ROWS) {
        fec::RowWork &w = work[t];
        w.ll = w.n = 0;
        todo[t] = fec::row_is_codeword(w) ? 0 : fec::locator(g, w) ? 1 : 2;
    }
    __syncthreads();
    if (todo[r] == 1) {
        fec::RowWork &w = work[r];
        for (int c = q; c < fec::N; c += fec::T2) {
            unsigned v;
            if (!fec::root_at(g, w, c, v)) continue;
            const int at = atomicAdd(&w.n, 1);                         // (LDS)
            if (at < fec::T) {
                w.pos[at] = uint8_t(c);
                w.val[at] = uint8_t(v);
            }
        }
    }
    __syncthreads();
    if (t < fec::ROWS) {
        const fec::RowWork &w = work[t];
        const bool holds = todo[t] == 1 && fec::pattern_holds(g, w);
        fec::FrameCounts f = {};
        fec::count_row(w, todo[t] == 0, holds, f);
        counts[t] = f;
        if (holds) {
            for (int i = 0; i < w.n; i++) {
                if (w.pos[i] >= fec::K) continue;
                const int b = fec::frame_index(t, w.pos[i]);
                slot(b / fec::SLOT_BYTES)[b % fec::SLOT_BYTES] = uint8_t(fr[b] ^ w.val[i]);
            }
        }
    }
    __syncthreads();
    if (t < COUNT_WORDS) {
        int32_t sum = 0;
        if (t < int(sizeof(fec::FrameCounts) / 4))
            for (int i = 0; i < fec::ROWS; i++) sum += reinterpret_cast<const int32_t *>(&counts[i])[t];
        reinterpret_cast<int32_t *>(e.counts)[size_t(k) * COUNT_WORDS + t] = sum;
    }
}

__global__ __launch_bounds__(64) void packet_fec_tally_kernel(const PacketFecEntry *table) {
    const PacketFecEntry e = table[blockIdx.x];
    const int lane = threadIdx.x;
    const uint32_t *acc = reinterpret_cast<const uint32_t *>(e.accepted);
    const int32_t *counts = reinterpret_cast<const int32_t *>(e.counts);
    const int n_accepted = int(acc[0] < unsigned(e.max_frames) ? acc[0] : unsigned(e.max_frames));
    int32_t clean = 0, corrected = 0, uncorrectable = 0, bytes = 0, parity = 0;
    for (int k = lane; k < n_accepted; k += 64) {
        const int32_t *f = counts + size_t(k) * COUNT_WORDS;
        clean += f[0];
        corrected += f[1];
        uncorrectable += f[2];
        bytes += f[3];
        parity += f[4];
    }
    for (int off = 1; off < 64; off <<= 1) {
        clean += __shfl_xor(clean, off);
        corrected += __shfl_xor(corrected, off);
        uncorrectable += __shfl_xor(uncorrectable, off);
        bytes += __shfl_xor(bytes, off);
        parity += __shfl_xor(parity, off);
    }
    if (lane == 0) {
        fec::Counters c;
        int32_t *words = reinterpret_cast<int32_t *>(e.result);
        c.cifs = int32_t(acc[4]);
        c.slots = int32_t(acc[5]);
        c.marks = int32_t(acc[6]);
        c.frames = int32_t(acc[7]);
        c.frames_cut = int32_t(acc[8]);
        c.frames_overlapping = int32_t(acc[9]);
        c.rows_clean = clean;
        c.rows_corrected = corrected;
        c.rows_uncorrectable = uncorrectable;
        c.bytes_corrected = bytes;
        c.parity_bytes_corrected = parity;
        c.reserved = 0;
        words[0] = c.cifs, words[1] = c.slots, words[2] = c.marks, words[3] = c.frames, words[4] = c.frames_cut, words[5] = c.frames_overlapping;
        words[6] = c.rows_clean, words[7] = c.rows_corrected, words[8] = c.rows_uncorrectable, words[9] = c.bytes_corrected;
        words[10] = c.parity_bytes_corrected, words[11] = c.reserved;
    }
}

size_t round16(size_t v) { return (v + 15) & ~size_t(15); }
size_t table_part(int n_entries) { return size_t(n_entries) * sizeof(PacketFecEntry); }
size_t marks_bytes(const PacketFecEntry &e, int n_cifs) { return round16(8 + size_t(n_cifs) * size_t(e.s)); }
size_t accepted_bytes(const PacketFecEntry &e, int n_cifs) { return round16(4 * (size_t(ACCEPT_HEAD_WORDS) + size_t(fec::max_frames(e.s, n_cifs)))); }
size_t counts_bytes(const PacketFecEntry &e, int n_cifs) { return 4 * size_t(COUNT_WORDS) * size_t(fec::max_frames(e.s, n_cifs)); }
unsigned move_blocks_per_entry(const PacketFecEntry *entries, int n_entries, int n_cifs) {
    unsigned most = 0;
    for (int i = 0; i < n_entries; i++) {
        const int F = 64 / entries[i].s;
        const unsigned blocks = unsigned((int64_t(fec::delay(entries[i].s)) + n_cifs + F - 1) / F);
        most = blocks > most ? blocks : most;
    }
    return most;
}
unsigned frames_per_entry(const PacketFecEntry *entries, int n_entries, int n_cifs) {
    unsigned most = 0;
    for (int i = 0; i < n_entries; i++) {
        const unsigned frames = unsigned(fec::max_frames(entries[i].s, n_cifs));
        most = frames > most ? frames : most;
    }
    return most;
}

}  // namespace

size_t packet_fec_table_bytes(const PacketFecEntry *entries, int n_entries, int n_cifs) {
    size_t bytes = table_part(n_entries);
    for (int i = 0; i < n_entries; i++) bytes += marks_bytes(entries[i], n_cifs) + accepted_bytes(entries[i], n_cifs) + counts_bytes(entries[i], n_cifs);
    return bytes;
}

uint64_t packet_fec_blocks(const PacketFecEntry *entries, int n_entries, int n_cifs) {
    const uint64_t move = uint64_t(n_entries) * move_blocks_per_entry(entries, n_entries, n_cifs);
    const uint64_t correct = uint64_t(n_entries) * frames_per_entry(entries, n_entries, n_cifs);
    return move > correct ? move : correct;
}

hipError_t launch_packet_fec(PacketFecEntry *entries, int n_entries, int n_cifs, void *d_table, size_t table_bytes, hipStream_t stream) {
    if (n_entries <= 0) return hipSuccess;
    if (!d_table || n_cifs < 0 || n_cifs > fec::MAX_N_CIFS || (reinterpret_cast<uintptr_t>(d_table) & 15)) return hipErrorInvalidValue;
    for (int i = 0; i < n_entries; i++) {
        const PacketFecEntry &e = entries[i];
        if (e.s < 1 || e.s > fec::MAX_SLOTS || e.in_stride < uint64_t(fec::SLOT_BYTES) * e.s || e.out_stride < uint64_t(fec::SLOT_BYTES) * e.s ||
            !e.state_out || !e.result || (n_cifs > 0 && (!e.in || !e.out)))
            return hipErrorInvalidValue;
    }
    if (table_bytes < packet_fec_table_bytes(entries, n_entries, n_cifs)) return hipErrorInvalidValue;
    if (packet_fec_blocks(entries, n_entries, n_cifs) >= (uint64_t(1) << 31)) return hipErrorInvalidValue;
    size_t at = table_part(n_entries);
    for (int i = 0; i < n_entries; i++) {
        PacketFecEntry &e = entries[i];
        const uint64_t base = uint64_t(reinterpret_cast<uintptr_t>(d_table));
        e.max_frames = fec::max_frames(e.s, n_cifs);
        e.marks = base + at;
        at += marks_bytes(e, n_cifs);
        e.accepted = base + at;
        at += accepted_bytes(e, n_cifs);
        e.counts = base + at;
        at += counts_bytes(e, n_cifs);
    }
    // (pageable memory: the copy has left `entries` when the call returns)
    hipError_t err = hipMemcpyAsync(d_table, entries, table_part(n_entries), hipMemcpyHostToDevice, stream);
    if (err != hipSuccess) return err;
    const PacketFecEntry *table = static_cast<const PacketFecEntry *>(d_table);
    const unsigned move = move_blocks_per_entry(entries, n_entries, n_cifs), frames = frames_per_entry(entries, n_entries, n_cifs);
    hipLaunchKernelGGL(packet_fec_move_kernel, dim3(unsigned(n_entries) * move), dim3(64), 0, stream, table, n_cifs, move);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    hipLaunchKernelGGL(packet_fec_accept_kernel, dim3(unsigned(n_entries)), dim3(64), 0, stream, table, n_cifs);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    hipLaunchKernelGGL(packet_fec_correct_kernel, dim3(unsigned(n_entries) * frames), dim3(CORRECT_LANES), 0, stream, table, n_cifs, frames);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    hipLaunchKernelGGL(packet_fec_tally_kernel, dim3(unsigned(n_entries)), dim3(64), 0, stream, table);
    return hipGetLastError();
}

}  // namespace dabk
