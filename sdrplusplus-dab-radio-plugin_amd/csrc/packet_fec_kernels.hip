// packet_fec_kernels.hip -- RS(204,188) correction of the FEC frames of packet-mode sub-channels, errors only
// (dabgpu_packet_fec_dev) and with the failed packet CRCs as erasures (dabgpu_packet_fec_erasures_dev).  Contract:
// include/dabgpu_packet_fec.h; code: that header and include/dabgpu_packet_fec_erasures.h, shared with the host twins and the
// host mirror.
//
// One set of kernel bodies, template <bool Erasures>; the eight kernels are their instantiations under fixed names.  What the
// erasure call adds stands under `if constexpr (Erasures)`, and the errors-only kernels hold none of it.
//
// The window of an entry is its D carried frames followed by the call's n frames.  Four launches on the caller's stream, no
// host synchronisation, no global atomics; what one launch leaves for the next lies behind the entry table in the stage area.
//
// Move: a wave takes 64 / S whole frames of the window and copies each to where it goes -- the first n to d_out, the last D
// into the new state record -- by wave_copy (16-byte accesses where source and destination share a phase, else 4-byte, else
// a byte a lane; d_in and d_out may lie on any byte).  A fresh start has no carried frames: padding packets are written.  A
// lane per slot of a new frame writes its mark, from the bytes as received.
//   Erasures: a lane per slot of each arriving frame also computes dabgpu_packet::slot_verdict from the source bytes (the
//   packet CRC over 1 .. 4 slots; every slot's verdict is needed, so none is skipped).  Kind and length come out as four
//   ballots, and the frame's chain is resolved from them into one word, a suspect bit per slot, by every lane alike (S <= 64
//   steps on wave-uniform values).  The words lie in the stage area beside the marks, one per window frame: those of the D
//   carried frames are taken from the old head.
//
// Accept: one wave per entry.  A lane per new slot counts the nine marks that would end a frame there; the candidates of 64
// slots come out as one ballot and lane 0 resolves the accept chain in order (dabgpu_packet_fec::judge).  The list of accepted
// frames and the call's counters go to the stage area, the new record's head to d_state_out.
//   Erasures: it also counts the suspect bits of the new frames and packs those of the last D window frames into the new head.
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
//   Erasures: a frame none of whose rows is left over by that rule, or whose f is 0 or beyond 16, ends there.  Otherwise one
//   lane builds the erasure locator in LDS, one lane a row forms the modified syndromes and runs Berlekamp-Massey on those
//   above f, the row's 16 lanes search the 204 positions with Forney's values, and one lane a row holds the pattern to the
//   definition and writes the data bytes.  Everything indexed by a variable lies in LDS.
//
// Tally: one wave per entry sums the frames' counts into the result record (Erasures: the wider one).
//
// The GF tables come from a constexpr table, copied into LDS by all lanes, as in dabplus_kernels.hip.  That file keeps its own
// copy of the table and of gmul / gdiv: sharing them through a header would have meant rebuilding its code object.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/dabgpu_packet_fec_erasures.h"
#include "kernels.hpp"
#include "wave_copy.hpp"

namespace dabk {
namespace {

namespace fec = dabgpu_packet_fec;
namespace pkt = dabgpu_packet;

__device__ const fec::Gf GF_TABLES = fec::make_gf();

constexpr int CORRECT_LANES = 192;        // 16 lanes a row
// count, word 1 (Erasures: the new slots' suspects, else 0), 2 x 0, the call's Counters (12 words); then the accepted ends
constexpr int ACCEPT_HEAD_WORDS = 16;
// a frame's FrameCounts, 3 x 0; Erasures: its ErasureFrameCounts, with suspects, beyond erasures, 2 x 0
template <bool Erasures> constexpr int COUNT_WORDS = Erasures ? 12 : 8;
template <bool Erasures> constexpr int SUM_WORDS = Erasures ? 10 : 5;          // of those, what the tally sums
template <bool Erasures> constexpr int RESULT_WORDS = int(sizeof(std::conditional_t<Erasures, fec::ErasureCounters, fec::Counters>) / 4);
template <bool Erasures> using FrameCountsOf = std::conditional_t<Erasures, fec::ErasureFrameCounts, fec::FrameCounts>;
static_assert(sizeof(fec::Counters) == 48 && sizeof(fec::FrameCounts) == 20 && sizeof(fec::ErasureFrameCounts) == 32 &&
                  CORRECT_LANES == fec::ROWS * fec::T2 && RESULT_WORDS<false> == 12 && RESULT_WORDS<true> == 20,
              "records of the stage area");

// what only the erasure correct kernel keeps in LDS
struct ErasureLds {
    fec::ErasureWork ework[fec::ROWS];
    fec::ErasureSet es;
    uint8_t need[fec::ROWS];              // step 3: 0 no, 1 wanted, 2 an errata locator to search
};
struct NoLds {};

template <bool Erasures> __device__ __forceinline__ bool record_ok(const fec::Head &h, int S) {
    if constexpr (Erasures) return fec::head_ok_erasures(h, S);
    else return fec::head_ok(h, S);
}

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

template <bool Erasures> __device__ __forceinline__ void move_body(const PacketFecEntry *table, int n_cifs, unsigned blocks_per_entry) {
    __shared__ fec::Head h;
    const unsigned entry = blockIdx.x / blocks_per_entry, block = blockIdx.x - entry * blocks_per_entry;
    const PacketFecEntry e = table[entry];
    const int lane = threadIdx.x, S = e.s, D = fec::delay(S), fb = fec::SLOT_BYTES * S, F = 64 / S;
    const int total = D + n_cifs;
    const int64_t f0 = int64_t(block) * F;
    if (f0 >= total) return;                                           // (an entry of larger S has fewer blocks than the grid)
    load_head(e, h, lane);
    __syncthreads();
    const bool fresh = !record_ok<Erasures>(h, S);
    uint8_t *marks = reinterpret_cast<uint8_t *>(e.marks);
    [[maybe_unused]] uint64_t *sus = nullptr;                          // Erasures: [D + n_cifs], a word per window frame
    if constexpr (Erasures) sus = reinterpret_cast<uint64_t *>(e.suspects);
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
            if constexpr (Erasures) {
                const uint32_t v = lane < S ? pkt::slot_verdict(src, S, lane, 1) : uint32_t(pkt::SLOT_FEC) | (1u << 2);
                const int kind = pkt::verdict_kind(v), more = pkt::verdict_slots(v) - 1;
                const uint64_t bad = __ballot(kind == int(pkt::SLOT_BAD)), good = __ballot(kind == int(pkt::SLOT_GOOD));
                const uint64_t l0 = __ballot(more & 1), l1 = __ballot(more & 2);
                const uint64_t word = fec::suspects_of_chain(S, [&](int pos) {
                    const uint32_t kd = ((bad >> pos) & 1u) ? uint32_t(pkt::SLOT_BAD) : ((good >> pos) & 1u) ? uint32_t(pkt::SLOT_GOOD) : uint32_t(pkt::SLOT_FEC);
                    const uint32_t L = 1u + uint32_t((l0 >> pos) & 1u) + 2u * uint32_t((l1 >> pos) & 1u);
                    return kd | (L << 2);
                });
                if (lane == 0) sus[wf] = word;
            }
        } else if (fresh) {
            for (int i = lane; i < fb; i += 64) dst[i] = fec::padding_byte(i % fec::SLOT_BYTES);
            if constexpr (Erasures)
                if (lane == 0) sus[wf] = 0;
        } else {
            wave_copy(dst, reinterpret_cast<const uint8_t *>(e.state_in) + fec::HEAD_BYTES + size_t(wf) * fb, fb, lane);
            if constexpr (Erasures)
                if (lane == 0) sus[wf] = fec::get_bits(h.reserved, wf * S, S);
        }
    }
}

template <bool Erasures> __device__ __forceinline__ void accept_body(const PacketFecEntry *table, int n_cifs) {
    __shared__ fec::Head h;
    __shared__ fec::Counters c;
    __shared__ int n_accepted;
    const PacketFecEntry e = table[blockIdx.x];
    const int lane = threadIdx.x, S = e.s;
    // (what the slot loop needs of the entry is taken here, so its scalar loads go out together ahead of the barrier)
    const uint8_t *m = reinterpret_cast<const uint8_t *>(e.marks) + 8;  // m[j]: the mark of new slot j, j >= -8
    uint32_t *acc = reinterpret_cast<uint32_t *>(e.accepted);
    const int slots = n_cifs * S;
    load_head(e, h, lane);
    __syncthreads();
    if (lane == 0) {
        if (!record_ok<Erasures>(h, S)) {
            if constexpr (Erasures) fec::head_fresh_erasures(h, S);
            else fec::head_fresh(h, S);
        }
        c = fec::Counters{};
        c.cifs = n_cifs;
        c.slots = n_cifs * S;
        n_accepted = 0;
    }
    __syncthreads();
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
    [[maybe_unused]] int n_suspect = 0;                                  // Erasures: the suspect bits of the new frames
    if constexpr (Erasures) {
        const uint64_t *sus = reinterpret_cast<const uint64_t *>(e.suspects);
        const int D = fec::delay(S);
        for (int k = lane; k < n_cifs; k += 64) n_suspect += __popcll(sus[D + k]);
        for (int off = 1; off < 64; off <<= 1) n_suspect += __shfl_xor(n_suspect, off);
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
    if constexpr (Erasures) {
        const uint64_t *sus = reinterpret_cast<const uint64_t *>(e.suspects);
        const int D = fec::delay(S);
        if (lane < fec::SUSPECT_BYTES) {                               // the last D window frames' bits, carried slot i at bit i
            unsigned byte = 0;
            for (int b = 0; b < 8; b++) {
                const int i = 8 * lane + b;
                if (i >= D * S) break;
                const int wf = n_cifs + i / S;
                byte |= unsigned((sus[wf] >> (i % S)) & 1u) << b;
            }
            h.reserved[lane] = uint8_t(byte);
        }
    }
    __syncthreads();
    if (lane < fec::HEAD_BYTES / 16) reinterpret_cast<uint4 *>(e.state_out)[lane] = reinterpret_cast<const uint4 *>(&h)[lane];
    if constexpr (Erasures) {
        if (lane < 4) acc[lane] = lane == 0 ? uint32_t(n_accepted) : lane == 1 ? uint32_t(n_suspect) : 0u;
    } else {
        if (lane < 4) acc[lane] = lane == 0 ? uint32_t(n_accepted) : 0u;
    }
    if (lane < int(sizeof(fec::Counters) / 4)) acc[4 + lane] = reinterpret_cast<const uint32_t *>(&c)[lane];
}

template <bool Erasures> __device__ __forceinline__ void correct_body(const PacketFecEntry *table, int n_cifs, unsigned frames_per_entry) {
    __shared__ fec::Gf g;
    __shared__ __attribute__((aligned(16))) uint8_t fr[(fec::FRAME_BYTES + 15) & ~15];
    __shared__ uint8_t part[fec::T2][CORRECT_LANES];
    __shared__ fec::RowWork work[fec::ROWS];
    __shared__ std::conditional_t<Erasures, ErasureLds, NoLds> er;     // (never named in the errors-only kernel, so not allocated)
    __shared__ FrameCountsOf<Erasures> counts[fec::ROWS];
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
    // (the table copy stands behind the staging: the frame's global loads go out first)
    reinterpret_cast<uint32_t *>(&g)[t] = reinterpret_cast<const uint32_t *>(&GF_TABLES)[t];
    if constexpr (Erasures) {
        if (t < 128) {                                                 // the suspect bits of the 94 table slots: two ballots
            bool bit = false;
            if (t < fec::DATA_SLOTS) {
                const int w = first + t, wf = w / S;                   // (wf < D + n_cifs: the frame lies inside the window)
                bit = ((reinterpret_cast<const uint64_t *>(e.suspects)[wf] >> (w - wf * S)) & 1u) != 0;
            }
            const uint64_t b = __ballot(bit);
            if ((t & 63) == 0) er.es.slots[t >> 6] = b;
        }
    }
    __syncthreads();
    int f = 0;                                                         // Erasures: the frame's erased columns
    if constexpr (Erasures) f = 2 * (__popcll(er.es.slots[0]) + __popcll(er.es.slots[1]));
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
        FrameCountsOf<Erasures> fc = {};
        if constexpr (Erasures) {
            er.need[t] = todo[t] != 0 && !holds && f >= 2 && f <= fec::MAX_ERASED;
            if (!er.need[t]) fec::count_row(w, todo[t] == 0, holds, fc.f);
        } else {
            fec::count_row(w, todo[t] == 0, holds, fc);
        }
        counts[t] = fc;
        if (holds) fec::write_back(slot, fr, t, w.pos, w.val, w.n);
    }
    __syncthreads();
    if constexpr (Erasures) {
        unsigned any = 0;                                              // (the same for every lane: the branch is the workgroup's)
        for (int i = 0; i < fec::ROWS; i++) any |= er.need[i];
        if (any) {
            if (t == 0) fec::erasure_locator(g, er.es);
            __syncthreads();
            if (t < fec::ROWS && er.need[t]) er.need[t] = fec::errata_locator(g, er.es, work[t].syn, er.ework[t]) ? 2 : 1;
            __syncthreads();
            if (er.need[r] == 2) {
                fec::ErasureWork &w = er.ework[r];
                for (int c = q; c < fec::N; c += fec::T2) {
                    unsigned v;
                    if (!fec::errata_root_at(g, w, c, v)) continue;
                    const int at = atomicAdd(&w.n, 1);                 // (LDS)
                    if (at < fec::T2) {
                        w.pos[at] = uint8_t(c);
                        w.val[at] = uint8_t(v);
                    }
                }
            }
            __syncthreads();
            if (t < fec::ROWS && er.need[t]) {
                const fec::ErasureWork &w = er.ework[t];
                const bool holds = er.need[t] == 2 && fec::errata_holds(g, er.es, work[t].syn, w);
                fec::ErasureFrameCounts fc = counts[t];
                fec::count_erasure_row(er.es, w, holds, fc);
                counts[t] = fc;
                if (holds) fec::write_back(slot, fr, t, w.pos, w.val, w.n);
            }
            __syncthreads();
        }
    }
    if (t < COUNT_WORDS<Erasures>) {
        int32_t sum = 0;
        if (t < int(sizeof(FrameCountsOf<Erasures>) / 4))
            for (int i = 0; i < fec::ROWS; i++) sum += reinterpret_cast<const int32_t *>(&counts[i])[t];
        else if (Erasures && t == 8)
            sum = f >= 2;
        else if (Erasures && t == 9)
            sum = f > fec::MAX_ERASED;
        reinterpret_cast<int32_t *>(e.counts)[size_t(k) * COUNT_WORDS<Erasures> + t] = sum;
    }
}

template <bool Erasures> __device__ __forceinline__ void tally_body(const PacketFecEntry *table) {
    constexpr int CW = COUNT_WORDS<Erasures>, SW = SUM_WORDS<Erasures>;
    const PacketFecEntry e = table[blockIdx.x];
    const int lane = threadIdx.x;
    const uint32_t *acc = reinterpret_cast<const uint32_t *>(e.accepted);
    const int32_t *counts = reinterpret_cast<const int32_t *>(e.counts);
    const int n_accepted = int(acc[0] < unsigned(e.max_frames) ? acc[0] : unsigned(e.max_frames));
    int32_t sum[SW];
#pragma unroll
    for (int i = 0; i < SW; i++) sum[i] = 0;
    for (int k = lane; k < n_accepted; k += 64) {
        const int32_t *f = counts + size_t(k) * CW;
#pragma unroll
        for (int i = 0; i < SW; i++) sum[i] += f[i];
    }
    for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
        for (int i = 0; i < SW; i++) sum[i] += __shfl_xor(sum[i], off);
    }
    if (lane == 0) {
        int32_t *words = reinterpret_cast<int32_t *>(e.result);
        // cifs, slots, marks, frames, frames_cut, frames_overlapping: the accept launch's
        words[0] = int32_t(acc[4]), words[1] = int32_t(acc[5]), words[2] = int32_t(acc[6]), words[3] = int32_t(acc[7]);
        words[4] = int32_t(acc[8]), words[5] = int32_t(acc[9]);
        // rows_clean, rows_corrected, rows_uncorrectable, bytes_corrected, parity_bytes_corrected, reserved
        words[6] = sum[0], words[7] = sum[1], words[8] = sum[2], words[9] = sum[3], words[10] = sum[4], words[11] = 0;
        if constexpr (Erasures) {
            // slots_suspect, frames_with_suspects, frames_beyond_erasures, rows_erasure_corrected, erased_bytes_changed,
            // erasure_other_bytes_corrected, 2 x 0
            words[12] = int32_t(acc[1]), words[13] = sum[8], words[14] = sum[9], words[15] = sum[5], words[16] = sum[6], words[17] = sum[7];
            words[18] = 0, words[19] = 0;
        }
    }
}

// the kernels' names stand in traces and in the tests of the device listing
__global__ __launch_bounds__(64) void packet_fec_move_kernel(const PacketFecEntry *table, int n_cifs, unsigned blocks_per_entry) {
    move_body<false>(table, n_cifs, blocks_per_entry);
}
__global__ __launch_bounds__(64) void packet_fec_accept_kernel(const PacketFecEntry *table, int n_cifs) { accept_body<false>(table, n_cifs); }
__global__ __launch_bounds__(CORRECT_LANES) void packet_fec_correct_kernel(const PacketFecEntry *table, int n_cifs, unsigned frames_per_entry) {
    correct_body<false>(table, n_cifs, frames_per_entry);
}
__global__ __launch_bounds__(64) void packet_fec_tally_kernel(const PacketFecEntry *table) { tally_body<false>(table); }
__global__ __launch_bounds__(64) void packet_fec_erasure_move_kernel(const PacketFecEntry *table, int n_cifs, unsigned blocks_per_entry) {
    move_body<true>(table, n_cifs, blocks_per_entry);
}
__global__ __launch_bounds__(64) void packet_fec_erasure_accept_kernel(const PacketFecEntry *table, int n_cifs) { accept_body<true>(table, n_cifs); }
__global__ __launch_bounds__(CORRECT_LANES) void packet_fec_erasure_correct_kernel(const PacketFecEntry *table, int n_cifs, unsigned frames_per_entry) {
    correct_body<true>(table, n_cifs, frames_per_entry);
}
__global__ __launch_bounds__(64) void packet_fec_erasure_tally_kernel(const PacketFecEntry *table) { tally_body<true>(table); }

size_t round16(size_t v) { return (v + 15) & ~size_t(15); }
size_t table_part(int n_entries) { return size_t(n_entries) * sizeof(PacketFecEntry); }
size_t marks_bytes(const PacketFecEntry &e, int n_cifs) { return round16(8 + size_t(n_cifs) * size_t(e.s)); }
size_t accepted_bytes(const PacketFecEntry &e, int n_cifs) { return round16(4 * (size_t(ACCEPT_HEAD_WORDS) + size_t(fec::max_frames(e.s, n_cifs)))); }
size_t counts_bytes(const PacketFecEntry &e, int n_cifs, bool erasures) {
    return 4 * size_t(erasures ? COUNT_WORDS<true> : COUNT_WORDS<false>) * size_t(fec::max_frames(e.s, n_cifs));
}
size_t suspects_bytes(const PacketFecEntry &e, int n_cifs, bool erasures) {
    return erasures ? round16(8 * (size_t(fec::delay(e.s)) + size_t(n_cifs))) : 0;
}
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

size_t packet_fec_table_bytes(const PacketFecEntry *entries, int n_entries, int n_cifs, bool erasures) {
    size_t bytes = table_part(n_entries);
    for (int i = 0; i < n_entries; i++) {
        const PacketFecEntry &e = entries[i];
        bytes += marks_bytes(e, n_cifs) + accepted_bytes(e, n_cifs) + counts_bytes(e, n_cifs, erasures) + suspects_bytes(e, n_cifs, erasures);
    }
    return bytes;
}

uint64_t packet_fec_blocks(const PacketFecEntry *entries, int n_entries, int n_cifs) {
    const uint64_t move = uint64_t(n_entries) * move_blocks_per_entry(entries, n_entries, n_cifs);
    const uint64_t correct = uint64_t(n_entries) * frames_per_entry(entries, n_entries, n_cifs);
    return move > correct ? move : correct;
}

hipError_t launch_packet_fec(PacketFecEntry *entries, int n_entries, int n_cifs, bool erasures, void *d_table, size_t table_bytes, hipStream_t stream) {
    if (n_entries <= 0) return hipSuccess;
    if (!d_table || n_cifs < 0 || n_cifs > fec::MAX_N_CIFS || (reinterpret_cast<uintptr_t>(d_table) & 15)) return hipErrorInvalidValue;
    for (int i = 0; i < n_entries; i++) {
        const PacketFecEntry &e = entries[i];
        if (e.s < 1 || e.s > fec::MAX_SLOTS || e.in_stride < uint64_t(fec::SLOT_BYTES) * e.s || e.out_stride < uint64_t(fec::SLOT_BYTES) * e.s ||
            !e.state_out || !e.result || (n_cifs > 0 && (!e.in || !e.out)))
            return hipErrorInvalidValue;
    }
    if (table_bytes < packet_fec_table_bytes(entries, n_entries, n_cifs, erasures)) return hipErrorInvalidValue;
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
        at += counts_bytes(e, n_cifs, erasures);
        e.suspects = erasures ? base + at : 0;
        at += suspects_bytes(e, n_cifs, erasures);
    }
    // (pageable memory: the copy has left `entries` when the call returns)
    hipError_t err = hipMemcpyAsync(d_table, entries, table_part(n_entries), hipMemcpyHostToDevice, stream);
    if (err != hipSuccess) return err;
    const PacketFecEntry *table = static_cast<const PacketFecEntry *>(d_table);
    const unsigned move = move_blocks_per_entry(entries, n_entries, n_cifs), frames = frames_per_entry(entries, n_entries, n_cifs);
    const auto move_kernel = erasures ? packet_fec_erasure_move_kernel : packet_fec_move_kernel;
    const auto accept_kernel = erasures ? packet_fec_erasure_accept_kernel : packet_fec_accept_kernel;
    const auto correct_kernel = erasures ? packet_fec_erasure_correct_kernel : packet_fec_correct_kernel;
    const auto tally_kernel = erasures ? packet_fec_erasure_tally_kernel : packet_fec_tally_kernel;
    hipLaunchKernelGGL(move_kernel, dim3(unsigned(n_entries) * move), dim3(64), 0, stream, table, n_cifs, move);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    hipLaunchKernelGGL(accept_kernel, dim3(unsigned(n_entries)), dim3(64), 0, stream, table, n_cifs);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    hipLaunchKernelGGL(correct_kernel, dim3(unsigned(n_entries) * frames), dim3(CORRECT_LANES), 0, stream, table, n_cifs, frames);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    hipLaunchKernelGGL(tally_kernel, dim3(unsigned(n_entries)), dim3(64), 0, stream, table);
    return hipGetLastError();
}

}  // namespace dabk
