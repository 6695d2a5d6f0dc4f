// dmb_kernels.hip -- T-DMB stream-mode sub-channels to checked TS packets (dabgpu_dmb_follow_dev).  Contract and code:
// include/dabgpu_dmb.h, shared with the host twin; the outer code's pieces are include/dabgpu_packet_fec.h's.
//
// Three launches on the caller's stream, no host synchronisation, no global atomics; what one launch leaves for the next lies
// behind the entry table in the stage area (DMB_SYNC_WORDS words and a start per packet, per entry).
//
// Sync: one workgroup of 256 lanes per entry, lane phi < 204 owning phase phi.  A lane walks the positions of its phase through
// the call's rows (neighbouring lanes read neighbouring bytes) from the carried run counter, and never walks a position
// twice.  The call is resolved lock by lock: while locked, the one lane of the locked phase walks on until the eighth miss
// in a row (or the end); while unlocked, every lane that holds no candidate walks on to its next position with run >= 5 at
// or after the search's start, and the smallest candidate of the workgroup is the lock.  A candidate that the next search
// starts beyond is dropped and its lane walks on.  Every lock's emitted packets are an arithmetic progression
// (dabgpu_dmb::lock_packets): all lanes write their starts.  Then every lane walks to the end for the new run counters, and all
// lanes copy the last 2650 bytes of the stream into the new record and move the packets the old record held deferred.
//
// Packets: one workgroup of 256 lanes per emitted packet (the grid is sized for the most there can be; the rest exit).  Lane
// i < 204 fetches y[s + 204 (i mod 12) + i] from the carried bytes or the call's rows -- a wave touches twelve runs of bytes
// 12 apart, which is what the interleaver left; not staged, not tuned -- and adds it into 16 syndromes of its own
// (dabgpu_packet_fec::syndrome_add); the 204 x 16 partial sums meet through LDS in two steps of 16.  A packet that is no
// codeword: Berlekamp-Massey on one lane (its arrays in LDS), the 204 positions of the root search a lane each with Forney's
// value at every root, one lane holds the pattern to the definition, corrects or marks the packet in LDS and makes the
// record.  47 lanes write the 188 bytes as words, one lane the record as one 16-byte store.
//
// (The grid is n_entries x the largest entry's packets: with mixed bit rates -- 8 kbit/s beside 544 -- most workgroups of the
// small entries exit at once.  Not tuned.)  A packet goes behind the ones the old record held deferred: into the output, into
// the new record's deferred places, or, beyond those, nowhere (it is not decoded then).
//
// Continuity: one workgroup of 256 lanes per entry, the 8192 last counters and the census in LDS, the emitted packets in chunks
// of 256, a lane each.  Inside a chunk a lane finds the previous good packet of its PID by comparing against the chunk's PIDs
// in LDS; the first of a PID in the chunk takes the table's.  PIDs that appear for the first time get their census slots in
// stream order (a ballot per wave, the waves' counts through LDS).  Counts are LDS atomics on integers.  The last of a PID in
// the chunk writes the table.  (A lane scans the chunk's 256 PIDs in LDS twice: 256 x 256 byte reads a chunk.  3 % of the call's
// kernel time as measured; not tuned.)  Only emitted packets pass here -- deferred ones do when a later call emits them.  At the end: the result record, and the census, the table and their two head fields into the
// new state record (the sync launch wrote the rest of it).
#include <hip/hip_runtime.h>

#include "../../include/dabgpu_dmb.h"
#include "kernels.hpp"

namespace dabk {
namespace {

namespace dmb = dabgpu_dmb;
namespace fec = dabgpu_packet_fec;

__device__ const fec::Gf DMB_GF_TABLES = fec::make_gf();

constexpr int LANES = 256;
// the words the sync launch leaves in front of the packet starts
enum SyncWord { W_COUNT = 0, W_DROPPED, W_HITS, W_LOCKS, W_LOSSES, W_LOCKED, W_PHASE, W_FRESH, W_POS_LO, W_POS_HI, W_DEFERRED_IN };
static_assert(W_DEFERRED_IN < DMB_SYNC_WORDS && dmb::CODED_BYTES <= LANES && dmb::TS_BYTES % 4 == 0, "the launches' shapes");

__device__ __forceinline__ int64_t min_i64(int64_t a, int64_t b) { return a < b ? a : b; }

__global__ __launch_bounds__(LANES) void dmb_sync_kernel(const DmbEntry *table, int n_cifs) {
    __shared__ dmb::Head h;
    __shared__ long long wave_min[LANES / 64];
    __shared__ long long sh_end;
    __shared__ int sh_misses, sh_hits;
    const DmbEntry e = table[blockIdx.x];
    const int t = threadIdx.x, fb = dmb::frame_bytes(e.kbps);
    const dmb::State *old = reinterpret_cast<const dmb::State *>(e.state_in);
    dmb::State *st = reinterpret_cast<dmb::State *>(e.state_out);
    const uint8_t *in = reinterpret_cast<const uint8_t *>(e.in);
    uint32_t *sync = reinterpret_cast<uint32_t *>(e.sync);
    if (t < int(sizeof(dmb::Head) / 16)) reinterpret_cast<uint4 *>(&h)[t] = old ? reinterpret_cast<const uint4 *>(old)[t] : make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    const bool fresh = !old || !dmb::head_ok(h, e.kbps);
    __syncthreads();
    if (fresh && t == 0) dmb::head_fresh(h, e.kbps);
    __syncthreads();
    const int64_t p0 = h.pos, p1 = p0 + int64_t(fb) * n_cifs;
    const int d_in = fresh ? 0 : int(h.n_deferred);                  // (head_ok held it to DEFER_ROOM; read before lane 0 rewrites the head)

    // this lane's walk: q the next position of its phase, (row, col) where that lies in the call's rows
    const bool walker = t < dmb::CODED_BYTES;
    int64_t q = p0 + (t + dmb::CODED_BYTES - int(p0 % dmb::CODED_BYTES)) % dmb::CODED_BYTES;
    if (!walker) q = p1;
    int row = int((q - p0) / fb), col = int((q - p0) % fb);
    unsigned run = (walker && !fresh) ? old->run[t] : 0u;
    auto step = [&](int64_t &pos) {
        const bool hit = in[uint64_t(row) * e.in_stride + uint64_t(col)] == dmb::SYNC_BYTE;
        run = dmb::run_step(run, hit);
        pos = q;
        q += dmb::CODED_BYTES;
        col += dmb::CODED_BYTES;
        while (col >= fb) col -= fb, row++;
        return hit;
    };

    // (these are the same in every lane)
    bool locked = h.locked != 0;
    int64_t start = h.lock_start, from = p0;
    int misses = h.misses, hits = 0, locks = 0, losses = 0, dropped = 0, count = 0;
    int64_t cand = dmb::NEVER;
    for (;;) {
        if (locked) {
            if (walker && t == int(start % dmb::CODED_BYTES)) {
                int64_t end = dmb::NEVER, pos;
                int m = misses, hh = 0;
                while (q < p1) {
                    if (step(pos)) {
                        m = 0;
                        hh++;
                    } else if (++m == dmb::LOSS_MISSES) {
                        end = pos;
                        break;
                    }
                }
                sh_end = end;
                sh_misses = m;
                sh_hits = hh;
                cand = dmb::NEVER;
            }
            __syncthreads();
            const int64_t end = sh_end;
            hits += sh_hits;
            misses = sh_misses;
            const dmb::LockPackets lp = dmb::lock_packets(start, end, p0, p1);
            dropped += lp.dropped;
            for (int j = t; j < lp.count; j += LANES)
                if (count + j < e.max_packets)
                    sync[DMB_SYNC_WORDS + count + j] = uint32_t(lp.first + int64_t(dmb::CODED_BYTES) * j - (p0 - dmb::TAIL_BYTES));
            count += lp.count;
            __syncthreads();
            if (end == dmb::NEVER) break;
            locked = false;
            losses++;
            misses = 0;
            from = end + 1;
            if (cand < from) cand = dmb::NEVER;
        }
        if (walker && cand == dmb::NEVER) {
            int64_t pos;
            while (q < p1) {
                step(pos);
                if (run >= unsigned(dmb::LOCK_RUN) && pos >= from) {
                    cand = pos;
                    break;
                }
            }
        }
        long long best = cand;
        for (int off = 1; off < 64; off <<= 1) best = min_i64(best, __shfl_xor(best, off));
        if ((t & 63) == 0) wave_min[t >> 6] = best;
        __syncthreads();
        best = min_i64(min_i64(wave_min[0], wave_min[1]), min_i64(wave_min[2], wave_min[3]));
        __syncthreads();
        if (best == dmb::NEVER) break;
        locked = true;
        start = best;
        misses = 0;
        locks++;
        hits++;
    }
    {
        int64_t pos;
        while (q < p1) step(pos);
    }
    if (t < 208) st->run[t] = walker ? uint8_t(run) : uint8_t(0);
    if (count > e.max_packets) count = e.max_packets;
    // the packets the old record holds deferred go first: to the output, or into the new record again; what the new record
    // does not hold of its 64 places is zero (the packets launch fills the places of this call's own packets)
    const int64_t beyond = int64_t(d_in) + count - e.capacity;
    const int d_out = beyond < 0 ? 0 : beyond < dmb::DEFER_ROOM ? int(beyond) : dmb::DEFER_ROOM;
    for (int i = t; i < d_in * (dmb::TS_BYTES / 4 + 4); i += LANES) {
        const int d = i / (dmb::TS_BYTES / 4 + 4), w = i - d * (dmb::TS_BYTES / 4 + 4);
        const int fate = dmb::fate_of(d, e.capacity);
        if (fate == dmb::LOST) continue;
        const bool rec = w >= dmb::TS_BYTES / 4;
        uint32_t v = rec ? reinterpret_cast<const uint32_t *>(&old->deferred_rec[d])[w - dmb::TS_BYTES / 4]
                         : reinterpret_cast<const uint32_t *>(old->deferred_ts + size_t(d) * dmb::TS_BYTES)[w];
        if (rec && w == dmb::TS_BYTES / 4 + 1) v &= 0xFFFF1FFFu;    // (the PID of a record this code wrote has 13 bits)
        const int at = fate == dmb::EMITTED ? d : d - e.capacity;
        uint8_t *ts = fate == dmb::EMITTED ? reinterpret_cast<uint8_t *>(e.ts) : st->deferred_ts;
        dmb::Record *rs = fate == dmb::EMITTED ? reinterpret_cast<dmb::Record *>(e.records) : st->deferred_rec;
        if (rec) reinterpret_cast<uint32_t *>(&rs[at])[w - dmb::TS_BYTES / 4] = v;
        else reinterpret_cast<uint32_t *>(ts + size_t(at) * dmb::TS_BYTES)[w] = v;
    }
    for (int i = t; i < (dmb::DEFER_ROOM - d_out) * (dmb::TS_BYTES / 4); i += LANES)
        reinterpret_cast<uint32_t *>(st->deferred_ts + size_t(d_out) * dmb::TS_BYTES)[i] = 0u;
    for (int i = t; i < (dmb::DEFER_ROOM - d_out) * 4; i += LANES) reinterpret_cast<uint32_t *>(&st->deferred_rec[d_out])[i] = 0u;
    for (int j = t; j < dmb::TAIL_ROOM; j += LANES) {
        const int64_t p = p1 - dmb::TAIL_BYTES + j;
        uint8_t v = 0;
        if (j >= dmb::TAIL_BYTES) {
        } else if (p >= p0) {
            const int64_t o = p - p0;
            v = in[uint64_t(o / fb) * e.in_stride + uint64_t(o % fb)];
        } else if (p >= 0 && !fresh) {
            v = old->tail[p - (p0 - dmb::TAIL_BYTES)];
        }
        st->tail[j] = v;
    }
    if (t == 0) {
        h.pos = p1;
        h.locked = locked;
        h.lock_start = locked ? start : 0;
        h.misses = uint8_t(locked ? misses : 0);
        h.n_deferred = uint32_t(d_out);
    }
    __syncthreads();
    if (t < int(sizeof(dmb::Head) / 16)) reinterpret_cast<uint4 *>(st)[t] = reinterpret_cast<const uint4 *>(&h)[t];
    if (t < DMB_SYNC_WORDS) {
        uint32_t v = 0;
        switch (t) {
        case W_COUNT: v = uint32_t(count); break;
        case W_DEFERRED_IN: v = uint32_t(d_in); break;
        case W_DROPPED: v = uint32_t(dropped); break;
        case W_HITS: v = uint32_t(hits); break;
        case W_LOCKS: v = uint32_t(locks); break;
        case W_LOSSES: v = uint32_t(losses); break;
        case W_LOCKED: v = locked; break;
        case W_PHASE: v = locked ? uint32_t(start % dmb::CODED_BYTES) : 0xFFFFFFFFu; break;
        case W_FRESH: v = fresh; break;
        case W_POS_LO: v = uint32_t(uint64_t(p0) & 0xFFFFFFFFu); break;
        case W_POS_HI: v = uint32_t(uint64_t(p0) >> 32); break;
        default: break;
        }
        sync[t] = v;
    }
}

__global__ __launch_bounds__(LANES) void dmb_packets_kernel(const DmbEntry *table, int n_cifs, unsigned packets_per_entry) {
    __shared__ fec::Gf g;
    __shared__ __attribute__((aligned(16))) uint8_t x[208];
    __shared__ __attribute__((aligned(16))) uint8_t part[fec::T2][LANES];
    __shared__ uint8_t part2[fec::T2][16];
    __shared__ fec::RowWork w;
    __shared__ dmb::Record rec;
    __shared__ int found;
    const unsigned entry = blockIdx.x / packets_per_entry, k = blockIdx.x - entry * packets_per_entry;
    const DmbEntry e = table[entry];
    const uint32_t *sync = reinterpret_cast<const uint32_t *>(e.sync);
    const unsigned count = sync[W_COUNT] < unsigned(e.max_packets) ? sync[W_COUNT] : unsigned(e.max_packets);
    if (k >= count) return;
    const int t = threadIdx.x, fb = dmb::frame_bytes(e.kbps);
    const int64_t total = int64_t(dmb::TAIL_BYTES) + int64_t(fb) * n_cifs;     // the carried bytes, then the call's
    // where this packet goes: behind the deferred ones, into the output, the new record's deferred places, or nowhere
    const int64_t j = int64_t(sync[W_DEFERRED_IN] < unsigned(dmb::DEFER_ROOM) ? sync[W_DEFERRED_IN] : unsigned(dmb::DEFER_ROOM)) + k;
    const int fate = dmb::fate_of(j, e.capacity);
    if (fate == dmb::LOST) return;
    dmb::State *st = reinterpret_cast<dmb::State *>(e.state_out);
    uint8_t *ts_at = fate == dmb::EMITTED ? reinterpret_cast<uint8_t *>(e.ts) + size_t(j) * dmb::TS_BYTES : st->deferred_ts + size_t(j - e.capacity) * dmb::TS_BYTES;
    dmb::Record *rec_at = fate == dmb::EMITTED ? reinterpret_cast<dmb::Record *>(e.records) + j : &st->deferred_rec[j - e.capacity];
    int64_t rel = sync[DMB_SYNC_WORDS + k];
    // (what the sync launch wrote lies inside the carried and the new bytes; held there whatever a record says)
    if (rel + dmb::SPAN > total) rel = total - dmb::SPAN;
    if (rel < 0) rel = 0;
    const bool fresh = sync[W_FRESH] != 0;
    const int64_t p0 = int64_t((uint64_t(sync[W_POS_HI]) << 32) | sync[W_POS_LO]);
    if (t < dmb::CODED_BYTES) {
        const int64_t r = dmb::gather_at(rel, t);
        uint8_t v = 0;
        if (r >= dmb::TAIL_BYTES) {
            const int64_t o = r - dmb::TAIL_BYTES;
            v = reinterpret_cast<const uint8_t *>(e.in)[uint64_t(o / fb) * e.in_stride + uint64_t(o % fb)];
        } else if (!fresh) {
            v = reinterpret_cast<const dmb::State *>(e.state_in)->tail[r];
        }
        x[t] = v;
    }
    // (the table copy stands behind the gather: the packet's global loads go out first)
    if (t < int(sizeof(fec::Gf) / 4)) reinterpret_cast<uint32_t *>(&g)[t] = reinterpret_cast<const uint32_t *>(&DMB_GF_TABLES)[t];
    __syncthreads();
    {
        unsigned sy[fec::T2];
#pragma unroll
        for (int i = 0; i < fec::T2; i++) sy[i] = 0;
        if (t < dmb::CODED_BYTES) fec::syndrome_add(g, x[t], t, sy);
#pragma unroll
        for (int i = 0; i < fec::T2; i++) part[i][t] = uint8_t(sy[i]);
    }
    __syncthreads();
    {
        const uint4 v = reinterpret_cast<const uint4 *>(&part[t >> 4][0])[t & 15];   // 16 lanes' sums of syndrome t / 16
        unsigned f = v.x ^ v.y ^ v.z ^ v.w;
        f ^= f >> 16;
        f ^= f >> 8;
        part2[t >> 4][t & 15] = uint8_t(f);
    }
    __syncthreads();
    if (t < fec::T2) {
        unsigned f = 0;
        for (int i = 0; i < 16; i++) f ^= part2[t][i];
        w.syn[t] = uint8_t(f);
    }
    if (t == 0) w.ll = w.n = 0, found = 0;
    __syncthreads();
    const bool codeword = fec::row_is_codeword(w);                   // (the same in every lane: the branch is the workgroup's)
    if (!codeword) {
        if (t == 0) found = fec::locator(g, w) ? 1 : 0;
        __syncthreads();
        if (found && t < dmb::CODED_BYTES) {
            unsigned v;
            if (fec::root_at(g, w, t, v)) {
                const int at = atomicAdd(&w.n, 1);                   // (LDS)
                if (at < fec::T) {
                    w.pos[at] = uint8_t(t);
                    w.val[at] = uint8_t(v);
                }
            }
        }
        __syncthreads();
    }
    if (t == 0) {
        const bool holds = !codeword && found && fec::pattern_holds(g, w);
        rec = dmb::finish_packet(x, w, codeword, holds, p0 - dmb::TAIL_BYTES + rel);
    }
    __syncthreads();
    if (t < dmb::TS_BYTES / 4)
        reinterpret_cast<uint32_t *>(ts_at)[t] = reinterpret_cast<const uint32_t *>(x)[t];
    if (t == 64) *reinterpret_cast<uint4 *>(rec_at) = *reinterpret_cast<const uint4 *>(&rec);
}

// the counts of a call that the continuity launch sums
enum Sum { S_CLEAN = 0, S_CORRECTED, S_UNCORRECTABLE, S_BYTES, S_PARITY, S_DISCONTINUITIES, S_DUPLICATES, S_WORDS };

__global__ __launch_bounds__(LANES) void dmb_continuity_kernel(const DmbEntry *table, int n_cifs) {
    __shared__ __attribute__((aligned(16))) uint8_t last[dmb::PIDS];
    __shared__ __attribute__((aligned(16))) dmb::CensusEntry census[dmb::CENSUS];
    __shared__ uint16_t chunk_pid[LANES];
    __shared__ uint8_t chunk_cc[LANES];
    __shared__ int wave_new[LANES / 64];
    __shared__ int n_pids, overflowed;
    __shared__ int sums[S_WORDS];
    const DmbEntry e = table[blockIdx.x];
    const int t = threadIdx.x;
    const uint32_t *sync = reinterpret_cast<const uint32_t *>(e.sync);
    const dmb::State *old = reinterpret_cast<const dmb::State *>(e.state_in);
    dmb::State *st = reinterpret_cast<dmb::State *>(e.state_out);
    const bool fresh = sync[W_FRESH] != 0;
    const int completed = int(sync[W_COUNT] < unsigned(e.max_packets) ? sync[W_COUNT] : unsigned(e.max_packets));
    const int d_in = int(sync[W_DEFERRED_IN] < unsigned(dmb::DEFER_ROOM) ? sync[W_DEFERRED_IN] : unsigned(dmb::DEFER_ROOM));
    const int64_t all = int64_t(d_in) + completed;                    // the packets of the call; the first `capacity` are emitted
    const int count = int(all < e.capacity ? all : e.capacity);
    const int64_t held = all - count < dmb::DEFER_ROOM ? all - count : dmb::DEFER_ROOM;
    const int n_old = fresh ? 0 : int(old->head.n_pids);           // (head_ok held it to CENSUS)
    for (int i = t; i < dmb::PIDS / 16; i += LANES)
        reinterpret_cast<uint4 *>(last)[i] = fresh ? make_uint4(~0u, ~0u, ~0u, ~0u) : reinterpret_cast<const uint4 *>(old->last)[i];
    for (int i = t; i < int(sizeof(census) / 4); i += LANES)
        reinterpret_cast<uint32_t *>(census)[i] = i / 5 < n_old ? reinterpret_cast<const uint32_t *>(old->census)[i] : 0u;
    if (t == 0) n_pids = n_old, overflowed = fresh ? 0 : int(old->head.pids_overflowed);
    if (t < S_WORDS) sums[t] = 0;
    __syncthreads();
    const dmb::Record *records = reinterpret_cast<const dmb::Record *>(e.records);
    for (int base = 0; base < count; base += LANES) {
        const int i = base + t;
        dmb::Record r = {};
        if (i < count) *reinterpret_cast<uint4 *>(&r) = reinterpret_cast<const uint4 *>(records)[i];
        const bool good = i < count && r.status != dmb::UNCORRECTABLE;
        const unsigned pid = r.pid & 0x1FFFu, cc = r.byte3 & 15u;
        chunk_pid[t] = good ? uint16_t(pid) : uint16_t(0xFFFF);
        chunk_cc[t] = uint8_t(cc);
        __syncthreads();
        unsigned previous = dmb::NO_COUNTER;
        bool first_here = true, last_here = true, is_new = false;
        if (good) {
            for (int j = 0; j < t; j++)
                if (chunk_pid[j] == pid) previous = chunk_cc[j], first_here = false;
            for (int j = t + 1; j < LANES && last_here; j++) last_here = chunk_pid[j] != pid;
            if (first_here) previous = last[pid];
            is_new = first_here && previous == dmb::NO_COUNTER;
        }
        // the census slots of PIDs that appear for the first time, in stream order
        const uint64_t ballot = __ballot(is_new);
        if ((t & 63) == 0) wave_new[t >> 6] = __popcll(ballot);
        __syncthreads();
        int rank = __popcll(ballot & ((uint64_t(1) << (t & 63)) - 1)), all_new = 0;
        for (int wv = 0; wv < LANES / 64; wv++) {
            if (wv < (t >> 6)) rank += wave_new[wv];
            all_new += wave_new[wv];
        }
        const int n_before = n_pids;
        if (is_new && n_before + rank < dmb::CENSUS) {
            dmb::CensusEntry c = {};
            c.pid = uint16_t(pid);
            census[n_before + rank] = c;
        }
        __syncthreads();
        if (t == 0) {
            const int room = dmb::CENSUS - n_before, added = all_new < room ? all_new : room;
            n_pids = n_before + added;
            overflowed += all_new - added;
        }
        __syncthreads();
        if (good) {
            const int v = dmb::continuity(r, previous);
            const int slot = dmb::census_find(census, n_pids, pid);
            if (slot >= 0) {
                atomicAdd(&census[slot].packets, 1u);              // (LDS, as all of these)
                if (v == dmb::DISCONTINUITY) atomicAdd(&census[slot].discontinuities, 1u);
                if (v == dmb::DUPLICATE) atomicAdd(&census[slot].duplicates, 1u);
                if (dmb::scrambled(r)) atomicAdd(&census[slot].scrambled, 1u);
            }
            atomicAdd(&sums[r.status == dmb::CORRECTED ? S_CORRECTED : S_CLEAN], 1);
            if (r.corrected_data) atomicAdd(&sums[S_BYTES], int(r.corrected_data));
            if (r.corrected_parity) atomicAdd(&sums[S_PARITY], int(r.corrected_parity));
            if (v == dmb::DISCONTINUITY) atomicAdd(&sums[S_DISCONTINUITIES], 1);
            if (v == dmb::DUPLICATE) atomicAdd(&sums[S_DUPLICATES], 1);
            if (last_here) last[pid] = uint8_t(cc);
        } else if (i < count) {
            atomicAdd(&sums[S_UNCORRECTABLE], 1);
        }
        __syncthreads();
    }
    for (int i = t; i < dmb::PIDS / 16; i += LANES) reinterpret_cast<uint4 *>(st->last)[i] = reinterpret_cast<const uint4 *>(last)[i];
    for (int i = t; i < int(sizeof(census) / 4); i += LANES) reinterpret_cast<uint32_t *>(st->census)[i] = reinterpret_cast<const uint32_t *>(census)[i];
    if (t == 0) {
        st->head.n_pids = uint8_t(n_pids);
        st->head.pids_overflowed = uint32_t(overflowed);
        dmb::Result res = {};
        res.cifs = n_cifs;
        res.bytes = dmb::frame_bytes(e.kbps) * n_cifs;
        res.sync_hits = int32_t(sync[W_HITS]);
        res.locks = int32_t(sync[W_LOCKS]);
        res.lock_losses = int32_t(sync[W_LOSSES]);
        res.packets_emitted = count;
        res.packets_clean = sums[S_CLEAN];
        res.packets_corrected = sums[S_CORRECTED];
        res.packets_uncorrectable = sums[S_UNCORRECTABLE];
        res.packets_dropped = int32_t(sync[W_DROPPED]);
        res.bytes_corrected = sums[S_BYTES];
        res.parity_bytes_corrected = sums[S_PARITY];
        res.discontinuities = sums[S_DISCONTINUITIES];
        res.duplicates = sums[S_DUPLICATES];
        res.locked = int32_t(sync[W_LOCKED]);
        res.phase = int32_t(sync[W_PHASE]);
        res.pids = n_pids;
        res.pids_overflowed = overflowed;
        res.packets_deferred = int32_t(held);
        res.packets_lost = int32_t(all - count - held);
        *reinterpret_cast<dmb::Result *>(e.result) = res;
    }
}

size_t round16(size_t v) { return (v + 15) & ~size_t(15); }
size_t table_part(int n_entries) { return round16(size_t(n_entries) * sizeof(DmbEntry)); }
size_t sync_bytes(const DmbEntry &e) { return round16(4 * (size_t(DMB_SYNC_WORDS) + size_t(e.max_packets))); }

}  // namespace

uint64_t dmb_blocks(const DmbEntry *entries, int n_entries) {
    uint64_t most = 0;
    for (int i = 0; i < n_entries; i++) most = uint64_t(entries[i].max_packets) > most ? uint64_t(entries[i].max_packets) : most;
    return most * uint64_t(n_entries > 0 ? n_entries : 0);
}

size_t dmb_table_bytes(const DmbEntry *entries, int n_entries) {
    size_t bytes = table_part(n_entries);
    for (int i = 0; i < n_entries; i++) bytes += sync_bytes(entries[i]);
    return bytes;
}

hipError_t launch_dmb(DmbEntry *entries, int n_entries, int n_cifs, void *d_table, size_t table_bytes, hipStream_t stream) {
    if (n_entries <= 0) return hipSuccess;
    if (!d_table || n_entries > DMB_MAX_ENTRIES || n_cifs < 0 || n_cifs > dmb::MAX_N_CIFS || (reinterpret_cast<uintptr_t>(d_table) & 15))
        return hipErrorInvalidValue;
    unsigned most = 0;
    for (int i = 0; i < n_entries; i++) {
        const DmbEntry &e = entries[i];
        if (!dmb::bitrate_ok(e.kbps) || e.in_stride < uint64_t(dmb::frame_bytes(e.kbps)) || !e.state_out || !e.result || (n_cifs > 0 && !e.in) ||
            e.max_packets != dmb::new_packets(e.kbps, n_cifs) || e.capacity < 0 || (e.capacity > 0 && (!e.ts || !e.records)))
            return hipErrorInvalidValue;
        most = unsigned(e.max_packets) > most ? unsigned(e.max_packets) : most;
    }
    if (table_bytes < dmb_table_bytes(entries, n_entries) || dmb_blocks(entries, n_entries) > DMB_MAX_BLOCKS) return hipErrorInvalidValue;
    size_t at = table_part(n_entries);
    for (int i = 0; i < n_entries; i++) {
        entries[i].sync = uint64_t(reinterpret_cast<uintptr_t>(d_table)) + at;
        at += sync_bytes(entries[i]);
    }
    // (pageable memory: the copy has left `entries` when the call returns)
    hipError_t err = hipMemcpyAsync(d_table, entries, size_t(n_entries) * sizeof(DmbEntry), hipMemcpyHostToDevice, stream);
    if (err != hipSuccess) return err;
    const DmbEntry *table = static_cast<const DmbEntry *>(d_table);
    hipLaunchKernelGGL(dmb_sync_kernel, dim3(unsigned(n_entries)), dim3(LANES), 0, stream, table, n_cifs);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    if (most > 0) {
        hipLaunchKernelGGL(dmb_packets_kernel, dim3(unsigned(n_entries) * most), dim3(LANES), 0, stream, table, n_cifs, most);
        if ((err = hipGetLastError()) != hipSuccess) return err;
    }
    hipLaunchKernelGGL(dmb_continuity_kernel, dim3(unsigned(n_entries)), dim3(LANES), 0, stream, table, n_cifs);
    return hipGetLastError();
}

}  // namespace dabk
