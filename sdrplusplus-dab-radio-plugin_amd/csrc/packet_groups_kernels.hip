// packet_groups_kernels.hip -- the data groups (or raw bytes) of any packet-mode component (dabgpu_packet_groups_dev;
// contract and code: include/dabgpu_data_groups.h, shared with the host twin).
//
// The scan launch of packet_kernels.hip runs first, as it stands: it leaves per frame the list of followed packets with their
// position, length and the header bytes h0 and h2.  This kernel: one workgroup of W = PACKET_GROUPS_CHUNK lanes per entry.
// Frames are taken W at a time (a prefix sum of their followed counts), their followed packets W at a time: a chunk.  In a
// chunk every packet has a lane.
//   * the useful bytes of the chunk's packets go into LDS, a wave per packet (coalesced; read once from memory)
//   * "a group is open" before each packet, were no group too long: a prefix scan of maps of {0, 1} (open_map, compose)
//   * the bytes a group has before each packet: a segmented sum of udl, segments starting at first-packets.  `have` only grows
//     inside a group, so "too long" is a threshold on that sum, and the group is really open iff it was and the sum has not
//     passed 16384.  With both, step_packet() gives every lane exactly what the serial walk does for its packet.
//   * the group CRC: every lane's register over its packet's bytes in LDS, joined by a segmented scan of (register,
//     x^(8 bytes)) pairs (crc_join): no lane runs over more than one packet
//   * a lane per closing packet parses the headers (from the group's first 16 bytes, kept per group in LDS as they arrive),
//     looks back for the repeat rule, and an (index, offset) scan over the groups to emit gives its record and byte offset
//   * the bytes go from LDS to d_bytes + offset, a wave per packet, for a group that closed in the chunk; a group still open
//     at the chunk's end is gathered in the new state record's group buffer and goes from there when it closes
// The carry from chunk to chunk is the state record's head and the emission numbers, in LDS.  Lane 0 walks nothing.
#include <hip/hip_runtime.h>

#include "../../include/dabgpu_data_groups.h"
#include "kernels.hpp"

namespace dabk {
namespace {

namespace dg = dabgpu_groups;
namespace pkt = dabgpu_packet;

constexpr int W = PACKET_GROUPS_CHUNK, WAVES = W / 64;
// a packet's useful bytes (at most 91) in LDS: 25 dwords apart, so the lanes' byte-serial CRC reads meet 64 banks
constexpr int PKT_STRIDE = 100;
static_assert(PKT_STRIDE >= pkt::MAX_PACKET_BYTES - 5 && W % 64 == 0 && W >= 64, "shape of a chunk");

struct Pair {
    uint32_t a, b;
};

// inclusive scan over the workgroup's lanes in order; op(earlier, later), op(identity, v) == v
template <class Op>
__device__ __forceinline__ Pair block_scan(Pair v, Op op, Pair identity, Pair *wave_total, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    for (int d = 1; d < 64; d <<= 1) {
        Pair u = {uint32_t(__shfl_up(int(v.a), d)), uint32_t(__shfl_up(int(v.b), d))};
        if (lane >= d) v = op(u, v);
    }
    __syncthreads();                                                   // (the totals of the scan before have been read)
    if (lane == 63) wave_total[wave] = v;
    __syncthreads();
    Pair before = identity;
    for (int w = 0; w < wave; w++) before = op(before, wave_total[w]);
    return op(before, v);
}

struct Carry {                                                         // dg::Head and the call's emission numbers
    int32_t seen, prev, open, have;
    uint32_t crc, type_mask;
    uint32_t em_count, em_offset;
    uint8_t last_ci[16];
};

struct Shared {
    __attribute__((aligned(16))) uint8_t bytes[W * PKT_STRIDE];
    __attribute__((aligned(16))) uint8_t heads[(W + 1) * dg::HEAD_BYTES];   // [0]: the group open when the chunk began
    int32_t frame_cum[W];                                              // followed packets up to and with each frame of the block
    uint32_t pk_word[W];                                               // pos | L << 8 | h0 << 16 | h2 << 24, held inside the frame
    int32_t pk_frame[W];
    int32_t h_after[W];
    int32_t a_gid[W], a_at[W];                                         // the group a packet's bytes join (-1: none), and where
    int32_t close_lane[W + 1];                                         // by group: the lane that closed it, or -1
    int32_t g_dst[W];                                                  // by closing lane: offset in d_bytes, or -1
    Pair em_incl[W];
    uint8_t open_after[W], g_acc[W], g_type[W], g_ci[W];
    Pair wave_total[WAVES];
    Carry carry;
    int32_t end_gid;                                                   // the group open at the chunk's end, or -1
    PacketGroupsEntry e;                                               // (read where they are used: vector registers, not scalar ones)
    PacketEntry se;
    int32_t counters[sizeof(dg::Counters) / 4];
};

__device__ __forceinline__ void add_counters(Shared &sh, const dg::Counters &c) {
    const int32_t *v = reinterpret_cast<const int32_t *>(&c);
#pragma unroll
    for (int i = 0; i < int(sizeof(dg::Counters) / 4); i++)
        if (v[i]) atomicAdd(&sh.counters[i], v[i]);
}

// the chunk's packets' useful bytes, LDS -> memory, a wave per packet: dst_of(p) -> where, or nullptr
template <class Where>
__device__ __forceinline__ void copy_out(const Shared &sh, int n, int tid, Where dst_of) {
    const int lane = tid & 63, wave = tid >> 6;
    for (int p = wave; p < n; p += WAVES) {
        uint8_t *dst = dst_of(p);
        if (!dst) continue;
        const int udl = int(sh.pk_word[p] >> 24) & 0x7F;
        for (int b = lane; b < udl; b += 64) dst[b] = sh.bytes[p * PKT_STRIDE + b];
    }
}

__global__ __launch_bounds__(W) void packet_groups_kernel(const PacketEntry *scan_table, const PacketGroupsEntry *table, int n_cifs) {
    __shared__ Shared sh;
    const int tid = threadIdx.x;
    if (tid < int(sizeof(PacketGroupsEntry) / 4))
        reinterpret_cast<uint32_t *>(&sh.e)[tid] = reinterpret_cast<const uint32_t *>(table + blockIdx.x)[tid];
    if (tid < int(sizeof(PacketEntry) / 4))
        reinterpret_cast<uint32_t *>(&sh.se)[tid] = reinterpret_cast<const uint32_t *>(scan_table + blockIdx.x)[tid];
    __syncthreads();
    const PacketEntry &se = sh.se;
    const int S = __builtin_amdgcn_readfirstlane(se.s), rw = packet_record_words(S);   // (the same in every lane: one scalar)
    const PacketGroupsEntry &e = sh.e;
    const uint32_t *records = reinterpret_cast<const uint32_t *>(se.records);
    const dg::State *st_in = reinterpret_cast<const dg::State *>(e.state_in);
    dg::State *st_out = reinterpret_cast<dg::State *>(e.state_out);
    uint8_t *stage = st_out->group;
    const int mode = e.mode != 0;

    if (tid == 0) {
        const dg::Head h = dg::read_head(st_in, mode);
        Carry &c = sh.carry;
        c.seen = h.seen;
        c.prev = h.prev;
        c.open = h.open;
        c.have = h.have;
        c.crc = h.crc;
        c.type_mask = h.type_mask;
        c.em_count = c.em_offset = 0;
        for (int t = 0; t < 16; t++) c.last_ci[t] = uint8_t(dg::last_ci_of(h, t));
    }
    for (int i = tid; i < int(sizeof(dg::Counters) / 4); i += W) sh.counters[i] = 0;
    __syncthreads();
    // the group open when the call began: into the new record's buffer, its first bytes into heads[0]
    {
        const int have = sh.carry.have;                                // (0 without a record, or when none is open)
        for (int i = tid; i < have; i += W) {
            const uint8_t v = st_in->group[i];
            stage[i] = v;
            if (i < dg::HEAD_BYTES) sh.heads[i] = v;
        }
    }
    // the scan's counters, a lane per frame
    dg::Counters mine = {};
    for (int k = tid; k < n_cifs; k += W) {
        const uint32_t w = records[size_t(k) * rw + 1];
        const int n = int(records[size_t(k) * rw]);
        mine.packets_followed += n < S ? n : S;
        mine.packets_fec += int(w & 0xFF);
        mine.slots_bad += int((w >> 8) & 0xFF);
        mine.packets_padding += int((w >> 16) & 0xFF);
        mine.packets_other += int(w >> 24);
    }
    if (tid == 0) {
        mine.cifs = n_cifs;
        mine.slots = n_cifs * S;
    }
    __syncthreads();

    const Pair zero = {0, 0};
    auto sum2 = [](Pair x, Pair y) { return Pair{x.a + y.a, x.b + y.b}; };
    for (int k0 = 0; k0 < n_cifs; k0 += W) {
        // ---- a block of W frames: the prefix sum of their followed counts
        {
            const int k = k0 + tid;
            int n = k < n_cifs ? int(records[size_t(k) * rw]) : 0;
            n = n < 0 ? 0 : n > S ? S : n;
            const Pair incl = block_scan(Pair{uint32_t(n), 0}, sum2, zero, sh.wave_total, tid);
            sh.frame_cum[tid] = int(incl.a);
        }
        __syncthreads();
        const int total = sh.frame_cum[W - 1];
        for (int base = 0; base < total; base += W) {
            const int n = total - base < W ? total - base : W;         // packets of this chunk
            const bool valid = tid < n;
            __syncthreads();                                           // (the chunk before has been read)
            // ---- A. every packet its lane
            int k = 0, pos = 0, L = 1;
            dg::Packet q = dg::packet_fields(0, 0x80, 1);              // (no lane: a command packet; it changes nothing)
            if (valid) {
                const int p = base + tid;
                int lo = 0, hi = W - 1;                                // the first frame whose cumulative count is beyond p
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (sh.frame_cum[mid] > p) hi = mid;
                    else lo = mid + 1;
                }
                const int idx = p - (lo ? sh.frame_cum[lo - 1] : 0);
                k = k0 + lo;
                const uint32_t w = records[size_t(k) * rw + 4 + idx];
                pos = int(w & 0xFF);
                L = int((w >> 8) & 0xFF);
                // (what the scan wrote; held inside the frame whatever the record says)
                L = L < 1 ? 1 : L > 4 ? 4 : L;
                L = L > S ? S : L;
                pos = pos + L > S ? S - L : pos;
                q = dg::packet_fields(int((w >> 16) & 0xFF), int(w >> 24), L);
                sh.pk_word[tid] = uint32_t(pos) | (uint32_t(L) << 8) | (w & 0xFFFF0000u);
                sh.pk_frame[tid] = k;
            }
            const bool data = valid && !q.malformed && !q.cmd;
            if (tid < n && !data) sh.pk_word[tid] &= 0x80FFFFFFu;      // (udl 0: no byte of it is read)
            sh.close_lane[tid] = -1;
            if (tid == 0) {
                sh.close_lane[W] = -1;
                sh.end_gid = -1;
            }
            __syncthreads();
            {
                const int lane = tid & 63, wave = tid >> 6;
                for (int p = wave; p < n; p += WAVES) {
                    const uint32_t w = sh.pk_word[p];
                    const int udl = int(w >> 24) & 0x7F;
                    const uint8_t *src = reinterpret_cast<const uint8_t *>(se.in) + size_t(sh.pk_frame[p]) * se.in_stride +
                                         pkt::SLOT_BYTES * int(w & 0xFF) + 3;
                    for (int b = lane; b < udl; b += 64) sh.bytes[p * PKT_STRIDE + b] = src[b];
                }
            }
            const Carry cy = sh.carry;                                 // what holds before the chunk's first packet
            const int prev_ci = tid ? int((sh.pk_word[tid ? tid - 1 : 0] >> 20) & 3) : cy.prev;
            const bool brk = valid && dg::is_break(tid ? true : cy.seen != 0, prev_ci, q.ci);

            if (mode) {
                // ---- mode 1: one stream; a record per break
                const Pair own = {data ? uint32_t(q.udl) : 0u, brk ? 1u : 0u};
                const Pair incl = block_scan(own, sum2, zero, sh.wave_total, tid);
                const uint32_t at = cy.em_offset + (incl.a - own.a), index = cy.em_count + (incl.b - own.b);
                bool fits = false;
                if (brk) {
                    mine.continuity_breaks++;
                    if (index < uint32_t(e.max_groups)) {
                        dg::Record r = {};
                        r.offset = int32_t(at);
                        r.cif = k;
                        r.slot = uint8_t(pos);
                        r.flags = dg::DG_BREAK;
                        reinterpret_cast<dg::Record *>(e.groups)[index] = r;
                        mine.groups_emitted++;
                    } else {
                        mine.groups_no_room++;
                    }
                }
                if (valid && q.malformed) mine.packets_malformed++;
                else if (valid && q.cmd) mine.packets_command++;
                else if (data) {
                    fits = uint64_t(at) + uint32_t(q.udl) <= uint64_t(uint32_t(e.bytes_capacity));
                    if (fits) mine.bytes_emitted += q.udl;
                    else mine.bytes_no_room += q.udl;
                }
                sh.a_at[tid] = fits ? int32_t(at) : -1;
                __syncthreads();
                copy_out(sh, n, tid, [&](int p) { return sh.a_at[p] >= 0 ? reinterpret_cast<uint8_t *>(e.bytes) + sh.a_at[p] : nullptr; });
                __syncthreads();
                if (tid == n - 1) {
                    Carry &c = sh.carry;
                    c.seen = 1;
                    c.prev = q.ci;
                    c.em_offset = cy.em_offset + incl.a;
                    c.em_count = cy.em_count + incl.b;
                }
                continue;
            }

            // ---- B. open before each packet, were no group too long
            const uint32_t map = valid ? dg::open_map(q, brk) : dg::OPEN_MAP_IDENTITY;
            const Pair maps = block_scan(Pair{map, 0}, [](Pair x, Pair y) { return Pair{dg::compose(x.a, y.a), 0}; },
                                         Pair{dg::OPEN_MAP_IDENTITY, 0}, sh.wave_total, tid);
            sh.open_after[tid] = uint8_t(dg::apply(maps.a, cy.open));
            // ---- C. the bytes of the group so far: a sum of udl that starts again at every first-packet
            const bool head = data && q.first;
            const Pair sums = block_scan(Pair{data ? uint32_t(q.udl) : 0u, head ? 1u : 0u},
                                         [](Pair x, Pair y) { return Pair{y.b ? y.a : x.a + y.a, x.b + y.b}; }, zero, sh.wave_total, tid);
            const int gid = int(sums.b);                               // 0: the group open when the chunk began
            sh.h_after[tid] = int(sums.a) + (gid == 0 ? cy.have : 0);
            __syncthreads();
            // ---- D. the packet's step, as the serial walk takes it
            const int have_before = tid ? sh.h_after[tid - 1] : cy.have;
            int open = (tid ? sh.open_after[tid - 1] : cy.open) && have_before <= dg::GROUP_CAP;
            int have = have_before;
            int act = dg::ACT_NONE;
            if (valid) act = dg::step_packet(q, brk, open, have, mine);
            const int at = have - q.udl;                               // (of a packet that appends)
            // ---- E. its bytes: the group's first ones into heads[], their CRC piece
            dg::CrcPiece piece = {0, 1};
            if (act & dg::ACT_APPEND) {
                const uint8_t *mine_bytes = sh.bytes + tid * PKT_STRIDE;
                piece = dg::crc_piece(mine_bytes, q.udl, head ? 0xFFFFu : 0u);
                for (int b = 0; b < q.udl && at + b < dg::HEAD_BYTES; b++) sh.heads[gid * dg::HEAD_BYTES + at + b] = mine_bytes[b];
            }
            sh.a_gid[tid] = (act & dg::ACT_APPEND) ? gid : -1;
            sh.a_at[tid] = at;
            const Pair regs = block_scan(Pair{piece.reg | (piece.shift << 16), head ? 1u : 0u},
                                         [](Pair x, Pair y) {
                                             if (y.b) return Pair{y.a, x.b + y.b};
                                             const dg::CrcPiece j = dg::crc_join(dg::CrcPiece{x.a & 0xFFFF, x.a >> 16}, dg::CrcPiece{y.a & 0xFFFF, y.a >> 16});
                                             return Pair{j.reg | (j.shift << 16), x.b};
                                         },
                                         Pair{1u << 16, 0}, sh.wave_total, tid);
            uint32_t reg = regs.a & 0xFFFF;
            if (gid == 0) reg = dg::crc_join(dg::CrcPiece{cy.crc, 1}, dg::CrcPiece{regs.a & 0xFFFF, regs.a >> 16}).reg;
            __syncthreads();                                           // heads[] is whole
            // ---- F. a lane per closed group: headers, verdict
            dg::Record r = {};
            bool accepted = false;
            if (act == dg::ACT_CLOSE) {
                const int verdict = dg::close_group(sh.heads + gid * dg::HEAD_BYTES, have, reg, k, pos, r);
                dg::count_verdict(verdict, r, mine);
                accepted = verdict == dg::GROUP_ACCEPTED;
                sh.close_lane[gid] = tid;
            }
            sh.g_acc[tid] = accepted;
            sh.g_type[tid] = r.type;
            sh.g_ci[tid] = r.continuity;
            if (tid == n - 1 && open) sh.end_gid = gid;
            __syncthreads();
            // ---- G. repeats: the latest earlier accepted group of the type, in the chunk or before it
            bool emit = accepted;
            if (accepted) {
                int j = tid - 1;
                while (j >= 0 && !(sh.g_acc[j] && sh.g_type[j] == r.type)) j--;
                const bool repeat = j >= 0 ? sh.g_ci[j] == r.continuity
                                           : ((cy.type_mask >> r.type) & 1) && sh.carry.last_ci[r.type & 15] == r.continuity;
                if (repeat) {
                    mine.groups_repeated++;
                    r.flags |= dg::DG_REPEAT;
                    emit = e.keep_repeats != 0;
                }
            }
            // ---- H. the groups to emit: index and offset
            const Pair own = {emit ? 1u : 0u, emit ? dg::round16(uint32_t(have)) : 0u};
            const Pair incl = block_scan(own, [](Pair x, Pair y) { return Pair{x.a + y.a, dg::offset_add(x.b, y.b)}; }, zero, sh.wave_total, tid);
            sh.em_incl[tid] = incl;
            __syncthreads();
            int32_t dst = -1;
            if (emit) {
                const Pair excl = tid ? sh.em_incl[tid - 1] : zero;
                const uint32_t index = cy.em_count + excl.a, offset = dg::offset_add(cy.em_offset, excl.b);
                if (dg::has_room(index, offset, have, e.max_groups, e.bytes_capacity)) {
                    r.offset = int32_t(offset);
                    reinterpret_cast<dg::Record *>(e.groups)[index] = r;
                    dst = int32_t(offset);
                    mine.groups_emitted++;
                    mine.bytes_emitted += have;
                } else {
                    mine.groups_no_room++;
                }
            }
            sh.g_dst[tid] = dst;
            __syncthreads();
            // ---- I. the bytes.  The group open when the chunk began, if it closed here: its earlier bytes from the buffer
            {
                const int cl = sh.close_lane[0];
                const int32_t d0 = cl >= 0 ? sh.g_dst[cl] : -1;
                if (d0 >= 0)
                    for (int i = tid; i < cy.have; i += W) reinterpret_cast<uint8_t *>(e.bytes)[d0 + i] = stage[i];
            }
            __syncthreads();                                           // (before the buffer takes the next open group)
            copy_out(sh, n, tid, [&](int p) -> uint8_t * {
                const int g = sh.a_gid[p];
                if (g < 0) return nullptr;
                const int cl = sh.close_lane[g];
                if (cl >= 0) return sh.g_dst[cl] >= 0 ? reinterpret_cast<uint8_t *>(e.bytes) + sh.g_dst[cl] + sh.a_at[p] : nullptr;
                return g == sh.end_gid ? stage + sh.a_at[p] : nullptr;
            });
            __syncthreads();
            // ---- J. the carry
            if (tid < 16) {
                int j = n - 1;
                while (j >= 0 && !(sh.g_acc[j] && sh.g_type[j] == tid)) j--;
                if (j >= 0) {
                    sh.carry.last_ci[tid] = sh.g_ci[j];
                    atomicOr(&sh.carry.type_mask, 1u << tid);
                }
            }
            uint32_t head_word[dg::HEAD_BYTES / 4] = {};
            const bool last_lane = tid == n - 1;
            if (last_lane && open && gid != 0)
                for (int i = 0; i < dg::HEAD_BYTES / 4; i++) head_word[i] = reinterpret_cast<const uint32_t *>(sh.heads + gid * dg::HEAD_BYTES)[i];
            __syncthreads();
            if (last_lane) {
                Carry &c = sh.carry;
                c.seen = 1;
                c.prev = q.ci;
                c.open = open;
                c.have = open ? have : 0;
                c.crc = open ? reg : 0;
                c.em_count = cy.em_count + incl.a;
                c.em_offset = dg::offset_add(cy.em_offset, incl.b);
                if (open && gid != 0)
                    for (int i = 0; i < dg::HEAD_BYTES / 4; i++) reinterpret_cast<uint32_t *>(sh.heads)[i] = head_word[i];
            }
        }
        __syncthreads();
    }
    __syncthreads();
    // ---- the new record and the result
    add_counters(sh, mine);
    const int have = sh.carry.open ? sh.carry.have : 0;
    for (int i = have + tid; i < dg::GROUP_CAP; i += W) stage[i] = 0;
    if (tid == 0) {
        const Carry &c = sh.carry;
        dg::Head h = {};
        h.seen = uint8_t(c.seen);
        h.prev = uint8_t(c.prev);
        h.open = uint8_t(c.open);
        h.have = c.have;
        h.crc = c.crc;
        for (int t = 0; t < 16; t++)
            if ((c.type_mask >> t) & 1) dg::set_last_ci(h, t, c.last_ci[t]);
        dg::write_head(st_out, h);
    }
    __syncthreads();
    for (int i = tid; i < int(sizeof(dg::Counters) / 4); i += W) reinterpret_cast<int32_t *>(e.result)[i] = sh.counters[i];
}

size_t tables_bytes(int n_entries) { return size_t(n_entries) * (sizeof(PacketEntry) + sizeof(PacketGroupsEntry)); }

}  // namespace

size_t packet_groups_table_bytes(const PacketEntry *entries, int n_entries, int n_cifs) {
    return packet_table_bytes(entries, n_entries, n_cifs, false) + size_t(n_entries > 0 ? n_entries : 0) * sizeof(PacketGroupsEntry);
}

hipError_t launch_packet_groups(PacketEntry *scan, const PacketGroupsEntry *entries, int n_entries, int n_cifs, void *d_table,
                                size_t table_bytes, hipStream_t stream) {
    if (n_entries <= 0) return hipSuccess;
    if (!d_table || n_cifs < 0 || n_cifs > pkt::MAX_N_CIFS || (reinterpret_cast<uintptr_t>(d_table) & 15)) return hipErrorInvalidValue;
    for (int i = 0; i < n_entries; i++) {
        const PacketEntry &s = scan[i];
        const PacketGroupsEntry &e = entries[i];
        if (s.s < 1 || s.s > pkt::MAX_SLOTS || s.in_stride < uint64_t(pkt::SLOT_BYTES) * s.s || e.bytes_capacity < 0 || e.max_groups < 0 ||
            !e.state_out || !e.result || uint64_t(n_cifs) * uint64_t(pkt::SLOT_BYTES * s.s) >= (uint64_t(1) << 31))
            return hipErrorInvalidValue;
    }
    if (table_bytes < packet_groups_table_bytes(scan, n_entries, n_cifs)) return hipErrorInvalidValue;
    if (packet_scan_blocks(scan, n_entries, n_cifs) >= (uint64_t(1) << 31)) return hipErrorInvalidValue;
    size_t at = tables_bytes(n_entries);
    for (int i = 0; i < n_entries; i++) {
        scan[i].records = uint64_t(reinterpret_cast<uintptr_t>(d_table)) + at;
        at += size_t(n_cifs) * size_t(packet_record_words(scan[i].s)) * 4;
    }
    // (pageable memory: the copies have left the host arrays when the call returns)
    const size_t scan_bytes = size_t(n_entries) * sizeof(PacketEntry);
    hipError_t err = hipMemcpyAsync(d_table, scan, scan_bytes, hipMemcpyHostToDevice, stream);
    if (err != hipSuccess) return err;
    void *at_entries = static_cast<uint8_t *>(d_table) + scan_bytes;
    err = hipMemcpyAsync(at_entries, entries, size_t(n_entries) * sizeof(PacketGroupsEntry), hipMemcpyHostToDevice, stream);
    if (err != hipSuccess) return err;
    const PacketEntry *d_scan = static_cast<const PacketEntry *>(d_table);
    err = launch_packet_scan(d_scan, scan, n_entries, n_cifs, stream);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(packet_groups_kernel, dim3(unsigned(n_entries)), dim3(W), 0, stream, d_scan,
                       static_cast<const PacketGroupsEntry *>(at_entries), n_cifs);
    return hipGetLastError();
}

}  // namespace dabk
