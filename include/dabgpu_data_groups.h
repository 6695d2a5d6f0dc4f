/* dabgpu_data_groups.h -- the MSC data groups (or, without data groups, the raw useful bytes) of ANY packet-mode service
 * component, from the logical frames of its sub-channel: TPEG, SPI/EPG, Journaline, filecasting, transparent data channels.
 *
 * One implementation of the contract below (EN 300 401 clauses 5.3.2 and 5.3.3): the kernel behind dabgpu_packet_groups_dev
 * (csrc/packet_groups_kernels.hip, a lane per followed packet), the host twin dabgpu_packet_groups_host and the serial walk
 * in this file all run these functions.  Plain C++17, header-only, no allocation, no table in memory; __host__ __device__
 * under hipcc.  Nothing here interprets the content of a group.
 *
 * THE CONTRACT of one entry (a sub-channel and one packet address) in one call, every ambiguity decided.
 *
 * The scan of a frame (rules 1-4) and steps a-e of "Followed packets" are dabgpu_packet_walk.h's, word for word, with its
 * counters: cifs, slots, slots_bad, packets_*, continuity_breaks, groups_opened, groups_unfinished, groups_too_long,
 * group_bytes.  The cap on a group is 16384 bytes.
 *
 * MODE 0 (the component's DG flag is 0: data groups are used).
 *   f. the udl bytes from offset 3 are appended; group_bytes += udl.
 *   g. last: the group closes with n = have bytes, groups_closed++, and no group is open.  First match wins:
 *        n < 4                                              -> groups_malformed++   (as the slides call decides)
 *        b0 = byte 0: extension flag 0x80, CRC flag 0x40, segment flag 0x20, user access flag 0x10, type = b0 & 0x0F;
 *        byte 1: continuity = high nibble, repetition = low nibble.
 *        CRC flag set and the CRC (the packet CRC's polynomial, start and complement) over bytes 0 .. n - 3 is not bytes
 *          n - 2, n - 1 (big-endian)                        -> groups_crc_failed++  (the CRC is judged before the headers,
 *                                                              as in "Closing a group" of the slideshow contract)
 *        end = n - 2 with the CRC flag, else n; o = 2
 *        extension flag: o + 2 > end -> groups_malformed++; extension = the 16 bits at o; o += 2
 *        segment flag:   o + 2 > end -> groups_malformed++; segment = the 16 bits at o (last(1) number(15)); o += 2
 *        user access flag: o + 1 > end -> groups_malformed++; ua = byte at o; o += 1; li = ua & 0x0F;
 *          transport-id flag (ua & 0x10) set and li < 2 -> groups_malformed++; o + li > end -> groups_malformed++;
 *          transport id = the 16 bits at o when its flag is set; the end user address is the other li - 2 (or li) bytes;
 *          o += li
 *        the group is ACCEPTED: data field = bytes o .. end - 1 (it may be empty).  CRC flag clear: groups_no_crc++.
 *
 * Repeats.  An accepted group is a repeat when the latest earlier accepted group of the same type on this entry (this call
 * or an earlier one, emitted or not) has the same continuity index: groups_repeated++ (whatever keep_repeats says).  With
 * keep_repeats == 0 it is not emitted; otherwise it is, with DG_REPEAT in its flags.
 *
 * Emission.  The groups to emit (accepted, and not a repeat unless repeats are kept) are numbered i = 0, 1, ... in closing
 * order within THIS call; offset_i = the sum over j < i of length_j rounded up to 16 (held at 2^31 once it reaches it).
 * Group i is emitted iff i < max_groups and offset_i + length_i <= bytes_capacity: groups_emitted++, bytes_emitted +=
 * length_i, its n bytes at d_bytes + offset_i and record i at d_groups + i; else groups_no_room++.  The emitted groups are
 * therefore a prefix of the groups to emit.  Records beyond the emitted ones and bytes outside the emitted groups are not
 * written.
 *
 * MODE 1 (DG flag 1: no data groups).  Steps a, b, c as above, except that nothing is ever open: a break leaves a record
 * (below) instead of dropping.  A packet that passes them contributes its udl bytes to one stream; first and last are not
 * looked at.  at = the sum of udl of the contributing packets before it in THIS call.  It is emitted (its bytes at d_bytes +
 * at, bytes_emitted += udl) iff at + udl <= bytes_capacity; else bytes_no_room += udl.  Every continuity break is numbered
 * i = 0, 1, ... within this call; with i < max_groups record i is {offset = at of the packet that broke, length 0, cif, slot,
 * flags = DG_BREAK, every other field 0} and groups_emitted++, else groups_no_room++.  The other groups_* counters stay 0,
 * group_bytes too.
 * An open group in the state record is forgotten without a count.
 *
 * The state record: seen, prev, open, have, the CRC register over the open group (not complemented), the last continuity
 * index per type (16 bytes and a mask), and the open group's bytes (16384; zero behind `have`).  All zero = a fresh start; a
 * record this code did not write is a fresh start, and no value in it makes a call read or write outside the record.  A
 * stream may be cut into calls anywhere; a group may span any number of calls.
 */
#ifndef DABGPU_DATA_GROUPS_H
#define DABGPU_DATA_GROUPS_H

#include "dabgpu_packet_walk.h"

namespace dabgpu_groups {

namespace pad = dabgpu_pad;
namespace pkt = dabgpu_packet;

constexpr int GROUP_CAP = 16384;
constexpr int HEAD_BYTES = 16;            /* of a group: more than the headers read (2 + 2 + 2 + 1 + 2) */
constexpr int RECORD_BYTES = 32;
constexpr uint32_t OFFSET_SAT = 0x80000000u;

enum Flag : uint16_t {
    DG_EXTENSION = 1, DG_CRC = 2, DG_SEGMENT = 4, DG_USER_ACCESS = 8, DG_TRANSPORT_ID = 16, DG_REPEAT = 32, DG_BREAK = 64
};

struct Record {                           /* == dabgpu_data_group */
    int32_t offset, length, cif;
    uint8_t slot, type, continuity, repetition;
    uint16_t flags, extension;
    int32_t segment, transport_id;
    uint16_t data_offset, data_length;
};

struct Counters {                         /* == dabgpu_packet_groups_result */
    int32_t cifs, slots, slots_bad;
    int32_t packets_fec, packets_padding, packets_other, packets_followed;
    int32_t continuity_breaks, packets_malformed, packets_command, packets_orphan;
    int32_t groups_opened, groups_unfinished, groups_too_long;
    int32_t group_bytes;
    int32_t groups_closed, groups_malformed, groups_crc_failed, groups_no_crc;
    int32_t groups_repeated, groups_emitted, groups_no_room;
    int32_t bytes_emitted, bytes_no_room;
    int32_t reserved[4];
};

struct alignas(16) State {                /* all zero = a fresh start */
    uint8_t seen, prev, open, pad;
    uint16_t have;                        /* bytes of the open group */
    uint16_t crc;                         /* the register over them (start all ones, not complemented) */
    uint16_t type_mask;                   /* types of which an accepted group has been seen */
    uint8_t reserved[6];
    uint8_t last_ci[16];                  /* ... and the continuity index of the latest one */
    uint8_t group[GROUP_CAP];
};
static_assert(sizeof(Record) == RECORD_BYTES && sizeof(Counters) == 112 && sizeof(State) == 32 + GROUP_CAP, "records of the ABI");
constexpr int STATE_HEAD_BYTES = 32;      /* of the record, in front of the group's bytes */

/* what a call keeps in registers: the record's head */
struct Head {
    uint8_t seen, prev, open;
    int32_t have;
    uint32_t crc;
    uint32_t type_mask;
    uint64_t last_ci;                     /* a nibble per type */
};
DABGPU_MOT_FN int last_ci_of(const Head &h, int type) { return int((h.last_ci >> (4 * type)) & 15); }
DABGPU_MOT_FN void set_last_ci(Head &h, int type, int ci) {
    h.last_ci = (h.last_ci & ~(uint64_t(15) << (4 * type))) | (uint64_t(ci) << (4 * type));
    h.type_mask |= 1u << type;
}

/* the head of a record, a fresh start when this code did not write it */
DABGPU_MOT_FN Head read_head(const State *st, int mode) {
    Head h = {};
    if (!st) return h;
    bool ok = st->seen <= 1 && st->prev <= 3 && st->open <= 1 && st->pad == 0 && st->have <= GROUP_CAP &&
              (st->open || (st->have == 0 && st->crc == 0)) && (st->seen || (st->prev == 0 && !st->open));
    for (int i = 0; i < 6; i++) ok = ok && st->reserved[i] == 0;
    for (int t = 0; t < 16; t++) ok = ok && st->last_ci[t] <= (((st->type_mask >> t) & 1) ? 15 : 0);
    if (!ok) return h;
    h.seen = st->seen;
    h.prev = st->prev;
    h.type_mask = st->type_mask;
    for (int t = 0; t < 16; t++) h.last_ci |= uint64_t(st->last_ci[t]) << (4 * t);
    if (mode == 0 && st->open) {
        h.open = 1;
        h.have = st->have;
        h.crc = st->crc;
    }
    return h;
}
DABGPU_MOT_FN void write_head(State *st, const Head &h) {
    st->seen = h.seen;
    st->prev = h.prev;
    st->open = h.open;
    st->pad = 0;
    st->have = uint16_t(h.open ? h.have : 0);
    st->crc = uint16_t(h.open ? h.crc : 0);
    st->type_mask = uint16_t(h.type_mask);
    for (int i = 0; i < 6; i++) st->reserved[i] = 0;
    for (int t = 0; t < 16; t++) st->last_ci[t] = uint8_t(last_ci_of(h, t));
}

/* ---- one followed packet, from the two header bytes the scan keeps -------------------------------------------------- */
struct Packet {
    int ci, first, last, cmd, udl, malformed;
};
DABGPU_MOT_FN Packet packet_fields(int h0, int h2, int L) {
    Packet p;
    p.ci = (h0 >> 4) & 3;
    p.first = (h0 >> 3) & 1;
    p.last = (h0 >> 2) & 1;
    p.cmd = h2 >> 7;
    p.udl = h2 & 0x7F;
    p.malformed = p.udl > pkt::SLOT_BYTES * L - 5;
    return p;
}
DABGPU_MOT_FN bool is_break(bool seen, int prev, int ci) { return seen && ci != ((prev + 1) & 3); }

/* What steps a-d and g do to "a group is open" when no group grows too long, as a map of {0, 1}: bit 0 = the outcome with
 * none open, bit 1 = with one open.  Maps compose (compose(f, g) = g after f), so "open before packet i" is a prefix scan. */
DABGPU_MOT_FN uint32_t open_map(const Packet &p, bool brk) {
    uint32_t m = 0;
    for (int o0 = 0; o0 < 2; o0++) {
        int o = o0;
        if (brk) o = 0;
        if (p.malformed) o = 0;
        else if (p.cmd) {}
        else if (p.first) o = !p.last;
        else if (o) o = !p.last;
        m |= uint32_t(o) << o0;
    }
    return m;
}
constexpr uint32_t OPEN_MAP_IDENTITY = 2;
DABGPU_MOT_FN uint32_t compose(uint32_t f, uint32_t g) { return ((g >> (f & 1)) & 1) | (((g >> ((f >> 1) & 1)) & 1) << 1); }
DABGPU_MOT_FN int apply(uint32_t f, int open) { return int((f >> open) & 1); }

/* Steps a-g of mode 0 for one packet, given what is true before it: `open` (a group is open) and `have` (its bytes).
 * Counts into c; -> what the packet does */
enum Action : int { ACT_NONE = 0, ACT_APPEND = 1, ACT_CLOSE = 3 };   /* CLOSE includes APPEND */
DABGPU_MOT_FN int step_packet(const Packet &p, bool brk, int &open, int &have, Counters &c) {
    if (brk) {
        c.continuity_breaks++;
        if (open) c.groups_unfinished++;
        open = 0;
    }
    if (p.malformed) {
        c.packets_malformed++;
        if (open) c.groups_unfinished++;
        open = 0;
        return ACT_NONE;
    }
    if (p.cmd) {
        c.packets_command++;
        return ACT_NONE;
    }
    if (p.first) {
        if (open) c.groups_unfinished++;
        open = 1;
        have = 0;
        c.groups_opened++;
    } else if (!open) {
        c.packets_orphan++;
        return ACT_NONE;
    }
    if (have + p.udl > GROUP_CAP) {
        c.groups_too_long++;
        open = 0;
        return ACT_NONE;
    }
    have += p.udl;
    c.group_bytes += p.udl;
    if (!p.last) return ACT_APPEND;
    open = 0;
    c.groups_closed++;
    return ACT_CLOSE;
}

/* ---- the group CRC in pieces ---------------------------------------------------------------------------------------
 * The register after bytes A then B is reg(A) x^(8 |B|) mod g + reg0(B), reg0 = the register from zero: (register, x^(8 n))
 * pairs of consecutive pieces join associatively, so the pieces of a group may be computed apart and scanned. */
DABGPU_MOT_FN uint32_t mulmod(uint32_t a, uint32_t b) {
    uint32_t r = 0;
    for (int i = 15; i >= 0; i--) {
        r <<= 1;
        if (r & 0x10000u) r ^= 0x11021u;
        if ((b >> i) & 1) r ^= a;
    }
    return r;
}
struct CrcPiece {
    uint32_t reg, shift;                  /* shift = x^(8 bytes) mod g */
};
DABGPU_MOT_FN CrcPiece crc_piece(const uint8_t *p, int n, uint32_t start) {
    CrcPiece q = {start, 1};
    for (int i = 0; i < n; i++) {
        q.reg = pad::crc16_step(q.reg, p[i]);
        q.shift = pad::crc16_step(q.shift, 0);
    }
    return q;
}
DABGPU_MOT_FN CrcPiece crc_join(const CrcPiece &a, const CrcPiece &b) {
    CrcPiece q = {mulmod(a.reg, b.shift) ^ b.reg, mulmod(a.shift, b.shift)};
    return q;
}

/* ---- a closed group ------------------------------------------------------------------------------------------------ */
enum Verdict : int { GROUP_ACCEPTED = 0, GROUP_MALFORMED = 1, GROUP_CRC_FAILED = 2 };
/* head: the group's first min(n, HEAD_BYTES) bytes; reg: the register over all n bytes.  Fills r but offset and DG_REPEAT */
DABGPU_MOT_FN int close_group(const uint8_t *head, int n, uint32_t reg, int cif, int slot, Record &r) {
    if (n < 4) return GROUP_MALFORMED;
    const int b0 = head[0];
    if ((b0 & 0x40) && reg != pad::CRC_GOOD_RESIDUE) return GROUP_CRC_FAILED;
    const int end = (b0 & 0x40) ? n - 2 : n;
    int o = 2, flags = (b0 & 0x40) ? DG_CRC : 0;
    r.extension = 0;
    r.segment = r.transport_id = -1;
    if (b0 & 0x80) {
        if (o + 2 > end) return GROUP_MALFORMED;
        r.extension = uint16_t((head[o] << 8) | head[o + 1]);
        flags |= DG_EXTENSION;
        o += 2;
    }
    if (b0 & 0x20) {
        if (o + 2 > end) return GROUP_MALFORMED;
        r.segment = (head[o] << 8) | head[o + 1];
        flags |= DG_SEGMENT;
        o += 2;
    }
    if (b0 & 0x10) {
        if (o + 1 > end) return GROUP_MALFORMED;
        const int ua = head[o], li = ua & 0x0F, tid = (ua >> 4) & 1;
        o += 1;
        if ((tid && li < 2) || o + li > end) return GROUP_MALFORMED;
        flags |= DG_USER_ACCESS;
        if (tid) {
            r.transport_id = (head[o] << 8) | head[o + 1];
            flags |= DG_TRANSPORT_ID;
        }
        flags |= (li - 2 * tid) << 8;
        o += li;
    }
    r.offset = 0;
    r.length = n;
    r.cif = cif;
    r.slot = uint8_t(slot);
    r.type = uint8_t(b0 & 0x0F);
    r.continuity = uint8_t(head[1] >> 4);
    r.repetition = uint8_t(head[1] & 0x0F);
    r.flags = uint16_t(flags);
    r.data_offset = uint16_t(o);
    r.data_length = uint16_t(end - o);
    return GROUP_ACCEPTED;
}
DABGPU_MOT_FN void count_verdict(int verdict, const Record &r, Counters &c) {
    /* (sums, not branches: the compiler would make an indexed counter of three branches, and that is scratch on the device) */
    c.groups_malformed += verdict == GROUP_MALFORMED;
    c.groups_crc_failed += verdict == GROUP_CRC_FAILED;
    c.groups_no_crc += verdict == GROUP_ACCEPTED && !(r.flags & DG_CRC);
}

/* the running numbers of a call's emission: groups (or breaks) so far, and the offset of the next (mode 1: `at`) */
struct Emission {
    uint32_t count, offset;
};
DABGPU_MOT_FN uint32_t round16(uint32_t n) { return (n + 15u) & ~15u; }
DABGPU_MOT_FN uint32_t offset_add(uint32_t a, uint32_t b) {
    const uint64_t s = uint64_t(a) + b;
    return s > OFFSET_SAT ? OFFSET_SAT : uint32_t(s);
}
DABGPU_MOT_FN bool has_room(uint32_t index, uint32_t offset, int length, int max_groups, int bytes_capacity) {
    return index < uint32_t(max_groups) && uint64_t(offset) + uint32_t(length) <= uint64_t(uint32_t(bytes_capacity));
}

/* ---- the serial walk: the host twin ----------------------------------------------------------------------------------- */
struct Call {
    int32_t mode, keep_repeats, bytes_capacity, max_groups;
    uint8_t *bytes;
    Record *groups;
};

/* one entry of a call on memory the caller can address; st_out: a whole record, != st_in */
inline void walk_frames(const State *st_in, State *st_out, Counters &c, const Call &call, const uint8_t *in, uint64_t in_stride,
                        int n_cifs, int S, int address, int fec) {
    Head h = read_head(st_in, call.mode);
    uint8_t *group = st_out->group;
    for (int i = 0; i < h.have; i++) group[i] = st_in->group[i];
    Emission em = {0, 0};
    pkt::Counters scan = {};
    for (int k = 0; k < n_cifs; k++) {
        const uint8_t *frame = in + uint64_t(k) * in_stride;
        pkt::scan_frame(scan, frame, S, address, fec, [&](int pos, int L) {
            const uint8_t *p = frame + pkt::SLOT_BYTES * pos;
            const Packet q = packet_fields(p[0], p[2], L);
            const bool brk = is_break(h.seen, h.prev, q.ci);
            h.seen = 1;
            h.prev = uint8_t(q.ci);
            if (call.mode) {
                if (brk) {
                    c.continuity_breaks++;
                    if (em.count < uint32_t(call.max_groups)) {
                        Record r = {};
                        r.offset = int32_t(em.offset);
                        r.cif = k;
                        r.slot = uint8_t(pos);
                        r.flags = DG_BREAK;
                        call.groups[em.count] = r;
                        c.groups_emitted++;
                    } else {
                        c.groups_no_room++;
                    }
                    em.count++;
                }
                if (q.malformed) c.packets_malformed++;
                else if (q.cmd) c.packets_command++;
                else {
                    if (uint64_t(em.offset) + uint32_t(q.udl) <= uint64_t(uint32_t(call.bytes_capacity))) {
                        for (int i = 0; i < q.udl; i++) call.bytes[em.offset + i] = p[3 + i];
                        c.bytes_emitted += q.udl;
                    } else {
                        c.bytes_no_room += q.udl;
                    }
                    em.offset = offset_add(em.offset, uint32_t(q.udl));
                }
                return;
            }
            int open = h.open, have = h.have;
            const int at = q.first ? 0 : have;
            const int act = step_packet(q, brk, open, have, c);
            if (act & ACT_APPEND) {
                for (int i = 0; i < q.udl; i++) group[at + i] = p[3 + i];
                const CrcPiece piece = crc_piece(p + 3, q.udl, q.first ? 0xFFFFu : 0u);
                h.crc = q.first ? piece.reg : crc_join(CrcPiece{h.crc, 1}, piece).reg;
            }
            h.open = uint8_t(open);
            h.have = open ? have : 0;
            if (act != ACT_CLOSE) return;
            Record r;
            const int verdict = close_group(group, have, h.crc, k, pos, r);
            count_verdict(verdict, r, c);
            if (verdict != GROUP_ACCEPTED) return;
            const bool repeat = ((h.type_mask >> r.type) & 1) && last_ci_of(h, r.type) == r.continuity;
            set_last_ci(h, r.type, r.continuity);
            if (repeat) {
                c.groups_repeated++;
                if (!call.keep_repeats) return;
                r.flags |= DG_REPEAT;
            }
            if (has_room(em.count, em.offset, have, call.max_groups, call.bytes_capacity)) {
                r.offset = int32_t(em.offset);
                call.groups[em.count] = r;
                for (int i = 0; i < have; i++) call.bytes[em.offset + i] = group[i];
                c.groups_emitted++;
                c.bytes_emitted += have;
            } else {
                c.groups_no_room++;
            }
            em.count++;
            em.offset = offset_add(em.offset, round16(uint32_t(have)));
        });
    }
    c.cifs = scan.cifs;
    c.slots = scan.slots;
    c.slots_bad = scan.slots_bad;
    c.packets_fec = scan.packets_fec;
    c.packets_padding = scan.packets_padding;
    c.packets_other = scan.packets_other;
    c.packets_followed = scan.packets_followed;
    write_head(st_out, h);
    for (int i = h.open ? h.have : 0; i < GROUP_CAP; i++) group[i] = 0;
}

}  /* namespace dabgpu_groups */
#endif
