/* dabgpu_packet_walk.h -- the slideshow objects (MOT, header mode) of a packet-mode service component, from the logical
 * frames of its sub-channel.
 *
 * One implementation of the contract below (EN 300 401 clauses 5.3.2 and 5.3.3): the kernels behind
 * dabgpu_packet_slides_dev, the host twin dabgpu_packet_slides_host and the host mirror's Basic_Data_Packet_Channel all run
 * this code.  Plain C++17, header-only, no allocation, no table in memory; __host__ __device__ under hipcc.  A data group,
 * once its packets are put together, is what dabgpu_mot_walk.h's Sink::close_group() takes: from there on ("Closing a
 * group", "Assembly", completion, the slot format) this is the slideshow call's code, unchanged.
 *
 * THE CONTRACT of one entry (a sub-channel and one packet address) in one call, every ambiguity decided.
 *
 * A logical frame of a sub-channel with bit rate R kbit/s has 3 R bytes: S = R / 8 slots of 24 bytes.  Packets do not
 * straddle frames.  Scan of one frame: pos = 0; while pos < S, with h0 h1 h2 the bytes at 24 pos:
 *   L = (h0 >> 6) + 1 slots; addr = ((h0 & 3) << 8) | h1.  First match wins:
 *   1. the entry's fec is non-zero, addr == 1022 and L == 1: packets_fec++, pos += 1 (the 24 bytes of an FEC packet carry no
 *      packet CRC; they are not checked and not corrected)
 *   2. pos + L > S: slots_bad++, pos += 1
 *   3. the FIB's CRC (x^16 + x^12 + x^5 + 1, register all ones, complemented, big-endian) over the first 24 L - 2 bytes does
 *      not equal the last two -- the residue over all 24 L bytes is not dabgpu_pad::CRC_GOOD_RESIDUE: slots_bad++, pos += 1
 *      (the scan resynchronises at the next slot: a length that could not be checked is not trusted)
 *   4. else a good packet, pos += L: addr == 0: packets_padding++; addr != the entry's address: packets_other++; else
 *      packets_followed++ and the packet is followed.
 *
 * Followed packets, in frame and position order; ci = (h0 >> 4) & 3, first = (h0 >> 3) & 1, last = (h0 >> 2) & 1,
 * cmd = h2 >> 7, udl = h2 & 0x7F.  "Dropped" below: an open group is forgotten and groups_unfinished++; nothing when none
 * is open.
 *   a. a followed packet has been seen before (in this call or an earlier one) and ci != (prev + 1) & 3:
 *      continuity_breaks++, dropped.  Then prev = ci, in every case.
 *   b. udl > 24 L - 5: packets_malformed++, dropped; next packet.
 *   c. cmd: packets_command++; next packet (an open group stays as it is).
 *   d. first: dropped, then a new group opens empty, groups_opened++.  Not first and no group open: packets_orphan++; next
 *      packet.
 *   e. have + udl > 16384: groups_too_long++, the group is forgotten (not counted as unfinished); next packet.
 *   f. the udl bytes from offset 3 are appended (a copy order: forward, from the frame into the arena's group buffer);
 *      group_bytes += udl.
 *   g. last: have < 4: groups_malformed++ (of the embedded record), the group is forgotten.  Else the group closes with
 *      need = have by "Closing a group" and "Assembly" of dabgpu_mot_slides_dev, word for word (a clear CRC flag is
 *      groups_crc_failed).  A completed object's record has superframe = the index of the logical frame in this call and
 *      au = the slot position of the closing packet.
 *
 * Counters: cifs = n_cifs, slots = n_cifs S; of the embedded dabgpu_mot_result the fields only PAD gives (aus .. fields_ignored,
 * lengths_*, groups_no_length, xpad_bytes) stay 0.
 *
 * The state record: the slideshow state (assembly, last object, head of the open group) plus seen, prev and the open group's
 * length and CRC register.  All zero = a fresh start; a record this code did not write for an arena of this size is a fresh
 * start.  It goes with the arena from call to call, so a group or an object may span any number of calls; no frame is
 * carried.
 */
#ifndef DABGPU_PACKET_WALK_H
#define DABGPU_PACKET_WALK_H

#include "dabgpu_mot_walk.h"

namespace dabgpu_packet {

namespace pad = dabgpu_pad;
namespace mot = dabgpu_mot;

constexpr int SLOT_BYTES = 24, MAX_SLOTS = 64, MAX_PACKET_BYTES = 96;
constexpr int FEC_ADDRESS = 1022;
constexpr int MAX_N_CIFS = 1 << 24;       /* slots = n_cifs * S stays an int32 */
/* one more order kind than dabgpu_mot::OrderKind: arena[dst + i] = packet[src + i], i < len (the packet's useful bytes) */
constexpr int32_t ORDER_PACKET = 5;

struct Counters {                         /* == dabgpu_packet_result */
    int32_t cifs, slots, slots_bad;
    int32_t packets_fec, packets_padding, packets_other, packets_followed;
    int32_t continuity_breaks, packets_malformed, packets_command, packets_orphan;
    int32_t groups_opened, groups_unfinished, groups_too_long;
    int32_t group_bytes;                  /* useful bytes the orders of this call moved: packet -> group */
    int32_t reserved;
    mot::Counters mot;
};

struct alignas(16) State {                /* all zero = a fresh start */
    mot::State mot;                       /* its X-PAD fields (cont_type .. group_crc) stay zero between packets */
    uint8_t seen, prev;                   /* a followed packet has been seen; its continuity index */
    uint8_t open, pad;
    uint16_t have;                        /* bytes of the open group */
    uint16_t crc;                         /* the CRC register over them, complemented */
    uint8_t reserved[8];
};
static_assert(sizeof(Counters) == 192 && sizeof(State) == 176, "records of the ABI");

DABGPU_MOT_FN bool bitrate_ok(int kbps) { return kbps >= 8 && kbps <= 512 && kbps % 8 == 0; }

DABGPU_MOT_FN void forget_group(State &st) {
    st.open = 0;
    st.have = st.crc = 0;
}
DABGPU_MOT_FN void drop_open(State &st, Counters &c) {
    if (st.open) c.groups_unfinished++;
    forget_group(st);
}

/* the fields of this record, without the assembly's part */
DABGPU_MOT_FN bool own_ok(const State &st, int32_t body_capacity) {
    const mot::State &m = st.mot;
    bool ok = st.seen <= 1 && st.prev <= 3 && st.open <= 1 && st.pad == 0 && st.have <= mot::GROUP_CAP &&
              (st.open || (st.have == 0 && st.crc == 0)) && (st.seen || (st.prev == 0 && !st.open));
    for (int i = 0; i < 8; i++) ok = ok && st.reserved[i] == 0;
    return ok && m.cont_type == 0 && m.last_len == 0 && m.group_open == 0 && m.armed == 0 && m.next_length == 0 &&
           m.body_capacity == body_capacity;
}
DABGPU_MOT_FN void sanitize(State &st, int32_t body_capacity) {
    if (!own_ok(st, body_capacity)) {
        uint8_t *p = reinterpret_cast<uint8_t *>(&st);
        for (unsigned i = 0; i < sizeof(State); i++) p[i] = 0;
        st.mot.body_capacity = body_capacity;
    }
    /* the assembly's part is judged by its own rules; whatever it leaves, `have` bounds every order of the open group */
    mot::sanitize(st.mot, body_capacity);
}

/* What the slot at `pos` of a frame of S slots is, taken as the start of a packet: kind | L << 2 | addr << 5 */
enum SlotKind : uint32_t { SLOT_BAD = 0, SLOT_FEC = 1, SLOT_GOOD = 2 };
DABGPU_MOT_FN uint32_t slot_verdict(const uint8_t *frame, int S, int pos, int fec) {
    const uint8_t *p = frame + SLOT_BYTES * pos;
    const uint32_t L = (p[0] >> 6) + 1u, addr = ((p[0] & 3u) << 8) | p[1];
    const uint32_t fields = (L << 2) | (addr << 5);
    if (fec && addr == uint32_t(FEC_ADDRESS) && L == 1) return SLOT_FEC | fields;
    if (pos + int(L) > S) return SLOT_BAD | fields;
    uint32_t crc = 0xFFFF;
    for (int i = 0; i < SLOT_BYTES * int(L); i++) crc = pad::crc16_step(crc, p[i]);
    return (crc == pad::CRC_GOOD_RESIDUE ? SLOT_GOOD : SLOT_BAD) | fields;
}
DABGPU_MOT_FN int verdict_kind(uint32_t v) { return int(v & 3); }
DABGPU_MOT_FN int verdict_slots(uint32_t v) { return int((v >> 2) & 7); }
DABGPU_MOT_FN int verdict_address(uint32_t v) { return int(v >> 5); }

struct FrameTally {
    int32_t fec, bad, padding, other, followed;
};
/* The chain of one frame: verdict(pos) is slot_verdict of that slot (computed here, or read back from where a wave left
 * it); followed(pos, L) is called for every followed packet in position order. */
template <class Verdict, class Followed>
DABGPU_MOT_FN void resolve_chain(int S, int address, FrameTally &t, Verdict verdict, Followed followed) {
    for (int pos = 0; pos < S;) {
        const uint32_t v = verdict(pos);
        const int kind = verdict_kind(v), L = verdict_slots(v), addr = verdict_address(v);
        if (kind == SLOT_FEC) {
            t.fec++;
            pos += 1;
        } else if (kind == SLOT_BAD) {
            t.bad++;
            pos += 1;
        } else {
            if (addr == 0) {
                t.padding++;
            } else if (addr != address) {
                t.other++;
            } else {
                t.followed++;
                followed(pos, L);
            }
            pos += L;
        }
    }
}

/* how many bytes of a followed packet steps a .. g read: the header and the useful bytes (none of a malformed one) */
DABGPU_MOT_FN int packet_read_bytes(int L, int h2) {
    const int udl = h2 & 0x7F;
    return udl > SLOT_BYTES * L - 5 ? 3 : 3 + udl;
}

/* One followed packet of L slots: steps a .. f, and of g what comes before the group closes.  pkt: its first
 * packet_read_bytes() bytes.  Leaves the packet's order in `ord` (ORDER_PACKET's src counts from pkt; at most one).  -> true
 * when a group is ready to close: its length is in st.mot.group_need, its CRC register in st.mot.group_crc, its first bytes in
 * st.mot.head, and the caller's sink closes it (its orders follow this one in `ord`). */
DABGPU_MOT_FN bool take_packet(State &st, Counters &c, mot::Orders &ord, const uint8_t *pkt, int L) {
    ord.n = 0;
    const int h0 = pkt[0], h2 = pkt[2];
    const int ci = (h0 >> 4) & 3, first = (h0 >> 3) & 1, last = (h0 >> 2) & 1, cmd = h2 >> 7, udl = h2 & 0x7F;
    if (st.seen && ci != ((st.prev + 1) & 3)) {
        c.continuity_breaks++;
        drop_open(st, c);
    }
    st.seen = 1;
    st.prev = uint8_t(ci);
    if (udl > SLOT_BYTES * L - 5) {
        c.packets_malformed++;
        drop_open(st, c);
        return false;
    }
    if (cmd) {
        c.packets_command++;
        return false;
    }
    if (first) {
        drop_open(st, c);
        st.open = 1;
        c.groups_opened++;
    } else if (!st.open) {
        c.packets_orphan++;
        return false;
    }
    const int have = st.have;
    if (have + udl > mot::GROUP_CAP) {
        c.groups_too_long++;
        forget_group(st);
        return false;
    }
    uint32_t crc = st.crc ^ 0xFFFFu;
    for (int i = 0; i < udl; i++) {
        const uint8_t v = pkt[3 + i];
        crc = pad::crc16_step(crc, v);
        if (have + i < mot::HEAD_BYTES) st.mot.head[have + i] = v;
    }
    mot::push_order(ord, ORDER_PACKET, 3, uint32_t(have), udl);
    c.group_bytes += udl;
    st.have = uint16_t(have + udl);
    st.crc = uint16_t(crc ^ 0xFFFFu);
    if (!last) return false;
    const int need = st.have;
    const uint16_t reg = st.crc;
    forget_group(st);
    if (need < 4) {
        c.mot.groups_malformed++;
        return false;
    }
    st.mot.group_need = uint16_t(need);
    st.mot.group_crc = reg;
    return true;
}

/* One followed packet of L slots: steps a .. g, the closed group into the slideshow call's sink */
DABGPU_MOT_FN void follow_packet(State &st, Counters &c, mot::Orders &ord, const mot::Call &call, const uint8_t *pkt, int L) {
    if (!take_packet(st, c, ord, pkt, L)) return;
    mot::Sink k{st.mot, c.mot, ord, call, pkt};
    k.close_group();
}

/* One order on memory the caller can address: the host's executor (the kernel has its own, a wave wide) */
inline void execute_order(const mot::Order &o, const mot::Orders &ord, const uint8_t *pkt, uint8_t *arena, uint8_t *slides) {
    if (o.kind == ORDER_PACKET)
        for (int i = 0; i < o.len; i++) arena[o.dst + i] = pkt[o.src + i];
    else
        mot::execute(o, ord, pkt, arena, slides);
}

/* The scan of one logical frame and its counters: followed(pos, L) takes every followed packet in position order */
template <class Followed>
inline void scan_frame(Counters &c, const uint8_t *frame, int S, int address, int fec, Followed followed) {
    FrameTally t = {};
    resolve_chain(S, address, t, [&](int pos) { return slot_verdict(frame, S, pos, fec); }, followed);
    c.cifs++;
    c.slots += S;
    c.packets_fec += t.fec;
    c.slots_bad += t.bad;
    c.packets_padding += t.padding;
    c.packets_other += t.other;
    c.packets_followed += t.followed;
}

/* One logical frame (index k of the call) of one entry, on memory the caller can read and write */
inline void walk_frame(State &st, Counters &c, const mot::Call &entry, const uint8_t *frame, int k, int S, int address, int fec,
                       uint8_t *arena, uint8_t *slides) {
    mot::Orders ord;
    mot::Call call = entry;
    call.superframe = k;
    scan_frame(c, frame, S, address, fec, [&](int pos, int L) {
        const uint8_t *pkt = frame + SLOT_BYTES * pos;
        call.au = pos;
        follow_packet(st, c, ord, call, pkt, L);
        for (int i = 0; i < ord.n; i++) execute_order(ord.o[i], ord, pkt, arena, slides);
    });
}

/* One entry of a call: the twin of the two kernels */
inline void walk_frames(State &st, Counters &c, const mot::Call &entry, const uint8_t *in, uint64_t in_stride, int n_cifs, int S,
                        int address, int fec, uint8_t *arena, uint8_t *slides) {
    for (int k = 0; k < n_cifs; k++) walk_frame(st, c, entry, in + uint64_t(k) * in_stride, k, S, address, fec, arena, slides);
}

}  /* namespace dabgpu_packet */
#endif
