/* dabgpu_mot_carousel.h -- the objects of a MOT directory carousel (EN 301 234 clause 7.2) of a packet-mode service
 * component, from the logical frames of its sub-channel.
 *
 * One implementation of the contract below: the kernel behind dabgpu_packet_carousel_dev, the host twin
 * dabgpu_packet_carousel_host, the directory parser behind dabgpu_mot_directory_parse and the host mirror's
 * Basic_Data_Packet_Channel all run this code.  Plain C++17, header-only, no allocation, no table in memory;
 * __host__ __device__ under hipcc.  The scan of a frame and the followed packets are dabgpu_packet_walk.h's functions
 * (slot_verdict, resolve_chain, take_packet); the parse of a closed group and the placement of a segment are
 * dabgpu_mot_walk.h's (group_segment, place): the same functions the slides calls run, not copies.
 *
 * The control moves no payload byte: it updates state and counters and returns copy orders, which the caller executes in
 * their order, each complete before the next begins (a loop on the host, the whole wave in the kernel).  Control reads the
 * bytes of the packet and nothing of the arena, with one exception that is a phase of its own: the directory check, behind
 * the orders of the packet that completed the directory, reads the directory's bytes in the arena and leaves the index in
 * the state record, so that every later step is arena-free again.  Per followed packet:
 *   1. take_packet + close_group -> orders, executed
 *   2. when the directory became full: check_directory_phase -> orders, executed; if it became current, clear_stale
 *   3. emit_attempt -> orders, executed
 *
 * THE CONTRACT of one entry (a sub-channel and one packet address) in one call, every ambiguity decided.
 *
 * Frames, packets, groups.  The scan of a frame (steps 1-4) and steps a-g of the followed packets are those of
 * dabgpu_packet_walk.h, word for word, with the same counters in the head of the result (a dabgpu_packet_result; of its
 * embedded dabgpu_mot_result the fields groups_ok .. groups_repeated, segments_*, objects_completed, objects_mismatched,
 * objects_too_large and object_bytes count here, the others stay 0).  A closed group goes through "Closing a group" of
 * dabgpu_mot_slides_dev, word for word, up to the type test, which here is:
 *   type 4: a body segment; type 6: a directory segment; type 3: groups_header_mode++; type 7:
 *   groups_compressed_directory++; any other: groups_ignored_type++.
 * Types 4 and 6 then pass the rest of "Closing a group" (segment flag .. z != end - o; groups_ok++).
 *
 * Placing a segment into the directory or into a body assembly follows "Assembly" of dabgpu_mot_slides_dev from
 * "n >= ..." on, word for word: at most 256 segments for both kinds, at most directory_capacity bytes for the directory and
 * object_capacity for a body.  A segment that is present is not overwritten, so a part may become full by a repetition:
 * segment 0 placed as a non-last segment of S bytes and sent again as the last segment with z <= S bytes makes a part of one
 * segment.  Its length is then what the last-segment group said, z, and its bytes are the first z of those placed first.
 *
 * Directory: one buffer.  For a type-6 segment of transport id t, first match wins:
 *   t equals the current (complete, valid) directory's id -> groups_repeated++, dropped
 *   there is a current directory, or no directory under assembly, or t differs from the id under assembly: the current
 *     directory and its index are forgotten, the delivered marks are cleared, the directory assembly is emptied and takes
 *     t.  Body assemblies are kept.
 *   the assembly is marked too large -> dropped (until the id changes)
 *   else the segment is placed.
 * Directory check: when segments 0 .. last are present, behind the copy that places the last one, the directory of D bytes
 * is checked.  First match wins:
 *   1. D < 13, or the low 30 bits of bytes 0-3 (big-endian) != D         -> directories_mismatched++
 *   2. byte 0 bit 7 (compression) set                                   -> directories_mismatched++
 *   3. N = bytes 4, 5; period = bytes 6-8; segment size = 13 bits of bytes 9, 10; X = bytes 11, 12; o = 13 + X
 *   4. o > D                                                             -> directories_mismatched++
 *   5. N > 256                                                           -> directories_too_large++
 *   6. for i < N: o + 9 > D -> mismatched.  tid = 2 bytes at o; the 7 bytes behind it are the header core: body_size(28)
 *      header_size(13) content_type(6) subtype(9).  header_size < 7 or o + 2 + header_size > D -> mismatched.  Index entry
 *      i = (tid, o + 2, header_size, body_size, type, subtype); o += 2 + header_size.
 *   7. o != D                                                            -> directories_mismatched++
 * On a failure the assembly is emptied and there is no current directory.  Else directories_completed++, it is current (the
 * assembly is emptied, the bytes stay where they are), its D bytes go to d_directory (object_bytes += D), and every body
 * assembly whose id is not in the index is emptied, objects_stale++ each.  A transport id listed twice means its lowest i.
 * directory_id, directory_bytes, directory_objects, directory_period and directory_segment_size of the result describe the
 * directory that is current at the end of the call (also one merely carried in from the state); without one directory_id
 * is -1 and the others 0.
 *
 * Bodies.  A type-4 segment of id t:
 *   1. with a current directory: t not listed -> groups_unlisted++, dropped; t listed and delivered -> groups_repeated++,
 *      dropped.  Without one every body is taken (bodies may arrive before their directory).
 *   2. it goes to the assembly that holds t, else to the lowest-numbered empty one, else the assembly whose stamp is oldest
 *      (lowest number on a tie) is emptied, objects_evicted++, and takes t.  The stamp: a 32-bit count of placed body
 *      segments is kept in the state; an assembly that takes an id is stamped with the count, and with the count after
 *      each of its placed segments; age = (count - stamp) mod 2^32.
 *   3. the assembly is marked too large -> dropped; else the segment is placed (object_bytes += z).
 *
 * Emission: one attempt behind every followed packet, after its orders (and the directory check's) have been executed.
 * Without a current directory nothing.  Else the lowest-numbered assembly that is full (segments 0 .. last) and whose id the
 * directory lists, entry e.  First match wins:
 *   assembled bytes != e's body_size             -> objects_mismatched++, emptied, not marked delivered
 *   32 + header_size + bytes > object_stride     -> objects_dropped++, marked delivered, emptied (object_stride as the entry
 *                                                   gives it, also with max_objects == 0)
 *   objects_written == max_objects               -> objects_deferred++, once per call per assembly; it stays as it is
 *   else slot objects_written of THIS call receives a dabgpu_mot_carousel_object record -- transport_id, content_type,
 *     content_subtype, header_bytes, body_bytes, frame = index of the logical frame in this call, slot = slot position of
 *     the packet this attempt follows, directory_id --, then e's header bytes from the directory, then the body;
 *     objects_written++, objects_completed++, object_bytes += header + body, marked delivered, emptied.
 * A call without followed packets emits nothing.
 *
 * State and arena.  The state record has a fixed size: the packet state, the directory part, 32 body parts, the index of 256
 * entries, the delivered bits, the counts.  All zero = a fresh start; a record this code did not write for exactly these
 * directory_capacity, assemblies and object_capacity is one.  The arena: group buffer [0, 16384) | directory
 * [16384, + directory_capacity rounded up to 16) | K bodies of object_capacity rounded up to 16 each.  It belongs to the
 * state; a group, a directory or an object may span any number of calls, cut anywhere.
 */
#ifndef DABGPU_MOT_CAROUSEL_H
#define DABGPU_MOT_CAROUSEL_H

#include "dabgpu_packet_walk.h"

namespace dabgpu_carousel {

namespace pad = dabgpu_pad;
namespace mot = dabgpu_mot;
namespace pkt = dabgpu_packet;

constexpr int MAX_ASSEMBLIES = 32, INDEX_MAX = 256, SEGMENTS = 256;
constexpr int DIRECTORY_CAP_MIN = 16, DIRECTORY_CAP_MAX = 1 << 20;
constexpr int DIRECTORY_OFF = mot::GROUP_CAP;
constexpr int DIRECTORY_FIXED = 13, ENTRY_FIXED = 9, CORE_BYTES = 7;
/* two more order kinds than dabgpu_packet's; mot::ORDER_RECORD writes record[src] to objects[dst ..] here */
constexpr int32_t ORDER_DIRECTORY = 6;    /* directory[dst + i] = arena[src + i]: the checked directory to d_directory */
constexpr int32_t ORDER_OBJECT = 7;       /* objects[dst + i] = arena[src + i]: header or body of an object into its slot */

struct Counters {                         /* == dabgpu_packet_carousel_result */
    pkt::Counters head;
    int32_t groups_header_mode, groups_compressed_directory, groups_unlisted;
    int32_t directories_completed, directories_mismatched, directories_too_large;
    int32_t objects_stale, objects_evicted, objects_dropped, objects_deferred, objects_written;
    int32_t directory_id, directory_bytes, directory_objects, directory_period, directory_segment_size;
};

struct Body {                             /* one body under assembly */
    uint16_t tid;
    uint8_t valid, too_large;
    uint32_t stamp;
    int32_t pad[2];
    mot::Part part;
};

struct IndexEntry {                       /* one object the current directory lists */
    uint32_t offset;                      /* of its header in the directory */
    uint32_t body_size;
    uint16_t tid, header_size, subtype;
    uint8_t type, pad;
};

struct alignas(16) State {                /* all zero = a fresh start */
    pkt::State pkt;                       /* its mot part serves the open group (head, group_need, group_crc) alone */
    int32_t directory_capacity, assemblies, object_capacity;
    uint32_t placed;                      /* body segments placed so far, mod 2^32 */
    uint16_t dir_tid, cur_tid;            /* of the directory under assembly; of the current one */
    uint8_t dir_valid, dir_too_large, cur_valid;
    uint8_t check_pending;                /* the directory became full in this packet (never set between packets) */
    int32_t cur_bytes, cur_objects, cur_period, cur_segment_size;
    int32_t pad;
    mot::Part dir;
    Body body[MAX_ASSEMBLIES];
    uint32_t delivered[INDEX_MAX / 32];   /* bit i = the object of index entry i has been delivered (or dropped) */
    IndexEntry index[INDEX_MAX];
};

struct Call {                             /* what the caller's entry says, and where the walk is */
    int32_t directory_capacity, assemblies, object_capacity, max_objects;
    uint32_t object_stride;
    int32_t frame, slot;
    uint32_t deferred;                    /* bit k = assembly k has been counted in objects_deferred in this call */
};

static_assert(sizeof(Counters) == 256 && sizeof(Body) == 64 && sizeof(IndexEntry) == 16 && sizeof(State) == 6448 &&
                  sizeof(State) % 16 == 0,
              "records of the ABI");

DABGPU_MOT_FN uint32_t round16(uint32_t n) { return (n + 15u) & ~15u; }
DABGPU_MOT_FN uint32_t body_off(const Call &call, int k) {
    return uint32_t(DIRECTORY_OFF) + round16(uint32_t(call.directory_capacity)) + uint32_t(k) * round16(uint32_t(call.object_capacity));
}
DABGPU_MOT_FN bool sizes_ok(int64_t directory_capacity, int64_t assemblies, int64_t object_capacity) {
    return directory_capacity >= DIRECTORY_CAP_MIN && directory_capacity <= DIRECTORY_CAP_MAX && assemblies >= 1 &&
           assemblies <= MAX_ASSEMBLIES && object_capacity >= 0 && object_capacity <= mot::BODY_CAP_MAX;
}
/* (sizes_ok: at most 16 KiB + 1 MiB + 32 * 2 MiB, every offset an int32) */
DABGPU_MOT_FN uint64_t arena_bytes(int directory_capacity, int assemblies, int object_capacity) {
    return uint64_t(DIRECTORY_OFF) + round16(uint32_t(directory_capacity)) + uint64_t(assemblies) * round16(uint32_t(object_capacity));
}

DABGPU_MOT_FN void empty_part(mot::Part &q) {
    q.seg_size = q.last = q.last_len = q.pad = 0;
    for (int w = 0; w < SEGMENTS / 32; w++) q.have[w] = 0;
}
DABGPU_MOT_FN void empty_body(Body &b) {
    b.tid = 0;
    b.valid = b.too_large = 0;
    b.stamp = 0;
    b.pad[0] = b.pad[1] = 0;
    empty_part(b.part);
}
DABGPU_MOT_FN void empty_directory_assembly(State &st) {
    st.dir_valid = st.dir_too_large = st.check_pending = 0;
    st.dir_tid = 0;
    empty_part(st.dir);
}
DABGPU_MOT_FN void forget_current(State &st) {
    st.cur_valid = 0;
    st.cur_tid = 0;
    st.cur_bytes = st.cur_objects = st.cur_period = st.cur_segment_size = 0;
    for (int w = 0; w < INDEX_MAX / 32; w++) st.delivered[w] = 0;
}
/* the lowest index entry of the current directory with this id, -1 = not listed (the serial definition; a wave may search
 * with a lane per entry and take the lowest set bit of the ballot) */
DABGPU_MOT_FN int find_listed(const State &st, int tid) {
    for (int i = 0; i < st.cur_objects; i++)
        if (st.index[i].tid == tid) return i;
    return -1;
}

/* what this code can have written for these sizes, and nothing that would make an order leave the arena, d_directory or a
 * slot; else a fresh start */
DABGPU_MOT_FN void sanitize(State &st, int32_t directory_capacity, int32_t assemblies, int32_t object_capacity) {
    bool ok = st.directory_capacity == directory_capacity && st.assemblies == assemblies && st.object_capacity == object_capacity &&
              pkt::own_ok(st.pkt, object_capacity) && mot::state_ok(st.pkt.mot, object_capacity) && st.dir_valid <= 1 &&
              st.dir_too_large <= 1 && st.cur_valid <= 1 && st.check_pending == 0 && st.pad == 0 && !(st.cur_valid && st.dir_valid) &&
              mot::part_ok(st.dir, 1, directory_capacity) && !mot::part_full(st.dir);
    if (ok && st.cur_valid) {
        ok = st.cur_bytes >= DIRECTORY_FIXED && st.cur_bytes <= directory_capacity && st.cur_objects >= 0 && st.cur_objects <= INDEX_MAX;
        for (int i = 0; ok && i < st.cur_objects; i++) {
            const IndexEntry &e = st.index[i];
            ok = e.header_size >= CORE_BYTES && e.header_size <= mot::SEGMENT_MAX && e.offset >= uint32_t(DIRECTORY_FIXED + 2) &&
                 e.offset + e.header_size <= uint32_t(st.cur_bytes);
        }
    }
    for (int k = 0; ok && k < MAX_ASSEMBLIES; k++) {
        const Body &b = st.body[k];
        ok = b.valid <= 1 && b.too_large <= 1 && b.pad[0] == 0 && b.pad[1] == 0 && mot::part_ok(b.part, 1, object_capacity) &&
             (k < assemblies || !b.valid);
    }
    if (ok) return;
    uint8_t *p = reinterpret_cast<uint8_t *>(&st);
    for (unsigned i = 0; i < sizeof(State); i++) p[i] = 0;
    st.directory_capacity = directory_capacity;
    st.assemblies = assemblies;
    st.object_capacity = object_capacity;
    st.pkt.mot.body_capacity = object_capacity;
}

/* ---------------------------------------------------------------------------------------------------------------------
 * The directory check, rules 1-7 over the D bytes at d.  entry(i, tid, offset, header_size, body_size, type, subtype) takes
 * the index entries as the chain finds them (entries given before a later rule fails are void). */
struct DirectoryInfo {                    /* == dabgpu_mot_directory */
    int32_t objects, period, segment_size, extension_offset, extension_bytes, directory_bytes;
    int32_t reserved[2];
};
enum CheckResult : int { CHECK_OK = 0, CHECK_MISMATCHED = 1, CHECK_TOO_LARGE = 2 };
template <class Entry> DABGPU_MOT_FN int check_directory(const uint8_t *d, int D, DirectoryInfo &info, Entry entry) {
    if (D < DIRECTORY_FIXED) return CHECK_MISMATCHED;
    const uint32_t size = ((uint32_t(d[0]) & 0x3F) << 24) | (uint32_t(d[1]) << 16) | (uint32_t(d[2]) << 8) | d[3];
    if (size != uint32_t(D)) return CHECK_MISMATCHED;
    if (d[0] & 0x80) return CHECK_MISMATCHED;
    const int N = (d[4] << 8) | d[5], X = (d[11] << 8) | d[12];
    info.objects = N;
    info.period = (d[6] << 16) | (d[7] << 8) | d[8];
    info.segment_size = ((d[9] & 0x1F) << 8) | d[10];
    info.extension_offset = DIRECTORY_FIXED;
    info.extension_bytes = X;
    info.directory_bytes = D;
    info.reserved[0] = info.reserved[1] = 0;
    int o = DIRECTORY_FIXED + X;
    if (o > D) return CHECK_MISMATCHED;
    if (N > INDEX_MAX) return CHECK_TOO_LARGE;
    for (int i = 0; i < N; i++) {
        if (o + ENTRY_FIXED > D) return CHECK_MISMATCHED;
        const uint8_t *k = d + o + 2;
        const int tid = (d[o] << 8) | d[o + 1];
        const int body_size = (k[0] << 20) | (k[1] << 12) | (k[2] << 4) | (k[3] >> 4);
        const int header_size = ((k[3] & 0x0F) << 9) | (k[4] << 1) | (k[5] >> 7);
        if (header_size < CORE_BYTES || o + 2 + header_size > D) return CHECK_MISMATCHED;
        entry(i, tid, o + 2, header_size, body_size, (k[5] >> 1) & 0x3F, ((k[5] & 1) << 8) | k[6]);
        o += 2 + header_size;
    }
    return o == D ? CHECK_OK : CHECK_MISMATCHED;
}

/* ---------------------------------------------------------------------------------------------------------------------
 * Control */
DABGPU_MOT_FN void directory_segment(State &st, Counters &c, mot::Orders &ord, const Call &call, const mot::GroupSegment &g) {
    mot::Counters &mc = c.head.mot;
    if (st.cur_valid && st.cur_tid == g.tid) {
        mc.groups_repeated++;
        return;
    }
    if (st.cur_valid || !st.dir_valid || st.dir_tid != g.tid) {
        forget_current(st);
        empty_directory_assembly(st);
        st.dir_valid = 1;
        st.dir_tid = uint16_t(g.tid);
    }
    if (st.dir_too_large) return;
    const int at = mot::place(st.dir, st.dir_too_large, mc, SEGMENTS, call.directory_capacity, g.n, g.last, g.z);
    if (at == mot::PLACE_DROPPED) return;
    if (at >= 0) {
        mot::push_order(ord, mot::ORDER_MOVE, g.o, uint32_t(DIRECTORY_OFF + at), g.z);
        mc.object_bytes += g.z;
    }
    if (mot::part_full(st.dir)) st.check_pending = 1;
}

DABGPU_MOT_FN void body_segment(State &st, Counters &c, mot::Orders &ord, const Call &call, const mot::GroupSegment &g) {
    mot::Counters &mc = c.head.mot;
    if (st.cur_valid) {
        const int i = find_listed(st, g.tid);
        if (i < 0) {
            c.groups_unlisted++;
            return;
        }
        if ((st.delivered[i >> 5] >> (i & 31)) & 1) {
            mc.groups_repeated++;
            return;
        }
    }
    /* (the serial definition; a wave may search with a lane per assembly) */
    int k = -1, empty = -1, oldest = 0;
    uint32_t age = 0;
    for (int j = 0; j < call.assemblies; j++) {
        const Body &b = st.body[j];
        if (b.valid && b.tid == g.tid && k < 0) k = j;
        if (!b.valid && empty < 0) empty = j;
        if (st.placed - b.stamp > age) {
            age = st.placed - b.stamp;
            oldest = j;
        }
    }
    if (k < 0) {
        k = empty;
        if (k < 0) {
            k = oldest;
            c.objects_evicted++;
        }
        Body &b = st.body[k];
        empty_body(b);
        b.valid = 1;
        b.tid = uint16_t(g.tid);
        b.stamp = st.placed;
    }
    Body &b = st.body[k];
    if (b.too_large) return;
    const int at = mot::place(b.part, b.too_large, mc, SEGMENTS, call.object_capacity, g.n, g.last, g.z);
    if (at < 0) return;
    mot::push_order(ord, mot::ORDER_MOVE, g.o, body_off(call, k) + uint32_t(at), g.z);
    mc.object_bytes += g.z;
    st.placed++;
    b.stamp = st.placed;
}

/* a data group whose bytes are all there (take_packet returned true): "Closing a group" with this call's type test */
DABGPU_MOT_FN void close_group(State &st, Counters &c, mot::Orders &ord, const Call &call) {
    mot::State &m = st.pkt.mot;
    mot::Counters &mc = c.head.mot;
    const int need = m.group_need;
    const uint8_t b0 = m.head[0];
    const bool good = (b0 & 0x40) && (m.group_crc ^ 0xFFFFu) == pad::CRC_GOOD_RESIDUE;
    mot::drop_group(m);
    if (!good) {
        mc.groups_crc_failed++;
        return;
    }
    const int type = b0 & 0x0F;
    if (type == 3) {
        c.groups_header_mode++;
        return;
    }
    if (type == 7) {
        c.groups_compressed_directory++;
        return;
    }
    if (type != 4 && type != 6) {
        mc.groups_ignored_type++;
        return;
    }
    mot::GroupSegment g;
    if (!mot::group_segment(m.head, need, mc, g)) return;
    if (type == 6) directory_segment(st, c, ord, call, g);
    else body_segment(st, c, ord, call, g);
}

/* phase 1 of a followed packet of L slots; pkt: its first pkt::packet_read_bytes() bytes */
DABGPU_MOT_FN void follow_packet(State &st, Counters &c, mot::Orders &ord, const Call &call, const uint8_t *pkt, int L) {
    if (pkt::take_packet(st.pkt, c.head, ord, pkt, L)) close_group(st, c, ord, call);
}

/* phase 2, when st.check_pending: the directory's bytes are in place at `directory` = arena + DIRECTORY_OFF.  -> true when
 * the directory has become current: the caller then clears the stale assemblies, clear_stale() or a lane per assembly */
DABGPU_MOT_FN bool check_directory_phase(State &st, Counters &c, mot::Orders &ord, const uint8_t *directory) {
    ord.n = 0;
    const int D = mot::part_bytes(st.dir), tid = st.dir_tid;
    empty_directory_assembly(st);
    DirectoryInfo info = {};
    IndexEntry *index = st.index;
    const int r = check_directory(directory, D, info, [index](int i, int id, int offset, int header_size, int body_size, int type, int subtype) {
        IndexEntry &e = index[i];
        e.offset = uint32_t(offset);
        e.body_size = uint32_t(body_size);
        e.tid = uint16_t(id);
        e.header_size = uint16_t(header_size);
        e.subtype = uint16_t(subtype);
        e.type = uint8_t(type);
        e.pad = 0;
    });
    if (r != CHECK_OK) {
        if (r == CHECK_TOO_LARGE) c.directories_too_large++;
        else c.directories_mismatched++;
        return false;
    }
    c.directories_completed++;
    st.cur_valid = 1;
    st.cur_tid = uint16_t(tid);
    st.cur_bytes = D;
    st.cur_objects = info.objects;
    st.cur_period = info.period;
    st.cur_segment_size = info.segment_size;
    mot::push_order(ord, ORDER_DIRECTORY, DIRECTORY_OFF, 0u, D);
    c.head.mot.object_bytes += D;
    return true;
}
/* assembly k holds an id the current directory does not list: no assembly depends on another, so a wave may ask a lane per
 * assembly, empty those that say yes and count them */
DABGPU_MOT_FN bool body_is_stale(const State &st, int k) { return st.body[k].valid && find_listed(st, st.body[k].tid) < 0; }
DABGPU_MOT_FN void clear_stale(State &st, Counters &c, const Call &call) {
    for (int k = 0; k < call.assemblies; k++)
        if (body_is_stale(st, k)) {
            empty_body(st.body[k]);
            c.objects_stale++;
        }
}

/* phase 3: one emission attempt */
DABGPU_MOT_FN void emit_attempt(State &st, Counters &c, mot::Orders &ord, Call &call) {
    ord.n = 0;
    if (!st.cur_valid) return;
    int k = -1, i = -1;
    for (int j = 0; j < call.assemblies && k < 0; j++)
        if (st.body[j].valid && mot::part_full(st.body[j].part)) {
            i = find_listed(st, st.body[j].tid);
            if (i >= 0) k = j;
        }
    if (k < 0) return;
    Body &b = st.body[k];
    const IndexEntry &e = st.index[i];
    const int bytes = mot::part_bytes(b.part), hbytes = e.header_size;
    if (uint32_t(bytes) != e.body_size) {
        c.head.mot.objects_mismatched++;
        empty_body(b);
        return;
    }
    if (uint32_t(mot::RECORD_BYTES + hbytes + bytes) > call.object_stride) {
        c.objects_dropped++;
        st.delivered[i >> 5] |= 1u << (i & 31);
        empty_body(b);
        return;
    }
    if (c.objects_written >= call.max_objects) {
        if (!((call.deferred >> k) & 1)) c.objects_deferred++;
        call.deferred |= 1u << k;
        return;
    }
    int32_t *r = ord.record[0];
    r[0] = b.tid;
    r[1] = e.type;
    r[2] = e.subtype;
    r[3] = hbytes;
    r[4] = bytes;
    r[5] = call.frame;
    r[6] = call.slot;
    r[7] = st.cur_tid;
    const uint32_t slot = uint32_t(c.objects_written) * call.object_stride;
    mot::push_order(ord, mot::ORDER_RECORD, 0, slot, mot::RECORD_BYTES);
    mot::push_order(ord, ORDER_OBJECT, int32_t(DIRECTORY_OFF + e.offset), slot + mot::RECORD_BYTES, hbytes);
    mot::push_order(ord, ORDER_OBJECT, int32_t(body_off(call, k)), slot + mot::RECORD_BYTES + uint32_t(hbytes), bytes);
    c.objects_written++;
    c.head.mot.objects_completed++;
    c.head.mot.object_bytes += hbytes + bytes;
    st.delivered[i >> 5] |= 1u << (i & 31);
    empty_body(b);
}

/* the end of a call: what the result says of the current directory */
DABGPU_MOT_FN void finish(const State &st, Counters &c) {
    c.directory_id = st.cur_valid ? int32_t(st.cur_tid) : -1;
    c.directory_bytes = st.cur_valid ? st.cur_bytes : 0;
    c.directory_objects = st.cur_valid ? st.cur_objects : 0;
    c.directory_period = st.cur_valid ? st.cur_period : 0;
    c.directory_segment_size = st.cur_valid ? st.cur_segment_size : 0;
}

/* ---------------------------------------------------------------------------------------------------------------------
 * Host side */
struct DirectoryObject {                  /* == dabgpu_mot_directory_object */
    int32_t transport_id, header_offset, header_bytes, body_bytes, content_type, content_subtype;
    int32_t reserved[2];
};
static_assert(sizeof(DirectoryInfo) == 32 && sizeof(DirectoryObject) == 32, "records of the ABI");

/* -> 0, -1 (the check refuses the directory) or -2 (more than `max` objects); writes only on 0 */
inline int parse_directory(const uint8_t *d, int n, DirectoryInfo &info, DirectoryObject *out, int max, int *n_out) {
    DirectoryInfo r = {};
    auto nothing = [](int, int, int, int, int, int, int) {};
    if (!d || n < 0 || check_directory(d, n, r, nothing) != CHECK_OK) return -1;
    if (r.objects > max) return -2;
    check_directory(d, n, r, [out](int i, int tid, int offset, int header_size, int body_size, int type, int subtype) {
        out[i] = DirectoryObject{tid, offset, header_size, body_size, type, subtype, {0, 0}};
    });
    info = r;
    *n_out = r.objects;
    return 0;
}

/* One order on memory the caller can address: the host's executor (the kernel has its own, a wave wide) */
inline void execute_order(const mot::Order &o, const mot::Orders &ord, const uint8_t *pkt, uint8_t *arena, uint8_t *directory,
                          uint8_t *objects) {
    if (o.kind == pkt::ORDER_PACKET)
        for (int i = 0; i < o.len; i++) arena[o.dst + i] = pkt[o.src + i];
    else if (o.kind == mot::ORDER_MOVE)
        for (int i = 0; i < o.len; i++) arena[o.dst + i] = arena[o.src + i];
    else if (o.kind == ORDER_DIRECTORY)
        for (int i = 0; i < o.len; i++) directory[o.dst + i] = arena[o.src + i];
    else if (o.kind == ORDER_OBJECT)
        for (int i = 0; i < o.len; i++) objects[o.dst + i] = arena[o.src + i];
    else if (o.kind == mot::ORDER_RECORD)
        for (int i = 0; i < mot::RECORD_BYTES; i++) objects[o.dst + i] = reinterpret_cast<const uint8_t *>(ord.record[o.src])[i];
}

/* One followed packet, its three phases, on memory the caller can read and write */
inline void walk_packet(State &st, Counters &c, Call &call, const uint8_t *pkt, int L, uint8_t *arena, uint8_t *directory,
                        uint8_t *objects) {
    mot::Orders ord;
    follow_packet(st, c, ord, call, pkt, L);
    for (int i = 0; i < ord.n; i++) execute_order(ord.o[i], ord, pkt, arena, directory, objects);
    if (st.check_pending) {
        if (check_directory_phase(st, c, ord, arena + DIRECTORY_OFF)) clear_stale(st, c, call);
        for (int i = 0; i < ord.n; i++) execute_order(ord.o[i], ord, pkt, arena, directory, objects);
    }
    emit_attempt(st, c, ord, call);
    for (int i = 0; i < ord.n; i++) execute_order(ord.o[i], ord, pkt, arena, directory, objects);
}

/* One entry of a call: the twin of the two kernels.  `call` keeps the deferred marks: one per call. */
inline void walk_frames(State &st, Counters &c, Call &call, const uint8_t *in, uint64_t in_stride, int n_cifs, int S, int address,
                        int fec, uint8_t *arena, uint8_t *directory, uint8_t *objects) {
    for (int k = 0; k < n_cifs; k++) {
        const uint8_t *frame = in + uint64_t(k) * in_stride;
        call.frame = k;
        pkt::scan_frame(c.head, frame, S, address, fec, [&](int pos, int L) {
            call.slot = pos;
            walk_packet(st, c, call, frame + pkt::SLOT_BYTES * pos, L, arena, directory, objects);
        });
    }
    finish(st, c);
}

}  /* namespace dabgpu_carousel */
#endif
