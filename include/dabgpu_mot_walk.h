/* dabgpu_mot_walk.h -- the slideshow objects (MOT, header mode) of a DAB+ service, from the X-PAD of its access units.
 *
 * One implementation of the contract that stands at dabgpu_mot_slides_dev in dabgpu.h (EN 300 401 clauses 5.3.3 and
 * 7.4.5.1, EN 301 234 clauses 5 and 6, TS 101 499 clause 6.2): the kernel, its host twin dabgpu_mot_slides_host and the
 * header parser behind dabgpu_mot_header_parse all run the code below.  Plain C++17, header-only, no allocation, no table
 * in memory; the walk is __host__ __device__ under hipcc and inline otherwise (the header parser and the order loop are
 * the host's).
 *
 * The X-PAD field walk is dabgpu_pad_walk.h's walk_fields(): the label's sink and this one run the same code up to the
 * sub-field.  This sink holds the CONTROL only: walk_au() takes one access unit and the state record, updates state and
 * counters, and returns copy orders.  It moves no payload byte itself; it reads the bytes of the access unit (for the CRC
 * and the first 32 bytes of a data group, which it keeps in the state) and nothing of the arena.  The caller executes the
 * orders in their order, each complete before the next one begins: a loop on the host, the whole wave in the kernel.
 *
 * The arena (belongs to the state, updated in place):
 *   [0, GROUP_CAP)                       the open X-PAD data group, as its bytes arrive
 *   [HEADER_OFF, HEADER_OFF + HEADER_CAP) the MOT header under assembly
 *   [BODY_OFF, BODY_OFF + body_capacity)  the MOT body under assembly
 */
#ifndef DABGPU_MOT_WALK_H
#define DABGPU_MOT_WALK_H

#include "dabgpu_pad_walk.h"

/* the control walk is inlined whole into its one caller (a call would need a stack, on the device scratch memory) */
#if defined(__HIPCC__)
#define DABGPU_MOT_FN __host__ __device__ __forceinline__
#else
#define DABGPU_MOT_FN inline
#endif

namespace dabgpu_mot {

namespace pad = dabgpu_pad;

constexpr int GROUP_CAP = 16384;          /* the length indicator has 14 bits */
constexpr int HEADER_CAP = 1024;          /* cap on header bytes */
constexpr int HEADER_SEGMENTS = 32;       /* ... and header segments */
constexpr int BODY_SEGMENTS = 256;        /* cap on body segments */
constexpr int SEGMENT_MAX = 8191;         /* the segmentation header has 13 bits */
constexpr int BODY_CAP_MAX = BODY_SEGMENTS * SEGMENT_MAX;
constexpr int HEADER_OFF = GROUP_CAP, BODY_OFF = GROUP_CAP + HEADER_CAP;
constexpr int HEAD_BYTES = 32;            /* of a data group, kept in the state: every header there can be and the MOT header core */
constexpr int RECORD_BYTES = 32;

struct Counters {                         /* == dabgpu_mot_result */
    int32_t aus, aus_lost, aus_with_xpad, pad_malformed, fields_ignored;
    int32_t lengths_ok, lengths_ignored, groups_no_length;
    int32_t groups_ok, groups_crc_failed, groups_ignored_type, groups_no_transport_id, groups_malformed, groups_repeated;
    int32_t segments_placed, segments_repeated, segments_early_last;
    int32_t objects_completed, objects_mismatched, objects_too_large;
    int32_t slides_written, slides_dropped;
    int32_t xpad_bytes, object_bytes;     /* payload bytes the orders of this call moved: X-PAD -> group, group -> object -> slot */
    int32_t reserved[8];
};

struct Part {                             /* header (0) or body (1) under assembly */
    int32_t seg_size;                     /* of the first non-last segment seen, 0 = not known */
    int32_t last;                         /* number of the last segment + 1, 0 = not seen */
    int32_t last_len;
    int32_t pad;
    uint32_t have[BODY_SEGMENTS / 32];    /* bit n = segment n present */
};

struct alignas(16) State {                /* all zero = a fresh start */
    uint8_t cont_type, last_len;          /* as dabgpu_pad::State */
    uint8_t group_open, armed;            /* armed: next_length waits for a type-12 sub-field */
    uint16_t next_length, group_need, group_have;
    uint16_t group_crc;                   /* the CRC register over the open group's bytes so far, complemented */
    uint8_t asm_valid, done_valid, too_large;
    uint8_t core_have;                    /* bit i = byte i of the header core is in core[] */
    uint16_t asm_tid, done_tid;
    int32_t body_capacity;                /* of the arena this record goes with */
    uint8_t core[8];
    uint8_t head[HEAD_BYTES];             /* the first bytes of the open group */
    Part part[2];
};

struct Call {                             /* what the caller's entry says, and where the walk is */
    int32_t body_capacity, max_slides;
    uint32_t slide_stride;
    int32_t superframe, au;
};

enum OrderKind : int32_t {
    ORDER_XPAD = 1,    /* arena[dst + i] = au[src - i], i < len: X-PAD bytes, reversed, into the group buffer */
    ORDER_MOVE = 2,    /* arena[dst + i] = arena[src + i]: a segment from the group buffer to its place (no overlap) */
    ORDER_SLIDE = 3,   /* slides[dst + i] = arena[src + i]: header or body of a completed object into its slot */
    ORDER_RECORD = 4   /* slides[dst ..] = record[src], 32 bytes */
};
struct Order {
    int32_t kind, src;
    uint32_t dst;
    int32_t len;
};
constexpr int MAX_ORDERS = 20;            /* four sub-fields: bytes in, a segment placed, header, body and record out */
struct Orders {
    int32_t n, pad[3];
    Order o[MAX_ORDERS];
    int32_t record[4][8];                 /* == dabgpu_mot_slide */
};
static_assert(sizeof(Counters) == 128 && sizeof(Part) == 48 && sizeof(State) == 160 && sizeof(Order) == 16, "records of the ABI");

DABGPU_PAD_FN uint64_t arena_bytes(int64_t body_capacity) { return uint64_t(BODY_OFF) + uint64_t((body_capacity + 15) & ~int64_t(15)); }
/* the body capacity an arena of that many bytes has (the caller has refused one below arena_bytes(0)) */
DABGPU_PAD_FN int32_t body_capacity_of(uint64_t bytes) {
    const uint64_t b = bytes - BODY_OFF;
    return b > uint64_t(BODY_CAP_MAX) ? BODY_CAP_MAX : int32_t(b);
}

DABGPU_MOT_FN void drop_group(State &st) {
    st.group_open = 0;
    st.group_need = st.group_have = st.group_crc = 0;
}
DABGPU_MOT_FN void drop_context(State &st) {
    st.cont_type = 0;
    st.armed = 0;
    st.next_length = 0;
    drop_group(st);
}
DABGPU_MOT_FN void empty_assembly(State &st) {
    st.asm_valid = st.too_large = st.core_have = 0;
    st.asm_tid = 0;
    for (int i = 0; i < 8; i++) st.core[i] = 0;
    for (int p = 0; p < 2; p++) {
        st.part[p].seg_size = st.part[p].last = st.part[p].last_len = st.part[p].pad = 0;
        for (int w = 0; w < BODY_SEGMENTS / 32; w++) st.part[p].have[w] = 0;
    }
}

DABGPU_MOT_FN int part_segments(int p) { return p ? BODY_SEGMENTS : HEADER_SEGMENTS; }
DABGPU_MOT_FN int part_cap(int p, int body_capacity) { return p ? body_capacity : HEADER_CAP; }
DABGPU_MOT_FN int top_segment(const Part &q) {            /* the highest segment present, -1 = none */
    for (int w = BODY_SEGMENTS / 32 - 1; w >= 0; w--)
        if (q.have[w])
            for (int b = 31; b >= 0; b--)
                if ((q.have[w] >> b) & 1) return 32 * w + b;
    return -1;
}
DABGPU_MOT_FN bool part_full(const Part &q) {             /* segments 0 .. last all there */
    if (!q.last) return false;
    for (int n = 0; n < q.last; n += 32) {
        const uint32_t need = q.last - n >= 32 ? 0xFFFFFFFFu : (1u << (q.last - n)) - 1u;
        if ((q.have[n >> 5] & need) != need) return false;
    }
    return true;
}
DABGPU_MOT_FN int part_bytes(const Part &q) { return (q.last - 1) * q.seg_size + q.last_len; }

/* what this code can have written for this arena, and nothing that would make an order leave it */
DABGPU_MOT_FN bool part_ok(const Part &q, int p, int cap) {
    if (q.seg_size < 0 || q.seg_size > SEGMENT_MAX || q.last < 0 || q.last > part_segments(p) || q.last_len < 0 ||
        q.last_len > SEGMENT_MAX || q.pad != 0)
        return false;
    if (!q.last && q.last_len) return false;
    const int top = top_segment(q);
    if (top >= part_segments(p)) return false;
    if (q.last && top >= q.last) return false;
    if (q.last > 1 && !q.seg_size) return false;
    if (q.last && q.seg_size && q.last_len > q.seg_size) return false;
    if (top > 0 && !q.seg_size) return false;
    if (top >= 0 && top != q.last - 1 && !q.seg_size) return false;
    if (top >= 0 && (top == q.last - 1 ? top * q.seg_size + q.last_len : (top + 1) * q.seg_size) > cap) return false;
    if (q.last && part_bytes(q) > cap) return false;
    return true;
}
DABGPU_MOT_FN bool state_ok(const State &st, int32_t body_capacity) {
    bool ok = (st.cont_type == 0 || st.cont_type == 3 || st.cont_type == 13) && st.last_len <= 48 && st.group_open <= 1 &&
              st.armed <= 1 && st.next_length < GROUP_CAP && (st.armed || !st.next_length) && st.asm_valid <= 1 &&
              st.done_valid <= 1 && st.too_large <= 1 && st.core_have <= 0x7F && st.body_capacity == body_capacity &&
              (st.group_open ? (st.group_need >= 4 && st.group_need < GROUP_CAP && st.group_have < st.group_need)
                             : (st.group_need == 0 && st.group_have == 0 && st.group_crc == 0));
    ok = ok && part_ok(st.part[0], 0, HEADER_CAP) && part_ok(st.part[1], 1, body_capacity);
    for (int w = 1; w < BODY_SEGMENTS / 32; w++) ok = ok && st.part[0].have[w] == 0;
    return ok;
}
DABGPU_MOT_FN void sanitize(State &st, int32_t body_capacity) {
    if (state_ok(st, body_capacity)) return;
    uint8_t *b = reinterpret_cast<uint8_t *>(&st);
    for (unsigned i = 0; i < sizeof(State); i++) b[i] = 0;
    st.body_capacity = body_capacity;
}

DABGPU_MOT_FN void push_order(Orders &ord, int32_t kind, int32_t src, uint32_t dst, int32_t len) {
    if (len <= 0 && kind != ORDER_RECORD) return;
    Order &o = ord.o[ord.n++];
    o.kind = kind;
    o.src = src;
    o.dst = dst;
    o.len = len;
}

/* "Assembly" from "n >= ..." on: segment n (last or not, z bytes) of a part of at most `segments` segments and `cap` bytes.
 * -> the offset in the part where the caller places it (it has been noted present: segments_placed++), PLACE_REPEATED (it was
 * there: segments_repeated++; the part may be full) or PLACE_DROPPED (a rule refused it and counted; the part is as it was,
 * or too_large is set) */
constexpr int PLACE_REPEATED = -1, PLACE_DROPPED = -2;
DABGPU_MOT_FN int place(Part &q, uint8_t &too_large, Counters &c, int segments, int cap, int n, bool last, int z) {
    if (n >= segments) {
        c.objects_too_large++;
        too_large = 1;
        return PLACE_DROPPED;
    }
    int size = q.seg_size;
    if (!last) {
        if (z == 0 || (size && z != size) || (q.last && n >= q.last - 1)) {
            c.groups_malformed++;
            return PLACE_DROPPED;
        }
        size = z;
    } else {
        if (n > 0 && !size) {
            c.segments_early_last++;
            return PLACE_DROPPED;
        }
        if ((q.last && (q.last - 1 != n || q.last_len != z)) || (size && z > size) || top_segment(q) > n) {
            c.groups_malformed++;
            return PLACE_DROPPED;
        }
    }
    const int at = n * size;                                           /* (n = 0 when the size is not known) */
    if (at + z > cap) {
        c.objects_too_large++;
        too_large = 1;
        return PLACE_DROPPED;
    }
    if (!last) {
        q.seg_size = size;
    } else {
        q.last = n + 1;
        q.last_len = z;
    }
    if ((q.have[n >> 5] >> (n & 31)) & 1) {
        c.segments_repeated++;
        return PLACE_REPEATED;
    }
    q.have[n >> 5] |= 1u << (n & 31);
    c.segments_placed++;
    return at;
}

/* "Closing a group" behind the type test: head = the first HEAD_BYTES of a group of `need` bytes whose CRC was good.
 * -> true: groups_ok++, and the segment is g (z bytes at group offset o); false: a rule refused the group and counted */
struct GroupSegment {
    int32_t tid, n, last, o, z;
};
DABGPU_MOT_FN bool group_segment(const uint8_t *head, int need, Counters &c, GroupSegment &g) {
    const uint8_t b0 = head[0];
    const int end = need - 2;                                          /* end: where the CRC begins */
    int o = 2;
    if (b0 & 0x80) o += 2;                                             /* the extension field */
    if (!(b0 & 0x20) || o + 2 > end) {
        c.groups_malformed++;
        return false;
    }
    g.last = head[o] >> 7;
    g.n = ((head[o] & 0x7F) << 8) | head[o + 1];
    o += 2;
    if (!(b0 & 0x10)) {
        c.groups_no_transport_id++;
        return false;
    }
    if (o + 1 > end) {
        c.groups_malformed++;
        return false;
    }
    const int ua = head[o], li = ua & 0x0F;
    o += 1;
    if (!(ua & 0x10)) {
        c.groups_no_transport_id++;
        return false;
    }
    if (li < 2 || o + li + 2 > end) {
        c.groups_malformed++;
        return false;
    }
    g.tid = (head[o] << 8) | head[o + 1];
    o += li;                                                           /* the end-user address behind the transport id */
    g.z = ((head[o] & 0x1F) << 8) | head[o + 1];                       /* (o + 2 <= 2 + 2 + 2 + 1 + 15 + 2 = 24) */
    o += 2;
    if (g.z != end - o) {
        c.groups_malformed++;
        return false;
    }
    g.o = o;
    c.groups_ok++;
    return true;
}

struct Sink {
    State &st;
    Counters &c;
    Orders &ord;
    const Call &call;
    const uint8_t *au;

    DABGPU_MOT_FN void drop_context() { dabgpu_mot::drop_context(st); }

    DABGPU_MOT_FN void order(int32_t kind, int32_t src, uint32_t dst, int32_t len) { push_order(ord, kind, src, dst, len); }

    /* header and body are all there */
    DABGPU_MOT_FN void complete() {
        const int hbytes = part_bytes(st.part[0]), bbytes = part_bytes(st.part[1]);
        const uint8_t *k = st.core;
        const int body_size = (k[0] << 20) | (k[1] << 12) | (k[2] << 4) | (k[3] >> 4);
        const int header_size = ((k[3] & 0x0F) << 9) | (k[4] << 1) | (k[5] >> 7);
        const int tid = st.asm_tid;
        if (st.core_have != 0x7F || header_size != hbytes || body_size != bbytes) {
            c.objects_mismatched++;
            empty_assembly(st);
            return;
        }
        c.objects_completed++;
        if (c.slides_written >= call.max_slides || uint32_t(RECORD_BYTES + hbytes + bbytes) > call.slide_stride) {
            c.slides_dropped++;
        } else {
            int rec = 0;                                               /* the records of this access unit's orders so far */
            for (int i = 0; i < ord.n; i++) rec += ord.o[i].kind == ORDER_RECORD;
            int32_t *r = ord.record[rec];
            r[0] = tid;
            r[1] = (k[5] >> 1) & 0x3F;
            r[2] = ((k[5] & 1) << 8) | k[6];
            r[3] = hbytes;
            r[4] = bbytes;
            r[5] = call.superframe;
            r[6] = call.au;
            r[7] = 0;
            const uint32_t slot = uint32_t(c.slides_written) * call.slide_stride;
            order(ORDER_RECORD, rec, slot, RECORD_BYTES);
            order(ORDER_SLIDE, HEADER_OFF, slot + RECORD_BYTES, hbytes);
            order(ORDER_SLIDE, BODY_OFF, slot + RECORD_BYTES + uint32_t(hbytes), bbytes);
            c.object_bytes += hbytes + bbytes;
            c.slides_written++;
        }
        empty_assembly(st);
        st.done_valid = 1;
        st.done_tid = uint16_t(tid);
    }

    /* a good group: segment n of the header (p = 0) or body (p = 1) of object tid, z bytes at group offset o */
    DABGPU_MOT_FN void segment(int p, int tid, int n, bool last, int o, int z) {
        if (st.done_valid && st.done_tid == tid) {
            c.groups_repeated++;
            return;
        }
        if (!st.asm_valid || st.asm_tid != tid) {
            empty_assembly(st);
            st.asm_valid = 1;
            st.asm_tid = uint16_t(tid);
        }
        if (st.too_large) return;
        const int at = place(st.part[p], st.too_large, c, part_segments(p), part_cap(p, call.body_capacity), n, last, z);
        if (at == PLACE_DROPPED) return;
        if (at >= 0) {
            order(ORDER_MOVE, o, uint32_t((p ? BODY_OFF : HEADER_OFF) + at), z);
            c.object_bytes += z;
            if (p == 0)                                                /* what of the header core lies in this segment */
                for (int h = at; h < 7 && h < at + z; h++) {
                    st.core[h] = st.head[o + h - at];
                    st.core_have |= uint8_t(1u << h);
                }
        }
        if (part_full(st.part[0]) && part_full(st.part[1])) complete();
    }

    /* a data group whose bytes are all there: head[] holds its first 32 */
    DABGPU_MOT_FN void close_group() {
        const int need = st.group_need;
        const uint8_t b0 = st.head[0];
        const bool good = (b0 & 0x40) && (st.group_crc ^ 0xFFFFu) == pad::CRC_GOOD_RESIDUE;
        drop_group(st);
        if (!good) {
            c.groups_crc_failed++;
            return;
        }
        const int type = b0 & 0x0F;
        if (type != 3 && type != 4) {
            c.groups_ignored_type++;
            return;
        }
        GroupSegment g;
        if (group_segment(st.head, need, c, g)) segment(type == 4, g.tid, g.n, g.last, g.o, g.z);
    }

    DABGPU_MOT_FN void subfield(int type, const uint8_t *xpad_end, int at, int len) {
        if (type == 1) {                                               /* the data group length indicator */
            if (len < 4) {
                c.lengths_ignored++;
                return;
            }
            const uint8_t b0 = xpad_end[-at], b1 = xpad_end[-(at + 1)], b2 = xpad_end[-(at + 2)], b3 = xpad_end[-(at + 3)];
            uint32_t crc = pad::crc16_step(pad::crc16_step(0xFFFF, b0), b1) ^ 0xFFFF;
            if (crc != ((uint32_t(b2) << 8) | b3)) {
                c.lengths_ignored++;
                return;
            }
            c.lengths_ok++;
            st.armed = 1;
            st.next_length = uint16_t(((b0 & 0x3F) << 8) | b1);
            return;
        }
        if (type == 12) {
            drop_group(st);
            const int need = st.next_length;
            const bool armed = st.armed;
            st.armed = 0;
            st.next_length = 0;
            if (!armed) {
                c.groups_no_length++;
                return;
            }
            if (need < 4) {                                            /* no room for the header and the CRC */
                c.groups_malformed++;
                return;
            }
            st.group_open = 1;
            st.group_need = uint16_t(need);
        }
        if ((type != 12 && type != 13) || !st.group_open) return;
        const int have = st.group_have, need = st.group_need;
        const int take = len < need - have ? len : need - have;        /* bytes beyond the length are padding */
        uint32_t crc = st.group_crc ^ 0xFFFFu;
        for (int i = 0; i < take; i++) {
            const uint8_t v = xpad_end[-(at + i)];
            crc = pad::crc16_step(crc, v);
            if (have + i < HEAD_BYTES) st.head[have + i] = v;
        }
        order(ORDER_XPAD, int32_t(xpad_end - au) - at, uint32_t(have), take);
        c.xpad_bytes += take;
        st.group_have = uint16_t(have + take);
        st.group_crc = uint16_t(crc ^ 0xFFFFu);
        if (have + take == need) close_group();
    }
};

/* au: the access unit without its CRC, len >= 0 bytes; len < 0: lost (au is not read).  ord: this access unit's orders */
DABGPU_MOT_FN void walk_au(State &st, Counters &c, Orders &ord, const Call &call, const uint8_t *au, int len) {
    ord.n = 0;
    Sink k{st, c, ord, call, au};
    pad::walk_fields(k, au, len);
}

/* ---------------------------------------------------------------------------------------------------------------------
 * The MOT header (EN 301 234 clause 6, TS 101 499 clause 6.2), host side: == dabgpu_mot_header */
constexpr int TEXT_MAX = 255;
struct Text {
    int32_t length;                       /* -1 = the parameter is not there */
    uint8_t bytes[TEXT_MAX + 1];          /* bytes behind `length` are zero */
};
struct Header {
    int32_t body_size, header_size, content_type, content_subtype;
    int32_t n_params, n_unknown;
    int32_t name_charset;                 /* -1 = no ContentName */
    int32_t has_trigger, trigger_now;     /* now: the validity bit is clear */
    uint32_t trigger_time;                /* the first four bytes, big-endian */
    int32_t has_expire, expire_now;
    uint32_t expire_time;
    int32_t has_category, category_id, slide_id;
    Text name, category_title, click_through_url, alternative_location_url;
};
static_assert(sizeof(Text) == 260 && sizeof(Header) == 64 + 4 * 260, "records of the ABI");

/* -> 0, or -1 (the header is not n bytes of a well-formed MOT header) or -2 (a text longer than TEXT_MAX); `out` is written
 * only on 0 */
inline int parse_header(const uint8_t *h, int n, Header &out) {
    if (!h || n < 7) return -1;
    Header r{};
    r.body_size = (h[0] << 20) | (h[1] << 12) | (h[2] << 4) | (h[3] >> 4);
    r.header_size = ((h[3] & 0x0F) << 9) | (h[4] << 1) | (h[5] >> 7);
    r.content_type = (h[5] >> 1) & 0x3F;
    r.content_subtype = ((h[5] & 1) << 8) | h[6];
    if (r.header_size != n) return -1;
    r.name_charset = -1;
    r.name.length = r.category_title.length = r.click_through_url.length = r.alternative_location_url.length = -1;
    int at = 7;
    while (at < n) {
        const int pli = h[at] >> 6, id = h[at] & 0x3F;
        at++;
        int len = pli == 0 ? 0 : pli == 1 ? 1 : pli == 2 ? 4 : -1;
        if (len < 0) {
            if (at >= n) return -1;
            len = h[at] & 0x7F;
            if (h[at] & 0x80) {
                if (at + 1 >= n) return -1;
                len = (len << 8) | h[at + 1];
                at++;
            }
            at++;
        }
        if (at + len > n) return -1;
        const uint8_t *d = h + at;
        Text *text = nullptr;
        int skip = 0;
        r.n_params++;
        if (id == 0x0C) {
            if (len < 1) return -1;
            r.name_charset = d[0] >> 4;
            text = &r.name;
            skip = 1;
        } else if (id == 0x05 || id == 0x04) {
            if (len < 4) return -1;
            const uint32_t t = (uint32_t(d[0]) << 24) | (uint32_t(d[1]) << 16) | (uint32_t(d[2]) << 8) | d[3];
            if (id == 0x05) {
                r.has_trigger = 1;
                r.trigger_now = !(d[0] >> 7);
                r.trigger_time = t;
            } else {
                r.has_expire = 1;
                r.expire_now = !(d[0] >> 7);
                r.expire_time = t;
            }
        } else if (id == 0x25) {
            if (len < 2) return -1;
            r.has_category = 1;
            r.category_id = d[0];
            r.slide_id = d[1];
        } else if (id == 0x26) {
            text = &r.category_title;
        } else if (id == 0x27) {
            text = &r.click_through_url;
        } else if (id == 0x28) {
            text = &r.alternative_location_url;
        } else {
            r.n_unknown++;
        }
        if (text) {
            if (len - skip > TEXT_MAX) return -2;
            text->length = len - skip;
            for (int i = 0; i < TEXT_MAX + 1; i++) text->bytes[i] = i < len - skip ? d[skip + i] : 0;
        }
        at += len;
    }
    out = r;
    return 0;
}

/* One order on memory the caller can address: the host's executor (the kernel has its own, a wave wide) */
inline void execute(const Order &o, const Orders &ord, const uint8_t *au, uint8_t *arena, uint8_t *slides) {
    if (o.kind == ORDER_XPAD)
        for (int i = 0; i < o.len; i++) arena[o.dst + i] = au[o.src - i];
    else if (o.kind == ORDER_MOVE)
        for (int i = 0; i < o.len; i++) arena[o.dst + i] = arena[o.src + i];
    else if (o.kind == ORDER_SLIDE)
        for (int i = 0; i < o.len; i++) slides[o.dst + i] = arena[o.src + i];
    else if (o.kind == ORDER_RECORD)
        for (int i = 0; i < RECORD_BYTES; i++) slides[o.dst + i] = reinterpret_cast<const uint8_t *>(ord.record[o.src])[i];
}

/* One entry of a call, on memory the caller can read and write: the twin of the kernel's loop */
inline void walk_superframes(State &st, Counters &c, const Call &entry, const uint8_t *data, uint64_t data_stride,
                             const int32_t *status, int n_superframes, int s, uint8_t *arena, uint8_t *slides) {
    Orders ord;
    Call call = entry;
    for (int k = 0; k < n_superframes; k++) {
        const int32_t *row = status + 16 * int64_t(k);
        const int n = pad::visited_aus(row[0], row[3]);
        for (int a = 0; a < n; a++) {
            int b = 0;
            const int len = pad::au_span(row[0], row[3], row[4], row[5 + a], row[6 + a], a, s, &b);
            const uint8_t *au = data + uint64_t(k) * data_stride + (len < 0 ? 0 : b);
            call.superframe = k;
            call.au = a;
            walk_au(st, c, ord, call, au, len);
            for (int i = 0; i < ord.n; i++) execute(ord.o[i], ord, au, arena, slides);
        }
    }
}

}  /* namespace dabgpu_mot */
#endif
