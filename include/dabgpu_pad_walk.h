/* dabgpu_pad_walk.h -- the dynamic label of a DAB+ service, from the PAD of its access units.
 *
 * One implementation of the contract that stands at dabgpu_pad_labels_dev in dabgpu.h (EN 300 401 clauses 7.4.2 - 7.4.5,
 * TS 102 563 clause 5.4): the kernel, its host twin dabgpu_pad_labels_host and the host mirror's DAB+ channel all run
 * walk_au() below.  Plain C++17, header-only, no allocation, no table in memory; every function is __host__ __device__
 * under hipcc and inline otherwise.
 *
 * The X-PAD field walk itself (walk_fields: locating the PAD, F-PAD, short and variable X-PAD, the content-indicator list,
 * continuation without one) is a template over its sink; the label's sink is below, the slideshow's in dabgpu_mot_walk.h.
 *
 * walk_au takes ONE access unit -- its bytes without the AU CRC, or "lost" -- and a state record, and updates the state
 * (continuation context, open data group, segment assembly, current label) and the counters.  It reads nothing outside
 * [au, au + len), whatever the bytes say.  The decisions the standards leave open, as taken here:
 *   - a short X-PAD field's content indicator counts as a list of one 4-byte sub-field (what a CI-less variable field
 *     behind it continues with);
 *   - a content-indicator list resets the continued type before its sub-fields set it: an empty list leaves none;
 *   - of several segments with the last flag, the most recent one names the last segment;
 *   - a completed label sets the label record's toggle whether its text changed or not; a clear command zeroes the record;
 *   - text bytes behind `length` are zero;
 *   - a state record whose fields are out of range (not written by this code) is a fresh start.
 */
#ifndef DABGPU_PAD_WALK_H
#define DABGPU_PAD_WALK_H

#include <stdint.h>

#if defined(__HIPCC__)
#define DABGPU_PAD_FN __host__ __device__ inline
#else
#define DABGPU_PAD_FN inline
#endif

namespace dabgpu_pad {

struct Label {                 /* == dabgpu_pad_label */
    int32_t length, charset, toggle, reserved;
    uint8_t text[128];
};

struct Counters {              /* == dabgpu_pad_result */
    int32_t aus, aus_lost, aus_with_xpad, pad_malformed, fields_ignored, groups_ok, groups_crc_failed, commands_ignored,
        labels_completed, changes, reserved[6];
};

constexpr int GROUP_MAX = 20;  /* prefix 2 + at most 16 bytes + CRC 2 */

struct alignas(16) State {     /* all zero = a fresh start */
    uint8_t cont_type;         /* 0 = none, 3 = DLS continuation, 13 = the other application's */
    uint8_t last_len;          /* length of the last sub-field of the most recent content-indicator list */
    uint8_t group_open, group_have, group_need;   /* need: 0 until the prefix is there */
    uint8_t asm_toggle, asm_have /* bit m = segment m present */, asm_last /* last segment + 1, 0 = not seen */;
    uint8_t asm_charset, pad0;
    uint16_t group_crc;        /* the CRC register over the open group's bytes so far, complemented (0 = none yet) */
    uint8_t pad2[4];
    uint8_t group[32];
    uint8_t seg_len[8], pad1[8];
    uint8_t seg[8][16];
    Label label;
};
static_assert(sizeof(Label) == 144 && sizeof(Counters) == 64 && sizeof(State) == 336, "records of the ABI");

DABGPU_PAD_FN void drop_group(State &st) {
    st.group_open = st.group_have = st.group_need = 0;
    st.group_crc = 0;
}
DABGPU_PAD_FN void drop_context(State &st) {
    st.cont_type = 0;
    drop_group(st);
}
DABGPU_PAD_FN void empty_assembly(State &st) { st.asm_have = st.asm_last = st.asm_charset = 0; }

/* anything this code cannot have written: start afresh */
DABGPU_PAD_FN void sanitize(State &st) {
    bool ok = (st.cont_type == 0 || st.cont_type == 3 || st.cont_type == 13) && st.last_len <= 48 && st.group_open <= 1 &&
              st.group_have <= GROUP_MAX && st.group_need <= GROUP_MAX && st.asm_toggle <= 1 && st.asm_last <= 8 &&
              st.asm_charset <= 15 && st.label.length >= 0 && st.label.length <= 128 &&
              (st.group_open ? (st.group_have < 2 ? st.group_need == 0 : st.group_have < st.group_need)
                             : (st.group_have == 0 && st.group_need == 0));
    for (int m = 0; m < 8; m++) ok = ok && st.seg_len[m] <= 16;
    if (ok) return;
    uint8_t *b = reinterpret_cast<uint8_t *>(&st);
    for (unsigned i = 0; i < sizeof(State); i++) b[i] = 0;
}

/* the FIB CRC: CCITT 0x1021, start 0xFFFF, complemented -- a byte a step (x^16 + x^12 + x^5 + 1 has so few terms that the
 * eight shifts of one byte fold into three).  A message followed by its complemented CRC leaves the register at 0x1D0F. */
DABGPU_PAD_FN uint32_t crc16_step(uint32_t crc, uint8_t v) {
    uint32_t x = (crc >> 8) ^ v;
    x ^= x >> 4;
    return ((crc << 8) ^ (x << 12) ^ (x << 5) ^ x) & 0xFFFF;
}
DABGPU_PAD_FN uint32_t crc16(const uint8_t *p, int n) {
    uint32_t crc = 0xFFFF;
    for (int i = 0; i < n; i++) crc = crc16_step(crc, p[i]);
    return crc ^ 0xFFFF;
}
constexpr uint32_t CRC_GOOD_RESIDUE = 0x1D0F;

DABGPU_PAD_FN void complete_label(State &st, Counters &c) {
    const int last = st.asm_last - 1, old_length = st.label.length;
    int length = 0;
    bool differs = st.label.charset != st.asm_charset;
    for (int m = 0; m <= last; m++) {
        for (int i = 0; i < st.seg_len[m] && length < 128; i++, length++) {
            const uint8_t v = st.seg[m][i];
            if (st.label.text[length] != v) {                          /* (one pass: what differs is replaced as it is found) */
                st.label.text[length] = v;
                differs = true;
            }
        }
    }
    for (int i = length; i < old_length; i++) st.label.text[i] = 0;    /* bytes behind the length stay zero */
    c.labels_completed++;
    if (differs || old_length != length) {
        st.label.length = length;
        st.label.charset = st.asm_charset;
        c.changes++;
    }
    st.label.toggle = st.asm_toggle;
    empty_assembly(st);
}

/* a data group whose bytes are all there */
DABGPU_PAD_FN void close_group(State &st, Counters &c) {
    const uint8_t b0 = st.group[0], b1 = st.group[1];
    const bool good = (st.group_crc ^ 0xFFFFu) == CRC_GOOD_RESIDUE;
    if (!good) {
        c.groups_crc_failed++;
    } else {
        c.groups_ok++;
        if (b0 & 0x10) {
            if ((b0 & 0x0F) == 1) {                                   /* clear */
                empty_assembly(st);
                if (st.label.length != 0) c.changes++;
                uint8_t *l = reinterpret_cast<uint8_t *>(&st.label);
                for (unsigned i = 0; i < sizeof(Label); i++) l[i] = 0;
            } else {
                c.commands_ignored++;                                 /* DL Plus: checked, not read */
            }
        } else {
            const int toggle = b0 >> 7, first = (b0 >> 6) & 1, last = (b0 >> 5) & 1, nbytes = (b0 & 0x0F) + 1;
            if (toggle != st.asm_toggle) {
                empty_assembly(st);
                st.asm_toggle = uint8_t(toggle);
            }
            const int m = first ? 0 : (b1 >> 4) & 7;
            if (first) st.asm_charset = b1 >> 4;
            for (int i = 0; i < nbytes; i++) st.seg[m][i] = st.group[2 + i];
            st.seg_len[m] = uint8_t(nbytes);
            st.asm_have |= uint8_t(1u << m);
            if (last) st.asm_last = uint8_t(m + 1);
            if (st.asm_last) {
                const uint32_t need = (2u << (st.asm_last - 1)) - 1u;  /* segments 0 .. last */
                if ((st.asm_have & need) == need) complete_label(st, c);
            }
        }
    }
    drop_group(st);
}

/* bytes a data group has in all, from its prefix; 0 = a command nobody knows */
DABGPU_PAD_FN int group_length(uint8_t b0, uint8_t b1) {
    if (!(b0 & 0x10)) return 2 + (b0 & 0x0F) + 1 + 2;
    if ((b0 & 0x0F) == 1) return 4;
    if ((b0 & 0x0F) == 2) return 2 + (b1 & 0x0F) + 1 + 2;
    return 0;
}

/* one sub-field: `len` logical X-PAD bytes from logical byte `at`; logical byte i is xpad_end[-i].  The open group's
 * counters stay in locals while its bytes come in (a byte store may alias every field of the record). */
DABGPU_PAD_FN void subfield(State &st, Counters &c, int type, const uint8_t *xpad_end, int at, int len) {
    if (type == 2) {
        drop_group(st);
        st.group_open = 1;
    }
    if ((type == 2 || type == 3) && st.group_open) {
        int have = st.group_have, need = st.group_need;
        uint32_t crc = st.group_crc ^ 0xFFFFu;
        bool open = true;
        for (int i = 0; i < len; i++) {
            const uint8_t v = xpad_end[-(at + i)];
            st.group[have++] = v;
            crc = crc16_step(crc, v);
            if (have == 2) {
                need = group_length(st.group[0], st.group[1]);
                if (!need) {
                    c.commands_ignored++;
                    open = false;
                    break;
                }
            }
            if (have == need) {
                st.group_crc = uint16_t(crc ^ 0xFFFFu);
                close_group(st, c);
                open = false;
                break;                                                /* what is left of the sub-field is ignored */
            }
        }
        if (open) {
            st.group_have = uint8_t(have);
            st.group_need = uint8_t(need);
            st.group_crc = uint16_t(crc ^ 0xFFFFu);
        } else {
            drop_group(st);
        }
    }
}

/* what a CI-less field behind a sub-field of this type continues with */
DABGPU_PAD_FN uint8_t continued_type(int type) { return (type == 2 || type == 3) ? 3 : (type == 12 || type == 13) ? 13 : 0; }

DABGPU_PAD_FN int subfield_length(int index) { return ((index & 1) ? 6 : 4) << (index >> 1); }

/* one sub-field to the sink; its type names what a CI-less field behind it continues */
template <class Sink> DABGPU_PAD_FN void field(Sink &sink, int type, const uint8_t *xpad_end, int at, int len) {
    sink.subfield(type, xpad_end, at, len);
    sink.st.cont_type = continued_type(type);
}

/* The X-PAD field walk of one access unit, for any sink (the label's below, the slideshow's in dabgpu_mot_walk.h): locating
 * the PAD, F-PAD, short and variable X-PAD, the content-indicator list, continuation without one.  A sink has
 *   st: a state record with cont_type and last_len;  c: counters with aus, aus_lost, aus_with_xpad, pad_malformed,
 *   fields_ignored;  drop_context(): no continued type, no open data group;
 *   subfield(type, xpad_end, at, len): `len` logical bytes from logical byte `at`, logical byte i = xpad_end[-i].
 * au: the access unit without its CRC, len >= 0 bytes; len < 0: the access unit is lost (au is not read) */
template <class Sink> DABGPU_PAD_FN void walk_fields(Sink &sink, const uint8_t *au, int len) {
    auto &st = sink.st;
    auto &c = sink.c;
    c.aus++;
    if (len < 0) {
        c.aus_lost++;
        sink.drop_context();
        return;
    }
    if (len < 2 || (au[0] >> 5) != 4) return;                         /* no data stream element in front: no PAD */
    int n = au[1], o = 2;
    if (n == 255) {
        if (len < 3) {
            c.pad_malformed++;
            sink.drop_context();
            return;
        }
        n += au[2];
        o = 3;
    }
    if (n < 2 || o + n > len) {
        c.pad_malformed++;
        sink.drop_context();
        return;
    }
    const uint8_t *p = au + o;
    const uint8_t f0 = p[n - 2], f1 = p[n - 1];
    if ((f0 >> 6) != 0) return;
    const int ind = (f0 >> 4) & 3, ci = (f1 >> 1) & 1, avail = n - 2;
    if (ind == 0 || ind == 3) return;
    const uint8_t *x = p + n - 3;                                     /* logical byte i = x[-i], i < avail */
    /* the sub-fields of this field: 8 bits of length and 8 of type each, packed; they go to the sink from ONE place below */
    uint32_t lens = 0, types = 0;
    int count = 0, at = 0, last_after = -1;                           /* last_after: last_len behind the field; -1 = as it is */
    if (ind == 1) {
        if (avail < 4) {
            c.pad_malformed++;
            sink.drop_context();
            return;
        }
        if (ci) {
            types = x[0] & 0x1F;
            lens = 3;
            at = 1;
            last_after = 4;
        } else if (st.cont_type) {
            types = st.cont_type;
            lens = 4;
        } else {
            c.fields_ignored++;
            return;
        }
        count = 1;
    } else if (!ci) {
        if (!st.cont_type) {
            c.fields_ignored++;
            return;
        }
        types = st.cont_type;
        lens = uint32_t(st.last_len < avail ? st.last_len : avail);
        count = 1;
    } else {
        /* the list: up to four content indicators */
        int total = 0;
        bool bad = false;
        for (int k = 0; k < 4; k++) {
            if (at >= avail) {
                bad = true;
                break;
            }
            const uint8_t v = x[-at];
            at++;
            const int type = v & 0x1F;
            if (type == 0) break;
            if (type == 31) {
                if (at >= avail) {
                    bad = true;
                    break;
                }
                at++;                                                 /* the extended type: its sub-field is skipped */
            }
            const int l = subfield_length(v >> 5);
            lens |= uint32_t(l) << (8 * k);
            types |= uint32_t(type) << (8 * k);
            total += l;
            count++;
        }
        if (bad || at + total > avail) {
            c.pad_malformed++;
            sink.drop_context();
            return;
        }
        st.cont_type = 0;
        if (count) last_after = int((lens >> (8 * (count - 1))) & 0xFF);
    }
    for (int k = 0; k < count; k++) {
        const int l = (lens >> (8 * k)) & 0xFF, type = (types >> (8 * k)) & 0xFF;
        field(sink, type, x, at, l);
        at += l;
    }
    if (last_after >= 0) st.last_len = uint8_t(last_after);
    if (count) c.aus_with_xpad++;
}

/* the label's sink, and the walk under the name it has always had */
struct LabelSink {
    State &st;
    Counters &c;
    DABGPU_PAD_FN void drop_context() { dabgpu_pad::drop_context(st); }
    DABGPU_PAD_FN void subfield(int type, const uint8_t *xpad_end, int at, int len) { dabgpu_pad::subfield(st, c, type, xpad_end, at, len); }
};
DABGPU_PAD_FN void walk_au(State &st, Counters &c, const uint8_t *au, int len) {
    LabelSink k{st, c};
    walk_fields(k, au, len);
}

/* How many access units of a super-frame are visited: one, lost, when firecode_ok == 0 or num_aus <= 0 (how many it
 * carried is not known); else num_aus, at most 7.  au_span: access unit a of a data part of 110 s bytes, b = au_start[a],
 * e = au_start[a + 1] -> its length without the CRC and *begin, or -1 = lost. */
DABGPU_PAD_FN int visited_aus(int firecode_ok, int num_aus) { return !firecode_ok || num_aus <= 0 ? 1 : num_aus > 7 ? 7 : num_aus; }
DABGPU_PAD_FN int au_span(int firecode_ok, int num_aus, int au_crc_mask, int b, int e, int a, int s, int *begin) {
    if (!firecode_ok || num_aus <= 0 || !((au_crc_mask >> a) & 1)) return -1;
    if (!(b >= 0 && e <= 110 * s && b < e && e - b > 2)) return -1;
    *begin = b;
    return e - b - 2;
}

/* One entry of a call, on memory the caller can read: the twin of the kernel's loop.  status rows are 16 int32 words
 * {firecode_ok, rs_corrected, rs_uncorrectable, num_aus, au_crc_mask, au_start[8], reserved[3]}. */
DABGPU_PAD_FN void walk_superframes(State &st, Counters &c, const uint8_t *data, uint64_t data_stride, const int32_t *status,
                                    int n_superframes, int s) {
    for (int k = 0; k < n_superframes; k++) {
        const int32_t *row = status + 16 * int64_t(k);
        const int n = visited_aus(row[0], row[3]);
        for (int a = 0; a < n; a++) {
            int b = 0;
            const int len = au_span(row[0], row[3], row[4], row[5 + a], row[6 + a], a, s, &b);
            walk_au(st, c, data + uint64_t(k) * data_stride + (len < 0 ? 0 : b), len);
        }
    }
}

}  /* namespace dabgpu_pad */
#endif
