/* dabgpu_fig.h -- what the FIBs of one ensemble announce, as the five listing calls of dabgpu.h report it.
 *
 * One implementation of the contracts that stand at dabgpu_fig_subchannels, dabgpu_fig_audio_components,
 * dabgpu_fig_packet_components, dabgpu_fig_user_applications and dabgpu_fig_stream_components in dabgpu.h (ETSI EN 300 401
 * clauses 5.2.2, 6.2 - 6.3): those five functions are their argument check and one call into here.  Plain C++17, header-only,
 * no HIP, host only; the bytes are untrusted and nothing outside [fib, fib + n_frames * 12 * 32) and
 * [crc_ok, crc_ok + n_frames * 12) is read, whatever they say (tests/fig_listing_fuzz.cpp).
 *
 *   for_each_fig0      the FIBs of a batch, FIG by FIG: the one place that knows how a FIB ends and what a FIG 0 header holds
 *   walk_0_1 ... _14   the entries of one FIG 0 body, decoded; each stops where the body cuts an entry off
 *   subchannels ...    the five listings: what each keeps, how many, in which order
 *
 * Every callable returns an int: 0 to go on, anything else ends the walk and is what the walk returns.
 */
#ifndef DABGPU_FIG_H
#define DABGPU_FIG_H

#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "dabgpu.h"

namespace dabgpu_fig {

constexpr int FIBS_PER_FRAME = 12, FIB_BYTES = 32, FIB_DATA_BYTES = 30;
constexpr int MAX_SUBCHANNELS = 64;    /* SubChId is 6 bits: the listings by sub-channel can never hold more */
constexpr int MAX_FOUND = 256;         /* what a listing by a wider key keeps: far more than 12 FIBs a frame announce */

/* Which FIG 0s a walk takes, as the bits of the header byte that must be clear. */
constexpr uint8_t CURRENT = 0x80;                /* C/N = 0 alone: dabgpu_fig_subchannels */
constexpr uint8_t CURRENT_THIS_ENSEMBLE = 0xC0;  /* C/N = 0 and OE = 0: the other four calls */

struct Fig0 {
    const uint8_t *b;          /* b[0]: the FIG 0 header; b[1 .. len - 1]: the body */
    int len;                   /* 1 .. 29 */
    int cn, oe, pd, ext;
};

/* f(Fig0) for every FIG of type 0 that passes `gate`, in the CRC-clean FIBs of the batch, in order.  A FIB ends at the
 * marker 0xFF, at a FIG of length 0 and at one that would run over the 30 data bytes. */
template <class F> int for_each_fig0(const uint8_t *fib, const uint8_t *crc_ok, int n_frames, uint8_t gate, F f) {
    for (int k = 0; k < n_frames * FIBS_PER_FRAME; k++) {
        if (!crc_ok[k]) continue;
        const uint8_t *d = fib + size_t(k) * FIB_BYTES;
        for (int i = 0; i < FIB_DATA_BYTES;) {
            if (d[i] == 0xFF) break;
            const int type = d[i] >> 5, len = d[i] & 0x1F;
            if (len == 0 || i + 1 + len > FIB_DATA_BYTES) break;
            const uint8_t *b = d + i + 1;
            i += 1 + len;
            if (type != 0 || (b[0] & gate)) continue;
            if (const int rc = f(Fig0{b, len, b[0] >> 7, (b[0] >> 6) & 1, (b[0] >> 5) & 1, b[0] & 0x1F})) return rc;
        }
    }
    return 0;
}

inline uint32_t sid_at(const Fig0 &g, int j) {             /* 16 bits, or 32 with P/D = 1 */
    uint32_t sid = 0;
    for (int q = 0; q < (g.pd ? 4 : 2); q++) sid = (sid << 8) | g.b[j + q];
    return sid;
}

/* FIG 0/1, sub-channel organisation (clause 6.2.1): SubChId (6), start address (10), then the short form -- 0, table switch
 * (1), table index (6) -- or the long form -- 1, option (3), protection level (2), size (10) */
struct Organisation {
    int id, start, long_form;
    int option, level, size;   /* long form; level 1 .. 4 */
    int table_switch, index;   /* short form */
};
template <class F> int walk_0_1(const Fig0 &g, F f) {
    const uint8_t *b = g.b;
    for (int j = 1; j + 3 <= g.len;) {
        Organisation e{};
        e.id = b[j] >> 2;
        e.start = ((b[j] & 3) << 8) | b[j + 1];
        e.long_form = b[j + 2] >> 7;
        if (e.long_form) {
            if (j + 4 > g.len) break;
            e.option = (b[j + 2] >> 4) & 7;
            e.level = ((b[j + 2] >> 2) & 3) + 1;
            e.size = ((b[j + 2] & 3) << 8) | b[j + 3];
            j += 4;
        } else {
            e.table_switch = (b[j + 2] >> 6) & 1;
            e.index = b[j + 2] & 0x3F;
            j += 3;
        }
        if (const int rc = f(e)) return rc;
    }
    return 0;
}
/* a long-form entry with a reserved option is not one a receiver can use: every listing passes it over */
inline bool usable(const Organisation &e) { return !e.long_form || e.option <= 1; }

/* FIG 0/2, service organisation (clause 6.3.1): SId, Rfa (1) CAId (3) NumComponents (4), then two bytes per component that
 * begin with TMId (2).  A service whose components the body does not hold ends the walk. */
struct Component {
    uint32_t sid;
    int tmid;
    uint8_t c0, c1;            /* the two bytes as sent: their layout depends on TMId */
    int subchid() const { return c1 >> 2; }                 /* TMId 0, 1 */
    int type() const { return c0 & 0x3F; }                  /* TMId 0: ASCTy; TMId 1: DSCTy */
    int scid() const { return ((c0 & 0x3F) << 6) | (c1 >> 2); }   /* TMId 3 */
    int primary() const { return (c1 >> 1) & 1; }
    int ca() const { return c1 & 1; }
};
template <class F> int walk_0_2(const Fig0 &g, F f) {
    const uint8_t *b = g.b;
    const int sid_bytes = g.pd ? 4 : 2;
    for (int j = 1; j + sid_bytes + 1 <= g.len;) {
        const uint32_t sid = sid_at(g, j);
        const int ncomp = b[j + sid_bytes] & 0x0F;
        j += sid_bytes + 1;
        if (j + 2 * ncomp > g.len) break;
        for (int c = 0; c < ncomp; c++, j += 2)
            if (const int rc = f(Component{sid, b[j] >> 6, b[j], b[j + 1]})) return rc;
    }
    return 0;
}

/* FIG 0/3, service component in packet mode (clause 6.3.2): SCId (12), Rfa (3), CAOrg flag (1), DG flag (1), Rfu (1),
 * DSCTy (6), SubChId (6), packet address (10), CAOrg (16) if flagged.  An entry whose CAOrg field is cut off ends the walk. */
struct PacketMode {
    int scid, subchid, address, dscty, dg_flag;
};
template <class F> int walk_0_3(const Fig0 &g, F f) {
    const uint8_t *b = g.b;
    for (int j = 1; j + 5 <= g.len;) {
        const PacketMode e = {(b[j] << 4) | (b[j + 1] >> 4), b[j + 3] >> 2, ((b[j + 3] & 3) << 8) | b[j + 4], b[j + 2] & 0x3F, b[j + 2] >> 7};
        j += 5 + 2 * (b[j + 1] & 1);
        if (j > g.len) break;
        if (const int rc = f(e)) return rc;
    }
    return 0;
}

/* FIG 0/8, service component global definition (clause 6.3.5): SId, Ext flag (1), Rfa (3), SCIdS (4), then L/S flag (1) and
 * the short form -- MSC/FIC flag (1), SubChId or FIDCId (6) -- or the long form -- Rfa (3), SCId (12) --, then Rfa (8) if Ext */
struct Global {
    uint32_t sid;
    int scids, long_form, id;
    bool fidc;                 /* short form with MSC/FIC flag 1: `id` is a FIDCId, not a sub-channel */
};
template <class F> int walk_0_8(const Fig0 &g, F f) {
    const uint8_t *b = g.b;
    const int sid_bytes = g.pd ? 4 : 2;
    for (int j = 1; j + sid_bytes + 2 <= g.len;) {
        Global e{};
        e.sid = sid_at(g, j);
        const int extended = b[j + sid_bytes] >> 7;
        e.scids = b[j + sid_bytes] & 0x0F;
        e.long_form = b[j + sid_bytes + 1] >> 7;
        j += sid_bytes + 1;
        if (j + (e.long_form ? 2 : 1) + extended > g.len) break;
        e.id = e.long_form ? ((b[j] & 0x0F) << 8) | b[j + 1] : b[j] & 0x3F;
        e.fidc = !e.long_form && (b[j] & 0x40);
        j += (e.long_form ? 2 : 1) + extended;
        if (const int rc = f(e)) return rc;
    }
    return 0;
}

/* FIG 0/13, user application information (clause 6.3.6): SId, SCIdS (4), number of applications (4), then per application
 * its type (11), data length (5) and data.  An application the body cuts off ends the walk. */
struct Application {
    uint32_t sid;
    int scids, ua_type, data_length;
    const uint8_t *data;
};
template <class F> int walk_0_13(const Fig0 &g, F f) {
    const uint8_t *b = g.b;
    const int sid_bytes = g.pd ? 4 : 2;
    for (int j = 1; j + sid_bytes + 1 <= g.len;) {
        const uint32_t sid = sid_at(g, j);
        const int scids = b[j + sid_bytes] >> 4, count = b[j + sid_bytes] & 0x0F;
        j += sid_bytes + 1;
        for (int a = 0; a < count; a++) {
            if (j + 2 > g.len) return 0;
            const int ua_type = (b[j] << 3) | (b[j + 1] >> 5), data_length = b[j + 1] & 0x1F;
            if (j + 2 + data_length > g.len) return 0;
            if (const int rc = f(Application{sid, scids, ua_type, data_length, b + j + 2})) return rc;
            j += 2 + data_length;
        }
    }
    return 0;
}

/* FIG 0/14, FEC sub-channel organisation (clause 6.2.2): SubChId (6), FEC scheme (2) */
template <class F> int walk_0_14(const Fig0 &g, F f) {
    for (int j = 1; j < g.len; j++)
        if (const int rc = f(g.b[j] >> 2, g.b[j] & 3)) return rc;
    return 0;
}

/* ---- what the listings share ---- */

/* SubChId -> start address, first announcement first (-1: not announced) */
struct StartAddresses {
    int of[MAX_SUBCHANNELS];
    StartAddresses() { std::fill(of, of + MAX_SUBCHANNELS, -1); }
    void note(const Fig0 &g) {
        walk_0_1(g, [&](const Organisation &e) {
            if (usable(e) && of[e.id] < 0) of[e.id] = e.start;
            return 0;
        });
    }
};

/* a list that keeps its first `CAP` entries, each key once */
template <class T, int CAP> struct FirstOf {
    T list[CAP];
    int n = 0;
    template <class Same> const T *find(Same same) const {
        for (int i = 0; i < n; i++)
            if (same(list[i])) return &list[i];
        return nullptr;
    }
    template <class Same> void add(const T &e, Same same) {
        if (!find(same) && n < CAP) list[n++] = e;
    }
};

/* the end of every listing: sorted (entries that compare equal stay in the order they were found), counted into *n, and
 * copied out if they fit -- DABGPU_ERR_CAPACITY leaves `out` as it was */
template <class T, class Less> int hand_over(T *found, int count, Less less, T *out, int max, int *n) {
    std::stable_sort(found, found + count, less);
    *n = count;
    if (count > max) return DABGPU_ERR_CAPACITY;
    std::copy(found, found + count, out);
    return DABGPU_OK;
}

/* the listings by sub-channel (audio: TMId 0, stream data: TMId 1): FIG 0/1 first, then FIG 0/2; each SubChId once, its first
 * component; one whose sub-channel is not announced is left out; sorted by start address.  make(Component, start) -> T */
template <class T, class Make> int components_by_subchannel(const uint8_t *fib, const uint8_t *crc_ok, int n_frames, int tmid, Make make, T *out,
                                                            int max, int *n) {
    StartAddresses start;
    for_each_fig0(fib, crc_ok, n_frames, CURRENT_THIS_ENSEMBLE, [&](const Fig0 &g) {
        if (g.ext == 1) start.note(g);
        return 0;
    });
    T found[MAX_SUBCHANNELS];
    bool seen[MAX_SUBCHANNELS] = {};
    int count = 0;
    for_each_fig0(fib, crc_ok, n_frames, CURRENT_THIS_ENSEMBLE, [&](const Fig0 &g) {
        if (g.ext != 2) return 0;
        return walk_0_2(g, [&](const Component &c) {
            if (c.tmid != tmid || seen[c.subchid()] || start.of[c.subchid()] < 0) return 0;
            seen[c.subchid()] = true;
            found[count++] = make(c, start.of[c.subchid()]);
            return 0;
        });
    });
    return hand_over(found, count, [](const T &a, const T &b) { return a.start_address < b.start_address; }, out, max, n);
}

/* ---- the five listings (arguments as checked by their callers in dabgpu.h) ---- */

/* dabgpu_fig_subchannels.  profile(Organisation, dabgpu_subchannel &) -> 0 and the descriptor, or the status the call returns
 * AT ONCE: it runs on the first usable entry of each SubChId, in the order the FIBs carry them. */
template <class Profile> int subchannels(const uint8_t *fib, const uint8_t *crc_ok, int n_frames, Profile profile, dabgpu_subchannel *out,
                                         int max, int *n) {
    dabgpu_subchannel found[MAX_SUBCHANNELS];
    bool seen[MAX_SUBCHANNELS] = {};
    int count = 0;
    const int rc = for_each_fig0(fib, crc_ok, n_frames, CURRENT, [&](const Fig0 &g) {
        if (g.ext != 1) return 0;
        return walk_0_1(g, [&](const Organisation &e) {
            if (!usable(e) || seen[e.id]) return 0;
            dabgpu_subchannel sc{};
            if (const int bad = profile(e, sc)) return bad;
            seen[e.id] = true;
            found[count++] = sc;
            return 0;
        });
    });
    if (rc) return rc;
    return hand_over(found, count, [](const dabgpu_subchannel &a, const dabgpu_subchannel &b) { return a.start_address < b.start_address; }, out,
                     max, n);
}

/* dabgpu_fig_audio_components: TMId 0 -- ASCTy (6), SubChId (6), P/S (1), CA flag (1) */
inline int audio_components(const uint8_t *fib, const uint8_t *crc_ok, int n_frames, dabgpu_audio_component *out, int max, int *n) {
    return components_by_subchannel(fib, crc_ok, n_frames, 0, [](const Component &c, int start) {
        dabgpu_audio_component a{};
        a.sid = c.sid;
        a.subchid = c.subchid();
        a.start_address = start;
        a.ascty = c.type();
        a.primary = c.primary();
        return a;
    }, out, max, n);
}

/* dabgpu_fig_stream_components: TMId 1 -- DSCTy (6), SubChId (6), P/S (1), CA flag (1) */
inline int stream_components(const uint8_t *fib, const uint8_t *crc_ok, int n_frames, dabgpu_stream_component *out, int max, int *n) {
    return components_by_subchannel(fib, crc_ok, n_frames, 1, [](const Component &c, int start) {
        dabgpu_stream_component a{};
        a.sid = c.sid;
        a.subchid = c.subchid();
        a.start_address = start;
        a.dscty = c.type();
        a.primary = c.primary();
        a.ca = c.ca();
        return a;
    }, out, max, n);
}

/* dabgpu_fig_packet_components: FIG 0/1 SubChId -> start address, FIG 0/3 SCId -> the packet-mode description (first one),
 * FIG 0/14 SubChId -> FEC scheme (first one) first; then FIG 0/2, the components with TMId 3 -- SCId (12), P/S (1), CA (1) --
 * each (sub-channel, packet address) once; sorted by (start address, packet address) */
inline int packet_components(const uint8_t *fib, const uint8_t *crc_ok, int n_frames, dabgpu_packet_component *out, int max, int *n) {
    StartAddresses start;
    FirstOf<PacketMode, MAX_FOUND> described;
    int fec_of[MAX_SUBCHANNELS] = {};
    bool fec_seen[MAX_SUBCHANNELS] = {};
    for_each_fig0(fib, crc_ok, n_frames, CURRENT_THIS_ENSEMBLE, [&](const Fig0 &g) {
        if (g.ext == 1) start.note(g);
        if (g.ext == 3) walk_0_3(g, [&](const PacketMode &e) {
            described.add(e, [&](const PacketMode &o) { return o.scid == e.scid; });
            return 0;
        });
        if (g.ext == 14) walk_0_14(g, [&](int id, int scheme) {
            if (!fec_seen[id]) fec_of[id] = scheme;
            fec_seen[id] = true;
            return 0;
        });
        return 0;
    });
    FirstOf<dabgpu_packet_component, MAX_FOUND> found;
    for_each_fig0(fib, crc_ok, n_frames, CURRENT_THIS_ENSEMBLE, [&](const Fig0 &g) {
        if (g.ext != 2) return 0;
        return walk_0_2(g, [&](const Component &c) {
            if (c.tmid != 3) return 0;
            const PacketMode *q = described.find([&](const PacketMode &o) { return o.scid == c.scid(); });
            if (!q || start.of[q->subchid] < 0) return 0;
            dabgpu_packet_component a{};
            a.sid = c.sid;
            a.scid = q->scid;
            a.subchid = q->subchid;
            a.start_address = start.of[q->subchid];
            a.packet_address = q->address;
            a.dscty = q->dscty;
            a.dg_flag = q->dg_flag;
            a.fec_scheme = fec_of[q->subchid];
            a.primary = c.primary();
            found.add(a, [&](const dabgpu_packet_component &o) { return o.subchid == a.subchid && o.packet_address == a.packet_address; });
            return 0;
        });
    });
    return hand_over(found.list, found.n, [](const dabgpu_packet_component &a, const dabgpu_packet_component &b) {
        return a.start_address != b.start_address ? a.start_address < b.start_address : a.packet_address < b.packet_address;
    }, out, max, n);
}

/* dabgpu_fig_user_applications: FIG 0/8 (SId, SCIdS) -> SubChId or SCId (first one; a FIDC is none), FIG 0/3 SCId -> (SubChId,
 * packet address) first; then FIG 0/13, each (SId, SCIdS, type) once, joined through them; sorted by (sid, scids, ua_type) */
inline int user_applications(const uint8_t *fib, const uint8_t *crc_ok, int n_frames, dabgpu_user_application *out, int max, int *n) {
    FirstOf<Global, MAX_FOUND> globals;
    FirstOf<PacketMode, MAX_FOUND> described;
    for_each_fig0(fib, crc_ok, n_frames, CURRENT_THIS_ENSEMBLE, [&](const Fig0 &g) {
        if (g.ext == 3) walk_0_3(g, [&](const PacketMode &e) {
            described.add(e, [&](const PacketMode &o) { return o.scid == e.scid; });
            return 0;
        });
        if (g.ext == 8) walk_0_8(g, [&](const Global &e) {
            if (!e.fidc) globals.add(e, [&](const Global &o) { return o.sid == e.sid && o.scids == e.scids; });
            return 0;
        });
        return 0;
    });
    FirstOf<dabgpu_user_application, MAX_FOUND> found;
    for_each_fig0(fib, crc_ok, n_frames, CURRENT_THIS_ENSEMBLE, [&](const Fig0 &g) {
        if (g.ext != 13) return 0;
        return walk_0_13(g, [&](const Application &e) {
            dabgpu_user_application u{};
            u.sid = e.sid;
            u.scids = e.scids;
            u.ua_type = e.ua_type;
            u.subchid = u.scid = u.packet_address = -1;
            u.data_length = e.data_length > 23 ? 23 : e.data_length;
            std::copy(e.data, e.data + u.data_length, u.data);
            if (const Global *gl = globals.find([&](const Global &o) { return o.sid == e.sid && o.scids == e.scids; })) {
                if (!gl->long_form) {
                    u.subchid = gl->id;
                } else {
                    u.tmid_packet = 1;
                    u.scid = gl->id;
                    if (const PacketMode *q = described.find([&](const PacketMode &o) { return o.scid == gl->id; })) {
                        u.subchid = q->subchid;
                        u.packet_address = q->address;
                    }
                }
            }
            found.add(u, [&](const dabgpu_user_application &o) { return o.sid == u.sid && o.scids == u.scids && o.ua_type == u.ua_type; });
            return 0;
        });
    });
    return hand_over(found.list, found.n, [](const dabgpu_user_application &a, const dabgpu_user_application &b) {
        if (a.sid != b.sid) return a.sid < b.sid;
        if (a.scids != b.scids) return a.scids < b.scids;
        return a.ua_type < b.ua_type;
    }, out, max, n);
}

}  // namespace dabgpu_fig

#endif
