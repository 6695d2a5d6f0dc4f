/* dabgpu_edi.h -- EDI (ETSI TS 102 693) over the AF layer of TS 102 821: ensembles written as AF packets and AF packet
 * byte streams read back into FIBs with CRC flags and logical frames per sub-channel.
 *
 * One implementation of the contract below: the kernel behind dabgpu_edi_frames_dev (csrc/edi_kernels.hip) lays a packet
 * out with prefix_byte / est_head_byte, the host calls dabgpu_edi_parse, dabgpu_edi_streams_from_packet and
 * dabgpu_edi_read_host run parse / walk / read_entry, and write_packet is the serial writer of host code that links
 * nothing.  Plain C++17, header-only, no table in memory; __host__ __device__ under hipcc.  A packet is reached through a
 * byte accessor g(i) = byte i of the packet, so the same checks run on a pointer, on a stream made of two pieces and on LDS.
 *
 * THE FORMAT, STATED AS KNOWN.  Neither specification was at hand when this was written and no other implementation was
 * compared against: parity with other EDI tools is not pinned (says how a user pins it).  One
 * line per field, so that a line can be corrected.  All integers are big-endian, bit fields MSB first.
 *
 * AF packet:
 *   2    SYNC = "AF"
 *   4    LEN = payload bytes
 *   2    SEQ, + 1 per packet modulo 65536
 *   1    AR: bit 7 CF = 1 (CRC used), bits 6..4 MAJ = 1, bits 3..0 MIN = 0.  Written 0x90; read: AR & 0xF0 == 0x90
 *   1    PT = 'T'
 *   LEN  payload: TAG items
 *   2    CRC over everything before it, by the FIB's rule: x^16 + x^12 + x^5 + 1, start all ones, complemented
 *
 * TAG item: a 4-byte name, a 4-byte length in BITS, the value of ceil(bits / 8) bytes.  Items follow one another from
 * payload byte 0 while at least 8 bytes remain; fewer than 8 remaining bytes are padding and are ignored.  An item whose
 * value would end behind the payload makes the packet MALFORMED.
 *
 * Items read and written:
 *   "*ptr"   64 bits: protocol "DETI" (4 bytes), major 0 (16 bits), minor 0 (16 bits).  Read: another length is malformed,
 *            another protocol makes the packet not a DETI packet, major and minor are not judged.
 *   "deti"   ATSTF(1) FICF(1) RFUDF(1) FCTH(5) FCT(8)
 *            STAT(8) MID(2) FP(3) RFA(2) RFU(1) MNSC(16)
 *            if ATSTF: UTCO(8) SECONDS(32) TSTA(24)
 *            if FICF:  96 FIC bytes
 *            if RFUDF: 3 bytes
 *            The CIF count is dlfc = 250 FCTH + FCT; FCTH > 19 or FCT > 249 is malformed.  The length must be exactly
 *            the 48 + 64 ATSTF + 768 FICF + 24 RFUDF bits the flags imply, else malformed (a deti shorter than 16 bits too).
 *   "est" n  (fourth byte of the name n = 1..64)  SCID(6) SAD(10) TPL(6) RFA(2), then 8 STL bytes of the sub-channel's
 *            data of this CIF.  The length is 24 + 64 STL bits: a length that is not, or an STL above 1023, is malformed.
 *            "est" with a fourth byte outside 1..64 is another name.
 *   Every other name is stepped over ("*dmy" included).
 *
 * A DETI PACKET is well formed, holds exactly one deti, its est numbers are exactly 1..N with none twice (N = 0: none; in
 * any order), and every "*ptr" it holds names "DETI".
 *
 * The writer writes "*ptr", "deti", then est1..estN in the plan's order (ascending SAD), ATSTF = RFUDF = 0, FICF = 1, STAT =
 * the byte the ETI writer puts into ERR, MID = 1, FP = dlfc mod 8, RFA = RFU = 0, MNSC = 0xFFFF, TPL as in the ETI frame's
 * STC, the payload zero-padded to a multiple of 8 bytes.  A plan's packet has one size:
 * 10 + pad8(126 + sum(11 + 8 STL)) + 2.
 *
 * THE CONTRACT of one entry of dabgpu_edi_read_host in one call.
 *
 * Stream.  S = the carried tail of the state (0 .. 8191 bytes; a tail length above 8191 counts as 8191) followed by the
 * entry's n_bytes new bytes.  MAX_PACKET = 8192 bytes, header and CRC included.
 *
 * H(q): q + 10 <= |S| and the ten bytes at q are a plausible header: "AF", 12 + LEN <= MAX_PACKET, AR & 0xF0 == 0x90,
 * PT == 'T'.   C(q): H(q), q + 12 + LEN <= |S| and the packet's CRC holds.
 *
 * Walk from p = 0:
 *   1. C(p): the packet is judged (below); p += 12 + LEN.
 *   2. otherwise q = the smallest position above p with C(q).  If there is one: skipped += q - p, resyncs++, p = q.
 *   3. if there is none: t = the smallest position >= p at which H holds and the packet is incomplete
 *      (t + 12 + LEN > |S|), or else max(p, |S| - 9).  skipped += t - p, S[t ..) is the new tail, stop.  The tail is below
 *      8192 bytes by construction.
 * A packet whose CRC fails is never stepped over by its own LEN (LEN may be the damaged field): its loss shows in the next
 * row's gap.  resyncs counts stretches of skipped bytes: a stretch that a call's end cuts (t > p in step 3) is counted by
 * the call that reaches its end (the state carries in_skip), so that a stream fed in pieces counts what one call counts.
 *
 * Judging a CRC-good packet.  SEQ_BREAK is settled first: there is a previous CRC-good packet (carried in the state) and SEQ
 * is not its SEQ + 1 modulo 65536.  Malformed: bad_tags++.  Well formed but not a DETI packet: not_deti++.  A DETI packet
 * while a plan is given whose est set (N, and per n: SCID, SAD, TPL, STL) differs from the plan's STC words: other_plan++.
 * None of these gives a row.  Otherwise the packet is row r (r counts from 0 in each call).  With no plan (DISCOVERY)
 * every DETI packet is a row and only FIC and status leave.
 *
 * Rows all fit: max_rows(n_bytes, plan) = (8191 + n_bytes) / m with m the smallest packet that can give a row: 12 + 14
 * (a deti without FIC and nothing else; "*ptr" is optional) in discovery and 12 + 14 + sum(11 + 8 STL) with a plan.
 *
 * Row: the 96 FIC bytes, or zero with NO_FIC when FICF = 0; the three FIB CRC flags computed here (zero without FIC; STAT
 * is reported, not trusted); every wanted stream's 8 STL bytes.
 *
 * Status per row (32 bytes): offset in S, packet length (12 + LEN), dlfc, SEQ, gap = (dlfc - (previous row's dlfc + 1))
 * mod 5000 with the previous row's dlfc carried in the state and 0 for a stream's first row, FP, STAT, MID, fib_ok bits,
 * UTCO / SECONDS / TSTA when ATSTF (else 0 / 0 / 0xFFFFFF), flags GAP (gap != 0), SEQ_BREAK, FP_MISMATCH (FP != dlfc mod 8),
 * STAT_FIELD (STAT != 0xFF), FIB_CRC (FIC present and fib_ok != 7), NO_FIC, TIME (ATSTF).
 *
 * Result per entry: rows, not_deti, bad_tags, other_plan, skipped, resyncs, gap sum, FIB errors, tail bytes.
 *
 * State: a head of 96 bytes (tail length, have_prev / last dlfc, have_seq / last SEQ, in_skip, running totals) and 8192 tail
 * bytes, zero behind the tail.  All zero = a stream that starts.  A record this code did not write is read as it is: the
 * tail length clamped, the three flags != 0 = set, last_dlfc taken modulo 5000; no value makes a call read outside the
 * record.
 */
#ifndef DABGPU_EDI_H
#define DABGPU_EDI_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DABGPU_EDI_FN __host__ __device__ inline
#else
#define DABGPU_EDI_FN inline
#endif

namespace dabgpu_edi {

constexpr int MAX_PACKET = 8192;
constexpr int MAX_TAIL = MAX_PACKET - 1;
constexpr int AF_HEADER_BYTES = 10;
constexpr int AF_OVERHEAD = 12;               /* header + CRC */
constexpr int MAX_STREAMS = 64;
constexpr int FIC_BYTES = 96;
constexpr int CIF_COUNTS = 5000;
constexpr int MIN_ROW_PACKET = AF_OVERHEAD + 8 + 6;   /* a deti item without FIC */
/* the writer's packet: AF header, "*ptr" item, the deti item up to its FIC | FIC | est items */
constexpr int W_PREFIX_BYTES = AF_HEADER_BYTES + 16 + 8 + 6;
constexpr int W_FIC_AT = W_PREFIX_BYTES;
constexpr int W_EST_AT = W_FIC_AT + FIC_BYTES;
constexpr int EST_HEAD_BYTES = 11;            /* name, length, SCID / SAD / TPL / RFA */

enum Verdict : int { DETI = 0, BAD_HEADER = 1, BAD_CRC = 2, BAD_TAGS = 3, NOT_DETI = 4, OTHER_PLAN = 5 };
enum Flag : uint8_t { FLAG_GAP = 1, FLAG_SEQ_BREAK = 2, FLAG_FP_MISMATCH = 4, FLAG_STAT_FIELD = 8, FLAG_FIB_CRC = 16, FLAG_NO_FIC = 32,
                      FLAG_TIME = 64 };

struct Status {                           /* == dabgpu_edi_read_status */
    uint32_t offset;
    uint16_t length, dlfc, seq, gap;
    uint8_t fp, stat, mid, fib_ok;
    uint8_t flags, utco, reserved_a, reserved_b;     /* (no arrays: a record lives in registers on the device) */
    uint32_t seconds, tsta, reserved2;
};

struct Result {                           /* == dabgpu_edi_read_result */
    uint32_t rows, not_deti, bad_tags, other_plan;
    uint32_t skipped, resyncs, gap_sum, fib_errors;
    uint32_t tail_bytes, reserved_a, reserved_b, reserved_c;
};

struct Head {                             /* the first 96 bytes of a state record */
    uint32_t tail_bytes;
    uint8_t have_prev, have_seq, in_skip, reserved;
    uint16_t last_dlfc, last_seq;
    uint32_t reserved1;
    uint64_t rows, not_deti, bad_tags, other_plan, skipped, resyncs, gap_sum, fib_errors;
    uint64_t reserved2, reserved3;
};

constexpr int STATE_HEAD_BYTES = 96;
constexpr int STATE_BYTES = STATE_HEAD_BYTES + MAX_PACKET;
static_assert(sizeof(Status) == 32 && sizeof(Result) == 48 && sizeof(Head) == STATE_HEAD_BYTES && STATE_BYTES % 16 == 0,
              "records of the ABI");

/* what a walk compares a packet's est set with: the STC words of a dabgpu_eti_plan (SCID:6 SAD:10 TPL:6 STL:10 each) */
struct PlanKey {
    int32_t nst;
    uint8_t stc[4 * MAX_STREAMS];
};

struct Fields {                           /* of a well-formed packet (parse) */
    int32_t len;                          /* payload bytes */
    int32_t seq;
    int32_t n_deti, n_ptr, n_est, n_other;
    int32_t atstf, ficf, rfudf, dlfc, stat, mid, fp, rfa, rfu, mnsc;
    int32_t utco, tsta;
    uint32_t seconds;
    int32_t fic_at;                       /* offset in the packet of the 96 FIC bytes, -1 without */
    uint8_t sstc[MAX_STREAMS][3];         /* by est number - 1: SCID / SAD / TPL / RFA as in the item */
    int16_t stl[MAX_STREAMS];             /* -1: that est is not there */
    int16_t data_at[MAX_STREAMS];         /* offset in the packet of its 8 STL bytes */
};

DABGPU_EDI_FN uint32_t crc_byte(uint32_t crc, uint32_t b) {
    crc ^= b << 8;
    for (int i = 0; i < 8; i++) crc = (crc & 0x8000u) ? ((crc << 1) ^ 0x1021u) & 0xFFFFu : (crc << 1) & 0xFFFFu;
    return crc;
}

DABGPU_EDI_FN uint32_t clamp_tail(uint32_t tail_bytes) { return tail_bytes > uint32_t(MAX_TAIL) ? uint32_t(MAX_TAIL) : tail_bytes; }
DABGPU_EDI_FN constexpr int pad8(int n) { return (n + 7) & ~7; }
/* the writer's packet for nst streams of data_bytes bytes per CIF together */
DABGPU_EDI_FN constexpr int packet_bytes(int nst, int data_bytes) {
    return AF_HEADER_BYTES + pad8(W_EST_AT - AF_HEADER_BYTES + EST_HEAD_BYTES * nst + data_bytes) + 2;
}
/* the smallest packet that gives a row under a plan of nst streams and data_bytes bytes per CIF (nst = data_bytes = 0: discovery) */
DABGPU_EDI_FN constexpr int min_row_packet(int nst, int data_bytes) { return MIN_ROW_PACKET + EST_HEAD_BYTES * nst + data_bytes; }
DABGPU_EDI_FN uint32_t max_rows(uint32_t n_bytes, int nst, int data_bytes) {
    return uint32_t((uint64_t(MAX_TAIL) + n_bytes) / uint64_t(min_row_packet(nst, data_bytes)));
}

template <class G> DABGPU_EDI_FN uint32_t be16(G g, int at) { return (g(at) << 8) | g(at + 1); }
template <class G> DABGPU_EDI_FN uint32_t be32(G g, int at) { return (g(at) << 24) | (g(at + 1) << 16) | (g(at + 2) << 8) | g(at + 3); }

/* H: the ten bytes behind g are a plausible header; total = 12 + LEN */
template <class G> DABGPU_EDI_FN bool header_ok(G g, int &total) {
    if (g(0) != 'A' || g(1) != 'F' || (g(8) & 0xF0u) != 0x90u || g(9) != 'T') return false;
    const uint32_t len = be32(g, 2);
    if (len > uint32_t(MAX_PACKET - AF_OVERHEAD)) return false;
    total = int(len) + AF_OVERHEAD;
    return true;
}

/* the CRC of a packet of `total` bytes, serially */
template <class G> DABGPU_EDI_FN bool crc_ok(G g, int total) {
    uint32_t crc = 0xFFFFu;
    for (int i = 0; i < total - 2; i++) crc = crc_byte(crc, g(i));
    return (crc ^ 0xFFFFu) == be16(g, total - 2);
}

/* The TAG walk and the deti / est parse of a packet whose header and CRC hold: DETI, NOT_DETI or BAD_TAGS.  f is filled
 * as far as the items go (all of it for DETI and NOT_DETI).  Reads bytes 0 .. total - 3 only. */
template <class G> DABGPU_EDI_FN int parse(G g, int total, Fields &f) {
    f.len = total - AF_OVERHEAD;
    f.seq = int(be16(g, 6));
    f.n_deti = f.n_ptr = f.n_est = f.n_other = 0;
    f.atstf = f.ficf = f.rfudf = f.dlfc = f.stat = f.mid = f.fp = f.rfa = f.rfu = f.mnsc = 0;
    f.utco = 0;
    f.seconds = 0;
    f.tsta = 0xFFFFFF;
    f.fic_at = -1;
    for (int k = 0; k < MAX_STREAMS; k++) {
        f.stl[k] = -1;
        f.data_at[k] = 0;
        f.sstc[k][0] = f.sstc[k][1] = f.sstc[k][2] = 0;
    }
    bool foreign_ptr = false, est_twice = false;
    const int end = AF_HEADER_BYTES + f.len;
    int at = AF_HEADER_BYTES;
    while (end - at >= 8) {
        const uint32_t n0 = g(at), n1 = g(at + 1), n2 = g(at + 2), n3 = g(at + 3);
        const uint32_t bits = be32(g, at + 4);
        const uint32_t bytes = bits / 8 + (bits % 8 ? 1u : 0u);
        const int v = at + 8;
        if (bytes > uint32_t(end - v)) return BAD_TAGS;
        if (n0 == '*' && n1 == 'p' && n2 == 't' && n3 == 'r') {
            if (bits != 64) return BAD_TAGS;
            f.n_ptr++;
            if (g(v) != 'D' || g(v + 1) != 'E' || g(v + 2) != 'T' || g(v + 3) != 'I') foreign_ptr = true;
        } else if (n0 == 'd' && n1 == 'e' && n2 == 't' && n3 == 'i') {
            if (bits < 16) return BAD_TAGS;
            const uint32_t b0 = g(v), fct = g(v + 1);
            const int atstf = int(b0 >> 7), ficf = int((b0 >> 6) & 1), rfudf = int((b0 >> 5) & 1), fcth = int(b0 & 31);
            if (bits != uint32_t(48 + 64 * atstf + 768 * ficf + 24 * rfudf) || fcth > 19 || fct > 249) return BAD_TAGS;
            if (f.n_deti++ == 0) {
                f.atstf = atstf;
                f.ficf = ficf;
                f.rfudf = rfudf;
                f.dlfc = 250 * fcth + int(fct);
                f.stat = int(g(v + 2));
                const uint32_t b3 = g(v + 3);
                f.mid = int(b3 >> 6);
                f.fp = int((b3 >> 3) & 7);
                f.rfa = int((b3 >> 1) & 3);
                f.rfu = int(b3 & 1);
                f.mnsc = int(be16(g, v + 4));
                int w = v + 6;
                if (atstf) {
                    f.utco = int(g(w));
                    f.seconds = be32(g, w + 1);
                    f.tsta = int((g(w + 5) << 16) | (g(w + 6) << 8) | g(w + 7));
                    w += 8;
                }
                if (ficf) f.fic_at = w;
            }
        } else if (n0 == 'e' && n1 == 's' && n2 == 't' && n3 >= 1 && n3 <= uint32_t(MAX_STREAMS)) {
            if (bits < 24 || (bits - 24) % 64 || (bits - 24) / 64 > 1023) return BAD_TAGS;
            const int k = int(n3) - 1;
            if (f.stl[k] >= 0) {
                est_twice = true;
            } else {
                f.n_est++;
                f.stl[k] = int16_t((bits - 24) / 64);
                f.data_at[k] = int16_t(v + 3);
                f.sstc[k][0] = uint8_t(g(v));
                f.sstc[k][1] = uint8_t(g(v + 1));
                f.sstc[k][2] = uint8_t(g(v + 2));
            }
        } else {
            f.n_other++;
        }
        at = v + int(bytes);
    }
    if (f.n_deti != 1 || foreign_ptr || est_twice) return NOT_DETI;
    for (int k = 0; k < f.n_est; k++)
        if (f.stl[k] < 0) return NOT_DETI;          /* a hole: some number above n_est is there instead */
    return DETI;
}

/* a DETI packet's est set against the plan's STC words */
DABGPU_EDI_FN bool plan_differs(const Fields &f, const PlanKey &plan) {
    if (f.n_est != plan.nst) return true;
    for (int k = 0; k < f.n_est; k++) {
        const uint8_t *stc = plan.stc + 4 * k;
        if (f.sstc[k][0] != stc[0] || f.sstc[k][1] != stc[1] || (f.sstc[k][2] & 0xFCu) != (stc[2] & 0xFCu) ||
            int(f.stl[k]) != (((stc[2] & 3) << 8) | stc[3]))
            return true;
    }
    return false;
}

/* 1 when FIB j of the FIC at fic_at passes its CRC */
template <class G> DABGPU_EDI_FN uint8_t fib_crc_ok(G g, int fic_at, int j) {
    const int at = fic_at + 32 * j;
    uint32_t crc = 0xFFFFu;
    for (int i = 0; i < 30; i++) crc = crc_byte(crc, g(at + i));
    return (crc ^ 0xFFFFu) == be16(g, at + 30) ? 1 : 0;
}

/* what a walk carries from packet to packet, in a call and between calls */
struct Carry {
    bool have_prev, have_seq, in_skip;
    uint32_t last_dlfc, last_seq;
};

DABGPU_EDI_FN Carry carry_of(const Head &h) {
    Carry c;
    c.have_prev = h.have_prev != 0;
    c.have_seq = h.have_seq != 0;
    c.in_skip = h.in_skip != 0;
    c.last_dlfc = uint32_t(h.last_dlfc) % uint32_t(CIF_COUNTS);
    c.last_seq = h.last_seq;
    return c;
}

/* a row's record from its fields and what came before it */
DABGPU_EDI_FN Status make_status(uint32_t offset, int total, const Fields &f, uint32_t fib_ok, bool seq_break, const Carry &c) {
    Status st;
    st.offset = offset;
    st.length = uint16_t(total);
    st.dlfc = uint16_t(f.dlfc);
    st.seq = uint16_t(f.seq);
    const int gap = c.have_prev ? ((f.dlfc - int(c.last_dlfc) - 1) % CIF_COUNTS + CIF_COUNTS) % CIF_COUNTS : 0;
    st.gap = uint16_t(gap);
    st.fp = uint8_t(f.fp);
    st.stat = uint8_t(f.stat);
    st.mid = uint8_t(f.mid);
    st.fib_ok = uint8_t(f.ficf ? fib_ok : 0);
    st.flags = uint8_t((gap ? FLAG_GAP : 0) | (seq_break ? FLAG_SEQ_BREAK : 0) | (f.fp != (f.dlfc & 7) ? FLAG_FP_MISMATCH : 0) |
                       (f.stat != 0xFF ? FLAG_STAT_FIELD : 0) | (f.ficf && st.fib_ok != 7 ? FLAG_FIB_CRC : 0) |
                       (f.ficf ? 0 : FLAG_NO_FIC) | (f.atstf ? FLAG_TIME : 0));
    st.utco = uint8_t(f.utco);
    st.reserved_a = st.reserved_b = 0;
    st.seconds = f.seconds;
    st.tsta = uint32_t(f.tsta);
    st.reserved2 = 0;
    return st;
}

/* a row's share of the counters */
DABGPU_EDI_FN void count_row(Result &c, const Status &st) {
    c.rows++;
    c.gap_sum += st.gap;
    if (!(st.flags & FLAG_NO_FIC)) c.fib_errors += 3u - ((st.fib_ok & 1u) + ((st.fib_ok >> 1) & 1u) + ((st.fib_ok >> 2) & 1u));
}

/* the head of the next call's state */
DABGPU_EDI_FN Head next_head(const Head &in, const Result &c, const Carry &k) {
    Head h = in;
    h.tail_bytes = c.tail_bytes;
    h.have_prev = k.have_prev ? 1 : 0;
    h.have_seq = k.have_seq ? 1 : 0;
    h.in_skip = k.in_skip ? 1 : 0;
    h.reserved = 0;
    h.last_dlfc = uint16_t(k.last_dlfc);
    h.last_seq = uint16_t(k.last_seq);
    h.reserved1 = 0;
    h.rows += c.rows;
    h.not_deti += c.not_deti;
    h.bad_tags += c.bad_tags;
    h.other_plan += c.other_plan;
    h.skipped += c.skipped;
    h.resyncs += c.resyncs;
    h.gap_sum += c.gap_sum;
    h.fib_errors += c.fib_errors;
    h.reserved2 = h.reserved3 = 0;
    return h;
}

struct PtrPacket {
    const uint8_t *p;
    DABGPU_EDI_FN uint32_t operator()(int i) const { return p[i]; }
};

/* C(q) on a contiguous S; total is set when it holds */
inline bool good_at(const uint8_t *s, size_t len, size_t q, int &total) {
    if (q + AF_HEADER_BYTES > len) return false;
    const PtrPacket g{s + q};
    return header_ok(g, total) && q + size_t(total) <= len && crc_ok(g, total);
}

/* The serial walk over a contiguous S.  row(r, p, total, fields, seq_break, carry, packet accessor) is called for every row
 * in order and returns the row's Status (the walk counts it); plan may be NULL.  k: the carry, in and out.  f: room for one
 * packet's fields.  Fills c (tail_bytes included) and returns where the new tail begins. */
template <class Row> inline size_t walk(const uint8_t *s, size_t len, const PlanKey *plan, Carry &k, Result &c, Fields &f, Row row) {
    size_t p = 0;
    uint32_t r = 0;
    for (;;) {
        int total = 0;
        if (!good_at(s, len, p, total)) {
            size_t q = p + 1;
            while (q + AF_HEADER_BYTES <= len && !good_at(s, len, q, total)) q++;
            if (q + AF_HEADER_BYTES > len) {
                size_t t = p;
                int tt = 0;
                while (t + AF_HEADER_BYTES <= len && !(header_ok(PtrPacket{s + t}, tt) && t + size_t(tt) > len)) t++;
                if (t + AF_HEADER_BYTES > len) t = len >= 9 && len - 9 > p ? len - 9 : p;
                if (t > p) {
                    c.skipped += uint32_t(t - p);
                    k.in_skip = true;
                }
                p = t;
                break;
            }
            c.skipped += uint32_t(q - p);
            p = q;
            k.in_skip = true;
        }
        if (k.in_skip) {
            c.resyncs++;
            k.in_skip = false;
        }
        const PtrPacket g{s + p};
        const uint32_t seq = be16(g, 6);
        const bool seq_break = k.have_seq && seq != ((k.last_seq + 1) & 0xFFFFu);
        k.have_seq = true;
        k.last_seq = seq;
        const int verdict = parse(g, total, f);
        if (verdict == BAD_TAGS) c.bad_tags++;
        else if (verdict == NOT_DETI) c.not_deti++;
        else if (plan && plan_differs(f, *plan)) c.other_plan++;
        else {
            const Status st = row(r, uint32_t(p), total, f, seq_break, k, g);
            count_row(c, st);
            k.have_prev = true;
            k.last_dlfc = uint32_t(f.dlfc);
            r++;
        }
        p += size_t(total);
    }
    c.tail_bytes = uint32_t(len - p);
    return p;
}

/* One entry on host pointers: what dabgpu_edi_read_host does per entry.  s / len: S already put together (the clamped
 * tail of state_in, then the new bytes).  out[k] (est k + 1, NULL = not wanted) takes 8 STL bytes per row; with
 * plan == NULL nothing but the FIC leaves.  state_out: STATE_BYTES, written whole. */
struct HostOut {
    uint8_t *fib, *crc_ok;
    Status *status;
    Result *result;
    uint8_t *const *out;                  /* [plan nst] in the PLAN's order, or NULL */
};

inline void read_entry(const uint8_t *s, size_t len, const Head &in, const PlanKey *plan, const HostOut &o, uint8_t *state_out) {
    Result c{};
    Carry k = carry_of(in);
    Fields f;
    const size_t p = walk(s, len, plan, k, c, f, [&](uint32_t r, uint32_t at, int total, const Fields &ff, bool seq_break, const Carry &kk,
                                                      const PtrPacket &g) {
        uint32_t fib_ok = 0;
        uint8_t *fib = o.fib + size_t(r) * FIC_BYTES, *ok = o.crc_ok + size_t(r) * 3;
        for (int i = 0; i < FIC_BYTES; i++) fib[i] = ff.ficf ? uint8_t(g(ff.fic_at + i)) : 0;
        for (int j = 0; j < 3; j++) {
            ok[j] = ff.ficf ? fib_crc_ok(g, ff.fic_at, j) : 0;
            fib_ok |= uint32_t(ok[j]) << j;
        }
        if (plan && o.out)
            for (int n = 0; n < plan->nst; n++) {
                if (!o.out[n]) continue;
                const int bytes = 8 * int(ff.stl[n]);
                uint8_t *d = o.out[n] + size_t(r) * size_t(bytes);
                for (int i = 0; i < bytes; i++) d[i] = uint8_t(g(ff.data_at[n] + i));
            }
        const Status st = make_status(at, total, ff, fib_ok, seq_break, kk);
        o.status[r] = st;
        return st;
    });
    *o.result = c;
    const Head h = next_head(in, c, k);
    const uint8_t *hb = reinterpret_cast<const uint8_t *>(&h);
    for (int i = 0; i < STATE_HEAD_BYTES; i++) state_out[i] = hb[i];
    for (size_t i = 0; i < size_t(MAX_PACKET); i++) state_out[STATE_HEAD_BYTES + i] = i < len - p ? s[p + i] : 0;
}

/* ---- the writer's packet ---------------------------------------------------------------------------------------------- */

/* byte i (0 .. W_PREFIX_BYTES - 1) of the writer's packet: the AF header, the "*ptr" item and the deti item up to its FIC.
 * len: the payload's bytes; stat: the ETI writer's ERR byte */
DABGPU_EDI_FN uint32_t prefix_byte(int i, uint32_t len, uint32_t seq, uint32_t dlfc, uint32_t stat) {
    switch (i) {
    case 0: return 'A';
    case 1: return 'F';
    case 2: return (len >> 24) & 0xFFu;
    case 3: return (len >> 16) & 0xFFu;
    case 4: return (len >> 8) & 0xFFu;
    case 5: return len & 0xFFu;
    case 6: return (seq >> 8) & 0xFFu;
    case 7: return seq & 0xFFu;
    case 8: return 0x90u;                          /* CF = 1, MAJ = 1, MIN = 0 */
    case 9: return 'T';
    case 10: return '*';
    case 11: return 'p';
    case 12: return 't';
    case 13: return 'r';
    case 17: return 64;                            /* bits */
    case 18: return 'D';
    case 19: return 'E';
    case 20: return 'T';
    case 21: return 'I';
    case 26: return 'd';
    case 27: return 'e';
    case 28: return 't';
    case 29: return 'i';
    case 32: return (48u + 768u) >> 8;             /* bits: the fixed fields and the FIC */
    case 33: return (48u + 768u) & 0xFFu;
    case 34: return 0x40u | (dlfc / 250u);         /* ATSTF = 0, FICF = 1, RFUDF = 0, FCTH */
    case 35: return dlfc % 250u;                   /* FCT */
    case 36: return stat & 0xFFu;
    case 37: return 0x40u | ((dlfc & 7u) << 3);    /* MID = 1, FP, RFA = RFU = 0 */
    case 38: return 0xFFu;                         /* MNSC */
    case 39: return 0xFFu;
    default: return 0;                             /* lengths' upper bytes, major and minor */
    }
}

/* byte i (0 .. 10) of the head of est item n (1 ..): the name, 24 + 64 STL bits, SCID / SAD / TPL from the STC word */
DABGPU_EDI_FN uint32_t est_head_byte(int i, int n, const uint8_t *stc) {
    const uint32_t stl = ((uint32_t(stc[2]) & 3u) << 8) | stc[3], bits = 24u + 64u * stl;
    switch (i) {
    case 0: return 'e';
    case 1: return 's';
    case 2: return 't';
    case 3: return uint32_t(n);
    case 4: return 0;
    case 5: return (bits >> 16) & 0xFFu;
    case 6: return (bits >> 8) & 0xFFu;
    case 7: return bits & 0xFFu;
    case 8: return stc[0];
    case 9: return stc[1];
    default: return stc[2] & 0xFCu;                /* RFA = 0 */
    }
}

/* One packet, serially: put(i, byte) for every byte 0 .. packet_bytes - 1 in order.  fic(i): the 96 FIC bytes; data(k, i):
 * byte i of the plan's stream k of this CIF.  Returns the packet's bytes. */
template <class Put, class Fic, class Data>
inline int write_packet(Put put, const PlanKey &plan, uint32_t seq, uint32_t dlfc, uint32_t stat, Fic fic, Data data) {
    int data_bytes = 0;
    for (int k = 0; k < plan.nst; k++) data_bytes += 8 * (((plan.stc[4 * k + 2] & 3) << 8) | plan.stc[4 * k + 3]);
    const int total = packet_bytes(plan.nst, data_bytes);
    uint32_t crc = 0xFFFFu;
    int at = 0;
    const auto emit = [&](uint32_t b) {
        crc = crc_byte(crc, b & 0xFFu);
        put(at++, uint8_t(b));
    };
    for (int i = 0; i < W_PREFIX_BYTES; i++) emit(prefix_byte(i, uint32_t(total - AF_OVERHEAD), seq, dlfc, stat));
    for (int i = 0; i < FIC_BYTES; i++) emit(fic(i));
    for (int k = 0; k < plan.nst; k++) {
        const uint8_t *stc = plan.stc + 4 * k;
        for (int i = 0; i < EST_HEAD_BYTES; i++) emit(est_head_byte(i, k + 1, stc));
        const int bytes = 8 * (((stc[2] & 3) << 8) | stc[3]);
        for (int i = 0; i < bytes; i++) emit(data(k, i));
    }
    while (at < total - 2) emit(0);
    const uint32_t c = crc ^ 0xFFFFu;
    put(at++, uint8_t(c >> 8));
    put(at++, uint8_t(c & 0xFFu));
    return total;
}

}  // namespace dabgpu_edi
#endif
