/* dabgpu_eti_read.h -- ETI(NI) byte streams read back into FIBs with CRC flags and logical frames per sub-channel.
 *
 * One implementation of the contract below: the kernels behind dabgpu_eti_read_dev (csrc/eti_read_kernels.hip), the host
 * twin dabgpu_eti_read_host and the host mirror's BasicRadio::ProcessEti all run these functions.  Plain C++17,
 * header-only, no table in memory; __host__ __device__ under hipcc.  A frame is reached through a byte accessor
 * g(i) = byte i of the frame, so the same checks run on a pointer, on a stream made of two pieces and on LDS.
 *
 * THE CONTRACT of one entry in one call.
 *
 * Stream.  S = the carried tail of the state (0 .. 6143 bytes; a tail length above 6143 counts as 6143) followed by the
 * entry's n_bytes new bytes.  At most max_frames = (6143 + n_bytes) / 6144 rows are emitted.
 *
 * Verdict of a position q with q + 6144 <= |S|: what dabgpu_eti_parse returns on S[q .. q + 6144) -- 0, BAD_SYNC 1,
 * BAD_HEADER 2, BAD_HEADER_CRC 3, BAD_DATA_CRC 4 -- or OTHER_PLAN 5 when it returns 0, a plan is given and NST, FL or an
 * STC word differs from the plan's.  q is a CANDIDATE when its verdict is 0, 4 or 5: everything up to the header CRC
 * holds (the first 12 + 4 NST bytes).
 *
 * Walk from p = 0, r = 0:
 *   1. p + 6144 > |S|: stop.
 *   2. p is a candidate: row r is position p; r++, p += 6144.
 *   3. otherwise q = the smallest candidate with p < q <= |S| - 6144.  If there is one: skipped += q - p, resyncs++,
 *      p = q.  If not: skipped += max(0, |S| - 6143 - p), p = max(p, |S| - 6143), stop.
 *   4. S[p ..) is the new tail.
 *
 * Row.  Verdict 0 = TAKEN: the 96 FIC bytes, the three FIB CRC flags (the FIC decoder's rule: CRC-16 x^16 + x^12 + x^5 + 1,
 * start all ones, complemented, over 30 bytes against the last two) and every wanted stream's 8 STL bytes leave.  Verdict
 * 4 or 5 keeps its place: FIC, flags and stream rows are zero.
 *
 * Status per row: offset in S, verdict, FCT, FP, ERR (the header's, for every verdict), fib_ok bits (0 unless taken),
 * gap = (FCT - (previous row's FCT + 1)) mod 250 with the previous row's FCT carried in the state and 0 for a stream's
 * first row, flags GAP (gap != 0), FP_BREAK (there is a previous row and FP is not its FP + 1 mod 8), ERR_FIELD
 * (ERR != 0xFF), FIB_CRC (taken and fib_ok != 7).
 *
 * State: a head of 80 bytes (tail length, whether there is a previous row, its FCT and FP, running totals) and 6144 tail
 * bytes, zero behind the tail.  All zero = a stream that starts.  A record this code did not write is read as it is: the
 * tail length clamped, have_prev != 0 = there is a previous row, last_fct and last_fp taken as the numbers they are; no
 * value makes a call read outside the record.
 */
#ifndef DABGPU_ETI_READ_H
#define DABGPU_ETI_READ_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DABGPU_ETI_FN __host__ __device__ inline
#else
#define DABGPU_ETI_FN inline
#endif

namespace dabgpu_eti_read {

constexpr int FRAME_BYTES = 6144;
constexpr int MAX_TAIL = FRAME_BYTES - 1;
constexpr int MAX_STREAMS = 64;
constexpr int FIC_BYTES = 96;
constexpr int MAX_HEADER_BYTES = 12 + 4 * MAX_STREAMS;

enum Verdict : int { TAKEN = 0, BAD_SYNC = 1, BAD_HEADER = 2, BAD_HEADER_CRC = 3, BAD_DATA_CRC = 4, OTHER_PLAN = 5 };
enum Flag : uint8_t { FLAG_GAP = 1, FLAG_FP_BREAK = 2, FLAG_ERR_FIELD = 4, FLAG_FIB_CRC = 8 };

struct Status {                           /* == dabgpu_eti_read_status */
    uint32_t offset;
    uint8_t verdict, fct, fp, err;
    uint8_t fib_ok, gap, flags, reserved;
    uint32_t reserved2;
};

struct Result {                           /* == dabgpu_eti_read_result */
    uint32_t rows, taken, bad_data_crc, other_plan;
    uint32_t skipped, resyncs, gap_sum, fib_errors;
    uint32_t tail_bytes, reserved[3];
};

struct Head {                             /* the first 80 bytes of a state record */
    uint32_t tail_bytes;
    uint8_t have_prev, last_fct, last_fp, reserved;
    uint64_t rows, taken, bad_data_crc, other_plan, skipped, resyncs, gap_sum, fib_errors;
    uint64_t reserved2;
};

constexpr int STATE_HEAD_BYTES = 80;
constexpr int STATE_BYTES = STATE_HEAD_BYTES + FRAME_BYTES;
static_assert(sizeof(Status) == 16 && sizeof(Result) == 48 && sizeof(Head) == STATE_HEAD_BYTES && STATE_BYTES % 16 == 0,
              "records of the ABI");

/* what a walk compares a frame's header with: NST, FL and the STC words of a dabgpu_eti_plan */
struct PlanKey {
    int32_t nst, fl;
    uint8_t stc[4 * MAX_STREAMS];
};

struct Fields {                           /* of a frame whose header holds */
    int32_t err, fct, fp, nst, fl;
    int32_t fic_offset;                   /* 12 + 4 nst */
    int32_t data_bytes;                   /* FIC + streams: what the data CRC covers */
};

DABGPU_ETI_FN uint32_t crc_byte(uint32_t crc, uint32_t b) {
    crc ^= b << 8;
    for (int i = 0; i < 8; i++) crc = (crc & 0x8000u) ? ((crc << 1) ^ 0x1021u) & 0xFFFFu : (crc << 1) & 0xFFFFu;
    return crc;
}

DABGPU_ETI_FN uint32_t clamp_tail(uint32_t tail_bytes) { return tail_bytes > uint32_t(MAX_TAIL) ? uint32_t(MAX_TAIL) : tail_bytes; }

/* FSYNC is one of the two patterns, the one FCT's parity asks for, and FCT counts below 250 (bytes 1 .. 4) */
DABGPU_ETI_FN bool sync_ok(uint32_t b1, uint32_t b2, uint32_t b3, uint32_t fct) {
    const bool even = b1 == 0x07 && b2 == 0x3A && b3 == 0xB6, odd = b1 == 0xF8 && b2 == 0xC5 && b3 == 0x49;
    return (even || odd) && odd == bool(fct & 1) && fct < 250;
}

/* 0 when the frame behind g is a candidate (f is filled), else BAD_SYNC / BAD_HEADER / BAD_HEADER_CRC.  Reads bytes
 * 0 .. 11 + 4 NST at most, and none behind byte 7 unless NST <= 64. */
template <class G> DABGPU_ETI_FN int header_verdict(G g, Fields &f) {
    if (!sync_ok(g(1), g(2), g(3), g(4))) return BAD_SYNC;
    const uint32_t b5 = g(5), b6 = g(6), b7 = g(7);
    const int nst = int(b5 & 0x7f), fl = int(((b6 & 7) << 8) | b7);
    if (!(b5 & 0x80) || ((b6 >> 3) & 3) != 1 || nst > MAX_STREAMS) return BAD_HEADER;
    uint32_t crc = 0xFFFFu;
    crc = crc_byte(crc_byte(crc_byte(crc_byte(crc, g(4)), b5), b6), b7);
    int stl_sum = 0;
    for (int k = 0; k < nst; k++) {
        const uint32_t s2 = g(10 + 4 * k), s3 = g(11 + 4 * k);
        stl_sum += int(((s2 & 3) << 8) | s3);
        crc = crc_byte(crc_byte(crc_byte(crc_byte(crc, g(8 + 4 * k)), g(9 + 4 * k)), s2), s3);
    }
    if (fl != nst + 1 + 24 + 2 * stl_sum || 4 * fl + 16 > FRAME_BYTES) return BAD_HEADER;
    const int at = 8 + 4 * nst;
    crc = crc_byte(crc_byte(crc, g(at)), g(at + 1)) ^ 0xFFFFu;
    if (crc != ((g(at + 2) << 8) | g(at + 3))) return BAD_HEADER_CRC;
    f.err = int(g(0));
    f.fct = int(g(4));
    f.fp = int(b6 >> 5);
    f.nst = nst;
    f.fl = fl;
    f.fic_offset = 12 + 4 * nst;
    f.data_bytes = FIC_BYTES + 8 * stl_sum;
    return TAKEN;
}

/* the fields of a frame header_verdict has passed already, from its first 8 bytes (FL stands for the STL sum) */
template <class G> DABGPU_ETI_FN void candidate_fields(G g, Fields &f) {
    const uint32_t b6 = g(6);
    f.err = int(g(0));
    f.fct = int(g(4));
    f.fp = int(b6 >> 5);
    f.nst = int(g(5) & 0x7f);
    f.fl = int(((b6 & 7) << 8) | g(7));
    f.fic_offset = 12 + 4 * f.nst;
    f.data_bytes = 4 * (f.fl - f.nst - 1);
}

/* a candidate's header against the plan's */
template <class G> DABGPU_ETI_FN bool plan_differs(G g, const Fields &f, const PlanKey &plan) {
    if (f.nst != plan.nst || f.fl != plan.fl) return true;
    for (int i = 0; i < 4 * f.nst; i++)
        if (g(8 + i) != plan.stc[i]) return true;
    return false;
}

/* the data CRC of a candidate, serially */
template <class G> DABGPU_ETI_FN bool data_crc_ok(G g, const Fields &f) {
    uint32_t crc = 0xFFFFu;
    for (int i = 0; i < f.data_bytes; i++) crc = crc_byte(crc, g(f.fic_offset + i));
    const int at = f.fic_offset + f.data_bytes;
    return (crc ^ 0xFFFFu) == ((g(at) << 8) | g(at + 1));
}

/* 1 when FIB j of the FIC passes its CRC */
template <class G> DABGPU_ETI_FN uint8_t fib_crc_ok(G g, const Fields &f, int j) {
    const int at = f.fic_offset + 32 * j;
    uint32_t crc = 0xFFFFu;
    for (int i = 0; i < 30; i++) crc = crc_byte(crc, g(at + i));
    return (crc ^ 0xFFFFu) == ((g(at + 30) << 8) | g(at + 31)) ? 1 : 0;
}

/* a row's record from its fields and the row before (prev_have = 0: a stream's first row) */
DABGPU_ETI_FN Status make_status(uint32_t offset, int verdict, const Fields &f, uint32_t fib_ok, bool prev_have, uint32_t prev_fct,
                                 uint32_t prev_fp) {
    Status st;
    st.offset = offset;
    st.verdict = uint8_t(verdict);
    st.fct = uint8_t(f.fct);
    st.fp = uint8_t(f.fp);
    st.err = uint8_t(f.err);
    st.fib_ok = uint8_t(verdict == TAKEN ? fib_ok : 0);
    const int gap = prev_have ? ((f.fct - int(prev_fct) - 1) % 250 + 250) % 250 : 0;
    st.gap = uint8_t(gap);
    st.flags = uint8_t((gap ? FLAG_GAP : 0) | (prev_have && uint32_t(f.fp) != ((prev_fp + 1) & 7) ? FLAG_FP_BREAK : 0) |
                       (f.err != 0xFF ? FLAG_ERR_FIELD : 0) | (verdict == TAKEN && st.fib_ok != 7 ? FLAG_FIB_CRC : 0));
    st.reserved = 0;
    st.reserved2 = 0;
    return st;
}

/* a row's share of the counters */
DABGPU_ETI_FN void count_row(Result &c, const Status &st) {
    c.rows++;
    c.taken += st.verdict == TAKEN;
    c.bad_data_crc += st.verdict == BAD_DATA_CRC;
    c.other_plan += st.verdict == OTHER_PLAN;
    c.gap_sum += st.gap;
    if (st.verdict == TAKEN) c.fib_errors += 3u - ((st.fib_ok & 1u) + ((st.fib_ok >> 1) & 1u) + ((st.fib_ok >> 2) & 1u));
}

/* the head of the next call's state */
DABGPU_ETI_FN Head next_head(const Head &in, const Result &c, bool have_last, uint32_t last_fct, uint32_t last_fp) {
    Head h = in;
    h.tail_bytes = c.tail_bytes;
    h.have_prev = uint8_t(have_last || in.have_prev ? 1 : 0);
    h.last_fct = uint8_t(have_last ? last_fct : in.last_fct);
    h.last_fp = uint8_t(have_last ? last_fp : in.last_fp);
    h.reserved = 0;
    h.rows += c.rows;
    h.taken += c.taken;
    h.bad_data_crc += c.bad_data_crc;
    h.other_plan += c.other_plan;
    h.skipped += c.skipped;
    h.resyncs += c.resyncs;
    h.gap_sum += c.gap_sum;
    h.fib_errors += c.fib_errors;
    h.reserved2 = 0;
    return h;
}

/* The serial walk over a contiguous S.  row(r, p, verdict, fields, frame accessor) is called for every emitted row in
 * order and returns the row's Status (the walk counts it); plan may be NULL.  Fills c (tail_bytes included) and returns
 * where the new tail begins. */
struct PtrFrame {
    const uint8_t *p;
    DABGPU_ETI_FN uint32_t operator()(int i) const { return p[i]; }
};

template <class Row> inline size_t walk(const uint8_t *s, size_t len, const PlanKey *plan, Result &c, Row row) {
    size_t p = 0;
    uint32_t r = 0;
    Fields f{};
    while (p + FRAME_BYTES <= len) {
        const PtrFrame g{s + p};
        if (header_verdict(g, f) == TAKEN) {
            int verdict = data_crc_ok(g, f) ? TAKEN : BAD_DATA_CRC;
            if (verdict == TAKEN && plan && plan_differs(g, f, *plan)) verdict = OTHER_PLAN;
            const Status st = row(r, uint32_t(p), verdict, f, g);
            count_row(c, st);
            r++;
            p += FRAME_BYTES;
            continue;
        }
        size_t q = p + 1;
        Fields fq{};
        while (q + FRAME_BYTES <= len && header_verdict(PtrFrame{s + q}, fq) != TAKEN) q++;
        if (q + FRAME_BYTES <= len) {
            c.skipped += uint32_t(q - p);
            c.resyncs++;
            p = q;
        } else {
            const size_t stop = len - MAX_TAIL;           /* len >= 6144 here */
            if (stop > p) {
                c.skipped += uint32_t(stop - p);
                p = stop;
            }
            break;
        }
    }
    c.tail_bytes = uint32_t(len - p);
    return p;
}

/* One entry on host pointers: what dabgpu_eti_read_host does per entry.  s / len: S already put together (the clamped
 * tail of state_in, then the new bytes).  out[k] (frame order, NULL = not wanted) takes bytes[k] per row from offset[k]
 * behind the FIC; with plan == NULL nothing but the FIC leaves.  state_out: STATE_BYTES, written whole. */
struct HostOut {
    uint8_t *fib, *crc_ok;
    Status *status;
    Result *result;
    uint8_t *const *out;                  /* [plan nst] in FRAME order, or NULL */
    const int32_t *offset, *bytes;        /* the plan's */
};

inline void read_entry(const uint8_t *s, size_t len, const Head &in, const PlanKey *plan, const HostOut &o, uint8_t *state_out) {
    Result c{};
    bool have = in.have_prev != 0;
    uint32_t fct = in.last_fct, fp = in.last_fp;
    bool any = false;
    const size_t p = walk(s, len, plan, c, [&](uint32_t r, uint32_t at, int verdict, const Fields &f, const PtrFrame &g) {
        uint32_t fib_ok = 0;
        uint8_t *fib = o.fib + size_t(r) * FIC_BYTES, *ok = o.crc_ok + size_t(r) * 3;
        for (int i = 0; i < FIC_BYTES; i++) fib[i] = verdict == TAKEN ? uint8_t(g(f.fic_offset + i)) : 0;
        for (int j = 0; j < 3; j++) {
            ok[j] = verdict == TAKEN ? fib_crc_ok(g, f, j) : 0;
            fib_ok |= uint32_t(ok[j]) << j;
        }
        if (plan && o.out)
            for (int k = 0; k < plan->nst; k++) {
                if (!o.out[k]) continue;
                uint8_t *d = o.out[k] + size_t(r) * size_t(o.bytes[k]);
                for (int i = 0; i < o.bytes[k]; i++) d[i] = verdict == TAKEN ? uint8_t(g(f.fic_offset + FIC_BYTES + o.offset[k] + i)) : 0;
            }
        const Status st = make_status(at, verdict, f, fib_ok, have, fct, fp);
        o.status[r] = st;
        have = any = true;
        fct = uint32_t(f.fct);
        fp = uint32_t(f.fp);
        return st;
    });
    *o.result = c;
    const Head h = next_head(in, c, any, fct, fp);
    const uint8_t *hb = reinterpret_cast<const uint8_t *>(&h);
    for (int i = 0; i < STATE_HEAD_BYTES; i++) state_out[i] = hb[i];
    for (size_t i = 0; i < size_t(FRAME_BYTES); i++) state_out[STATE_HEAD_BYTES + i] = i < len - p ? s[p + i] : 0;
}

}  // namespace dabgpu_eti_read
#endif
