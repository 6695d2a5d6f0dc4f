/* dabgpu_packet_fec.h -- Reed-Solomon RS(204,188) correction of the FEC frames of a packet-mode sub-channel (EN 300 401
 * clause 5.3.5), on its logical frames, in front of the packet scan of dabgpu_packet_walk.h.
 *
 * One implementation of the contract below: the kernels behind dabgpu_packet_fec_dev, the host twin dabgpu_packet_fec_host
 * and the host mirror's Basic_Data_Packet_Channel all run this code.  Plain C++17, header-only, no allocation;
 * __host__ __device__ under hipcc.  The one table (GF(2^8) exp / log, 768 bytes) is made by the compiler (make_gf()) and
 * handed in by the caller: a constant on the host, a copy in LDS on the device.
 *
 * THE CONTRACT of one entry (a sub-channel) in one call, every ambiguity decided.  Where this text and the standard's wording
 * could part, this text governs.
 *
 * Slots.  A sub-channel of bit rate R kbit/s has S = R / 8 slots of 24 bytes per logical frame.  The slots of a stream are
 * numbered g = 0, 1, ... from a fresh start, across frames and calls.
 *
 * FEC frame.  103 consecutive slots.  The first 94 are the application data table, 2256 bytes A[0..2255] in stream order;
 * the last 9 are FEC packets.  A slot with header bytes h0 h1 is MARK c when (h0 >> 6) == 0 and
 * (((h0 & 3) << 8) | h1) == 1022 and c = (h0 >> 2) & 15 is at most 8.  P[0..197] is bytes 2..23 of the nine FEC packets,
 * concatenated: P[0..191] is the RS data table, P[192..197] is ignored.  Row r (0..11) is the codeword
 * cw_r[c] = A[12 c + r] for c < 188 and cw_r[188 + j] = P[12 j + r] for j < 16 (both tables are filled column by column).
 * GF(2^8), x^8 + x^4 + x^3 + x^2 + 1, alpha = 2; generator prod_{i=0..15} (x + alpha^i); cw_r[0] is the coefficient of
 * x^203: RS(255,239) shortened by 51 leading zeros.  S_k = sum_c cw_r[c] alpha^(k (203 - c)), k = 0..15 -- the conventions
 * of the DAB+ super-frame's RS(120,110), with 16 syndromes instead of 10.
 *
 * Finding frames.  No phase is assumed and no lock is kept.  A frame ENDS at slot q when at least 7 of the slots q - 8 + i
 * (i = 0..8) are mark i; slots before the fresh start are no mark.  (7 of 9: two damaged FEC headers are tolerated; a third
 * lost FEC packet would by itself put about 6 errors into every row's parity.  Seven 16-bit coincidences do not happen in
 * noise.)  Marks are taken from the bytes as received, whatever a correction made of them later.  Candidates are taken in
 * ascending q.  One whose first slot q - 102 is below 0 is counted as frames_cut; else one whose first slot is at or before the
 * end of the last accepted frame is counted as frames_overlapping; neither is processed.  Every other candidate is accepted
 * (frames++), becomes the last accepted frame and is processed in the call in which its last slot arrives.
 *
 * Correction.  Bounded-distance decoding, errors only, per row.  If a codeword exists within Hamming distance 8 of the
 * received 204 bytes (every differing position inside the 204; such a codeword is unique), the row's 188 data bytes are
 * replaced by that codeword's: rows_corrected++, bytes_corrected += the differing data positions (c < 188),
 * parity_bytes_corrected += the others.  A row that is a codeword: rows_clean++.  Otherwise the row stays as received and
 * rows_uncorrectable++.  The FEC packets themselves are written out as received.
 *   How: Berlekamp-Massey on the 16 syndromes, the roots of the locator among the 204 positions, Forney's values -- and then
 *   the pattern is held to the definition (as many roots as the locator's degree, at most 8, no zero value, and the pattern's
 *   own 16 syndromes equal the received word's), so what is applied is a codeword within distance 8 and nothing else is.
 *
 * Delay.  An FEC frame is complete 102 slots after its first slot, so output lags input by a fixed D = ceil(102 / S) frames
 * (102 at 8 kbit/s, 2 at 512 kbit/s).  Output frame f of a call is stream frame F0 + f - D, F0 the frames seen since the
 * fresh start.  Stream frames below 0 are S copies of one padding packet: address 0, one slot, first and last set, 19 zero
 * data bytes and a correct CRC (0C 00 00, 19 x 00, CRC; the packet scan counts it as packets_padding).
 *
 * The state record is opaque: a 64-byte head (F0, the end of the last accepted frame, the marks of the last 8 slots as
 * received) and the last D frames, already corrected where their FEC frame has ended; state_bytes(S) of it, at most 3664.
 * A fresh start: no record (NULL), all zero, or a record this code did not write for this bit rate (head_ok()).  The result
 * of a stream does not depend on where it is cut into calls, calls of fewer than D frames and of none included.
 *
 * Counters of a call: cifs = n_cifs, slots = n_cifs S, marks = the marks among them.
 *
 * ERASURES.  A second pair of calls, dabgpu_packet_fec_erasures_dev / _host, beside the pair above, which stays as it is; the
 * code is include/dabgpu_packet_fec_erasures.h (process_erasures, the twin of process).  Everything above holds for it --
 * slots, FEC frames, marks, finding frames, delay, padding, the counters of a call -- with these additions.
 *
 * Suspect slots.  Each logical frame is scanned once, when it arrives, on its bytes as received, exactly like the marks.  The
 * scan is that of dabgpu_packet_walk.h, steps 1 - 4, with fec non-zero.  A slot is SUSPECT when that scan counts it as
 * slots_bad (steps 2 and 3: a length that does not fit the frame, a packet CRC that does not check).  A slot covered by a good
 * packet is not suspect; a slot taken as an FEC packet is not suspect.  Packets do not straddle logical frames, so the result
 * does not depend on how the stream is cut into calls.  Padding frames below stream frame 0 have no suspect slot.
 *
 * Erased columns.  For an accepted FEC frame, suspect slot i (0..93) of its data table erases columns 2i and 2i + 1 of every
 * row (the table is filled column by column, 12 bytes a column).  E is that set of columns, f = |E| = 2 x (suspect table slots),
 * the same for all twelve rows.  The nine FEC packets carry no CRC, so parity columns are never erased.
 *
 * A row, in this order:
 *   1. a codeword: rows_clean++.
 *   2. else the errors-only rule above (a codeword within distance 8), with its counters: whatever the other call corrects, this
 *      one corrects identically.
 *   3. else, if 2 <= f <= 16: the codeword that equals the received row outside E except in at most e positions, where e = 0 is
 *      allowed whenever f <= 16 and e >= 1 only when 2 e + f <= 14.  (Two such codewords would differ in at most f + 2 e <= 16
 *      positions, fewer than the minimum distance 17: there is at most one.)  If it exists, the row's data bytes become that
 *      codeword's: rows_erasure_corrected++, erased_bytes_changed += the positions in E that changed,
 *      erasure_other_bytes_corrected += the changed positions outside E, data and parity together.
 *   4. else rows_uncorrectable++ and the row stays as received.
 *   The margin of two symbols for e >= 1 is a decision of this contract, not a measurement.  With 2 e + f = 16 nothing is left
 *   to check the error locator against: a row with more real errors than e -- a burst in the CRC-less FEC packets -- would be
 *   miscorrected with probability about 0.74^e / e!, which spoils bytes of packets whose CRC was good.  Two spare symbols divide
 *   that by 65 536.  With e = 0 a miscorrection can only change bytes of slots that were bad already.
 *   (f = 2 adds nothing to rule 2: e <= 6 is at most eight wrong bytes.  Step 3 begins to tell at f = 4.)
 *   How: one erasure locator per frame, E being shared by the rows.  Per row the modified syndromes, Berlekamp-Massey on those
 *   above f, the roots of the errata locator among the 204 positions, Forney's values (in E they may be zero) -- and then the
 *   pattern is held to the definition as pattern_holds does above: its 16 syndromes equal the row's, every position outside E is
 *   distinct and non-zero, and their count is within the bound.
 *
 * State record.  Of the same size, state_bytes(S); a magic of its own; the suspect bits of the D S carried slots (at most 150,
 * S = 50) in the head's 32 reserved bytes, carried slot i at bit i & 7 of byte i >> 3.  A record of one call is a fresh start
 * for the other.  head_ok_erasures() holds the bits of unused positions -- beyond D S, and in padding frames -- to zero.
 *
 * Counters.  The twelve words above with the same meaning, then slots_suspect (among the call's new slots),
 * frames_with_suspects (accepted frames with f >= 2), frames_beyond_erasures (of those, f > 16), rows_erasure_corrected,
 * erased_bytes_changed, erasure_other_bytes_corrected, and padding to 80 bytes.
 *
 * Not provided: correction of the FEC packets' own bytes in the output; erasure of parity columns; FEC schemes other than 1.
 */
#ifndef DABGPU_PACKET_FEC_H
#define DABGPU_PACKET_FEC_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DABGPU_FEC_FN __host__ __device__ __forceinline__
#else
#define DABGPU_FEC_FN inline
#endif

namespace dabgpu_packet_fec {

constexpr int SLOT_BYTES = 24, MAX_SLOTS = 64;
constexpr int FRAME_SLOTS = 103, DATA_SLOTS = 94, FEC_SLOTS = 9;
constexpr int FRAME_BYTES = SLOT_BYTES * FRAME_SLOTS, DATA_BYTES = SLOT_BYTES * DATA_SLOTS;
constexpr int ROWS = 12, N = 204, K = 188, T2 = 16, T = 8;
constexpr int FEC_ADDRESS = 1022, MARKS_NEEDED = 7;
constexpr int MAX_N_CIFS = 1 << 24;       /* slots = n_cifs * S stays an int32 */
constexpr uint8_t MARK_NONE = 0xFF;
constexpr uint32_t MAGIC = 0x43454650u;   /* "PFEC" */
constexpr int HEAD_BYTES = 64;
constexpr int64_t MAX_FRAMES_SEEN = int64_t(1) << 40;

struct Counters {                         /* == dabgpu_packet_fec_result */
    int32_t cifs, slots, marks;
    int32_t frames, frames_cut, frames_overlapping;
    int32_t rows_clean, rows_corrected, rows_uncorrectable;
    int32_t bytes_corrected, parity_bytes_corrected;
    int32_t reserved;
};

struct alignas(16) Head {                 /* the first 64 bytes of a state record; the carried frames follow */
    uint32_t magic;
    int32_t slots;                        /* S the record was written for */
    int64_t frames_seen;                  /* F0 */
    int64_t last_end;                     /* slot number of the last accepted frame's last slot, -1: none */
    uint8_t tail[8];                      /* the marks of slots F0 S - 8 .. F0 S - 1, as received */
    uint8_t reserved[32];
};
static_assert(sizeof(Counters) == 48 && sizeof(Head) == HEAD_BYTES, "records of the ABI");

DABGPU_FEC_FN bool bitrate_ok(int kbps) { return kbps >= 8 && kbps <= 512 && kbps % 8 == 0; }
DABGPU_FEC_FN int delay(int S) { return (FRAME_SLOTS - 1 + S - 1) / S; }
DABGPU_FEC_FN int carried_bytes(int S) { return delay(S) * S * SLOT_BYTES; }
DABGPU_FEC_FN int state_bytes(int S) { return HEAD_BYTES + ((carried_bytes(S) + 15) & ~15); }
/* the FEC frames that can end in one call of n frames: they do not overlap and lie inside the carried and the new frames */
DABGPU_FEC_FN int max_frames(int S, int n) { return int((int64_t(delay(S)) + n) * S / FRAME_SLOTS) + 1; }

/* the padding packet of stream frames below 0: byte i of its 24 */
constexpr uint32_t padding_crc() {
    uint32_t crc = 0xFFFF;
    for (int i = 0; i < SLOT_BYTES - 2; i++) {
        crc ^= uint32_t(i == 0 ? 0x0C : 0) << 8;
        for (int b = 0; b < 8; b++) crc = (crc & 0x8000u) ? ((crc << 1) ^ 0x1021u) & 0xFFFFu : (crc << 1) & 0xFFFFu;
    }
    return crc ^ 0xFFFFu;
}
constexpr uint32_t PADDING_CRC = padding_crc();
DABGPU_FEC_FN uint8_t padding_byte(int i) {
    return i == 0 ? uint8_t(0x0C) : i == SLOT_BYTES - 2 ? uint8_t(PADDING_CRC >> 8) : i == SLOT_BYTES - 1 ? uint8_t(PADDING_CRC & 0xFF) : uint8_t(0);
}

DABGPU_FEC_FN uint8_t mark_of(unsigned h0, unsigned h1) {
    const unsigned c = (h0 >> 2) & 15u;
    return ((h0 >> 6) == 0 && (((h0 & 3u) << 8) | h1) == unsigned(FEC_ADDRESS) && c <= 8) ? uint8_t(c) : MARK_NONE;
}

DABGPU_FEC_FN void head_fresh(Head &h, int S) {
    uint8_t *p = reinterpret_cast<uint8_t *>(&h);
    for (int i = 0; i < HEAD_BYTES; i++) p[i] = 0;
    h.magic = MAGIC;
    h.slots = S;
    h.last_end = -1;
    for (int i = 0; i < 8; i++) h.tail[i] = MARK_NONE;
}
/* a record with this magic, written for S slots a frame: everything but what `reserved` may hold */
DABGPU_FEC_FN bool head_written(const Head &h, int S, uint32_t magic) {
    bool ok = h.magic == magic && h.slots == S && h.frames_seen >= 0 && h.frames_seen <= MAX_FRAMES_SEEN;
    ok = ok && h.last_end >= -1 && (h.last_end == -1 || (h.last_end >= FRAME_SLOTS - 1 && h.last_end < h.frames_seen * S));
    for (int i = 0; i < 8; i++)
        ok = ok && (h.tail[i] == MARK_NONE || (h.tail[i] <= 8 && h.frames_seen * S - 8 + i >= 0));
    return ok;
}
/* a record this code wrote for S slots a frame */
DABGPU_FEC_FN bool head_ok(const Head &h, int S) {
    bool ok = head_written(h, S, MAGIC);
    for (int i = 0; i < 32; i++) ok = ok && h.reserved[i] == 0;
    return ok;
}

/* a frame ends at new slot j of a call: mark(jj) is the mark of new slot jj, jj >= -8 (below 0: the record's tail) */
template <class Mark> DABGPU_FEC_FN bool ends_here(Mark mark, int64_t j) {
    int hits = 0;
    for (int i = 0; i < FEC_SLOTS; i++) hits += mark(j - (FEC_SLOTS - 1) + i) == i;
    return hits >= MARKS_NEEDED;
}
enum Verdict : int { ACCEPTED = 0, CUT = 1, OVERLAPPING = 2 };
/* the candidate that ends at slot number g_end; an accepted one becomes the last accepted frame */
DABGPU_FEC_FN int judge(Head &h, Counters &c, int64_t g_end) {
    const int64_t first = g_end - (FRAME_SLOTS - 1);
    if (first < 0) {
        c.frames_cut++;
        return CUT;
    }
    if (first <= h.last_end) {
        c.frames_overlapping++;
        return OVERLAPPING;
    }
    c.frames++;
    h.last_end = g_end;
    return ACCEPTED;
}

/* ---- GF(2^8), x^8 + x^4 + x^3 + x^2 + 1, alpha = 2 */
struct alignas(16) Gf {
    uint8_t exp[512];
    uint8_t log[256];
};
constexpr Gf make_gf() {
    Gf g{};
    unsigned x = 1;
    for (int i = 0; i < 255; i++) {
        g.exp[i] = uint8_t(x);
        g.log[x] = uint8_t(i);
        x <<= 1;
        if (x & 0x100u) x ^= 0x11Du;
    }
    for (int i = 255; i < 512; i++) g.exp[i] = g.exp[i - 255];
    g.log[0] = 0;
    return g;
}
static_assert(sizeof(Gf) == 768, "copied as 192 words");
DABGPU_FEC_FN unsigned gmul(const Gf &g, unsigned a, unsigned b) { return (a && b) ? g.exp[g.log[a] + g.log[b]] : 0u; }
DABGPU_FEC_FN unsigned gdiv(const Gf &g, unsigned a, unsigned b) { return a ? g.exp[g.log[a] + 255 - g.log[b]] : 0u; }   /* b != 0 */
/* v alpha^e, e >= 0 */
DABGPU_FEC_FN unsigned gscale(const Gf &g, unsigned v, int e) { return v ? g.exp[(g.log[v] + e) % 255] : 0u; }

/* where byte c of row r's codeword lies among the 2472 bytes of an FEC frame */
DABGPU_FEC_FN int frame_index(int r, int c) {
    if (c < K) return ROWS * c + r;
    const int p = ROWS * (c - K) + r;
    return DATA_BYTES + SLOT_BYTES * (p / 22) + 2 + p % 22;
}

/* the byte v at codeword position c, into the 16 syndromes: one log look-up, then 16 independent exp look-ups (the index
 * advances by 203 - c per k), not a dependent Horner chain */
template <class Syn> DABGPU_FEC_FN void syndrome_add(const Gf &g, unsigned v, int c, Syn &S) {
    if (!v) return;
    const int p = N - 1 - c;              /* < 255 */
    int idx = g.log[v];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < T2; k++) {
        S[k] ^= g.exp[idx];
        idx += p;
        if (idx >= 255) idx -= 255;
    }
}

/* what decoding one row needs beside the table: on the device in LDS (indexed by variables, so never in registers) */
struct RowWork {
    uint8_t syn[T2];
    uint8_t L[T2 + 1], B[T2 + 1], Tm[T2 + 1];   /* locator, Berlekamp-Massey's previous one, a copy */
    uint8_t Om[T];                        /* evaluator */
    uint8_t pos[T], val[T];               /* the pattern: codeword positions and values */
    int32_t ll, n;                        /* the locator's degree; roots found (counted beyond T, stored up to T) */
};

DABGPU_FEC_FN bool row_is_codeword(const RowWork &w) {
    unsigned any = 0;
    for (int k = 0; k < T2; k++) any |= w.syn[k];
    return any == 0;
}

/* Berlekamp-Massey on w.syn, then the evaluator: w.L, w.ll, w.Om; false when the locator's degree is beyond T */
DABGPU_FEC_FN bool locator(const Gf &g, RowWork &w) {
    for (int i = 0; i <= T2; i++) w.L[i] = w.B[i] = 0;
    w.L[0] = w.B[0] = 1;
    int ll = 0, m = 1;
    unsigned bb = 1;
    for (int n = 0; n < T2; n++) {
        unsigned d = w.syn[n];
        for (int i = 1; i <= ll && i <= n; i++) d ^= gmul(g, w.L[i], w.syn[n - i]);
        if (d == 0) {
            m++;
            continue;
        }
        for (int i = 0; i <= T2; i++) w.Tm[i] = w.L[i];
        const unsigned coef = gdiv(g, d, bb);
        for (int i = m; i <= T2; i++) w.L[i] ^= uint8_t(gmul(g, coef, w.B[i - m]));
        if (2 * ll <= n) {
            ll = n + 1 - ll;
            for (int i = 0; i <= T2; i++) w.B[i] = w.Tm[i];
            bb = d;
            m = 1;
        } else {
            m++;
        }
    }
    w.ll = ll;
    w.n = 0;
    if (ll > T) return false;
    for (int i = 0; i < T; i++) {
        unsigned v = 0;
        for (int j = 0; j <= i && j <= ll; j++) v ^= gmul(g, w.L[j], w.syn[i - j]);
        w.Om[i] = uint8_t(v);
    }
    return true;
}

/* is codeword position c a root of the locator, and with which value (Forney; 0: none can be given) */
DABGPU_FEC_FN bool root_at(const Gf &g, const RowWork &w, int c, unsigned &value) {
    const int p = N - 1 - c, xinv = (255 - p) % 255;
    unsigned ev = 0;
    for (int j = 0; j <= w.ll; j++) ev ^= gscale(g, w.L[j], xinv * j);
    if (ev) return false;
    unsigned om = 0, dl = 0;
    for (int j = 0; j < w.ll; j++) om ^= gscale(g, w.Om[j], xinv * j);
    for (int j = 1; j <= w.ll; j += 2) dl ^= gscale(g, w.L[j], xinv * (j - 1));
    value = dl ? gmul(g, g.exp[p], gdiv(g, om, dl)) : 0u;
    return true;
}

/* the pattern held to the definition: the corrected row is a codeword within distance T of the received one */
DABGPU_FEC_FN bool pattern_holds(const Gf &g, const RowWork &w) {
    if (w.ll < 1 || w.ll > T || w.n != w.ll) return false;
    for (int i = 0; i < w.n; i++)
        if (!w.val[i] || w.pos[i] >= N) return false;
    for (int k = 0; k < T2; k++) {
        unsigned s = 0;
        for (int i = 0; i < w.n; i++) s ^= gscale(g, w.val[i], k * (N - 1 - w.pos[i]));
        if (s != w.syn[k]) return false;
    }
    return true;
}

struct FrameCounts {
    int32_t rows_clean, rows_corrected, rows_uncorrectable, bytes_corrected, parity_bytes_corrected;
};
/* a row that has been through locator / root_at / pattern_holds (or is a codeword): its counts */
DABGPU_FEC_FN void count_row(const RowWork &w, bool codeword, bool holds, FrameCounts &f) {
    if (codeword) {
        f.rows_clean++;
    } else if (!holds) {
        f.rows_uncorrectable++;
    } else {
        f.rows_corrected++;
        for (int i = 0; i < w.n; i++) (w.pos[i] < K ? f.bytes_corrected : f.parity_bytes_corrected)++;
    }
}

/* ---- a held pattern applied (kernels and host path) */

/* the data bytes of a held pattern (n positions and values) of row r, written where they lie: slot(i) is the 24 bytes of the
 * frame's slot i, fr the frame as received */
template <class Slot> DABGPU_FEC_FN void write_back(Slot slot, const uint8_t *fr, int r, const uint8_t *pos, const uint8_t *val, int n) {
    for (int i = 0; i < n; i++) {
        if (pos[i] >= K) continue;
        const int b = frame_index(r, pos[i]);
        slot(b / SLOT_BYTES)[b % SLOT_BYTES] = uint8_t(fr[b] ^ val[i]);
    }
}

/* ---- the host path: the rows of one FEC frame */

/* the 2472 bytes of the frame whose slot i (0..102) is the 24 bytes at slot(i) */
template <class Slot> inline void load_frame(Slot slot, uint8_t *fr) {
    for (int i = 0; i < FRAME_SLOTS; i++) {
        const uint8_t *p = slot(i);
        for (int b = 0; b < SLOT_BYTES; b++) fr[SLOT_BYTES * i + b] = p[b];
    }
}

/* Row r of the frame fr by the errors-only rule: its syndromes into w, and for a row that is no codeword Berlekamp-Massey, the
 * roots among the 204 positions and pattern_holds.  True: w holds the pattern to apply. */
inline bool decode_row(const Gf &g, const uint8_t *fr, int r, RowWork &w, bool &codeword) {
    unsigned S[T2] = {};
    for (int col = 0; col < N; col++) syndrome_add(g, fr[frame_index(r, col)], col, S);
    for (int k = 0; k < T2; k++) w.syn[k] = uint8_t(S[k]);
    w.ll = w.n = 0;
    codeword = row_is_codeword(w);
    if (codeword || !locator(g, w)) return false;
    for (int col = 0; col < N; col++) {
        unsigned v;
        if (!root_at(g, w, col, v)) continue;
        if (w.n < T) {
            w.pos[w.n] = uint8_t(col);
            w.val[w.n] = uint8_t(v);
        }
        w.n++;
    }
    return pattern_holds(g, w);
}

inline void add_counts(Counters &c, const FrameCounts &f) {
    c.rows_clean += f.rows_clean;
    c.rows_corrected += f.rows_corrected;
    c.rows_uncorrectable += f.rows_uncorrectable;
    c.bytes_corrected += f.bytes_corrected;
    c.parity_bytes_corrected += f.parity_bytes_corrected;
}

/* One FEC frame whose slot i (0..102) is the 24 bytes at slot(i): corrected in place */
template <class Slot> inline void correct_frame(const Gf &g, Slot slot, Counters &c) {
    uint8_t fr[FRAME_BYTES];
    load_frame(slot, fr);
    FrameCounts f = {};
    for (int r = 0; r < ROWS; r++) {
        RowWork w;
        bool codeword;
        const bool holds = decode_row(g, fr, r, w, codeword);
        count_row(w, codeword, holds, f);
        if (holds) write_back(slot, fr, r, w.pos, w.val, w.n);
    }
    add_counts(c, f);
}

/* ---- the host path: the window of one call */

/* One entry of a call on memory the caller can read and write.  state_in: state_bytes(S) or NULL; state_out: state_bytes(S), no
 * overlap with state_in; out: [n][out_stride], no overlap with in.  The window is the D carried frames, then the n new ones; its
 * first n frames go out, its last D are carried on. */
struct Window {
    const uint8_t *state_in;
    uint8_t *state_out;
    const uint8_t *in;
    uint64_t in_stride;
    int n, S;
    uint8_t *out;
    uint64_t out_stride;
    /* where window frame wf goes, and window slot w */
    uint8_t *frame(int64_t wf) const { return wf < n ? out + uint64_t(wf) * out_stride : state_out + HEAD_BYTES + (wf - n) * (SLOT_BYTES * S); }
    uint8_t *slot(int64_t w) const { return frame(w / S) + SLOT_BYTES * (w % S); }
    /* the mark of new slot j, j >= -8, from the bytes as received (below 0: the tail of the head the call began with) */
    uint8_t mark(const Head &h, int64_t j) const {
        if (j < 0) return h.tail[8 + j];
        const uint8_t *p = in + uint64_t(j / S) * in_stride + SLOT_BYTES * (j % S);
        return mark_of(p[0], p[1]);
    }
};

/* the head a call begins with: the record's where ok() knows it, else what fresh() makes.  True: a fresh start. */
inline bool start_head(Head &h, const uint8_t *state_in, int S, bool (*ok)(const Head &, int), void (*fresh)(Head &, int)) {
    bool is_fresh = state_in == nullptr;
    if (!is_fresh) {
        for (int i = 0; i < HEAD_BYTES; i++) reinterpret_cast<uint8_t *>(&h)[i] = state_in[i];
        is_fresh = !ok(h, S);
    }
    if (is_fresh) fresh(h, S);
    return is_fresh;
}

/* every frame of the window to where it goes, as received (a fresh start has padding for carried frames); the record's tail
 * beyond the carried frames zeroed */
inline void move_window(const Window &w, bool fresh) {
    const int D = delay(w.S), fb = SLOT_BYTES * w.S;
    for (int64_t wf = 0; wf < int64_t(D) + w.n; wf++) {
        uint8_t *d = w.frame(wf);
        if (wf >= D) {
            const uint8_t *s = w.in + uint64_t(wf - D) * w.in_stride;
            for (int i = 0; i < fb; i++) d[i] = s[i];
        } else if (fresh) {
            for (int i = 0; i < fb; i++) d[i] = padding_byte(i % SLOT_BYTES);
        } else {
            const uint8_t *s = w.state_in + HEAD_BYTES + wf * fb;
            for (int i = 0; i < fb; i++) d[i] = s[i];
        }
    }
    for (int i = HEAD_BYTES + D * fb; i < state_bytes(w.S); i++) w.state_out[i] = 0;
}

/* new slot j of the call: its mark is counted; true when an accepted frame ends there, `first` its first slot counted from the
 * window's */
inline bool frame_ends(const Window &w, Head &h, Counters &c, int64_t j, int64_t &first) {
    auto mark = [&](int64_t jj) { return w.mark(h, jj); };
    c.marks += mark(j) != MARK_NONE;
    if (!ends_here(mark, j) || judge(h, c, h.frames_seen * w.S + j) != ACCEPTED) return false;
    first = int64_t(delay(w.S)) * w.S + j - (FRAME_SLOTS - 1);
    return true;
}

/* the head moves on by the call's n frames and is stored */
inline void store_head(Head &h, const Window &w) {
    const int64_t slots = int64_t(w.n) * w.S;
    uint8_t tail[8];
    for (int i = 0; i < 8; i++) tail[i] = w.mark(h, slots - 8 + i);
    for (int i = 0; i < 8; i++) h.tail[i] = tail[i];
    h.frames_seen += w.n;
    for (int i = 0; i < HEAD_BYTES; i++) w.state_out[i] = reinterpret_cast<const uint8_t *>(&h)[i];
}

/* One entry of a call: the twin of the kernels.  c: the counts of this call. */
inline void process(const Gf &g, const uint8_t *state_in, uint8_t *state_out, Counters &c, const uint8_t *in, uint64_t in_stride, int n, int S,
                    uint8_t *out, uint64_t out_stride) {
    const Window w = {state_in, state_out, in, in_stride, n, S, out, out_stride};
    Head h;
    move_window(w, start_head(h, state_in, S, head_ok, head_fresh));
    c = Counters{};
    c.cifs = n;
    c.slots = n * S;
    for (int64_t j = 0, first; j < int64_t(n) * S; j++)
        if (frame_ends(w, h, c, j, first)) correct_frame(g, [&](int i) { return w.slot(first + i); }, c);
    store_head(h, w);
}

}  /* namespace dabgpu_packet_fec */
#endif
