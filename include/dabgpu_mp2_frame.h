/* dabgpu_mp2_frame.h -- DAB (MPEG layer II) audio frames: header check, the ISO CRC over bit allocation and SCFSI, pairing
 * of 24 kHz frames, and the lift of a frame's PAD into the row layout dabgpu_pad_labels_dev / dabgpu_mot_slides_dev read.
 *
 * One implementation: the kernels (csrc/mp2_kernels.hip), the host twin dabgpu_mp2_follow_host and the host mirror's
 * Basic_DAB_Channel all run the functions below.  Plain C++17, header-only, no allocation, no table in memory (the
 * tables are packed constants and comparisons); every function is __host__ __device__ under hipcc and inline otherwise.
 * A frame is handed over as a callable `f(i)` = byte i of the frame, 0 <= i < L: nothing here reads outside [0, L).
 *
 * THE CONTRACT (EN 300 401 clauses 7.3, 7.4.1; ISO/IEC 11172-3 clause 2.4.1 and Annex B; ISO/IEC 13818-3 for ID = 0),
 * every ambiguity decided.  B = the sub-channel's bit rate in kbit/s (8 .. 384, a multiple of 8); a logical frame is
 * 3 B bytes.
 *
 * Header (bytes 0 .. 3 of a logical frame).  VALID when: the first 12 bits are 0xFFF; layer (2 bits) is 10b; the
 * sampling index (2 bits) is 01b; the bit-rate index is 1 .. 14 and names B in the table of the header's ID (MPEG-1 for
 * ID = 1, LSF for ID = 0); and, for ID = 1, the pair (mode, B) is one ISO 11172-3 2.4.2.3 allows: 32, 48, 56, 80 only
 * single channel (mode 11b), 224, 256, 320, 384 only the other three modes.  ID = 0 has no such restriction.  Padding,
 * private, copyright, original and emphasis bits are not looked at.  ID = 1 is 48 kHz: the frame is ONE logical frame,
 * L = 3 B.  ID = 0 is 24 kHz: the frame is TWO consecutive logical frames, L = 6 B (its table ends at B = 160).
 *
 * ISO CRC.  Protection bit 1: no CRC; the frame is header-valid, counts in frames_no_crc and delivers no PAD.
 * Protection bit 0: bytes 4, 5 hold the CRC-16 (x^16 + x^15 + x^2 + 1 = 0x8005, start 0xFFFF, most significant bit
 * first, not reflected, no final XOR), big-endian, over header bits 16 .. 31 (bytes 2, 3), then from byte 6 on the
 * bit-allocation bits, then the SCFSI bits, as they lie in the stream.  Channels = 1 for mode 11b, else 2; rate per
 * channel = B / channels.  Sub-band sb < sblimit has nbal(sb) allocation bits (the table block below).  With two
 * channels, sub-bands below the bound carry one field per channel, those at or above it ONE field that serves both; the
 * bound is sblimit except in joint stereo (mode 01b): 4, 8, 12, 16 for mode extension 0 .. 3, clamped to sblimit.
 * SCFSI: 2 bits per (sub-band, channel) whose allocation is not zero -- a shared field that is not zero counts for both
 * channels.  The protected bits end there.  If they would run past L the frame fails (it counts in crc_failed); so does
 * a CRC that differs.  Scale factors and samples are not read.
 *
 * ScF-CRC bytes: c of them lie in front of the last 2 + 4 bytes of the frame; they are stepped over, never checked
 * (nothing pins which frame's scale factors they cover).  c is in the table block.
 *
 * PAD row.  F-PAD = f(L-2), f(L-1).  X-PAD logical byte 0 is f(L-3); logical bytes 0 .. 3 are f(L-6 .. L-3], logical
 * bytes 4 and up go on backwards in front of the ScF-CRC bytes.  For a frame with a valid header, protection bit 0 and a
 * good CRC (a GOOD frame): x = min(196, L - 8 - c), p = f[L-2-c-x .. L-6-c) ++ f[L-6 .. L-2), and the row is
 *     0x80, x + 2, p (x bytes), F-PAD0, F-PAD1, 0, 0, then zeros to ROW_BYTES = 220
 * -- a data stream element with tag 0 of one pseudo access unit of x + 6 bytes, the last two standing for the AU CRC the
 * walks step over.  Its status: firecode_ok = 1, num_aus = 1, au_crc_mask = 1, au_start = {0, x + 6}, everything else 0.
 * A slot that is not a good frame (invalid header, no CRC, CRC failed) becomes a row of 220 zeros with firecode_ok = 1,
 * num_aus = 1, au_crc_mask = 0, au_start = {0, 0}: one lost AU for the walks.  (c depends on the mode, so a slot without
 * a valid header has no PAD position to lift from.)  220 = 110 * 2: the PAD and slideshow entries take the rows with
 * bitrate_kbps = 16 and data_stride >= 220.
 *
 * Following, one entry in one call.  F = the `held` logical frame of carry_in (0 or 1) followed by the n_cifs new ones,
 * T = held + n_cifs.  hits1 = frames of F with a valid ID = 1 header; votes0[r] = frames i = r (mod 2) with a valid
 * ID = 0 header, hits0 = their sum; hits = hits1 + hits0.  (Header-valid is all that votes: the CRC is not looked at.)
 *   hits1 >= 1 and hits1 >= hits0       -> 48 kHz, phase 0, votes = hits1
 *   else hits0 >= 1                     -> 24 kHz, phase p = 1 if votes0[1] > votes0[0] else 0 (with two residues, "a synced
 *                                          carry stays on 0 unless another residue has strictly more" and "the smallest residue
 *                                          with the maximum" are the same rule), votes = votes0[p]
 *   else the carry is synced            -> the carry's rate, phase 0, votes = 0
 *   else                                -> no rate: no rows, phase = -1, carry_out holds the last min(1, T) frame with
 *                                          synced = 0, dropped = the rest.
 * 48 kHz: slot k is frame k; n_rows = T, nothing is held, dropped = 0.  24 kHz: slot k is frames p + 2k, p + 2k + 1;
 * n_rows = (T - p) / 2, dropped = p, an unpaired last half is held.  synced = 1 iff votes > 0 or n_rows = 0; a carry that
 * is not synced records no rate.  Rows come in slot order; every slot is parsed for the chosen ID (a valid header of the
 * other ID is a header error); rows beyond n_rows are not written.  frames = n_rows; header_errors + frames_no_crc +
 * crc_failed + good frames = frames.  mode = the mode bits of the first frame i = phase (mod slot length), i < T, whose
 * header is valid for the chosen ID; -1 when there is none.
 *
 * The carry record: 16-byte header {int32 synced, held, rate (0 none, 1 = 48 kHz, 2 = 24 kHz), magic}, then one logical
 * frame of 3 B bytes, the whole rounded up to 16 bytes; written whole (header, the held frame, zeros behind it).  A record
 * this code did not write -- wrong magic (all zero included), a field out of range, synced without a rate or a rate
 * without synced, a held frame at 48 kHz -- is a fresh start: not synced, nothing held.
 */
#ifndef DABGPU_MP2_FRAME_H
#define DABGPU_MP2_FRAME_H

#include <stdint.h>

#if defined(__HIPCC__)
#define DABGPU_MP2_FN __host__ __device__ inline
#define DABGPU_MP2_FN_MEMBER __host__ __device__
#else
#define DABGPU_MP2_FN inline
#define DABGPU_MP2_FN_MEMBER
#endif

namespace dabgpu_mp2 {

/* ------------------------------------------------------------------------------------------------------------------
 * THE TABLE BLOCK: stated from the standards as known; one line each, so that one line can be corrected.
 * Bit rates in units of 8 kbit/s, index 0 in the low byte (index 0 = free format and 15 = forbidden: never valid).    */
/* ISO 11172-3 2.4.2.3, layer II, ID = 1:  -, 32, 48, 56, 64, 80, 96, 112 | 128, 160, 192, 224, 256, 320, 384, -       */
constexpr uint64_t BITRATE8_ID1_LO = 0x0E0C0A0807060400ull, BITRATE8_ID1_HI = 0x003028201C181410ull;
/* ISO 13818-3 2.4.2.3, layers II/III, ID = 0:  -, 8, 16, 24, 32, 40, 48, 56 | 64, 80, 96, 112, 128, 144, 160, -       */
constexpr uint64_t BITRATE8_ID0_LO = 0x0706050403020100ull, BITRATE8_ID0_HI = 0x001412100E0C0A08ull;
/* ISO 11172-3 2.4.2.3: bit rates (kbit/s) only single channel may use | only the two-channel modes may use            */
DABGPU_MP2_FN bool mono_only_rate(int B) { return B == 32 || B == 48 || B == 56 || B == 80; }
DABGPU_MP2_FN bool two_channel_only_rate(int B) { return B == 224 || B == 256 || B == 320 || B == 384; }
/* ISO 11172-3 Annex B table B.2: nbal is 4 below sub-band T4, 3 below T3, 2 below sblimit                             */
struct AllocTable { int sblimit, t4, t3; };
/*   B.2c, 48 kHz at 32 or 48 kbit/s per channel: sblimit 8, sub-bands 0-1: 4 bits, 2-7: 3                             */
constexpr AllocTable ALLOC_48K_SMALL = {8, 2, 8};
/*   B.2a, 48 kHz otherwise: sblimit 27, sub-bands 0-10: 4, 11-22: 3, 23-26: 2                                         */
constexpr AllocTable ALLOC_48K_LARGE = {27, 11, 23};
/*   ISO 13818-3 table B.1, 24 kHz, any rate: sblimit 30, sub-bands 0-3: 4, 4-10: 3, 11-29: 2                          */
constexpr AllocTable ALLOC_24K = {30, 4, 11};
DABGPU_MP2_FN bool small_table_rate(int per_channel_kbps) { return per_channel_kbps == 32 || per_channel_kbps == 48; }
/* EN 300 401 7.3.1.5 / 7.4.1: ScF-CRC bytes in front of the fixed PAD bytes                                           */
DABGPU_MP2_FN int scf_crc_bytes(int id, int per_channel_kbps) { return id == 1 ? (per_channel_kbps < 56 ? 2 : 4) : 4; }
/* ------------------------------------------------------------------------------------------------------------------ */

constexpr int ROW_BYTES = 220;         /* = 110 * 2: a row of the PAD calls at PAD_KBPS */
constexpr int PAD_KBPS = 16;
constexpr int XPAD_MAX = 196;
constexpr int FRONT_BYTES = 48;        /* the parse reads at most 6 + ceil((2 * 88 + 2 * 54) / 8) = 42 bytes from the front */
constexpr int32_t CARRY_MAGIC = 0x4332504D;
constexpr int CARRY_HEADER = 16;
enum Rate { RATE_NONE = 0, RATE_48K = 1, RATE_24K = 2 };
enum Kind { FRAME_GOOD = 0, FRAME_HEADER_ERROR = 1, FRAME_NO_CRC = 2, FRAME_CRC_FAILED = 3 };

struct Result {                /* == dabgpu_mp2_result */
    int32_t id, sample_rate, bitrate_kbps, mode, phase, held, synced, hits;
    int32_t frames, header_errors, crc_failed, frames_no_crc, dropped, reserved[3];
};
static_assert(sizeof(Result) == 64, "record of the ABI");

DABGPU_MP2_FN bool bitrate_ok(int B) { return B >= 8 && B <= 384 && B % 8 == 0; }
DABGPU_MP2_FN int carry_bytes(int B) { return (CARRY_HEADER + 3 * B + 15) & ~15; }

DABGPU_MP2_FN int bitrate_of_index(int id, int idx) {
    const uint64_t w = id ? (idx < 8 ? BITRATE8_ID1_LO : BITRATE8_ID1_HI) : (idx < 8 ? BITRATE8_ID0_LO : BITRATE8_ID0_HI);
    return int((w >> (8 * (idx & 7))) & 0xFF) * 8;
}

/* the four header bytes, big-endian in h: -> the header's ID (0, 1) when it is valid for B, else -1 */
DABGPU_MP2_FN int header_id(uint32_t h, int B) {
    if ((h >> 20) != 0xFFFu || ((h >> 17) & 3) != 2 || ((h >> 10) & 3) != 1) return -1;
    const int id = int((h >> 19) & 1), idx = int((h >> 12) & 15), mode = int((h >> 6) & 3);
    if (idx == 0 || idx == 15 || bitrate_of_index(id, idx) != B) return -1;
    if (id == 1 && (mode == 3 ? two_channel_only_rate(B) : mono_only_rate(B))) return -1;
    return id;
}
DABGPU_MP2_FN int header_mode(uint32_t h) { return int((h >> 6) & 3); }

/* CRC-16 0x8005, most significant bit first: a byte a step.  The eight shifts of one byte fold into
 * T[x] = (x << 1) ^ (x << 2) ^ (parity(x) ? 0x8003 : 0), held to the bit-serial definition for all 256 bytes by
 * tests/mp2_frame_fuzz.cpp. */
DABGPU_MP2_FN uint32_t crc_step_byte(uint32_t crc, uint32_t v) {
    const uint32_t x = ((crc >> 8) ^ v) & 0xFF;
    uint32_t p = x ^ (x >> 4);
    p ^= p >> 2;
    p ^= p >> 1;
    return ((crc << 8) ^ (x << 1) ^ (x << 2) ^ ((p & 1) ? 0x8003u : 0u)) & 0xFFFF;
}
DABGPU_MP2_FN uint32_t crc_step_bit(uint32_t crc, uint32_t bit) {
    const uint32_t top = ((crc >> 15) ^ bit) & 1;
    return ((crc << 1) ^ (top ? 0x8005u : 0u)) & 0xFFFF;
}

struct Shape {                 /* what the mode and the rate say about a frame with a valid header */
    AllocTable t;
    int channels, bound, c;
};
DABGPU_MP2_FN Shape frame_shape(uint32_t h, int id, int B) {
    Shape s;
    const int mode = header_mode(h);
    s.channels = mode == 3 ? 1 : 2;
    const int per_channel = B / s.channels;
    s.t = id == 1 ? (small_table_rate(per_channel) ? ALLOC_48K_SMALL : ALLOC_48K_LARGE) : ALLOC_24K;
    s.bound = s.t.sblimit;
    if (mode == 1) {
        const int jb = 4 * (int((h >> 4) & 3) + 1);
        s.bound = jb < s.t.sblimit ? jb : s.t.sblimit;
    }
    s.c = scf_crc_bytes(id, per_channel);
    return s;
}
DABGPU_MP2_FN int nbal(const AllocTable &t, int sb) { return sb < t.t4 ? 4 : sb < t.t3 ? 3 : 2; }

/* n (1 .. 4) bits at bit position pos, most significant first; the caller has checked pos + n <= 8 L */
template <class Bytes>
DABGPU_MP2_FN uint32_t get_bits(const Bytes &f, int pos, int n) {
    const int at = pos >> 3, in = pos & 7;
    uint32_t v = uint32_t(f(at)) << 8;
    if (in + n > 8) v |= f(at + 1);
    return (v >> (16 - in - n)) & ((1u << n) - 1);
}

DABGPU_MP2_FN uint32_t header_word(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3) {
    return (b0 << 24) | (b1 << 16) | (b2 << 8) | b3;
}

/* One frame of L bytes (L = 3 B for want_id 1, 6 B for 0) -> its Kind; c_out: the ScF-CRC count (valid headers only). */
template <class Bytes>
DABGPU_MP2_FN int parse_frame(const Bytes &f, int L, int B, int want_id, int *c_out) {
    *c_out = 0;
    if (L < 4) return FRAME_HEADER_ERROR;
    const uint32_t h = header_word(f(0), f(1), f(2), f(3));
    if (header_id(h, B) != want_id) return FRAME_HEADER_ERROR;
    const Shape s = frame_shape(h, want_id, B);
    *c_out = s.c;
    if ((h >> 16) & 1) return FRAME_NO_CRC;
    int pos = 48, nz = 0;
    for (int sb = 0; sb < s.t.sblimit; sb++) {
        const int n = nbal(s.t, sb);
        const int fields = s.channels == 2 && sb < s.bound ? 2 : 1;
        if (pos + fields * n > 8 * L) return FRAME_CRC_FAILED;
        for (int k = 0; k < fields; k++, pos += n)
            if (get_bits(f, pos, n)) nz += s.channels == 2 && fields == 1 ? 2 : 1;
    }
    const int end = pos + 2 * nz;
    if (end > 8 * L) return FRAME_CRC_FAILED;
    uint32_t crc = crc_step_byte(crc_step_byte(0xFFFF, f(2)), f(3));
    int at = 6;
    for (; 8 * (at + 1) <= end; at++) crc = crc_step_byte(crc, f(at));
    if (end & 7) {
        const uint32_t v = f(at);
        for (int b = 0; b < (end & 7); b++) crc = crc_step_bit(crc, (v >> (7 - b)) & 1);
    }
    return crc == ((uint32_t(f(4)) << 8) | f(5)) ? FRAME_GOOD : FRAME_CRC_FAILED;
}

DABGPU_MP2_FN int xpad_bytes(int L, int c) { return L - 8 - c < XPAD_MAX ? L - 8 - c : XPAD_MAX; }

/* byte j (0 .. 219) of the row of a GOOD frame */
template <class Bytes>
DABGPU_MP2_FN uint8_t row_byte(const Bytes &f, int L, int c, int x, int j) {
    if (j == 0) return 0x80;
    if (j == 1) return uint8_t(x + 2);
    const int q = j - 2;
    if (q < x - 4) return f(L - 2 - c - x + q);
    if (q < x + 2) return f(L - 6 + (q - (x - 4)));
    return 0;
}
/* word w (0 .. 15) of a slot's dabgpu_superframe_status; x < 0: not a good frame */
DABGPU_MP2_FN int32_t status_word(int w, int x) {
    return w == 0 || w == 3 ? 1 : w == 4 ? (x >= 0 ? 1 : 0) : w == 6 ? (x >= 0 ? x + 6 : 0) : 0;
}

struct Carry { int synced, held, rate; };
DABGPU_MP2_FN Carry read_carry(int32_t synced, int32_t held, int32_t rate, int32_t magic) {
    Carry c = {0, 0, 0};
    const bool ok = magic == CARRY_MAGIC && (synced == 0 || synced == 1) && (held == 0 || held == 1) && rate >= 0 && rate <= 2 &&
                    (synced == 1) == (rate != 0) && !(rate == RATE_48K && held);
    if (ok) { c.synced = synced; c.held = held; c.rate = rate; }
    return c;
}

struct Plan {
    int rate, phase, n_rows, first_kept, kept, dropped, synced, votes;
};
/* the rate and phase of one entry in one call, and what follows from them */
DABGPU_MP2_FN Plan decide(const Carry &cy, int T, int hits1, int votes0_0, int votes0_1) {
    Plan p = {RATE_NONE, -1, 0, 0, 0, 0, 0, 0};
    const int hits0 = votes0_0 + votes0_1;
    if (hits1 >= 1 && hits1 >= hits0) {
        p.rate = RATE_48K; p.phase = 0; p.votes = hits1;
    } else if (hits0 >= 1) {
        p.rate = RATE_24K; p.phase = votes0_1 > votes0_0 ? 1 : 0; p.votes = p.phase ? votes0_1 : votes0_0;
    } else if (cy.synced) {
        p.rate = cy.rate; p.phase = 0;
    }
    if (p.rate == RATE_NONE) {
        p.kept = T < 1 ? T : 1;
        p.first_kept = T - p.kept;
        p.dropped = p.first_kept;
        return p;
    }
    const int per = p.rate == RATE_24K ? 2 : 1;
    p.n_rows = T - p.phase >= per ? (T - p.phase) / per : 0;
    p.first_kept = p.phase + per * p.n_rows;
    if (p.first_kept > T) p.first_kept = T;                            /* (T = 0 with phase 1 cannot happen: no votes then) */
    p.kept = T - p.first_kept;
    p.dropped = p.phase;
    p.synced = p.votes > 0 || p.n_rows == 0;
    return p;
}
DABGPU_MP2_FN int slot_frames(int rate) { return rate == RATE_24K ? 2 : 1; }

DABGPU_MP2_FN Result plan_result(const Plan &p, int B, int hits, int mode) {
    Result r = {};
    r.id = p.rate == RATE_48K ? 1 : p.rate == RATE_24K ? 0 : -1;
    r.sample_rate = p.rate == RATE_48K ? 48000 : p.rate == RATE_24K ? 24000 : 0;
    r.bitrate_kbps = p.rate == RATE_NONE ? 0 : B;
    r.mode = p.rate == RATE_NONE ? -1 : mode;
    r.phase = p.phase; r.held = p.kept; r.synced = p.synced; r.hits = hits;
    r.frames = p.n_rows; r.dropped = p.dropped;
    return r;
}

/* a frame that lies in two pieces: bytes [0, split) at a, the rest at b (a 24 kHz frame's two logical frames) */
struct TwoPart {
    const uint8_t *a, *b;
    int split;
    DABGPU_MP2_FN_MEMBER uint8_t operator()(int i) const { return i < split ? a[i] : b[i - split]; }
};

}  // namespace dabgpu_mp2

#endif
