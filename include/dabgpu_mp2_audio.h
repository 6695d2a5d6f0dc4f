/* dabgpu_mp2_audio.h -- DAB (MPEG layer II) audio frames past the ISO CRC: bit allocation, SCFSI, scale factors, sample
 * unpacking with the grouped code words, requantisation and scaling to the 36 x 32 sub-band samples of each channel, and
 * the audio level record of a frame.  The sibling of dabgpu_mp2_frame.h, whose frame_shape, nbal, get_bits and TwoPart it
 * uses.  The polyphase synthesis to PCM is NOT here (it needs the 512-tap window of ISO 11172-3 table B.3).
 *
 * One implementation: the kernel (csrc/mp2_audio_kernels.hip) runs the pieces below a lane per cell, the host twin
 * dabgpu_mp2_subbands_host and the host mirror's Basic_DAB_Channel run decode_frame, the serial decoder built from the
 * same pieces.  Plain C++17, header-only, no allocation, no table in memory; __host__ __device__ under hipcc.  A frame is
 * a callable `f(i)` = byte i, 0 <= i < L: nothing here reads outside [0, L).
 *
 * THE CONTRACT (ISO/IEC 11172-3 clauses 2.4.1.6, 2.4.2.6, 2.4.3.3 and Annex B tables B.1, B.2, B.4; ISO/IEC 13818-3 table
 * B.1 for ID = 0), every ambiguity decided.
 *
 * Input.  A GOOD frame of the follow call (dabgpu_mp2_frame.h): a header valid for the entry's rate and the chosen ID,
 * protection bit 0, ISO CRC good.  Shape s = frame_shape(header, id, B).  Layout: bits 0 .. 31 header, 32 .. 47 CRC, then
 * allocation, SCFSI, scale factors, samples.
 *
 * Cells.  A cell is a pair (sb, ch), sb < sblimit, ch < channels; stream order is sb-major, ch-minor.  Below the bound
 * every cell has its own allocation field of nbal(sb) bits; at or above the bound (two channels only) ONE field serves
 * both cells.  A cell is ACTIVE when its allocation index a is not 0.
 *
 * Quantisation classes.  The class of an active cell is its number of levels n, by table, sub-band and a = 1 .. 2^nbal - 1
 * (the table block below).  Classes 3, 5 and 9 are GROUPED: three samples share one code word of 5, 7 or 10 bits.  Every
 * other class n = 2^b - 1 carries three samples of b bits each.
 *
 * SCFSI.  Two bits per active cell, in stream order.  A shared allocation gives both cells their own SCFSI and their own
 * scale factors.
 *
 * Scale factors.  6-bit indices, in stream order per active cell.  A frame has three parts: granules 0-3, 4-7, 8-11.
 *     SCFSI 0: three indices sent: part 0 = first,  part 1 = second, part 2 = third
 *     SCFSI 1: two:                part 0 = first,  part 1 = first,  part 2 = second
 *     SCFSI 2: one:                part 0 = first,  part 1 = first,  part 2 = first
 *     SCFSI 3: two:                part 0 = first,  part 1 = second, part 2 = second
 * S[i] = 2^(1 - i/3) for i = 0 .. 62, computed as (float)C[i % 3] scaled exactly by 2^-(i / 3), C = {2, 2^(2/3), 2^(1/3)}
 * evaluated in double and rounded once to float.  Index 63 is forbidden by the standard; here it is factor 0 (the cell is
 * silent for that part), every SENT index that is 63 counts once in the level record's scf63, and the frame is still
 * decoded.
 *
 * Samples.  For granule g = 0 .. 11, for sb < sblimit, for each allocation field of that sub-band (one per channel below
 * the bound, one shared field at or above it), an active field carries
 *     grouped:   one code c;  s0 = c % n, s1 = (c / n) % n, s2 = (c / n^2) % n.  A code >= n^3 is decoded by exactly this
 *                arithmetic.
 *     otherwise: s0, s1, s2 of b bits each, most significant bit first.  The all-ones code is decoded as it comes.
 * A shared field's three codes serve both channels, each with its own scale factor.
 *
 * Value.  v = ((float)(2 s + 1 - n) * R[n]) * S[i], R[n] = (float)(1.0 / n) evaluated in double and rounded once: two IEEE
 * single-precision multiplications and no addition, so the value is the same bits on the device, in the host twin and in
 * numpy float32.  (2 s + 1 - n) / n equals the standard's C (s'' + D), s'' being the code with its most significant bit
 * inverted read as a two's complement fraction, for every class: for n = 2^b - 1, C = 2^b / n and D = 2^(1-b), so
 * C (s'' + D) = (2^b / n) (s - 2^(b-1) + 1) / 2^(b-1) = (2 s + 1 - n) / n; for the grouped classes 5 and 9 (b = 3, 4),
 * C = 2^b / n and D = 1/2 give (2^b / n) (s - 2^(b-2)) / 2^(b-1) = (2 s + 1 - n) / n as well.  Worked example, n = 3
 * (C = 4/3, D = 1/2), s = 0: code 00 -> 10 = -1, 4/3 (-1 + 1/2) = -2/3 = (0 + 1 - 3) / 3.
 * Sample index t = 3 g + k.  The output is v[ch][t][sb]; inactive cells and sb >= sblimit are 0, channel 1 of a
 * single-channel frame is 0.
 *
 * End of audio.  E = the bit position behind the last sample.  E > 8 (L - 6 - c) is an OVERRUN (the audio would run into
 * the ScF-CRC bytes or the fixed PAD): kind 2, all values 0, nothing past L is read.  Running out of bits while still in
 * the allocation, SCFSI or scale factors -- the end of any of them behind 8 (L - 6 - c) -- is the same overrun.  The
 * ScF-CRC stays unchecked, as the sibling contract says.
 *
 * Level record (32 bytes): int32 kind (0 decoded, 1 not a GOOD frame, 2 overrun), channels (0 when kind != 0), cells
 * (active cells), scf63; float power[2] (the sum over the channel's 1152 values of v^2, in any order, with or without fused
 * multiply-add), peak[2] (max |v|, exact).  Kind 1 and 2: everything behind kind is 0.  These are SUB-BAND-DOMAIN figures:
 * a full-scale sinusoid has a sub-band amplitude of about 1, and how they map to PCM dBFS is a convention nobody here has
 * measured.  Silence is power == 0, or a threshold the caller chooses.
 *
 * A slot of the follow call whose status says GOOD but whose header is not valid for the entry's rate and the chosen ID
 * (it cannot come out of the follow call) is kind 1.
 */
#ifndef DABGPU_MP2_AUDIO_H
#define DABGPU_MP2_AUDIO_H

#include <math.h>
#include <stdint.h>

#include "dabgpu_mp2_frame.h"

namespace dabgpu_mp2 {

/* ------------------------------------------------------------------------------------------------------------------
 * THE TABLE BLOCK: stated from the standards as known; one line each, so that one line can be corrected.  A row is the
 * levels of allocation index a = 1, 2, ... of the sub-bands it names, five bits a class, twelve classes a word.        */
struct LevelRow { uint64_t lo, hi; };
/* class code: 1, 2, 3 = the grouped classes 3, 5, 9; b + 1 = the class 2^b - 1 of b = 3 .. 16 bits a sample          */
constexpr int level_code(int n) {
    if (n == 3) return 1;
    if (n == 5) return 2;
    if (n == 9) return 3;
    int b = 0;
    while ((1 << b) - 1 < n) b++;
    return b + 1;
}
template <class... T>
constexpr LevelRow level_row(T... levels) {
    const int v[] = {levels...};
    LevelRow r = {0, 0};
    for (int i = 0; i < int(sizeof...(levels)); i++) {
        const uint64_t c = uint64_t(level_code(v[i]));
        if (i < 12) r.lo |= c << (5 * i); else r.hi |= c << (5 * (i - 12));
    }
    return r;
}
/* ISO 11172-3 table B.2a (48 kHz, the large table), sub-bands 0-2                                                    */
constexpr LevelRow LEVELS_48K_LARGE_0 = level_row(3, 7, 15, 31, 63, 127, 255, 511, 1023, 2047, 4095, 8191, 16383, 32767, 65535);
/*   ... sub-bands 3-10                                                                                                */
constexpr LevelRow LEVELS_48K_LARGE_3 = level_row(3, 5, 7, 9, 15, 31, 63, 127, 255, 511, 1023, 2047, 4095, 8191, 65535);
/*   ... sub-bands 11-22                                                                                               */
constexpr LevelRow LEVELS_48K_LARGE_11 = level_row(3, 5, 7, 9, 15, 31, 65535);
/*   ... sub-bands 23-26                                                                                               */
constexpr LevelRow LEVELS_48K_LARGE_23 = level_row(3, 5, 65535);
/* ISO 11172-3 table B.2c (48 kHz, the small table), sub-bands 0-1                                                    */
constexpr LevelRow LEVELS_48K_SMALL_0 = level_row(3, 5, 9, 15, 31, 63, 127, 255, 511, 1023, 2047, 4095, 8191, 16383, 32767);
/*   ... sub-bands 2-7                                                                                                 */
constexpr LevelRow LEVELS_48K_SMALL_2 = level_row(3, 5, 9, 15, 31, 63, 127);
/* ISO 13818-3 table B.1 (24 kHz), sub-bands 0-3                                                                      */
constexpr LevelRow LEVELS_24K_0 = level_row(3, 5, 7, 9, 15, 31, 63, 127, 255, 511, 1023, 2047, 4095, 8191, 16383);
/*   ... sub-bands 4-10                                                                                                */
constexpr LevelRow LEVELS_24K_4 = level_row(3, 5, 9, 15, 31, 63, 127);
/*   ... sub-bands 11-29                                                                                               */
constexpr LevelRow LEVELS_24K_11 = level_row(3, 5, 9);
/* the sub-bands at which the large table changes its row behind the first (the other tables change at t4 and t3)     */
constexpr int LARGE_ROW_1 = 3, LARGE_ROW_2 = 11, LARGE_ROW_3 = 23;
/* 2^(2/3) and 2^(1/3) in double                                                                                       */
constexpr double SCF_C1 = 1.5874010519681994, SCF_C2 = 1.2599210498948732;
/* ------------------------------------------------------------------------------------------------------------------ */

constexpr int GRANULES = 12, SAMPLES = 36, SUBBANDS = 32;
constexpr int FRAME_VALUES = 2 * SAMPLES * SUBBANDS;       /* v[2][36][32] */
enum AudioKind { AUDIO_DECODED = 0, AUDIO_NOT_GOOD = 1, AUDIO_OVERRUN = 2 };

struct Level {                 /* == dabgpu_mp2_level */
    int32_t kind, channels, cells, scf63;
    float power[2], peak[2];
};
static_assert(sizeof(Level) == 32, "record of the ABI");
struct AudioResult {           /* == dabgpu_mp2_audio_result */
    int32_t decoded, not_good, overrun, silent, reserved[4];
};
static_assert(sizeof(AudioResult) == 32, "record of the ABI");

/* the class n of allocation index a (1 .. 2^nbal - 1) in sub-band sb of table t */
DABGPU_MP2_FN int levels(const AllocTable &t, int sb, int a) {
    LevelRow r;
    if (t.sblimit == ALLOC_48K_LARGE.sblimit)
        r = sb < LARGE_ROW_1 ? LEVELS_48K_LARGE_0 : sb < LARGE_ROW_2 ? LEVELS_48K_LARGE_3 : sb < LARGE_ROW_3 ? LEVELS_48K_LARGE_11 : LEVELS_48K_LARGE_23;
    else if (t.sblimit == ALLOC_48K_SMALL.sblimit)
        r = sb < t.t4 ? LEVELS_48K_SMALL_0 : LEVELS_48K_SMALL_2;
    else
        r = sb < t.t4 ? LEVELS_24K_0 : sb < t.t3 ? LEVELS_24K_4 : LEVELS_24K_11;
    const int c = int(((a <= 12 ? r.lo >> (5 * (a - 1)) : r.hi >> (5 * (a - 13)))) & 31);
    return c == 1 ? 3 : c == 2 ? 5 : c == 3 ? 9 : (1 << (c - 1)) - 1;
}
DABGPU_MP2_FN bool grouped(int n) { return n == 3 || n == 5 || n == 9; }
/* bits of one sample of an ungrouped class n = 2^b - 1 | of the code word of a grouped one */
DABGPU_MP2_FN int sample_bits(int n) {
    int b = 2;
    while ((1 << b) - 1 < n) b++;
    return b;
}
DABGPU_MP2_FN int code_bits(int n) { return n == 3 ? 5 : n == 5 ? 7 : 10; }
/* bits an active field of class n takes in one granule */
DABGPU_MP2_FN int field_bits(int n) { return grouped(n) ? code_bits(n) : 3 * sample_bits(n); }
/* the three samples of a grouped code word (n is 3, 5 or 9: divisions by constants) */
DABGPU_MP2_FN void group_split(uint32_t c, int n, uint32_t s[3]) {
    if (n == 3) { s[0] = c % 3; s[1] = (c / 3) % 3; s[2] = (c / 9) % 3; }
    else if (n == 5) { s[0] = c % 5; s[1] = (c / 5) % 5; s[2] = (c / 25) % 5; }
    else { s[0] = c % 9; s[1] = (c / 9) % 9; s[2] = (c / 81) % 9; }
}
/* R[n] */
DABGPU_MP2_FN float recip(int n) { return float(1.0 / double(n)); }
/* S[i], 0 for the forbidden index 63 */
DABGPU_MP2_FN float scale_factor(int i) {
    if (i >= 63) return 0.0f;
    const float c = i % 3 == 0 ? 2.0f : i % 3 == 1 ? float(SCF_C1) : float(SCF_C2);
    return ldexpf(c, -(i / 3));
}
DABGPU_MP2_FN float value(uint32_t s, int n, float r, float scf) { return (float(2 * int(s) + 1 - n) * r) * scf; }
/* which of the indices sent (0, 1, 2) holds in part p (0, 1, 2), and how many are sent */
DABGPU_MP2_FN int scf_sent(int scfsi) { return scfsi == 0 ? 3 : scfsi == 2 ? 1 : 2; }
DABGPU_MP2_FN int scf_of_part(int scfsi, int p) {
    return scfsi == 0 ? p : scfsi == 1 ? (p == 2 ? 1 : 0) : scfsi == 2 ? 0 : (p == 0 ? 0 : 1);
}

/* allocation bits of the sub-bands below sb of ONE channel's worth of fields (sb <= sblimit) */
DABGPU_MP2_FN int nbal_below(const AllocTable &t, int sb) {
    const int a = sb < t.t4 ? sb : t.t4, b = sb < t.t3 ? sb : t.t3;
    return 4 * a + 3 * (b - a) + 2 * (sb - b);
}
/* bit position of the allocation field of cell (sb, ch); sb = sblimit, ch = 0: the end of the allocation */
DABGPU_MP2_FN int alloc_position(const Shape &s, int sb, int ch) {
    int pos = 48 + nbal_below(s.t, sb);
    if (s.channels == 2) pos += nbal_below(s.t, sb < s.bound ? sb : s.bound) + (ch == 1 && sb < s.bound ? nbal(s.t, sb) : 0);
    return pos;
}
/* the bit position the audio must end in front of */
DABGPU_MP2_FN int audio_limit(int L, int c) { return 8 * (L - 6 - c); }

/* n (1 .. 16) bits at bit position pos, most significant first; the caller has checked pos + n <= 8 L */
template <class Bytes>
DABGPU_MP2_FN uint32_t get_bits_wide(const Bytes &f, int pos, int n) {
    const int at = pos >> 3, in = pos & 7;
    uint32_t v = uint32_t(f(at)) << 16;
    if (in + n > 8) v |= uint32_t(f(at + 1)) << 8;
    if (in + n > 16) v |= f(at + 2);
    return (v >> (24 - in - n)) & ((1u << n) - 1);
}

DABGPU_MP2_FN Level empty_level(int kind) {
    Level lv = {kind, 0, 0, 0, {0.0f, 0.0f}, {0.0f, 0.0f}};
    return lv;
}

/* The serial decoder.  One frame of L bytes whose header word h is valid for (id, B) and whose ISO CRC the caller found
 * good -> its level record; v: nullptr, or the frame's FRAME_VALUES values v[ch][t][sb], all written (zeros for kind 2). */
template <class Bytes>
DABGPU_MP2_FN Level decode_frame(const Bytes &f, int L, int B, int id, float *v) {
    if (v) for (int i = 0; i < FRAME_VALUES; i++) v[i] = 0.0f;
    if (L < 4) return empty_level(AUDIO_NOT_GOOD);
    const uint32_t h = header_word(f(0), f(1), f(2), f(3));
    if (header_id(h, B) != id) return empty_level(AUDIO_NOT_GOOD);
    const Shape s = frame_shape(h, id, B);
    const int limit = audio_limit(L, s.c);
    int pos = alloc_position(s, s.t.sblimit, 0);
    if (pos > limit) return empty_level(AUDIO_OVERRUN);
    uint8_t n_of[2][SUBBANDS] = {}, scfsi[2][SUBBANDS] = {}, scf[2][SUBBANDS][3] = {};   /* class (0: inactive; 16 bits: 0xFF) */
    int cells = 0;
    for (int sb = 0; sb < s.t.sblimit; sb++)
        for (int ch = 0; ch < s.channels; ch++) {
            const int a = int(get_bits(f, alloc_position(s, sb, ch), nbal(s.t, sb)));
            const int n = a ? levels(s.t, sb, a) : 0;
            n_of[ch][sb] = uint8_t(n == 0 ? 0 : grouped(n) ? n : 0x80 | sample_bits(n));
            cells += a != 0;
        }
    if (pos + 2 * cells > limit) return empty_level(AUDIO_OVERRUN);
    int sent = 0;
    for (int sb = 0; sb < s.t.sblimit; sb++)
        for (int ch = 0; ch < s.channels; ch++)
            if (n_of[ch][sb]) {
                scfsi[ch][sb] = uint8_t(get_bits(f, pos, 2));
                sent += scf_sent(scfsi[ch][sb]);
                pos += 2;
            }
    if (pos + 6 * sent > limit) return empty_level(AUDIO_OVERRUN);
    Level lv = empty_level(AUDIO_DECODED);
    for (int sb = 0; sb < s.t.sblimit; sb++)
        for (int ch = 0; ch < s.channels; ch++)
            if (n_of[ch][sb]) {
                uint8_t idx[3] = {0, 0, 0};
                for (int j = 0; j < scf_sent(scfsi[ch][sb]); j++, pos += 6) {
                    idx[j] = uint8_t(get_bits_wide(f, pos, 6));
                    lv.scf63 += idx[j] == 63;
                }
                for (int p = 0; p < 3; p++) scf[ch][sb][p] = idx[scf_of_part(scfsi[ch][sb], p)];
            }
    auto class_of = [&](int ch, int sb) { const int q = n_of[ch][sb]; return q & 0x80 ? (1 << (q & 0x7F)) - 1 : q; };
    int granule = 0;
    for (int sb = 0; sb < s.t.sblimit; sb++)
        for (int ch = 0; ch < (s.channels == 2 && sb < s.bound ? 2 : 1); ch++)
            if (n_of[ch][sb]) granule += field_bits(class_of(ch, sb));
    if (pos + GRANULES * granule > limit) {
        lv.scf63 = 0;
        lv.kind = AUDIO_OVERRUN;
        return lv;
    }
    lv.channels = s.channels;
    lv.cells = cells;
    for (int g = 0; g < GRANULES; g++)
        for (int sb = 0; sb < s.t.sblimit; sb++)
            for (int fch = 0; fch < (s.channels == 2 && sb < s.bound ? 2 : 1); fch++) {
                if (!n_of[fch][sb]) continue;
                const int n = class_of(fch, sb);
                uint32_t smp[3];
                if (grouped(n)) {
                    group_split(get_bits_wide(f, pos, code_bits(n)), n, smp);
                    pos += code_bits(n);
                } else {
                    const int b = sample_bits(n);
                    for (int k = 0; k < 3; k++, pos += b) smp[k] = get_bits_wide(f, pos, b);
                }
                const bool shared = s.channels == 2 && sb >= s.bound;
                for (int ch = fch; ch < (shared ? 2 : fch + 1); ch++) {
                    const float r = recip(n), sf = scale_factor(scf[ch][sb][g >> 2]);
                    for (int k = 0; k < 3; k++) {
                        const float x = value(smp[k], n, r, sf);
                        if (v) v[(ch * SAMPLES + 3 * g + k) * SUBBANDS + sb] = x;
                        lv.power[ch] += x * x;
                        const float m = x < 0 ? -x : x;
                        if (m > lv.peak[ch]) lv.peak[ch] = m;
                    }
                }
            }
    return lv;
}

}  // namespace dabgpu_mp2

#endif
