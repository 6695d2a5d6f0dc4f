/* dabgpu_packet_fec_erasures.h -- RS(204,188) correction of packet-mode FEC frames with the failed packet CRCs as erasures.
 *
 * The contract is the section "Erasures" at the top of dabgpu_packet_fec.h; this is its one implementation: the kernels behind
 * dabgpu_packet_fec_erasures_dev, the host twin dabgpu_packet_fec_erasures_host and the host mirror's
 * Basic_Data_Packet_Channel all run this code.  Plain C++17, header-only, no allocation; __host__ __device__ under hipcc.
 * Everything of the errors-only call is used as it is (marks, frames, syndromes, Berlekamp-Massey, pattern_holds): a row that
 * call corrects is corrected here by the same functions.  The slot scan is dabgpu_packet_walk.h's slot_verdict.
 */
#ifndef DABGPU_PACKET_FEC_ERASURES_H
#define DABGPU_PACKET_FEC_ERASURES_H

#include "dabgpu_packet_fec.h"
#include "dabgpu_packet_walk.h"

namespace dabgpu_packet_fec {

constexpr uint32_t ERASURE_MAGIC = 0x45454650u;   /* "PFEE" */
constexpr int MAX_ERASED = T2;                    /* f beyond this: frames_beyond_erasures */
constexpr int ERASURE_MARGIN = 2;                 /* e >= 1 only when 2 e + f <= T2 - ERASURE_MARGIN */
constexpr int SUSPECT_BYTES = 32;                 /* Head::reserved: a suspect bit per carried slot */

/* the carried slots D S of every S fit the head's reserved bytes */
constexpr int most_carried_slots() {
    int most = 0;
    for (int S = 1; S <= MAX_SLOTS; S++) {
        const int D = (FRAME_SLOTS - 1 + S - 1) / S;
        most = D * S > most ? D * S : most;
    }
    return most;
}
static_assert(most_carried_slots() == 150 && most_carried_slots() <= 8 * SUSPECT_BYTES && sizeof(Head::reserved) == SUSPECT_BYTES,
              "a suspect bit per carried slot in the head");

struct ErasureCounters {                  /* == dabgpu_packet_fec_erasure_result */
    Counters c;                           /* as the errors-only call counts them */
    int32_t slots_suspect;                /* among the call's new slots */
    int32_t frames_with_suspects;         /* accepted frames with f >= 2 */
    int32_t frames_beyond_erasures;       /* of those, f > 16 */
    int32_t rows_erasure_corrected;
    int32_t erased_bytes_changed, erasure_other_bytes_corrected;
    int32_t reserved2[2];
};
static_assert(sizeof(ErasureCounters) == 80, "record of the ABI");

/* n <= 64 bits from bit `at` of p, and back */
DABGPU_FEC_FN uint64_t get_bits(const uint8_t *p, int at, int n) {
    uint64_t v = 0;
    for (int i = 0; i < n; i++) v |= uint64_t((p[(at + i) >> 3] >> ((at + i) & 7)) & 1u) << i;
    return v;
}
DABGPU_FEC_FN void put_bits(uint8_t *p, int at, int n, uint64_t v) {
    for (int i = 0; i < n; i++)
        if ((v >> i) & 1u) p[(at + i) >> 3] = uint8_t(p[(at + i) >> 3] | (1u << ((at + i) & 7)));
}

DABGPU_FEC_FN void head_fresh_erasures(Head &h, int S) {
    head_fresh(h, S);
    h.magic = ERASURE_MAGIC;
}
/* a record the erasure call wrote for S slots a frame: bit i of `reserved` is carried slot i; none beyond D S, none in a
 * padding frame */
DABGPU_FEC_FN bool head_ok_erasures(const Head &h, int S) {
    bool ok = head_written(h, S, ERASURE_MAGIC);
    if (!ok) return false;
    const int D = delay(S), used = D * S;
    const int padding = h.frames_seen < D ? int(D - h.frames_seen) * S : 0;
    for (int i = 0; i < SUSPECT_BYTES; i++) {
        int lo = padding - 8 * i, hi = used - 8 * i;
        lo = lo < 0 ? 0 : lo > 8 ? 8 : lo;
        hi = hi < 0 ? 0 : hi > 8 ? 8 : hi;
        const unsigned allowed = hi > lo ? ((1u << hi) - 1u) & ~((1u << lo) - 1u) : 0u;
        ok = ok && (h.reserved[i] & ~allowed) == 0;
    }
    return ok;
}

/* The suspect slots of one logical frame as received: verdict(pos) is dabgpu_packet::slot_verdict(frame, S, pos, 1) */
template <class Verdict> DABGPU_FEC_FN uint64_t suspects_of_chain(int S, Verdict verdict) {
    uint64_t bits = 0;
    for (int pos = 0; pos < S;) {
        const uint32_t v = verdict(pos);
        const int kind = dabgpu_packet::verdict_kind(v);
        if (kind == int(dabgpu_packet::SLOT_BAD)) bits |= uint64_t(1) << pos;
        pos += kind == int(dabgpu_packet::SLOT_GOOD) ? dabgpu_packet::verdict_slots(v) : 1;
    }
    return bits;
}
DABGPU_FEC_FN uint64_t suspects_of(const uint8_t *frame, int S) {
    return suspects_of_chain(S, [&](int pos) { return dabgpu_packet::slot_verdict(frame, S, pos, 1); });
}

/* ---- the rows: erasures E shared by the twelve rows of a frame */
struct alignas(8) ErasureSet {
    uint64_t slots[2];                    /* bit i: table slot i (0..93) is suspect */
    int32_t f;                            /* 2 x the suspect table slots */
    uint8_t G[T2 + 1];                    /* prod over E of (1 + alpha^(203 - c) x); only when 2 <= f <= 16 */
};
DABGPU_FEC_FN bool erased(const ErasureSet &e, int c) { return c < K && ((e.slots[c >> 7] >> ((c >> 1) & 63)) & 1u) != 0; }
/* step 3 is open to the rows of this frame */
DABGPU_FEC_FN bool erasures_usable(const ErasureSet &e) { return e.f >= 2 && e.f <= MAX_ERASED; }

/* e.slots is set: f, and the erasure locator when it will be used */
DABGPU_FEC_FN void erasure_locator(const Gf &g, ErasureSet &e) {
    int n = 0;
    for (int i = 0; i < DATA_SLOTS; i++) n += int((e.slots[i >> 6] >> (i & 63)) & 1u);
    e.f = 2 * n;
    for (int i = 0; i <= T2; i++) e.G[i] = 0;
    e.G[0] = 1;
    if (!erasures_usable(e)) return;
    int deg = 0;
    for (int c = 0; c < K; c++) {
        if (!erased(e, c)) continue;
        const unsigned X = g.exp[N - 1 - c];
        deg++;
        for (int j = deg; j >= 1; j--) e.G[j] = uint8_t(e.G[j] ^ gmul(g, e.G[j - 1], X));
    }
}

struct ErasureWork {                      /* on the device in LDS, as RowWork */
    uint8_t Ts[T2];                       /* the modified syndromes above f */
    uint8_t L[T2 + 1], B[T2 + 1], Tm[T2 + 1];   /* Berlekamp-Massey's; then L is the errata locator */
    uint8_t Om[T2];                       /* errata evaluator */
    uint8_t pos[T2], val[T2];             /* the pattern: codeword positions and values (in E they may be zero) */
    int32_t deg, e, n;                    /* the errata locator's degree; the error locator's; roots found */
};

/* Modified syndromes, Berlekamp-Massey on those above f, errata locator and evaluator; false: no pattern within the bound */
DABGPU_FEC_FN bool errata_locator(const Gf &g, const ErasureSet &es, const uint8_t *syn, ErasureWork &w) {
    const int f = es.f, M = T2 - f;
    w.deg = w.e = w.n = 0;
    for (int k = f; k < T2; k++) {
        unsigned t = 0;
        for (int j = 0; j <= f; j++) t ^= gmul(g, es.G[j], syn[k - j]);
        w.Ts[k - f] = uint8_t(t);
    }
    for (int i = 0; i <= T2; i++) w.L[i] = w.B[i] = 0;
    w.L[0] = w.B[0] = 1;
    int ll = 0, m = 1;
    unsigned bb = 1;
    for (int n = 0; n < M; n++) {
        unsigned d = w.Ts[n];
        for (int i = 1; i <= ll && i <= n; i++) d ^= gmul(g, w.L[i], w.Ts[n - i]);
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
    if (ll > 0 && 2 * ll + f > T2 - ERASURE_MARGIN) return false;
    w.e = ll;
    w.deg = ll + f;                       /* <= 16 */
    for (int i = 0; i <= T2; i++) w.Tm[i] = 0;
    for (int i = 0; i <= ll; i++)
        for (int j = 0; j <= f; j++) w.Tm[i + j] ^= uint8_t(gmul(g, w.L[i], es.G[j]));
    for (int i = 0; i <= T2; i++) w.L[i] = w.Tm[i];
    for (int i = 0; i < w.deg; i++) {
        unsigned v = 0;
        for (int j = 0; j <= i; j++) v ^= gmul(g, w.L[j], syn[i - j]);
        w.Om[i] = uint8_t(v);
    }
    return true;
}

/* is codeword position c a root of the errata locator, and with which value (Forney) */
DABGPU_FEC_FN bool errata_root_at(const Gf &g, const ErasureWork &w, int c, unsigned &value) {
    const int p = N - 1 - c, xinv = (255 - p) % 255;
    unsigned ev = 0;
    for (int j = 0; j <= w.deg; j++) ev ^= gscale(g, w.L[j], xinv * j);
    if (ev) return false;
    unsigned om = 0, dl = 0;
    for (int j = 0; j < w.deg; j++) om ^= gscale(g, w.Om[j], xinv * j);
    for (int j = 1; j <= w.deg; j += 2) dl ^= gscale(g, w.L[j], xinv * (j - 1));
    value = dl ? gmul(g, g.exp[p], gdiv(g, om, dl)) : 0u;
    return true;
}

/* the pattern held to the definition: its 16 syndromes are the row's, all of E and e more positions, those non-zero, within
 * the bound (the search visits every position once, so they are distinct) */
DABGPU_FEC_FN bool errata_holds(const Gf &g, const ErasureSet &es, const uint8_t *syn, const ErasureWork &w) {
    if (!erasures_usable(es) || w.deg < es.f || w.deg > T2 || w.n != w.deg) return false;
    int outside = 0;
    for (int i = 0; i < w.n; i++) {
        if (w.pos[i] >= N) return false;
        if (erased(es, w.pos[i])) continue;
        if (!w.val[i]) return false;
        outside++;
    }
    if (outside != w.deg - es.f || (outside > 0 && 2 * outside + es.f > T2 - ERASURE_MARGIN)) return false;
    for (int k = 0; k < T2; k++) {
        unsigned s = 0;
        for (int i = 0; i < w.n; i++) s ^= gscale(g, w.val[i], k * (N - 1 - w.pos[i]));
        if (s != syn[k]) return false;
    }
    return true;
}

struct ErasureFrameCounts {
    FrameCounts f;
    int32_t rows_erasure_corrected, erased_bytes_changed, erasure_other_bytes_corrected;
};
static_assert(sizeof(ErasureFrameCounts) == 32, "eight words");
/* a row the errors-only rule left (count_row has not seen it): step 3's verdict */
DABGPU_FEC_FN void count_erasure_row(const ErasureSet &es, const ErasureWork &w, bool holds, ErasureFrameCounts &f) {
    if (!holds) {
        f.f.rows_uncorrectable++;
        return;
    }
    f.rows_erasure_corrected++;
    for (int i = 0; i < w.n; i++) {
        if (!w.val[i]) continue;
        (erased(es, w.pos[i]) ? f.erased_bytes_changed : f.erasure_other_bytes_corrected)++;
    }
}

/* ---- the host path */

/* One FEC frame whose slot i (0..102) is the 24 bytes at slot(i), suspect(i) the suspect bit of table slot i (0..93) */
template <class Slot, class Suspect> inline void correct_frame_erasures(const Gf &g, Slot slot, Suspect suspect, ErasureCounters &c) {
    uint8_t fr[FRAME_BYTES];
    load_frame(slot, fr);
    ErasureSet es = {};
    for (int i = 0; i < DATA_SLOTS; i++)
        if (suspect(i)) {
            es.slots[i >> 6] |= uint64_t(1) << (i & 63);
            es.f += 2;
        }
    bool located = false;                 /* the locator is made for the first row that needs it */
    c.frames_with_suspects += es.f >= 2;
    c.frames_beyond_erasures += es.f > MAX_ERASED;
    ErasureFrameCounts f = {};
    for (int r = 0; r < ROWS; r++) {
        RowWork w;
        bool codeword;
        const bool holds = decode_row(g, fr, r, w, codeword);
        if (codeword || holds || !erasures_usable(es)) {
            count_row(w, codeword, holds, f.f);
            if (holds) write_back(slot, fr, r, w.pos, w.val, w.n);
            continue;
        }
        if (!located) erasure_locator(g, es);
        located = true;
        ErasureWork ew;
        bool eholds = false;
        if (errata_locator(g, es, w.syn, ew)) {
            for (int col = 0; col < N; col++) {
                unsigned v;
                if (!errata_root_at(g, ew, col, v)) continue;
                if (ew.n < T2) {
                    ew.pos[ew.n] = uint8_t(col);
                    ew.val[ew.n] = uint8_t(v);
                }
                ew.n++;
            }
            eholds = errata_holds(g, es, w.syn, ew);
        }
        count_erasure_row(es, ew, eholds, f);
        if (eholds) write_back(slot, fr, r, ew.pos, ew.val, ew.n);
    }
    add_counts(c.c, f.f);
    c.rows_erasure_corrected += f.rows_erasure_corrected;
    c.erased_bytes_changed += f.erased_bytes_changed;
    c.erasure_other_bytes_corrected += f.erasure_other_bytes_corrected;
}

/* One entry of a call: the twin of the erasure kernels, with the arguments of process() and its window functions.  A record
 * process() wrote is a fresh start here, and the other way round. */
inline void process_erasures(const Gf &g, const uint8_t *state_in, uint8_t *state_out, ErasureCounters &c, const uint8_t *in, uint64_t in_stride,
                             int n, int S, uint8_t *out, uint64_t out_stride) {
    const Window w = {state_in, state_out, in, in_stride, n, S, out, out_stride};
    const int D = delay(S);
    Head h;
    move_window(w, start_head(h, state_in, S, head_ok_erasures, head_fresh_erasures));
    c = ErasureCounters{};
    c.c.cifs = n;
    c.c.slots = n * S;
    /* the suspect words of the last D + 1 window frames, window frame wf at wf % (D + 1): a frame that ends in new frame k
     * began at most D frames before it */
    uint64_t ring[FRAME_SLOTS];
    const int R = D + 1;
    for (int wf = 0; wf < D; wf++) ring[wf % R] = get_bits(h.reserved, wf * S, S);
    for (int64_t j = 0, first; j < int64_t(n) * S; j++) {
        if (j % S == 0) {
            const uint64_t word = suspects_of(in + uint64_t(j / S) * in_stride, S);
            ring[(D + j / S) % R] = word;
            for (int i = 0; i < S; i++) c.slots_suspect += int((word >> i) & 1u);
        }
        if (!frame_ends(w, h, c.c, j, first)) continue;
        correct_frame_erasures(
            g, [&](int i) { return w.slot(first + i); }, [&](int i) { return ((ring[((first + i) / S) % R] >> ((first + i) % S)) & 1u) != 0; }, c);
    }
    uint8_t bits[SUSPECT_BYTES] = {};
    for (int k = 0; k < D; k++) put_bits(bits, k * S, S, ring[(int64_t(n) + k) % R]);
    for (int i = 0; i < SUSPECT_BYTES; i++) h.reserved[i] = bits[i];
    store_head(h, w);
}

}  /* namespace dabgpu_packet_fec */
#endif
