/* dabgpu_dmb.h -- T-DMB stream-mode sub-channels (ETSI TS 102 427): the MPEG-2 transport stream of a stream-mode data
 * sub-channel (FIG 0/2, TMId 1, DSCTy 24), from its logical frames to checked 188-byte TS packets.
 *
 * One implementation of the contract below: the kernels behind dabgpu_dmb_follow_dev, the host twin dabgpu_dmb_follow_host and
 * the stand-alone fuzz program (tests/dmb_fuzz.cpp) all run this code.  Plain C++17, header-only, no allocation;
 * __host__ __device__ under hipcc.  The outer code is the RS(204,188) of dabgpu_packet_fec.h: its syndrome_add, locator,
 * root_at, pattern_holds and Gf tables are used here, not copied.
 *
 * PARITY WITH OTHER DMB TOOLS IS NOT PINNED: no DMB multiplexer or receiver was at hand when this was written.  Every constant
 * taken from a standard stands on one line below, so that a wrong one is corrected in one place:
 */
#ifndef DABGPU_DMB_H
#define DABGPU_DMB_H

#include "dabgpu_packet_fec.h"

namespace dabgpu_dmb {

namespace fec = dabgpu_packet_fec;

constexpr int SYNC_BYTE = 0x47;           /* ISO/IEC 13818-1: the first byte of every TS packet                               */
constexpr int TS_BYTES = 188;             /* ISO/IEC 13818-1: a TS packet                                                     */
constexpr int CODED_BYTES = 204;          /* TS 102 427: a TS packet and 16 bytes of RS(204,188)                              */
constexpr int BRANCHES = 12;              /* TS 102 427: branches of the convolutional byte interleaver                       */
constexpr int BRANCH_CELLS = 17;          /* TS 102 427: branch j is a FIFO of 17 j cells, so it delays by 12 * 17 j = 204 j  */
constexpr int NULL_PID = 0x1FFF;          /* ISO/IEC 13818-1: null packets, exempt from the continuity rules                  */
constexpr int LOCK_RUN = 5;               /* THIS PROJECT'S CHOICE: sync bytes in a row, 204 apart, that lock                 */
constexpr int LOSS_MISSES = 8;            /* THIS PROJECT'S CHOICE: missing sync bytes in a row, at the locked phase, that unlock */

/* THE CONTRACT of one entry (a stream-mode sub-channel) in one call, every ambiguity decided.  Where this text and a
 * standard's wording could part, this text governs.
 *
 * Input.  The logical frames of 3 R bytes (R the bit rate in kbit/s, a multiple of 8 in 8 .. 1824 -- 1824 = 32 x 57 at protection level 4-B takes
 * 855 of the CIF's 864 capacity units: the largest rate of a sub-channel the decode call accepts), concatenated in
 * order across frames and calls: one byte stream y[p], p = 0, 1, ... from a fresh start.  Packets do not align with frames.
 *
 * Sync.  hit(p) <=> y[p] == 0x47.  run(p) = hit(p) ? min(run(p - 204) + 1, 255) : 0, run = 0 below p = 0: a function of the
 * bytes alone, kept for all 204 phases whatever the lock does.  While unlocked the receiver locks at the smallest p, at or
 * after the position where the search began (0, or one past a loss), with run(p) >= LOCK_RUN.  The lock's START is that p;
 * its phase is p mod 204.  While locked only the positions START + 204 k, k >= 1, are looked at: a hit clears the miss count,
 * a miss raises it, and at the LOSS_MISSES-th miss in a row the lock is lost AT that position, its END; the search resumes
 * at END + 1 (with the run counters as the bytes made them, so another phase can lock at once).  A lock therefore spans
 * [START, END), END - START a multiple of 204 and at least 8 x 204.
 *   sync_hits counts, among the call's bytes, the lock positions and the hits looked at while locked; locks and lock_losses
 *   count the STARTs and ENDs among the call's bytes.
 *
 * Packets.  Every position s = START + 204 k inside [START, END) starts a coded packet, whether y[s] is a hit or not (the outer
 * code restores a damaged sync byte).  In the transmitter byte i of coded packet n goes through branch i mod 12, a FIFO that
 * delays it by 204 (i mod 12) positions; the sync byte goes through branch 0.  Hence
 *     x[i] = y[s + 204 (i mod 12) + i],  i = 0 .. 203:
 * de-interleaving is a gather and needs no FIFO.  The packet is complete when y[s + 2447] has arrived and is emitted in the
 * call that brings that byte.  It is emitted only if its lock is still held at s + 2244 (s + 2244 < END: the position where
 * its last branch begins); the others -- the last min(11, all) packets of a lock that ends -- are counted as packets_dropped
 * in the call that brings END.  Emitted packets keep stream order.
 *
 * Outer code.  x[0 .. 203] is one row of dabgpu_packet_fec.h's RS(204,188): GF(2^8), x^8 + x^4 + x^3 + x^2 + 1, alpha = 2,
 * generator prod_{i=0..15} (x + alpha^i), x[0] the coefficient of x^203.  Bounded-distance decoding, errors only: if a
 * codeword lies within Hamming distance 8 of x it replaces x (status 1, corrected_data = differing positions below 188,
 * corrected_parity = the others); x a codeword: status 0; otherwise status 2, x stays as received and the
 * transport_error_indicator is set in the output (byte 1 |= 0x80).
 *
 * Output.  The first 188 bytes of every emitted packet, back to back in d_ts, and a Record per packet in d_records.  PID, the
 * fourth byte (transport_scrambling_control, adaptation_field_control, continuity_counter) and the discontinuity flag of
 * the record are those of the 188 bytes as written out (for status 2: as received).
 *
 * Continuity and PID census (ISO/IEC 13818-1 clause 2.4.3.3, restated).  Packets of status 2 take no part.  For every other
 * ("good") packet, in stream order: its PREVIOUS packet is the last good packet of the same PID, in this call or any earlier
 * one.  The packet is judged when it has a previous packet, its PID is not 0x1FFF, and it is not EXEMPT (adaptation field
 * present -- adaptation_field_control bit 1 -- with adaptation_field_length >= 1 and discontinuity_indicator set).  Judged
 * with payload (adaptation_field_control bit 0): counter == previous + 1 mod 16 is in order; counter == previous counts as
 * duplicates (every repetition, not only the first); anything else as discontinuities.  Judged without payload: a counter
 * that differs from previous counts as discontinuities.  Whatever the verdict, the packet becomes the previous packet of
 * its PID.  The census lists the first 32 distinct PIDs of good packets in the order they first appeared (0x1FFF included),
 * each with cumulative counts of packets, discontinuities, duplicates and scrambled packets (transport_scrambling_control
 * != 0); pids_overflowed counts the distinct PIDs that appeared when the list was full.
 *
 * State.  One opaque record of STATE_BYTES: a head (magic, bit rate, stream position, the lock, the deferred count), the 204 run
 * counters, the last 2447 + 203 bytes of the stream (a packet one byte short of complete began 2447 bytes ago; the 203 beyond
 * that are carried and not read), the census, the last counter of all 8192 PIDs (0xFF: none yet) and the deferred packets.  NULL, all zero, or a record head_ok() does not know for this bit rate: a fresh start.
 * THE OUTPUT OF A STREAM DOES NOT DEPEND ON WHERE IT IS CUT INTO CALLS, calls of no frames and of fewer bytes than a packet
 * included: packets, records, census and final state are equal, and the counters of the calls add up to the same sums.
 *
 * Buffers and deferral.  A call of n frames completes at most new_packets(R, n) = ceil(3 R n / 204) packets (two packets lie at
 * least 204 bytes apart, also across locks).  The caller gives room for `capacity` packets, any number from 0.  The packets of
 * a call are those the state record holds deferred, in their order, then the completed ones, in stream order; the first
 * `capacity` of them are EMITTED: written to d_ts / d_records, counted by status, and taken through continuity and census --
 * all of that happens at emission, so records, counters and census do not depend on when a packet was emitted.  The next up
 * to DEFER_ROOM = 64 are DEFERRED: kept in the new state record as they would have been written (188 bytes and the record)
 * and emitted first by the next call; packets_deferred says how many the new record holds.  Whatever is beyond that is LOST
 * and counted as packets_lost: cut independence holds for a stream as long as nothing was lost, which a caller has in hand --
 * max_packets(R, n) = new_packets(R, n) + DEFER_ROOM always holds everything.  (DECIDED HERE: the issue lets deferral be
 * unbounded; a state record of fixed size cannot.)
 *
 * Not provided: anything inside the TS (PSI, PES, SL, OD, BIFS, video); erasure decoding from the channel decoder's
 * reliability; stream-mode data of another DSCTy; the transmit side.
 */

constexpr int N = fec::N, K = fec::K, T = fec::T, T2 = fec::T2;
constexpr int SPAN = CODED_BYTES * (BRANCHES - 1) + CODED_BYTES;   /* 2448: a packet lies in y[s .. s + 2447]                   */
constexpr int LAST_BRANCH_AT = CODED_BYTES * (BRANCHES - 1);       /* 2244                                                      */
constexpr int TAIL_BYTES = SPAN - 1 + CODED_BYTES - 1;             /* 2447 + 203 carried bytes: y[P - 2650 .. P - 1]            */
constexpr int TAIL_ROOM = (TAIL_BYTES + 15) & ~15;                 /* 2656                                                      */
constexpr int DEFER_ROOM = 64;            /* deferred packets a state record holds                                              */
constexpr int MAX_KBPS = 1824, MAX_N_CIFS = 1 << 16;               /* bytes of a call = 3 R n stays far below 2^31              */
constexpr int CENSUS = 32, PIDS = 8192;
constexpr uint8_t NO_COUNTER = 0xFF;
constexpr uint32_t MAGIC = 0x31424D44u;   /* "DMB1" */
constexpr int64_t MAX_POS = int64_t(1) << 56;
constexpr int64_t NEVER = int64_t(1) << 62;

static_assert(N == CODED_BYTES && K == TS_BYTES && BRANCHES * BRANCH_CELLS == CODED_BYTES && SPAN == 2448, "the outer code is the packet FEC's");

enum Status : uint8_t { AS_RECEIVED = 0, CORRECTED = 1, UNCORRECTABLE = 2 };
enum RecordFlags : uint8_t { FLAG_EXEMPT = 1 };   /* a set discontinuity_indicator in an adaptation field of length >= 1 */

struct alignas(16) Record {               /* == dabgpu_dmb_record */
    uint8_t status;                       /* Status */
    uint8_t corrected_data, corrected_parity;
    uint8_t byte3;                        /* scrambling control << 6 | adaptation_field_control << 4 | continuity_counter */
    uint16_t pid;
    uint8_t flags;                        /* RecordFlags */
    uint8_t reserved;
    uint32_t position;                    /* s modulo 2^32 */
    uint32_t reserved2;
};

struct Result {                           /* == dabgpu_dmb_result: counts of THIS call, then where the stream stands */
    int32_t cifs, bytes, sync_hits, locks, lock_losses;
    int32_t packets_emitted, packets_clean, packets_corrected, packets_uncorrectable, packets_dropped;
    int32_t bytes_corrected, parity_bytes_corrected;
    int32_t discontinuities, duplicates;
    int32_t locked, phase;                /* at the end of the call; phase -1 when unlocked */
    int32_t pids, pids_overflowed;        /* cumulative: census entries in use, distinct PIDs beyond them */
    int32_t packets_deferred;             /* held in the new state record, emitted first by the next call */
    int32_t packets_lost;                 /* of THIS call: beyond the room and beyond DEFER_ROOM */
};
constexpr int SUMMED_COUNTERS = 14;       /* cifs .. duplicates: the counts of a call that add up over calls (packets_lost does too) */

struct CensusEntry {
    uint16_t pid, reserved;
    uint32_t packets, discontinuities, duplicates, scrambled;
};

struct alignas(16) Head {
    uint32_t magic;
    int32_t kbps;
    int64_t pos;                          /* P: bytes since the fresh start */
    int64_t lock_start;                   /* START of the lock held at P */
    uint8_t locked, misses, n_pids, reserved0;
    uint32_t pids_overflowed;
    uint32_t n_deferred;                  /* packets in State::deferred_* */
    uint8_t reserved[28];
};

struct State {
    Head head;
    uint8_t run[208];                     /* run[phi]: run(p) of the last p < P with p mod 204 == phi; 4 x 0 */
    uint8_t tail[TAIL_ROOM];              /* tail[j] = y[P - 2650 + j], j < 2650; 0 where that lies below 0, and 6 x 0 */
    CensusEntry census[CENSUS];
    uint8_t last[PIDS];                   /* the counter of the last good packet of every PID, or NO_COUNTER */
    uint8_t deferred_ts[DEFER_ROOM * TS_BYTES];   /* the first n_deferred: as they would have been written; the rest 0 */
    Record deferred_rec[DEFER_ROOM];
};
constexpr int STATE_BYTES = int(sizeof(State));
constexpr int RUN_AT = 64, TAIL_AT = 272, CENSUS_AT = 2928, LAST_AT = 3568, DEFERRED_TS_AT = 11760, DEFERRED_REC_AT = 23792;
static_assert(sizeof(Record) == 16 && sizeof(Result) == 80 && sizeof(Head) == 64 && sizeof(CensusEntry) == 20 && STATE_BYTES == 24816 && offsetof(Result, locked) == 4 * SUMMED_COUNTERS &&
                  STATE_BYTES % 16 == 0 && offsetof(State, run) == RUN_AT && offsetof(State, tail) == TAIL_AT &&
                  offsetof(State, census) == CENSUS_AT && offsetof(State, last) == LAST_AT &&
                  offsetof(State, deferred_ts) == DEFERRED_TS_AT && offsetof(State, deferred_rec) == DEFERRED_REC_AT,
              "records of the ABI");

DABGPU_FEC_FN bool bitrate_ok(int kbps) { return kbps >= 8 && kbps <= MAX_KBPS && kbps % 8 == 0; }
DABGPU_FEC_FN int frame_bytes(int kbps) { return 3 * kbps; }
DABGPU_FEC_FN int new_packets(int kbps, int n_cifs) { return int((int64_t(frame_bytes(kbps)) * n_cifs + CODED_BYTES - 1) / CODED_BYTES); }
DABGPU_FEC_FN int max_packets(int kbps, int n_cifs) { return new_packets(kbps, n_cifs) + DEFER_ROOM; }
/* where packet j of a call goes: < capacity emitted, then deferred, then lost */
enum Fate : int { EMITTED = 0, DEFERRED = 1, LOST = 2 };
DABGPU_FEC_FN int fate_of(int64_t j, int capacity) { return j < capacity ? EMITTED : j - capacity < DEFER_ROOM ? DEFERRED : LOST; }

DABGPU_FEC_FN void head_fresh(Head &h, int kbps) {
    uint8_t *p = reinterpret_cast<uint8_t *>(&h);
    for (int i = 0; i < int(sizeof(Head)); i++) p[i] = 0;
    h.magic = MAGIC;
    h.kbps = kbps;
}
/* a record this code wrote for this bit rate */
DABGPU_FEC_FN bool head_ok(const Head &h, int kbps) {
    bool ok = h.magic == MAGIC && h.kbps == kbps && h.pos >= 0 && h.pos <= MAX_POS && h.locked <= 1 && h.n_pids <= CENSUS && h.reserved0 == 0;
    ok = ok && h.n_deferred <= uint32_t(DEFER_ROOM);
    ok = ok && (h.locked ? h.lock_start >= 0 && h.lock_start < h.pos && h.misses < LOSS_MISSES : h.lock_start == 0 && h.misses == 0);
    ok = ok && (h.n_pids == CENSUS || h.pids_overflowed == 0);
    for (int i = 0; i < 28; i++) ok = ok && h.reserved[i] == 0;
    return ok;
}

DABGPU_FEC_FN uint8_t run_step(unsigned run, bool hit) { return hit ? uint8_t(run < 255 ? run + 1 : 255) : uint8_t(0); }

/* where byte i of the coded packet that starts at s lies in the stream */
DABGPU_FEC_FN int64_t gather_at(int64_t s, int i) { return s + CODED_BYTES * (i % BRANCHES) + i; }

/* The packets of the lock [start, end) (end = NEVER: still held) that a call bringing y[p0 .. p1 - 1] emits: s = first + 204 j,
 * j < count; and the packets of that lock the call counts as dropped. */
struct LockPackets {
    int64_t first;
    int32_t count, dropped;
};
DABGPU_FEC_FN int64_t ceil_div_204(int64_t a) { return a <= 0 ? 0 : (a + CODED_BYTES - 1) / CODED_BYTES; }
DABGPU_FEC_FN LockPackets lock_packets(int64_t start, int64_t end, int64_t p0, int64_t p1) {
    /* k_lo: the first k whose packet is complete at or after p0; k_hi: the first whose last byte lies at or beyond p1 */
    const int64_t k_lo = ceil_div_204(p0 - (SPAN - 1) - start);
    int64_t k_hi = ceil_div_204(p1 - (SPAN - 1) - start);
    LockPackets r = {start + CODED_BYTES * k_lo, 0, 0};
    if (end != NEVER) {
        const int64_t starts = (end - start) / CODED_BYTES, kept = starts > BRANCHES - 1 ? starts - (BRANCHES - 1) : 0;
        if (k_hi > kept) k_hi = kept;
        if (end >= p0 && end < p1) r.dropped = int32_t(starts - kept);
    }
    r.count = k_hi > k_lo ? int32_t(k_hi - k_lo) : 0;
    return r;
}

/* ---- one coded packet through the outer code.  w.syn holds the 16 syndromes of x.  Serial: the host path; the kernel runs
 * the same steps with the root search spread over its lanes. */
DABGPU_FEC_FN bool find_pattern(const fec::Gf &g, fec::RowWork &w) {
    w.ll = w.n = 0;
    if (!fec::locator(g, w)) return false;
    for (int c = 0; c < N; c++) {
        unsigned v;
        if (!fec::root_at(g, w, c, v)) continue;
        if (w.n < T) {
            w.pos[w.n] = uint8_t(c);
            w.val[w.n] = uint8_t(v);
        }
        w.n++;
    }
    return fec::pattern_holds(g, w);
}

/* x (204 bytes, as received) after the outer code said `codeword` or `holds` with the pattern in w: x corrected in place or
 * marked, and its record */
DABGPU_FEC_FN Record finish_packet(uint8_t *x, const fec::RowWork &w, bool codeword, bool holds, int64_t s) {
    Record r = {};
    if (codeword) {
        r.status = AS_RECEIVED;
    } else if (holds) {
        r.status = CORRECTED;
        for (int i = 0; i < w.n; i++) {
            x[w.pos[i]] ^= w.val[i];
            if (w.pos[i] < K) r.corrected_data++;
            else r.corrected_parity++;
        }
    } else {
        r.status = UNCORRECTABLE;
        x[1] |= 0x80;
    }
    r.pid = uint16_t(((x[1] & 0x1Fu) << 8) | x[2]);
    r.byte3 = x[3];
    r.flags = ((x[3] & 0x20) && x[4] >= 1 && (x[5] & 0x80)) ? FLAG_EXEMPT : 0;
    r.position = uint32_t(uint64_t(s) & 0xFFFFFFFFu);
    return r;
}

/* ---- continuity: the verdict of a good packet whose previous packet of the same PID had counter `previous` (NO_COUNTER:
 * there is none) */
enum Verdict : int { IN_ORDER = 0, DISCONTINUITY = 1, DUPLICATE = 2 };
DABGPU_FEC_FN int continuity(const Record &r, unsigned previous) {
    if (previous == NO_COUNTER || r.pid == NULL_PID || (r.flags & FLAG_EXEMPT)) return IN_ORDER;
    const unsigned cc = r.byte3 & 15u;
    if (r.byte3 & 0x10) return cc == ((previous + 1) & 15u) ? IN_ORDER : cc == previous ? DUPLICATE : DISCONTINUITY;
    return cc == previous ? IN_ORDER : DISCONTINUITY;
}
DABGPU_FEC_FN bool scrambled(const Record &r) { return (r.byte3 & 0xC0) != 0; }

/* the census entry of a PID, or -1 */
DABGPU_FEC_FN int census_find(const CensusEntry *census, int n_pids, unsigned pid) {
    for (int i = 0; i < n_pids; i++)
        if (census[i].pid == pid) return i;
    return -1;
}

/* ---- the host path: one entry of a call on memory the caller can read and write */

struct Input {
    const uint8_t *tail;                  /* the carried bytes, or NULL on a fresh start */
    const uint8_t *in;
    uint64_t in_stride;
    int64_t p0, p1;
    int fb;
    /* y[q], p0 - 2448 <= q < p1 */
    uint8_t at(int64_t q) const {
        if (q < p0) return (tail && q >= p0 - TAIL_BYTES) ? tail[q - (p0 - TAIL_BYTES)] : uint8_t(0);
        const int64_t o = q - p0;
        return in[uint64_t(o / fb) * in_stride + uint64_t(o % fb)];
    }
};

/* One entry of a call: the twin of the kernels.  state_in: STATE_BYTES or NULL; state_out: STATE_BYTES, no overlap with
 * state_in; ts: capacity x 188 bytes; records: as many. */
inline void process(const fec::Gf &g, const uint8_t *state_in, uint8_t *state_out, Result &res, const uint8_t *in, uint64_t in_stride, int n,
                    int kbps, uint8_t *ts, Record *records, int capacity) {
    const State *old = reinterpret_cast<const State *>(state_in);
    State *st = reinterpret_cast<State *>(state_out);
    Head h;
    bool fresh = state_in == nullptr;
    if (!fresh) {
        for (int i = 0; i < int(sizeof(Head)); i++) reinterpret_cast<uint8_t *>(&h)[i] = state_in[i];
        fresh = !head_ok(h, kbps);
    }
    if (fresh) head_fresh(h, kbps);
    for (int i = 0; i < 208; i++) st->run[i] = fresh ? uint8_t(0) : old->run[i];
    for (int i = 0; i < CENSUS; i++) st->census[i] = (fresh || i >= h.n_pids) ? CensusEntry{} : old->census[i];
    for (int i = 0; i < PIDS; i++) st->last[i] = fresh ? NO_COUNTER : old->last[i];
    const int fb = frame_bytes(kbps);
    const Input y = {fresh ? nullptr : old->tail, in, in_stride, h.pos, h.pos + int64_t(fb) * n, fb};
    res = Result{};
    res.cifs = n;
    res.bytes = fb * n;

    /* packet j of the call, as it would be written (x: its 188 bytes, r: its record), to where it goes */
    int64_t n_call = 0;
    uint32_t n_deferred = 0;
    auto deliver = [&](const uint8_t *x, const Record &r) {
        const int64_t j = n_call++;
        const int fate = fate_of(j, capacity);
        if (fate == LOST) {
            res.packets_lost++;
            return;
        }
        if (fate == DEFERRED) {
            const size_t q = size_t(j - capacity);
            for (int i = 0; i < TS_BYTES; i++) st->deferred_ts[q * TS_BYTES + i] = x[i];
            st->deferred_rec[q] = r;
            n_deferred++;
            return;
        }
        const int at = res.packets_emitted++;
        for (int i = 0; i < TS_BYTES; i++) ts[size_t(at) * TS_BYTES + i] = x[i];
        records[at] = r;
        if (r.status == UNCORRECTABLE) {
            res.packets_uncorrectable++;
            return;
        }
        (r.status == CORRECTED ? res.packets_corrected : res.packets_clean)++;
        res.bytes_corrected += r.corrected_data;
        res.parity_bytes_corrected += r.corrected_parity;
        if (st->last[r.pid] == NO_COUNTER) {          /* a PID's first good packet */
            if (h.n_pids < CENSUS) {
                st->census[h.n_pids] = CensusEntry{};
                st->census[h.n_pids++].pid = r.pid;
            } else {
                h.pids_overflowed++;
            }
        }
        const int slot = census_find(st->census, h.n_pids, r.pid);
        const int v = continuity(r, st->last[r.pid]);
        res.discontinuities += v == DISCONTINUITY;
        res.duplicates += v == DUPLICATE;
        if (slot >= 0) {
            CensusEntry &c = st->census[slot];
            c.packets++;
            c.discontinuities += v == DISCONTINUITY;
            c.duplicates += v == DUPLICATE;
            c.scrambled += scrambled(r);
        }
        st->last[r.pid] = uint8_t(r.byte3 & 15u);
    };
    for (int i = 0; i < DEFER_ROOM * TS_BYTES; i++) st->deferred_ts[i] = 0;
    for (int i = 0; i < DEFER_ROOM; i++) st->deferred_rec[i] = Record{};
    if (!fresh)
        for (uint32_t d = 0; d < h.n_deferred; d++) {
            Record r = old->deferred_rec[d];
            r.pid &= 0x1FFF;                          /* (a record this code wrote has it so) */
            deliver(old->deferred_ts + size_t(d) * TS_BYTES, r);
        }

    auto emit = [&](int64_t start, int64_t end) {
        const LockPackets lp = lock_packets(start, end, y.p0, y.p1);
        res.packets_dropped += lp.dropped;
        for (int j = 0; j < lp.count; j++) {
            const int64_t s = lp.first + int64_t(CODED_BYTES) * j;
            uint8_t x[N];
            unsigned S[T2] = {};
            for (int i = 0; i < N; i++) {
                x[i] = y.at(gather_at(s, i));
                fec::syndrome_add(g, x[i], i, S);
            }
            fec::RowWork w;
            for (int k = 0; k < T2; k++) w.syn[k] = uint8_t(S[k]);
            w.ll = w.n = 0;
            const bool codeword = fec::row_is_codeword(w), holds = !codeword && find_pattern(g, w);
            const Record r = finish_packet(x, w, codeword, holds, s);
            deliver(x, r);
        }
    };

    for (int64_t q = y.p0; q < y.p1; q++) {
        const int phi = int(q % CODED_BYTES);
        const bool hit = y.at(q) == SYNC_BYTE;
        const uint8_t run = st->run[phi] = run_step(st->run[phi], hit);
        if (!h.locked) {
            if (run >= LOCK_RUN) {
                h.locked = 1;
                h.lock_start = q;
                h.misses = 0;
                res.locks++;
                res.sync_hits++;
            }
        } else if (phi == int(h.lock_start % CODED_BYTES)) {
            if (hit) {
                h.misses = 0;
                res.sync_hits++;
            } else if (++h.misses == LOSS_MISSES) {
                emit(h.lock_start, q);
                h.locked = 0;
                h.lock_start = 0;
                h.misses = 0;
                res.lock_losses++;
            }
        }
    }
    if (h.locked) emit(h.lock_start, NEVER);

    for (int j = 0; j < TAIL_ROOM; j++) {
        const int64_t q = y.p1 - TAIL_BYTES + j;
        st->tail[j] = (q < 0 || j >= TAIL_BYTES) ? uint8_t(0) : y.at(q);
    }
    h.pos = y.p1;
    h.n_deferred = n_deferred;
    res.packets_deferred = int32_t(n_deferred);
    res.locked = h.locked;
    res.phase = h.locked ? int32_t(h.lock_start % CODED_BYTES) : -1;
    res.pids = h.n_pids;
    res.pids_overflowed = int32_t(h.pids_overflowed);
    st->head = h;
}

}  /* namespace dabgpu_dmb */
#endif
