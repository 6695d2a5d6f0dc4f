/* dabgpu_pft.h -- the PFT layer of ETSI TS 102 821: AF packets cut into PF fragments, with Reed-Solomon RS(255,207) over
 * interleaved chunks so that whole datagrams may be lost, and PF fragment byte streams put back together into AF packets.
 *
 * One implementation of the contract below: the kernel behind dabgpu_pft_fragments_dev (csrc/pft_kernels.hip) and the host
 * call dabgpu_pft_fragments_host lay fragments out with layout / parity_byte / fragment_header; the kernels behind
 * dabgpu_pft_read_dev (csrc/pft_read_kernels.hip), dabgpu_pft_read_host and the host mirror's BasicRadio::ProcessPft run
 * header_ok and the scalar steps (before_join / join / next_complete / flush_list / close_record); read_entry is the serial
 * reader of host code that links nothing.  Plain C++17, header-only; __host__ __device__ under hipcc.  Bytes are reached
 * through a byte accessor g(i).  The one table in memory (GF(2^8) exp / log, 768 bytes) is made by the compiler (make_gf())
 * and handed in by the caller: a constant on the host, a copy in LDS on the device.
 *
 * THE FORMAT, STATED AS KNOWN.  The specification was not at hand when this was written and no other implementation was
 * compared against: parity with ODR-DabMux / ODR-DabMod or any other EDI tool is not pinned (says
 * how a user pins it).  One line per field, so that a line can be corrected.  All integers are big-endian.
 *
 * PF fragment:
 *   2    "PF"
 *   2    Pseq    one value per AF packet, + 1 per packet modulo 65536
 *   3    Findex  0 .. Fcount - 1
 *   3    Fcount
 *   2    FEC(1) Addr(1) Plen(14)      Plen = payload bytes of this fragment
 *   if FEC:  1 RSk   1 RSz
 *   if Addr: 2 Source   2 Dest
 *   2    HCRC over every header byte before it, by the FIB's rule: x^16 + x^12 + x^5 + 1, start all ones, complemented
 *   Plen payload bytes                (header: 14 / 16 / 18 / 20 bytes)
 *
 * Without FEC the AF packet's l bytes are cut in order into fragments of s bytes; the last has l - (Fcount - 1) s.
 *
 * With FEC:  c = ceil(l / 207) chunks, k = ceil(l / c), z = c k - l zero bytes behind the packet, RSk = k, RSz = z.
 *   Codeword.  Chunk i (k data bytes in front) is one codeword with 48 parity bytes: RS(255,207) shortened by 207 - k
 *              leading zeros.
 *   Field.     GF(2^8), x^8 + x^4 + x^3 + x^2 + 1, alpha = 2.
 *   Generator. prod_{i = 0..47} (x + alpha^(FIRST_ROOT + i)), FIRST_ROOT = 1: THE LINE MOST LIKELY TO NEED CORRECTING.
 *   Order.     The first data byte is the coefficient of the highest power.
 *   Block.     The RS block of B = c (k + 48) bytes is all chunks' data (c k bytes, so the packet and its z zeros), then
 *              all chunks' parity: chunk i's parity lies at c k + 48 i.
 *   Fragments. Fragment g, payload byte j, is block byte j Fcount + g, or zero where that index is >= B.  Every fragment has
 *              Plen = s.
 *   Reader.    c = floor(Fcount Plen / (RSk + 48)), l = c RSk - RSz.
 *
 * THE WRITER'S LAYOUT, layout(l, fec, m, max_payload, addr).  Without FEC s = max_payload, f = ceil(l / s).  With FEC
 * s0 = min(floor(48 c / (m + 1)), max_payload), f = ceil(B / s0), s = ceil(B / f): the interleave depends on f alone, so
 * evening s out costs no protection.  guaranteed_losses is the largest n such that ANY n missing fragments leave every chunk
 * at most 48 erased positions, computed exactly from the bytes each fragment holds of each chunk (0 without FEC).  A
 * fragment's share of a chunk rounds up for the data and the parity positions separately, so that f alone can fall short
 * of m (m = 8: 7 at a third of all sizes): with m > 0, f is then the smallest one above that rule's with floor(f s / (k + 48))
 * == c and guaranteed_losses >= m.  Refused unless 12 <= l <= 8192, 1 <= f <= 256, 1 <= s <= 8192, m >= 0 and, with FEC,
 * floor(f s / (k + 48)) == c (the reader's view gives the writer's c).
 *
 * THE CONTRACT of one entry of dabgpu_pft_read_host in one call, every ambiguity decided.
 *
 * Stream.  S = the carried tail of the state (0 .. 8211 bytes; a tail length above 8211 counts as 8211) followed by the
 * entry's n_bytes new bytes: datagram payloads concatenated by the caller, or a file.
 *
 * H(q): the header at q -- 14 / 16 / 18 / 20 bytes, as the flags at q + 10 say -- lies inside S and is plausible: "PF",
 * 1 <= Fcount <= 256, Findex < Fcount, 1 <= Plen <= 8192, with FEC 1 <= RSk <= 207, HCRC holds.
 * T(q): H(q) and the fragment (header + Plen) lies inside S.
 * U(q): H(q) cannot be decided yet: q + 12 > |S|, or the bytes at q are "PF" and the header the flags imply ends behind S.
 * None of the three changes for a position once more bytes follow it, except that U gives way to a decision and H to T.
 *
 * Walk from p = 0: q = the smallest position >= p with H(q) or U(q), or |S| when there is none; skipped += q - p, p = q.
 *   T(p): the fragment is taken (below), p += header + Plen, and the walk goes on.  If bytes were skipped in front of it,
 *         resyncs++.
 *   otherwise (the fragment at p is incomplete, its header is cut, or p = |S|): S[p ..) is the new tail, stop.
 * The tail is at most 8211 bytes by construction (a header of 20 and 8192 payload bytes, less one).  resyncs counts
 * stretches of skipped bytes; a stretch that a call's end cuts is counted by the call that reaches its end (the state
 * carries in_skip).  Payload bytes are never searched for headers: a "PF" inside a taken fragment's payload is payload.  A
 * plausible header whose fragment never completes holds the walk for at most 8211 bytes: a stream that ends is FLUSHed.
 *
 * Groups and the horizon.  H = the last Pseq emitted or given up, carried.  Open groups exist only at H + 1 and H + 2.  For a
 * taken fragment with Pseq p (fragments++):
 *   a. no horizon: H = p - 1.
 *   b. d = (p - H) mod 65536.  d == 0 or d >= 32768: the fragment is late.  If the 16 taken fragments before it were all
 *      late (late_run == 16), the horizon is forgotten instead: the open groups that hold a fragment are closed in ascending
 *      order (an empty or unsupported one is dropped without a count), H = p - 1, and the fragment goes on at c. with d = 1.
 *      Otherwise late++, late_run++, the fragment is dropped.  A fragment that is not late sets late_run = 0.
 *   c. d >= 3: the groups H + 1 .. p - 2 are closed in ascending order, H = p - 2.  Closing a group that holds no fragment
 *      (none came, or it was unsupported) only adds 1 to `missing` and gives no record.
 *   d. the fragment joins group p.  A group's parameters (Fcount, FEC, Addr, RSk, RSz, Source, Dest, and with FEC Plen) are
 *      those of its first fragment in stream order; a fragment that disagrees is `mismatched` and dropped.  Without FEC,
 *      s is the Plen of the group's first fragment that is not the last index; another fragment that is not the last index
 *      has to have Plen == s, and the last index Plen <= s, whichever comes second being the one that is mismatched (a
 *      group of one fragment has s = its Plen).  A Findex already held counts in `duplicates` and is dropped.
 *      A group is unsupported when Fcount s > MAX_BLOCK = 10496 or, with FEC, c < 1, c > 40, l < 12 or l > 8192: what it
 *      holds is dropped, and every fragment of it counts in `unsupported` (the one that shows it and the later ones).
 *   e. while group H + 1 is complete (all Fcount indexes held): it is closed, H += 1.
 * Output is therefore strictly in Pseq order, which the EDI reader's SEQ check wants.
 *
 * The entry's FLUSH flag, at the call's end: the open groups that hold a fragment are closed in ascending order with the
 * flag FLUSHED, H = the last one closed; if that is H + 2 and group H + 1 held nothing, missing++.
 *
 * Closing a group that holds a fragment gives record r (r counts from 0 in each call):
 *   complete:   the packet is emitted.  With FEC no RS arithmetic is done and the parity is not judged.
 *   incomplete, without FEC:  LOST.
 *   incomplete, with FEC:  chunk i's erased positions are those (of its k + 48) whose block index modulo Fcount names a
 *               missing fragment.  Any chunk with more than 48: LOST.  Otherwise every chunk with erasures is filled by
 *               ERASURE-ONLY DECODING -- the unique values at the e erased positions that make syndromes 1 .. e (the
 *               roots alpha^FIRST_ROOT .. alpha^(FIRST_ROOT + e - 1)) vanish -- the packet is emitted with RECOVERED, and
 *               with INCONSISTENT when any of the 48 syndromes of a filled chunk is then non-zero (a received byte was
 *               wrong).  chunks_filled and bytes_filled count the chunks with erasures and their erased positions.
 * Emission: the packet's l bytes are appended to the entry's output, packets back to back; AF_OK is set when the bytes
 * begin with a header that dabgpu_edi::header_ok accepts, 12 + LEN == l and the AF CRC holds.  Packets without AF_OK are
 * emitted too (the EDI reader resynchronises over them).  A LOST group gives a record of length 0.
 *
 * Record (32 bytes): offset in the call's output, length, pseq, fcount, received, plen (s), rs_k, rs_z, chunks,
 * max_erasures (the worst chunk), flags, source, dest.
 * Result (64 bytes, a call's new fragments only): records, packets, lost, recovered, fragments, duplicates, mismatched,
 * late, unsupported, missing, skipped, resyncs, out_bytes, tail_bytes, chunks_filled, bytes_filled.
 *
 * Sizes.  A call emits at most the payload bytes it took and the two carried groups held: out_bytes <= 2 MAX_BLOCK + |S|,
 * so read_out_bytes(n_bytes) = 29216 + n_bytes suffices; read_max_records(n_bytes) = 2 + (8211 + n_bytes) / 15 (the
 * smallest fragment has 15 bytes).  Nothing can run out of room.
 *
 * State record (STATE_BYTES): a head of 144 bytes (tail length, horizon, late run, in_skip, running totals), the two open
 * groups (slot Pseq & 1: a 64-byte head with the parameters and a 256-bit received map, then MAX_BLOCK bytes with fragment
 * Findex at Findex s -- without FEC the last index lies at the END of the buffer, MAX_BLOCK - Plen, since it may come before
 * s is known -- zero where nothing is held), and 8224 tail bytes, zero behind the tail.  All zero = a stream that starts.
 * A record this code did not write is read as it is: the tail length and the late run clamped, flags != 0 = set, and a
 * group head that is not one this code writes for the carried horizon (sanitize) is an empty group; no value makes a call
 * read outside the record.
 *
 * The result of a stream does not depend on where it is cut into calls: records, output bytes and totals agree, calls of
 * no bytes included.
 *
 * NOT PROVIDED.  Errors in received bytes are not sought (erasures only: a wrong byte shows as INCONSISTENT or a missing
 * AF_OK); Addr filtering (Source / Dest are reported); sockets; sender-side spreading of fragments in time.
 */
#ifndef DABGPU_PFT_H
#define DABGPU_PFT_H

#include <stddef.h>
#include <stdint.h>

#include "dabgpu_edi.h"

#if defined(__HIPCC__)
#define DABGPU_PFT_FN __host__ __device__ inline
#else
#define DABGPU_PFT_FN inline
#endif

namespace dabgpu_pft {

constexpr int FIRST_ROOT = 1;                 /* the generator's roots are alpha^FIRST_ROOT .. alpha^(FIRST_ROOT + 47) */
constexpr int PARITY = 48;
constexpr int RS_K = 207;
constexpr int MAX_CHUNKS = 40;
constexpr int MAX_FRAGMENTS = 256;
constexpr int MAX_PLEN = 8192;
constexpr int MAX_BLOCK = 10496;
constexpr int MIN_PACKET = dabgpu_edi::AF_OVERHEAD;
constexpr int MAX_PACKET = dabgpu_edi::MAX_PACKET;
constexpr int MIN_HEADER = 14;
constexpr int MAX_HEADER = 20;
constexpr int MIN_FRAGMENT = MIN_HEADER + 1;
constexpr int MAX_TAIL = MAX_HEADER + MAX_PLEN - 1;
constexpr int LATE_RUN = 16;
constexpr int OUT_SLACK = (2 * MAX_BLOCK + MAX_TAIL + 15) / 16 * 16;

enum Flag : uint16_t { FLAG_FEC = 1, FLAG_ADDR = 2, FLAG_RECOVERED = 4, FLAG_INCONSISTENT = 8, FLAG_LOST = 16, FLAG_AF_OK = 32,
                       FLAG_FLUSHED = 64 };
enum EntryFlag : int32_t { READ_FLUSH = 1 };

struct Layout {                           /* == dabgpu_pft_layout_info */
    int32_t packet_bytes, fec, m, max_payload, addr;
    int32_t chunks, rs_k, rs_z, block_bytes;
    int32_t fcount, plen, header_bytes;
    int32_t stream_bytes;                 /* all fragments of one packet, headers included */
    int32_t guaranteed_losses;
    int32_t reserved_a, reserved_b;
};

struct Record {                           /* == dabgpu_pft_read_record */
    uint32_t offset;
    uint16_t length, pseq, fcount, received, plen;
    uint8_t rs_k, rs_z, chunks, max_erasures;
    uint16_t flags, source, dest;
    uint32_t reserved_a, reserved_b;      /* (no arrays: a record lives in registers on the device) */
};

struct Result {                           /* == dabgpu_pft_read_result */
    uint32_t records, packets, lost, recovered;
    uint32_t fragments, duplicates, mismatched, late;
    uint32_t unsupported, missing, skipped, resyncs;
    uint32_t out_bytes, tail_bytes, chunks_filled, bytes_filled;
};

struct Head {                             /* the first 144 bytes of a state record */
    uint32_t tail_bytes;
    uint8_t have_horizon, in_skip, late_run, reserved;
    uint16_t horizon, reserved1;
    uint32_t reserved2;
    uint64_t records, packets, lost, recovered, fragments, duplicates, mismatched, late, unsupported, missing, skipped, resyncs,
        out_bytes, chunks_filled, bytes_filled, reserved3;
};

enum GroupKind : uint8_t { GROUP_EMPTY = 0, GROUP_OPEN = 1, GROUP_UNSUPPORTED = 2 };

struct GroupHead {                        /* 64 bytes in front of each group's buffer */
    uint8_t kind, fec, addr, have_s;
    uint16_t pseq, fcount;
    uint16_t s, last_len;                 /* s: every fragment's Plen with FEC; without, see d. above.  last_len: without FEC, the last index's */
    uint16_t received, source;
    uint16_t dest, length;                /* length: l, with FEC */
    uint8_t rs_k, rs_z, chunks, reserved;
    uint32_t reserved1, reserved2;
    uint64_t map[4];                      /* bit Findex: held */
};

constexpr int STATE_HEAD_BYTES = 144;
constexpr int GROUP_HEAD_BYTES = 64;
constexpr int GROUP_BYTES = GROUP_HEAD_BYTES + MAX_BLOCK;
constexpr int STATE_GROUPS_AT = STATE_HEAD_BYTES;
constexpr int STATE_TAIL_AT = STATE_GROUPS_AT + 2 * GROUP_BYTES;
constexpr int STATE_TAIL_ROOM = (MAX_TAIL + 15) / 16 * 16;
constexpr int STATE_BYTES = STATE_TAIL_AT + STATE_TAIL_ROOM;
static_assert(sizeof(Layout) == 64 && sizeof(Record) == 32 && sizeof(Result) == 64 && sizeof(Head) == STATE_HEAD_BYTES &&
                  sizeof(GroupHead) == GROUP_HEAD_BYTES && STATE_BYTES % 16 == 0 && STATE_TAIL_AT % 16 == 0 && GROUP_BYTES % 16 == 0,
              "records of the ABI");
static_assert(MAX_CHUNKS * (RS_K + PARITY) <= MAX_BLOCK && MAX_BLOCK % 16 == 0, "a block of 40 chunks fits");

DABGPU_PFT_FN uint32_t clamp_tail(uint32_t tail_bytes) { return tail_bytes > uint32_t(MAX_TAIL) ? uint32_t(MAX_TAIL) : tail_bytes; }
DABGPU_PFT_FN uint64_t read_out_bytes(uint32_t n_bytes) { return uint64_t(OUT_SLACK) + n_bytes; }
DABGPU_PFT_FN uint32_t read_max_records(uint32_t n_bytes) { return 2u + uint32_t((uint64_t(MAX_TAIL) + n_bytes) / uint64_t(MIN_FRAGMENT)); }

/* ---- GF(2^8), x^8 + x^4 + x^3 + x^2 + 1, alpha = 2 ---------------------------------------------------------------------- */
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
DABGPU_PFT_FN constexpr unsigned gmul(const Gf &g, unsigned a, unsigned b) { return (a && b) ? g.exp[g.log[a] + g.log[b]] : 0u; }
DABGPU_PFT_FN constexpr unsigned gdiv(const Gf &g, unsigned a, unsigned b) { return a ? g.exp[g.log[a] + 255 - g.log[b]] : 0u; }   /* b != 0 */
/* v alpha^e, 0 <= e < 255 */
DABGPU_PFT_FN constexpr unsigned gscale(const Gf &g, unsigned v, int e) { return v ? g.exp[g.log[v] + e] : 0u; }

/* What data byte r positions before a chunk's last data byte adds to parity byte q: the coefficient of x^(47 - q) in
 * x^(48 + r) mod generator, as its logarithm (ZERO_LOG where the coefficient is zero).  Made by the compiler. */
constexpr uint8_t ZERO_LOG = 255;
struct ParityTable {
    uint8_t lg[RS_K][PARITY];
};
constexpr ParityTable make_parity_table() {
    const Gf g = make_gf();
    unsigned gen[PARITY + 1] = {1};                     /* gen[i] = coefficient of x^i */
    for (int i = 0; i < PARITY; i++) {
        const unsigned root = g.exp[(FIRST_ROOT + i) % 255];
        for (int j = i + 1; j >= 1; j--) gen[j] = gen[j - 1] ^ gmul(g, gen[j], root);
        gen[0] = gmul(g, gen[0], root);
    }
    ParityTable t{};
    unsigned rem[PARITY] = {};                          /* x^(48 + r) mod gen, rem[i] = coefficient of x^i */
    for (int i = 0; i < PARITY; i++) rem[i] = gen[i];   /* r = 0: x^48 = the generator's lower part */
    for (int r = 0; r < RS_K; r++) {
        for (int q = 0; q < PARITY; q++) t.lg[r][q] = rem[PARITY - 1 - q] ? g.log[rem[PARITY - 1 - q]] : ZERO_LOG;
        const unsigned top = rem[PARITY - 1];
        for (int i = PARITY - 1; i >= 1; i--) rem[i] = rem[i - 1] ^ gmul(g, top, gen[i]);
        rem[0] = gmul(g, top, gen[0]);
    }
    return t;
}
/* parity byte q of the chunk whose k data bytes are d(0 .. k - 1) */
template <class D> DABGPU_PFT_FN unsigned parity_byte(const Gf &g, const ParityTable &t, D d, int k, int q) {
    unsigned p = 0;
    for (int j = 0; j < k; j++) {
        const unsigned v = d(j), lg = t.lg[k - 1 - j][q];
        if (v && lg != ZERO_LOG) p ^= g.exp[g.log[v] + lg];
    }
    return p;
}

/* ---- sizes -------------------------------------------------------------------------------------------------------------- */
DABGPU_PFT_FN constexpr int header_bytes(int fec, int addr) { return MIN_HEADER + (fec ? 2 : 0) + (addr ? 4 : 0); }
/* how many of the indexes 0 .. x - 1 are g modulo f */
DABGPU_PFT_FN int count_mod(int x, int g, int f) { return x > g ? (x - g - 1) / f + 1 : 0; }
/* the positions of chunk i (of c chunks of k data bytes) that fragment g of f holds */
DABGPU_PFT_FN int fragment_chunk_bytes(int c, int k, int f, int g, int i) {
    const int d0 = i * k, p0 = c * k + PARITY * i;
    return count_mod(d0 + k, g, f) - count_mod(d0, g, f) + count_mod(p0 + PARITY, g, f) - count_mod(p0, g, f);
}
/* where position j (0 .. k + 47) of chunk i lies in the block */
DABGPU_PFT_FN int block_index(int c, int k, int i, int j) { return j < k ? i * k + j : c * k + PARITY * i + (j - k); }

/* The writer's layout; false = refused (out is not written). */
inline bool layout(int l, int fec, int m, int max_payload, int addr, Layout &out) {
    if (l < MIN_PACKET || l > MAX_PACKET || m < 0 || max_payload < 1) return false;
    Layout a{};
    a.packet_bytes = l;
    a.fec = fec ? 1 : 0;
    a.m = m;
    a.max_payload = max_payload;
    a.addr = addr ? 1 : 0;
    a.header_bytes = header_bytes(fec, addr);
    if (!fec) {
        const int s = max_payload > MAX_PLEN ? MAX_PLEN : max_payload;
        const int f = (l + s - 1) / s;
        if (f > MAX_FRAGMENTS) return false;
        a.fcount = f;
        a.plen = s;
        a.stream_bytes = f * a.header_bytes + l;
        out = a;
        return true;
    }
    const int c = (l + RS_K - 1) / RS_K, k = (l + c - 1) / c, B = c * (k + PARITY);
    const int64_t per = int64_t(PARITY) * c / (int64_t(m) + 1);
    const int s0 = int(per < max_payload ? per : max_payload);
    if (s0 < 1) return false;
    for (int f = (B + s0 - 1) / s0; f <= MAX_FRAGMENTS; f++) {
        const int s = (B + f - 1) / f;
        if (s < 1 || s > MAX_PLEN || f * s / (k + PARITY) != c) {
            if (m == 0) return false;
            continue;
        }
        /* per chunk: the largest n whose n heaviest fragments still hold at most 48 of its positions */
        int best = f;
        for (int i = 0; i < c; i++) {
            int hist[PARITY + 2] = {};                  /* fragments by the positions they hold, 49 = more than 48 */
            for (int g = 0; g < f; g++) {
                const int n = fragment_chunk_bytes(c, k, f, g, i);
                hist[n > PARITY ? PARITY + 1 : n]++;
            }
            int n = 0, sum = 0;
            bool full = hist[PARITY + 1] > 0;
            for (int v = PARITY; v >= 1 && !full; v--)
                for (int u = 0; u < hist[v]; u++) {
                    if (sum + v > PARITY) {
                        full = true;
                        break;
                    }
                    sum += v;
                    n++;
                }
            if (!full) n = f;                           /* (fragments that hold nothing of it may all go) */
            if (n < best) best = n;
        }
        if (best < m) continue;                         /* data and parity positions round up separately: one fragment more */
        a.chunks = c;
        a.rs_k = k;
        a.rs_z = c * k - l;
        a.block_bytes = B;
        a.fcount = f;
        a.plen = s;
        a.stream_bytes = f * (a.header_bytes + s);
        a.guaranteed_losses = best;
        out = a;
        return true;
    }
    return false;
}

/* ---- the fragment header ------------------------------------------------------------------------------------------------ */
struct FragHeader {
    uint32_t pseq, findex, fcount, fec, addr, plen, rs_k, rs_z, source, dest, header_bytes;
};

DABGPU_PFT_FN uint32_t crc_byte(uint32_t crc, uint32_t b) { return dabgpu_edi::crc_byte(crc, b); }

/* byte i (0 .. header_bytes - 3) of a fragment's header, in front of its HCRC */
DABGPU_PFT_FN uint32_t header_byte(int i, const FragHeader &h) {
    switch (i) {
    case 0: return 'P';
    case 1: return 'F';
    case 2: return (h.pseq >> 8) & 0xFFu;
    case 3: return h.pseq & 0xFFu;
    case 4: return (h.findex >> 16) & 0xFFu;
    case 5: return (h.findex >> 8) & 0xFFu;
    case 6: return h.findex & 0xFFu;
    case 7: return (h.fcount >> 16) & 0xFFu;
    case 8: return (h.fcount >> 8) & 0xFFu;
    case 9: return h.fcount & 0xFFu;
    case 10: return (h.fec ? 0x80u : 0u) | (h.addr ? 0x40u : 0u) | ((h.plen >> 8) & 0x3Fu);
    case 11: return h.plen & 0xFFu;
    default: break;
    }
    int at = i - 12;
    if (h.fec) {
        if (at == 0) return h.rs_k;
        if (at == 1) return h.rs_z;
        at -= 2;
    }
    switch (at) {
    case 0: return (h.source >> 8) & 0xFFu;
    case 1: return h.source & 0xFFu;
    case 2: return (h.dest >> 8) & 0xFFu;
    default: return h.dest & 0xFFu;
    }
}
/* the whole header with its HCRC: put(i, byte) for i = 0 .. header_bytes - 1 */
template <class Put> DABGPU_PFT_FN void write_header(Put put, const FragHeader &h) {
    const int n = int(h.header_bytes) - 2;
    uint32_t crc = 0xFFFFu;
    for (int i = 0; i < n; i++) {
        const uint32_t b = header_byte(i, h);
        crc = crc_byte(crc, b);
        put(i, uint8_t(b));
    }
    crc ^= 0xFFFFu;
    put(n, uint8_t(crc >> 8));
    put(n + 1, uint8_t(crc & 0xFFu));
}

/* H: `avail` bytes lie behind g(0); h is filled when it holds */
template <class G> DABGPU_PFT_FN bool header_ok(G g, uint32_t avail, FragHeader &h) {
    if (avail < 12u || g(0) != 'P' || g(1) != 'F') return false;
    const uint32_t b10 = g(10);
    h.fec = b10 >> 7;
    h.addr = (b10 >> 6) & 1u;
    h.header_bytes = uint32_t(header_bytes(int(h.fec), int(h.addr)));
    if (avail < h.header_bytes) return false;
    h.pseq = (g(2) << 8) | g(3);
    h.findex = (g(4) << 16) | (g(5) << 8) | g(6);
    h.fcount = (g(7) << 16) | (g(8) << 8) | g(9);
    h.plen = ((b10 & 0x3Fu) << 8) | g(11);
    if (h.fcount < 1u || h.fcount > uint32_t(MAX_FRAGMENTS) || h.findex >= h.fcount || h.plen < 1u || h.plen > uint32_t(MAX_PLEN)) return false;
    int at = 12;
    h.rs_k = h.rs_z = h.source = h.dest = 0;
    if (h.fec) {
        h.rs_k = g(12);
        h.rs_z = g(13);
        if (h.rs_k < 1u || h.rs_k > uint32_t(RS_K)) return false;
        at = 14;
    }
    if (h.addr) {
        h.source = (g(at) << 8) | g(at + 1);
        h.dest = (g(at + 2) << 8) | g(at + 3);
        at += 4;
    }
    uint32_t crc = 0xFFFFu;
    for (int i = 0; i < at; i++) crc = crc_byte(crc, g(i));
    return (crc ^ 0xFFFFu) == ((g(at) << 8) | g(at + 1));
}

/* ---- groups ------------------------------------------------------------------------------------------------------------- */
DABGPU_PFT_FN bool held(const GroupHead &g, uint32_t findex) { return (g.map[findex >> 6] >> (findex & 63u)) & 1u; }
DABGPU_PFT_FN int popcount64(uint64_t v) {
    int n = 0;
    for (; v; v &= v - 1) n++;
    return n;
}
DABGPU_PFT_FN void clear_head(GroupHead &g) {
    g.kind = g.fec = g.addr = g.have_s = 0;
    g.pseq = g.fcount = g.s = g.last_len = g.received = g.source = g.dest = g.length = 0;
    g.rs_k = g.rs_z = g.chunks = g.reserved = 0;
    g.reserved1 = g.reserved2 = 0;
    g.map[0] = g.map[1] = g.map[2] = g.map[3] = 0;
}
/* with FEC: chunks and l from the first fragment's fields, as the reader sees them; false = unsupported */
DABGPU_PFT_FN bool fec_view(uint32_t fcount, uint32_t s, uint32_t rs_k, uint32_t rs_z, uint32_t &c, uint32_t &l) {
    if (fcount * s > uint32_t(MAX_BLOCK)) return false;
    c = fcount * s / (rs_k + uint32_t(PARITY));
    if (c < 1u || c > uint32_t(MAX_CHUNKS) || c * rs_k < rs_z + uint32_t(MIN_PACKET) || c * rs_k - rs_z > uint32_t(MAX_PACKET)) return false;
    l = c * rs_k - rs_z;
    return true;
}
/* a group head as this code writes it for slot `slot` under the carried horizon; anything else is made an empty group */
DABGPU_PFT_FN void sanitize(GroupHead &g, int slot, bool have_horizon, uint32_t horizon) {
    const uint32_t d = (uint32_t(g.pseq) - horizon) & 0xFFFFu;
    bool ok = have_horizon && (g.kind == GROUP_OPEN || g.kind == GROUP_UNSUPPORTED) && (d == 1u || d == 2u) && int(g.pseq & 1u) == slot;
    if (ok && g.kind == GROUP_UNSUPPORTED) {
        const uint16_t pseq = g.pseq;
        clear_head(g);
        g.kind = GROUP_UNSUPPORTED;
        g.pseq = pseq;
        return;
    }
    if (ok) {
        ok = g.fcount >= 1 && g.fcount <= MAX_FRAGMENTS && g.fec <= 1 && g.addr <= 1 && g.have_s <= 1 && g.received <= g.fcount &&
             g.s <= MAX_PLEN && g.last_len <= MAX_PLEN && g.reserved == 0 && g.reserved1 == 0 && g.reserved2 == 0;
    }
    if (ok) {
        int n = 0;
        for (int w = 0; w < 4; w++) {
            const int lo = 64 * w;
            uint64_t allowed = 0;
            if (int(g.fcount) >= lo + 64) allowed = ~uint64_t(0);
            else if (int(g.fcount) > lo) allowed = (uint64_t(1) << (int(g.fcount) - lo)) - 1u;
            if (g.map[w] & ~allowed) ok = false;
            n += popcount64(g.map[w]);
        }
        if (n != int(g.received)) ok = false;
    }
    if (ok && g.fec) {
        uint32_t c = 0, l = 0;
        ok = g.have_s == 1 && g.s >= 1 && g.last_len == 0 && g.rs_k >= 1 && g.rs_k <= RS_K && fec_view(g.fcount, g.s, g.rs_k, g.rs_z, c, l) &&
             c == g.chunks && l == g.length;
    } else if (ok) {
        const bool have_last = held(g, uint32_t(g.fcount) - 1u);
        ok = g.rs_k == 0 && g.rs_z == 0 && g.chunks == 0 && g.length == 0 && (have_last ? g.last_len >= 1 : g.last_len == 0);
        if (ok && g.have_s) ok = g.s >= 1 && uint32_t(g.fcount) * g.s <= uint32_t(MAX_BLOCK) && g.last_len <= g.s;
        if (ok && !g.have_s) ok = g.s == 0 && g.received == (have_last ? 1 : 0);
        if (ok && g.fcount == 1 && g.received == 1) ok = g.have_s == 1 && g.s == g.last_len;
    }
    if (!ok) clear_head(g);
}

/* where byte t (0 .. l - 1) of a complete group's packet lies in its buffer */
DABGPU_PFT_FN uint32_t packet_byte_at(const GroupHead &g, uint32_t t) {
    if (g.fec) return (t % g.fcount) * g.s + t / g.fcount;
    const uint32_t body = (uint32_t(g.fcount) - 1u) * g.s;
    return t < body ? t : uint32_t(MAX_BLOCK) - g.last_len + (t - body);
}
/* the erased positions of chunk i of an incomplete group with FEC */
DABGPU_PFT_FN int lowest_bit(uint64_t v) {          /* v != 0 */
#if defined(__HIP_DEVICE_COMPILE__)
    return __ffsll(static_cast<unsigned long long>(v)) - 1;
#else
    return __builtin_ctzll(v);
#endif
}
/* (a step per MISSING fragment, read off the received map: the usual loss is a few fragments of a packet) */
DABGPU_PFT_FN int chunk_erasures(const GroupHead &g, int i) {
    int n = 0;
    for (int w = 0; 64 * w < int(g.fcount); w++) {
        const int left = int(g.fcount) - 64 * w;
        uint64_t missing = ~g.map[w] & (left >= 64 ? ~uint64_t(0) : (uint64_t(1) << left) - 1u);
        for (; missing; missing &= missing - 1u)
            n += fragment_chunk_bytes(g.chunks, g.rs_k, g.fcount, 64 * w + lowest_bit(missing), i);
    }
    return n;
}

/* what a walk carries from fragment to fragment, in a call and between calls: the head's fields, the two group heads and
 * the call's counters.  (skipped, resyncs and in_skip belong to the walk over positions, not to these steps.) */
struct Walk {
    uint32_t have_horizon, horizon, late_run;
    Result c;
    GroupHead g[2];
};

DABGPU_PFT_FN void walk_begin(Walk &w, const Head &in) {
    w.have_horizon = in.have_horizon != 0;
    w.horizon = in.horizon;
    w.late_run = in.late_run > LATE_RUN ? uint32_t(LATE_RUN) : in.late_run;
    w.c = Result{};
}

/* closing the group of slot `slot` that holds nothing: missing++ when `counted` */
DABGPU_PFT_FN void drop_empty(Walk &w, int slot, bool counted) {
    clear_head(w.g[slot]);
    if (counted) w.c.missing++;
}
DABGPU_PFT_FN bool holds(const GroupHead &g) { return g.kind == GROUP_OPEN && g.received > 0; }

/* Steps a, b and c for a taken fragment.  Returns -1 when the fragment is dropped as late, else the number (0 .. 2) of
 * groups the caller has to close, slots in close_slot, before it goes on with join(). */
DABGPU_PFT_FN int before_join(Walk &w, const FragHeader &h, int close_slot[2]) {
    w.c.fragments++;
    int n = 0;
    if (!w.have_horizon) {
        w.have_horizon = 1;
        w.horizon = (h.pseq - 1u) & 0xFFFFu;
    }
    uint32_t d = (h.pseq - w.horizon) & 0xFFFFu;
    if (d == 0u || d >= 32768u) {
        if (w.late_run < uint32_t(LATE_RUN)) {
            w.late_run++;
            w.c.late++;
            return -1;
        }
        for (uint32_t k = 1; k <= 2; k++) {
            const int slot = int((w.horizon + k) & 1u);
            if (holds(w.g[slot])) close_slot[n++] = slot;
            else drop_empty(w, slot, false);
        }
        w.horizon = (h.pseq - 1u) & 0xFFFFu;
        w.late_run = 0;
        return n;
    }
    w.late_run = 0;
    if (d >= 3u) {
        const uint32_t closing = d - 2u;
        for (uint32_t k = 1; k <= 2 && k <= closing; k++) {
            const int slot = int((w.horizon + k) & 1u);
            if (holds(w.g[slot])) close_slot[n++] = slot;
            else drop_empty(w, slot, true);
        }
        if (closing > 2u) w.c.missing += closing - 2u;
        w.horizon = (h.pseq - 2u) & 0xFFFFu;
    }
    return n;
}

/* Step d.  What the caller has to do with the fragment's payload. */
struct Move {
    int32_t slot;
    int32_t clear;                        /* the slot's buffer is zeroed first (what the group held is dropped) */
    uint32_t at, n;                       /* then n payload bytes go to buffer offset at (n = 0: the fragment is dropped) */
};
DABGPU_PFT_FN Move join(Walk &w, const FragHeader &h) {
    Move mv{int32_t(h.pseq & 1u), 0, 0u, 0u};
    GroupHead &g = w.g[mv.slot];
    if (g.kind == GROUP_EMPTY) {
        clear_head(g);
        g.kind = GROUP_OPEN;
        g.pseq = uint16_t(h.pseq);
        g.fcount = uint16_t(h.fcount);
        g.fec = uint8_t(h.fec);
        g.addr = uint8_t(h.addr);
        g.rs_k = uint8_t(h.rs_k);
        g.rs_z = uint8_t(h.rs_z);
        g.source = uint16_t(h.source);
        g.dest = uint16_t(h.dest);
        if (h.fec) {
            uint32_t c = 0, l = 0;
            if (!fec_view(h.fcount, h.plen, h.rs_k, h.rs_z, c, l)) {
                const uint16_t pseq = g.pseq;
                clear_head(g);
                g.kind = GROUP_UNSUPPORTED;
                g.pseq = pseq;
            } else {
                g.have_s = 1;
                g.s = uint16_t(h.plen);
                g.chunks = uint8_t(c);
                g.length = uint16_t(l);
            }
        }
    }
    if (g.kind == GROUP_UNSUPPORTED) {
        w.c.unsupported++;
        return mv;
    }
    if (h.fcount != g.fcount || h.fec != g.fec || h.addr != g.addr || h.rs_k != g.rs_k || h.rs_z != g.rs_z || h.source != g.source ||
        h.dest != g.dest || (g.fec && h.plen != g.s)) {
        w.c.mismatched++;
        return mv;
    }
    if (held(g, h.findex)) {
        w.c.duplicates++;
        return mv;
    }
    const bool last = h.findex + 1u == h.fcount;
    if (g.fec) {
        mv.at = h.findex * g.s;
    } else if (last) {
        if (g.have_s && h.plen > g.s) {
            w.c.mismatched++;
            return mv;
        }
        if (g.fcount == 1) {
            g.have_s = 1;
            g.s = uint16_t(h.plen);
        }
        g.last_len = uint16_t(h.plen);
        mv.at = uint32_t(MAX_BLOCK) - h.plen;
    } else {
        if (!g.have_s) {
            if (g.last_len > h.plen) {
                w.c.mismatched++;
                return mv;
            }
            if (h.fcount * h.plen > uint32_t(MAX_BLOCK)) {
                const uint16_t pseq = g.pseq;
                mv.clear = g.received > 0;
                clear_head(g);
                g.kind = GROUP_UNSUPPORTED;
                g.pseq = pseq;
                w.c.unsupported++;
                return mv;
            }
            g.have_s = 1;
            g.s = uint16_t(h.plen);
        } else if (h.plen != g.s) {
            w.c.mismatched++;
            return mv;
        }
        mv.at = h.findex * g.s;
    }
    g.map[h.findex >> 6] |= uint64_t(1) << (h.findex & 63u);
    g.received++;
    mv.n = h.plen;
    return mv;
}

/* Step e: the slot of group H + 1 when it is complete (the caller closes it with advance), else -1 */
DABGPU_PFT_FN int next_complete(const Walk &w) {
    if (!w.have_horizon) return -1;
    const int slot = int((w.horizon + 1u) & 1u);
    const GroupHead &g = w.g[slot];
    return g.kind == GROUP_OPEN && g.received == g.fcount && uint32_t(g.pseq) == ((w.horizon + 1u) & 0xFFFFu) ? slot : -1;
}

/* FLUSH: the slots to close with FLAG_FLUSHED, in order; the horizon moves here */
DABGPU_PFT_FN int flush_list(Walk &w, int close_slot[2]) {
    if (!w.have_horizon) return 0;
    int n = 0;
    const int s1 = int((w.horizon + 1u) & 1u), s2 = s1 ^ 1;
    const bool h1 = holds(w.g[s1]), h2 = holds(w.g[s2]);
    if (h1) close_slot[n++] = s1;
    if (h2) {
        if (!h1) drop_empty(w, s1, true);
        close_slot[n++] = s2;
    }
    w.horizon = (w.horizon + (h2 ? 2u : h1 ? 1u : 0u)) & 0xFFFFu;
    return n;
}

/* What closing a group that holds a fragment comes to: its record and where its bytes go.  worst / with / erased: the
 * largest chunk_erasures, the chunks that have any and their sum (all 0 for a complete group and without FEC). */
enum CloseKind : int32_t { CLOSE_LOST = 0, CLOSE_COPY = 1, CLOSE_FILL = 2 };
DABGPU_PFT_FN int close_record(Walk &w, int slot, int worst, int with, int erased, uint32_t extra_flags, Record &r) {
    const GroupHead &g = w.g[slot];
    const bool complete = g.received == g.fcount;
    int kind = CLOSE_COPY;
    uint32_t flags = extra_flags | (g.fec ? uint32_t(FLAG_FEC) : 0u) | (g.addr ? uint32_t(FLAG_ADDR) : 0u), length = 0;
    if (!complete && (!g.fec || worst > PARITY)) {
        kind = CLOSE_LOST;
        flags |= FLAG_LOST;
        w.c.lost++;
    } else {
        length = g.fec ? g.length : (uint32_t(g.fcount) - 1u) * g.s + g.last_len;
        w.c.packets++;
        if (!complete) {
            kind = CLOSE_FILL;
            flags |= FLAG_RECOVERED;
            w.c.recovered++;
            w.c.chunks_filled += uint32_t(with);
            w.c.bytes_filled += uint32_t(erased);
        }
    }
    r.offset = w.c.out_bytes;
    r.length = uint16_t(length);
    r.pseq = g.pseq;
    r.fcount = g.fcount;
    r.received = g.received;
    r.plen = g.s;
    r.rs_k = g.rs_k;
    r.rs_z = g.rs_z;
    r.chunks = g.chunks;
    r.max_erasures = uint8_t(worst > 255 ? 255 : worst);
    r.flags = uint16_t(flags);
    r.source = g.source;
    r.dest = g.dest;
    r.reserved_a = r.reserved_b = 0;
    w.c.out_bytes += length;
    w.c.records++;
    return kind;
}
/* after the caller has moved the bytes: the slot is empty again (the caller zeroes its buffer) */
DABGPU_PFT_FN void close_done(Walk &w, int slot, bool advance) {
    clear_head(w.g[slot]);
    if (advance) w.horizon = (w.horizon + 1u) & 0xFFFFu;
}

/* the head of the next call's state; skipped, resyncs, tail_bytes of c are the position walk's */
DABGPU_PFT_FN Head next_head(const Head &in, const Walk &w, bool in_skip) {
    Head h = in;
    const Result &c = w.c;
    h.tail_bytes = c.tail_bytes;
    h.have_horizon = w.have_horizon ? 1 : 0;
    h.in_skip = in_skip ? 1 : 0;
    h.late_run = uint8_t(w.late_run);
    h.reserved = 0;
    h.horizon = uint16_t(w.have_horizon ? w.horizon : 0u);
    h.reserved1 = 0;
    h.reserved2 = 0;
    h.records += c.records;
    h.packets += c.packets;
    h.lost += c.lost;
    h.recovered += c.recovered;
    h.fragments += c.fragments;
    h.duplicates += c.duplicates;
    h.mismatched += c.mismatched;
    h.late += c.late;
    h.unsupported += c.unsupported;
    h.missing += c.missing;
    h.skipped += c.skipped;
    h.resyncs += c.resyncs;
    h.out_bytes += c.out_bytes;
    h.chunks_filled += c.chunks_filled;
    h.bytes_filled += c.bytes_filled;
    h.reserved3 = 0;
    return h;
}

/* ---- erasure-only decoding, serially ------------------------------------------------------------------------------------ */
/* One codeword of n = k + 48 bytes behind get / put (byte 0 = the highest power), e <= 48 erased positions pos[0 .. e - 1]
 * ascending, read as zero.  Fills them (contract) and returns true when all 48 syndromes then vanish. */
template <class Get, class Put> inline bool fill_erasures(const Gf &g, Get get, Put put, int n, const int *pos, int e) {
    unsigned S[PARITY] = {}, gamma[PARITY + 1] = {1}, omega[PARITY] = {}, X[PARITY] = {};
    int t = 0;
    for (int j = 0; j < n; j++) {
        const bool erased = t < e && pos[t] == j;
        if (erased) t++;
        const unsigned v = erased ? 0u : get(j);
        for (int m = 0; m < PARITY; m++) S[m] = gscale(g, S[m], (FIRST_ROOT + m) % 255) ^ v;
    }
    for (int u = 0; u < e; u++) {
        X[u] = unsigned(n - 1 - pos[u]);                    /* the logarithm of the locator */
        for (int j = u + 1; j >= 1; j--) gamma[j] ^= gscale(g, gamma[j - 1], int(X[u]));
    }
    for (int j = 0; j < e; j++)
        for (int i = 0; i <= j; i++) omega[j] ^= gmul(g, S[i], gamma[j - i]);
    unsigned after[PARITY];
    for (int m = 0; m < PARITY; m++) after[m] = S[m];
    for (int u = 0; u < e; u++) {
        const int xinv = (255 - int(X[u])) % 255;
        unsigned num = 0, den = 1;
        for (int j = e - 1; j >= 0; j--) num = gscale(g, num, xinv) ^ omega[j];
        for (int v = 0; v < e; v++)
            if (v != u) den = gmul(g, den, 1u ^ g.exp[(int(X[v]) + xinv) % 255]);
        const unsigned y = gdiv(g, num, gscale(g, den, int(X[u]) * FIRST_ROOT % 255));
        put(pos[u], uint8_t(y));
        for (int m = 0; m < PARITY; m++) after[m] ^= gscale(g, y, int(X[u]) * (FIRST_ROOT + m) % 255);
    }
    unsigned any = 0;
    for (int m = 0; m < PARITY; m++) any |= after[m];
    return any == 0;
}

/* AF_OK of l bytes behind g */
template <class G> DABGPU_PFT_FN bool af_ok(G g, uint32_t l) {
    int total = 0;
    return l >= uint32_t(dabgpu_edi::AF_OVERHEAD) && dabgpu_edi::header_ok(g, total) && uint32_t(total) == l && dabgpu_edi::crc_ok(g, total);
}

/* ---- the serial reader: one entry on host pointers ----------------------------------------------------------------------- */
struct PtrBytes {
    const uint8_t *p;
    DABGPU_PFT_FN uint32_t operator()(int i) const { return p[i]; }
};

/* a position of a contiguous S: 2 = T, 1 = H with an incomplete fragment or U (the walk stops there), 0 = neither */
template <class G> DABGPU_PFT_FN int position_status(G g, uint32_t avail, FragHeader &h) {
    if (avail < 12u) return 1;
    if (g(0) != 'P' || g(1) != 'F') return 0;
    const uint32_t b10 = g(10);
    if (avail < uint32_t(header_bytes(int(b10 >> 7), int((b10 >> 6) & 1u)))) return 1;
    if (!header_ok(g, avail, h)) return 0;
    return h.header_bytes + h.plen <= avail ? 2 : 1;
}
inline int fragment_at(const uint8_t *s, size_t len, size_t q, FragHeader &h) {
    return position_status(PtrBytes{s + q}, uint32_t(len - q > size_t(MAX_TAIL) + 1 ? size_t(MAX_TAIL) + 1 : len - q), h);
}

/* s / len: S already put together.  state_in: STATE_BYTES or NULL; state_out: STATE_BYTES, written whole; out:
 * read_out_bytes, records: read_max_records of the entry's new bytes.  scratch: MAX_BLOCK bytes of the caller's. */
inline void read_entry(const Gf &gf, const uint8_t *s, size_t len, const uint8_t *state_in, uint32_t entry_flags, uint8_t *out, Record *records,
                       uint32_t max_records, Result *result, uint8_t *state_out, uint8_t *scratch) {
    Head in{};
    Walk w;
    uint8_t *const hb = reinterpret_cast<uint8_t *>(&in);
    for (int i = 0; i < STATE_HEAD_BYTES; i++) hb[i] = state_in ? state_in[i] : 0;
    walk_begin(w, in);
    uint8_t *buf[2] = {state_out + STATE_GROUPS_AT + GROUP_HEAD_BYTES, state_out + STATE_GROUPS_AT + GROUP_BYTES + GROUP_HEAD_BYTES};
    for (int j = 0; j < 2; j++) {
        const uint8_t *src = state_in ? state_in + STATE_GROUPS_AT + j * GROUP_BYTES : nullptr;
        uint8_t *gh = reinterpret_cast<uint8_t *>(&w.g[j]);
        for (int i = 0; i < GROUP_HEAD_BYTES; i++) gh[i] = src ? src[i] : 0;
        sanitize(w.g[j], j, w.have_horizon != 0, w.horizon);
        for (int i = 0; i < MAX_BLOCK; i++) buf[j][i] = src && w.g[j].kind == GROUP_OPEN ? src[GROUP_HEAD_BYTES + i] : 0;
    }
    bool in_skip = in.in_skip != 0;
    const auto close = [&](int slot, uint32_t extra, bool advance) {
        const GroupHead &g = w.g[slot];
        int worst = 0, with = 0, erased = 0;
        if (g.fec && g.received < g.fcount)
            for (int i = 0; i < g.chunks; i++) {
                const int n = chunk_erasures(g, i);
                worst = n > worst ? n : worst;
                with += n > 0;
                erased += n;
            }
        Record r;
        const int kind = close_record(w, slot, worst, with, erased, extra, r);
        uint8_t *dst = out + r.offset;
        if (kind == CLOSE_COPY) {
            for (uint32_t t = 0; t < r.length; t++) dst[t] = buf[slot][packet_byte_at(g, t)];
        } else if (kind == CLOSE_FILL) {
            const int c = g.chunks, k = g.rs_k, n = k + PARITY, B = c * n;
            for (int idx = 0; idx < B; idx++) {
                const uint32_t f = uint32_t(idx) % g.fcount;
                scratch[idx] = held(g, f) ? buf[slot][f * g.s + uint32_t(idx) / g.fcount] : 0;
            }
            for (int i = 0; i < c; i++) {
                int pos[PARITY], e = 0;
                for (int j = 0; j < n && e < PARITY; j++)
                    if (!held(g, uint32_t(block_index(c, k, i, j)) % g.fcount)) pos[e++] = j;
                if (!e) continue;
                const bool clean = fill_erasures(gf, [&](int j) -> unsigned { return scratch[block_index(c, k, i, j)]; },
                                                 [&](int j, uint8_t v) { scratch[block_index(c, k, i, j)] = v; }, n, pos, e);
                if (!clean) r.flags |= FLAG_INCONSISTENT;
            }
            for (uint32_t t = 0; t < r.length; t++) dst[t] = scratch[t];
        }
        if (kind != CLOSE_LOST && af_ok(PtrBytes{dst}, r.length)) r.flags |= FLAG_AF_OK;
        if (w.c.records <= max_records) records[w.c.records - 1] = r;
        for (int i = 0; i < MAX_BLOCK; i++) buf[slot][i] = 0;
        close_done(w, slot, advance);
    };
    size_t p = 0;
    uint32_t skipped = 0, resyncs = 0;
    FragHeader h{};
    for (;;) {
        size_t q = p;
        int status = 0;
        while (q < len && (status = fragment_at(s, len, q, h)) == 0) q++;
        if (q > p) {
            skipped += uint32_t(q - p);
            in_skip = true;
            p = q;
        }
        if (p >= len || status != 2) break;
        if (in_skip) {
            resyncs++;
            in_skip = false;
        }
        int slots[2];
        const int n = before_join(w, h, slots);
        if (n >= 0) {
            for (int i = 0; i < n; i++) close(slots[i], 0u, false);
            const Move mv = join(w, h);
            if (mv.clear)
                for (int i = 0; i < MAX_BLOCK; i++) buf[mv.slot][i] = 0;
            for (uint32_t i = 0; i < mv.n; i++) buf[mv.slot][mv.at + i] = s[p + h.header_bytes + i];
            for (int slot; (slot = next_complete(w)) >= 0;) close(slot, 0u, true);
        }
        p += h.header_bytes + h.plen;
    }
    if (entry_flags & uint32_t(READ_FLUSH)) {
        int slots[2];
        const int n = flush_list(w, slots);
        for (int i = 0; i < n; i++) close(slots[i], FLAG_FLUSHED, false);
    }
    w.c.skipped = skipped;
    w.c.resyncs = resyncs;
    w.c.tail_bytes = uint32_t(len - p);
    *result = w.c;
    const Head hn = next_head(in, w, in_skip);
    const uint8_t *hs = reinterpret_cast<const uint8_t *>(&hn);
    for (int i = 0; i < STATE_HEAD_BYTES; i++) state_out[i] = hs[i];
    for (int j = 0; j < 2; j++) {
        const uint8_t *gh = reinterpret_cast<const uint8_t *>(&w.g[j]);
        for (int i = 0; i < GROUP_HEAD_BYTES; i++) state_out[STATE_GROUPS_AT + j * GROUP_BYTES + i] = gh[i];
    }
    for (size_t i = 0; i < size_t(STATE_TAIL_ROOM); i++) state_out[STATE_TAIL_AT + i] = i < len - p ? s[p + i] : 0;
}

/* ---- the serial writer -------------------------------------------------------------------------------------------------- */
/* One AF packet af(0 .. l - 1) as the fragments of `a`: put(i, byte) for every byte 0 .. a.stream_bytes - 1 (not in order).
 * block: a.block_bytes bytes of the caller's (unused without FEC). */
template <class Af, class Put>
inline void write_fragments(const Gf &gf, const ParityTable &pt, const Layout &a, uint32_t pseq, uint32_t source, uint32_t dest, Af af, Put put,
                            uint8_t *block) {
    const int l = a.packet_bytes, f = a.fcount, s = a.plen, hl = a.header_bytes;
    if (a.fec) {
        const int c = a.chunks, k = a.rs_k;
        for (int i = 0; i < c * k; i++) block[i] = i < l ? uint8_t(af(i)) : 0;
        for (int i = 0; i < c; i++)
            for (int q = 0; q < PARITY; q++)
                block[c * k + PARITY * i + q] = uint8_t(parity_byte(gf, pt, [&](int j) -> unsigned { return block[i * k + j]; }, k, q));
    }
    for (int g = 0; g < f; g++) {
        FragHeader h{};
        h.pseq = pseq & 0xFFFFu;
        h.findex = uint32_t(g);
        h.fcount = uint32_t(f);
        h.fec = uint32_t(a.fec);
        h.addr = uint32_t(a.addr);
        h.plen = uint32_t(a.fec || g + 1 < f ? s : l - (f - 1) * s);
        h.rs_k = uint32_t(a.rs_k);
        h.rs_z = uint32_t(a.rs_z);
        h.source = a.addr ? source & 0xFFFFu : 0u;
        h.dest = a.addr ? dest & 0xFFFFu : 0u;
        h.header_bytes = uint32_t(hl);
        const int at = g * (hl + s);
        write_header([&](int i, uint8_t b) { put(at + i, b); }, h);
        for (int j = 0; j < int(h.plen); j++) {
            const int idx = j * f + g;
            put(at + hl + j, a.fec ? (idx < a.block_bytes ? block[idx] : uint8_t(0)) : uint8_t(af(g * s + j)));
        }
    }
}

}  // namespace dabgpu_pft
#endif
