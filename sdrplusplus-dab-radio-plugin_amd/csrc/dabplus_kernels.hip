// dabplus_kernels.hip -- DAB+ audio super-frame checks on the GPU: the step after the
// MSC Viterbi for DAB+ subchannels.  The reference shows the results as the "Firecode / RS / AU" error flags and
// GetSuperFrameHeader() (/root/reference/src/render_radio_block.cpp:414-437); the code is in the absent
// DAB-Radio submodule, so this restates ETSI TS 102 563 (see oracle/dabplus_oracle.c for the conventions).
//
// One 64-thread workgroup per super-frame (120*s bytes, s = bitrate/8 <= 64):
//   thread j < s     RS(120,110) decode of byte-interleaved column j: syndromes by Horner, and only if one is
//                    non-zero Berlekamp-Massey + Chien + Forney (<= 5 byte errors), GF(2^8)/0x11D via log tables
//   thread 0         Fire code over header bytes 2..10, AU table (2/3/4/6 access units, 12-bit starts)
//   all 64 threads   CRC16-CCITT of each access unit in turn: every lane takes a contiguous piece from register state 0 (the first
//                    piece from 0xFFFF), multiplies it by x^(8 * bytes behind the piece) mod the generator, and the wave XORs
//                    the sixty-four results -- the CRC is linear over GF(2)
// Byte-serial integer work at kB/s rates: one LDS-resident super-frame, no attempt at a roofline.
//
// Two kernels run that body: dabplus_superframe_kernel on super-frames the caller has aligned, and dabplus_follow_kernel
// on the super-frames dabplus_align_kernel has found in the logical frames of many sub-channels (one wave per
// sub-channel: raw Fire check of every frame, votes per residue mod 5, the carry record for the next call).
#include "kernels.hpp"

namespace dabk {

namespace {

struct alignas(16) GfLds {
    uint8_t exp[512];
    uint8_t log[256];
};
// GF(2^8) tables, x^8 + x^4 + x^3 + x^2 + 1, alpha = 2: made by the compiler, copied into LDS by all lanes (one thread
// building them with a 512-step loop at the head of every launch was ~3 us of a ~40 us kernel)
constexpr GfLds make_gf_tables() {
    GfLds g{};
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
__device__ const GfLds GF_TABLES = make_gf_tables();
static_assert(sizeof(GfLds) == 768, "copied as 192 words");

// x^(8 k) mod x^16 + x^12 + x^5 + 1 for k = 0 .. 110 * 64 + 65: what a CRC register that has taken a piece of an access unit still
// has to be multiplied by when k more bytes follow the piece
constexpr int CRC_Z_MAX = 110 * 64 + 66;
struct alignas(16) CrcShift {
    uint16_t z[CRC_Z_MAX];                                     // (copied into LDS as 32-bit words)
};
constexpr CrcShift make_crc_shift() {
    CrcShift t{};
    unsigned v = 1;
    for (int k = 0; k < CRC_Z_MAX; k++) {
        t.z[k] = uint16_t(v);
        for (int b = 0; b < 8; b++) v = (v & 0x8000u) ? (((v << 1) ^ 0x1021u) & 0xFFFFu) : (v << 1);
    }
    return t;
}
__device__ const CrcShift CRC_SHIFT = make_crc_shift();

// a(x) b(x) mod x^16 + x^12 + x^5 + 1 (16-bit operands)
__device__ __forceinline__ unsigned crc_mulmod(unsigned a, unsigned b) {
    unsigned r = 0;
#pragma unroll
    for (int bit = 15; bit >= 0; bit--) {
        r = (r & 0x8000u) ? (((r << 1) ^ 0x1021u) & 0xFFFFu) : (r << 1);
        if ((a >> bit) & 1u) r ^= b;
    }
    return r;
}

__device__ __forceinline__ unsigned gmul(const GfLds &g, unsigned a, unsigned b) {
    return (a && b) ? g.exp[g.log[a] + g.log[b]] : 0u;
}
__device__ __forceinline__ unsigned gdiv(const GfLds &g, unsigned a, unsigned b) {   // b != 0
    return a ? g.exp[g.log[a] + 255 - g.log[b]] : 0u;
}
// coefficient c (non-zero handled by caller) times X^-j, with xinv = log(X^-1)
__device__ __forceinline__ unsigned gpow_term(const GfLds &g, unsigned c, int xinv, int j) {
    return c ? g.exp[(g.log[c] + xinv * j) % 255] : 0u;
}

__device__ __forceinline__ unsigned crc_ccitt_byte(unsigned crc, unsigned byte) {
    crc = ((crc >> 8) | (crc << 8)) & 0xFFFFu;
    crc ^= byte;
    crc ^= (crc & 0xFFu) >> 4;
    crc ^= (crc << 12) & 0xFFFFu;
    crc ^= ((crc & 0xFFu) << 5) & 0xFFFFu;
    return crc;
}

// The ten syndromes of all s columns, on all 64 lanes: S_k = sum_i r_i alpha^(k (119 - i)).  Lane (column c, part q) takes
// the bytes i = q len .. (q + 1) len - 1 of its column term by term -- one log look-up per byte, then ten INDEPENDENT exp
// look-ups (the index advances by 119 - i per k) -- and XORs its partial sums into syn[c][k].  (Horner on one lane per
// column, as before, was 1 200 dependent three-look-up multiplications: ~50 us of a super-frame's ~100; this is ~2.)
__device__ __forceinline__ void rs_syndromes(const GfLds &g, const uint8_t *sf, int s, int tid, unsigned (*syn)[10]) {
    constexpr int N = 120, T2 = 10;
    const int parts = max(1, 64 / s);
    const int len = (N + parts - 1) / parts;
    const int c = tid % s, q = tid / s;
    if (q >= parts) return;
    unsigned S[T2];
#pragma unroll
    for (int k = 0; k < T2; k++) S[k] = 0;
    const int i1 = min(N, (q + 1) * len);
    for (int i = q * len; i < i1; i++) {
        const unsigned r = sf[c + s * i];
        if (!r) continue;
        const int p = N - 1 - i;                                // < 255
        int idx = g.log[r];                                     // k = 0: alpha^0
#pragma unroll
        for (int k = 0; k < T2; k++) {
            S[k] ^= g.exp[idx];
            idx += p;
            if (idx >= 255) idx -= 255;
        }
    }
#pragma unroll
    for (int k = 0; k < T2; k++)
        if (S[k]) atomicXor(&syn[c][k], S[k]);
}

// in-place RS(120,110) decode of the column {sf[j + s*i]} from its syndromes; returns corrected bytes or -1
__device__ int rs_decode_column(const GfLds &g, uint8_t *sf, int j, int s, const unsigned *syn) {
    constexpr int N = 120, T2 = 10;
    unsigned S[T2];
    unsigned any = 0;
#pragma unroll
    for (int k = 0; k < T2; k++) { S[k] = syn[k]; any |= S[k]; }
    if (!any) return 0;
    // Berlekamp-Massey (fixed-bound loops so everything stays in registers)
    unsigned L[T2 + 1], B[T2 + 1], Tm[T2 + 1];
#pragma unroll
    for (int i = 0; i <= T2; i++) { L[i] = 0; B[i] = 0; }
    L[0] = 1; B[0] = 1;
    int ll = 0, m = 1;
    unsigned bb = 1;
#pragma unroll
    for (int n = 0; n < T2; n++) {
        unsigned d = S[n];
#pragma unroll
        for (int i = 1; i <= T2; i++)
            if (i <= ll && i <= n) d ^= gmul(g, L[i], S[n - i]);
        if (d == 0) { m++; continue; }
#pragma unroll
        for (int i = 0; i <= T2; i++) Tm[i] = L[i];
        const unsigned coef = gdiv(g, d, bb);
#pragma unroll
        for (int i = 0; i <= T2; i++)
            if (i >= m) L[i] ^= gmul(g, coef, B[(i - m) < 0 ? 0 : (i - m)]);
        if (2 * ll <= n) {
            ll = n + 1 - ll;
#pragma unroll
            for (int i = 0; i <= T2; i++) B[i] = Tm[i];
            bb = d;
            m = 1;
        } else {
            m++;
        }
    }
    if (ll > 5) return -1;
    unsigned Om[T2];
#pragma unroll
    for (int i = 0; i < T2; i++) {
        unsigned v = 0;
#pragma unroll
        for (int jj = 0; jj <= 5; jj++)
            if (jj <= i && jj <= ll) v ^= gmul(g, L[jj], S[i - jj]);
        Om[i] = v;
    }
    int nerr = 0;
    int pos[5];
    unsigned val[5];
    for (int i = 0; i < N; i++) {
        const int p = N - 1 - i;
        const int xinv = (255 - p) % 255;
        unsigned ev = 0;
#pragma unroll
        for (int jj = 0; jj <= 5; jj++) ev ^= gpow_term(g, L[jj], xinv, jj);
        if (ev) continue;
        if (nerr == 5) return -1;
        unsigned om = 0, dl = 0;
#pragma unroll
        for (int jj = 0; jj < T2; jj++) om ^= gpow_term(g, Om[jj], xinv, jj);
        dl = gpow_term(g, L[1], xinv, 0) ^ gpow_term(g, L[3], xinv, 2) ^ gpow_term(g, L[5], xinv, 4);
        if (dl == 0) return -1;
        const unsigned e = gmul(g, g.exp[p % 255], gdiv(g, om, dl));
#pragma unroll
        for (int q = 0; q < 5; q++)
            if (q == nerr) { pos[q] = i; val[q] = e; }
        nerr++;
    }
    if (nerr != ll) return -1;
#pragma unroll
    for (int q = 0; q < 5; q++)
        if (q < nerr) sf[j + s * pos[q]] ^= uint8_t(val[q]);
    return nerr;
}

// The Fire code of a super-frame header (TS 102 563 clause 5.2) over bytes 2..10 against bytes 0..1, the eleven bytes packed
// little-endian in three words.  An all-zero header is its own (zero) check word: that is silence or erasures, not a super-frame.
__device__ __forceinline__ bool fire_header_ok(uint32_t w0, uint32_t w1, uint32_t w2) {
    const uint32_t w[3] = {w0, w1, w2};
    unsigned crc = 0, any = 0;
#pragma unroll
    for (int i = 0; i < 11; i++) {
        const unsigned byte = (w[i >> 2] >> (8 * (i & 3))) & 0xFFu;
        any |= byte;
        if (i < 2) continue;
        crc ^= byte << 8;
#pragma unroll
        for (int b = 0; b < 8; b++) crc = (crc & 0x8000u) ? ((crc << 1) ^ 0x782Fu) : (crc << 1);
        crc &= 0xFFFFu;
    }
    return any != 0 && crc == (((w0 & 0xFFu) << 8) | ((w0 >> 8) & 0xFFu));
}

// where one workgroup keeps its super-frame: [GF tables | 120 s bytes, rounded up to 16 | CRC shift table]
struct SuperframeLds {
    GfLds *g;
    uint8_t *sf;
    uint16_t *zt;
};
__device__ __forceinline__ SuperframeLds superframe_lds(unsigned char *smem, int s) {
    SuperframeLds l;
    l.g = reinterpret_cast<GfLds *>(smem);
    l.sf = smem + sizeof(GfLds);
    l.zt = reinterpret_cast<uint16_t *>(smem + sizeof(GfLds) + ((size_t(120) * s + 15) & ~size_t(15)));
    return l;
}
__host__ __device__ constexpr size_t superframe_lds_bytes(int s) {
    return sizeof(GfLds) + ((size_t(120) * s + 15) & ~size_t(15)) + (((size_t(110) * s + 66) * 2 + 3) & ~size_t(3));
}
// the GF tables and the shift-table entries a super-frame of this s can ask for, into LDS (before the body's first barrier)
__device__ __forceinline__ void superframe_stage_tables(const SuperframeLds &l, int s, int tid) {
    const int n_z = 110 * s + 66;
    for (int i = tid; i < 192; i += 64) reinterpret_cast<uint32_t *>(l.g)[i] = reinterpret_cast<const uint32_t *>(&GF_TABLES)[i];
    for (int i = tid; i < n_z / 2; i += 64) reinterpret_cast<uint32_t *>(l.zt)[i] = reinterpret_cast<const uint32_t *>(&CRC_SHIFT)[i];
}

// One super-frame that its workgroup has put into l.sf (and the tables beside it; no barrier yet): RS, then the Fire code, the
// AU table and the CRCs, then the 110 s data bytes to `dst` and the record to `status`.  Shared by the kernel that takes
// aligned super-frames and the one that follows a sub-channel (dabplus_follow_kernel): what they emit for the same 120 s
// bytes is the same by construction.  `t0`: the caller's clock at its start (DABPLUS_PHASE_TIMING only).
__device__ __forceinline__ void superframe_body(const SuperframeLds &l, int s, int tid, uint8_t *dst, SuperframeStatus *status,
                                                long long t0) {
    GfLds &g = *l.g;
    uint8_t *sf = l.sf;
    const uint16_t *zt = l.zt;
    __shared__ int sh_corrected, sh_bad, sh_mask, sh_naus;
    __shared__ int sh_start[8];
    __shared__ unsigned sh_syn[64][10];
#ifdef DABPLUS_PHASE_TIMING
    long long t1 = 0, t2 = 0, t3 = 0;
#define STAMP(v) v = wall_clock64()
#else
#define STAMP(v)
#endif
    if (tid == 0) { sh_corrected = 0; sh_bad = 0; sh_mask = 0; sh_naus = 0; }
    if (tid < 8) sh_start[tid] = 0;
    for (int i = tid; i < 64 * 10; i += 64) (&sh_syn[0][0])[i] = 0;
    __syncthreads();
    STAMP(t1);
    rs_syndromes(g, sf, s, tid, sh_syn);
    __syncthreads();
    if (tid < s) {
        const int r = rs_decode_column(g, sf, tid, s, sh_syn[tid]);
        if (r < 0) atomicAdd(&sh_bad, 1);
        else if (r > 0) atomicAdd(&sh_corrected, r);
    }
    __syncthreads();
    STAMP(t2);
    int fire_ok = 0;
    if (tid == 0) {
        unsigned crc = 0, any = unsigned(sf[0]) | sf[1];
        for (int i = 2; i < 11; i++) {
            any |= sf[i];
            crc ^= unsigned(sf[i]) << 8;
            for (int b = 0; b < 8; b++) crc = (crc & 0x8000u) ? ((crc << 1) ^ 0x782Fu) : (crc << 1);
            crc &= 0xFFFFu;
        }
        // an all-zero header is its own (zero) check word: that is silence or erasures, not a super-frame
        fire_ok = any != 0 && crc == ((unsigned(sf[0]) << 8) | sf[1]);
        if (fire_ok) {
            const int dac_rate = (sf[2] >> 6) & 1, sbr = (sf[2] >> 5) & 1;
            const int naus = dac_rate ? (sbr ? 3 : 6) : (sbr ? 2 : 4);
            sh_start[0] = naus == 2 ? 5 : naus == 3 ? 6 : naus == 4 ? 8 : 11;
            // the 12-bit start addresses follow the header byte back to back: bytes 3 .. 10 as one 64-bit word
            unsigned long long w = 0;
            for (int i = 3; i < 11; i++) w = (w << 8) | sf[i];
            for (int a = 1; a < naus; a++) sh_start[a] = int((w >> (64 - 12 * a)) & 0xFFFu);
            sh_start[naus] = 110 * s;
            sh_naus = naus;
        }
    }
    __syncthreads();
    {
        const int naus = sh_naus;
        for (int a = 0; a < naus; a++) {
            const int b0 = sh_start[a], b1 = sh_start[a + 1];                 // (the same for every lane)
            if (!(b0 >= 3 && b1 <= 110 * s && b1 - b0 >= 3)) continue;
            // len payload bytes, cut into 64 pieces of m, padded AT THE FRONT: lane l takes the padded positions
            // [l m, (l + 1) m), and (63 - l) m bytes follow its piece
            const int len = b1 - 2 - b0, m = (len + 63) >> 6, pad = 64 * m - len;
            int lo = tid * m - pad;
            const int hi = lo + m;
            unsigned crc = 0;
            if (hi > 0) {
                if (lo <= 0) { lo = 0; crc = 0xFFFFu; }                        // the piece the message starts in
                for (int i = lo; i < hi; i++) crc = crc_ccitt_byte(crc, sf[b0 + i]);
                crc = crc_mulmod(crc, zt[(63 - tid) * m]);
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) crc ^= unsigned(__shfl_xor(int(crc), off));
            crc ^= 0xFFFFu;
            if (tid == 0 && crc == ((unsigned(sf[b1 - 2]) << 8) | sf[b1 - 1])) sh_mask |= 1 << a;
        }
    }
    __syncthreads();
    STAMP(t3);
    for (int i = tid; i < 110 * s; i += 64) dst[i] = sf[i];
    if (tid == 0) {
        SuperframeStatus st;
        st.firecode_ok = fire_ok;
        st.rs_corrected = sh_corrected;
        st.rs_uncorrectable = sh_bad;
        st.num_aus = sh_naus;
        st.au_crc_mask = sh_mask;
        for (int a = 0; a < 8; a++) st.au_start[a] = sh_start[a];
        st.reserved[0] = st.reserved[1] = st.reserved[2] = 0;
#ifdef DABPLUS_PHASE_TIMING
        st.reserved[0] = int(t1 - t0); st.reserved[1] = int(t2 - t1); st.reserved[2] = int(t3 - t2);   // 100 MHz ticks: staging | RS | header + CRCs
#endif
        *status = st;
    }
    (void)t0;
}

__global__ __launch_bounds__(64) void dabplus_superframe_kernel(const uint8_t *in, size_t in_stride, int s,
                                                                uint8_t *out, SuperframeStatus *status,
                                                                unsigned long long *done_flag, unsigned long long done_seq) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const SuperframeLds l = superframe_lds(smem, s);
    uint8_t *sf = l.sf;
    const int tid = threadIdx.x;
    const int nbytes = 120 * s;
    const uint8_t *src = in + size_t(blockIdx.x) * in_stride;
#ifdef DABPLUS_PHASE_TIMING
    const long long t0 = wall_clock64();
#else
    const long long t0 = 0;
#endif
    superframe_stage_tables(l, s, tid);
    // the super-frame into LDS: 16 bytes per lane and trip when the source allows (one or two round trips -- the source
    // may be the caller's page-locked host buffer), bytes otherwise
    if (((reinterpret_cast<uintptr_t>(src) | size_t(nbytes)) & 15) == 0) {
        for (int i = tid; i < nbytes / 16; i += 64) reinterpret_cast<uint4 *>(sf)[i] = reinterpret_cast<const uint4 *>(src)[i];
    } else {
        for (int i = tid; i < nbytes; i += 64) sf[i] = src[i];
    }
    superframe_body(l, s, tid, out + size_t(blockIdx.x) * size_t(110 * s), status + blockIdx.x, t0);
    if (done_flag) {
        // (a launch of ONE workgroup: launch_dabplus_superframes.)  Every lane's stores -- the corrected bytes, lane 0's status
        // record -- are out at system scope before the barrier; only then is the word stored that the host is watching.
        __threadfence_system();
        __syncthreads();
        if (tid == 0) __hip_atomic_store(done_flag, done_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ------------------------------------------------------------------------------------------ following a sub-channel
// dabgpu_dabplus_follow_dev: the logical frames of a call are the `held` frames of the carry record followed by the
// n_cifs new ones; frame i of that sequence:
__device__ __forceinline__ const uint8_t *follow_frame(const FollowEntry &e, int held, int i) {
    const int lf = 24 * e.s;
    return i < held ? reinterpret_cast<const uint8_t *>(e.carry_in) + FOLLOW_CARRY_HEADER + size_t(i) * lf
                    : reinterpret_cast<const uint8_t *>(e.in) + size_t(i - held) * e.in_stride;
}

// n bytes (a multiple of 8; dst on 8 bytes) by the lanes of one wave: 16 or 8 bytes a lane where the addresses allow
__device__ __forceinline__ void follow_copy(uint8_t *dst, const uint8_t *src, int n, int lane) {
    const uintptr_t both = reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src);
    if (((both | uintptr_t(n)) & 15) == 0) {
        for (int i = lane; i < n / 16; i += 64) reinterpret_cast<uint4 *>(dst)[i] = reinterpret_cast<const uint4 *>(src)[i];
    } else if ((both & 7) == 0) {
        for (int i = lane; i < n / 8; i += 64) reinterpret_cast<uint2 *>(dst)[i] = reinterpret_cast<const uint2 *>(src)[i];
    } else {
        for (int i = lane; i < n; i += 64) dst[i] = src[i];
    }
}

// One wave64 per entry: the raw Fire check of every frame's first eleven bytes, the five votes by ballot, the phase, the
// plan for the follow kernel, the result record and the whole carry record (header, tail frames, zeros behind them).
__global__ __launch_bounds__(64) void dabplus_align_kernel(const FollowEntry *table, FollowPlan *plan, int n_cifs) {
    const FollowEntry e = table[blockIdx.x];
    const int lane = threadIdx.x;
    const int lf = 24 * e.s;
    int synced = 0, held = 0;
    if (e.carry_in) {
        const int4 h = *reinterpret_cast<const int4 *>(e.carry_in);
        // (a record this call did not write, or a damaged one: anything but 0..4 held frames is a fresh start)
        if (h.y >= 0 && h.y <= 4) { synced = h.x != 0; held = h.y; }
    }
    const int T = held + n_cifs;
    int votes[5] = {0, 0, 0, 0, 0};
    for (int i0 = 0; i0 < T; i0 += 64) {
        const int i = i0 + lane;
        bool hit = false;
        if (i < T) {
            const uint8_t *f = follow_frame(e, held, i);
            uint32_t w0, w1, w2;
            if ((reinterpret_cast<uintptr_t>(f) & 15) == 0) {              // (a logical frame is at least 24 bytes long)
                const uint4 v = *reinterpret_cast<const uint4 *>(f);
                w0 = v.x; w1 = v.y; w2 = v.z;
            } else {
                w0 = uint32_t(f[0]) | (uint32_t(f[1]) << 8) | (uint32_t(f[2]) << 16) | (uint32_t(f[3]) << 24);
                w1 = uint32_t(f[4]) | (uint32_t(f[5]) << 8) | (uint32_t(f[6]) << 16) | (uint32_t(f[7]) << 24);
                w2 = uint32_t(f[8]) | (uint32_t(f[9]) << 8) | (uint32_t(f[10]) << 16);
            }
            hit = fire_header_ok(w0, w1, w2);
        }
        const int r = i % 5;
#pragma unroll
        for (int q = 0; q < 5; q++) votes[q] += __popcll(__ballot(hit && r == q));
    }
    int best = 0, raw_hits = 0;
#pragma unroll
    for (int q = 0; q < 5; q++) {
        raw_hits += votes[q];
        best = max(best, votes[q]);
    }
    int p = -1;
    if (synced && votes[0] == best) {
        p = 0;                                                       // nothing outvotes the phase the stream is on
    } else if (best > 0) {
#pragma unroll
        for (int q = 4; q >= 0; q--)
            if (votes[q] == best) p = q;                             // the smallest residue with the maximum
    }
    int n_sf = 0, first_kept, dropped, synced_out = 0;
    if (p < 0) {
        first_kept = T - min(4, T);
        dropped = first_kept;
    } else {
        n_sf = T - p >= 5 ? (T - p) / 5 : 0;
        first_kept = p + 5 * n_sf;
        dropped = p;
#pragma unroll
        for (int q = 0; q < 5; q++)
            if (q == p) synced_out = votes[q] > 0 || n_sf == 0;
    }
    const int kept = T - first_kept;                                   // 0..4
    uint8_t *co = reinterpret_cast<uint8_t *>(e.carry_out);
    for (int j = 0; j < kept; j++)
        follow_copy(co + FOLLOW_CARRY_HEADER + size_t(j) * lf, follow_frame(e, held, first_kept + j), lf, lane);
    for (int i = kept * lf / 8 + lane; i < 4 * lf / 8; i += 64)
        reinterpret_cast<uint2 *>(co + FOLLOW_CARRY_HEADER)[i] = make_uint2(0u, 0u);
    if (lane == 0) {
        *reinterpret_cast<int4 *>(co) = make_int4(synced_out, kept, 0, 0);
        FollowPlan pl;
        pl.phase = p; pl.n_superframes = n_sf; pl.held = held; pl.reserved = 0;
        plan[blockIdx.x] = pl;
        FollowResult r;
        r.n_superframes = n_sf; r.phase = p; r.synced = synced_out; r.dropped = dropped; r.raw_hits = raw_hits; r.held = kept;
        r.reserved[0] = r.reserved[1] = 0;
        *reinterpret_cast<FollowResult *>(e.result) = r;
    }
}

// Workgroup (entry, k) of a grid of n_entries * max_sf: super-frame k of the entry's plan, or nothing.  Its five logical
// frames -- out of the carry, the new input, or both -- go into LDS with the entry's own s and in_stride; then the body
// every super-frame gets.  The dynamic LDS is sized for the largest s of the table.
__global__ __launch_bounds__(64) void dabplus_follow_kernel(const FollowEntry *table, const FollowPlan *plan, int max_sf) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int ei = blockIdx.x / unsigned(max_sf), k = blockIdx.x % unsigned(max_sf);
    const FollowPlan pl = plan[ei];
    if (k >= pl.n_superframes) return;                                 // (the whole workgroup, before any barrier)
    const FollowEntry e = table[ei];
    const int s = e.s, tid = threadIdx.x, lf = 24 * s;
    const SuperframeLds l = superframe_lds(smem, s);
#ifdef DABPLUS_PHASE_TIMING
    const long long t0 = wall_clock64();
#else
    const long long t0 = 0;
#endif
    superframe_stage_tables(l, s, tid);
    const int f0 = pl.phase + 5 * k;
#pragma unroll 1
    for (int j = 0; j < 5; j++) follow_copy(l.sf + j * lf, follow_frame(e, pl.held, f0 + j), lf, tid);
    superframe_body(l, s, tid, reinterpret_cast<uint8_t *>(e.data) + size_t(k) * size_t(110 * s),
                    reinterpret_cast<SuperframeStatus *>(e.status) + k, t0);
}

}  // namespace

hipError_t launch_dabplus_superframes(const uint8_t *in, size_t in_stride, int n_superframes, int s, uint8_t *out,
                                      SuperframeStatus *status, hipStream_t stream, unsigned long long *done_flag,
                                      unsigned long long done_seq) {
    if (n_superframes <= 0) return hipSuccess;
    if (s < 1 || s > 64 || (done_flag && n_superframes != 1)) return hipErrorInvalidValue;
    const size_t lds = superframe_lds_bytes(s);
    hipLaunchKernelGGL(dabplus_superframe_kernel, dim3(unsigned(n_superframes)), dim3(64), lds, stream, in, in_stride,
                       s, out, status, done_flag, done_seq);
    return hipGetLastError();
}

size_t follow_table_bytes(int n_entries) {
    return size_t(n_entries) * (sizeof(FollowEntry) + sizeof(FollowPlan));
}

hipError_t launch_dabplus_follow(const FollowEntry *entries, int n_entries, int n_cifs, void *d_table, size_t table_bytes,
                                 hipStream_t stream) {
    if (n_entries <= 0) return hipSuccess;
    if (n_cifs < 0 || !d_table || table_bytes < follow_table_bytes(n_entries) || (reinterpret_cast<uintptr_t>(d_table) & 15))
        return hipErrorInvalidValue;
    int max_s = 1;
    for (int i = 0; i < n_entries; i++) {
        if (entries[i].s < 1 || entries[i].s > 64) return hipErrorInvalidValue;
        max_s = entries[i].s > max_s ? entries[i].s : max_s;
    }
    const int max_sf = (n_cifs + 4) / 5;
    if (size_t(n_entries) * size_t(max_sf > 0 ? max_sf : 1) > size_t(0x7fffffff)) return hipErrorInvalidValue;
    // (pageable memory: the copy has left `entries` when the call returns)
    hipError_t err = hipMemcpyAsync(d_table, entries, size_t(n_entries) * sizeof(FollowEntry), hipMemcpyHostToDevice, stream);
    if (err != hipSuccess) return err;
    const FollowEntry *table = static_cast<const FollowEntry *>(d_table);
    FollowPlan *plan = reinterpret_cast<FollowPlan *>(static_cast<char *>(d_table) + size_t(n_entries) * sizeof(FollowEntry));
    hipLaunchKernelGGL(dabplus_align_kernel, dim3(unsigned(n_entries)), dim3(64), 0, stream, table, plan, n_cifs);
    if (max_sf > 0)
        hipLaunchKernelGGL(dabplus_follow_kernel, dim3(unsigned(n_entries) * unsigned(max_sf)), dim3(64), superframe_lds_bytes(max_s),
                           stream, table, plan, max_sf);
    return hipGetLastError();
}

}  // namespace dabk
