// mod_kernels.hip -- ETI(NI) frames modulated into Mode-I IQ (include/dabgpu.h, "ETI(NI) to IQ"): the transmit side of
// EN 300 401 clauses 11, 12 and 14, the mirror image of the front end and the channel decoder.
//
// mod_encode_kernel   one workgroup per (ensemble, ETI frame).  Every codeword of the frame -- the FIC group of its three
//                     FIBs, then each sub-channel -- is scrambled, run through the K = 7 mother code and punctured, one
//                     thread per input byte.  A byte is eight trellis steps = one 32-flag puncturing vector, and a profile
//                     is up to four runs of 128-bit blocks with one puncturing index each, so the byte's first output bit
//                     is run base + block * (32 + 4 PI) + vector * (8 + PI): no scan over a mask.  The bits are OR-ed
//                     into the frame's coded record in LDS (neighbouring bytes share words) and leave as 16-byte stores;
//                     the last 15 records' CIF parts are also written to the state record of the next call.
// mod_phase_kernel    the pre-pass: one thread per (transmission frame, 32 carriers).  It walks the 75 data symbols, gathers
//                     each symbol's two bit planes through the time interleaver (sixteen coded records, one masked word
//                     each), turns them into quarter turns and keeps their running sum as two bit planes per symbol: the
//                     differential modulation done once per carrier instead of l times by the wave of symbol l.
// mod_symbol_kernel   one workgroup per OFDM symbol (and one per null symbol).  Carrier k of symbol l is the exact point
//                     exp(j pi e / 4), e = 2 prs(k) + l + 2 sum (mod 8): nothing accumulates over the frame.  The inverse
//                     transform is the shared forward one on the conjugate spectrum; the 2552 samples leave LDS as 16-byte
//                     stores, the cyclic prefix first.  The null symbol's workgroup checks the four ETI headers of its
//                     frame and writes the frame's status.
#include "kernels.hpp"
#include "dab_tables.hpp"
#include "fft_common.hpp"

namespace dabk {

using namespace dab;

namespace {

static_assert(sizeof(ModState) == 103680 && sizeof(ModStatus) == 8, "mirror dabgpu_mod_state / dabgpu_mod_status");
static_assert(sizeof(ModArgs) <= 4096, "passed by value");
static_assert(MOD_CODED_WORDS % 4 == 0 && MOD_FIC_WORDS % 4 == 0 && MOD_CIF_WORDS % 4 == 0, "16-byte stores");
static_assert(4 * MOD_FIC_WORDS * 32 == NB_FIC_BITS && MOD_CIF_WORDS * 32 == NB_CIF_BITS && MOD_SYM_WORDS * 32 == NB_SYM_BITS, "Mode I");

constexpr int MOD_WG = 256;
constexpr int MOD_PHASE_WG = 192;              // four frames of 48 word columns
constexpr float MOD_SCALE = 0.025515518153991441f;   // 1 / sqrt(1536): unit mean power

// taps of the four generators (133, 171, 145, 133 octal) on a register whose bit d is the input d steps back
constexpr uint32_t MOD_TAPS[4] = {0x6D, 0x4F, 0x53, 0x6D};

// an ETI frame is taken when FSYNC is one of its two patterns and FICF/NST, MID/FL and every STC word are the plan's
__device__ __forceinline__ bool eti_word_fits(const ModArgs &a, const uint32_t *f, int i) {
    const uint32_t w = f[i];
    if (i == 0) return (w >> 8) == 0xB63A07u || (w >> 8) == 0x49C5F8u;
    if (i == 1) return ((w ^ a.header[1]) & 0xFF1FFF00u) == 0u;
    return w == a.header[i];
}

// bit reversal of three bits: the order in which the eight groups of a puncturing vector gain their bits
__device__ __forceinline__ int bitrev3(int g) { return ((g & 1) << 2) | (g & 2) | (g >> 2); }

__global__ __launch_bounds__(MOD_WG) void mod_encode_kernel(ModTables tab, ModArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t s_out[MOD_CODED_WORDS];
    __shared__ int s_bad;
    const int tid = threadIdx.x;
    const int n_cif = a.frames_per_stream * 4;
    const int carry = n_cif < MOD_DEPTH ? MOD_DEPTH - n_cif : 0;
    const int s = blockIdx.x / (n_cif + carry), u = blockIdx.x % (n_cif + carry);
    if (u >= n_cif) {
        // a call shorter than the interleaver's depth: slot j of the new record is slot n_cif + j of the old one
        if (!a.state_out) return;
        const int j = u - n_cif;
        uint4 *dst = reinterpret_cast<uint4 *>(a.state_out[s].cif[j]);
        const uint4 *src = a.state_in ? reinterpret_cast<const uint4 *>(a.state_in[s].cif[n_cif + j]) : nullptr;
        for (int i = tid; i < MOD_CIF_WORDS / 4; i += MOD_WG) dst[i] = src ? src[i] : make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    const size_t row = size_t(s) * n_cif + u;
    const uint8_t *f = a.eti + row * ETI_FRAME_BYTES;
    for (int i = tid; i < MOD_CODED_WORDS; i += MOD_WG) s_out[i] = 0u;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    if (tid < 2 + a.nst && !eti_word_fits(a, reinterpret_cast<const uint32_t *>(f), tid)) s_bad = 1;
    __syncthreads();
    const bool bad = s_bad != 0;                               // a refused frame is modulated as zero bytes

    for (int c = 0; c < a.n_codes; c++) {
        const ModCode &code = a.code[c];
        const int nbytes = code.in_bytes;
        const uint8_t *in = f + code.in_offset;
        int first_block[5], first_bit[5];
        first_block[0] = 0;
        first_bit[0] = 0;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            first_block[r + 1] = first_block[r] + code.blocks[r];
            first_bit[r + 1] = first_bit[r] + code.blocks[r] * (32 + 4 * code.pi[r]);
        }
        for (int k = tid; k <= nbytes; k += MOD_WG) {
            const uint32_t prev = k > 0 ? uint32_t((bad ? 0 : in[k - 1]) ^ tab.prbs[(k - 1) % MOD_PRBS_BYTES]) : 0u;
            unsigned long long acc = 0ull;
            int n = 0, pos;
            if (k < nbytes) {
                const uint32_t w = (prev << 8) | uint32_t((bad ? 0 : in[k]) ^ tab.prbs[k % MOD_PRBS_BYTES]);
                const int block = k >> 2;
                int r = 0;
#pragma unroll
                for (int q = 1; q < 4; q++) r += block >= first_block[q] ? 1 : 0;
                const int pi = r == 0 ? code.pi[0] : r == 1 ? code.pi[1] : r == 2 ? code.pi[2] : code.pi[3];
                const int b0 = r == 0 ? first_block[0] : r == 1 ? first_block[1] : r == 2 ? first_block[2] : first_block[3];
                const int p0 = r == 0 ? first_bit[0] : r == 1 ? first_bit[1] : r == 2 ? first_bit[2] : first_bit[3];
                pos = p0 + (block - b0) * (32 + 4 * pi) + (k & 3) * (8 + pi);
#pragma unroll
                for (int g = 0; g < 8; g++) {
                    const uint32_t reg = (w >> (7 - g)) & 0x7Fu;
                    const int ones = 1 + (pi >> 3) + (bitrev3(g) < (pi & 7) ? 1 : 0);
#pragma unroll
                    for (int x = 0; x < 4; x++)
                        if (x < ones) acc |= (unsigned long long)(__popc(reg & MOD_TAPS[x]) & 1) << n++;
                }
            } else {
                // the tail: six zero inputs flush the register, the first two outputs of each are sent
                const uint32_t w = prev << 8;
                pos = first_bit[4];
#pragma unroll
                for (int g = 0; g < 6; g++) {
                    const uint32_t reg = (w >> (7 - g)) & 0x7Fu;
                    acc |= (unsigned long long)(__popc(reg & MOD_TAPS[0]) & 1) << n++;
                    acc |= (unsigned long long)(__popc(reg & MOD_TAPS[1]) & 1) << n++;
                }
            }
            acc <<= (pos & 31);
            const int word = code.out_word + (pos >> 5);
            if (uint32_t(acc)) atomicOr(&s_out[word], uint32_t(acc));
            if (uint32_t(acc >> 32)) atomicOr(&s_out[word + 1], uint32_t(acc >> 32));
        }
    }
    __syncthreads();
    uint4 *dst = reinterpret_cast<uint4 *>(a.coded + row * MOD_CODED_WORDS);
    for (int i = tid; i < MOD_CODED_WORDS / 4; i += MOD_WG) dst[i] = reinterpret_cast<const uint4 *>(s_out)[i];
    const int slot = u - (n_cif - MOD_DEPTH);
    if (a.state_out && slot >= 0) {
        uint4 *keep = reinterpret_cast<uint4 *>(a.state_out[s].cif[slot]);
        for (int i = tid; i < MOD_CIF_WORDS / 4; i += MOD_WG) keep[i] = reinterpret_cast<const uint4 *>(s_out + MOD_FIC_WORDS)[i];
    }
}

// word `cw` of the CIF of ETI frame t of stream s after time interleaving: bit i comes from the coded record of frame
// t - D(i mod 16), D = the bit reversal of four bits -- sixteen records, two bits of the word each
__device__ __forceinline__ uint32_t interleaved_word(const ModArgs &a, int s, int n_cif, int t, int cw) {
    uint32_t v = 0u;
#pragma unroll
    for (int d = 0; d < TDI_DEPTH; d++) {
        const int kk = ((d & 1) << 3) | ((d & 2) << 1) | ((d & 4) >> 1) | (d >> 3);
        const uint32_t mask = (1u << kk) | (1u << (kk + 16));
        const int r = t - d;
        uint32_t w = 0u;
        if (r >= 0) w = a.coded[(size_t(s) * n_cif + r) * MOD_CODED_WORDS + MOD_FIC_WORDS + cw];
        else if (a.state_in) w = a.state_in[s].cif[MOD_DEPTH + r][cw];
        v |= w & mask;
    }
    return v;
}

// word W of the 7200 that hold a transmission frame's 230 400 bits
__device__ __forceinline__ uint32_t frame_word(const ModArgs &a, int s, int n_cif, int f, int W) {
    if (W < 4 * MOD_FIC_WORDS) return a.coded[(size_t(s) * n_cif + 4 * f + W / MOD_FIC_WORDS) * MOD_CODED_WORDS + W % MOD_FIC_WORDS];
    const int m = W - 4 * MOD_FIC_WORDS;
    return interleaved_word(a, s, n_cif, 4 * f + m / MOD_CIF_WORDS, m % MOD_CIF_WORDS);
}

__global__ __launch_bounds__(MOD_PHASE_WG) void mod_phase_kernel(ModArgs a) {
    const long long g = (long long)blockIdx.x * MOD_PHASE_WG + threadIdx.x;
    const long long n_frames = (long long)a.n_streams * a.frames_per_stream;
    const long long frame = g / (MOD_SYM_WORDS / 2);
    const int w = int(g % (MOD_SYM_WORDS / 2));
    if (frame >= n_frames) return;
    const int s = int(frame / a.frames_per_stream), f = int(frame % a.frames_per_stream);
    const int n_cif = a.frames_per_stream * 4;
    uint32_t *cum = a.cum + size_t(frame) * NB_DATA_SYMBOLS * MOD_SYM_WORDS;
    uint32_t lo = 0u, hi = 0u;
    for (int l = 0; l < NB_DATA_SYMBOLS; l++) {
        const uint32_t p0 = frame_word(a, s, n_cif, f, l * MOD_SYM_WORDS + w);
        const uint32_t p1 = frame_word(a, s, n_cif, f, l * MOD_SYM_WORDS + MOD_SYM_WORDS / 2 + w);
        // (p0, p1) = (0,0) (1,0) (1,1) (0,1) is 0, 1, 2, 3 quarter turns on top of the eighth turn every symbol adds
        const uint32_t qlo = p0 ^ p1, qhi = p1;
        hi ^= qhi ^ (lo & qlo);
        lo ^= qlo;
        cum[l * MOD_SYM_WORDS + w] = lo;
        cum[l * MOD_SYM_WORDS + MOD_SYM_WORDS / 2 + w] = hi;
    }
}

// exp(j pi e / 4) for e = 0..7
__device__ __forceinline__ float2 eighth_turn(int e) {
    const float mx = (e & 1) ? SQRT1_2 : ((e & 2) ? 0.0f : 1.0f), my = (e & 1) ? SQRT1_2 : ((e & 2) ? 1.0f : 0.0f);
    return make_float2(((e + 5) & 7) < 3 ? -mx : mx, e > 4 ? -my : my);
}

__global__ __launch_bounds__(MOD_WG) void mod_symbol_kernel(ModTables tab, ModArgs a) {
    __shared__ __attribute__((aligned(16))) float2 t1[NB_FFT];
    __shared__ __attribute__((aligned(16))) float2 x[NB_FFT];
    __shared__ uint32_t s_cum[MOD_SYM_WORDS];
    __shared__ uint32_t s_refused;
    const int tid = threadIdx.x;
    const long long frame = blockIdx.x / MOD_ITEMS;
    const int item = blockIdx.x % MOD_ITEMS;
    float2 *out = a.iq + size_t(frame) * a.frame_stride;
    const float scale = a.gain * MOD_SCALE;

    if (item == 0) {
        // the null symbol, and the frame's status from the headers of its four ETI frames
        if (tid == 0) s_refused = 0u;
        __syncthreads();
        const uint32_t *f0 = reinterpret_cast<const uint32_t *>(a.eti + size_t(frame) * 4 * ETI_FRAME_BYTES);
        for (int i = tid; i < 4 * (2 + a.nst); i += MOD_WG) {
            const int j = i / (2 + a.nst);
            if (!eti_word_fits(a, f0 + j * (ETI_FRAME_BYTES / 4), i % (2 + a.nst))) atomicOr(&s_refused, 1u << j);
        }
        __syncthreads();
        if (tid == 0) {
            const uint32_t fp = (f0[1] >> 21) & 7u;
            ModStatus st;
            st.flags = (s_refused ? uint32_t(MOD_BAD_INPUT) : 0u) | ((fp & 3u) ? uint32_t(MOD_MISALIGNED) : 0u);
            st.refused = uint8_t(s_refused);
            st.reserved[0] = st.reserved[1] = st.reserved[2] = 0;
            a.status[frame] = st;
        }
        float4 *dst = reinterpret_cast<float4 *>(out);
        const float4 *src = reinterpret_cast<const float4 *>(tab.null_symbol);
        for (int i = tid; i < NB_NULL_PERIOD / 2; i += MOD_WG) {
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (src) {
                v = src[i];
                v = make_float4(v.x * a.gain, v.y * a.gain, v.z * a.gain, v.w * a.gain);
            }
            dst[i] = v;
        }
        return;
    }

    const int l = item - 1;                                    // 0 = the phase reference symbol
    if (l > 0 && tid < MOD_SYM_WORDS) s_cum[tid] = a.cum[(size_t(frame) * NB_DATA_SYMBOLS + (l - 1)) * MOD_SYM_WORDS + tid];
    __syncthreads();
    float2 v[8];
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int b = tid + r * MOD_WG;
        const int n = tab.n_of_bin[b];
        float2 z = make_float2(0.0f, 0.0f);
        if (n >= 0) {
            int e = 2 * tab.prs_qt[b];
            if (l > 0) {
                const uint32_t lo = (s_cum[n >> 5] >> (n & 31)) & 1u, hi = (s_cum[MOD_SYM_WORDS / 2 + (n >> 5)] >> (n & 31)) & 1u;
                e += l + 2 * int(lo + 2u * hi);
            }
            z = eighth_turn((8 - (e & 7)) & 7);                // the conjugate: the forward transform then gives the conjugate of the inverse
        }
        v[r] = z;
    }
    block_fft2048(v, t1, x, tab.twiddle, tab.twiddle + TWC8_OFF, tab.twiddle + TWC64_OFF, tid);
    // sample o of the symbol is t[(o + 2048 - 504) mod 2048]: pairs of samples, the prefix first
    float4 *dst = reinterpret_cast<float4 *>(out + NB_NULL_PERIOD + size_t(l) * NB_SYM_PERIOD);
    for (int i = tid; i < NB_SYM_PERIOD / 2; i += MOD_WG) {
        const float4 t = reinterpret_cast<const float4 *>(x)[(i + (NB_FFT - NB_CP) / 2) & (NB_FFT / 2 - 1)];
        dst[i] = make_float4(t.x * scale, -t.y * scale, t.z * scale, -t.w * scale);
    }
}

// t[n] = sum over the transmitter's 32 carriers of R[k] exp(2 pi j k n / 2048) / sqrt(1536), extended cyclically in front
__global__ __launch_bounds__(MOD_WG) void mod_tii_kernel(const int8_t *prs_qt, int pattern, int sub_id, float2 *out) {
    const int i = blockIdx.x * MOD_WG + threadIdx.x;
    if (i >= NB_NULL_PERIOD) return;
    const int n = (i + NB_FFT - (NB_NULL_PERIOD - NB_FFT)) & (NB_FFT - 1);
    float sx = 0.0f, sy = 0.0f;
    for (int b = 0; b < TII_POSITIONS; b++) {
        if (!((pattern >> (7 - b)) & 1)) continue;
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int k = tii_base(q) + 2 * sub_id + 48 * b + h;
                const int bin = (k + NB_FFT) & (NB_FFT - 1);
                const int ph = (bin * n + 512 * prs_qt[bin]) & (NB_FFT - 1);        // 2048ths of a turn
                float sn, cs;
                sincospif(float(ph) * (1.0f / 1024.0f), &sn, &cs);
                sx += cs;
                sy += sn;
            }
    }
    out[i] = make_float2(sx * MOD_SCALE, sy * MOD_SCALE);
}

}  // namespace

hipError_t launch_mod_encode(const ModTables &t, const ModArgs &a, hipStream_t s) {
    if (a.n_streams <= 0 || a.frames_per_stream <= 0) return hipSuccess;
    if (!t.prbs || !a.eti || !a.coded || !a.cum || a.n_codes != a.nst + 1) return hipErrorInvalidValue;
    const int n_cif = a.frames_per_stream * 4;
    const int carry = n_cif < MOD_DEPTH ? MOD_DEPTH - n_cif : 0;
    hipLaunchKernelGGL(mod_encode_kernel, dim3(unsigned(a.n_streams) * unsigned(n_cif + carry)), dim3(MOD_WG), 0, s, t, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const long long threads = (long long)a.n_streams * a.frames_per_stream * (MOD_SYM_WORDS / 2);
    hipLaunchKernelGGL(mod_phase_kernel, dim3(unsigned((threads + MOD_PHASE_WG - 1) / MOD_PHASE_WG)), dim3(MOD_PHASE_WG), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_mod_symbols(const ModTables &t, const ModArgs &a, hipStream_t s) {
    if (a.n_streams <= 0 || a.frames_per_stream <= 0) return hipSuccess;
    if (!t.n_of_bin || !t.prs_qt || !t.twiddle || !a.eti || !a.cum || !a.iq || !a.status) return hipErrorInvalidValue;
    const long long items = (long long)a.n_streams * a.frames_per_stream * MOD_ITEMS;
    hipLaunchKernelGGL(mod_symbol_kernel, dim3(unsigned(items)), dim3(MOD_WG), 0, s, t, a);
    return hipGetLastError();
}

hipError_t launch_mod_tii(const int8_t *prs_qt, int main_id, int sub_id, float2 *out, hipStream_t s) {
    if (!prs_qt || !out || main_id < 0 || main_id >= TII_PATTERNS || sub_id < 0 || sub_id >= TII_COMBS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mod_tii_kernel, dim3((NB_NULL_PERIOD + MOD_WG - 1) / MOD_WG), dim3(MOD_WG), 0, s, prs_qt,
                       tii_pattern_mask(main_id), sub_id, out);
    return hipGetLastError();
}

}  // namespace dabk
