// eti_kernels.hip -- decoded ensembles written as ETI(NI) frames (include/dabgpu.h, "ETI(NI) output").
//
// eti_anchor_kernel   one workgroup per stream: finds the call's first CIF whose first FIB is valid and begins with FIG 0/0
//                     (the anchor of the CIF count), settles the count of the call's first CIF, and moves the FIC of the last
//                     15 CIFs into the history record the next call continues from.
// eti_frame_kernel    one wave per output frame, four frames per workgroup.  The frame is put together in LDS -- the
//                     header from the plan's constant part, the CIF's 96 FIC bytes, every sub-channel's bytes gathered in
//                     8-byte words (sub-channel sizes are multiples of 24 bytes, the header one of 4: LDS takes the
//                     misalignment, global memory sees whole 16-byte stores) -- then the data CRC is folded over it and
//                     the 6144 bytes leave as six 16-byte stores per lane.
//
// The data CRC (FIC + sub-channels, up to ~5.5 KB) is not a serial chain: CRC-16 is linear over GF(2).  The data, padded
// with zero bytes IN FRONT to 64 equal chunks (leading zeros do not move a CRC that starts from zero), is folded chunk per
// lane from a zero start with a 256-entry table in LDS; lane i's remainder is multiplied by x^(8 C (63 - i)) mod P -- its
// chunk's way to the end of the data, a per-call constant from the host -- and the 64 products are added with six
// cross-lane exchanges.  The start value 0xFFFF contributes 0xFFFF x^(8 L) mod P, one more constant, and the result is
// inverted.  The header CRC changes from frame to frame only through FCT and FP: the host computes it once with both
// zero and the kernel adds the two bytes' own remainders.
#include "eti_cif.hpp"

namespace dabk {

namespace {

static_assert(sizeof(EtiHistory) == 1504 && sizeof(EtiStatus) == 8, "mirror dabgpu_eti_history / dabgpu_eti_status");
static_assert(sizeof(EtiArgs) <= 4096, "passed by value");

constexpr int ETI_WG = 256;
constexpr int ETI_WAVES = ETI_WG / 64;
constexpr int ETI_FRAME_WORDS = ETI_FRAME_BYTES / 4;
constexpr int ETI_FIC_WORDS = ETI_FIC_BYTES / 4;
constexpr int ETI_MAP_WORDS = 768;             // 8-byte words of sub-channel data a frame can hold (< 6144 / 8)

__global__ __launch_bounds__(ETI_WG) void eti_anchor_kernel(EtiAnchorArgs p) {
    __shared__ int s_anchor;
    const int tid = threadIdx.x, s = blockIdx.x;
    const int n_cif = p.frames_per_stream * 4;
    const uint8_t *fib = p.fib + size_t(s) * n_cif * ETI_FIC_BYTES;         // [n_cif][96]: 4 groups of 3 FIBs per frame
    const uint8_t *ok = p.crc_ok + size_t(s) * n_cif * 3;
    const EtiHistory *hin = p.history_in ? p.history_in + s : nullptr;
    const int valid_in = eti_history_valid(hin);
    if (tid == 0) s_anchor = 0x7fffffff;
    __syncthreads();
    for (int c = tid; c < n_cif; c += ETI_WG) {
        const uint32_t *w = reinterpret_cast<const uint32_t *>(fib + size_t(c) * ETI_FIC_BYTES);
        if (eti_fig0_0_count(w[0], w[1], ok[c * 3]) >= 0) {
            atomicMin(&s_anchor, c);
            break;
        }
    }
    __syncthreads();
    const int anchor = s_anchor;
    int base, no_anchor = 0;
    const int start = p.cif_start ? p.cif_start[s] : -1;
    if (start >= 0) {
        base = start % ETI_CIF_COUNTS;
    } else if (anchor < n_cif) {
        const uint32_t *w = reinterpret_cast<const uint32_t *>(fib + size_t(anchor) * ETI_FIC_BYTES);
        const int count = eti_fig0_0_count(w[0], w[1], 1);
        base = (count + ETI_CIF_COUNTS - anchor % ETI_CIF_COUNTS) % ETI_CIF_COUNTS;
    } else {
        no_anchor = 1;
        base = valid_in > 0 ? int(uint32_t(hin->next_count) % uint32_t(ETI_CIF_COUNTS)) : 0;
    }
    if (tid == 0) p.base[s] = base | (no_anchor << 16);
    if (!p.history_out) return;
    EtiHistory *hout = p.history_out + s;
    // slot j of the new record is CIF n_cif - 15 + j of this call, or (a call shorter than 15 CIFs) slot n_cif + j of the old one
    for (int i = tid; i < ETI_FIC_DELAY * ETI_FIC_WORDS; i += ETI_WG) {
        const int j = i / ETI_FIC_WORDS, word = i % ETI_FIC_WORDS;
        const int c = n_cif - ETI_FIC_DELAY + j;
        uint32_t v = 0;
        if (c >= 0) v = reinterpret_cast<const uint32_t *>(fib + size_t(c) * ETI_FIC_BYTES)[word];
        else if (n_cif + j >= ETI_FIC_DELAY - valid_in) v = reinterpret_cast<const uint32_t *>(hin->fib[n_cif + j])[word];
        reinterpret_cast<uint32_t *>(hout->fib[j])[word] = v;
    }
    if (tid < ETI_FIC_DELAY * 3 + 3) {
        const int j = tid / 3, b = tid % 3;
        const int c = n_cif - ETI_FIC_DELAY + j;
        uint8_t v = 0;
        if (j < ETI_FIC_DELAY) {
            if (c >= 0) v = ok[c * 3 + b];
            else if (n_cif + j >= ETI_FIC_DELAY - valid_in) v = hin->crc_ok[n_cif + j][b];
        }
        (&hout->crc_ok[0][0])[tid] = v;                                     // the 3 bytes of padding behind the flags too
    }
    if (tid == 0) {
        const long long held = (long long)valid_in + n_cif;
        hout->next_count = int((long long)(base + n_cif % ETI_CIF_COUNTS) % ETI_CIF_COUNTS);
        hout->valid = held > ETI_FIC_DELAY ? ETI_FIC_DELAY : int(held);
        hout->reserved[0] = 0;
        hout->reserved[1] = 0;
    }
}

__global__ __launch_bounds__(ETI_WG) void eti_frame_kernel(EtiArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t s_frame[ETI_WAVES][ETI_FRAME_WORDS];
    __shared__ unsigned long long s_src[ETI_MAX_STREAMS];      // address of sub-channel k's data minus its offset in the frame
    __shared__ uint32_t s_bytes[ETI_MAX_STREAMS];
    __shared__ uint16_t s_tab[256];
    __shared__ uint8_t s_map[ETI_MAP_WORDS];                   // 8-byte word of the data -> sub-channel
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_cif = a.frames_per_stream * 4;
    const long long total = (long long)a.n_streams * n_cif;
    const long long g = (long long)blockIdx.x * ETI_WAVES + wave;
    const bool live = g < total;
    uint32_t *W = s_frame[wave];

    // per workgroup: the byte table of the CRC, the sub-channel of every data word, the sources
    s_tab[tid] = eti_crc_table_entry(tid);
    if (tid < a.nst) {
        s_src[tid] = (unsigned long long)(uintptr_t)a.out[tid] - a.offset[tid];
        s_bytes[tid] = a.bytes[tid];
    }
    for (int k = 0; k < a.nst; k++) {
        const int first = a.offset[k] >> 3, n = a.bytes[k] >> 3;
        for (int w = tid; w < n; w += ETI_WG) s_map[first + w] = uint8_t(k);
    }
#pragma unroll
    for (int j = 0; j < ETI_FRAME_BYTES / 16 / 64; j++)
        reinterpret_cast<uint4 *>(W)[lane + 64 * j] = make_uint4(0x55555555u, 0x55555555u, 0x55555555u, 0x55555555u);
    __syncthreads();

    const int s = live ? int(g / n_cif) : 0, t = live ? int(g % n_cif) : 0;
    const size_t row = size_t(s) * n_cif + t;
    const int fic_word = 3 + a.nst;                            // ERR/FSYNC, FC, STC, MNSC/CRC come first
    const int data_word = fic_word + ETI_FIC_WORDS;
    const int n_w8 = a.data_bytes >> 3;
    uint32_t flags = 0, fib_ok = 0;
    int count = 0;
    if (live) {
        const EtiCif cif = eti_cif(a.fib, a.crc_ok, a.history_in, a.base, s, t, n_cif);
        count = cif.count;
        fib_ok = cif.fib_ok;
        flags = cif.flags;
        if (lane < ETI_FIC_WORDS) W[fic_word + lane] = cif.fic ? reinterpret_cast<const uint32_t *>(cif.fic)[lane] : 0u;
        const uint32_t fct = uint32_t(count % 250), fp = uint32_t(count & 7) << 5;
        if (lane < a.nst) W[2 + lane] = a.header[2 + lane];
        if (lane == 0) {
            W[0] = cif.err | ((fct & 1u) ? 0x49C5F800u : 0xB63A0700u);
            W[1] = a.header[1] | fct | (fp << 16);
            const uint32_t hc = uint32_t(a.header_crc0) ^ eti_gf_mul(a.fct_shift, fct, 8) ^ eti_gf_mul(a.fp_shift, fp, 8);
            W[2 + a.nst] = 0xFFFFu | ((hc >> 8) << 16) | ((hc & 0xffu) << 24);
        }
        // the sub-channels' bytes of this CIF: 8-byte words, four loads in flight per lane
        for (int w0 = lane; w0 < n_w8; w0 += 4 * 64) {
            uint2 v[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int w = w0 + 64 * u;
                if (w < n_w8) {
                    const int k = s_map[w];
                    v[u] = *reinterpret_cast<const uint2 *>(uintptr_t(s_src[k] + row * s_bytes[k] + (unsigned long long)w * 8u));
                }
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int w = w0 + 64 * u;
                if (w < n_w8) {
                    W[data_word + 2 * w] = v[u].x;
                    W[data_word + 2 * w + 1] = v[u].y;
                }
            }
        }
    }
    __syncthreads();
    if (live) {
        // lane i folds padded words [i C/4, (i + 1) C/4); the first `lead` padded words are the zeros in front
        const int n_words = ETI_FIC_WORDS + 2 * n_w8;
        const int lead = 64 * a.chunk_words - n_words;
        uint32_t crc = 0;
        for (int j = 0; j < a.chunk_words; j++) {
            const int m = lane * a.chunk_words + j - lead;
            if (m >= 0) {
                const uint32_t v = W[fic_word + m];
                crc = ((crc << 8) & 0xffffu) ^ s_tab[(crc >> 8) ^ (v & 0xffu)];
                crc = ((crc << 8) & 0xffffu) ^ s_tab[(crc >> 8) ^ ((v >> 8) & 0xffu)];
                crc = ((crc << 8) & 0xffffu) ^ s_tab[(crc >> 8) ^ ((v >> 16) & 0xffu)];
                crc = ((crc << 8) & 0xffffu) ^ s_tab[(crc >> 8) ^ (v >> 24)];
            }
        }
        uint32_t r = eti_gf_mul(crc, a.lane_shift[lane], 16);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) r ^= uint32_t(__shfl_xor(int(r), d, 64));
        r = (r ^ a.data_init ^ 0xffffu) & 0xffffu;
        if (lane == 0) {
            W[data_word + 2 * n_w8] = (r >> 8) | ((r & 0xffu) << 8) | 0xFFFF0000u;
            W[data_word + 2 * n_w8 + 1] = 0xFFFFFFFFu;
        }
    }
    __syncthreads();
    if (live) {
        uint4 *dst = reinterpret_cast<uint4 *>(a.eti + row * ETI_FRAME_BYTES);
#pragma unroll
        for (int j = 0; j < ETI_FRAME_BYTES / 16 / 64; j++) dst[lane + 64 * j] = reinterpret_cast<const uint4 *>(W)[lane + 64 * j];
        if (lane == 0) {
            EtiStatus st;
            st.cif_count = uint16_t(count);
            st.flags = uint8_t(flags);
            st.fib_ok = uint8_t(fib_ok);
            st.length = uint16_t(4 * (data_word + 2 * n_w8 + 2));
            st.reserved = 0;
            a.status[row] = st;
        }
    }
}

}  // namespace

hipError_t launch_eti_anchor(const EtiAnchorArgs &p, hipStream_t s) {
    if (p.n_streams <= 0 || p.frames_per_stream <= 0) return hipSuccess;
    if (!p.fib || !p.crc_ok || !p.base) return hipErrorInvalidValue;
    hipLaunchKernelGGL(eti_anchor_kernel, dim3(unsigned(p.n_streams)), dim3(ETI_WG), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_eti(const EtiAnchorArgs &p, const EtiArgs &a, hipStream_t s) {
    if (a.n_streams <= 0 || a.frames_per_stream <= 0) return hipSuccess;
    if (!a.fib || !a.crc_ok || !a.base || !a.eti || !a.status || p.base != a.base || p.n_streams != a.n_streams ||
        p.frames_per_stream != a.frames_per_stream)
        return hipErrorInvalidValue;
    hipError_t e = launch_eti_anchor(p, s);
    if (e != hipSuccess) return e;
    const long long total = (long long)a.n_streams * a.frames_per_stream * 4;
    hipLaunchKernelGGL(eti_frame_kernel, dim3(unsigned((total + ETI_WAVES - 1) / ETI_WAVES)), dim3(ETI_WG), 0, s, a);
    return hipGetLastError();
}

}  // namespace dabk
