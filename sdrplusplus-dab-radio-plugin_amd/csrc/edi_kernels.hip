// edi_kernels.hip -- decoded ensembles written as EDI: one AF packet per CIF (include/dabgpu_edi.h, the contract;
// include/dabgpu.h, "EDI output").
//
// The first launch is the ETI writer's own pre-pass (eti_anchor_kernel: the anchor of the CIF count, the history record).
// edi_packet_kernel   one wave per packet, four packets per workgroup.  What the packet says about its CIF -- FIC or
//                     warm-up, count, STAT, flags -- is eti_cif(), the ETI writer's decision.  The packet is put together
//                     in LDS at the 16-byte phase its place in the output stream has (packets are 12 + 8 k bytes and lie
//                     back to back, so the phases 0, 4, 8 and 12 all occur): the 40 fixed bytes and the est heads from
//                     the header's prefix_byte / est_head_byte, the FIC as words, every sub-channel's bytes loaded as
//                     8-byte words and stored as bytes (an est head is 11 bytes: no two items share an alignment).  The
//                     CRC is folded a chunk of bytes per lane as the ETI writer folds its data CRC, and the packet
//                     leaves through wave_copy: 16-byte stores between an unaligned head and tail.
#include "eti_cif.hpp"
#include "wave_copy.hpp"

#include "../../include/dabgpu_edi.h"

namespace dabk {

namespace {

namespace edi = dabgpu_edi;

constexpr int EDI_WG = 256;
constexpr int EDI_WAVES = EDI_WG / 64;
constexpr int EDI_BUF = EDI_MAX_WRITER_PACKET + 16;         // a packet behind its phase
constexpr int EDI_MAP_WORDS = 768;                           // 8-byte words of sub-channel data a CIF can hold
static_assert(sizeof(EdiArgs) <= 4096, "passed by value");
static_assert(EDI_BUF % 16 == 0 && EDI_MAX_WRITER_PACKET >= edi::packet_bytes(ETI_MAX_STREAMS, ETI_FRAME_BYTES - 116 - 4 * ETI_MAX_STREAMS),
              "the largest plan an ETI frame holds");

__global__ __launch_bounds__(EDI_WG) void edi_packet_kernel(EdiArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t s_pkt[EDI_WAVES][EDI_BUF];
    __shared__ unsigned long long s_src[ETI_MAX_STREAMS];      // address of sub-channel k's data minus its offset among the data
    __shared__ uint32_t s_bytes[ETI_MAX_STREAMS];
    __shared__ uint16_t s_at[ETI_MAX_STREAMS];                 // where est item k + 1 begins in the packet
    __shared__ uint16_t s_tab[256];
    __shared__ uint8_t s_stc[4 * ETI_MAX_STREAMS];
    __shared__ uint8_t s_map[EDI_MAP_WORDS];                   // 8-byte word of the data -> sub-channel
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_cif = a.frames_per_stream * 4;
    const long long total = (long long)a.n_streams * n_cif;
    const long long g = (long long)blockIdx.x * EDI_WAVES + wave;
    const bool live = g < total;

    s_tab[tid] = eti_crc_table_entry(tid);
    if (tid < a.nst) {
        s_src[tid] = (unsigned long long)(uintptr_t)a.out[tid] - a.offset[tid];
        s_bytes[tid] = a.bytes[tid];
        s_at[tid] = uint16_t(edi::W_EST_AT + edi::EST_HEAD_BYTES * tid + a.offset[tid]);
    }
    if (tid < 4 * a.nst) s_stc[tid] = a.stc[tid];
    for (int k = 0; k < a.nst; k++) {
        const int first = a.offset[k] >> 3, n = a.bytes[k] >> 3;
        for (int w = tid; w < n; w += EDI_WG) s_map[first + w] = uint8_t(k);
    }
    __syncthreads();

    const int s = live ? int(g / n_cif) : 0, t = live ? int(g % n_cif) : 0;
    const size_t row = size_t(s) * n_cif + t;
    const int P = a.packet_bytes, L = P - 2;
    const int n_w8 = a.data_bytes >> 3;
    uint8_t *dst = a.edi + size_t(s) * a.stream_stride + size_t(t) * size_t(P);
    uint8_t *B = s_pkt[wave] + (live ? int((size_t(t) * size_t(P)) & 15) : 0);
    uint32_t flags = 0, fib_ok = 0;
    int count = 0;
    if (live) {
        const EtiCif cif = eti_cif(a.fib, a.crc_ok, a.history_in, a.base, s, t, n_cif);
        count = cif.count;
        fib_ok = cif.fib_ok;
        flags = cif.flags;
        const uint32_t seq = ((a.seq_start ? a.seq_start[s] : 0u) + uint32_t(t)) & 0xffffu;
        if (lane < edi::W_PREFIX_BYTES) B[lane] = uint8_t(edi::prefix_byte(lane, uint32_t(P - edi::AF_OVERHEAD), seq, uint32_t(count), cif.err));
        if (lane < ETI_FIC_BYTES / 4)
            reinterpret_cast<uint32_t *>(B + edi::W_FIC_AT)[lane] = cif.fic ? reinterpret_cast<const uint32_t *>(cif.fic)[lane] : 0u;
        for (int idx = lane; idx < edi::EST_HEAD_BYTES * a.nst; idx += 64) {
            const int k = idx / edi::EST_HEAD_BYTES, i = idx - edi::EST_HEAD_BYTES * k;
            B[s_at[k] + i] = uint8_t(edi::est_head_byte(i, k + 1, s_stc + 4 * k));
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
                    const int k = s_map[w];
                    uint8_t *d = B + edi::W_EST_AT + edi::EST_HEAD_BYTES * (k + 1) + 8 * w;
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        d[i] = uint8_t(v[u].x >> (8 * i));
                        d[4 + i] = uint8_t(v[u].y >> (8 * i));
                    }
                }
            }
        }
        // the payload's padding
        for (int i = edi::W_EST_AT + edi::EST_HEAD_BYTES * a.nst + a.data_bytes + lane; i < L; i += 64) B[i] = 0;
    }
    __syncthreads();
    if (live) {
        // lane i folds bytes [i C - lead, (i + 1) C - lead) of the packet: `lead` zero bytes stand in front of it
        const int lead = 64 * a.chunk_bytes - L;
        uint32_t crc = 0;
        for (int j = 0; j < a.chunk_bytes; j++) {
            const int m = lane * a.chunk_bytes + j - lead;
            if (m >= 0) crc = ((crc << 8) & 0xffffu) ^ s_tab[(crc >> 8) ^ B[m]];
        }
        uint32_t r = eti_gf_mul(crc, a.lane_shift[lane], 16);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) r ^= uint32_t(__shfl_xor(int(r), d, 64));
        r = (r ^ a.crc_init ^ 0xffffu) & 0xffffu;
        if (lane == 0) {
            B[L] = uint8_t(r >> 8);
            B[L + 1] = uint8_t(r & 0xffu);
        }
    }
    __syncthreads();
    if (live) {
        wave_copy(dst, B, P, lane);
        if (lane == 0) {
            EtiStatus st;
            st.cif_count = uint16_t(count);
            st.flags = uint8_t(flags);
            st.fib_ok = uint8_t(fib_ok);
            st.length = uint16_t(P);
            st.reserved = 0;
            a.status[row] = st;
        }
    }
}

}  // namespace

hipError_t launch_edi(const EtiAnchorArgs &p, const EdiArgs &a, hipStream_t s) {
    if (a.n_streams <= 0 || a.frames_per_stream <= 0) return hipSuccess;
    const size_t span = size_t(a.frames_per_stream) * 4u * size_t(a.packet_bytes > 0 ? a.packet_bytes : 0);
    if (!a.fib || !a.crc_ok || !a.base || !a.edi || !a.status || p.base != a.base || p.n_streams != a.n_streams ||
        p.frames_per_stream != a.frames_per_stream || a.nst < 0 || a.nst > ETI_MAX_STREAMS ||
        a.packet_bytes != dabgpu_edi::packet_bytes(a.nst, a.data_bytes) || a.packet_bytes > EDI_MAX_WRITER_PACKET ||
        a.data_bytes > 8 * EDI_MAP_WORDS || a.stream_stride < span || (a.stream_stride & 15u) ||
        (reinterpret_cast<uintptr_t>(a.edi) & 15u) || 64 * a.chunk_bytes < a.packet_bytes - 2)
        return hipErrorInvalidValue;
    hipError_t e = launch_eti_anchor(p, s);
    if (e != hipSuccess) return e;
    const long long total = (long long)a.n_streams * a.frames_per_stream * 4;
    hipLaunchKernelGGL(edi_packet_kernel, dim3(unsigned((total + EDI_WAVES - 1) / EDI_WAVES)), dim3(EDI_WG), 0, s, a);
    return hipGetLastError();
}

}  // namespace dabk
