// pft_kernels.hip -- AF packets written as PF fragments with RS(255,207) parity (include/dabgpu.h, "EDI PFT layer"; the
// format and the layout rule: include/dabgpu_pft.h).
//
// pft_fragments_kernel   a workgroup per (packet, stream).  The packet and its zero bytes come into LDS as the front of the
//                        RS block; every fragment's header is made with its HCRC by a lane of its own; a lane per (chunk,
//                        parity byte) then sums what each of the chunk's k data bytes adds to that byte -- the table of
//                        x^(48 + r) mod generator is made by the compiler, so no lane waits for another and there is no
//                        serial division -- and the packet's fragments leave as one byte range, by the interleave rule,
//                        in whole words between its unaligned ends.
#include "kernels.hpp"

#include "../../include/dabgpu_pft.h"

namespace dabk {

namespace {

namespace pf = dabgpu_pft;

constexpr int WG = 256;
constexpr int BLOCK_ROOM = pf::MAX_CHUNKS * (pf::RS_K + pf::PARITY);        // >= MAX_PACKET
static_assert(BLOCK_ROOM >= pf::MAX_PACKET && BLOCK_ROOM % 4 == 0 && sizeof(pf::Gf) == 192 * 4, "the block holds a packet without FEC too");

__device__ const pf::Gf GF_TABLES = pf::make_gf();
__device__ const pf::ParityTable PARITY_TABLE = pf::make_parity_table();

__global__ __launch_bounds__(WG) void pft_fragments_kernel(PftArgs a) {
    __shared__ pf::Gf g;
    __shared__ __attribute__((aligned(16))) uint8_t s_block[BLOCK_ROOM];
    __shared__ uint8_t s_head[pf::MAX_FRAGMENTS][pf::MAX_HEADER];
    const int tid = threadIdx.x;
    const unsigned pkt = blockIdx.x, stream = blockIdx.y;
    if (tid < 192) reinterpret_cast<uint32_t *>(&g)[tid] = reinterpret_cast<const uint32_t *>(&GF_TABLES)[tid];
    const int l = a.packet_bytes, f = a.fcount, s = a.plen, hl = a.header_bytes, c = a.chunks, k = a.rs_k;
    const uint8_t *af = a.af + size_t(stream) * a.in_stride + size_t(pkt) * size_t(l);
    const int front = a.fec ? c * k : l;
    for (int i = tid; i < front; i += WG) s_block[i] = i < l ? af[i] : uint8_t(0);
    const uint32_t pseq = (a.pseq_start[stream] + pkt) & 0xFFFFu;
    for (int n = tid; n < f; n += WG) {
        pf::FragHeader h;
        h.pseq = pseq;
        h.findex = uint32_t(n);
        h.fcount = uint32_t(f);
        h.fec = uint32_t(a.fec);
        h.addr = uint32_t(a.addr);
        h.plen = uint32_t(a.fec || n + 1 < f ? s : l - (f - 1) * s);
        h.rs_k = uint32_t(k);
        h.rs_z = uint32_t(a.rs_z);
        h.source = a.addr ? a.source & 0xFFFFu : 0u;
        h.dest = a.addr ? a.dest & 0xFFFFu : 0u;
        h.header_bytes = uint32_t(hl);
        uint8_t *dst = s_head[n];
        pf::write_header([dst](int i, uint8_t b) { dst[i] = b; }, h);
    }
    __syncthreads();
    if (a.fec) {
        // parity byte q of chunk i lies at c k + 48 i + q
        for (int t = tid; t < pf::PARITY * c; t += WG) {
            const uint8_t *d = s_block + (t / pf::PARITY) * k;
            s_block[c * k + t] = uint8_t(pf::parity_byte(g, PARITY_TABLE, [d](int j) -> unsigned { return d[j]; }, k, t % pf::PARITY));
        }
        __syncthreads();
    }
    // byte o of the packet's fragments (only the last fragment without FEC is shorter than hl + s)
    const int fb = hl + s, B = a.block_bytes;
    const auto byte_at = [&](uint32_t o) -> uint32_t {
        const uint32_t n = o / uint32_t(fb), r = o - n * uint32_t(fb);
        if (r < uint32_t(hl)) return s_head[n][r];
        const uint32_t j = r - uint32_t(hl);
        if (!a.fec) return s_block[n * uint32_t(s) + j];
        const uint32_t idx = j * uint32_t(f) + n;
        return idx < uint32_t(B) ? s_block[idx] : 0u;
    };
    uint8_t *out = a.pf + size_t(stream) * a.out_stride + size_t(pkt) * size_t(a.stream_bytes);
    const uint32_t total = uint32_t(a.stream_bytes);
    const uint32_t lead = min(uint32_t(-reinterpret_cast<uintptr_t>(out)) & 3u, total), words = (total - lead) / 4u;
    if (uint32_t(tid) < lead) out[tid] = uint8_t(byte_at(uint32_t(tid)));
    uint32_t *out32 = reinterpret_cast<uint32_t *>(out + lead);
    for (uint32_t w = uint32_t(tid); w < words; w += WG) {
        const uint32_t o = lead + 4u * w;
        out32[w] = byte_at(o) | (byte_at(o + 1u) << 8) | (byte_at(o + 2u) << 16) | (byte_at(o + 3u) << 24);
    }
    const uint32_t done = lead + 4u * words;
    if (done + uint32_t(tid) < total) out[done + uint32_t(tid)] = uint8_t(byte_at(done + uint32_t(tid)));
}

}  // namespace

hipError_t launch_pft(const PftArgs &a, int n_streams, int n_packets, hipStream_t s) {
    if (n_streams <= 0 || n_packets <= 0) return hipSuccess;
    if (n_streams > 65535 || a.fcount < 1 || a.fcount > pf::MAX_FRAGMENTS || a.header_bytes > pf::MAX_HEADER || a.packet_bytes > pf::MAX_PACKET ||
        (a.fec ? a.block_bytes : a.packet_bytes) > BLOCK_ROOM)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(pft_fragments_kernel, dim3(unsigned(n_packets), unsigned(n_streams)), dim3(WG), 0, s, a);
    return hipGetLastError();
}

}  // namespace dabk
