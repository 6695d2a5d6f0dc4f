// dabgpu_pft_api.hip -- the C ABI of the PFT layer of EDI (include/dabgpu.h, "EDI PFT layer"): the layout rule, the writer
// (AF packets -> PF fragments) and the reader (PF fragment byte streams -> AF packet byte streams), each on device memory and
// as a twin on host memory (no context, no GPU: the serial code of include/dabgpu_pft.h).
#include "dabgpu_ctx.hpp"

#include <cstddef>
#include <cstring>

#include "../../include/dabgpu_pft.h"

using namespace dabapi;
namespace pf = dabgpu_pft;

static_assert(sizeof(dabgpu_pft_layout_info) == sizeof(pf::Layout) && sizeof(dabgpu_pft_read_record) == sizeof(pf::Record) &&
                  sizeof(dabgpu_pft_read_result) == sizeof(pf::Result),
              "ABI structs mirror the header's");
static_assert(offsetof(dabgpu_pft_layout_info, guaranteed_losses) == offsetof(pf::Layout, guaranteed_losses) &&
                  offsetof(dabgpu_pft_layout_info, stream_bytes) == offsetof(pf::Layout, stream_bytes) &&
                  offsetof(dabgpu_pft_read_record, flags) == offsetof(pf::Record, flags) &&
                  offsetof(dabgpu_pft_read_record, dest) == offsetof(pf::Record, dest) &&
                  offsetof(dabgpu_pft_read_record, max_erasures) == offsetof(pf::Record, max_erasures) &&
                  offsetof(dabgpu_pft_read_result, bytes_filled) == offsetof(pf::Result, bytes_filled),
              "... field for field");
static_assert(DABGPU_PFT_FEC == pf::FLAG_FEC && DABGPU_PFT_ADDR == pf::FLAG_ADDR && DABGPU_PFT_RECOVERED == pf::FLAG_RECOVERED &&
                  DABGPU_PFT_INCONSISTENT == pf::FLAG_INCONSISTENT && DABGPU_PFT_LOST == pf::FLAG_LOST && DABGPU_PFT_AF_OK == pf::FLAG_AF_OK &&
                  DABGPU_PFT_FLUSHED == pf::FLAG_FLUSHED && DABGPU_PFT_READ_FLUSH == pf::READ_FLUSH,
              "the header's values are the ABI's");

namespace {

constexpr int32_t PFT_READ_MAX_BYTES = 1 << 30;
const pf::Gf GF = pf::make_gf();
const pf::ParityTable PARITY_TABLE = pf::make_parity_table();

// a layout is taken only as dabgpu_pft_layout makes it from its first five fields
bool layout_consistent(const dabgpu_pft_layout_info *given, pf::Layout &a) {
    return given && pf::layout(given->packet_bytes, given->fec, given->m, given->max_payload, given->addr, a) &&
           std::memcmp(given, &a, sizeof a) == 0;
}

// everything both writer calls refuse
int fragments_check(const dabgpu_pft_layout_info *layout, int n_streams, int n_packets, const uint8_t *af, size_t in_stride, uint32_t source,
                    uint32_t dest, const uint8_t *out, size_t out_stride, pf::Layout &a) {
    if (!layout_consistent(layout, a) || n_streams < 0 || n_packets < 0 || source > 0xFFFFu || dest > 0xFFFFu) return DABGPU_ERR_ARG;
    if (n_streams > 65535 || uint64_t(n_packets) * uint64_t(a.stream_bytes) >= (uint64_t(1) << 31)) return DABGPU_ERR_ARG;
    if (n_streams == 0 || n_packets == 0) return DABGPU_OK;
    const uint64_t in_bytes = uint64_t(n_packets) * uint64_t(a.packet_bytes), out_bytes = uint64_t(n_packets) * uint64_t(a.stream_bytes);
    if (!af || !out || ((addr(af) | addr(out) | in_stride | out_stride) & 15u) || in_stride < in_bytes || out_stride < out_bytes) return DABGPU_ERR_ARG;
    const uint64_t in_span = uint64_t(n_streams - 1) * in_stride + in_bytes, out_span = uint64_t(n_streams - 1) * out_stride + out_bytes;
    if (overlaps(af, in_span, out, out_span)) return DABGPU_ERR_ARG;
    return DABGPU_OK;
}

// everything both reader calls refuse, before anything is done; fills the kernels' table when there is one
int read_check(const dabgpu_pft_read_entry *entries, int n_entries, dabk::PftReadEntry *table) {
    if (n_entries < 0 || (n_entries > 0 && !entries)) return DABGPU_ERR_ARG;
    for (int i = 0; i < n_entries; i++) {
        const dabgpu_pft_read_entry &e = entries[i];
        if (e.n_bytes < 0 || e.n_bytes > PFT_READ_MAX_BYTES || (e.n_bytes > 0 && !e.d_bytes) || (e.flags & ~DABGPU_PFT_READ_FLUSH)) return DABGPU_ERR_ARG;
        if (!e.d_state_out || !e.d_out || !e.d_records || !e.d_result) return DABGPU_ERR_ARG;
        if ((addr(e.d_bytes) | addr(e.d_state_in) | addr(e.d_state_out) | addr(e.d_out)) & 15) return DABGPU_ERR_ARG;
        if ((addr(e.d_records) | addr(e.d_result)) & 3) return DABGPU_ERR_ARG;
        const uint64_t sb = pf::STATE_BYTES;
        if (e.d_state_in && overlaps(e.d_state_in, sb, e.d_state_out, sb)) return DABGPU_ERR_ARG;
    }
    if (!table) return DABGPU_OK;
    for (int i = 0; i < n_entries; i++) {
        const dabgpu_pft_read_entry &e = entries[i];
        dabk::PftReadEntry &t = table[i];
        t.bytes = addr(e.d_bytes);
        t.state_in = addr(e.d_state_in);
        t.state_out = addr(e.d_state_out);
        t.out = addr(e.d_out);
        t.records = addr(e.d_records);
        t.result = addr(e.d_result);
        t.n_bytes = e.n_bytes;
        t.flags = e.flags;
        t.max_records = pf::read_max_records(uint32_t(e.n_bytes));
    }
    return DABGPU_OK;
}

}  // namespace

extern "C" {

int dabgpu_pft_layout(int packet_bytes, int fec, int m, int max_payload, int addr_fields, dabgpu_pft_layout_info *info) {
    pf::Layout a;
    if (!info || !pf::layout(packet_bytes, fec, m, max_payload, addr_fields, a)) return DABGPU_ERR_ARG;
    std::memcpy(info, &a, sizeof a);
    return DABGPU_OK;
}

int dabgpu_pft_fragments_dev(dabgpu_ctx *ctx, const dabgpu_pft_layout_info *layout, int n_streams, int n_packets, const uint8_t *d_af,
                             size_t in_stride, const uint32_t *pseq_start, uint32_t source, uint32_t dest, uint8_t *d_pf, size_t out_stride,
                             void *stream) {
    if (!ctx) return DABGPU_ERR_ARG;
    pf::Layout a;
    const int bad = fragments_check(layout, n_streams, n_packets, d_af, in_stride, source, dest, d_pf, out_stride, a);
    if (bad) return bad;
    if (n_streams == 0 || n_packets == 0) return DABGPU_OK;
    DeviceGuard guard(ctx);
    hipStream_t s = pick_stream(ctx, stream);
    const size_t stage_bytes = size_t(n_streams) * 4u;
    // (growing the area must not race with a launch that still reads the old one)
    if (ctx->stage_bytes[STAGE_PFT] < stage_bytes) HIP_TRY(hipStreamSynchronize(s));
    void *base = nullptr;
    const int rc = stage(ctx, STAGE_PFT, stage_bytes, &base);
    if (rc) return rc;
    {
        // through a pageable copy: the transfer has left it when hipMemcpyAsync returns, so the caller may add to pseq_start at
        // once, whatever kind of memory it lies in
        std::vector<uint32_t> pseq(size_t(n_streams), 0u);
        if (pseq_start) std::memcpy(pseq.data(), pseq_start, stage_bytes);
        HIP_TRY(hipMemcpyAsync(base, pseq.data(), stage_bytes, hipMemcpyHostToDevice, s));
    }
    dabk::PftArgs k{};
    k.af = d_af;
    k.pf = d_pf;
    k.in_stride = in_stride;
    k.out_stride = out_stride;
    k.pseq_start = static_cast<const uint32_t *>(base);
    k.packet_bytes = a.packet_bytes;
    k.fec = a.fec;
    k.addr = a.addr;
    k.chunks = a.chunks;
    k.rs_k = a.rs_k;
    k.rs_z = a.rs_z;
    k.block_bytes = a.block_bytes;
    k.fcount = a.fcount;
    k.plen = a.plen;
    k.header_bytes = a.header_bytes;
    k.stream_bytes = a.stream_bytes;
    k.source = source;
    k.dest = dest;
    HIP_TRY(dabk::launch_pft(k, n_streams, n_packets, s));
    return DABGPU_OK;
}

int dabgpu_pft_fragments_host(const dabgpu_pft_layout_info *layout, int n_streams, int n_packets, const uint8_t *af, size_t in_stride,
                              const uint32_t *pseq_start, uint32_t source, uint32_t dest, uint8_t *out, size_t out_stride) {
    pf::Layout a;
    const int bad = fragments_check(layout, n_streams, n_packets, af, in_stride, source, dest, out, out_stride, a);
    if (bad) return bad;
    std::vector<uint8_t> block(size_t(a.block_bytes) + 1u);
    for (int s = 0; s < n_streams; s++)
        for (int n = 0; n < n_packets; n++) {
            const uint8_t *src = af + size_t(s) * in_stride + size_t(n) * size_t(a.packet_bytes);
            uint8_t *dst = out + size_t(s) * out_stride + size_t(n) * size_t(a.stream_bytes);
            pf::write_fragments(GF, PARITY_TABLE, a, (pseq_start ? pseq_start[s] : 0u) + uint32_t(n), source, dest,
                                [src](int i) -> unsigned { return src[i]; }, [dst](int i, uint8_t b) { dst[i] = b; }, block.data());
        }
    return DABGPU_OK;
}

size_t dabgpu_pft_read_state_bytes(void) { return size_t(pf::STATE_BYTES); }

size_t dabgpu_pft_read_out_bytes(int n_bytes) {
    return n_bytes < 0 || n_bytes > PFT_READ_MAX_BYTES ? 0 : size_t(pf::read_out_bytes(uint32_t(n_bytes)));
}

int dabgpu_pft_read_max_records(int n_bytes) {
    return n_bytes < 0 || n_bytes > PFT_READ_MAX_BYTES ? 0 : int(pf::read_max_records(uint32_t(n_bytes)));
}

int dabgpu_pft_read_dev(dabgpu_ctx *ctx, const dabgpu_pft_read_entry *entries, int n_entries, void *stream) {
    if (!ctx || n_entries > dabk::PFT_READ_MAX_ENTRIES) return DABGPU_ERR_ARG;
    // everything is checked before anything is enqueued: a refused call leaves every output as it was
    std::vector<dabk::PftReadEntry> table(size_t(n_entries > 0 ? n_entries : 0), dabk::PftReadEntry{});
    const int bad = read_check(entries, n_entries, table.data());
    if (bad) return bad;
    if (n_entries == 0) return DABGPU_OK;
    size_t table_bytes = (table.size() * sizeof(dabk::PftReadEntry) + 15) / 16 * 16;
    for (const dabk::PftReadEntry &t : table) table_bytes += dabk::pft_read_scratch_bytes(t.n_bytes);
    return launch_entry_table(ctx, STAGE_PFT_READ, table_bytes, stream, [&](void *d_table, size_t, hipStream_t s) {
        return dabk::launch_pft_read(table.data(), n_entries, d_table, s);
    });
}

int dabgpu_pft_read_host(const dabgpu_pft_read_entry *entries, int n_entries) {
    const int bad = read_check(entries, n_entries, nullptr);
    if (bad) return bad;
    std::vector<uint8_t> s;
    std::vector<uint8_t> scratch(static_cast<size_t>(pf::MAX_BLOCK), uint8_t(0));
    for (int i = 0; i < n_entries; i++) {
        const dabgpu_pft_read_entry &e = entries[i];
        const uint8_t *state_in = static_cast<const uint8_t *>(e.d_state_in);
        pf::Head in{};
        if (state_in) std::memcpy(&in, state_in, sizeof in);
        const size_t tail = pf::clamp_tail(in.tail_bytes);
        s.resize(tail + size_t(e.n_bytes));
        if (tail) std::memcpy(s.data(), state_in + pf::STATE_TAIL_AT, tail);
        if (e.n_bytes) std::memcpy(s.data() + tail, e.d_bytes, size_t(e.n_bytes));
        pf::read_entry(GF, s.data(), s.size(), state_in, uint32_t(e.flags), e.d_out, reinterpret_cast<pf::Record *>(e.d_records),
                       pf::read_max_records(uint32_t(e.n_bytes)), reinterpret_cast<pf::Result *>(e.d_result), static_cast<uint8_t *>(e.d_state_out),
                       scratch.data());
    }
    return DABGPU_OK;
}

}  // extern "C"
