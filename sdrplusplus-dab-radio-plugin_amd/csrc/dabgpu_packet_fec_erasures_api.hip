// dabgpu_packet_fec_erasures_api.hip -- the C ABI of RS(204,188) correction of packet-mode FEC frames with failed packet CRCs
// as erasures (include/dabgpu.h, "... with failed packet CRCs as erasures"): the batch call on device memory and its twin on
// host memory (no context, no GPU: the same code, include/dabgpu_packet_fec_erasures.h).  The sibling of
// dabgpu_packet_fec_api.hip, which is as it was: the same refusals, a stage slot of its own.
#include "dabgpu_ctx.hpp"

#include <cstring>

#include "../../include/dabgpu_packet_fec_erasures.h"

using namespace dabapi;
namespace fec = dabgpu_packet_fec;

static_assert(sizeof(dabgpu_packet_fec_erasure_result) == sizeof(fec::ErasureCounters) && sizeof(dabgpu_packet_fec_erasure_entry) == 64 &&
                  sizeof(dabgpu_packet_fec_erasure_entry) == sizeof(dabgpu_packet_fec_entry),
              "ABI structs mirror the header's");

// everything both calls refuse, before anything is done; fills the kernels' table when there is one
static int packet_fec_erasures_check(const dabgpu_packet_fec_erasure_entry *entries, int n_entries, int n_cifs, dabk::PacketFecErasureEntry *table) {
    if (n_entries < 0 || n_cifs < 0 || n_cifs > fec::MAX_N_CIFS || (n_entries > 0 && !entries)) return DABGPU_ERR_ARG;
    auto addr = [](const void *p) { return uint64_t(reinterpret_cast<uintptr_t>(p)); };
    for (int i = 0; i < n_entries; i++) {
        const dabgpu_packet_fec_erasure_entry &e = entries[i];
        if (!fec::bitrate_ok(e.bitrate_kbps)) return DABGPU_ERR_ARG;
        const uint64_t fb = uint64_t(3) * uint64_t(e.bitrate_kbps), sb = uint64_t(fec::state_bytes(e.bitrate_kbps / 8));
        if (e.in_stride < fb || e.out_stride < fb) return DABGPU_ERR_ARG;
        if (n_cifs > 0 && (!e.d_in || !e.d_out)) return DABGPU_ERR_ARG;
        if (!e.d_state_out || !e.d_result) return DABGPU_ERR_ARG;
        if ((addr(e.d_state_in) | addr(e.d_state_out)) & 15) return DABGPU_ERR_ARG;
        if (addr(e.d_result) & 3) return DABGPU_ERR_ARG;
        if (e.d_state_in && addr(e.d_state_in) < addr(e.d_state_out) + sb && addr(e.d_state_out) < addr(e.d_state_in) + sb) return DABGPU_ERR_ARG;
        if (n_cifs > 0) {
            const uint64_t in_span = uint64_t(n_cifs - 1) * e.in_stride + fb, out_span = uint64_t(n_cifs - 1) * e.out_stride + fb;
            if (addr(e.d_in) < addr(e.d_out) + out_span && addr(e.d_out) < addr(e.d_in) + in_span) return DABGPU_ERR_ARG;
        }
        if (!table) continue;
        dabk::PacketFecErasureEntry &t = table[i];
        t.in = addr(e.d_in);
        t.in_stride = e.in_stride;
        t.out = addr(e.d_out);
        t.out_stride = e.out_stride;
        t.state_in = addr(e.d_state_in);
        t.state_out = addr(e.d_state_out);
        t.result = addr(e.d_result);
        t.s = e.bitrate_kbps / 8;
    }
    return DABGPU_OK;
}

int dabgpu_packet_fec_erasures_dev(dabgpu_ctx *ctx, const dabgpu_packet_fec_erasure_entry *entries, int n_entries, int n_cifs, void *stream) {
    if (!ctx) return DABGPU_ERR_ARG;
    // everything is checked before anything is enqueued: a refused call leaves every output as it was
    std::vector<dabk::PacketFecErasureEntry> table(size_t(n_entries > 0 ? n_entries : 0), dabk::PacketFecErasureEntry{});
    const int bad = packet_fec_erasures_check(entries, n_entries, n_cifs, table.data());
    if (bad) return bad;
    if (n_entries == 0) return DABGPU_OK;
    if (dabk::packet_fec_erasure_blocks(table.data(), n_entries, n_cifs) >= (uint64_t(1) << 31)) return DABGPU_ERR_CAPACITY;
    DeviceGuard guard(ctx);
    hipStream_t s = pick_stream(ctx, stream);
    const size_t table_bytes = dabk::packet_fec_erasure_table_bytes(table.data(), n_entries, n_cifs);
    // (growing the table must not race with a launch that still reads the old one)
    if (ctx->stage_bytes[STAGE_PACKET_FEC_ERASURES] < table_bytes) HIP_TRY(hipStreamSynchronize(s));
    void *d_table = nullptr;
    const int rc = stage(ctx, STAGE_PACKET_FEC_ERASURES, table_bytes, &d_table);
    if (rc) return rc;
    HIP_TRY(dabk::launch_packet_fec_erasures(table.data(), n_entries, n_cifs, d_table, ctx->stage_bytes[STAGE_PACKET_FEC_ERASURES], s));
    return DABGPU_OK;
}

int dabgpu_packet_fec_erasures_host(const dabgpu_packet_fec_erasure_entry *entries, int n_entries, int n_cifs) {
    const int bad = packet_fec_erasures_check(entries, n_entries, n_cifs, nullptr);
    if (bad) return bad;
    static const fec::Gf gf = fec::make_gf();
    for (int i = 0; i < n_entries; i++) {
        const dabgpu_packet_fec_erasure_entry &e = entries[i];
        fec::ErasureCounters c;
        fec::process_erasures(gf, static_cast<const uint8_t *>(e.d_state_in), static_cast<uint8_t *>(e.d_state_out), c, e.d_in, e.in_stride, n_cifs,
                              e.bitrate_kbps / 8, e.d_out, e.out_stride);
        std::memcpy(e.d_result, &c, sizeof c);
    }
    return DABGPU_OK;
}
