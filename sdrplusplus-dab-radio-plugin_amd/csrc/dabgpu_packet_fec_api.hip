// dabgpu_packet_fec_api.hip -- the C ABI of RS(204,188) correction of packet-mode FEC frames (include/dabgpu.h, "FEC frames
// of packet-mode sub-channels" and "... with failed packet CRCs as erasures"): for each of the two, the batch call on device
// memory and its twin on host memory (no context, no GPU: the same code, include/dabgpu_packet_fec.h and
// include/dabgpu_packet_fec_erasures.h).  One implementation over the entry type; each call has a stage slot of its own.
#include "dabgpu_ctx.hpp"

#include <cstddef>
#include <cstring>
#include <type_traits>

#include "../../include/dabgpu_packet_fec_erasures.h"

using namespace dabapi;
namespace fec = dabgpu_packet_fec;

// the two entry structs are one layout: what serves one serves the other
#define SAME_FIELD(f)                                                                                         \
    static_assert(offsetof(dabgpu_packet_fec_entry, f) == offsetof(dabgpu_packet_fec_erasure_entry, f) &&    \
                      sizeof(dabgpu_packet_fec_entry::f) == sizeof(dabgpu_packet_fec_erasure_entry::f),       \
                  "ABI entry structs are equal field for field")
SAME_FIELD(d_in);
SAME_FIELD(in_stride);
SAME_FIELD(bitrate_kbps);
SAME_FIELD(reserved);
SAME_FIELD(d_out);
SAME_FIELD(out_stride);
SAME_FIELD(d_state_in);
SAME_FIELD(d_state_out);
SAME_FIELD(d_result);
#undef SAME_FIELD
static_assert(sizeof(dabgpu_packet_fec_result) == sizeof(fec::Counters) && sizeof(dabgpu_packet_fec_erasure_result) == sizeof(fec::ErasureCounters) &&
                  sizeof(dabgpu_packet_fec_entry) == 64 && sizeof(dabgpu_packet_fec_erasure_entry) == 64,
              "ABI structs mirror the header's");

size_t dabgpu_packet_fec_state_bytes(int bitrate_kbps) { return fec::bitrate_ok(bitrate_kbps) ? size_t(fec::state_bytes(bitrate_kbps / 8)) : 0; }
int dabgpu_packet_fec_delay(int bitrate_kbps) { return fec::bitrate_ok(bitrate_kbps) ? fec::delay(bitrate_kbps / 8) : -1; }

// everything the calls refuse, before anything is done; fills the kernels' table when there is one
template <class Entry> static int packet_fec_check(const Entry *entries, int n_entries, int n_cifs, dabk::PacketFecEntry *table) {
    if (n_entries < 0 || n_cifs < 0 || n_cifs > fec::MAX_N_CIFS || (n_entries > 0 && !entries)) return DABGPU_ERR_ARG;
    for (int i = 0; i < n_entries; i++) {
        const Entry &e = entries[i];
        if (!fec::bitrate_ok(e.bitrate_kbps)) return DABGPU_ERR_ARG;
        const uint64_t fb = uint64_t(3) * uint64_t(e.bitrate_kbps), sb = uint64_t(fec::state_bytes(e.bitrate_kbps / 8));
        if (e.in_stride < fb || e.out_stride < fb) return DABGPU_ERR_ARG;
        if (n_cifs > 0 && (!e.d_in || !e.d_out)) return DABGPU_ERR_ARG;
        if (!e.d_state_out || !e.d_result) return DABGPU_ERR_ARG;
        if ((addr(e.d_state_in) | addr(e.d_state_out)) & 15) return DABGPU_ERR_ARG;
        if (addr(e.d_result) & 3) return DABGPU_ERR_ARG;
        if (e.d_state_in && overlaps(e.d_state_in, sb, e.d_state_out, sb)) return DABGPU_ERR_ARG;
        if (n_cifs > 0) {
            const uint64_t in_span = uint64_t(n_cifs - 1) * e.in_stride + fb, out_span = uint64_t(n_cifs - 1) * e.out_stride + fb;
            if (overlaps(e.d_in, in_span, e.d_out, out_span)) return DABGPU_ERR_ARG;
        }
        if (!table) continue;
        dabk::PacketFecEntry &t = table[i];
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

template <class Entry> static int packet_fec_dev(dabgpu_ctx *ctx, const Entry *entries, int n_entries, int n_cifs, void *stream) {
    constexpr bool erasures = std::is_same_v<Entry, dabgpu_packet_fec_erasure_entry>;
    constexpr StageSlot slot = erasures ? STAGE_PACKET_FEC_ERASURES : STAGE_PACKET_FEC;
    if (!ctx) return DABGPU_ERR_ARG;
    // everything is checked before anything is enqueued: a refused call leaves every output as it was
    std::vector<dabk::PacketFecEntry> table(size_t(n_entries > 0 ? n_entries : 0), dabk::PacketFecEntry{});
    const int bad = packet_fec_check(entries, n_entries, n_cifs, table.data());
    if (bad) return bad;
    if (n_entries == 0) return DABGPU_OK;
    if (dabk::packet_fec_blocks(table.data(), n_entries, n_cifs) >= (uint64_t(1) << 31)) return DABGPU_ERR_CAPACITY;
    const size_t table_bytes = dabk::packet_fec_table_bytes(table.data(), n_entries, n_cifs, erasures);
    return launch_entry_table(ctx, slot, table_bytes, stream, [&](void *d_table, size_t slot_bytes, hipStream_t s) {
        return dabk::launch_packet_fec(table.data(), n_entries, n_cifs, erasures, d_table, slot_bytes, s);
    });
}

template <class Entry> static int packet_fec_host(const Entry *entries, int n_entries, int n_cifs) {
    const int bad = packet_fec_check(entries, n_entries, n_cifs, nullptr);
    if (bad) return bad;
    static const fec::Gf gf = fec::make_gf();
    for (int i = 0; i < n_entries; i++) {
        const Entry &e = entries[i];
        const uint8_t *state_in = static_cast<const uint8_t *>(e.d_state_in);
        uint8_t *state_out = static_cast<uint8_t *>(e.d_state_out);
        const int S = e.bitrate_kbps / 8;
        if constexpr (std::is_same_v<Entry, dabgpu_packet_fec_erasure_entry>) {
            fec::ErasureCounters c;
            fec::process_erasures(gf, state_in, state_out, c, e.d_in, e.in_stride, n_cifs, S, e.d_out, e.out_stride);
            std::memcpy(e.d_result, &c, sizeof c);
        } else {
            fec::Counters c;
            fec::process(gf, state_in, state_out, c, e.d_in, e.in_stride, n_cifs, S, e.d_out, e.out_stride);
            std::memcpy(e.d_result, &c, sizeof c);
        }
    }
    return DABGPU_OK;
}

int dabgpu_packet_fec_dev(dabgpu_ctx *ctx, const dabgpu_packet_fec_entry *entries, int n_entries, int n_cifs, void *stream) {
    return packet_fec_dev(ctx, entries, n_entries, n_cifs, stream);
}
int dabgpu_packet_fec_host(const dabgpu_packet_fec_entry *entries, int n_entries, int n_cifs) { return packet_fec_host(entries, n_entries, n_cifs); }
int dabgpu_packet_fec_erasures_dev(dabgpu_ctx *ctx, const dabgpu_packet_fec_erasure_entry *entries, int n_entries, int n_cifs, void *stream) {
    return packet_fec_dev(ctx, entries, n_entries, n_cifs, stream);
}
int dabgpu_packet_fec_erasures_host(const dabgpu_packet_fec_erasure_entry *entries, int n_entries, int n_cifs) {
    return packet_fec_host(entries, n_entries, n_cifs);
}
