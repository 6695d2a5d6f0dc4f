// dabgpu_packet_groups_api.hip -- the C ABI of the data groups of any packet-mode component (include/dabgpu.h, "Data groups of
// ANY packet-mode service component"): the batch call on device memory, its twin on host memory (no context, no GPU: the
// serial walk of include/dabgpu_data_groups.h over the same functions the kernel calls), and which application a component's
// data is for (host, FIG 0/13 from FIBs).
#include "dabgpu_ctx.hpp"

#include <algorithm>
#include <cstring>

#include "../../include/dabgpu_data_groups.h"
#include "../../include/dabgpu_fig.h"

using namespace dabapi;
namespace dg = dabgpu_groups;
namespace pkt = dabgpu_packet;

static_assert(sizeof(dabgpu_data_group) == sizeof(dg::Record) && sizeof(dabgpu_packet_groups_result) == sizeof(dg::Counters) &&
                  sizeof(dabgpu_packet_groups_entry) == 88 && sizeof(dabgpu_user_application) == 56,
              "ABI structs mirror the header's");
static_assert(DABGPU_DG_EXTENSION == dg::DG_EXTENSION && DABGPU_DG_CRC == dg::DG_CRC && DABGPU_DG_SEGMENT == dg::DG_SEGMENT &&
                  DABGPU_DG_USER_ACCESS == dg::DG_USER_ACCESS && DABGPU_DG_TRANSPORT_ID == dg::DG_TRANSPORT_ID &&
                  DABGPU_DG_REPEAT == dg::DG_REPEAT && DABGPU_DG_BREAK == dg::DG_BREAK,
              "flags of a record");

size_t dabgpu_packet_groups_state_bytes(void) { return sizeof(dg::State); }
int dabgpu_packet_groups_chunk(void) { return dabk::PACKET_GROUPS_CHUNK; }

// everything both calls refuse, before anything is done; fills the kernels' tables when there are any
static int groups_check(const dabgpu_packet_groups_entry *entries, int n_entries, int n_cifs, dabk::PacketEntry *scan,
                        dabk::PacketGroupsEntry *table) {
    if (n_entries < 0 || n_cifs < 0 || n_cifs > pkt::MAX_N_CIFS || (n_entries > 0 && !entries)) return DABGPU_ERR_ARG;
    const uint64_t sb = sizeof(dg::State);
    for (int i = 0; i < n_entries; i++) {
        const dabgpu_packet_groups_entry &e = entries[i];
        if (!pkt::bitrate_ok(e.bitrate_kbps)) return DABGPU_ERR_ARG;
        if (e.in_stride < size_t(3) * size_t(e.bitrate_kbps)) return DABGPU_ERR_ARG;
        if (e.address < 1 || e.address > 1023) return DABGPU_ERR_ARG;
        if (n_cifs > 0 && !e.d_in) return DABGPU_ERR_ARG;
        if (e.mode != 0 && e.mode != 1) return DABGPU_ERR_ARG;
        if (!e.d_state_out || !e.d_result) return DABGPU_ERR_ARG;
        if ((addr(e.d_state_in) | addr(e.d_state_out) | addr(e.d_bytes)) & 15) return DABGPU_ERR_ARG;
        if ((addr(e.d_result) | addr(e.d_groups)) & 3) return DABGPU_ERR_ARG;
        if (e.d_state_in && overlaps(e.d_state_in, sb, e.d_state_out, sb)) return DABGPU_ERR_ARG;
        if (e.bytes_capacity < 0 || e.max_groups < 0) return DABGPU_ERR_ARG;
        if ((e.bytes_capacity > 0 && !e.d_bytes) || (e.max_groups > 0 && !e.d_groups)) return DABGPU_ERR_ARG;
    }
    for (int i = 0; i < n_entries; i++) {
        const dabgpu_packet_groups_entry &e = entries[i];
        if (uint64_t(n_cifs) * uint64_t(3 * e.bitrate_kbps) >= (uint64_t(1) << 31)) return DABGPU_ERR_CAPACITY;
        if (!scan) continue;
        dabk::PacketEntry &s = scan[i];
        s.in = addr(e.d_in);
        s.in_stride = e.in_stride;
        s.s = e.bitrate_kbps / 8;
        s.address = e.address;
        s.fec = e.fec != 0;
        dabk::PacketGroupsEntry &t = table[i];
        t.state_in = addr(e.d_state_in);
        t.state_out = addr(e.d_state_out);
        t.bytes = addr(e.d_bytes);
        t.groups = addr(e.d_groups);
        t.result = addr(e.d_result);
        t.bytes_capacity = e.bytes_capacity;
        t.max_groups = e.max_groups;
        t.mode = e.mode;
        t.keep_repeats = e.keep_repeats != 0;
    }
    return DABGPU_OK;
}

int dabgpu_packet_groups_dev(dabgpu_ctx *ctx, const dabgpu_packet_groups_entry *entries, int n_entries, int n_cifs, void *stream) {
    if (!ctx) return DABGPU_ERR_ARG;
    // everything is checked before anything is enqueued: a refused call leaves every output as it was
    const size_t n = size_t(n_entries > 0 ? n_entries : 0);
    std::vector<dabk::PacketEntry> scan(n, dabk::PacketEntry{});
    std::vector<dabk::PacketGroupsEntry> table(n, dabk::PacketGroupsEntry{});
    const int bad = groups_check(entries, n_entries, n_cifs, scan.data(), table.data());
    if (bad) return bad;
    if (n_entries == 0) return DABGPU_OK;
    if (dabk::packet_scan_blocks(scan.data(), n_entries, n_cifs) >= (uint64_t(1) << 31)) return DABGPU_ERR_CAPACITY;
    const size_t table_bytes = dabk::packet_groups_table_bytes(scan.data(), n_entries, n_cifs);
    return launch_entry_table(ctx, STAGE_PACKET_GROUPS, table_bytes, stream, [&](void *d_table, size_t slot_bytes, hipStream_t s) {
        return dabk::launch_packet_groups(scan.data(), table.data(), n_entries, n_cifs, d_table, slot_bytes, s);
    });
}

int dabgpu_packet_groups_host(const dabgpu_packet_groups_entry *entries, int n_entries, int n_cifs) {
    const int bad = groups_check(entries, n_entries, n_cifs, nullptr, nullptr);
    if (bad) return bad;
    for (int i = 0; i < n_entries; i++) {
        const dabgpu_packet_groups_entry &e = entries[i];
        dg::Call call{};
        call.mode = e.mode;
        call.keep_repeats = e.keep_repeats != 0;
        call.bytes_capacity = e.bytes_capacity;
        call.max_groups = e.max_groups;
        call.bytes = e.d_bytes;
        call.groups = reinterpret_cast<dg::Record *>(e.d_groups);
        dg::Counters c{};
        dg::walk_frames(static_cast<const dg::State *>(e.d_state_in), static_cast<dg::State *>(e.d_state_out), c, call, e.d_in,
                        e.in_stride, n_cifs, e.bitrate_kbps / 8, e.address, e.fec != 0);
        std::memcpy(e.d_result, &c, sizeof c);
    }
    return DABGPU_OK;
}

// ---- FIG 0/13 ----------------------------------------------------------------------------------------------------------
int dabgpu_fig_user_applications(const uint8_t *fib, const uint8_t *crc_ok, int n_frames, dabgpu_user_application *out, int max,
                                 int *n) {
    if (!fib || !crc_ok || !n || n_frames < 0 || max < 0 || (max > 0 && !out)) return DABGPU_ERR_ARG;
    return dabgpu_fig::user_applications(fib, crc_ok, n_frames, out, max, n);
}
