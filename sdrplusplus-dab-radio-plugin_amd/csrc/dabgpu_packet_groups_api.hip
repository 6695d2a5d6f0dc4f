// dabgpu_packet_groups_api.hip -- the C ABI of the data groups of any packet-mode component (include/dabgpu.h, "Data groups of
// ANY packet-mode service component"): the batch call on device memory, its twin on host memory (no context, no GPU: the
// serial walk of include/dabgpu_data_groups.h over the same functions the kernel calls), and which application a component's
// data is for (host, FIG 0/13 from FIBs).
#include "dabgpu_ctx.hpp"

#include <algorithm>
#include <cstring>

#include "../../include/dabgpu_data_groups.h"

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
    auto addr = [](const void *p) { return uint64_t(reinterpret_cast<uintptr_t>(p)); };
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
        if (e.d_state_in && addr(e.d_state_in) < addr(e.d_state_out) + sb && addr(e.d_state_out) < addr(e.d_state_in) + sb)
            return DABGPU_ERR_ARG;
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
    DeviceGuard guard(ctx);
    hipStream_t s = pick_stream(ctx, stream);
    const size_t table_bytes = dabk::packet_groups_table_bytes(scan.data(), n_entries, n_cifs);
    // (growing the table must not race with a launch that still reads the old one)
    if (ctx->stage_bytes[STAGE_PACKET_GROUPS] < table_bytes) HIP_TRY(hipStreamSynchronize(s));
    void *d_table = nullptr;
    const int rc = stage(ctx, STAGE_PACKET_GROUPS, table_bytes, &d_table);
    if (rc) return rc;
    HIP_TRY(dabk::launch_packet_groups(scan.data(), table.data(), n_entries, n_cifs, d_table, ctx->stage_bytes[STAGE_PACKET_GROUPS], s));
    return DABGPU_OK;
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
    // pass 0: FIG 0/8 (SId, SCIdS) -> SubChId or SCId, FIG 0/3 SCId -> (SubChId, packet address); pass 1: FIG 0/13.  Each list
    // keeps its first MAX_FOUND entries, as dabgpu_fig_packet_components does: far more than 12 FIBs a frame announce
    struct Global {
        uint32_t sid;
        int scids, ls, id;
    };
    struct Described {
        int scid, subchid, address;
    };
    constexpr int MAX_FOUND = 256;
    std::vector<Global> globals;
    std::vector<Described> described;
    std::vector<dabgpu_user_application> found;
    for (int pass = 0; pass < 2; pass++) {
        for (int k = 0; k < n_frames * dab::NB_FIBS; k++) {
            if (!crc_ok[k]) continue;
            const uint8_t *d = fib + size_t(k) * 32;
            for (int i = 0; i < 30;) {
                if (d[i] == 0xFF) break;
                const int type = d[i] >> 5, len = d[i] & 0x1F;
                if (len == 0 || i + 1 + len > 30) break;
                const uint8_t *b = d + i + 1;
                i += 1 + len;
                // type 0, current configuration (C/N = 0), this ensemble (OE = 0)
                if (type != 0 || (b[0] & 0xC0)) continue;
                const int ext = b[0] & 0x1F, pd = (b[0] >> 5) & 1, sid_bytes = pd ? 4 : 2;
                auto sid_at = [&](int j) {
                    uint32_t sid = 0;
                    for (int q = 0; q < sid_bytes; q++) sid = (sid << 8) | b[j + q];
                    return sid;
                };
                if (pass == 0 && ext == 3) {
                    for (int j = 1; j + 5 <= len;) {
                        const int scid = (b[j] << 4) | (b[j + 1] >> 4), caorg = b[j + 1] & 1;
                        const Described q = {scid, b[j + 3] >> 2, ((b[j + 3] & 3) << 8) | b[j + 4]};
                        j += 5 + 2 * caorg;
                        if (j > len) break;
                        bool known = false;
                        for (const Described &o : described) known = known || o.scid == scid;
                        if (!known && described.size() < size_t(MAX_FOUND)) described.push_back(q);
                    }
                } else if (pass == 0 && ext == 8) {
                    for (int j = 1; j + sid_bytes + 2 <= len;) {
                        const uint32_t sid = sid_at(j);
                        const int extended = b[j + sid_bytes] >> 7, scids = b[j + sid_bytes] & 0x0F, ls = b[j + sid_bytes + 1] >> 7;
                        j += sid_bytes + 1;
                        if (j + (ls ? 2 : 1) + extended > len) break;
                        const int id = ls ? ((b[j] & 0x0F) << 8) | b[j + 1] : b[j] & 0x3F;
                        const bool fidc = !ls && (b[j] & 0x40);        // short form, MSC/FIC flag 1: a FIDC, not a sub-channel
                        j += (ls ? 2 : 1) + extended;
                        if (fidc) continue;
                        bool known = false;
                        for (const Global &g : globals) known = known || (g.sid == sid && g.scids == scids);
                        if (!known && globals.size() < size_t(MAX_FOUND)) globals.push_back(Global{sid, scids, ls, id});
                    }
                } else if (pass == 1 && ext == 13) {
                    for (int j = 1; j + sid_bytes + 1 <= len;) {
                        const uint32_t sid = sid_at(j);
                        const int scids = b[j + sid_bytes] >> 4, count = b[j + sid_bytes] & 0x0F;
                        j += sid_bytes + 1;
                        bool cut = false;
                        for (int a = 0; a < count && !cut; a++) {
                            if (j + 2 > len) {
                                cut = true;
                                break;
                            }
                            const int ua_type = (b[j] << 3) | (b[j + 1] >> 5), data_length = b[j + 1] & 0x1F;
                            if (j + 2 + data_length > len) {
                                cut = true;
                                break;
                            }
                            bool seen = false;
                            for (const dabgpu_user_application &f : found)
                                seen = seen || (f.sid == sid && f.scids == scids && f.ua_type == ua_type);
                            if (!seen && found.size() < size_t(MAX_FOUND)) {
                                dabgpu_user_application u{};
                                u.sid = sid;
                                u.scids = scids;
                                u.ua_type = ua_type;
                                u.subchid = u.scid = u.packet_address = -1;
                                u.data_length = data_length > 23 ? 23 : data_length;
                                for (int q = 0; q < u.data_length; q++) u.data[q] = b[j + 2 + q];
                                for (const Global &g : globals) {
                                    if (g.sid != sid || g.scids != scids) continue;
                                    if (!g.ls) {
                                        u.subchid = g.id;
                                    } else {
                                        u.tmid_packet = 1;
                                        u.scid = g.id;
                                        for (const Described &o : described)
                                            if (o.scid == g.id) {
                                                u.subchid = o.subchid;
                                                u.packet_address = o.address;
                                                break;
                                            }
                                    }
                                    break;
                                }
                                found.push_back(u);
                            }
                            j += 2 + data_length;
                        }
                        if (cut) break;
                    }
                }
            }
        }
    }
    std::stable_sort(found.begin(), found.end(), [](const dabgpu_user_application &a, const dabgpu_user_application &b) {
        if (a.sid != b.sid) return a.sid < b.sid;
        if (a.scids != b.scids) return a.scids < b.scids;
        return a.ua_type < b.ua_type;
    });
    const int count = int(found.size());
    *n = count;
    if (count > max) return DABGPU_ERR_CAPACITY;
    for (int i = 0; i < count; i++) out[i] = found[i];
    return DABGPU_OK;
}
