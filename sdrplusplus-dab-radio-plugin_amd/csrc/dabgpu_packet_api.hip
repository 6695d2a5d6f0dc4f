// dabgpu_packet_api.hip -- the C ABI of packet-mode MOT services (include/dabgpu.h, "Packet-mode MOT services"): which
// components are packet mode (host, from FIBs), the batch call on device memory and its twin on host memory (no context, no
// GPU: the same code, include/dabgpu_packet_walk.h, its orders executed by a loop).
#include "dabgpu_ctx.hpp"

#include <algorithm>
#include <cstring>

#include "../../include/dabgpu_packet_walk.h"

using namespace dabapi;
namespace mot = dabgpu_mot;
namespace pkt = dabgpu_packet;

static_assert(sizeof(dabgpu_packet_result) == sizeof(pkt::Counters) && sizeof(dabgpu_packet_component) == 48,
              "ABI structs mirror the walk's");

size_t dabgpu_packet_state_bytes(void) { return sizeof(pkt::State); }

int dabgpu_fig_packet_components(const uint8_t *fib, const uint8_t *crc_ok, int n_frames, dabgpu_packet_component *out, int max,
                                 int *n) {
    if (!fib || !crc_ok || !n || n_frames < 0 || max < 0 || (max > 0 && !out)) return DABGPU_ERR_ARG;
    // pass 0: FIG 0/1 SubChId -> start address (as dabgpu_fig_audio_components), FIG 0/3 SCId -> the packet-mode description,
    // FIG 0/14 SubChId -> FEC scheme; pass 1: FIG 0/2 (clause 6.3.1), the components with TMId = 3: SCId (12), P/S (1), CA (1)
    struct Described {
        int scid, subchid, address, dscty, dg;
    };
    constexpr int MAX_FOUND = 256;
    int start_of[64], fec_of[64];
    for (int i = 0; i < 64; i++) start_of[i] = -1, fec_of[i] = 0;
    bool fec_seen[64] = {};
    Described described[MAX_FOUND];
    int n_described = 0;
    dabgpu_packet_component found[MAX_FOUND];
    int count = 0;
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
                const int ext = b[0] & 0x1F, pd = (b[0] >> 5) & 1;
                if (pass == 0 && ext == 1) {
                    for (int j = 1; j + 3 <= len;) {
                        const int id = b[j] >> 2, start = ((b[j] & 3) << 8) | b[j + 1];
                        if (b[j + 2] & 0x80) {
                            if (j + 4 > len) break;
                            const int option = (b[j + 2] >> 4) & 7;
                            j += 4;
                            if (option > 1) continue;          // (passed over by dabgpu_fig_subchannels as well)
                        } else {
                            j += 3;
                        }
                        if (start_of[id] < 0) start_of[id] = start;
                    }
                } else if (pass == 0 && ext == 3) {
                    for (int j = 1; j + 5 <= len;) {
                        const int scid = (b[j] << 4) | (b[j + 1] >> 4), caorg = b[j + 1] & 1;
                        Described q = {scid, b[j + 3] >> 2, ((b[j + 3] & 3) << 8) | b[j + 4], b[j + 2] & 0x3F, b[j + 2] >> 7};
                        j += 5 + 2 * caorg;
                        if (j > len) break;                    // (the CAOrg field is cut off)
                        bool known = false;
                        for (int q0 = 0; q0 < n_described; q0++) known = known || described[q0].scid == scid;
                        if (!known && n_described < MAX_FOUND) described[n_described++] = q;
                    }
                } else if (pass == 0 && ext == 14) {
                    for (int j = 1; j < len; j++) {
                        const int id = b[j] >> 2;
                        if (!fec_seen[id]) fec_of[id] = b[j] & 3;
                        fec_seen[id] = true;
                    }
                } else if (pass == 1 && ext == 2) {
                    const int sid_bytes = pd ? 4 : 2;
                    for (int j = 1; j + sid_bytes + 1 <= len;) {
                        uint32_t sid = 0;
                        for (int q = 0; q < sid_bytes; q++) sid = (sid << 8) | b[j + q];
                        const int ncomp = b[j + sid_bytes] & 0x0F;
                        j += sid_bytes + 1;
                        if (j + 2 * ncomp > len) break;
                        for (int c = 0; c < ncomp; c++, j += 2) {
                            if ((b[j] >> 6) != 3) continue;
                            const int scid = ((b[j] & 0x3F) << 6) | (b[j + 1] >> 2);
                            const Described *q = nullptr;
                            for (int q0 = 0; q0 < n_described && !q; q0++)
                                if (described[q0].scid == scid) q = &described[q0];
                            if (!q || start_of[q->subchid] < 0) continue;
                            bool seen = false;
                            for (int f = 0; f < count; f++)
                                seen = seen || (found[f].subchid == q->subchid && found[f].packet_address == q->address);
                            if (seen || count >= MAX_FOUND) continue;
                            dabgpu_packet_component a{};
                            a.sid = sid;
                            a.scid = scid;
                            a.subchid = q->subchid;
                            a.start_address = start_of[q->subchid];
                            a.packet_address = q->address;
                            a.dscty = q->dscty;
                            a.dg_flag = q->dg;
                            a.fec_scheme = fec_of[q->subchid];
                            a.primary = (b[j + 1] >> 1) & 1;
                            found[count++] = a;
                        }
                    }
                }
            }
        }
    }
    std::stable_sort(found, found + count, [](const dabgpu_packet_component &a, const dabgpu_packet_component &b) {
        return a.start_address != b.start_address ? a.start_address < b.start_address : a.packet_address < b.packet_address;
    });
    *n = count;
    if (count > max) return DABGPU_ERR_CAPACITY;
    for (int i = 0; i < count; i++) out[i] = found[i];
    return DABGPU_OK;
}

// everything both calls refuse, before anything is done; fills the kernels' table when there is one
static int packet_check(const dabgpu_packet_entry *entries, int n_entries, int n_cifs, dabk::PacketEntry *table) {
    if (n_entries < 0 || n_cifs < 0 || n_cifs > pkt::MAX_N_CIFS || (n_entries > 0 && !entries)) return DABGPU_ERR_ARG;
    auto addr = [](const void *p) { return uint64_t(reinterpret_cast<uintptr_t>(p)); };
    const uint64_t sb = sizeof(pkt::State);
    for (int i = 0; i < n_entries; i++) {
        const dabgpu_packet_entry &e = entries[i];
        if (!pkt::bitrate_ok(e.bitrate_kbps)) return DABGPU_ERR_ARG;
        if (e.in_stride < size_t(3) * size_t(e.bitrate_kbps)) return DABGPU_ERR_ARG;
        if (e.address < 1 || e.address > 1023) return DABGPU_ERR_ARG;
        if (n_cifs > 0 && !e.d_in) return DABGPU_ERR_ARG;
        if (!e.d_state_out || !e.d_arena || !e.d_result) return DABGPU_ERR_ARG;
        if ((addr(e.d_state_in) | addr(e.d_state_out) | addr(e.d_arena) | addr(e.d_slides)) & 15) return DABGPU_ERR_ARG;
        if (addr(e.d_result) & 3) return DABGPU_ERR_ARG;
        if (e.d_state_in && addr(e.d_state_in) < addr(e.d_state_out) + sb && addr(e.d_state_out) < addr(e.d_state_in) + sb)
            return DABGPU_ERR_ARG;
        if (e.arena_bytes < mot::arena_bytes(0) || e.max_slides < 0) return DABGPU_ERR_ARG;
        if (e.max_slides > 0 && (!e.d_slides || e.slide_stride < size_t(mot::RECORD_BYTES) || e.slide_stride % 16 ||
                                 e.slide_stride >= (uint64_t(1) << 31) || uint64_t(e.max_slides) * e.slide_stride >= (uint64_t(1) << 31)))
            return DABGPU_ERR_ARG;
        if (!table) continue;
        dabk::PacketEntry &t = table[i];
        t.in = addr(e.d_in);
        t.in_stride = e.in_stride;
        t.state_in = addr(e.d_state_in);
        t.state_out = addr(e.d_state_out);
        t.arena = addr(e.d_arena);
        t.slides = addr(e.d_slides);
        t.result = addr(e.d_result);
        t.slide_stride = e.max_slides > 0 ? uint32_t(e.slide_stride) : 0;
        t.max_slides = e.max_slides;
        t.body_capacity = mot::body_capacity_of(e.arena_bytes);
        t.s = e.bitrate_kbps / 8;
        t.address = e.address;
        t.fec = e.fec != 0;
    }
    return DABGPU_OK;
}

int dabgpu_packet_slides_dev(dabgpu_ctx *ctx, const dabgpu_packet_entry *entries, int n_entries, int n_cifs, void *stream) {
    if (!ctx) return DABGPU_ERR_ARG;
    // everything is checked before anything is enqueued: a refused call leaves every output as it was
    std::vector<dabk::PacketEntry> table(size_t(n_entries > 0 ? n_entries : 0), dabk::PacketEntry{});
    const int bad = packet_check(entries, n_entries, n_cifs, table.data());
    if (bad) return bad;
    if (n_entries == 0) return DABGPU_OK;
    if (dabk::packet_scan_blocks(table.data(), n_entries, n_cifs) >= (uint64_t(1) << 31)) return DABGPU_ERR_CAPACITY;
    DeviceGuard guard(ctx);
    hipStream_t s = pick_stream(ctx, stream);
    const size_t table_bytes = dabk::packet_table_bytes(table.data(), n_entries, n_cifs);
    // (growing the table must not race with a launch that still reads the old one)
    if (ctx->stage_bytes[STAGE_PACKET] < table_bytes) HIP_TRY(hipStreamSynchronize(s));
    void *d_table = nullptr;
    const int rc = stage(ctx, STAGE_PACKET, table_bytes, &d_table);
    if (rc) return rc;
    HIP_TRY(dabk::launch_packet_slides(table.data(), n_entries, n_cifs, d_table, ctx->stage_bytes[STAGE_PACKET], s));
    return DABGPU_OK;
}

int dabgpu_packet_slides_host(const dabgpu_packet_entry *entries, int n_entries, int n_cifs) {
    const int bad = packet_check(entries, n_entries, n_cifs, nullptr);
    if (bad) return bad;
    for (int i = 0; i < n_entries; i++) {
        const dabgpu_packet_entry &e = entries[i];
        mot::Call call{};
        call.body_capacity = mot::body_capacity_of(e.arena_bytes);
        call.max_slides = e.max_slides;
        call.slide_stride = e.max_slides > 0 ? uint32_t(e.slide_stride) : 0;
        pkt::State st;
        if (e.d_state_in) std::memcpy(&st, e.d_state_in, sizeof st);
        else std::memset(&st, 0, sizeof st);
        pkt::sanitize(st, call.body_capacity);
        pkt::Counters c{};
        pkt::walk_frames(st, c, call, e.d_in, e.in_stride, n_cifs, e.bitrate_kbps / 8, e.address, e.fec != 0,
                         static_cast<uint8_t *>(e.d_arena), e.d_slides);
        std::memcpy(e.d_state_out, &st, sizeof st);
        std::memcpy(e.d_result, &c, sizeof c);
    }
    return DABGPU_OK;
}
