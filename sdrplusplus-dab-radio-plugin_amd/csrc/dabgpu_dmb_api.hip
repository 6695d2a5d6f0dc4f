// dabgpu_dmb_api.hip -- the C ABI of T-DMB stream-mode sub-channels (include/dabgpu.h, "T-DMB"): the batch call on device
// memory and its twin on host memory (no context, no GPU: the serial code of include/dabgpu_dmb.h).
#include "dabgpu_ctx.hpp"

#include <algorithm>
#include <cstddef>
#include <cstring>

#include "../../include/dabgpu_dmb.h"
#include "../../include/dabgpu_fig.h"

using namespace dabapi;
namespace dmb = dabgpu_dmb;

static_assert(sizeof(dabgpu_dmb_record) == sizeof(dmb::Record) && sizeof(dabgpu_dmb_result) == sizeof(dmb::Result) &&
                  sizeof(dabgpu_dmb_census_entry) == sizeof(dmb::CensusEntry) && sizeof(dabgpu_dmb_entry) == 64 && sizeof(dabgpu_stream_component) == 32 &&
                  DABGPU_DSCTY_MPEG2_TS == 24,
              "ABI structs mirror the header's");
static_assert(offsetof(dabgpu_dmb_record, pid) == offsetof(dmb::Record, pid) && offsetof(dabgpu_dmb_record, position) == offsetof(dmb::Record, position) &&
                  offsetof(dabgpu_dmb_result, packets_dropped) == offsetof(dmb::Result, packets_dropped) &&
                  offsetof(dabgpu_dmb_result, pids_overflowed) == offsetof(dmb::Result, pids_overflowed) &&
                  offsetof(dabgpu_dmb_census_entry, scrambled) == offsetof(dmb::CensusEntry, scrambled),
              "... field for field");
static_assert(DABGPU_DMB_AS_RECEIVED == dmb::AS_RECEIVED && DABGPU_DMB_CORRECTED == dmb::CORRECTED && DABGPU_DMB_UNCORRECTABLE == dmb::UNCORRECTABLE &&
                  DABGPU_DMB_EXEMPT == dmb::FLAG_EXEMPT && DABGPU_DMB_TS_BYTES == dmb::TS_BYTES && DABGPU_DMB_CENSUS == dmb::CENSUS && DABGPU_DMB_DEFER_ROOM == dmb::DEFER_ROOM &&
                  offsetof(dabgpu_dmb_result, packets_lost) == offsetof(dmb::Result, packets_lost),
              "the header's values are the ABI's");

namespace {

// everything both calls refuse, before anything is done; fills the kernels' table when there is one
int dmb_check(const dabgpu_dmb_entry *entries, int n_entries, int n_cifs, dabk::DmbEntry *table) {
    if (n_entries < 0 || n_cifs < 0 || n_cifs > dmb::MAX_N_CIFS || (n_entries > 0 && !entries)) return DABGPU_ERR_ARG;
    for (int i = 0; i < n_entries; i++) {
        const dabgpu_dmb_entry &e = entries[i];
        if (!dmb::bitrate_ok(e.bitrate_kbps)) return DABGPU_ERR_ARG;
        if (e.in_stride < uint64_t(dmb::frame_bytes(e.bitrate_kbps)) || (n_cifs > 0 && !e.d_in)) return DABGPU_ERR_ARG;
        if (e.max_packets < 0 || (e.max_packets > 0 && (!e.d_ts || !e.d_records))) return DABGPU_ERR_ARG;
        if (!e.d_state_out || !e.d_result) return DABGPU_ERR_ARG;
        if ((addr(e.d_ts) | addr(e.d_records) | addr(e.d_state_in) | addr(e.d_state_out)) & 15) return DABGPU_ERR_ARG;
        if (addr(e.d_result) & 3) return DABGPU_ERR_ARG;
        const uint64_t sb = dmb::STATE_BYTES;
        if (e.d_state_in && overlaps(e.d_state_in, sb, e.d_state_out, sb)) return DABGPU_ERR_ARG;
        if (!table) continue;
        dabk::DmbEntry &t = table[i];
        t.in = addr(e.d_in);
        t.in_stride = e.in_stride;
        t.ts = addr(e.d_ts);
        t.records = addr(e.d_records);
        t.state_in = addr(e.d_state_in);
        t.state_out = addr(e.d_state_out);
        t.result = addr(e.d_result);
        t.kbps = e.bitrate_kbps;
        t.max_packets = dmb::new_packets(e.bitrate_kbps, n_cifs);
        t.capacity = e.max_packets;
    }
    return DABGPU_OK;
}

// ---- PSI sections out of TS packets (dabgpu_ts_programs)

// CRC-32/MPEG-2: x^32 + x^26 + x^23 + x^22 + x^16 + x^12 + x^11 + x^10 + x^8 + x^7 + x^5 + x^4 + x^2 + x + 1, register all
// ones, no reflection, no final inversion; over a section with its CRC_32 the register ends at 0
uint32_t crc32_mpeg2(const uint8_t *p, size_t n) {
    uint32_t crc = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) {
        crc ^= uint32_t(p[i]) << 24;
        for (int b = 0; b < 8; b++) crc = (crc & 0x80000000u) ? (crc << 1) ^ 0x04C11DB7u : crc << 1;
    }
    return crc;
}

// the sections of one PID, assembled packet by packet; done(section, bytes) for every complete one
template <class Done> void sections_of(const uint8_t *ts, int n_packets, int pid, Done done) {
    uint8_t sec[4096 + 3];
    int have = -1, last_cc = -1;                                    // have < 0: not inside a section
    auto add = [&](const uint8_t *p, int n) {                       // bytes of the section being assembled
        for (int i = 0; i < n && have >= 0; i++) {
            sec[have++] = p[i];
            if (have >= 3 && have == 3 + (((sec[1] & 0x0F) << 8) | sec[2])) {
                done(sec, have);
                have = -1;
                return i + 1;
            }
        }
        return n;
    };
    for (int k = 0; k < n_packets; k++) {
        const uint8_t *p = ts + size_t(k) * 188;
        if (p[0] != 0x47 || ((((p[1] & 0x1F) << 8) | p[2]) != pid)) continue;
        if (p[1] & 0x80) {                                          // transport_error_indicator: whatever it carried is lost
            have = -1, last_cc = -1;
            continue;
        }
        const int afc = (p[3] >> 4) & 3, cc = p[3] & 15;
        if (!(afc & 1)) continue;                                   // no payload: the counter stands
        if (last_cc >= 0 && cc == last_cc) continue;                // a duplicate
        if (last_cc >= 0 && cc != ((last_cc + 1) & 15)) have = -1;
        last_cc = cc;
        int at = 4;
        if (afc & 2) at += 1 + p[4];
        if (at >= 188) continue;
        if (p[1] & 0x40) {                                          // payload_unit_start_indicator: a pointer_field
            const int pointer = p[at++];
            if (at + pointer > 188) {
                have = -1;
                continue;
            }
            add(p + at, pointer);
            at += pointer;
            have = -1;                                              // (what the pointer did not complete is dropped)
            while (at < 188 && p[at] != 0xFF) {                     // sections back to back until stuffing
                have = 0;
                at += add(p + at, 188 - at);
            }
        } else {
            add(p + at, 188 - at);
        }
    }
}

}  // namespace

extern "C" {

int dabgpu_ts_programs(const uint8_t *ts, int n_packets, dabgpu_ts_info *info) {
    if (!info || n_packets < 0 || (n_packets > 0 && !ts)) return DABGPU_ERR_ARG;
    dabgpu_ts_info out{};
    out.transport_stream_id = out.network_pid = -1;
    sections_of(ts, n_packets, 0, [&](const uint8_t *s, int n) {
        if (s[0] != 0x00 || !(s[1] & 0x80) || n < 12) return;
        if (crc32_mpeg2(s, size_t(n)) != 0) {
            out.crc_errors++;
            return;
        }
        if (!(s[5] & 1)) return;                                    // current_next_indicator: not yet applicable
        out.pat_sections++;
        out.transport_stream_id = (s[3] << 8) | s[4];
        out.network_pid = -1;
        out.n_programs = 0;
        for (int i = 8; i + 4 <= n - 4; i += 4) {
            const int number = (s[i] << 8) | s[i + 1], pid = ((s[i + 2] & 0x1F) << 8) | s[i + 3];
            if (number == 0) {
                out.network_pid = pid;
                continue;
            }
            if (out.n_programs < DABGPU_TS_MAX_PROGRAMS) {
                dabgpu_ts_program pr{};
                pr.program_number = number;
                pr.pmt_pid = pid;
                out.programs[out.n_programs] = pr;
            }
            out.n_programs++;
        }
    });
    const int stored = out.n_programs < DABGPU_TS_MAX_PROGRAMS ? out.n_programs : DABGPU_TS_MAX_PROGRAMS;
    for (int q = 0; q < stored; q++) {
        bool done_before = false;                                   // (a PMT PID shared by programmes is assembled once)
        for (int q0 = 0; q0 < q; q0++) done_before = done_before || out.programs[q0].pmt_pid == out.programs[q].pmt_pid;
        if (done_before) continue;
        sections_of(ts, n_packets, out.programs[q].pmt_pid, [&](const uint8_t *s, int n) {
            if (s[0] != 0x02 || !(s[1] & 0x80) || n < 16) return;
            if (crc32_mpeg2(s, size_t(n)) != 0) {
                out.crc_errors++;
                return;
            }
            if (!(s[5] & 1)) return;
            const int number = (s[3] << 8) | s[4];
            for (int k = 0; k < stored; k++) {
                dabgpu_ts_program &pr = out.programs[k];
                if (pr.program_number != number || pr.pmt_pid != out.programs[q].pmt_pid) continue;
                out.pmt_sections++;
                pr.pmt_seen = 1;
                pr.pcr_pid = ((s[8] & 0x1F) << 8) | s[9];
                pr.iod_present = 0;
                pr.n_streams = 0;
                const int info_len = ((s[10] & 0x0F) << 8) | s[11], end = n - 4;
                int at = 12;
                if (at + info_len > end) return;
                for (int d = at; d + 2 <= at + info_len; d += 2 + s[d + 1]) pr.iod_present |= s[d] == 0x1D;
                at += info_len;
                while (at + 5 <= end) {
                    const int es_len = ((s[at + 3] & 0x0F) << 8) | s[at + 4];
                    if (at + 5 + es_len > end) break;
                    if (pr.n_streams < DABGPU_TS_MAX_STREAMS) {
                        pr.stream_type[pr.n_streams] = s[at];
                        pr.stream_pid[pr.n_streams] = ((s[at + 1] & 0x1F) << 8) | s[at + 2];
                    }
                    pr.n_streams++;
                    at += 5 + es_len;
                }
                break;
            }
        });
    }
    *info = out;
    return DABGPU_OK;
}

size_t dabgpu_dmb_state_bytes(void) { return size_t(dmb::STATE_BYTES); }

int dabgpu_dmb_max_packets(int bitrate_kbps, int n_cifs) {
    return (!dmb::bitrate_ok(bitrate_kbps) || n_cifs < 0 || n_cifs > dmb::MAX_N_CIFS) ? -1 : dmb::max_packets(bitrate_kbps, n_cifs);
}

int dabgpu_dmb_state_census(const void *state, int bitrate_kbps, dabgpu_dmb_census_entry *census) {
    if (!dmb::bitrate_ok(bitrate_kbps) || !census) return DABGPU_ERR_ARG;
    if (!state) return 0;
    dmb::Head h;
    std::memcpy(&h, state, sizeof h);
    if (!dmb::head_ok(h, bitrate_kbps)) return 0;
    std::memcpy(census, static_cast<const uint8_t *>(state) + dmb::CENSUS_AT, size_t(h.n_pids) * sizeof(dmb::CensusEntry));
    return h.n_pids;
}

int dabgpu_fig_stream_components(const uint8_t *fib, const uint8_t *crc_ok, int n_frames, dabgpu_stream_component *out, int max, int *n) {
    if (!fib || !crc_ok || !n || n_frames < 0 || max < 0 || (max > 0 && !out)) return DABGPU_ERR_ARG;
    return dabgpu_fig::stream_components(fib, crc_ok, n_frames, out, max, n);
}

int dabgpu_dmb_follow_dev(dabgpu_ctx *ctx, const dabgpu_dmb_entry *entries, int n_entries, int n_cifs, void *stream) {
    if (!ctx) return DABGPU_ERR_ARG;
    // everything is checked before anything is enqueued: a refused call leaves every output as it was
    std::vector<dabk::DmbEntry> table(size_t(n_entries > 0 ? n_entries : 0), dabk::DmbEntry{});
    const int bad = dmb_check(entries, n_entries, n_cifs, table.data());
    if (bad) return bad;
    if (n_entries == 0) return DABGPU_OK;
    if (n_entries > dabk::DMB_MAX_ENTRIES || dabk::dmb_blocks(table.data(), n_entries) > dabk::DMB_MAX_BLOCKS) return DABGPU_ERR_CAPACITY;
    const size_t table_bytes = dabk::dmb_table_bytes(table.data(), n_entries);
    return launch_entry_table(ctx, STAGE_DMB, table_bytes, stream, [&](void *d_table, size_t slot_bytes, hipStream_t s) {
        return dabk::launch_dmb(table.data(), n_entries, n_cifs, d_table, slot_bytes, s);
    });
}

int dabgpu_dmb_follow_host(const dabgpu_dmb_entry *entries, int n_entries, int n_cifs) {
    const int bad = dmb_check(entries, n_entries, n_cifs, nullptr);
    if (bad) return bad;
    static const dabgpu_packet_fec::Gf gf = dabgpu_packet_fec::make_gf();
    for (int i = 0; i < n_entries; i++) {
        const dabgpu_dmb_entry &e = entries[i];
        dmb::Result res;
        dmb::process(gf, static_cast<const uint8_t *>(e.d_state_in), static_cast<uint8_t *>(e.d_state_out), res, e.d_in, e.in_stride, n_cifs,
                     e.bitrate_kbps, e.d_ts, reinterpret_cast<dmb::Record *>(e.d_records), e.max_packets);
        std::memcpy(e.d_result, &res, sizeof res);
    }
    return DABGPU_OK;
}

}  // extern "C"
