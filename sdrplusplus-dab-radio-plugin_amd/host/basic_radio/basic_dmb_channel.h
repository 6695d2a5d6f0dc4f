// basic_radio/basic_dmb_channel.h -- what BasicRadio::Get_DMB_Channel returns: a stream-mode data sub-channel (FIG 0/2
// TMId 1) whose DSCTy says MPEG-2 transport stream (24): T-DMB video and visual radio.  Process takes the sub-channel's
// logical frames; every frame goes through the serial receiver of include/dabgpu_dmb.h -- the code dabgpu_dmb_follow_dev
// and dabgpu_dmb_follow_host run -- as a call of one frame with the state record handed on (no export of libdabgpu is
// called): sync search, the de-interleaving gather, RS(204,188), continuity counters and the PID census.  The TS packets a
// frame completes go to OnTransportPackets with their records, ready to be written to a file or pipe; the counters add up
// (GetStatistics), the census is the state record's.
#pragma once
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>
#include "dab/database/dab_database_entities.h"
#include "dabgpu_dmb.h"
#include "utility/observable.h"
#include "utility/span.h"

class Basic_DMB_Channel {
public:
    explicit Basic_DMB_Channel(const Subchannel &subchannel, int bitrate_kbps) : m_subchannel(subchannel), m_kbps(bitrate_kbps) {
        for (auto &st : m_state) st = std::make_unique<Record>();
        // (a bit rate the header refuses: Process counts every frame as ignored; the buffers are sized for the largest rate)
        const size_t room = size_t(dabgpu_dmb::max_packets(dabgpu_dmb::bitrate_ok(bitrate_kbps) ? bitrate_kbps : dabgpu_dmb::MAX_KBPS, 1));
        m_ts.resize(room * dabgpu_dmb::TS_BYTES);
        m_records.resize(room);
    }
    const Subchannel &GetSubchannel() const { return m_subchannel; }
    int GetBitrate() const { return m_kbps; }
    // (the 188-byte packets one frame completed, back to back, and a record for each)
    auto &OnTransportPackets() { return m_obs_packets; }
    // counts since the channel was opened (cifs, bytes, sync_hits, locks, ..., duplicates), and where the stream stands
    // (locked, phase, pids, pids_overflowed)
    const dabgpu_dmb::Result &GetStatistics() const { return m_total; }
    // the first 32 distinct PIDs in the order they appeared, cumulative counts
    tcb::span<const dabgpu_dmb::CensusEntry> GetCensus() const {
        const dabgpu_dmb::State &st = *reinterpret_cast<const dabgpu_dmb::State *>(m_state[m_turn]->bytes);
        return {st.census, m_started ? size_t(st.head.n_pids) : size_t(0)};
    }
    int GetTotalFramesIgnored() const { return m_total_ignored; }

    // one logical frame of the sub-channel: 3 * bit rate bytes (any other size is counted and ignored)
    void Process(tcb::span<const uint8_t> lf) {
        namespace dmb = dabgpu_dmb;
        static const dabgpu_packet_fec::Gf gf = dabgpu_packet_fec::make_gf();
        if (!dmb::bitrate_ok(m_kbps) || lf.size() != size_t(dmb::frame_bytes(m_kbps))) {
            m_total_ignored++;
            return;
        }
        dmb::Result r;
        dmb::process(gf, m_started ? m_state[m_turn]->bytes : nullptr, m_state[m_turn ^ 1]->bytes, r, lf.data(), lf.size(), 1, m_kbps, m_ts.data(),
                     m_records.data(), int(m_records.size()));
        m_turn ^= 1;
        m_started = true;
        int32_t *sum = reinterpret_cast<int32_t *>(&m_total);
        for (int i = 0; i < COUNTERS; i++) sum[i] += reinterpret_cast<const int32_t *>(&r)[i];
        m_total.locked = r.locked, m_total.phase = r.phase, m_total.pids = r.pids, m_total.pids_overflowed = r.pids_overflowed;
        m_total.packets_deferred = r.packets_deferred, m_total.packets_lost += r.packets_lost;    // (room for everything: both stay 0)
        if (r.packets_emitted)
            m_obs_packets.Notify(tcb::span<const uint8_t>(m_ts.data(), size_t(r.packets_emitted) * dmb::TS_BYTES),
                                 tcb::span<const dmb::Record>(m_records.data(), size_t(r.packets_emitted)));
    }

private:
    static constexpr int COUNTERS = dabgpu_dmb::SUMMED_COUNTERS;       // cifs .. duplicates
    struct Record {
        alignas(16) uint8_t bytes[dabgpu_dmb::STATE_BYTES] = {};       // all zero: a fresh start
    };
    Subchannel m_subchannel;
    int m_kbps;
    std::unique_ptr<Record> m_state[2];
    int m_turn = 0, m_total_ignored = 0;
    bool m_started = false;
    dabgpu_dmb::Result m_total{};
    std::vector<uint8_t> m_ts;
    std::vector<dabgpu_dmb::Record> m_records;
    Observable<tcb::span<const uint8_t>, tcb::span<const dabgpu_dmb::Record>> m_obs_packets;
};
