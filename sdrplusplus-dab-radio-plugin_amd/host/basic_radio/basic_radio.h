// basic_radio/basic_radio.h -- host-side mirror of the reference's BasicRadio for the hot path:
// ctor (/root/reference/src/radio_block.cpp:60), Process(span<const viterbi_bit_t>) (:42), GetMutex()
// (src/render_radio_block.cpp:124), On_Audio_Channel() (src/radio_block.cpp:62).
//
// Process splits a frame into FIC and MSC (row A7) and runs rows A8..A12 on the GPU through libdabgpu: the FIC and
// every registered sub-channel in ONE dabgpu_decode_stream_frames call per frame (one upload of the 230400 soft bits,
// three launches, one download, one synchronisation; the de-interleaver state never leaves the device).  A sub-channel the FIC announces in frame f is decoded from
// frame f+1 on.  The FIBs go through the FIG
// parser into the database; every audio component found there (DAB+ or DAB, EEP or UEP sub-channel)
// gets its sub-channel decoded and a Basic_DAB_Plus_Channel (8f-3) / Basic_DAB_Channel without being asked (On_Audio_Channel fires once per
// channel, as in the reference).  Audio decoding is outside the path: channels hand out access units.  A packet-mode
// component that carries MOT in data groups (FIG 0/3: DSCTy 60, DG flag 0) gets its sub-channel decoded and a
// Basic_Data_Packet_Channel that follows its packet address to slides.
#pragma once
#include <cstdint>
#include <mutex>
#include <vector>
#include <map>
#include <memory>
#include "basic_radio/basic_audio_channel.h"
#include "basic_radio/basic_dab_channel.h"
#include "basic_radio/basic_dab_plus_channel.h"
#include "basic_radio/basic_data_packet_channel.h"
#include "basic_radio/basic_dmb_channel.h"
#include "dab/constants/dab_parameters.h"
#include "dab/database/dab_database.h"
#include "dab/database/dab_database_updater.h"
#include "dab/fic/fic_parser.h"
#include "dabgpu.h"
#include "dabgpu_edi.h"
#include "dabgpu_eti_read.h"
#include "dabgpu_pft.h"
#include "utility/gpu_buffers.h"
#include "utility/observable.h"
#include "utility/span.h"
#include "viterbi_config.h"

class BasicRadio {
public:
    BasicRadio(const DAB_Parameters &params, size_t nb_threads = 0);
    ~BasicRadio();
    BasicRadio(const BasicRadio &) = delete;
    BasicRadio &operator=(const BasicRadio &) = delete;

    void Process(tcb::span<const viterbi_bit_t> buf);
    // The contribution side: the next bytes of an ETI(NI) byte stream (raw 6144-byte frames; cut anywhere, bytes may be
    // missing) instead of soft bits.  The header-only walk of include/dabgpu_eti_read.h runs on the host -- frames found,
    // both CRCs checked, resynchronised after damage, the unfinished tail kept for the next call -- and every taken frame's
    // FIBs go where Process sends them and its sub-channels' bytes to the channels Process feeds (the multiplex is read
    // from the frame's own STC and matched by start address).  No call into libdabgpu.
    void ProcessEti(tcb::span<const uint8_t> bytes);
    // running totals of ProcessEti: rows, taken, bad_data_crc, skipped, resyncs, gap_sum, fib_errors; tail_bytes held
    const dabgpu_eti_read::Head &GetEtiReadTotals() const { return m_eti_head; }
    // The same for an EDI byte stream (AF packets back to back, as a TCP capture is): the serial walk of
    // include/dabgpu_edi.h -- packets found by header and CRC, resynchronised after damage, the unfinished tail kept for the
    // next call -- and every DETI packet's FIBs and est items routed as ProcessEti routes a frame's.  No call into libdabgpu.
    void ProcessEdi(tcb::span<const uint8_t> bytes);
    // running totals of ProcessEdi: rows, not_deti, bad_tags, skipped, resyncs, gap_sum, fib_errors; tail_bytes held
    const dabgpu_edi::Head &GetEdiReadTotals() const { return m_edi_head; }
    // The same for EDI as it travels over UDP: a byte stream of PF fragments (datagram payloads one after the other).  The
    // serial reader of include/dabgpu_pft.h puts the AF packets back together -- fragments in any order, missing ones filled by
    // RS(255,207) erasure decoding where they can be -- and hands them to ProcessEdi.  flush: close every open group at the
    // end (the stream ends here).  No call into libdabgpu.
    void ProcessPft(tcb::span<const uint8_t> bytes, bool flush = false);
    // running totals of ProcessPft (records, packets, lost, recovered, fragments, ...)
    dabgpu_pft::Head GetPftReadTotals() const;
    std::mutex &GetMutex() { return m_mutex; }
    Observable<subchannel_id_t, Basic_Audio_Channel &> &On_Audio_Channel() { return m_obs_audio_channel; }
    // read under GetMutex(), as the GUI does (/root/reference/src/render_radio_block.cpp:124, 158-160, 239, 755)
    DAB_Database &GetDatabase() { return m_database; }
    const DAB_Database_Statistics &GetDatabaseStatistics() const { return m_updater.GetStatistics(); }
    const DAB_Misc_Info &GetMiscInfo() const { return m_updater.GetMiscInfo(); }     // render_radio_block.cpp:814
    Basic_Audio_Channel *Get_Audio_Channel(subchannel_id_t id) {
        auto it = m_channels.find(id);
        return it == m_channels.end() ? nullptr : it->second.get();
    }
    // the channel of a packet-mode sub-channel with a MOT component (render_radio_block.cpp:533), nullptr for any other
    Basic_Data_Packet_Channel *Get_Data_Packet_Channel(subchannel_id_t id) {
        auto it = m_packet_channels.find(id);
        return it == m_packet_channels.end() ? nullptr : it->second.get();
    }
    // the channel of a stream-mode data sub-channel whose DSCTy says MPEG-2 transport stream (T-DMB), nullptr for any other
    Basic_DMB_Channel *Get_DMB_Channel(subchannel_id_t id) {
        auto it = m_dmb_channels.find(id);
        return it == m_dmb_channels.end() ? nullptr : it->second.get();
    }
    // sub-channels listed in the FIC that cannot be decoded here (invalid profile, does not fit the CIF)
    int GetTotalUnsupportedSubchannels() const { return m_total_unsupported; }
    void SetAutoChannels(bool v) { m_auto_channels = v; }

    // ---- hot-path outputs (extensions) ----
    // 12 FIBs x 32 bytes and their CRC flags, once per frame
    Observable<tcb::span<const uint8_t>, tcb::span<const uint8_t>> &On_FIC() { return m_obs_fic; }
    // decoded logical frame of a registered subchannel: (index from AddSubchannel, bytes); 4 per frame
    Observable<int, tcb::span<const uint8_t>> &On_MSC_Frame() { return m_obs_msc; }
    // returns the subchannel index, or a negative dabgpu_status
    int AddSubchannel(const dabgpu_subchannel &sc);
    int GetTotalFIBs() const { return m_total_fibs; }
    int GetTotalFIBErrors() const { return m_total_fib_errors; }
    // frames whose sub-channels could not be decoded (the per-frame GPU call failed; the FIC was decoded on its own)
    int GetTotalFramesLost() const { return m_total_frames_lost; }
    // test hook (host/demo/dab_host_multi.cpp): the nth decode call into libdabgpu from now on reports a device failure
    void TestFailDeviceCall(int nth) { (void)dabgpu_test_fail_frame_call(m_ctx, nth); }

private:
    struct Subchannel {
        dabgpu_subchannel desc;
        int nbytes;
        int cifs_seen = 0;
        PinnedBuffer<uint8_t> out;
        Basic_DAB_Plus_Channel *dab_plus = nullptr;   // set for sub-channels opened from the database
        Basic_DAB_Channel *dab = nullptr;
        Basic_Data_Packet_Channel *packet = nullptr;
        Basic_DMB_Channel *dmb = nullptr;
    };
    bool describe_subchannel(::Subchannel &sub, dabgpu_subchannel &sc);
    int open_subchannel(const dabgpu_subchannel &sc);
    void update_audio_channels();
    void update_packet_channels();
    void update_dmb_channels();
    void update_channels_from_database();
    void process_fibs_locked();
    void process_fibs_locked(const uint8_t *fib, const uint8_t *crc, size_t n_fibs);
    void route_stream_locked(int start_address, int nbytes, const uint8_t *data);
    int add_subchannel_locked(const dabgpu_subchannel &sc);
    const DAB_Parameters m_params;
    dabgpu_ctx *m_ctx;
    std::mutex m_mutex;
    std::vector<Subchannel> m_subchannels;
    PinnedBuffer<uint8_t> m_fib, m_crc;
    PinnedBuffer<viterbi_bit_t> m_frame;                 // the frame's soft bits, staged for the single upload
    std::vector<dabgpu_subchannel> m_call_sc;            // argument arrays of the per-frame call
    std::vector<uint8_t *> m_call_out;
    int m_total_fibs = 0, m_total_fib_errors = 0;
    Observable<subchannel_id_t, Basic_Audio_Channel &> m_obs_audio_channel;
    Observable<tcb::span<const uint8_t>, tcb::span<const uint8_t>> m_obs_fic;
    Observable<int, tcb::span<const uint8_t>> m_obs_msc;
    DAB_Database m_database;
    DAB_Database_Updater m_updater{m_database};
    FIC_Parser m_fic_parser{m_updater};
    std::map<subchannel_id_t, std::unique_ptr<Basic_Audio_Channel>> m_channels;
    std::map<subchannel_id_t, std::unique_ptr<Basic_Data_Packet_Channel>> m_packet_channels;
    std::map<subchannel_id_t, std::unique_ptr<Basic_DMB_Channel>> m_dmb_channels;
    size_t m_seen_stream_components = 0;
    bool m_pending_streams = false;                      // ... a stream-mode data component
    std::vector<subchannel_id_t> m_rejected;             // sub-channels we looked at and cannot open
    size_t m_seen_components = 0;
    size_t m_seen_packet_described = 0;                  // packet components FIG 0/2 has named and FIG 0/3 described
    bool m_pending_components = false;                   // a component whose sub-channel is not described yet
    bool m_pending_packets = false;                      // ... a packet component
    bool m_auto_channels = true;
    int m_total_unsupported = 0;
    int m_total_frames_lost = 0;
    dabgpu_eti_read::Head m_eti_head{};                  // ProcessEti: the state between calls, its tail in m_eti_stream
    std::vector<uint8_t> m_eti_stream;                   // S of the current call; what the walk leaves is the next call's tail
    dabgpu_edi::Head m_edi_head{};                       // ProcessEdi: the same
    std::vector<uint8_t> m_edi_stream;
    mutable std::mutex m_pft_mutex;                      // ProcessPft's own (ProcessEdi takes m_mutex itself); GetPftReadTotals takes it too
    std::vector<uint8_t> m_pft_state, m_pft_next;        // ProcessPft: the state record between calls (empty: a stream that starts)
};
