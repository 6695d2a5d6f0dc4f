#include "basic_radio/basic_radio.h"

#include "dab/constants/subchannel_protection_tables.h"

#include <cstring>
#include <stdexcept>
#include <string>
#ifdef DABHOST_TIMING
#include <chrono>
#include <cstdio>
static double g_t[6];
static long g_n;
struct Tick { std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
              void lap(int i) { auto n = std::chrono::steady_clock::now(); g_t[i] += std::chrono::duration<double>(n - t).count(); t = n; } };
#define LAP(i) tick.lap(i)
#else
#define LAP(i)
#endif

BasicRadio::BasicRadio(const DAB_Parameters &params, size_t /*nb_threads*/) : m_params(params), m_ctx(nullptr) {
    dabgpu_cfg cfg{};
    cfg.device = GetDabGpuDefaultDevice();
    cfg.max_frames = 1;
    cfg.transmission_mode = 1;
    const int rc = dabgpu_create(&cfg, &m_ctx);
    if (rc != DABGPU_OK) throw std::runtime_error(std::string("BasicRadio: ") + dabgpu_strerror(rc));
    m_fib.resize(size_t(params.nb_fibs) * 32);
    m_crc.resize(size_t(params.nb_fibs));
    m_frame.resize(size_t(params.nb_frame_bits));
}

BasicRadio::~BasicRadio() {
#ifdef DABHOST_TIMING
    if (g_n) std::fprintf(stderr, "BasicRadio::Process per frame, us: set-up + copy %.1f | decode call %.1f | FIBs + FIG parser %.1f | sub-channel observers + channels %.1f | channel update %.1f (%ld frames)\n",
                          g_t[0] / g_n * 1e6, g_t[1] / g_n * 1e6, g_t[2] / g_n * 1e6, g_t[3] / g_n * 1e6, g_t[4] / g_n * 1e6, g_n);
#endif
    dabgpu_destroy(m_ctx);
}

int BasicRadio::AddSubchannel(const dabgpu_subchannel &sc) {
    std::lock_guard<std::mutex> lock(m_mutex);
    return add_subchannel_locked(sc);
}

// A sub-channel joins the per-frame call only if that call will accept it: inside the CIF and clear of every
// sub-channel already in the call (dabgpu_decode_frames_dev rejects a whole call whose sub-channels overlap -- one
// bad FIG 0/1 must not be able to silence the FIC and every other service).
int BasicRadio::add_subchannel_locked(const dabgpu_subchannel &sc) {
    const int nbytes = dabgpu_subchannel_bytes(&sc);
    if (nbytes < 0) return nbytes;
    if (sc.start_address < 0 || sc.length <= 0 || sc.start_address + sc.length > 864) return DABGPU_ERR_ARG;
    for (const Subchannel &o : m_subchannels)
        if (sc.start_address < o.desc.start_address + o.desc.length && o.desc.start_address < sc.start_address + sc.length)
            return DABGPU_ERR_ARG;
    Subchannel s;
    s.desc = sc;
    s.nbytes = nbytes;
    s.out.resize(size_t(m_params.nb_cifs) * nbytes);
    m_subchannels.push_back(std::move(s));
    return int(m_subchannels.size()) - 1;
}

void BasicRadio::Process(tcb::span<const viterbi_bit_t> buf) {
    if (buf.size() != size_t(m_params.nb_frame_bits)) return;   // the reference drops short frames the same way
    std::lock_guard<std::mutex> lock(m_mutex);
#ifdef DABHOST_TIMING
    Tick tick;
    g_n++;
#endif
    // A7..A12 in one call: the frame goes up once, the FIC and every registered sub-channel are decoded from that
    // copy, FIBs / CRC flags / logical frames / de-interleaver state come back together
    const size_t n_sub = m_subchannels.size();
    m_call_sc.resize(n_sub);
    m_call_out.resize(n_sub);
    for (size_t i = 0; i < n_sub; i++) {
        m_call_sc[i] = m_subchannels[i].desc;
        m_call_out[i] = m_subchannels[i].out.data();
    }
    std::memcpy(m_frame.data(), buf.data(), buf.size());
    LAP(0);
    // (the time de-interleaver state of every sub-channel stays on the device between frames)
    const int rc = dabgpu_decode_stream_frames(m_ctx, m_frame.data(), m_frame.size(), 1, m_fib.data(), m_crc.data(),
                                               m_call_sc.data(), int(n_sub), m_call_out.data());
    if (rc != DABGPU_OK) {
        // No exceptions on the streaming path.  The sub-channels' frame is lost (their de-interleaver rings on the device
        // were dropped by the failed call, so they start over), but the FIC must keep flowing: it is what repairs a
        // bad configuration.
        m_total_frames_lost++;
        for (Subchannel &s : m_subchannels) s.cifs_seen = 0;
        if (dabgpu_fic_decode(m_ctx, m_frame.data(), m_frame.size(), 1, m_fib.data(), m_crc.data()) != DABGPU_OK) return;
        process_fibs_locked();
        if (m_auto_channels) update_channels_from_database();
        return;
    }
    LAP(1);
    process_fibs_locked();
    LAP(2);
    for (size_t i = 0; i < n_sub; i++) {
        Subchannel &s = m_subchannels[i];
        for (int c = 0; c < m_params.nb_cifs; c++) {
            // the de-interleaver needs 16 CIFs before its first complete logical frame
            if (++s.cifs_seen < 16) continue;
            const tcb::span<const uint8_t> lf(s.out.data() + size_t(c) * s.nbytes, size_t(s.nbytes));
            m_obs_msc.Notify(int(i), lf);
            if (s.dab_plus) s.dab_plus->Process(lf);
            if (s.dab) s.dab->Process(lf);
            if (s.packet) s.packet->Process(lf);
            if (s.dmb) s.dmb->Process(lf);
        }
    }
    LAP(3);
    // sub-channels the FIC has announced by now join the call from the next frame on
    if (m_auto_channels) update_channels_from_database();
    LAP(4);
}

// FIB counters, the On_FIC observers and the FIG parser (mutex held)
void BasicRadio::process_fibs_locked() { process_fibs_locked(m_fib.data(), m_crc.data(), m_crc.size()); }

void BasicRadio::process_fibs_locked(const uint8_t *fib, const uint8_t *crc, size_t n_fibs) {
    for (size_t i = 0; i < n_fibs; i++) {
        m_total_fibs++;
        if (!crc[i]) m_total_fib_errors++;
    }
    m_obs_fic.Notify(tcb::span<const uint8_t>(fib, 32 * n_fibs), tcb::span<const uint8_t>(crc, n_fibs));
    for (size_t i = 0; i < n_fibs; i++)
        if (crc[i]) m_fic_parser.ProcessFIB(tcb::span<const uint8_t>(fib + 32 * i, 32));
}

void BasicRadio::ProcessEti(tcb::span<const uint8_t> bytes) {
    namespace er = dabgpu_eti_read;
    std::lock_guard<std::mutex> lock(m_mutex);
    // S = the tail the last call left + the new bytes
    m_eti_stream.insert(m_eti_stream.end(), bytes.begin(), bytes.end());
    er::Result c{};
    bool have = m_eti_head.have_prev != 0, any = false;
    uint32_t fct = m_eti_head.last_fct, fp = m_eti_head.last_fp;
    const size_t p = er::walk(m_eti_stream.data(), m_eti_stream.size(), nullptr, c,
                              [&](uint32_t, uint32_t at, int verdict, const er::Fields &f, const er::PtrFrame &g) {
        uint32_t fib_ok = 0;
        if (verdict == er::TAKEN) {
            // the FIC: three FIBs, their CRCs judged here
            const uint8_t *fic = g.p + f.fic_offset;
            uint8_t ok[3];
            for (int j = 0; j < 3; j++) {
                ok[j] = er::fib_crc_ok(g, f, j);
                fib_ok |= uint32_t(ok[j]) << j;
            }
            process_fibs_locked(fic, ok, 3);
            // the sub-channels: stream k of the frame's own STC goes to the open sub-channel at its start address
            size_t off = size_t(f.fic_offset) + er::FIC_BYTES;
            for (int k = 0; k < f.nst; k++) {
                const uint8_t *stc = g.p + 8 + 4 * k;
                const int sad = ((stc[0] & 3) << 8) | stc[1], nbytes = 8 * (((stc[2] & 3) << 8) | stc[3]);
                route_stream_locked(sad, nbytes, g.p + off);
                off += size_t(nbytes);
            }
            // sub-channels the FIC has announced by now are fed from the next frame on
            if (m_auto_channels) update_channels_from_database();
        }
        const er::Status st = er::make_status(at, verdict, f, fib_ok, have, fct, fp);
        have = any = true;
        fct = uint32_t(f.fct);
        fp = uint32_t(f.fp);
        return st;
    });
    m_eti_head = er::next_head(m_eti_head, c, any, fct, fp);
    m_eti_stream.erase(m_eti_stream.begin(), m_eti_stream.begin() + std::ptrdiff_t(p));
}

// one stream of a contribution frame or packet: its bytes of this CIF go to the open sub-channel at its start address
void BasicRadio::route_stream_locked(int start_address, int nbytes, const uint8_t *data) {
    for (size_t i = 0; i < m_subchannels.size(); i++) {
        Subchannel &s = m_subchannels[i];
        if (s.desc.start_address != start_address || s.nbytes != nbytes) continue;
        const tcb::span<const uint8_t> lf(data, size_t(nbytes));
        m_obs_msc.Notify(int(i), lf);
        if (s.dab_plus) s.dab_plus->Process(lf);
        if (s.dab) s.dab->Process(lf);
        if (s.packet) s.packet->Process(lf);
        if (s.dmb) s.dmb->Process(lf);
    }
}

void BasicRadio::ProcessEdi(tcb::span<const uint8_t> bytes) {
    namespace ed = dabgpu_edi;
    std::lock_guard<std::mutex> lock(m_mutex);
    // S = the tail the last call left + the new bytes
    m_edi_stream.insert(m_edi_stream.end(), bytes.begin(), bytes.end());
    ed::Result c{};
    ed::Carry k = ed::carry_of(m_edi_head);
    ed::Fields fields;
    const size_t p = ed::walk(m_edi_stream.data(), m_edi_stream.size(), nullptr, k, c, fields,
                              [&](uint32_t, uint32_t at, int total, const ed::Fields &f, bool seq_break, const ed::Carry &before, const ed::PtrPacket &g) {
        uint32_t fib_ok = 0;
        if (f.ficf) {
            // the FIC: three FIBs, their CRCs judged here
            uint8_t ok[3];
            for (int j = 0; j < 3; j++) {
                ok[j] = ed::fib_crc_ok(g, f.fic_at, j);
                fib_ok |= uint32_t(ok[j]) << j;
            }
            process_fibs_locked(g.p + f.fic_at, ok, 3);
        }
        // the sub-channels: est n of the packet goes to the open sub-channel at its start address
        for (int n = 0; n < f.n_est; n++)
            route_stream_locked(((f.sstc[n][0] & 3) << 8) | f.sstc[n][1], 8 * int(f.stl[n]), g.p + f.data_at[n]);
        // sub-channels the FIC has announced by now are fed from the next packet on
        if (m_auto_channels) update_channels_from_database();
        return ed::make_status(at, total, f, fib_ok, seq_break, before);
    });
    m_edi_head = ed::next_head(m_edi_head, c, k);
    m_edi_stream.erase(m_edi_stream.begin(), m_edi_stream.begin() + std::ptrdiff_t(p));
}

void BasicRadio::ProcessPft(tcb::span<const uint8_t> bytes, bool flush) {
    namespace pf = dabgpu_pft;
    static const pf::Gf gf = pf::make_gf();
    std::vector<uint8_t> out;
    pf::Result result{};
    {
        std::lock_guard<std::mutex> lock(m_pft_mutex);
        const uint8_t *state_in = m_pft_state.empty() ? nullptr : m_pft_state.data();
        pf::Head in{};
        if (state_in) std::memcpy(&in, state_in, sizeof in);
        // S = the tail the last call left + the new bytes
        const size_t tail = pf::clamp_tail(in.tail_bytes);
        std::vector<uint8_t> s(tail + bytes.size());
        if (tail) std::memcpy(s.data(), state_in + pf::STATE_TAIL_AT, tail);
        if (!bytes.empty()) std::memcpy(s.data() + tail, bytes.data(), bytes.size());
        out.resize(size_t(pf::read_out_bytes(uint32_t(bytes.size()))));
        std::vector<pf::Record> records(pf::read_max_records(uint32_t(bytes.size())));
        std::vector<uint8_t> scratch(static_cast<size_t>(pf::MAX_BLOCK), 0);
        m_pft_next.assign(size_t(pf::STATE_BYTES), 0);
        pf::read_entry(gf, s.data(), s.size(), state_in, flush ? uint32_t(pf::READ_FLUSH) : 0u, out.data(), records.data(), uint32_t(records.size()),
                       &result, m_pft_next.data(), scratch.data());
        m_pft_state.swap(m_pft_next);
    }
    // (packets that are no AF packets go along: ProcessEdi resynchronises over them and counts them)
    if (result.out_bytes) ProcessEdi({out.data(), size_t(result.out_bytes)});
}

dabgpu_pft::Head BasicRadio::GetPftReadTotals() const {
    dabgpu_pft::Head h{};
    std::lock_guard<std::mutex> lock(m_pft_mutex);
    if (!m_pft_state.empty()) std::memcpy(&h, m_pft_state.data(), sizeof h);
    return h;
}

// what the per-frame call needs to know of a sub-channel the FIC has described; false: a profile it cannot decode
bool BasicRadio::describe_subchannel(::Subchannel &sub, dabgpu_subchannel &sc) {
    sc = dabgpu_subchannel{};
    if (sub.is_uep) {
        // short form: bit rate, level and size come from the protection profile table
        if (dabgpu_uep_subchannel(sub.uep_prot_index, sub.start_address, &sc) != DABGPU_OK) return false;
        sub.length = uint16_t(sc.length);
        return true;
    }
    if (sub.eep_prot_level > 3 || sub.length == 0) return false;
    sc.start_address = sub.start_address;
    sc.length = sub.length;
    sc.protection_level = sub.eep_prot_level + 1;           // the ABI counts levels 1..4
    sc.eep_type = sub.eep_type == EEP_Type::TYPE_B ? 1 : 0;
    sc.bitrate_kbps = int(CalculateEEPBitrate(sub));
    return sc.bitrate_kbps > 0;
}

// the index of the described sub-channel in the per-frame call, joining it if need be; negative: it cannot join.
// A sub-channel registered by hand (AddSubchannel) that the FIC now announces with the same range and profile is
// already open: the channel attaches to it instead of claiming the range twice
int BasicRadio::open_subchannel(const dabgpu_subchannel &sc) {
    for (size_t k = 0; k < m_subchannels.size(); k++) {
        const dabgpu_subchannel &d = m_subchannels[k].desc;
        if (d.start_address == sc.start_address && d.length == sc.length && d.bitrate_kbps == sc.bitrate_kbps &&
            d.is_uep == sc.is_uep && d.eep_type == sc.eep_type && d.protection_level == sc.protection_level && !m_subchannels[k].dab_plus &&
            !m_subchannels[k].dab && !m_subchannels[k].packet && !m_subchannels[k].dmb)
            return int(k);
    }
    return add_subchannel_locked(sc);
}

// Open a data packet channel for every packet-mode component (MOT in data groups: slides and carousels; any other: its data
// groups or raw bytes as they are), once FIG 0/2, FIG 0/3 and
// FIG 0/1 have all spoken; further addresses of an open sub-channel join its channel (up to four)
void BasicRadio::update_packet_channels() {
    size_t described = 0;
    for (const auto &pc : m_database.packet_components) described += pc.has_service && pc.is_described;
    for (auto &kv : m_packet_channels) {
        kv.second->SetFecScheme(m_database.fec_scheme[kv.first & 63]);
        kv.second->SetFecCorrection(m_database.fec_scheme[kv.first & 63] == 1);
    }
    if (described == m_seen_packet_described && !m_pending_packets) return;
    m_pending_packets = false;
    for (const auto &pc : m_database.packet_components) {
        if (!pc.has_service || !pc.is_described) continue;
        // MOT in data groups goes to the slides and the carousel control; anything else is handed out as data groups or,
        // without data groups, as raw bytes
        const bool mot = pc.dscty == 60 && !pc.dg_flag;
        auto open = m_packet_channels.find(pc.subchannel_id);
        if (open != m_packet_channels.end()) {
            if (mot) open->second->FollowAddress(pc.packet_address);
            else open->second->FollowDataGroups(pc.packet_address, pc.dg_flag ? 1 : 0);
            continue;
        }
        if (m_channels.count(pc.subchannel_id)) continue;       // (an audio channel has the sub-channel)
        bool rejected = false;
        for (auto id : m_rejected) rejected |= (id == pc.subchannel_id);
        if (rejected) continue;
        ::Subchannel *sub = nullptr;
        for (auto &s : m_database.subchannels)
            if (s.id == pc.subchannel_id) sub = &s;
        if (!sub) {                                          // FIG 0/1 for it has not arrived yet
            m_pending_packets = true;
            continue;
        }
        dabgpu_subchannel sc{};
        // (packets need whole slots: a bit rate that is a multiple of 8, at most 512)
        const int idx = describe_subchannel(*sub, sc) && sc.bitrate_kbps % 8 == 0 && sc.bitrate_kbps <= 512 ? open_subchannel(sc) : -1;
        if (idx < 0) {
            m_rejected.push_back(sub->id);
            m_total_unsupported++;
            continue;
        }
        auto ch = std::make_unique<Basic_Data_Packet_Channel>(*sub, m_database.fec_scheme[sub->id & 63]);
        ch->SetFecCorrection(ch->GetFecScheme() == 1);
        if (mot) ch->FollowAddress(pc.packet_address);
        else ch->FollowDataGroups(pc.packet_address, pc.dg_flag ? 1 : 0);
        m_subchannels[size_t(idx)].packet = ch.get();
        m_packet_channels.emplace(sub->id, std::move(ch));
    }
    m_seen_packet_described = described;
}

// Open every component whose sub-channel the FIC has described (called with the mutex held).
void BasicRadio::update_channels_from_database() {
    update_audio_channels();
    update_packet_channels();
    update_dmb_channels();
}

// Open a DMB channel for every stream-mode data component whose DSCTy says MPEG-2 transport stream, once FIG 0/2 and
// FIG 0/1 have both spoken.  Components of another DSCTy stay in the database and are not followed.
void BasicRadio::update_dmb_channels() {
    if (m_database.stream_components.size() == m_seen_stream_components && !m_pending_streams) return;
    m_pending_streams = false;
    for (const auto &comp : m_database.stream_components) {
        if (comp.dscty != uint8_t(DataServiceType::MPEG2)) continue;
        if (m_dmb_channels.count(comp.subchannel_id) || m_channels.count(comp.subchannel_id) || m_packet_channels.count(comp.subchannel_id)) continue;
        bool rejected = false;
        for (auto id : m_rejected) rejected |= (id == comp.subchannel_id);
        if (rejected) continue;
        ::Subchannel *sub = nullptr;
        for (auto &s : m_database.subchannels)
            if (s.id == comp.subchannel_id) sub = &s;
        if (!sub) {                                          // FIG 0/1 for it has not arrived yet
            m_pending_streams = true;
            continue;
        }
        dabgpu_subchannel sc{};
        const int idx = describe_subchannel(*sub, sc) && dabgpu_dmb::bitrate_ok(sc.bitrate_kbps) ? open_subchannel(sc) : -1;
        if (idx < 0) {
            m_rejected.push_back(sub->id);
            m_total_unsupported++;
            continue;
        }
        auto ch = std::make_unique<Basic_DMB_Channel>(*sub, sc.bitrate_kbps);
        m_subchannels[size_t(idx)].dmb = ch.get();
        m_dmb_channels.emplace(sub->id, std::move(ch));
    }
    m_seen_stream_components = m_database.stream_components.size();
}

void BasicRadio::update_audio_channels() {
    if (m_database.service_components.size() == m_seen_components && !m_pending_components) return;
    m_pending_components = false;
    for (const auto &comp : m_database.service_components) {
        if (comp.transport_mode != TransportMode::STREAM_MODE_AUDIO) continue;
        const bool is_dab_plus = comp.audio_service_type == AudioServiceType::DAB_PLUS;
        const bool is_dab = comp.audio_service_type == AudioServiceType::DAB;
        if (!is_dab_plus && !is_dab) continue;
        if (m_channels.count(comp.subchannel_id)) continue;
        bool rejected = false;
        for (auto id : m_rejected) rejected |= (id == comp.subchannel_id);
        if (rejected) continue;
        ::Subchannel *sub = nullptr;
        for (auto &s : m_database.subchannels)
            if (s.id == comp.subchannel_id) sub = &s;
        if (!sub) {                                          // FIG 0/1 for it has not arrived yet
            m_pending_components = true;
            continue;
        }
        dabgpu_subchannel sc{};
        const int idx = describe_subchannel(*sub, sc) ? open_subchannel(sc) : -1;
        if (idx < 0) {
            m_rejected.push_back(sub->id);
            m_total_unsupported++;
            continue;
        }
        Basic_Audio_Channel *ref = nullptr;
        if (is_dab_plus) {
            auto ch = std::make_unique<Basic_DAB_Plus_Channel>(m_ctx, *sub, sc.bitrate_kbps);
            m_subchannels[size_t(idx)].dab_plus = ch.get();
            ref = ch.get();
            m_channels.emplace(sub->id, std::move(ch));
        } else {
            auto ch = std::make_unique<Basic_DAB_Channel>(*sub, sc.bitrate_kbps);
            m_subchannels[size_t(idx)].dab = ch.get();
            ref = ch.get();
            m_channels.emplace(sub->id, std::move(ch));
        }
        m_obs_audio_channel.Notify(sub->id, *ref);
    }
    m_seen_components = m_database.service_components.size();
}
