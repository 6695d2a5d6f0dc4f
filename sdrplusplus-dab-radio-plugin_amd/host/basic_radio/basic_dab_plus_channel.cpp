#include "basic_radio/basic_dab_plus_channel.h"

#include <cstring>
#include <memory>
#include <mutex>
#include <string>

Basic_DAB_Plus_Channel::Basic_DAB_Plus_Channel(dabgpu_ctx *ctx, const Subchannel &subchannel, int bitrate_kbps)
    : m_ctx(ctx), m_subchannel(subchannel), m_bitrate(bitrate_kbps), m_lf_bytes(size_t(bitrate_kbps) * 3) {
    m_window.resize(5 * m_lf_bytes);
    m_data.resize(size_t(110) * (bitrate_kbps / 8));
    m_status.resize(1);
    m_mot_call.body_capacity = MOT_BODY_CAPACITY;
    m_mot_call.max_slides = MOT_SLOTS;
    m_mot_call.slide_stride = uint32_t(dabgpu_mot::RECORD_BYTES + dabgpu_mot::HEADER_CAP + MOT_BODY_CAPACITY);
    m_mot_arena.resize(size_t(dabgpu_mot::arena_bytes(MOT_BODY_CAPACITY)));
    m_mot_slides.resize(size_t(MOT_SLOTS) * m_mot_call.slide_stride);
    dabgpu_mot::sanitize(m_mot, MOT_BODY_CAPACITY);
}

// one access unit through the MOT walk; its copy orders are executed here, and what completed goes to the manager
void Basic_DAB_Plus_Channel::WalkMot(const uint8_t *au, int len) {
    dabgpu_mot::Orders orders;
    m_mot_counts.slides_written = 0;                                   // the slots are this access unit's
    dabgpu_mot::walk_au(m_mot, m_mot_counts, orders, m_mot_call, au, len);
    for (int i = 0; i < orders.n; i++) dabgpu_mot::execute(orders.o[i], orders, au, m_mot_arena.data(), m_mot_slides.data());
    for (int k = 0; k < m_mot_counts.slides_written; k++) AddSlide(m_mot_slides.data() + size_t(k) * m_mot_call.slide_stride);
}

// (TWO PLACES: basic_pad_reader.h, Basic_Add_Slide, is this function for the layer-II channel; a change goes into both)
void Basic_DAB_Plus_Channel::AddSlide(const uint8_t *slot) {
    int32_t rec[8];
    std::memcpy(rec, slot, sizeof rec);
    const uint8_t *header = slot + dabgpu_mot::RECORD_BYTES, *body = header + rec[3];
    dabgpu_mot::Header h;
    if (dabgpu_mot::parse_header(header, rec[3], h) != 0 || h.content_type != 2) return;      // images only (TS 101 499 clause 6.2)
    auto text = [](const dabgpu_mot::Text &t) { return t.length > 0 ? std::string(reinterpret_cast<const char *>(t.bytes), size_t(t.length)) : std::string(); };
    auto slide = std::make_shared<Basic_Slideshow>();
    slide->transport_id = mot_transport_id_t(rec[0]);
    slide->name = text(h.name);
    slide->trigger_time = h.has_trigger && !h.trigger_now ? h.trigger_time : 0;
    slide->expire_time = h.has_expire && !h.expire_now ? h.expire_time : 0;
    slide->category_id = uint8_t(h.category_id);
    slide->slide_id = uint8_t(h.slide_id);
    slide->category_title = text(h.category_title);
    slide->click_through_url = text(h.click_through_url);
    slide->alt_location_url = text(h.alternative_location_url);
    slide->image_data.assign(body, body + rec[4]);
    auto lock = std::scoped_lock(m_slideshows.GetSlideshowsMutex());
    auto &all = m_slideshows.GetSlideshows();
    all.push_back(slide);
    m_slideshows.OnNewSlideshow().Notify(slide);
    while (all.size() > m_slideshows.GetMaxSize()) {                  // the oldest leaves
        auto oldest = all.front();
        m_slideshows.OnRemoveSlideshow().Notify(oldest);
        all.pop_front();
    }
}

void Basic_DAB_Plus_Channel::Process(tcb::span<const uint8_t> lf) {
    if (lf.size() != m_lf_bytes) return;
    std::memcpy(m_window.data() + size_t(m_frames_in_window) * m_lf_bytes, lf.data(), m_lf_bytes);
    if (++m_frames_in_window < 5) return;
    // five logical frames: a super-frame if we are aligned; the Fire code (checked after RS correction) says so
    dabgpu_superframe_status &st = m_status[0];
    const int rc = dabgpu_dabplus_superframes(m_ctx, m_window.data(), m_window.size(), 1, m_bitrate, m_data.data(), &st);
    if (rc != DABGPU_OK || !st.firecode_ok) {
        // not aligned (or a lost super-frame): slide by one logical frame and try again with the next one
        m_firecode_error = true;
        m_synced = false;
        dabgpu_pad::walk_au(m_pad, m_pad_counts, nullptr, -1);        // whatever PAD was being collected has a hole now
        WalkMot(nullptr, -1);
        std::memmove(m_window.data(), m_window.data() + m_lf_bytes, 4 * m_lf_bytes);
        m_frames_in_window = 4;
        return;
    }
    m_synced = true;
    m_frames_in_window = 0;
    m_total_superframes++;
    m_firecode_error = false;
    m_rs_error = st.rs_uncorrectable != 0;
    // header byte 2: rfa | dac_rate | sbr_flag | aac_channel_mode | ps_flag | mpeg_surround_config(3)
    const uint8_t h = m_data[2];
    const bool dac_rate = (h >> 6) & 1, sbr = (h >> 5) & 1, stereo = (h >> 4) & 1, ps = (h >> 3) & 1;
    m_header.sampling_rate = dac_rate ? 48000 : 32000;
    m_header.is_spectral_band_replication = sbr;
    m_header.is_stereo = stereo;
    m_header.is_parametric_stereo = ps;
    m_header.mpeg_surround = mpeg_surround_from_config(h & 7);
    m_header.nb_access_units = uint8_t(st.num_aus);
    bool au_error = false;
    const bool read_pad = m_controls.GetIsDecodeData();
    for (int a = 0; a < st.num_aus && a < 7; a++) {
        m_total_aus++;
        if (read_pad) {
            int at = 0;
            const int len = dabgpu_pad::au_span(st.firecode_ok, st.num_aus, st.au_crc_mask, st.au_start[a], st.au_start[a + 1], a,
                                                m_bitrate / 8, &at);
            dabgpu_pad::walk_au(m_pad, m_pad_counts, m_data.data() + at, len);
            WalkMot(m_data.data() + at, len);
        }
        if (!((st.au_crc_mask >> a) & 1)) {
            au_error = true;
            m_total_au_errors++;
            continue;
        }
        // the access unit handed on is the payload alone: its trailing CRC16 (already checked on the GPU) is dropped,
        // which is what an AAC decoder / ADTS muxer behind the observer expects
        const int b = st.au_start[a], e = st.au_start[a + 1] - 2;
        if (b < 0 || e <= b || size_t(e) + 2 > m_data.size()) continue;
        if (m_controls.GetIsDecodeAudio())
            m_obs_au.Notify(a, st.num_aus, tcb::span<const uint8_t>(m_data.data() + b, size_t(e - b)));
    }
    m_au_error = au_error;
    if (read_pad) m_dynamic_label.assign(reinterpret_cast<const char *>(m_pad.label.text), size_t(m_pad.label.length));
}
