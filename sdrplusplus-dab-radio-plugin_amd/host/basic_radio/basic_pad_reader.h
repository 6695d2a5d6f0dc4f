// basic_radio/basic_pad_reader.h -- what an audio channel does with the PAD of one access unit, whatever audio kind
// carried it: the label walk (include/dabgpu_pad_walk.h) and the slideshow walk (include/dabgpu_mot_walk.h) the GPU batch
// calls run, here on the host, the MOT walk's copy orders executed by a loop, and every completed image object handed
// to a Basic_Slideshow_Manager.  Basic_DAB_Channel reads its frames' PAD through it (the rows of
// include/dabgpu_mp2_frame.h are access units to it).
// TWO PLACES: Basic_DAB_Plus_Channel does the same with members of its own (basic_dab_plus_channel.cpp: WalkMot, AddSlide,
// MOT_BODY_CAPACITY, MOT_SLOTS), which tests/test_pad_slides.py holds to that file by its text.  A change to the mapping of
// a slot to a Basic_Slideshow, to the eviction or to the sizes goes into both until that channel is folded onto this reader.
#pragma once
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>
#include "basic_radio/basic_slideshow.h"
#include "dabgpu_mot_walk.h"
#include "dabgpu_pad_walk.h"

// one slot of the MOT walk (record, header, body) -> a Basic_Slideshow of the manager; images only (TS 101 499 clause 6.2)
inline void Basic_Add_Slide(Basic_Slideshow_Manager &manager, const uint8_t *slot) {
    int32_t rec[8];
    std::memcpy(rec, slot, sizeof rec);
    const uint8_t *header = slot + dabgpu_mot::RECORD_BYTES, *body = header + rec[3];
    dabgpu_mot::Header h;
    if (dabgpu_mot::parse_header(header, rec[3], h) != 0 || h.content_type != 2) return;
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
    auto lock = std::scoped_lock(manager.GetSlideshowsMutex());
    auto &all = manager.GetSlideshows();
    all.push_back(slide);
    manager.OnNewSlideshow().Notify(slide);
    while (all.size() > manager.GetMaxSize()) {                       // the oldest leaves
        auto oldest = all.front();
        manager.OnRemoveSlideshow().Notify(oldest);
        all.pop_front();
    }
}

class Basic_Pad_Reader {
public:
    Basic_Pad_Reader() {
        m_call.body_capacity = BODY_CAPACITY;
        m_call.max_slides = SLOTS;
        m_call.slide_stride = uint32_t(dabgpu_mot::RECORD_BYTES + dabgpu_mot::HEADER_CAP + BODY_CAPACITY);
        m_arena.resize(size_t(dabgpu_mot::arena_bytes(BODY_CAPACITY)));
        m_slides.resize(size_t(SLOTS) * m_call.slide_stride);
        dabgpu_mot::sanitize(m_mot, BODY_CAPACITY);
    }
    // one access unit without its CRC, or (nullptr, -1): a lost one
    void Walk(const uint8_t *au, int len, Basic_Slideshow_Manager &manager) {
        dabgpu_pad::walk_au(m_pad, m_pad_counts, au, len);
        dabgpu_mot::Orders orders;
        m_mot_counts.slides_written = 0;                               // the slots are this access unit's
        dabgpu_mot::walk_au(m_mot, m_mot_counts, orders, m_call, au, len);
        for (int i = 0; i < orders.n; i++) dabgpu_mot::execute(orders.o[i], orders, au, m_arena.data(), m_slides.data());
        for (int k = 0; k < m_mot_counts.slides_written; k++) Basic_Add_Slide(manager, m_slides.data() + size_t(k) * m_call.slide_stride);
    }
    const dabgpu_pad::Label &GetLabel() const { return m_pad.label; }
    const dabgpu_pad::Counters &GetPadCounters() const { return m_pad_counts; }
    const dabgpu_mot::Counters &GetMotCounters() const { return m_mot_counts; }

private:
    static constexpr int BODY_CAPACITY = 256 * 1024, SLOTS = 4;
    dabgpu_pad::State m_pad{};             // all zero: a fresh start
    dabgpu_pad::Counters m_pad_counts{};
    dabgpu_mot::State m_mot{};
    dabgpu_mot::Counters m_mot_counts{};
    dabgpu_mot::Call m_call{};
    std::vector<uint8_t> m_arena, m_slides;
};
