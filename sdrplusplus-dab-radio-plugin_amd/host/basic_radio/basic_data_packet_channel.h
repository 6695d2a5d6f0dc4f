// basic_radio/basic_data_packet_channel.h -- what BasicRadio::Get_Data_Packet_Channel returns
// (the reference's src/render_radio_block.cpp:533, 538-540, 592-593): a packet-mode sub-channel (TMId 3) whose MOT
// components are followed to their slides.  Process takes the sub-channel's logical frames; the scan and the walk are
// include/dabgpu_packet_walk.h, the code the GPU batch call dabgpu_packet_slides_dev runs, here on the host with its copy
// orders executed by a loop (no export of libdabgpu is called); every completed image object goes to the one slideshow
// manager, through Basic_Add_Slide as an audio channel's do.  Up to four packet addresses (DSCTy 60, DG flag 0) of the
// sub-channel are followed, each with a state record and an arena of its own.  FEC packets are counted; with
// SetFecCorrection(true) -- BasicRadio switches it on when FIG 0/14 gives the sub-channel FEC scheme 1 -- every logical frame
// first goes through the host path of include/dabgpu_packet_fec.h, the code dabgpu_packet_fec_dev runs: the FEC frames are
// corrected by RS(204,188) and the walk sees the stream delayed by ceil(102 / S) frames (padding packets at first).  With FEC
// scheme 1 that path is include/dabgpu_packet_fec_erasures.h's, the code dabgpu_packet_fec_erasures_dev runs: the packets whose
// CRC fails are erasures, so eight lost packets per FEC frame are recovered instead of four.
//
// Beside that walk, on the same followed packets, runs the control of include/dabgpu_mot_carousel.h, the code
// dabgpu_packet_carousel_dev runs: a component that speaks MOT directory mode (a directory in data groups of type 6, then
// bodies alone) yields its current directory and its objects here (GetDirectory, GetCarouselObjects), while the header-mode
// walk counts its groups as ignored; one that speaks header mode yields slides as before, and the carousel control counts
// groups_header_mode.  The two share nothing but the frame's scan: the walk, its counters and its slides are untouched.
//
// Components that are not MOT in data groups (DSCTy other than 60, or DG flag 1: TPEG, SPI, Journaline, transparent data
// channels) are followed by FollowDataGroups: every logical frame goes through the serial walk of
// include/dabgpu_data_groups.h, the code dabgpu_packet_groups_dev and dabgpu_packet_groups_host run, one frame a call with the
// state record handed on; every data group it emits goes to OnDataGroup (its record and its bytes), the raw bytes of a
// component without data groups to OnRawData with a record for every continuity break (where in them bytes are missing), the counters add up (GetDataGroupCounters).  MOT components go where they went.
#pragma once
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>
#include "basic_radio/basic_pad_reader.h"
#include "basic_radio/basic_slideshow.h"
#include "dab/database/dab_database_entities.h"
#include "dabgpu_packet_fec.h"
#include "dabgpu_packet_fec_erasures.h"
#include "dabgpu_mot_carousel.h"
#include "dabgpu_data_groups.h"
#include "dabgpu_packet_walk.h"
#include "utility/observable.h"
#include "utility/span.h"

class Basic_Data_Packet_Channel {
public:
    static constexpr int MAX_ADDRESSES = 4;
    explicit Basic_Data_Packet_Channel(const Subchannel &subchannel, int fec_scheme = 0) : m_subchannel(subchannel), m_fec(fec_scheme) {
        m_call.body_capacity = BODY_CAPACITY;
        m_call.max_slides = 1;                                         // (a packet closes at most one group: one object)
        m_call.slide_stride = uint32_t(dabgpu_mot::RECORD_BYTES + dabgpu_mot::HEADER_CAP + BODY_CAPACITY);
    }
    Basic_Slideshow_Manager &GetSlideshowManager() { return m_slideshows; }
    const Subchannel &GetSubchannel() const { return m_subchannel; }
    void SetFecScheme(int fec_scheme) { m_fec = fec_scheme; }
    int GetFecScheme() const { return m_fec; }
    // RS(204,188) correction in front of the walk, from the next frame on; switching it starts the FEC stream afresh
    void SetFecCorrection(bool on) {
        if (on != m_correct) m_fec_slots = 0;
        m_correct = on;
    }
    bool GetFecCorrection() const { return m_correct; }
    // counts since the correction was switched on (cifs, slots, marks, frames, rows_*, bytes_corrected ...)
    const dabgpu_packet_fec::Counters &GetFecCounters() const { return m_fec_counts.c; }
    // the same and what the erasure path adds (slots_suspect, rows_erasure_corrected ...; zero without FEC scheme 1)
    const dabgpu_packet_fec::ErasureCounters &GetFecErasureCounters() const { return m_fec_counts; }

    // a packet address (1 .. 1023) to follow from the next frame on: false for one out of range, and for a fifth
    bool FollowAddress(int address) {
        if (address < 1 || address > 1023) return false;
        for (const auto &f : m_followers)
            if (f->address == address) return true;
        if (int(m_followers.size()) >= MAX_ADDRESSES) return false;
        auto f = std::make_unique<Follower>();
        f->address = address;
        f->arena.resize(size_t(dabgpu_mot::arena_bytes(BODY_CAPACITY)));
        dabgpu_packet::sanitize(f->state, BODY_CAPACITY);
        f->carousel = std::make_unique<Carousel>();
        m_followers.push_back(std::move(f));
        if (m_slot.empty()) m_slot.resize(m_call.slide_stride);
        return true;
    }
    int GetTotalAddresses() const { return int(m_followers.size()); }
    int GetAddress(int i) const { return m_followers[size_t(i)]->address; }
    // counts since the address was added (slides_written: of the last packet alone)
    const dabgpu_packet::Counters &GetCounters(int i) const { return m_followers[size_t(i)]->counts; }
    // directory mode: counts since the address was added (objects_written: of the last packet alone; directory_*: of the
    // current directory), the current directory's bytes (empty: none; dabgpu_mot::parse_header reads a listed header) and
    // the objects delivered so far
    struct Carousel_Object {
        dabgpu_carousel::DirectoryObject entry;                        // header_offset: not kept (the header is here)
        int directory_id;
        std::vector<uint8_t> header, body;
    };
    const dabgpu_carousel::Counters &GetCarouselCounters(int i) const { return m_followers[size_t(i)]->carousel->counts; }
    tcb::span<const uint8_t> GetDirectory(int i) const {
        const Carousel &k = *m_followers[size_t(i)]->carousel;
        return {k.directory.data(), k.state.cur_valid ? size_t(k.state.cur_bytes) : size_t(0)};
    }
    const std::vector<Carousel_Object> &GetCarouselObjects(int i) const { return m_followers[size_t(i)]->carousel->objects; }
    // a packet address whose data groups (mode 0) or raw useful bytes (mode 1: the component's DG flag) are handed out as
    // they are, from the next frame on: false for an address or mode out of range, and for a fifth
    bool FollowDataGroups(int address, int mode, bool keep_repeats = false) {
        if (address < 1 || address > 1023 || mode < 0 || mode > 1) return false;
        for (const auto &f : m_data_followers)
            if (f->address == address) return f->call.mode == mode;
        if (int(m_data_followers.size()) >= MAX_ADDRESSES) return false;
        auto f = std::make_unique<DataFollower>();
        f->address = address;
        f->call.mode = mode;
        f->call.keep_repeats = keep_repeats;
        // (one frame a call: at most 64 packets close a group or break, one group of up to 16384 bytes among them)
        f->call.max_groups = dabgpu_packet::MAX_SLOTS;
        f->call.bytes_capacity = dabgpu_groups::GROUP_CAP + dabgpu_packet::MAX_SLOTS * 96;
        f->bytes.resize(size_t(f->call.bytes_capacity));
        f->records.resize(size_t(f->call.max_groups));
        f->call.bytes = f->bytes.data();
        f->call.groups = f->records.data();
        for (auto &st : f->state) st = std::make_unique<dabgpu_groups::State>();   // all zero: a fresh start
        m_data_followers.push_back(std::move(f));
        return true;
    }
    int GetTotalDataAddresses() const { return int(m_data_followers.size()); }
    int GetDataAddress(int i) const { return m_data_followers[size_t(i)]->address; }
    int GetDataMode(int i) const { return m_data_followers[size_t(i)]->call.mode; }
    // counts since the address was added
    const dabgpu_groups::Counters &GetDataGroupCounters(int i) const { return m_data_followers[size_t(i)]->counts; }
    // (packet address, the group's record -- cif counts the channel's frames, offset is 0 --, the whole group)
    auto &OnDataGroup() { return m_obs_data_group; }
    // (packet address, the useful bytes one frame added to the stream, one record per continuity break of that frame: flags
    // DABGPU_DG_BREAK, offset = where in these bytes bytes are missing in front, cif = the channel's frame count, slot)
    auto &OnRawData() { return m_obs_raw_data; }
    int GetTotalFrames() const { return m_total_frames; }
    int GetTotalFramesIgnored() const { return m_total_ignored; }

    // one logical frame of the sub-channel: 24 S bytes, S = bit rate / 8 in 1 .. 64 (any other size is counted and ignored)
    void Process(tcb::span<const uint8_t> lf) {
        namespace pkt = dabgpu_packet;
        const int S = int(lf.size() / pkt::SLOT_BYTES);
        if (lf.size() % pkt::SLOT_BYTES || S < 1 || S > pkt::MAX_SLOTS) {
            m_total_ignored++;
            return;
        }
        const uint8_t *frame = m_correct ? Correct(lf.data(), S) : lf.data();
        uint32_t verdicts[pkt::MAX_SLOTS];                             // one scan for every address
        for (int pos = 0; pos < S; pos++) verdicts[pos] = pkt::slot_verdict(frame, S, pos, m_fec);
        dabgpu_mot::Orders orders;
        dabgpu_mot::Call call = m_call;
        call.superframe = m_total_frames;
        for (auto &f : m_followers) {
            pkt::FrameTally t = {};
            pkt::Counters &c = f->counts;
            pkt::resolve_chain(
                S, f->address, t, [&](int pos) { return verdicts[pos]; },
                [&](int pos, int L) {
                    const uint8_t *packet = frame + pkt::SLOT_BYTES * pos;
                    call.au = pos;
                    c.mot.slides_written = 0;                          // the slot is this packet's
                    pkt::follow_packet(f->state, c, orders, call, packet, L);
                    for (int i = 0; i < orders.n; i++) pkt::execute_order(orders.o[i], orders, packet, f->arena.data(), m_slot.data());
                    if (c.mot.slides_written) Basic_Add_Slide(m_slideshows, m_slot.data());
                    f->carousel->Follow(packet, L, m_total_frames, pos);
                });
            for (pkt::Counters *k : {&c, &f->carousel->counts.head}) {   // (one scan: the same tally for both)
                k->cifs++;
                k->slots += S;
                k->packets_fec += t.fec;
                k->slots_bad += t.bad;
                k->packets_padding += t.padding;
                k->packets_other += t.other;
                k->packets_followed += t.followed;
            }
        }
        for (auto &f : m_data_followers) FollowData(*f, frame, S);
        m_total_frames++;
    }

private:
    struct DataFollower {
        int address = 0;
        dabgpu_groups::Call call{};
        dabgpu_groups::Counters counts{};
        std::unique_ptr<dabgpu_groups::State> state[2];
        int turn = 0;
        std::vector<uint8_t> bytes;
        std::vector<dabgpu_groups::Record> records;
    };
    // one logical frame of one address through dabgpu_groups::walk_frames, as a call of one frame
    void FollowData(DataFollower &f, const uint8_t *frame, int S) {
        namespace dg = dabgpu_groups;
        dg::Counters c{};
        dg::walk_frames(f.state[f.turn].get(), f.state[f.turn ^ 1].get(), c, f.call, frame, uint64_t(dabgpu_packet::SLOT_BYTES) * uint64_t(S), 1, S,
                        f.address, m_fec);
        f.turn ^= 1;
        int32_t *sum = reinterpret_cast<int32_t *>(&f.counts);
        for (size_t i = 0; i < sizeof c / sizeof(int32_t); i++) sum[i] += reinterpret_cast<const int32_t *>(&c)[i];
        if (f.call.mode) {
            if (c.bytes_emitted || c.groups_emitted)
            {
                for (int i = 0; i < c.groups_emitted; i++) f.records[size_t(i)].cif = m_total_frames;
                m_obs_raw_data.Notify(f.address, tcb::span<const uint8_t>(f.bytes.data(), size_t(c.bytes_emitted)),
                                      tcb::span<const dabgpu_groups::Record>(f.records.data(), size_t(c.groups_emitted)));
            }
            return;
        }
        for (int i = 0; i < c.groups_emitted; i++) {
            dg::Record r = f.records[size_t(i)];
            const uint8_t *g = f.bytes.data() + r.offset;
            r.cif = m_total_frames;
            r.offset = 0;
            m_obs_data_group.Notify(f.address, r, tcb::span<const uint8_t>(g, size_t(r.length)));
        }
    }

    // one logical frame through dabgpu_packet_fec::process_erasures (FEC scheme 1) or process: -> the frame D frames back,
    // corrected.  The two keep state records of their own kind: a change of scheme starts the FEC stream afresh
    const uint8_t *Correct(const uint8_t *lf, int S) {
        namespace fec = dabgpu_packet_fec;
        static const fec::Gf gf = fec::make_gf();
        const size_t nb = size_t(fec::state_bytes(S)), fb = size_t(fec::SLOT_BYTES) * size_t(S);
        const bool fresh = m_fec_slots != S;
        if (fresh) {                                                   // (the first frame, or a frame of another size)
            m_fec_slots = S;
            m_fec_turn = 0;
            m_fec_counts = fec::ErasureCounters{};
            for (auto &st : m_fec_state) st.assign(nb, 0);
            m_fec_out.assign(fb, 0);
        }
        fec::ErasureCounters c{};
        const uint8_t *state_in = fresh ? nullptr : m_fec_state[m_fec_turn].data();
        uint8_t *state_out = m_fec_state[m_fec_turn ^ 1].data();
        if (m_fec == 1)
            fec::process_erasures(gf, state_in, state_out, c, lf, fb, 1, S, m_fec_out.data(), fb);
        else
            fec::process(gf, state_in, state_out, c.c, lf, fb, 1, S, m_fec_out.data(), fb);
        m_fec_turn ^= 1;
        int32_t *sum = reinterpret_cast<int32_t *>(&m_fec_counts);
        for (size_t i = 0; i < sizeof c / sizeof(int32_t); i++) sum[i] += reinterpret_cast<const int32_t *>(&c)[i];
        return m_fec_out.data();
    }

    static constexpr int BODY_CAPACITY = 256 * 1024;
    // the directory-mode control of one address: a state record, an arena, the directory buffer and one slot of its own
    struct Carousel {
        static constexpr int DIRECTORY_CAPACITY = 64 * 1024, ASSEMBLIES = 8;
        dabgpu_carousel::State state{};    // all zero: a fresh start
        dabgpu_carousel::Counters counts{};
        dabgpu_carousel::Call call{};
        std::vector<uint8_t> arena, directory, slot;
        std::vector<Carousel_Object> objects;
        Carousel() {
            namespace car = dabgpu_carousel;
            call.directory_capacity = DIRECTORY_CAPACITY;
            call.assemblies = ASSEMBLIES;
            call.object_capacity = BODY_CAPACITY;
            call.max_objects = 1;                                      // (one emission attempt a packet: one object)
            call.object_stride = uint32_t(dabgpu_mot::RECORD_BYTES + dabgpu_mot::SEGMENT_MAX + BODY_CAPACITY);
            arena.resize(size_t(car::arena_bytes(DIRECTORY_CAPACITY, ASSEMBLIES, BODY_CAPACITY)));
            directory.resize(DIRECTORY_CAPACITY);
            slot.resize(call.object_stride);
            car::sanitize(state, DIRECTORY_CAPACITY, ASSEMBLIES, BODY_CAPACITY);
        }
        void Follow(const uint8_t *packet, int L, int frame, int pos) {
            namespace car = dabgpu_carousel;
            call.frame = frame;
            call.slot = pos;
            call.deferred = 0;
            counts.objects_written = 0;                                // the slot is this packet's
            car::walk_packet(state, counts, call, packet, L, arena.data(), directory.data(), slot.data());
            car::finish(state, counts);
            if (!counts.objects_written) return;
            int32_t rec[8];
            std::memcpy(rec, slot.data(), sizeof rec);
            Carousel_Object o;
            o.entry = car::DirectoryObject{rec[0], 0, rec[3], rec[4], rec[1], rec[2], {0, 0}};
            o.directory_id = rec[7];
            const uint8_t *h = slot.data() + dabgpu_mot::RECORD_BYTES;
            o.header.assign(h, h + rec[3]);
            o.body.assign(h + rec[3], h + rec[3] + rec[4]);
            objects.push_back(std::move(o));
        }
    };
    struct Follower {
        int address = 0;
        dabgpu_packet::State state{};      // all zero: a fresh start
        dabgpu_packet::Counters counts{};
        std::vector<uint8_t> arena;
        std::unique_ptr<Carousel> carousel;
    };
    Subchannel m_subchannel;
    int m_fec;
    dabgpu_mot::Call m_call{};
    std::vector<std::unique_ptr<Follower>> m_followers;
    std::vector<std::unique_ptr<DataFollower>> m_data_followers;
    Observable<int, const dabgpu_groups::Record &, tcb::span<const uint8_t>> m_obs_data_group;
    Observable<int, tcb::span<const uint8_t>, tcb::span<const dabgpu_groups::Record>> m_obs_raw_data;
    std::vector<uint8_t> m_slot;
    Basic_Slideshow_Manager m_slideshows;
    int m_total_frames = 0, m_total_ignored = 0;
    bool m_correct = false;
    int m_fec_slots = 0, m_fec_turn = 0;   // S the FEC state is for (0: none yet); which of the two records is current
    std::vector<uint8_t> m_fec_state[2], m_fec_out;
    dabgpu_packet_fec::ErasureCounters m_fec_counts{};
};
