// dabgpu_mot_api.hip -- the C ABI of the slideshow (include/dabgpu.h, "Slideshow"): the batch call on device memory, its
// twin on host memory (no context, no GPU: the same control walk, include/dabgpu_mot_walk.h, its orders executed by a
// loop) and the MOT header parser.
#include "dabgpu_ctx.hpp"

#include <cstring>

#include "../../include/dabgpu_mot_walk.h"

using namespace dabapi;
namespace mot = dabgpu_mot;

static_assert(sizeof(dabgpu_mot_result) == sizeof(mot::Counters) && sizeof(dabgpu_mot_slide) == mot::RECORD_BYTES &&
                  sizeof(dabgpu_mot_header) == sizeof(mot::Header) && sizeof(dabgpu_mot_text) == sizeof(mot::Text),
              "ABI structs mirror the walk's");
static_assert(sizeof(dabgpu_superframe_status) == 64, "the walk reads status rows as 16 words");

size_t dabgpu_mot_state_bytes(void) { return sizeof(mot::State); }
size_t dabgpu_mot_arena_bytes(size_t body_capacity) {
    return body_capacity > size_t(mot::BODY_CAP_MAX) ? 0 : size_t(mot::arena_bytes(int64_t(body_capacity)));
}

// everything both calls refuse, before anything is done; fills the kernel's table when there is one
static int mot_check(const dabgpu_mot_entry *entries, int n_entries, dabk::MotEntry *table) {
    if (n_entries < 0 || (n_entries > 0 && !entries)) return DABGPU_ERR_ARG;
    const uint64_t sb = sizeof(mot::State);
    for (int i = 0; i < n_entries; i++) {
        const dabgpu_mot_entry &e = entries[i];
        if (e.bitrate_kbps < 8 || e.bitrate_kbps > 512 || e.bitrate_kbps % 8) return DABGPU_ERR_ARG;
        const int s = e.bitrate_kbps / 8;
        if (e.max_superframes < 0 || e.data_stride < size_t(110) * s) return DABGPU_ERR_ARG;
        if (!e.d_data || !e.d_status || !e.d_follow || !e.d_state_out || !e.d_arena || !e.d_result) return DABGPU_ERR_ARG;
        if ((addr(e.d_state_in) | addr(e.d_state_out) | addr(e.d_arena) | addr(e.d_slides)) & 15) return DABGPU_ERR_ARG;
        if ((addr(e.d_status) | addr(e.d_follow) | addr(e.d_result)) & 3) return DABGPU_ERR_ARG;
        if (e.d_state_in && overlaps(e.d_state_in, sb, e.d_state_out, sb)) return DABGPU_ERR_ARG;
        if (e.arena_bytes < mot::arena_bytes(0) || e.max_slides < 0) return DABGPU_ERR_ARG;
        if (e.max_slides > 0 && (!e.d_slides || e.slide_stride < size_t(mot::RECORD_BYTES) || e.slide_stride % 16 ||
                                 e.slide_stride >= (uint64_t(1) << 31) || uint64_t(e.max_slides) * e.slide_stride >= (uint64_t(1) << 31)))
            return DABGPU_ERR_ARG;
        if (!table) continue;
        dabk::MotEntry &t = table[i];
        t.data = addr(e.d_data);
        t.data_stride = e.data_stride;
        t.status = addr(e.d_status);
        t.follow = addr(e.d_follow);
        t.state_in = addr(e.d_state_in);
        t.state_out = addr(e.d_state_out);
        t.arena = addr(e.d_arena);
        t.slides = addr(e.d_slides);
        t.result = addr(e.d_result);
        t.slide_stride = e.max_slides > 0 ? uint32_t(e.slide_stride) : 0;
        t.max_slides = e.max_slides;
        t.body_capacity = mot::body_capacity_of(e.arena_bytes);
        t.s = s;
        t.max_superframes = e.max_superframes;
    }
    return DABGPU_OK;
}

int dabgpu_mot_slides_dev(dabgpu_ctx *ctx, const dabgpu_mot_entry *entries, int n_entries, void *stream) {
    if (!ctx) return DABGPU_ERR_ARG;
    // everything is checked before anything is enqueued: a refused call leaves every output as it was
    std::vector<dabk::MotEntry> table(size_t(n_entries > 0 ? n_entries : 0), dabk::MotEntry{});
    const int bad = mot_check(entries, n_entries, table.data());
    if (bad) return bad;
    if (n_entries == 0) return DABGPU_OK;
    const size_t table_bytes = table.size() * sizeof(dabk::MotEntry);
    return launch_entry_table(ctx, STAGE_MOT, table_bytes, stream, [&](void *d_table, size_t slot_bytes, hipStream_t s) {
        return dabk::launch_mot_slides(table.data(), n_entries, d_table, slot_bytes, s);
    });
}

int dabgpu_mot_slides_host(const dabgpu_mot_entry *entries, int n_entries) {
    const int bad = mot_check(entries, n_entries, nullptr);
    if (bad) return bad;
    for (int i = 0; i < n_entries; i++) {
        const dabgpu_mot_entry &e = entries[i];
        mot::Call call{};
        call.body_capacity = mot::body_capacity_of(e.arena_bytes);
        call.max_slides = e.max_slides;
        call.slide_stride = e.max_slides > 0 ? uint32_t(e.slide_stride) : 0;
        mot::State st;
        if (e.d_state_in) std::memcpy(&st, e.d_state_in, sizeof st);
        else std::memset(&st, 0, sizeof st);
        mot::sanitize(st, call.body_capacity);
        mot::Counters c{};
        int n_sf = e.d_follow->n_superframes;
        n_sf = n_sf < 0 ? 0 : n_sf > e.max_superframes ? e.max_superframes : n_sf;
        mot::walk_superframes(st, c, call, e.d_data, e.data_stride, reinterpret_cast<const int32_t *>(e.d_status), n_sf,
                              e.bitrate_kbps / 8, static_cast<uint8_t *>(e.d_arena), e.d_slides);
        std::memcpy(e.d_state_out, &st, sizeof st);
        std::memcpy(e.d_result, &c, sizeof c);
    }
    return DABGPU_OK;
}

int dabgpu_mot_header_parse(const uint8_t *header, int n, dabgpu_mot_header *out) {
    if (!header || !out) return DABGPU_ERR_ARG;
    mot::Header h;
    const int rc = mot::parse_header(header, n, h);
    if (rc) return rc == -2 ? DABGPU_ERR_CAPACITY : DABGPU_ERR_ARG;
    std::memcpy(out, &h, sizeof h);
    return DABGPU_OK;
}
