// dabgpu_packet_api.hip -- the C ABI of packet-mode MOT services (include/dabgpu.h, "Packet-mode MOT services" and "Packet-mode
// MOT directory carousels"): which components are packet mode (host, from FIBs), the two batch calls on device memory and
// their twins on host memory (no context, no GPU: the same code, include/dabgpu_packet_walk.h and
// include/dabgpu_mot_carousel.h, its orders executed by a loop), the directory parser.
#include "dabgpu_ctx.hpp"

#include <algorithm>
#include <cstring>

#include "../../include/dabgpu_mot_carousel.h"
#include "../../include/dabgpu_fig.h"

using namespace dabapi;
namespace mot = dabgpu_mot;
namespace pkt = dabgpu_packet;
namespace car = dabgpu_carousel;

static_assert(sizeof(dabgpu_packet_carousel_result) == sizeof(car::Counters) && sizeof(dabgpu_mot_carousel_object) == mot::RECORD_BYTES &&
                  sizeof(dabgpu_mot_directory) == sizeof(car::DirectoryInfo) &&
                  sizeof(dabgpu_mot_directory_object) == sizeof(car::DirectoryObject) && sizeof(dabgpu_packet_carousel_entry) == 112,
              "ABI structs mirror the carousel's");
static_assert(sizeof(dabgpu_packet_result) == sizeof(pkt::Counters) && sizeof(dabgpu_packet_component) == 48,
              "ABI structs mirror the walk's");

size_t dabgpu_packet_state_bytes(void) { return sizeof(pkt::State); }

int dabgpu_fig_packet_components(const uint8_t *fib, const uint8_t *crc_ok, int n_frames, dabgpu_packet_component *out, int max,
                                 int *n) {
    if (!fib || !crc_ok || !n || n_frames < 0 || max < 0 || (max > 0 && !out)) return DABGPU_ERR_ARG;
    return dabgpu_fig::packet_components(fib, crc_ok, n_frames, out, max, n);
}

// everything both calls refuse, before anything is done; fills the kernels' table when there is one
static int packet_check(const dabgpu_packet_entry *entries, int n_entries, int n_cifs, dabk::PacketEntry *table) {
    if (n_entries < 0 || n_cifs < 0 || n_cifs > pkt::MAX_N_CIFS || (n_entries > 0 && !entries)) return DABGPU_ERR_ARG;
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
        if (e.d_state_in && overlaps(e.d_state_in, sb, e.d_state_out, sb)) return DABGPU_ERR_ARG;
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
    const size_t table_bytes = dabk::packet_table_bytes(table.data(), n_entries, n_cifs, false);
    return launch_entry_table(ctx, STAGE_PACKET, table_bytes, stream, [&](void *d_table, size_t slot_bytes, hipStream_t s) {
        return dabk::launch_packet_walk(table.data(), nullptr, n_entries, n_cifs, d_table, slot_bytes, s);
    });
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

// ---- MOT directory carousels ----------------------------------------------------------------------------------------
size_t dabgpu_packet_carousel_state_bytes(void) { return sizeof(car::State); }

size_t dabgpu_packet_carousel_arena_bytes(int directory_capacity, int assemblies, int object_capacity) {
    return car::sizes_ok(directory_capacity, assemblies, object_capacity) ? size_t(car::arena_bytes(directory_capacity, assemblies, object_capacity)) : 0;
}

// the entry as the slides call would see it: the shared fields are refused by the same code, word for word
static dabgpu_packet_entry as_packet_entry(const dabgpu_packet_carousel_entry &e) {
    dabgpu_packet_entry p{};
    p.d_in = e.d_in;
    p.in_stride = e.in_stride;
    p.bitrate_kbps = e.bitrate_kbps;
    p.address = e.address;
    p.fec = e.fec;
    p.d_state_in = e.d_state_in;
    p.d_state_out = e.d_state_out;
    p.d_arena = e.d_arena;
    // (the arena's size has its own rule here: the slides call's smallest arena is not this call's)
    p.arena_bytes = std::max<size_t>(e.arena_bytes, size_t(mot::arena_bytes(0)));
    p.d_slides = e.d_objects;
    p.slide_stride = e.object_stride;
    p.max_slides = e.max_objects;
    p.d_result = reinterpret_cast<dabgpu_packet_result *>(e.d_result);
    return p;
}

// everything both carousel calls refuse, before anything is done; fills the kernels' tables when there are any
static int carousel_check(const dabgpu_packet_carousel_entry *entries, int n_entries, int n_cifs, dabk::PacketEntry *table,
                          dabk::CarouselExtra *extras) {
    if (n_entries < 0 || n_cifs < 0 || n_cifs > pkt::MAX_N_CIFS || (n_entries > 0 && !entries)) return DABGPU_ERR_ARG;
    const uint64_t sb = sizeof(car::State);
    for (int i = 0; i < n_entries; i++) {
        const dabgpu_packet_carousel_entry &e = entries[i];
        const dabgpu_packet_entry p = as_packet_entry(e);
        const int bad = packet_check(&p, 1, n_cifs, table ? table + i : nullptr);
        if (bad) return bad;
        // (packet_check has held the two state records apart by the slides call's smaller record)
        if (e.d_state_in && overlaps(e.d_state_in, sb, e.d_state_out, sb)) return DABGPU_ERR_ARG;
        if (!car::sizes_ok(e.directory_capacity, e.assemblies, e.object_capacity)) return DABGPU_ERR_ARG;
        if (e.arena_bytes < car::arena_bytes(e.directory_capacity, e.assemblies, e.object_capacity)) return DABGPU_ERR_ARG;
        if (!e.d_directory || (addr(e.d_directory) & 15)) return DABGPU_ERR_ARG;
        if (!table) continue;
        table[i].body_capacity = e.object_capacity;
        // (compared as the entry gives it also when there is no slot; held below 2^31)
        table[i].slide_stride = uint32_t(std::min<uint64_t>(e.object_stride, 0x7FFFFFFFu));
        extras[i].directory = addr(e.d_directory);
        extras[i].directory_capacity = e.directory_capacity;
        extras[i].assemblies = e.assemblies;
    }
    return DABGPU_OK;
}

int dabgpu_packet_carousel_dev(dabgpu_ctx *ctx, const dabgpu_packet_carousel_entry *entries, int n_entries, int n_cifs, void *stream) {
    if (!ctx) return DABGPU_ERR_ARG;
    // everything is checked before anything is enqueued: a refused call leaves every output as it was
    const size_t n = size_t(n_entries > 0 ? n_entries : 0);
    std::vector<dabk::PacketEntry> table(n, dabk::PacketEntry{});
    std::vector<dabk::CarouselExtra> extras(n, dabk::CarouselExtra{});
    const int bad = carousel_check(entries, n_entries, n_cifs, table.data(), extras.data());
    if (bad) return bad;
    if (n_entries == 0) return DABGPU_OK;
    if (dabk::packet_scan_blocks(table.data(), n_entries, n_cifs) >= (uint64_t(1) << 31)) return DABGPU_ERR_CAPACITY;
    const size_t table_bytes = dabk::packet_table_bytes(table.data(), n_entries, n_cifs, true);
    return launch_entry_table(ctx, STAGE_PACKET_CAROUSEL, table_bytes, stream, [&](void *d_table, size_t slot_bytes, hipStream_t s) {
        return dabk::launch_packet_walk(table.data(), extras.data(), n_entries, n_cifs, d_table, slot_bytes, s);
    });
}

int dabgpu_packet_carousel_host(const dabgpu_packet_carousel_entry *entries, int n_entries, int n_cifs) {
    const int bad = carousel_check(entries, n_entries, n_cifs, nullptr, nullptr);
    if (bad) return bad;
    for (int i = 0; i < n_entries; i++) {
        const dabgpu_packet_carousel_entry &e = entries[i];
        car::Call call{};
        call.directory_capacity = e.directory_capacity;
        call.assemblies = e.assemblies;
        call.object_capacity = e.object_capacity;
        call.max_objects = e.max_objects;
        call.object_stride = uint32_t(std::min<uint64_t>(e.object_stride, 0x7FFFFFFFu));
        car::State st;
        if (e.d_state_in) std::memcpy(&st, e.d_state_in, sizeof st);
        else std::memset(&st, 0, sizeof st);
        car::sanitize(st, e.directory_capacity, e.assemblies, e.object_capacity);
        car::Counters c{};
        car::walk_frames(st, c, call, e.d_in, e.in_stride, n_cifs, e.bitrate_kbps / 8, e.address, e.fec != 0,
                         static_cast<uint8_t *>(e.d_arena), e.d_directory, e.d_objects);
        std::memcpy(e.d_state_out, &st, sizeof st);
        std::memcpy(e.d_result, &c, sizeof c);
    }
    return DABGPU_OK;
}

int dabgpu_mot_directory_parse(const uint8_t *dir, int n, dabgpu_mot_directory *info, dabgpu_mot_directory_object *out, int max,
                               int *n_out) {
    if (!dir || !info || !n_out || n < 0 || max < 0 || (max > 0 && !out)) return DABGPU_ERR_ARG;
    car::DirectoryInfo r;
    const int rc = car::parse_directory(dir, n, r, reinterpret_cast<car::DirectoryObject *>(out), max, n_out);
    if (rc) return rc == -2 ? DABGPU_ERR_CAPACITY : DABGPU_ERR_ARG;
    std::memcpy(info, &r, sizeof r);
    return DABGPU_OK;
}
