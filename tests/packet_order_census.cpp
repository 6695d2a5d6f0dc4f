// packet_order_census.cpp -- the copy orders include/dabgpu_packet_walk.h gives for a stream of logical frames, one line each,
// and what they leave (tests/test_packet_device_edges.py builds this with the host compiler under AddressSanitizer and UBSan
// and runs it as a child process; never on a GPU).
//
//   packet_order_census <stream file> <out file>
//
// The stream file, little-endian int32: S, address, fec, body_capacity, max_slides, slide_stride, n_cifs, then n_cifs x 24 S
// bytes.  One call from a fresh state over all frames, by the pieces walk_frame() is made of (resolve_chain, follow_packet,
// execute_order), so that every order can be printed and checked before it is executed:
//   "P k pos L udl orders"   a followed packet: frame, slot position, slots, useful data length, how many orders it left
//   "kind src dst len"       an order
// ORDER_PACKET must lie inside the packet's useful bytes and the group buffer; ORDER_MOVE and ORDER_SLIDE inside the arena and
// the slots, and an ORDER_MOVE must not overlap its source (wave_copy()'s precondition): status 3 or 4 otherwise.  Then
// walk_frames() runs over the same frames on buffers of its own: arena, slots, state and counters must be the same bytes
// (status 5 otherwise).  They go into the out file.  Every buffer is a 16-aligned heap block of exactly its size.
#include "dabgpu_packet_walk.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace mot = dabgpu_mot;
namespace pkt = dabgpu_packet;

static uint8_t *block(size_t n) {
    void *p = nullptr;
    if (posix_memalign(&p, 16, n ? n : 1)) std::exit(2);
    return static_cast<uint8_t *>(p);
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[7];
    if (std::fread(head, 4, 7, f) != 7) return 2;
    const int S = head[0], address = head[1], fec = head[2], n_cifs = head[6];
    mot::Call entry{};
    entry.body_capacity = head[3];
    entry.max_slides = head[4];
    entry.slide_stride = uint32_t(head[5]);
    if (S < 1 || S > pkt::MAX_SLOTS || address < 1 || address > 1023 || n_cifs < 0 || n_cifs > 4096 || entry.body_capacity < 0 ||
        entry.body_capacity > mot::BODY_CAP_MAX || entry.max_slides < 0 || entry.max_slides > 64 || entry.slide_stride % 16 ||
        entry.slide_stride > (1u << 20))
        return 2;
    const size_t fb = size_t(pkt::SLOT_BYTES) * size_t(S);
    uint8_t *frames = block(fb * size_t(n_cifs));
    if (std::fread(frames, 1, fb * size_t(n_cifs), f) != fb * size_t(n_cifs)) return 2;
    std::fclose(f);
    const size_t arena_size = size_t(mot::arena_bytes(entry.body_capacity)), slides_size = size_t(entry.max_slides) * entry.slide_stride;
    uint8_t *arena[2], *slides[2];
    pkt::State st[2];
    pkt::Counters c[2];
    for (int i = 0; i < 2; i++) {
        arena[i] = block(arena_size);
        slides[i] = block(slides_size);
        std::memset(arena[i], 0xA7, arena_size);
        std::memset(slides[i], 0xA7, slides_size);
        std::memset(&st[i], 0, sizeof st[i]);
        std::memset(&c[i], 0, sizeof c[i]);
        pkt::sanitize(st[i], entry.body_capacity);
    }
    mot::Orders ord;
    for (int k = 0; k < n_cifs; k++) {
        const uint8_t *frame = frames + fb * size_t(k);
        pkt::FrameTally t = {};
        mot::Call call = entry;
        call.superframe = k;
        pkt::resolve_chain(
            S, address, t, [&](int pos) { return pkt::slot_verdict(frame, S, pos, fec); },
            [&](int pos, int L) {
                const uint8_t *p = frame + pkt::SLOT_BYTES * pos;
                call.au = pos;
                pkt::follow_packet(st[0], c[0], ord, call, p, L);
                std::printf("P %d %d %d %d %d\n", k, pos, L, p[2] & 0x7F, ord.n);
                for (int i = 0; i < ord.n; i++) {
                    const mot::Order &o = ord.o[i];
                    std::printf("%d %d %u %d\n", o.kind, o.src, o.dst, o.len);
                    if (o.kind == pkt::ORDER_PACKET) {
                        if (o.len <= 0 || o.src != 3 || o.src + o.len > pkt::packet_read_bytes(L, p[2]) || size_t(o.dst) + size_t(o.len) > size_t(mot::GROUP_CAP))
                            std::exit(3);
                    } else if (o.kind == mot::ORDER_MOVE || o.kind == mot::ORDER_SLIDE) {
                        const bool move = o.kind == mot::ORDER_MOVE;
                        if (o.len <= 0 || o.src < 0 || size_t(o.src) + size_t(o.len) > arena_size || size_t(o.dst) + size_t(o.len) > (move ? arena_size : slides_size))
                            std::exit(3);
                        if (move && int64_t(o.src) < int64_t(o.dst) + o.len && int64_t(o.dst) < int64_t(o.src) + o.len) std::exit(4);
                    }
                    pkt::execute_order(o, ord, p, arena[0], slides[0]);
                }
            });
        c[0].cifs++;
        c[0].slots += S;
        c[0].packets_fec += t.fec;
        c[0].slots_bad += t.bad;
        c[0].packets_padding += t.padding;
        c[0].packets_other += t.other;
        c[0].packets_followed += t.followed;
    }
    pkt::walk_frames(st[1], c[1], entry, frames, fb, n_cifs, S, address, fec, arena[1], slides[1]);
    if (std::memcmp(arena[0], arena[1], arena_size) || std::memcmp(slides[0], slides[1], slides_size) || std::memcmp(&st[0], &st[1], sizeof st[0]) ||
        std::memcmp(&c[0], &c[1], sizeof c[0]))
        return 5;
    f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    std::fwrite(arena[0], 1, arena_size, f);
    std::fwrite(slides[0], 1, slides_size, f);
    std::fwrite(&st[0], 1, sizeof st[0], f);
    std::fwrite(&c[0], 1, sizeof c[0], f);
    std::fclose(f);
    for (int i = 0; i < 2; i++) {
        std::free(arena[i]);
        std::free(slides[i]);
    }
    std::free(frames);
    return 0;
}
