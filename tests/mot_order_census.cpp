// mot_order_census.cpp -- the copy orders include/dabgpu_mot_walk.h gives for a stream, one line each, and what they leave
// (tests/test_pad_slides_device.py builds this with the host compiler and runs it as a child process; never on a GPU).
//
//   mot_order_census <stream file> <out file>
//
// The stream file, little-endian int32: s, body_capacity, max_slides, slide_stride, rows, then rows x 110 s data bytes, then
// rows x 16 status words.  One call from a fresh state over all rows.  Every order is printed as "kind src dst len"; the
// arena and the slots, as the orders leave them, go into the out file.  Arena and slots are 16-aligned heap blocks of exactly
// their size, as the ABI asks of its callers.
//
// -DEMULATE: ORDER_MOVE and ORDER_SLIDE are executed as the kernel executes them, by csrc/wave_copy.hpp called for lane
// 0 .. 63 in turn, instead of mot::execute().  Before the copy proper each lane runs against a destination that holds no
// byte of the source, and what it wrote is counted: a byte that no lane or more than one lane writes ends the program with
// status 6.  -DMUTANT=k (with EMULATE): wave_copy_mutant.hpp (tests/wave_copy_mutants.py) in the header's place.
#include "dabgpu_mot_walk.h"

#if defined(EMULATE)
#if defined(MUTANT) && MUTANT
#include "wave_copy_mutant.hpp"
#if WAVE_COPY_MUTANT != MUTANT
#error "wave_copy_mutant.hpp is another mutant's"
#endif
#else
#include "wave_copy.hpp"
#endif
#endif

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace mot = dabgpu_mot;
namespace pad = dabgpu_pad;

static uint8_t *block(size_t n) {
    void *p = nullptr;
    if (posix_memalign(&p, 16, n ? n : 1)) std::exit(2);
    return static_cast<uint8_t *>(p);
}

#if defined(EMULATE)
static void wave(uint8_t *dst, const uint8_t *src, int len) {
    std::vector<uint8_t> before(dst, dst + len);
    std::vector<int> writers(size_t(len), 0);
    for (int i = 0; i < len; i++) dst[i] = uint8_t(~src[i]);
    for (int lane = 0; lane < 64; lane++) {
        dabk::wave_copy(dst, src, len, lane);
        for (int i = 0; i < len; i++)
            if (dst[i] == src[i]) {
                writers[size_t(i)]++;
                dst[i] = uint8_t(~src[i]);
            }
    }
    for (int i = 0; i < len; i++)
        if (writers[size_t(i)] != 1) {
            std::printf("LANES: byte %d of a copy of %d written by %d lanes\n", i, len, writers[size_t(i)]);
            std::exit(6);
        }
    std::memcpy(dst, before.data(), size_t(len));
    for (int lane = 0; lane < 64; lane++) dabk::wave_copy(dst, src, len, lane);
}
#endif

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[5];
    if (std::fread(head, 4, 5, f) != 5) return 2;
    const int s = head[0], rows = head[4];
    mot::Call call{};
    call.body_capacity = head[1];
    call.max_slides = head[2];
    call.slide_stride = uint32_t(head[3]);
    if (s < 1 || s > 64 || rows < 0 || rows > 4096 || call.body_capacity < 0 || call.body_capacity > mot::BODY_CAP_MAX || call.max_slides < 0 ||
        call.max_slides > 64 || call.slide_stride % 16 || call.slide_stride > (1u << 20))
        return 2;
    std::vector<uint8_t> data(size_t(rows) * 110 * size_t(s));
    std::vector<int32_t> status(size_t(rows) * 16);
    if (std::fread(data.data(), 1, data.size(), f) != data.size() || std::fread(status.data(), 4, status.size(), f) != status.size()) return 2;
    std::fclose(f);
    const size_t arena_size = size_t(mot::arena_bytes(call.body_capacity)), slides_size = size_t(call.max_slides) * call.slide_stride;
    uint8_t *arena = block(arena_size), *slides = block(slides_size);
    std::memset(arena, 0xA7, arena_size);
    std::memset(slides, 0xA7, slides_size);
    mot::State st;
    std::memset(&st, 0, sizeof st);
    mot::sanitize(st, call.body_capacity);
    mot::Counters c{};
    mot::Orders ord;
    for (int k = 0; k < rows; k++) {
        const int32_t *row = status.data() + 16 * size_t(k);
        const int n = pad::visited_aus(row[0], row[3]);
        for (int a = 0; a < n; a++) {
            int b = 0;
            const int len = pad::au_span(row[0], row[3], row[4], row[5 + a], row[6 + a], a, s, &b);
            const uint8_t *au = data.data() + size_t(k) * 110 * size_t(s) + (len < 0 ? 0 : b);
            call.superframe = k;
            call.au = a;
            mot::walk_au(st, c, ord, call, au, len);
            for (int i = 0; i < ord.n; i++) {
                const mot::Order &o = ord.o[i];
                std::printf("%d %d %u %d\n", o.kind, o.src, o.dst, o.len);
                if (o.kind == mot::ORDER_MOVE || o.kind == mot::ORDER_SLIDE) {
                    uint8_t *to = o.kind == mot::ORDER_MOVE ? arena : slides;
                    if (o.len <= 0 || o.src < 0 || size_t(o.src) + size_t(o.len) > arena_size ||
                        size_t(o.dst) + size_t(o.len) > (o.kind == mot::ORDER_MOVE ? arena_size : slides_size))
                        return 3;
#if defined(EMULATE)
                    wave(to + o.dst, arena + o.src, o.len);
                    continue;
#endif
                    (void)to;
                }
                mot::execute(o, ord, au, arena, slides);
            }
        }
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    std::fwrite(arena, 1, arena_size, f);
    std::fwrite(slides, 1, slides_size, f);
    std::fwrite(&st, 1, sizeof st, f);
    std::fwrite(&c, 1, sizeof c, f);
    std::fclose(f);
    std::free(arena);
    std::free(slides);
    return 0;
}
