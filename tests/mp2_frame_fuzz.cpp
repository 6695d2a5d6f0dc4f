// mp2_frame_fuzz.cpp -- include/dabgpu_mp2_frame.h on its own, under the host compiler's sanitizers (tests/test_mp2_follow.py
// builds this with -fsanitize=address,undefined and runs it): N frames of every legal length -- random bytes, random
// bytes behind a valid header, valid frames (a CRC computed here, bit by bit) and valid frames with bytes changed -- go
// through parse_frame and, when good, through row_byte for the whole row.  Every logical frame is copied to a heap block
// of exactly its size (a 24 kHz frame is two blocks), so a read outside [0, L) is a heap overflow; the accessor counts
// indices outside [0, L) as well.  First the byte-wise CRC step is held to the bit-wise one for every byte and register.
#include "dabgpu_mp2_frame.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

namespace mp2 = dabgpu_mp2;

static std::mt19937_64 rng(0xDAB2);
static int below(int n) { return int(rng() % uint64_t(n)); }
static long outside = 0;

struct Checked {
    const uint8_t *a, *b;
    int split, L;
    uint8_t operator()(int i) const {
        if (i < 0 || i >= L) { outside++; return 0; }
        return i < split ? a[i] : b[i - split];
    }
};

static void put_bits(std::vector<uint8_t> &f, int &pos, unsigned v, int n) {
    for (int k = n - 1; k >= 0; k--, pos++)
        if (size_t(pos >> 3) < f.size()) f[size_t(pos >> 3)] = uint8_t((f[size_t(pos >> 3)] & ~(0x80 >> (pos & 7))) | (((v >> k) & 1) ? (0x80 >> (pos & 7)) : 0));
}

// a valid frame for (id, B): a legal mode, random allocation and SCFSI, the CRC clocked bit by bit
static std::vector<uint8_t> valid_frame(int id, int B, int L) {
    std::vector<uint8_t> f(size_t(L), 0);
    for (uint8_t &v : f) v = uint8_t(rng());
    int idx = 0;
    for (int i = 1; i < 15; i++)
        if (mp2::bitrate_of_index(id, i) == B) idx = i;
    int mode = below(4);
    if (id == 1 && mp2::mono_only_rate(B)) mode = 3;
    if (id == 1 && mp2::two_channel_only_rate(B) && mode == 3) mode = below(3);
    f[0] = 0xFF;
    f[1] = uint8_t(0xF0 | (id << 3) | (2 << 1) | (below(8) == 0 ? 1 : 0));
    f[2] = uint8_t((idx << 4) | (1 << 2) | below(4));
    f[3] = uint8_t((mode << 6) | (below(4) << 4) | below(16));
    const uint32_t h = mp2::header_word(f[0], f[1], f[2], f[3]);
    const mp2::Shape s = mp2::frame_shape(h, id, B);
    int pos = 48, nz = 0;
    for (int sb = 0; sb < s.t.sblimit; sb++) {
        const int n = mp2::nbal(s.t, sb), fields = s.channels == 2 && sb < s.bound ? 2 : 1;
        for (int k = 0; k < fields; k++) {
            const unsigned a = below(3) == 0 ? 0u : unsigned(below(1 << n));
            put_bits(f, pos, a, n);
            if (a) nz += s.channels == 2 && fields == 1 ? 2 : 1;
        }
    }
    const int end = pos + 2 * nz;
    uint32_t crc = 0xFFFF;
    for (int p = 16; p < end; p++) {
        if (p == 32) p = 48;
        if (p >= 8 * L) break;
        crc = mp2::crc_step_bit(crc, (f[size_t(p >> 3)] >> (7 - (p & 7))) & 1);
    }
    f[4] = uint8_t(crc >> 8);
    f[5] = uint8_t(crc);
    return f;
}

int main(int argc, char **argv) {
    const long frames = argc > 1 ? atol(argv[1]) : 200000;
    for (uint32_t reg = 0; reg < 0x10000; reg += 257)
        for (uint32_t v = 0; v < 256; v++) {
            uint32_t bitwise = reg;
            for (int k = 7; k >= 0; k--) bitwise = mp2::crc_step_bit(bitwise, (v >> k) & 1);
            if (bitwise != mp2::crc_step_byte(reg, v)) { std::printf("crc step differs at %x %x\n", reg, v); return 5; }
        }
    long kinds[4] = {0, 0, 0, 0}, rows = 0;
    for (long w = 0; w < frames; w++) {
        const int B = 8 * (1 + below(48)), id = below(2), L = (id ? 3 : 6) * B, lf = 3 * B;
        bool named = false;
        for (int i = 1; i < 15; i++) named = named || mp2::bitrate_of_index(id, i) == B;
        std::vector<uint8_t> f(size_t(L), 0);
        const int how = below(8);
        if (how < 2 || !named) {
            for (uint8_t &v : f) v = uint8_t(rng());
            if (how == 1) { f[0] = 0xFF; f[1] = uint8_t(0xF4 | (id << 3)); f[2] = uint8_t((f[2] & 0xF3) | 4); }
        } else {
            f = valid_frame(id, B, L);
            if (how >= 5) for (int k = 1 + below(3); k > 0; k--) f[size_t(below(how == 5 ? 48 < L ? 48 : L : L))] ^= uint8_t(1 << below(8));
        }
        uint8_t *a = static_cast<uint8_t *>(std::malloc(size_t(lf))), *b = static_cast<uint8_t *>(std::malloc(size_t(lf)));
        if (!a || !b) return 2;
        std::memcpy(a, f.data(), size_t(lf));
        if (id == 0) std::memcpy(b, f.data() + lf, size_t(lf));
        const Checked bytes = {a, b, lf, L};
        int c = 0;
        const int kind = mp2::parse_frame(bytes, L, B, id, &c);
        if (kind < 0 || kind > 3) return 3;
        kinds[kind]++;
        if (kind == mp2::FRAME_GOOD) {
            const int x = mp2::xpad_bytes(L, c);
            if (x < 4 || x > mp2::XPAD_MAX || x + 6 > mp2::ROW_BYTES) return 4;
            unsigned sum = 0;
            for (int j = 0; j < mp2::ROW_BYTES; j++) sum += mp2::row_byte(bytes, L, c, x, j);
            rows += sum != 0;
            if (mp2::row_byte(bytes, L, c, x, x + 2) != f[size_t(L - 2)] || mp2::row_byte(bytes, L, c, x, x + 1) != f[size_t(L - 3)]) return 6;
        }
        // (an unmutated valid frame with the CRC is good)
        if (how >= 2 && how < 5 && named && !(f[1] & 1) && kind != mp2::FRAME_GOOD) return 7;
        std::free(a);
        std::free(b);
    }
    std::printf("frames=%ld good=%ld header=%ld no_crc=%ld crc_failed=%ld rows=%ld outside=%ld\n", frames, kinds[0], kinds[1], kinds[2],
                kinds[3], rows, outside);
    return outside == 0 ? 0 : 8;
}
