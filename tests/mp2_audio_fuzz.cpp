// mp2_audio_fuzz.cpp -- include/dabgpu_mp2_audio.h on its own, under the host compiler's sanitizers (tests/test_mp2_audio.py
// builds this with -fsanitize=address,undefined and runs it): N frames of every rate a header can name -- random bodies,
// bodies with a sparse allocation (so that the audio fits), and such frames with bytes changed -- get their ISO CRC
// repaired (clocked here, bit by bit) and go through parse_frame and the serial decoder decode_frame.  Every logical
// frame is copied to a heap block of exactly its size (a 24 kHz frame is two blocks), so a read outside [0, L) is a heap
// overflow, and the accessor aborts on an index outside [0, L).
#include "dabgpu_mp2_audio.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

namespace mp2 = dabgpu_mp2;

static std::mt19937_64 rng(0xDAB3);
static int below(int n) { return int(rng() % uint64_t(n)); }

struct Checked {
    const uint8_t *a, *b;
    int split, L;
    uint8_t operator()(int i) const {
        if (i < 0 || i >= L) std::abort();
        return i < split ? a[i] : b[i - split];
    }
};

static void put_bits(std::vector<uint8_t> &f, int &pos, unsigned v, int n) {
    for (int k = n - 1; k >= 0; k--, pos++)
        if (size_t(pos >> 3) < f.size()) f[size_t(pos >> 3)] = uint8_t((f[size_t(pos >> 3)] & ~(0x80 >> (pos & 7))) | (((v >> k) & 1) ? (0x80 >> (pos & 7)) : 0));
}

// the CRC over header bits 16 .. 31, allocation and SCFSI as they lie in f; false when they run past the frame
static bool repair_crc(std::vector<uint8_t> &f, int id, int B, int L) {
    const uint32_t h = mp2::header_word(f[0], f[1], f[2], f[3]);
    const mp2::Shape s = mp2::frame_shape(h, id, B);
    const Checked bytes = {f.data(), f.data(), L, L};
    int pos = 48, nz = 0;
    for (int sb = 0; sb < s.t.sblimit; sb++) {
        const int n = mp2::nbal(s.t, sb), fields = s.channels == 2 && sb < s.bound ? 2 : 1;
        for (int k = 0; k < fields; k++, pos += n) {
            if (pos + n > 8 * L) return false;
            if (mp2::get_bits(bytes, pos, n)) nz += s.channels == 2 && fields == 1 ? 2 : 1;
        }
    }
    const int end = pos + 2 * nz;
    if (end > 8 * L) return false;
    uint32_t crc = 0xFFFF;
    for (int p = 16; p < end; p++) {
        if (p == 32) p = 48;
        crc = mp2::crc_step_bit(crc, (f[size_t(p >> 3)] >> (7 - (p & 7))) & 1);
    }
    f[4] = uint8_t(crc >> 8);
    f[5] = uint8_t(crc);
    return true;
}

int main(int argc, char **argv) {
    const long frames = argc > 1 ? atol(argv[1]) : 60000;
    long good = 0, decoded = 0, overrun = 0, scf63 = 0, silent = 0;
    std::vector<float> v(size_t(mp2::FRAME_VALUES));
    for (long w = 0; w < frames; w++) {
        const int id = below(2), B = mp2::bitrate_of_index(id, 1 + below(14)), L = (id ? 3 : 6) * B, lf = 3 * B;
        int mode = below(4);
        if (id == 1 && mp2::mono_only_rate(B)) mode = 3;
        if (id == 1 && mp2::two_channel_only_rate(B) && mode == 3) mode = below(3);
        std::vector<uint8_t> f(size_t(L), 0);
        for (uint8_t &x : f) x = uint8_t(rng());
        int idx = 0;
        for (int i = 1; i < 15; i++)
            if (mp2::bitrate_of_index(id, i) == B) idx = i;
        f[0] = 0xFF;
        f[1] = uint8_t(0xF0 | (id << 3) | (2 << 1));
        f[2] = uint8_t((idx << 4) | (1 << 2) | below(4));
        f[3] = uint8_t((mode << 6) | (below(4) << 4) | below(16));
        const int how = below(4);
        if (how > 0) {                                 // a sparse allocation: the fewer fields, the sooner the audio fits
            const mp2::Shape s = mp2::frame_shape(mp2::header_word(f[0], f[1], f[2], f[3]), id, B);
            int pos = 48;
            for (int sb = 0; sb < s.t.sblimit; sb++)
                for (int k = 0; k < (s.channels == 2 && sb < s.bound ? 2 : 1); k++) {
                    const int n = mp2::nbal(s.t, sb);
                    put_bits(f, pos, below(how == 1 ? 2 : 6) == 0 ? unsigned(1 + below((1 << n) - 1)) : 0u, n);
                }
        }
        if (how == 3) for (int k = 1 + below(3); k > 0; k--) f[size_t(6 + below(L - 6))] ^= uint8_t(1 << below(8));
        const bool repaired = repair_crc(f, id, B, L);
        uint8_t *a = static_cast<uint8_t *>(std::malloc(size_t(lf))), *b = static_cast<uint8_t *>(std::malloc(size_t(lf)));
        if (!a || !b) return 2;
        std::memcpy(a, f.data(), size_t(lf));
        if (id == 0) std::memcpy(b, f.data() + lf, size_t(lf));
        const Checked bytes = {a, b, lf, L};
        int c = 0;
        const int kind = mp2::parse_frame(bytes, L, B, id, &c);
        if (repaired != (kind == mp2::FRAME_GOOD)) return 3;
        // (the decoder is safe on any frame with a valid header, GOOD or not; only GOOD ones are counted)
        const mp2::Level lv = mp2::decode_frame(bytes, L, B, id, v.data());
        const mp2::Level again = mp2::decode_frame(bytes, L, B, id, static_cast<float *>(nullptr));
        if (std::memcmp(&lv, &again, sizeof lv) != 0) return 4;
        if (lv.kind != mp2::AUDIO_DECODED && lv.kind != mp2::AUDIO_OVERRUN) return 5;
        float peak[2] = {0.0f, 0.0f};
        for (int i = 0; i < mp2::FRAME_VALUES; i++) {
            if (!std::isfinite(v[size_t(i)])) return 6;
            const float m = std::fabs(v[size_t(i)]);
            if (m > peak[i / (mp2::FRAME_VALUES / 2)]) peak[i / (mp2::FRAME_VALUES / 2)] = m;
        }
        if (peak[0] != lv.peak[0] || peak[1] != lv.peak[1]) return 7;
        if (lv.kind == mp2::AUDIO_OVERRUN && (lv.channels || lv.cells || lv.scf63 || lv.power[0] != 0.0f || lv.power[1] != 0.0f || peak[0] != 0.0f || peak[1] != 0.0f)) return 8;
        if (lv.kind == mp2::AUDIO_DECODED && (lv.channels != (mode == 3 ? 1 : 2) || lv.cells > 60 || lv.scf63 > 3 * lv.cells || peak[0] > 2.3f || peak[1] > 2.3f)) return 9;
        if (kind == mp2::FRAME_GOOD) {
            good++;
            decoded += lv.kind == mp2::AUDIO_DECODED;
            overrun += lv.kind == mp2::AUDIO_OVERRUN;
            scf63 += lv.scf63;
            silent += lv.kind == mp2::AUDIO_DECODED && lv.power[0] + lv.power[1] == 0.0f;
        }
        std::free(a);
        std::free(b);
    }
    std::printf("frames=%ld good=%ld decoded=%ld overrun=%ld scf63=%ld silent=%ld\n", frames, good, decoded, overrun, scf63, silent);
    return 0;
}
