// packet_fec_erasure_fuzz.cpp -- include/dabgpu_packet_fec_erasures.h's host path under AddressSanitizer and UBSan
// (tests/test_packet_fec_erasures.py builds and runs this; a stand-alone program, nothing of it is loaded into Python).
// Streams of random bit rate are fed to process_erasures in calls of random length (none, fewer than D, many frames): FEC
// frames whose data tables are packets of one (mostly) to four slots with true CRCs and true parity, then damaged -- wiped packets (up
// to eleven), random bytes, damaged length fields, marks removed -- between stretches of noise; the first state record of a
// stream is NULL, zeros, random bytes, a record of the errors-only call, or a valid head with random suspect bits over random
// frames.  Every buffer is a heap block of exactly its size, so a byte read or written outside is caught.
// argv: calls -> one line of totals.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "dabgpu_packet_fec_erasures.h"

namespace fec = dabgpu_packet_fec;

static const fec::Gf GF = fec::make_gf();

// the 16 parity bytes of 188 data bytes: d(x) x^16 mod the generator, by its roots (a systematic encoder by division)
static void parity_of(const uint8_t *data, uint8_t *par) {
    uint8_t gen[18] = {1};                                             // gen[i]: coefficient of x^i
    int deg = 0;
    for (int k = 0; k < 16; k++) {
        uint8_t nx[18] = {};
        for (int i = 0; i <= deg; i++) {
            nx[i + 1] ^= gen[i];
            nx[i] ^= uint8_t(fec::gmul(GF, gen[i], GF.exp[k]));
        }
        deg++;
        std::memcpy(gen, nx, size_t(deg) + 1);
    }
    uint8_t rem[16] = {};
    for (int c = 0; c < fec::K; c++) {
        const uint8_t fb = data[c] ^ rem[0];
        for (int j = 0; j < 15; j++) rem[j] = rem[j + 1] ^ uint8_t(fec::gmul(GF, fb, gen[15 - j]));
        rem[15] = uint8_t(fec::gmul(GF, fb, gen[0]));
    }
    std::memcpy(par, rem, 16);
}

int main(int argc, char **argv) {
    const long calls = argc > 1 ? std::atol(argv[1]) : 1000;
    std::mt19937 rng(20250311);
    auto below = [&](int n) { return int(rng() % unsigned(n)); };
    long frames = 0, clean = 0, corrected = 0, erasure_corrected = 0, uncorrectable = 0, suspect = 0, with = 0, beyond = 0, fresh = 0, carried = 0,
         empty = 0, done = 0;
    while (done < calls) {
        // one stream
        const int S = 1 + below(64), D = fec::delay(S), fb = fec::SLOT_BYTES * S, nb = fec::state_bytes(S);
        const int total_slots = 103 * (2 + below(4)) + below(200);
        std::vector<uint8_t> slots(size_t(total_slots + S) * fec::SLOT_BYTES);
        for (auto &v : slots) v = uint8_t(rng());
        for (int at = below(120); at + 103 <= total_slots; at += 103 + (below(4) ? 0 : below(60))) {
            uint8_t *f = slots.data() + size_t(at) * fec::SLOT_BYTES;
            for (int i = 0; i < 94;) {                                 // packets that stay inside their logical frame and the table
                const int room_frame = S - (at + i) % S, room = room_frame < 94 - i ? room_frame : 94 - i;
                const int L = below(8) ? 1 : 1 + below(room < 4 ? room : 4);      // mostly one slot: a lost packet is one suspect slot
                uint8_t *p = f + fec::SLOT_BYTES * i;
                p[0] = uint8_t(((L - 1) << 6) | (p[0] & 0x3C) | (p[0] & 1));     // an address below 512: never 1022
                const uint32_t crc = dabgpu_pad::crc16(p, fec::SLOT_BYTES * L - 2);
                p[fec::SLOT_BYTES * L - 2] = uint8_t(crc >> 8);
                p[fec::SLOT_BYTES * L - 1] = uint8_t(crc & 0xFF);
                i += L;
            }
            uint8_t rows[12][204];
            for (int r = 0; r < 12; r++) {
                for (int c = 0; c < fec::K; c++) rows[r][c] = f[fec::frame_index(r, c)];
                parity_of(rows[r], rows[r] + fec::K);
                for (int c = fec::K; c < fec::N; c++) f[fec::frame_index(r, c)] = rows[r][c];
            }
            for (int i = 0; i < 9; i++) {
                f[fec::SLOT_BYTES * (94 + i)] = uint8_t((i << 2) | 3);
                f[fec::SLOT_BYTES * (94 + i) + 1] = 0xFE;
            }
            const int kind = below(7);
            for (int k = 0; k < (kind == 1 ? 6 : kind == 2 ? 40 : 0); k++) f[below(fec::FRAME_BYTES)] ^= uint8_t(1 + below(255));
            const int wiped = kind == 3 || kind == 6 ? 1 + below(11) : 0;
            for (int k = 0; k < wiped; k++) {
                uint8_t *p = f + fec::SLOT_BYTES * below(94);
                for (int b = 0; b < fec::SLOT_BYTES; b++) p[b] = uint8_t(rng());
            }
            for (int k = 0; k < (kind == 6 ? below(4) : 0); k++) f[below(fec::FRAME_BYTES)] ^= uint8_t(1 + below(255));
            for (int k = 0; k < (kind == 4 ? 1 + below(3) : 0); k++) f[fec::SLOT_BYTES * (94 + below(9)) + 1] ^= 0x40;
            for (int k = 0; k < (kind == 5 ? 1 + below(5) : 0); k++) f[fec::SLOT_BYTES * below(94)] ^= 0xC0;
        }
        const int n_frames = total_slots / S;
        std::unique_ptr<uint8_t[]> state;                              // exactly nb bytes, or none
        const int start = below(5);
        if (start) {
            state.reset(new uint8_t[size_t(nb)]);
            for (int i = 0; i < nb; i++) state[i] = start == 1 ? 0 : uint8_t(rng());
            if (start >= 3) {                                          // a head this code could have written, random frames behind it
                fec::Head h;
                fec::head_fresh_erasures(h, S);
                h.frames_seen = below(1000);
                h.last_end = h.frames_seen * S >= 103 && below(2) ? h.frames_seen * S - 1 - below(50 < h.frames_seen * S - 102 ? 50 : 1) : -1;
                for (int i = 0; i < 8; i++)
                    if (h.frames_seen * S - 8 + i >= 0 && !below(3)) h.tail[i] = uint8_t(below(9));
                const int padding = h.frames_seen < D ? int(D - h.frames_seen) * S : 0;
                for (int i = padding; i < D * S; i++)
                    if (!below(6)) h.reserved[i >> 3] |= uint8_t(1u << (i & 7));
                if (start == 4) h.magic = fec::MAGIC;                  // the errors-only call's record (its reserved bytes are not zero: foreign there too)
                std::memcpy(state.get(), &h, sizeof h);
                carried += fec::head_ok_erasures(h, S);
            }
        }
        fresh += start < 3;
        for (int at = 0; at < n_frames && done < calls; done++) {
            const int kind = below(4);
            int n = kind == 0 ? 0 : kind == 1 ? 1 + below(D) : 1 + below(3 * D + 40);
            n = n < n_frames - at ? n : n_frames - at;
            empty += n == 0;
            const size_t stride_in = size_t(fb) + size_t(below(3)) * 5, stride_out = size_t(fb) + size_t(below(3)) * 7;
            const size_t in_bytes = n ? size_t(n - 1) * stride_in + size_t(fb) : 0, out_bytes = n ? size_t(n - 1) * stride_out + size_t(fb) : 0;
            std::unique_ptr<uint8_t[]> in(new uint8_t[in_bytes ? in_bytes : 1]), out(new uint8_t[out_bytes ? out_bytes : 1]), next(new uint8_t[size_t(nb)]);
            for (int k = 0; k < n; k++) std::memcpy(in.get() + size_t(k) * stride_in, slots.data() + size_t(at + k) * size_t(fb), size_t(fb));
            fec::ErasureCounters c;
            fec::process_erasures(GF, state.get(), next.get(), c, n ? in.get() : nullptr, stride_in, n, S, n ? out.get() : nullptr, stride_out);
            fec::Head h;
            std::memcpy(&h, next.get(), sizeof h);
            if (!fec::head_ok_erasures(h, S) || fec::head_ok(h, S) || c.c.cifs != n ||
                c.c.rows_clean + c.c.rows_corrected + c.rows_erasure_corrected + c.c.rows_uncorrectable != 12 * c.c.frames ||
                c.frames_beyond_erasures > c.frames_with_suspects || c.frames_with_suspects > c.c.frames || c.slots_suspect > c.c.slots) {
                std::printf("a call left a record or counts that do not hold\n");
                return 1;
            }
            frames += c.c.frames, clean += c.c.rows_clean, corrected += c.c.rows_corrected, erasure_corrected += c.rows_erasure_corrected;
            uncorrectable += c.c.rows_uncorrectable, suspect += c.slots_suspect, with += c.frames_with_suspects, beyond += c.frames_beyond_erasures;
            state = std::move(next);
            at += n;
        }
    }
    std::printf("calls=%ld frames=%ld clean=%ld corrected=%ld erasure_corrected=%ld uncorrectable=%ld suspect=%ld with_suspects=%ld beyond=%ld fresh=%ld "
                "carried=%ld empty=%ld\n", done, frames, clean, corrected, erasure_corrected, uncorrectable, suspect, with, beyond, fresh, carried, empty);
    return 0;
}
