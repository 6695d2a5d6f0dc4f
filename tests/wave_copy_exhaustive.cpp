// wave_copy_exhaustive.cpp -- csrc/wave_copy.hpp on its own, under the host compiler's sanitizers (tests/test_wave_copy.py
// builds this with -fsanitize=address,undefined and runs it as a child process; it never runs on a GPU).  A wave is the
// copy called for lane = 0 .. 63 in turn: the lanes of one copy do not depend on each other, so that is exact.
//
// Every destination phase 0 .. 15 x every source phase 0 .. 15 x every len of 0 .. 1100 and 4095, 4096, 4097, 8191:
//   pass 1  source and destination each END their heap block, exactly sized: one byte read or written too far is an
//           AddressSanitizer error, a word access off its alignment a UBSan one.  In front of the destination stand
//           sentinel bytes.  Afterwards the destination equals the source and the sentinels are whole.
//   pass 2  sentinels on both sides of the destination, and every lane reads a source of its own (16 L bytes further on in a
//           longer block: the same phase, contents that name the lane), so a destination byte says which lane wrote it; the
//           lanes run 0 .. 63 and then 63 .. 0.  Every byte has a writer, its first writer is its last (a byte is written
//           ONCE), and the sentinels are whole.
// -DMUTANT=k: the same against wave_copy_mutant.hpp (tests/wave_copy_mutants.py) -- that build must FAIL.
#if defined(MUTANT) && MUTANT
#include "wave_copy_mutant.hpp"
#if WAVE_COPY_MUTANT != MUTANT
#error "wave_copy_mutant.hpp is another mutant's"
#endif
#else
#include "wave_copy.hpp"
#endif

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static const int FRONT = 64, BACK = 32;
static const uint8_t SENTINEL = 0xA7;

static uint8_t *block(size_t n) {                                     // 16-aligned, n bytes and not one more
    void *p = nullptr;
    if (posix_memalign(&p, 16, n ? n : 1)) std::exit(2);
    return static_cast<uint8_t *>(p);
}
static uint8_t content(int i) { return uint8_t((i * 151) ^ (i >> 8) ^ 0x5C); }
// pass 2: byte i of lane L's source is lane_byte(16 L + i) = L + (i >> 4) + 67 (i & 15) (mod 256)
static uint8_t lane_byte(int j) { return uint8_t((j >> 4) + 67 * (j & 15)); }

static int fail(const char *what, int dp, int sp, int len, int at) {
    std::printf("FAILED: %s: dst phase %d, src phase %d, len %d, byte %d\n", what, dp, sp, len, at);
    return 5;
}

int main() {
    std::vector<int> lens;
    for (int n = 0; n <= 1100; n++) lens.push_back(n);
    for (int n : {4095, 4096, 4097, 8191}) lens.push_back(n);
    const auto t0 = std::chrono::steady_clock::now();
    long copies = 0;
    std::vector<uint8_t> first;
    for (int dp = 0; dp < 16; dp++)
        for (int sp = 0; sp < 16; sp++)
            for (int len : lens) {
                // ---- pass 1
                uint8_t *sb = block(size_t(sp + len)), *db = block(size_t(FRONT + dp + len));
                uint8_t *src = sb + sp, *dst = db + FRONT + dp;
                for (int i = 0; i < sp; i++) sb[i] = SENTINEL;
                for (int i = 0; i < len; i++) src[i] = content(i);
                std::memset(db, SENTINEL, size_t(FRONT + dp));
                for (int i = 0; i < len; i++) dst[i] = uint8_t(~content(i));
                for (int lane = 0; lane < 64; lane++) dabk::wave_copy(dst, src, len, lane);
                for (int i = 0; i < len; i++)
                    if (dst[i] != content(i)) return fail("pass 1: the destination is not the source", dp, sp, len, i);
                for (int i = 0; i < FRONT + dp; i++)
                    if (db[i] != SENTINEL) return fail("pass 1: a sentinel in front of the destination", dp, sp, len, i - FRONT - dp);
                for (int i = 0; i < len; i++)
                    if (src[i] != content(i)) return fail("pass 1: the source changed", dp, sp, len, i);
                std::free(sb);
                std::free(db);
                // ---- pass 2
                const int span = len + 16 * 63;
                sb = block(size_t(sp + span));
                db = block(size_t(FRONT + dp + len + BACK));
                src = sb + sp;
                dst = db + FRONT + dp;
                for (int j = 0; j < span; j++) src[j] = lane_byte(j);
                first.assign(size_t(len), 0);
                for (int dir = 0; dir < 2; dir++) {
                    std::memset(db, SENTINEL, size_t(FRONT + dp + len + BACK));
                    for (int i = 0; i < len; i++) dst[i] = uint8_t(lane_byte(i) + 64);       // the byte no lane brings
                    for (int k = 0; k < 64; k++) {
                        const int lane = dir ? 63 - k : k;
                        dabk::wave_copy(dst, src + 16 * lane, len, lane);
                    }
                    for (int i = 0; i < len; i++) {
                        const int writer = uint8_t(dst[i] - lane_byte(i));
                        if (writer >= 64) return fail("pass 2: a byte no lane wrote", dp, sp, len, i);
                        if (dir == 0) first[size_t(i)] = uint8_t(writer);
                        else if (first[size_t(i)] != writer) return fail("pass 2: a byte written by two lanes", dp, sp, len, i);
                    }
                    for (int i = 0; i < FRONT + dp; i++)
                        if (db[i] != SENTINEL) return fail("pass 2: a sentinel in front of the destination", dp, sp, len, i - FRONT - dp);
                    for (int i = 0; i < BACK; i++)
                        if (dst[len + i] != SENTINEL) return fail("pass 2: a sentinel behind the destination", dp, sp, len, len + i);
                }
                std::free(sb);
                std::free(db);
                copies += 3;
            }
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::printf("phases=256 lens=%zu copies=%ld seconds=%.2f\n", lens.size(), copies, seconds);
    return 0;
}
