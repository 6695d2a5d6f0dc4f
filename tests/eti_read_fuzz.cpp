// eti_read_fuzz.cpp -- include/dabgpu_eti_read.h on its own, under the host compiler's sanitizers (tests/test_eti_read.py
// builds this with -fsanitize=address,undefined and runs it): N streams of well-formed ETI(NI) frames of random multiplexes
// with bits changed, bytes taken out and put in, headers planted in the data and plain random bytes between them, read in
// calls of random sizes.  S, every output and both state records are heap blocks of exactly their size, so a read or write
// outside is reported; the state runs on from call to call and is now and then replaced by random bytes.  What a call emits is
// held to the contract's own bounds, and the pieces are held to one call over the whole stream.
#include "dabgpu_eti_read.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

namespace er = dabgpu_eti_read;
typedef std::vector<uint8_t> Bytes;

static std::mt19937_64 rng(0xE71DA7A);
static int below(int n) { return int(rng() % uint64_t(n)); }

#define REQUIRE(cond)                                                          \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::printf("line %d: %s\n", __LINE__, #cond);                     \
            std::exit(5);                                                      \
        }                                                                      \
    } while (0)

static uint32_t crc16(const uint8_t *p, size_t n) {
    uint32_t crc = 0xFFFFu;
    for (size_t i = 0; i < n; i++) crc = er::crc_byte(crc, p[i]);
    return crc ^ 0xFFFFu;
}

struct Mux {
    int nst;
    int stl[er::MAX_STREAMS];
    uint8_t stc[4 * er::MAX_STREAMS];
};

static Mux random_mux() {
    Mux m{};
    m.nst = below(6) == 0 ? below(65) : below(5);
    int room = (er::FRAME_BYTES - 16 - 4 * m.nst - 96 - 8) / 8;
    for (int k = 0; k < m.nst; k++) {
        m.stl[k] = room > 0 ? below(room < 200 ? room + 1 : 200) : 0;
        room -= m.stl[k];
        m.stc[4 * k] = uint8_t(rng());
        m.stc[4 * k + 1] = uint8_t(rng());
        m.stc[4 * k + 2] = uint8_t((below(64) << 2) | (m.stl[k] >> 8));
        m.stc[4 * k + 3] = uint8_t(m.stl[k]);
    }
    return m;
}

static Bytes frame_of(const Mux &m, int count) {
    Bytes f(er::FRAME_BYTES, 0x55);
    int sum = 0;
    for (int k = 0; k < m.nst; k++) sum += m.stl[k];
    const int fl = m.nst + 1 + 24 + 2 * sum, fct = count % 250;
    f[0] = below(10) ? 0xFF : uint8_t(rng());
    f[1] = fct & 1 ? 0xF8 : 0x07;
    f[2] = fct & 1 ? 0xC5 : 0x3A;
    f[3] = fct & 1 ? 0x49 : 0xB6;
    f[4] = uint8_t(fct);
    f[5] = uint8_t(0x80 | m.nst);
    f[6] = uint8_t(((count & 7) << 5) | (1 << 3) | (fl >> 8));
    f[7] = uint8_t(fl);
    std::memcpy(&f[8], m.stc, size_t(4 * m.nst));
    int at = 8 + 4 * m.nst;
    f[at] = f[at + 1] = 0xFF;
    const uint32_t hc = crc16(&f[4], size_t(at + 2 - 4));
    f[at + 2] = uint8_t(hc >> 8);
    f[at + 3] = uint8_t(hc);
    at += 4;
    const int data = 96 + 8 * sum;
    for (int i = 0; i < data; i++) f[at + i] = uint8_t(rng());
    for (int j = 0; j < 3; j++)
        if (below(8)) {
            const uint32_t c = crc16(&f[at + 32 * j], 30);
            f[at + 32 * j + 30] = uint8_t(c >> 8);
            f[at + 32 * j + 31] = uint8_t(c);
        }
    const uint32_t dc = crc16(&f[at], size_t(data));
    f[at + data] = uint8_t(dc >> 8);
    f[at + data + 1] = uint8_t(dc);
    for (int i = 2; i < 8; i++) f[at + data + i] = 0xFF;
    return f;
}

static Bytes random_stream(const Mux &m, int n_frames) {
    Bytes s;
    int count = below(5000);
    for (int i = 0; i < n_frames; i++, count++) {
        Bytes f = frame_of(below(12) ? m : random_mux(), count % 5000);
        switch (below(10)) {
            case 0: f[size_t(below(er::FRAME_BYTES))] ^= uint8_t(1 << below(8)); break;
            case 1: f[size_t(below(12 + 4 * m.nst))] ^= uint8_t(1 << below(8)); break;
            case 2: {
                const int at = below(6000);
                f.erase(f.begin() + at, f.begin() + at + 1 + below(30));
                break;
            }
            case 3: f.insert(f.begin() + below(6000), size_t(1 + below(20)), uint8_t(rng())); break;
            case 4: {                                                          // a header inside the frame, wherever it falls
                const Bytes g = frame_of(random_mux(), below(5000));
                const int at = below(er::FRAME_BYTES - 300);
                std::memcpy(&f[size_t(at)], g.data(), 280);
                break;
            }
            case 5: count += below(5); break;
            case 6: for (int k = below(3000); k > 0; k--) s.push_back(uint8_t(rng())); break;
            default: break;
        }
        s.insert(s.end(), f.begin(), f.end());
    }
    if (below(3) == 0) s.resize(s.size() - size_t(below(int(s.size() < 7000 ? s.size() : 7000))));
    return s;
}

struct Outputs {
    std::unique_ptr<uint8_t[]> fib, ok, state;
    std::unique_ptr<er::Status[]> status;
    std::vector<std::unique_ptr<uint8_t[]>> out;
    er::Result result{};
};

// one call: the state record `in` (STATE_BYTES, any bytes) and `n` new bytes -> outputs; returns rows
static uint32_t one_call(const uint8_t *in, const uint8_t *fresh, size_t n, const Mux *m, Outputs &o) {
    er::Head head{};
    std::memcpy(&head, in, sizeof head);
    const size_t tail = er::clamp_tail(head.tail_bytes);
    std::unique_ptr<uint8_t[]> s(new uint8_t[tail + n]);                      // exactly S
    std::memcpy(s.get(), in + er::STATE_HEAD_BYTES, tail);
    if (n) std::memcpy(s.get() + tail, fresh, n);
    const size_t rows = (er::MAX_TAIL + n) / er::FRAME_BYTES;
    o.fib.reset(new uint8_t[rows * 96]);
    o.ok.reset(new uint8_t[rows * 3]);
    o.status.reset(new er::Status[rows]);
    o.state.reset(new uint8_t[er::STATE_BYTES]);
    er::PlanKey key{};
    uint8_t *outs[er::MAX_STREAMS] = {};
    int32_t offset[er::MAX_STREAMS] = {}, bytes[er::MAX_STREAMS] = {};
    o.out.clear();
    if (m) {
        key.nst = m->nst;
        int sum = 0;
        for (int k = 0; k < m->nst; k++) {
            offset[k] = 8 * sum;
            bytes[k] = 8 * m->stl[k];
            sum += m->stl[k];
            o.out.emplace_back(below(4) ? new uint8_t[rows * size_t(bytes[k])] : nullptr);
            outs[k] = o.out.back().get();
        }
        key.fl = m->nst + 1 + 24 + 2 * sum;
        std::memcpy(key.stc, m->stc, size_t(4 * m->nst));
    }
    er::HostOut h{o.fib.get(), o.ok.get(), o.status.get(), &o.result, outs, offset, bytes};
    er::read_entry(s.get(), tail + n, head, m ? &key : nullptr, h, o.state.get());
    const er::Result &c = o.result;
    REQUIRE(c.rows <= rows && c.taken + c.bad_data_crc + c.other_plan == c.rows && c.tail_bytes <= uint32_t(er::MAX_TAIL));
    REQUIRE(size_t(c.rows) * er::FRAME_BYTES + c.skipped + c.tail_bytes == tail + n);
    REQUIRE(m || c.other_plan == 0);
    uint32_t before = 0;
    for (uint32_t r = 0; r < c.rows; r++) {
        const er::Status &st = o.status[r];
        REQUIRE(st.offset + er::FRAME_BYTES <= tail + n && (r == 0 || st.offset >= before + er::FRAME_BYTES));
        REQUIRE(st.verdict == er::TAKEN || st.verdict == er::BAD_DATA_CRC || st.verdict == er::OTHER_PLAN);
        REQUIRE(st.fct < 250 && st.fp < 8 && st.gap < 250 && st.reserved == 0 && st.reserved2 == 0);
        before = st.offset;
    }
    er::Head next{};
    std::memcpy(&next, o.state.get(), sizeof next);
    REQUIRE(next.tail_bytes == c.tail_bytes && next.rows == head.rows + c.rows);
    for (size_t i = c.tail_bytes; i < size_t(er::FRAME_BYTES); i++) REQUIRE(o.state[er::STATE_HEAD_BYTES + i] == 0);
    return c.rows;
}

int main(int argc, char **argv) {
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 200;
    long rows_seen = 0, resyncs = 0;
    for (int round = 0; round < rounds; round++) {
        const Mux m = random_mux();
        const bool planned = below(4) != 0;
        const Bytes s = below(15) ? random_stream(m, 1 + below(12)) : Bytes(size_t(below(30000)), uint8_t(rng()));
        const std::unique_ptr<uint8_t[]> zero(new uint8_t[er::STATE_BYTES]());
        // the whole stream in one call
        Outputs whole;
        const uint32_t want = one_call(zero.get(), s.data(), s.size(), planned ? &m : nullptr, whole);
        resyncs += whole.result.resyncs;
        // ... and in pieces
        std::unique_ptr<uint8_t[]> state(new uint8_t[er::STATE_BYTES]());
        uint32_t got = 0;
        Bytes fibs;
        for (size_t at = 0; at < s.size();) {
            const int kind = below(6);
            size_t n = kind == 0 ? size_t(below(3)) : kind == 1 ? size_t(6143 + below(3)) : size_t(below(20000));
            if (n > s.size() - at) n = s.size() - at;
            const std::unique_ptr<uint8_t[]> piece(new uint8_t[n ? n : 1]);
            std::memcpy(piece.get(), s.data() + at, n);
            Outputs o;
            const uint32_t r = one_call(state.get(), piece.get(), n, planned ? &m : nullptr, o);
            fibs.insert(fibs.end(), o.fib.get(), o.fib.get() + size_t(r) * 96);
            got += r;
            state = std::move(o.state);
            at += n;
        }
        REQUIRE(got == want && std::memcmp(state.get(), whole.state.get(), er::STATE_BYTES) == 0);
        REQUIRE(fibs.size() == size_t(want) * 96 && (want == 0 || std::memcmp(fibs.data(), whole.fib.get(), fibs.size()) == 0));
        rows_seen += want;
        // a state of random bytes, or of all ones, in front of the same stream
        std::unique_ptr<uint8_t[]> hostile(new uint8_t[er::STATE_BYTES]);
        for (int i = 0; i < er::STATE_BYTES; i++) hostile[i] = round & 1 ? uint8_t(rng()) : 0xFF;
        Outputs o;
        one_call(hostile.get(), s.data(), s.size() < 9000 ? s.size() : 9000, planned ? &m : nullptr, o);
    }
    REQUIRE(rows_seen > rounds && resyncs > rounds / 4);
    std::printf("ok: %d rounds, %ld rows, %ld resyncs\n", rounds, rows_seen, resyncs);
    return 0;
}
