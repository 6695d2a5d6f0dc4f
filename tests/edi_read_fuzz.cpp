// edi_read_fuzz.cpp -- include/dabgpu_edi.h alone, under AddressSanitizer and UBSan (tests/test_edi_read.py builds and runs
// it): the serial walk on random and mutated streams and states.  Every buffer is its own heap block of exactly the size
// the contract gives it, so a byte read or written outside one stops the run.  Checked besides: a stream fed in two pieces
// leaves the rows, counters and state one call leaves; the tail stays below 8192 bytes; a stream that is header-plausible
// every 10 bytes is walked to its end.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "dabgpu_edi.h"

namespace ed = dabgpu_edi;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return uint32_t(rng_state >> 16);
}
static uint32_t below(uint32_t n) { return n ? rnd() % n : 0; }

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("edi_read_fuzz FAILED line %d: %s\n", __LINE__, #c); \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

struct Plan {
    ed::PlanKey key{};
    int data_bytes = 0;
};

static Plan random_plan() {
    Plan p;
    p.key.nst = int(below(5));
    int sad = 0;
    for (int k = 0; k < p.key.nst; k++) {
        const int stl = 3 * (1 + int(below(8))), scid = int(below(64)), tpl = 0x20 | int(below(4));
        uint8_t *stc = p.key.stc + 4 * k;
        stc[0] = uint8_t((scid << 2) | (sad >> 8));
        stc[1] = uint8_t(sad & 0xff);
        stc[2] = uint8_t((tpl << 2) | (stl >> 8));
        stc[3] = uint8_t(stl & 0xff);
        sad += 40;
        p.data_bytes += 8 * stl;
    }
    return p;
}

static void append_packet(std::vector<uint8_t> &s, const Plan &p, uint32_t seq, uint32_t dlfc) {
    const size_t at = s.size();
    s.resize(at + size_t(ed::packet_bytes(p.key.nst, p.data_bytes)));
    uint8_t fic[96];
    for (int j = 0; j < 3; j++) {                      // FIBs with a right CRC, now and then a wrong one
        uint32_t crc = 0xFFFFu;
        for (int i = 0; i < 30; i++) {
            fic[32 * j + i] = uint8_t(rnd());
            crc = ed::crc_byte(crc, fic[32 * j + i]);
        }
        crc ^= 0xFFFFu;
        fic[32 * j + 30] = uint8_t(crc >> 8);
        fic[32 * j + 31] = uint8_t((crc & 0xFF) ^ (below(8) == 0 ? 1 : 0));
    }
    const int n = ed::write_packet([&](int i, uint8_t b) { s[at + size_t(i)] = b; }, p.key, seq, dlfc, below(4) ? 0xFF : 0xE1,
                                   [&](int i) { return uint32_t(fic[i]); }, [&](int, int) { return rnd() & 0xFFu; });
    CHECK(size_t(n) == s.size() - at);
    int total = 0;
    CHECK(ed::good_at(s.data(), s.size(), at, total) && total == n);
}

struct Outputs {
    uint32_t rows;
    std::unique_ptr<uint8_t[]> fib, ok, state;
    std::unique_ptr<ed::Status[]> status;
    std::vector<std::unique_ptr<uint8_t[]>> out;
    std::vector<uint8_t *> out_ptr;
    ed::Result result{};
};

// one call: S is put together in a heap block of exactly |S| bytes
static void run(const std::vector<uint8_t> &state_in, const uint8_t *bytes, size_t n, const Plan *plan, Outputs &o) {
    ed::Head in{};
    std::memcpy(&in, state_in.data(), sizeof in);
    const size_t tail = ed::clamp_tail(in.tail_bytes);
    std::unique_ptr<uint8_t[]> s(new uint8_t[tail + n ? tail + n : 1]);
    if (tail) std::memcpy(s.get(), state_in.data() + ed::STATE_HEAD_BYTES, tail);
    if (n) std::memcpy(s.get() + tail, bytes, n);
    o.rows = ed::max_rows(uint32_t(n), plan ? plan->key.nst : 0, plan ? plan->data_bytes : 0);
    CHECK(o.rows >= 1);
    o.fib.reset(new uint8_t[size_t(o.rows) * 96]);
    o.ok.reset(new uint8_t[size_t(o.rows) * 3]);
    o.status.reset(new ed::Status[o.rows]);
    o.state.reset(new uint8_t[ed::STATE_BYTES]);
    o.out.clear();
    o.out_ptr.clear();
    if (plan)
        for (int k = 0; k < plan->key.nst; k++) {
            const int stl = ((plan->key.stc[4 * k + 2] & 3) << 8) | plan->key.stc[4 * k + 3];
            o.out.emplace_back(below(4) ? new uint8_t[size_t(o.rows) * size_t(8 * stl)] : nullptr);
            o.out_ptr.push_back(o.out.back().get());
        }
    ed::HostOut h{};
    h.fib = o.fib.get();
    h.crc_ok = o.ok.get();
    h.status = o.status.get();
    h.result = &o.result;
    h.out = o.out_ptr.data();
    ed::read_entry(s.get(), tail + n, in, plan ? &plan->key : nullptr, h, o.state.get());
    CHECK(o.result.rows <= o.rows && o.result.tail_bytes <= uint32_t(ed::MAX_TAIL));
    ed::Head out{};
    std::memcpy(&out, o.state.get(), sizeof out);
    CHECK(out.tail_bytes == o.result.tail_bytes && out.last_dlfc < 5000);
    for (size_t i = out.tail_bytes; i < size_t(ed::MAX_PACKET); i++) CHECK(o.state[ed::STATE_HEAD_BYTES + i] == 0);
    for (uint32_t r = 0; r < o.result.rows; r++) {
        const ed::Status &st = o.status[r];
        CHECK(st.offset + st.length <= tail + n && st.dlfc < 5000 && st.gap < 5000 && st.length >= ed::MIN_ROW_PACKET);
    }
}

static void mutate(std::vector<uint8_t> &s) {
    const uint32_t n = 1 + below(6);
    for (uint32_t i = 0; i < n && !s.empty(); i++) {
        const size_t at = below(uint32_t(s.size()));
        switch (below(5)) {
        case 0: s[at] ^= uint8_t(1u << below(8)); break;
        case 1: s.erase(s.begin() + long(at), s.begin() + long(at + below(uint32_t(s.size() - at)) % 40)); break;
        case 2: s.insert(s.begin() + long(at), size_t(1 + below(30)), uint8_t(rnd())); break;
        case 3: if (at + 6 < s.size()) s[at + 2 + below(4)] = uint8_t(rnd()); break;             // (a LEN, if `at` is a header)
        default: s.resize(at); break;
        }
    }
}

int main(int argc, char **argv) {
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 100;
    const std::vector<uint8_t> zero_state(size_t(ed::STATE_BYTES), 0);
    for (int round = 0; round < rounds; round++) {
        const Plan plan = random_plan(), other = random_plan();
        std::vector<uint8_t> s;
        const uint32_t n_packets = 1 + below(12);
        uint32_t dlfc = below(5000), seq = below(65536);
        for (uint32_t i = 0; i < n_packets; i++) {
            append_packet(s, below(8) ? plan : other, seq++, dlfc);
            dlfc = (dlfc + 1 + (below(10) ? 0 : below(30))) % 5000;
            if (below(6) == 0) s.insert(s.end(), size_t(below(25)), uint8_t(rnd()));
        }
        if (round % 3) mutate(s);
        const Plan *use = round % 4 == 3 ? nullptr : &plan;
        // a state: a stream that starts, or anything at all
        std::vector<uint8_t> state = zero_state;
        if (round % 5 == 4)
            for (uint8_t &b : state) b = uint8_t(rnd());
        Outputs whole, a, b;
        run(state, s.data(), s.size(), use, whole);
        const size_t cut = below(uint32_t(s.size() + 1));
        run(state, s.data(), cut, use, a);
        const std::vector<uint8_t> mid(a.state.get(), a.state.get() + ed::STATE_BYTES);
        run(mid, s.data() + cut, s.size() - cut, use, b);
        CHECK(a.result.rows + b.result.rows == whole.result.rows);
        CHECK(a.result.skipped + b.result.skipped == whole.result.skipped && a.result.resyncs + b.result.resyncs == whole.result.resyncs);
        CHECK(a.result.not_deti + b.result.not_deti == whole.result.not_deti && a.result.bad_tags + b.result.bad_tags == whole.result.bad_tags);
        CHECK(a.result.other_plan + b.result.other_plan == whole.result.other_plan && a.result.gap_sum + b.result.gap_sum == whole.result.gap_sum);
        CHECK(std::memcmp(b.state.get(), whole.state.get(), size_t(ed::STATE_BYTES)) == 0);
        for (uint32_t r = 0; r < whole.result.rows; r++) {
            const Outputs &part = r < a.result.rows ? a : b;
            const uint32_t q = r < a.result.rows ? r : r - a.result.rows;
            CHECK(std::memcmp(whole.fib.get() + size_t(r) * 96, part.fib.get() + size_t(q) * 96, 96) == 0);
            CHECK(whole.status[r].dlfc == part.status[q].dlfc && whole.status[r].flags == part.status[q].flags && whole.status[r].gap == part.status[q].gap);
        }
    }
    // header-plausible every 10 bytes: at most n / 10 CRCs, every one of them fails, nothing is a row
    {
        std::vector<uint8_t> s;
        for (int i = 0; i < 2000; i++) {
            const uint8_t h[10] = {'A', 'F', 0, 0, uint8_t(i % 3 ? 0x0F : 0x00), uint8_t(0xA0 + i % 7), uint8_t(i >> 8), uint8_t(i), 0x90, 'T'};
            s.insert(s.end(), h, h + 10);
        }
        Outputs o;
        run(zero_state, s.data(), s.size(), nullptr, o);
        CHECK(o.result.rows == 0 && o.result.not_deti == 0 && o.result.bad_tags == 0 && o.result.resyncs == 0);
        CHECK(o.result.skipped + o.result.tail_bytes == s.size() && o.result.tail_bytes % 10 == 0 && o.result.tail_bytes > 0);
    }
    std::printf("edi_read_fuzz ok: %d rounds\n", rounds);
    return 0;
}
