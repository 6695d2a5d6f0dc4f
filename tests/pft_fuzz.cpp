// pft_fuzz.cpp -- include/dabgpu_pft.h alone under AddressSanitizer and UBSan (tests/test_pft.py builds and runs it):
//   pft_fuzz rounds
// Every round makes a stream of PF fragments from the header's writer (a random layout, with and without FEC and Addr),
// damages it (fragments dropped, doubled, swapped, bytes flipped, bytes removed, garbage put between, headers made to
// disagree), and reads it with the header's serial reader: once whole and once in random pieces from the same start -- the
// records, the output and the totals have to agree -- and once more from a random (hostile) state record.  Outputs lie in
// buffers of exactly the sizes the contract names, so that a byte too many is an error of the sanitizer.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "dabgpu_pft.h"

namespace pf = dabgpu_pft;

static const pf::Gf GF = pf::make_gf();
static const pf::ParityTable PT = pf::make_parity_table();

struct Run {
    std::vector<pf::Record> records;
    std::vector<uint8_t> out;
    pf::Result total{};
    std::vector<uint8_t> state;
};

static void fail(const char *what, unsigned round) {
    std::printf("pft_fuzz FAILED: %s (round %u)\n", what, round);
    std::exit(1);
}

// one call on buffers of exactly the contract's sizes; appends to run
static void call(Run &run, const uint8_t *bytes, size_t n, bool flush, unsigned round) {
    std::vector<uint8_t> state_out(static_cast<size_t>(pf::STATE_BYTES), 0xEE), scratch(static_cast<size_t>(pf::MAX_BLOCK), 0);
    const uint8_t *state_in = run.state.empty() ? nullptr : run.state.data();
    pf::Head in{};
    if (state_in) std::memcpy(&in, state_in, sizeof in);
    const size_t tail = pf::clamp_tail(in.tail_bytes);
    std::vector<uint8_t> s(tail + n);
    if (tail) std::memcpy(s.data(), state_in + pf::STATE_TAIL_AT, tail);
    if (n) std::memcpy(s.data() + tail, bytes, n);
    std::vector<uint8_t> out(static_cast<size_t>(pf::read_out_bytes(uint32_t(n))), 0);
    std::vector<pf::Record> records(pf::read_max_records(uint32_t(n)));
    pf::Result r{};
    pf::read_entry(GF, s.data(), s.size(), state_in, flush ? uint32_t(pf::READ_FLUSH) : 0u, out.data(), records.data(), uint32_t(records.size()), &r,
                   state_out.data(), scratch.data());
    if (r.records > records.size() || r.out_bytes > out.size() || r.tail_bytes > uint32_t(pf::MAX_TAIL)) fail("a count beyond its bound", round);
    uint32_t at = 0;
    for (uint32_t i = 0; i < r.records; i++) {
        pf::Record rec = records[i];
        if (rec.offset != at || ((rec.flags & pf::FLAG_LOST) != 0) != (rec.length == 0)) fail("record offsets", round);
        at += rec.length;
        rec.offset += uint32_t(run.out.size());
        run.records.push_back(rec);
    }
    if (at != r.out_bytes) fail("out_bytes", round);
    run.out.insert(run.out.end(), out.begin(), out.begin() + r.out_bytes);
    uint32_t *t = reinterpret_cast<uint32_t *>(&run.total);
    const uint32_t *c = reinterpret_cast<const uint32_t *>(&r);
    for (size_t i = 0; i < sizeof r / 4; i++) t[i] += c[i];
    run.total.tail_bytes = r.tail_bytes;
    run.state = state_out;
}

int main(int argc, char **argv) {
    const unsigned rounds = argc > 1 ? unsigned(std::atoi(argv[1])) : 100;
    std::mt19937 rng(12345);
    const auto pick = [&](uint32_t n) { return n ? uint32_t(rng() % n) : 0u; };
    unsigned long long packets = 0, recovered = 0, lost = 0;
    for (unsigned round = 0; round < rounds; round++) {
        // a stream of a few packets
        std::vector<std::vector<uint8_t>> frags;
        const int n_packets = 1 + int(pick(6));
        uint32_t pseq = pick(4) ? pick(65536) : 65534u;
        for (int n = 0; n < n_packets; n++) {
            pf::Layout a;
            const int sizes[] = {12, 13, 140, 207, 208, 415, 1000, 2476, 8192};
            const int l = pick(3) ? sizes[pick(9)] : 12 + int(pick(3000));
            const int fec = pick(4) != 0, m = int(pick(6)), addr = pick(3) == 0;
            const int max_payload = fec ? 1400 : 30 + int(pick(1400));
            if (!pf::layout(l, fec, m, max_payload, addr, a)) continue;
            std::vector<uint8_t> af(static_cast<size_t>(l), 0), all(static_cast<size_t>(a.stream_bytes), 0), block(static_cast<size_t>(a.block_bytes) + 1, 0);
            for (auto &b : af) b = uint8_t(rng());
            if (pick(2)) {                                   // ... a real AF packet
                af[0] = 'A', af[1] = 'F', af[2] = af[3] = 0, af[4] = uint8_t((l - 12) >> 8), af[5] = uint8_t(l - 12), af[8] = 0x90, af[9] = 'T';
                uint32_t crc = 0xFFFF;
                for (int i = 0; i < l - 2; i++) crc = pf::crc_byte(crc, af[size_t(i)]);
                crc ^= 0xFFFF;
                af[size_t(l) - 2] = uint8_t(crc >> 8), af[size_t(l) - 1] = uint8_t(crc);
            }
            pf::write_fragments(GF, PT, a, pseq, 0x1234, 0x5678, [&](int i) -> unsigned { return af[size_t(i)]; },
                                [&](int i, uint8_t b) { all[size_t(i)] = b; }, block.data());
            pseq = (pseq + (pick(8) ? 1u : 1u + pick(5))) & 0xFFFFu;
            const int fb = a.header_bytes + a.plen;
            for (int g = 0; g < a.fcount; g++) {
                const size_t from = size_t(g) * size_t(fb), to = g + 1 < a.fcount ? from + size_t(fb) : all.size();
                frags.emplace_back(all.begin() + std::ptrdiff_t(from), all.begin() + std::ptrdiff_t(to));
            }
        }
        // damage
        const uint32_t hits = pick(8);
        for (uint32_t h = 0; h < hits && !frags.empty(); h++) {
            const size_t i = pick(uint32_t(frags.size()));
            switch (frags[i].empty() ? 0u : pick(8)) {
            case 0: frags.erase(frags.begin() + std::ptrdiff_t(i)); break;
            case 1: frags.insert(frags.begin() + std::ptrdiff_t(i), frags[i]); break;
            case 2: std::swap(frags[i], frags[pick(uint32_t(frags.size()))]); break;
            case 3: frags[i][pick(uint32_t(frags[i].size()))] ^= uint8_t(1u << pick(8)); break;
            case 4: frags[i].erase(frags[i].begin() + std::ptrdiff_t(pick(uint32_t(frags[i].size())))); break;
            case 5: {
                std::vector<uint8_t> junk(pick(40));
                for (auto &b : junk) b = pick(4) ? uint8_t(rng()) : uint8_t("PF"[pick(2)]);
                frags.insert(frags.begin() + std::ptrdiff_t(i), junk);
                break;
            }
            case 6: frags[i].resize(pick(uint32_t(frags[i].size()) + 1)); break;
            default: {                                       // another Fcount, with a good HCRC again
                std::vector<uint8_t> &f = frags[i];
                pf::FragHeader fh;
                if (f.size() >= 20 && pf::header_ok(pf::PtrBytes{f.data()}, 20, fh)) {
                    fh.fcount = fh.findex + 1 + pick(3);
                    pf::write_header([&](int k, uint8_t b) { f[size_t(k)] = b; }, fh);
                }
            }
            }
        }
        std::vector<uint8_t> stream;
        for (const auto &f : frags) stream.insert(stream.end(), f.begin(), f.end());

        Run whole, pieces;
        call(whole, stream.data(), stream.size(), true, round);
        for (size_t at = 0;;) {
            const size_t n = std::min<size_t>(pick(3) ? pick(600) : pick(9000), stream.size() - at);
            const bool last = at + n == stream.size();
            call(pieces, stream.data() + at, n, last, round);
            at += n;
            if (last) break;
        }
        if (whole.records.size() != pieces.records.size() ||
            (!whole.records.empty() && std::memcmp(whole.records.data(), pieces.records.data(), whole.records.size() * sizeof(pf::Record))))
            fail("records depend on the cuts", round);
        if (whole.out != pieces.out) fail("output depends on the cuts", round);
        if (std::memcmp(&whole.total, &pieces.total, sizeof whole.total)) fail("totals depend on the cuts", round);
        packets += whole.total.packets, recovered += whole.total.recovered, lost += whole.total.lost;

        // a hostile state record in front of the same stream: anything may come out, nothing may be touched outside
        Run hostile;
        hostile.state.resize(size_t(pf::STATE_BYTES));
        for (auto &b : hostile.state) b = pick(3) ? uint8_t(rng()) : uint8_t(pick(3));
        if (pick(2)) std::memcpy(hostile.state.data(), whole.state.data(), size_t(pf::STATE_HEAD_BYTES));
        if (pick(2)) {                                        // group heads that nearly pass
            pf::GroupHead g{};
            g.kind = uint8_t(1 + pick(2)), g.fec = uint8_t(pick(2)), g.have_s = 1, g.fcount = uint16_t(1 + pick(300)), g.s = uint16_t(pick(9000));
            g.pseq = uint16_t(pick(65536)), g.received = uint16_t(pick(300)), g.rs_k = uint8_t(pick(256)), g.chunks = uint8_t(pick(60));
            g.length = uint16_t(pick(9000)), g.last_len = uint16_t(pick(9000)), g.map[pick(4)] = (uint64_t(rng()) << 32) | rng();
            std::memcpy(hostile.state.data() + pf::STATE_GROUPS_AT + pick(2) * pf::GROUP_BYTES, &g, sizeof g);
        }
        call(hostile, stream.data(), stream.size(), pick(2) != 0, round);
        call(hostile, nullptr, 0, true, round);
    }
    std::printf("pft_fuzz ok: %u rounds, %llu packets, %llu recovered, %llu lost\n", rounds, packets, recovered, lost);
    return 0;
}
