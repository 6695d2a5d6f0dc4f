// dmb_fuzz.cpp -- include/dabgpu_dmb.h alone under AddressSanitizer and UBSan (tests/test_dmb.py builds and runs it):
//   dmb_fuzz rounds
// Every round makes a byte stream of a random bit rate -- random bytes with sync bytes sown in at stride 204 over random
// stretches, so that locks are made and lost at random phases -- and puts it through the header's serial receiver: once whole
// and once in random cuts (calls of no frames among them) from the same start, and once more in cuts with random undersized
// buffers (packets deferred through the state record).  Packets, records, the totals and the final
// state record have to agree.  Then once more from a random (hostile) state record, with the record's magic and bit rate
// right in every second round, for the sanitizers alone.  Rows lie at a random stride and every buffer has exactly the size the
// contract names, so that a byte too many is an error of the sanitizer.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "dabgpu_dmb.h"

namespace dmb = dabgpu_dmb;

static const dabgpu_packet_fec::Gf GF = dabgpu_packet_fec::make_gf();

struct Run {
    std::vector<uint8_t> ts;
    std::vector<dmb::Record> records;
    int32_t total[dmb::SUMMED_COUNTERS] = {};
    int lost = 0, deferred = 0;
    std::vector<uint8_t> state;
};

static void fail(const char *what, unsigned round) {
    std::printf("dmb_fuzz FAILED: %s (round %u)\n", what, round);
    std::exit(1);
}

// one call of n frames on buffers of exactly the contract's sizes; appends to run
static void call(Run &run, const std::vector<uint8_t> &stream, size_t first_frame, int n, int kbps, size_t stride, unsigned round, int room = -1) {
    const size_t fb = size_t(dmb::frame_bytes(kbps));
    std::vector<uint8_t> rows(n ? (size_t(n) - 1) * stride + fb : 0);
    for (int f = 0; f < n; f++) std::memcpy(rows.data() + size_t(f) * stride, stream.data() + (first_frame + size_t(f)) * fb, fb);
    if (room < 0) room = dmb::max_packets(kbps, n);
    std::vector<uint8_t> ts(size_t(room) * dmb::TS_BYTES);
    std::vector<dmb::Record> records(static_cast<size_t>(room));
    alignas(16) static uint8_t state_in[dmb::STATE_BYTES], state_out[dmb::STATE_BYTES];
    if (!run.state.empty()) std::memcpy(state_in, run.state.data(), sizeof state_in);
    dmb::Result r;
    dmb::process(GF, run.state.empty() ? nullptr : state_in, state_out, r, rows.data(), stride, n, kbps, ts.data(), records.data(), room);
    if (r.packets_deferred < 0 || r.packets_deferred > dmb::DEFER_ROOM || r.packets_lost < 0) fail("deferred or lost out of range", round);
    run.lost += r.packets_lost;
    run.deferred = r.packets_deferred;
    if (r.packets_emitted < 0 || r.packets_emitted > room) fail("more packets than max_packets", round);
    if (r.packets_clean + r.packets_corrected + r.packets_uncorrectable != r.packets_emitted) fail("statuses do not add up", round);
    run.ts.insert(run.ts.end(), ts.begin(), ts.begin() + size_t(r.packets_emitted) * dmb::TS_BYTES);
    run.records.insert(run.records.end(), records.begin(), records.begin() + r.packets_emitted);
    for (int i = 0; i < dmb::SUMMED_COUNTERS; i++) run.total[i] += reinterpret_cast<const int32_t *>(&r)[i];
    run.state.assign(state_out, state_out + sizeof state_out);
}

int main(int argc, char **argv) {
    const unsigned rounds = argc > 1 ? unsigned(std::atoi(argv[1])) : 20;
    for (unsigned round = 0; round < rounds; round++) {
        std::mt19937 rng(round * 7919u + 1u);
        auto below = [&](unsigned n) { return unsigned(rng() % n); };
        const int rates[] = {8, 16, 128, 136, 544, 1824};
        const int kbps = rates[below(6)];
        const size_t fb = size_t(dmb::frame_bytes(kbps));
        const int n_frames = int(30000 / fb) + 1 + int(below(8));
        std::vector<uint8_t> stream(size_t(n_frames) * fb);
        for (auto &b : stream) b = uint8_t(rng());
        for (size_t at = below(500); at < stream.size();) {               // stretches of sync bytes at one phase
            const size_t len = 204 * (1 + below(40));
            for (size_t p = at; p < at + len && p < stream.size(); p += 204)
                if (below(8)) stream[p] = dmb::SYNC_BYTE;
            at += len + below(3000);
        }
        const size_t stride = fb + below(40);
        Run whole, cut, hostile;
        call(whole, stream, 0, n_frames, kbps, stride, round);
        for (int at = 0; at < n_frames;) {
            const int n = below(4) == 0 ? 0 : int(1 + below(unsigned(n_frames - at)));
            call(cut, stream, size_t(at), n, kbps, stride, round);
            at += n;
        }
        call(cut, stream, size_t(n_frames), 0, kbps, stride, round);
        // once more in cuts with random undersized buffers, then calls of no frames until nothing is deferred: the same again,
        // unless a packet found no place (which the counters have to say)
        Run small;
        for (int at = 0; at < n_frames;) {
            const int n = below(4) == 0 ? 0 : int(1 + below(unsigned(n_frames - at)));
            call(small, stream, size_t(at), n, kbps, stride, round, int(below(unsigned(dmb::max_packets(kbps, n)) + 1u)));
            at += n;
        }
        for (int k = 0; k < 3 && (small.deferred || k == 0); k++) call(small, stream, size_t(n_frames), 0, kbps, stride, round, dmb::DEFER_ROOM);
        if (small.deferred) fail("deferred packets left after a call with room for them", round);
        if (whole.lost) fail("a packet lost with room for everything", round);
        if (!small.lost) {
            if (whole.ts != small.ts || whole.records.size() != small.records.size() ||
                std::memcmp(whole.records.data(), small.records.data(), whole.records.size() * sizeof(dmb::Record)) != 0)
                fail("packets or records differ between full and undersized buffers", round);
            if (std::memcmp(whole.total, small.total, sizeof whole.total) != 0 || whole.state != small.state)
                fail("totals or state differ between full and undersized buffers", round);
        } else if (small.ts.size() + size_t(small.lost) * dmb::TS_BYTES != whole.ts.size()) {
            fail("emitted and lost packets do not add up", round);
        }
        if (whole.ts != cut.ts) fail("packets differ between one call and cuts", round);
        if (whole.records.size() != cut.records.size() ||
            std::memcmp(whole.records.data(), cut.records.data(), whole.records.size() * sizeof(dmb::Record)) != 0)
            fail("records differ between one call and cuts", round);
        if (std::memcmp(whole.total, cut.total, sizeof whole.total) != 0) fail("totals differ between one call and cuts", round);
        if (whole.state != cut.state) fail("state records differ between one call and cuts", round);
        hostile.state.resize(size_t(dmb::STATE_BYTES));
        for (auto &b : hostile.state) b = uint8_t(rng());
        if (round & 1) {
            dmb::Head h;
            dmb::head_fresh(h, kbps);
            h.pos = int64_t(rng()) << below(25);
            h.locked = uint8_t(below(2));
            h.lock_start = h.locked ? int64_t(rng() % uint64_t(h.pos + 1)) : 0;
            h.misses = uint8_t(h.locked ? below(8) : 0);
            h.n_pids = uint8_t(below(33));
            h.pids_overflowed = h.n_pids == dmb::CENSUS ? uint32_t(rng()) : 0u;
            h.n_deferred = below(unsigned(dmb::DEFER_ROOM) + 1u);
            std::memcpy(hostile.state.data(), &h, sizeof h);
        }
        call(hostile, stream, 0, n_frames / 2, kbps, stride, round);
        call(hostile, stream, size_t(n_frames / 2), n_frames - n_frames / 2, kbps, stride, round);
    }
    std::printf("dmb_fuzz ok: %u rounds\n", rounds);
    return 0;
}
