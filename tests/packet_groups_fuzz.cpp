// packet_groups_fuzz.cpp -- include/dabgpu_data_groups.h on its own, under the host compiler's sanitizers
// (tests/test_packet_groups.py builds this with -fsanitize=address,undefined and runs it): N calls of the serial walk, the twin
// of the kernel, on logical frames of random bit rates -- random bytes, and valid packets (data groups with every header
// option, good, absent and wrong CRCs, lengths up to beyond the cap, cut into packets of one address beside padding and other
// addresses) with continuity indices skipped, lengths that lie, command packets and bits changed.  The frames of a call, both
// state records, d_bytes and d_groups are heap blocks of exactly their size, so a read or write outside is reported; the
// state runs on from call to call and is now and then replaced by random bytes or has bits changed.  What was emitted is
// held to the contract's own bounds.
#include "dabgpu_data_groups.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <random>
#include <vector>

namespace dg = dabgpu_groups;
namespace pad = dabgpu_pad;
typedef std::vector<uint8_t> Bytes;

static std::mt19937_64 rng(0xDA7A6209);
static int below(int n) { return int(rng() % uint64_t(n)); }
static void put_crc(Bytes &g) {
    const uint32_t crc = pad::crc16(g.data(), int(g.size()));
    g.push_back(uint8_t(crc >> 8));
    g.push_back(uint8_t(crc));
}

#define REQUIRE(cond)                                                          \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::printf("line %d: %s\n", __LINE__, #cond);                     \
            std::exit(5);                                                      \
        }                                                                      \
    } while (0)

static const int ADDRESS = 37;
static std::deque<Bytes> queue;                                        // packets of ADDRESS waiting to be sent
static int next_ci = 0;
static bool quiet = false;                                             // (a group near the cap is sent as it is: else none would get there)

static Bytes packet(int address, const uint8_t *data, int n, int slots, bool first, bool last) {
    const int odd = quiet ? 1000 : below(150);
    Bytes p = {uint8_t(((slots - 1) << 6) | ((next_ci & 3) << 4) | (first << 3) | (last << 2) | (address >> 8)), uint8_t(address),
               uint8_t(((odd == 0) << 7) | ((odd == 1 ? n + 1 + below(40) : n) & 0x7F))};
    if (address == ADDRESS) next_ci += odd == 2 ? 2 : 1;
    p.insert(p.end(), data, data + n);
    p.resize(size_t(24 * slots - 2), uint8_t(rng()));
    put_crc(p);
    if (odd == 3) p[size_t(below(int(p.size())))] ^= uint8_t(1 << below(8));
    return p;
}

static void send_group(const Bytes &g) {
    for (size_t at = 0;;) {
        const int slots = quiet ? 4 : 1 + below(4), room = 24 * slots - 5;
        const int take = !quiet && below(12) == 0 ? 0 : int(std::min<size_t>(size_t(room), g.size() - at));
        const bool last = at + size_t(take) == g.size() && below(40) != 0;
        queue.push_back(packet(ADDRESS, g.data() + at, take, slots, at == 0 && below(40) != 0, last));
        at += size_t(take);
        if (last || at > g.size() + 100) break;
    }
}

static void make_group() {
    const int kind = below(40);
    int n = kind == 0 ? 16300 + below(200) : kind < 4 ? below(6) : below(kind < 30 ? 200 : 3000);
    const int flags = below(16);                                       // extension, CRC, segment, user access
    Bytes g = {uint8_t((flags << 4) | below(below(3) ? 3 : 16)), uint8_t((below(below(2) ? 2 : 16) << 4) | below(16))};
    if (flags & 8) g.insert(g.end(), {uint8_t(rng()), uint8_t(rng())});
    if (flags & 2) g.insert(g.end(), {uint8_t(rng()), uint8_t(rng())});
    if (flags & 1) {
        const int li = below(16), tid = below(2);
        g.push_back(uint8_t((below(8) << 5) | (tid << 4) | li));
        for (int i = 0, m = below(10) ? li : below(16); i < m; i++) g.push_back(uint8_t(rng()));
    }
    if (below(12) == 0) g.resize(size_t(below(int(g.size()) + 1)));
    for (int i = 0; i < n; i++) g.push_back(uint8_t(rng()));
    if (flags & 4) {
        put_crc(g);
        if (below(10) == 0) g[size_t(below(int(g.size())))] ^= uint8_t(1 << below(8));
    }
    quiet = kind == 0;
    send_group(g);
    quiet = false;
}

int main(int argc, char **argv) {
    const long n_calls = argc > 1 ? std::atol(argv[1]) : 2000;
    dg::Counters total = {};
    long fresh_starts = 0, carried_open = 0;
    bool tainted = false;                                              // the open group's bytes or register were changed from outside
    std::unique_ptr<uint8_t[]> state(new uint8_t[sizeof(dg::State) + 16]);
    auto aligned = [](uint8_t *p) { return p + (16 - (reinterpret_cast<uintptr_t>(p) & 15)) % 16; };
    std::memset(aligned(state.get()), 0, sizeof(dg::State));
    for (long call_no = 0; call_no < n_calls; call_no++) {
        const int S = 1 + below(below(4) ? 12 : 64), n_cifs = below(6), stride = 24 * S + below(3) * 7;
        // the frames: one heap block of exactly n_cifs rows
        Bytes frames(size_t(n_cifs) * size_t(stride), 0);
        for (int k = 0; k < n_cifs; k++) {
            uint8_t *row = frames.data() + size_t(k) * size_t(stride);
            if (below(15) == 0) {
                for (int i = 0; i < 24 * S; i++) row[i] = uint8_t(rng());
                continue;
            }
            for (int pos = 0; pos < S;) {
                while (queue.empty()) make_group();
                const int what = below(10);
                Bytes p;
                if (what < 7 && int(queue.front().size()) / 24 <= S - pos) {
                    p = queue.front();
                    queue.pop_front();
                } else {
                    const int slots = 1 + below(std::min(4, S - pos));
                    p = packet(what == 7 ? 1 + below(1023) : 0, nullptr, 0, slots, true, true);
                }
                std::memcpy(row + 24 * pos, p.data(), p.size());
                pos += int(p.size()) / 24;
            }
        }
        // the state going in: the one that came out, or random bytes, or that one with bits changed
        std::unique_ptr<uint8_t[]> state_out(new uint8_t[sizeof(dg::State) + 16]);
        uint8_t *in = aligned(state.get()), *out = aligned(state_out.get());
        const int spoil = below(60);
        if (spoil == 0)
            for (size_t i = 0; i < sizeof(dg::State); i++) in[i] = uint8_t(rng());
        else if (spoil == 1)
            in[size_t(below(40))] ^= uint8_t(1 << below(8));
        tainted = tainted || spoil < 2;
        dg::Call call = {};
        // (mode 1 forgets an open group: mostly between groups, so that long ones get through)
        call.mode = below(dg::read_head(reinterpret_cast<const dg::State *>(in), 0).open ? 200 : 6) == 0;
        call.keep_repeats = below(2);
        call.bytes_capacity = below(3) ? 20000 : below(600);
        call.max_groups = below(3) ? 64 : below(4);
        Bytes bytes(size_t(call.bytes_capacity), 0xA7);
        std::vector<dg::Record> groups(size_t(call.max_groups), dg::Record{});
        call.bytes = bytes.data();
        call.groups = groups.data();
        const dg::Head before = dg::read_head(reinterpret_cast<const dg::State *>(in), call.mode);
        fresh_starts += !before.seen;
        carried_open += before.open;
        dg::Counters c = {};
        dg::walk_frames(reinterpret_cast<const dg::State *>(in), reinterpret_cast<dg::State *>(out), c, call,
                        frames.data(), uint64_t(stride), n_cifs, S, ADDRESS, below(2));
        // what the contract bounds
        REQUIRE(c.cifs == n_cifs && c.slots == n_cifs * S);
        REQUIRE(c.groups_emitted >= 0 && c.groups_emitted <= call.max_groups && c.bytes_emitted <= call.bytes_capacity);
        uint32_t at = 0;
        for (int i = 0; i < c.groups_emitted && !call.mode; i++) {
            const dg::Record &r = groups[size_t(i)];
            REQUIRE(uint32_t(r.offset) == at && r.length >= 4 && r.length <= dg::GROUP_CAP && r.offset + r.length <= call.bytes_capacity);
            REQUIRE(r.data_offset + r.data_length + ((r.flags & dg::DG_CRC) ? 2 : 0) == r.length && r.cif >= 0 && r.cif < n_cifs && r.slot < S);
            REQUIRE(bytes[size_t(r.offset)] % 16 == r.type && ((r.flags & dg::DG_REPEAT) == 0 || call.keep_repeats));
            if ((r.flags & dg::DG_CRC) && !tainted) REQUIRE(pad::crc16(bytes.data() + r.offset, r.length - 2) == uint32_t((bytes[size_t(r.offset + r.length - 2)] << 8) | bytes[size_t(r.offset + r.length - 1)]));
            at = dg::offset_add(at, dg::round16(uint32_t(r.length)));
        }
        if (!call.mode) {
            REQUIRE(c.groups_closed == c.groups_malformed + c.groups_crc_failed + c.groups_emitted + c.groups_no_room +
                                           (call.keep_repeats ? 0 : c.groups_repeated));
        } else {
            REQUIRE(c.groups_emitted + c.groups_no_room == c.continuity_breaks && c.groups_closed == 0 && c.group_bytes == 0);
        }
        const dg::State *st = reinterpret_cast<const dg::State *>(out);
        tainted = tainted && st->open;
        REQUIRE(st->seen <= 1 && st->prev <= 3 && st->open <= 1 && st->have <= dg::GROUP_CAP && (!call.mode || !st->open));
        for (int i = st->have; i < dg::GROUP_CAP; i++) REQUIRE(st->group[i] == 0);
        const dg::Head again = dg::read_head(st, 0);
        REQUIRE(again.seen == st->seen && again.open == st->open && again.have == st->have);   // (what it wrote it takes back)
        const int32_t *v = reinterpret_cast<const int32_t *>(&c);
        int32_t *t = reinterpret_cast<int32_t *>(&total);
        for (size_t i = 0; i < sizeof c / 4; i++) t[i] += v[i];
        state.swap(state_out);
    }
    std::printf("calls=%ld groups_emitted=%d groups_crc_failed=%d groups_malformed=%d groups_repeated=%d groups_too_long=%d groups_no_room=%d "
                "continuity_breaks=%d bytes_no_room=%d fresh_starts=%ld carried_open=%ld groups_no_crc=%d packets_orphan=%d\n",
                n_calls, total.groups_emitted, total.groups_crc_failed, total.groups_malformed, total.groups_repeated, total.groups_too_long,
                total.groups_no_room, total.continuity_breaks, total.bytes_no_room, fresh_starts, carried_open, total.groups_no_crc, total.packets_orphan);
    return 0;
}
