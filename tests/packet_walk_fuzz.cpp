// packet_walk_fuzz.cpp -- include/dabgpu_packet_walk.h on its own, under the host compiler's sanitizers (tests/test_packet.py
// builds this with -fsanitize=address,undefined and runs it): N logical frames of random bit rates -- random bytes, and valid
// packets (MOT objects in data groups cut into packets of one address, beside padding, other addresses and FEC-shaped
// slots) with bytes changed, lengths and useful data lengths wrong, continuity broken -- each frame a heap block of exactly
// its size; the arena and the slide slots are heap blocks of exactly their size, too.  The scan and the walk run as the
// kernels run them (verdict per slot, chain, followed packets), the copy orders are executed with their bounds asserted
// first.  The state runs on from frame to frame; a "call" ends every 16 frames (counters and slots start again, the state
// goes through sanitize()); now and then the state is replaced by random bytes, or the arena by one of another size.
#include "dabgpu_packet_walk.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <random>
#include <vector>

namespace mot = dabgpu_mot;
namespace pad = dabgpu_pad;
namespace pkt = dabgpu_packet;
typedef std::vector<uint8_t> Bytes;

static std::mt19937_64 rng(0xFACE7);
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
static bool calm = false;                                              // the packets being made are left as they should be
static long calm_left = 0;                                             // ... and that many of them wait at the front of the queue
static int S = 8;                                                      // slots of a frame, until the bit rate changes

static Bytes packet(int address, const uint8_t *data, int n, int slots, bool first, bool last) {
    const int odd = calm ? 99 : below(40);
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
    for (size_t at = 0; at < g.size() || at == 0;) {
        const int slots = calm ? (S < 4 ? S : 4) : 1 + below(4), room = 24 * slots - 5;
        const int take = int(g.size() - at) < room ? int(g.size() - at) : room;
        const bool last = at + size_t(take) == g.size();
        queue.push_back(packet(ADDRESS, g.data() + at, take, slots, (at == 0) != (!calm && below(50) == 0), last != (!calm && below(50) == 0)));
        at += size_t(take);
        if (last) break;
    }
}

static void next_object(int body_capacity) {
    const int tid = below(6) ? int(rng() & 0xFFFF) : 7, hbytes = 7 + below(below(8) ? 40 : 1100), big = below(12) == 0;
    const int bbytes = big ? below(body_capacity + 40) : below(300), hseg = 1 + below(below(4) ? 64 : 1200), bseg = 1 + below(big ? 8191 : 96);
    Bytes header, body;
    header.resize(size_t(hbytes));
    body.resize(size_t(bbytes));
    for (uint8_t &v : header) v = uint8_t(rng());
    for (uint8_t &v : body) v = uint8_t(rng());
    const int hsays = below(16) ? hbytes : hbytes + 1, bsays = below(16) ? bbytes : bbytes + 1;
    header[0] = uint8_t(bsays >> 20); header[1] = uint8_t(bsays >> 12); header[2] = uint8_t(bsays >> 4);
    header[3] = uint8_t(((bsays & 15) << 4) | (hsays >> 9)); header[4] = uint8_t(hsays >> 1); header[5] = uint8_t(((hsays & 1) << 7) | (header[5] & 0x7F));
    for (int part = 0; part < 2; part++) {
        const Bytes &d = part ? body : header;
        const int size = part ? bseg : hseg, n = d.empty() ? 1 : int((d.size() + size_t(size) - 1) / size_t(size));
        for (int k = 0; k < n; k++) {
            const int at = k * size, z = int(d.size()) - at < size ? int(d.size()) - at : size, odd = below(30);
            Bytes g = {uint8_t(((odd != 0) << 6) | ((odd != 1) << 5) | ((odd != 2) << 4) | (odd == 3 ? 6 : 3 + part)), uint8_t(rng())};
            if (odd != 1) { g.push_back(uint8_t(((k == n - 1) << 7) | (k >> 8))); g.push_back(uint8_t(k)); }
            if (odd != 2) { g.push_back(0x12); g.push_back(uint8_t(tid >> 8)); g.push_back(uint8_t(tid)); }
            const int says = odd == 4 ? z + 1 : z;
            g.push_back(uint8_t(says >> 8));
            g.push_back(uint8_t(says));
            g.insert(g.end(), d.begin() + at, d.begin() + at + z);
            put_crc(g);
            send_group(g);
            if (below(8) == 0) send_group(g);                          // a repetition
        }
    }
    if (below(10) == 0) {                                              // very short groups
        Bytes g(size_t(below(6)), uint8_t(0x46));
        send_group(g);
    }
    if (below(25) == 0 && calm_left == 0) {                            // the longest group there may be, or a longer one: sent undisturbed
        while (!queue.empty()) queue.pop_front();
        Bytes g(size_t(16384 - 2 + below(2) * (1 + below(200))), uint8_t(0x46));
        put_crc(g);
        calm = true;
        send_group(g);
        calm = false;
        calm_left = long(queue.size());
    }
}

int main(int argc, char **argv) {
    const long frames = argc > 1 ? atol(argv[1]) : 60000;
    pkt::State st;
    std::memset(&st, 0, sizeof st);
    pkt::Counters c{}, all{};
    mot::Orders ord;
    mot::Call call{};
    uint8_t *arena = nullptr, *slides = nullptr;
    size_t arena_size = 0, slides_size = 0;
    long orders = 0, checked = 0;
    int fec = 0;
    for (long w = 0; w < frames; w++) {
        if (w % 16 == 0) {                                            // the next call
            for (size_t i = 0; i < sizeof(pkt::Counters) / 4; i++) reinterpret_cast<int32_t *>(&all)[i] += reinterpret_cast<int32_t *>(&c)[i];
            std::memset(&c, 0, sizeof c);
            if (!arena || below(40) == 0) {                           // another arena (and what the state says no longer goes with it)
                std::free(arena);
                call.body_capacity = below(3) ? 16 * below(64) : 8191 + below(2000);
                arena_size = size_t(mot::arena_bytes(call.body_capacity));
                call.body_capacity = mot::body_capacity_of(arena_size);
                arena = static_cast<uint8_t *>(std::malloc(arena_size));
                if (!arena) return 2;
                std::memset(arena, 0xA7, arena_size);
            }
            std::free(slides);
            call.max_slides = below(4);
            call.slide_stride = uint32_t(16 * (2 + below(below(4) ? 80 : 700)));
            slides_size = size_t(call.max_slides) * call.slide_stride;
            slides = static_cast<uint8_t *>(std::malloc(slides_size ? slides_size : 1));
            if (!slides) return 2;
            if (below(20) == 0 && calm_left == 0) {
                uint8_t *b = reinterpret_cast<uint8_t *>(&st);
                if (below(2)) for (size_t i = 0; i < sizeof st; i++) b[i] = uint8_t(rng());
                else for (int k = 1 + below(4); k > 0; k--) b[size_t(below(int(sizeof st)))] ^= uint8_t(1 << below(8));
            }
            pkt::sanitize(st, call.body_capacity);
            if (below(4) == 0 && calm_left == 0) S = below(3) ? 1 + below(12) : 1 + below(64);
            fec = below(3) == 0;
        }
        // the frame: a heap block of exactly 24 S bytes
        uint8_t *frame = static_cast<uint8_t *>(std::malloc(size_t(24 * S)));
        if (!frame) return 2;
        const int how = calm_left > 0 ? 2 : below(12);
        if (how == 0) {
            for (int i = 0; i < 24 * S; i++) frame[i] = uint8_t(rng());
        } else {
            int pos = 0;
            while (pos < S) {
                if (queue.empty()) next_object(call.body_capacity);
                const int kind = calm_left > 0 && S - pos >= 4 ? 3 : below(8);
                Bytes p;
                if (kind == 0) {
                    p = packet(0, nullptr, 0, 1 + below(4), false, false);
                } else if (kind == 1) {
                    uint8_t d[19];
                    for (uint8_t &v : d) v = uint8_t(rng());
                    p = packet(below(2) ? 1022 : 1 + below(1023), d, 19, 1, true, true);
                } else if (kind == 2 && fec) {
                    p.assign(24, uint8_t(rng()));
                    p[0] = uint8_t(0x03 | (below(4) << 4));
                    p[1] = 0xFE;
                } else {
                    p = queue.front();
                    const bool fits = pos + int(p.size()) / 24 <= S;
                    if (calm_left > 0 && !fits) {                      // (an undisturbed packet waits for a frame with room for it)
                        p = packet(0, nullptr, 0, 1, false, false);
                    } else if (fits || below(6) == 0) {
                        queue.pop_front();
                        calm_left -= calm_left > 0;
                    }
                }
                const int n = int(p.size()) < 24 * (S - pos) ? int(p.size()) : 24 * (S - pos);     // (one that overruns is cut off)
                std::memcpy(frame + 24 * pos, p.data(), size_t(n));
                pos += n / 24;
            }
            if (how == 1) for (int k = 1 + below(3); k > 0; k--) frame[below(24 * S)] = uint8_t(rng());
        }
        // scan as the kernel scans: a verdict per slot, then the chain
        uint32_t verdicts[pkt::MAX_SLOTS];
        for (int pos = 0; pos < S; pos++) verdicts[pos] = pkt::slot_verdict(frame, S, pos, fec);
        pkt::FrameTally t = {};
        call.superframe = int(w % 16);
        pkt::resolve_chain(
            S, ADDRESS, t, [&](int pos) { return verdicts[pos]; },
            [&](int pos, int L) {
                REQUIRE(pos >= 0 && L >= 1 && L <= 4 && pos + L <= S);
                const int need = pkt::packet_read_bytes(L, frame[24 * pos + 2]);
                REQUIRE(need >= 3 && need <= 24 * L - 2);
                uint8_t *block = static_cast<uint8_t *>(std::malloc(size_t(need)));      // what the walk kernel stages, exactly
                if (!block) std::exit(2);
                std::memcpy(block, frame + 24 * pos, size_t(need));
                call.au = pos;
                const int before = c.mot.slides_written;
                pkt::follow_packet(st, c, ord, call, block, L);
                REQUIRE(ord.n >= 0 && ord.n <= mot::MAX_ORDERS);
                int records = 0;
                for (int i = 0; i < ord.n; i++) {
                    const mot::Order &o = ord.o[i];
                    orders++;
                    if (o.kind == pkt::ORDER_PACKET) {
                        REQUIRE(i == 0 && o.len > 0 && o.src == 3 && o.src + o.len <= need && uint64_t(o.dst) + uint64_t(o.len) <= uint64_t(mot::GROUP_CAP));
                    } else if (o.kind == mot::ORDER_MOVE) {
                        REQUIRE(o.len > 0 && o.src >= 0 && o.src + o.len <= mot::GROUP_CAP && o.dst >= uint32_t(mot::HEADER_OFF) && uint64_t(o.dst) + uint64_t(o.len) <= arena_size);
                        REQUIRE(o.dst >= uint32_t(mot::BODY_OFF) || o.dst + uint32_t(o.len) <= uint32_t(mot::BODY_OFF));
                    } else if (o.kind == mot::ORDER_SLIDE) {
                        REQUIRE(o.len > 0 && o.src >= mot::HEADER_OFF && uint64_t(o.src) + uint64_t(o.len) <= arena_size && uint64_t(o.dst) + uint64_t(o.len) <= slides_size);
                    } else {
                        REQUIRE(o.kind == mot::ORDER_RECORD && o.src == records && o.src < 4 && uint64_t(o.dst) + mot::RECORD_BYTES <= slides_size && o.dst % 16 == 0);
                        records++;
                    }
                    pkt::execute_order(o, ord, block, arena, slides);
                }
                REQUIRE(c.mot.slides_written - before == records && c.mot.slides_written <= call.max_slides);
                for (int k = before; k < c.mot.slides_written; k++) {
                    const uint8_t *slot = slides + size_t(k) * call.slide_stride;
                    int32_t rec[8];
                    std::memcpy(rec, slot, sizeof rec);
                    const uint8_t *h = slot + mot::RECORD_BYTES;
                    REQUIRE(rec[3] >= 7 && rec[4] >= 0 && uint32_t(mot::RECORD_BYTES + rec[3] + rec[4]) <= call.slide_stride && rec[5] == call.superframe && rec[6] == pos);
                    REQUIRE((((h[3] & 0x0F) << 9) | (h[4] << 1) | (h[5] >> 7)) == rec[3] && ((h[0] << 20) | (h[1] << 12) | (h[2] << 4) | (h[3] >> 4)) == rec[4]);
                    checked++;
                }
                std::free(block);
                pkt::State copy = st;
                pkt::sanitize(copy, call.body_capacity);              // what the walk leaves is a record of its own
                REQUIRE(std::memcmp(&copy, &st, sizeof st) == 0);
            });
        REQUIRE(t.fec + t.bad + t.padding + t.other + t.followed <= S && (fec || t.fec == 0));
        c.cifs++;
        c.slots += S;
        c.packets_fec += t.fec;
        c.slots_bad += t.bad;
        c.packets_padding += t.padding;
        c.packets_other += t.other;
        c.packets_followed += t.followed;
        std::free(frame);
    }
    for (size_t i = 0; i < sizeof(pkt::Counters) / 4; i++) reinterpret_cast<int32_t *>(&all)[i] += reinterpret_cast<int32_t *>(&c)[i];
    std::free(arena);
    std::free(slides);
    std::printf("frames=%ld slots=%d bad=%d fec=%d padding=%d other=%d followed=%d breaks=%d malformed=%d command=%d orphan=%d opened=%d "
                "unfinished=%d too_long=%d groups_ok=%d crc_failed=%d repeated=%d placed=%d completed=%d slides=%d dropped=%d checked=%ld orders=%ld\n",
                frames, all.slots, all.slots_bad, all.packets_fec, all.packets_padding, all.packets_other, all.packets_followed,
                all.continuity_breaks, all.packets_malformed, all.packets_command, all.packets_orphan, all.groups_opened, all.groups_unfinished,
                all.groups_too_long, all.mot.groups_ok, all.mot.groups_crc_failed, all.mot.groups_repeated, all.mot.segments_placed,
                all.mot.objects_completed, all.mot.slides_written, all.mot.slides_dropped, checked, orders);
    return all.cifs == frames ? 0 : 4;
}
