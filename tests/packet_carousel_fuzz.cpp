// packet_carousel_fuzz.cpp -- include/dabgpu_mot_carousel.h on its own, under the host compiler's sanitizers
// (tests/test_packet_carousel.py builds this with -fsanitize=address,undefined and runs it): N logical frames of random bit
// rates -- random bytes, and valid packets (MOT directory carousels in data groups cut into packets of one address, beside
// padding and other addresses) with bytes changed, directories that lie about their sizes, transport ids that collide,
// segments out of order and repeated -- each frame a heap block of exactly its size; the arena, d_directory and the object
// slots are heap blocks of exactly their size, too.  The scan and the three phases of a followed packet run as the kernel
// runs them, the copy orders are executed with their bounds asserted first.  The state runs on from frame to frame; a "call"
// ends every 16 frames (counters and slots start again, the state goes through sanitize()); now and then the state is
// replaced by random bytes or has bits changed, or the three sizes change.
#include "dabgpu_mot_carousel.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <random>
#include <vector>

namespace mot = dabgpu_mot;
namespace pad = dabgpu_pad;
namespace pkt = dabgpu_packet;
namespace car = dabgpu_carousel;
typedef std::vector<uint8_t> Bytes;

static std::mt19937_64 rng(0xCA805E1);
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
static int S = 8;                                                      // slots of a frame, until the bit rate changes

static Bytes packet(int address, const uint8_t *data, int n, int slots, bool first, bool last) {
    const int odd = below(200);
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
        const int slots = 1 + below(S < 4 ? S : 4), room = 24 * slots - 5;
        const int take = int(g.size() - at) < room ? int(g.size() - at) : room;
        const bool last = at + size_t(take) == g.size();
        queue.push_back(packet(ADDRESS, g.data() + at, take, slots, at == 0, last));
        at += size_t(take);
        if (last) break;
    }
}

// the segments of one object part as data groups of `type`, shuffled a little, some repeated
static void send_part(int type, int tid, const Bytes &d, int size) {
    const int n = d.empty() ? 1 : int((d.size() + size_t(size) - 1) / size_t(size));
    std::vector<int> order(static_cast<size_t>(n));
    for (int k = 0; k < n; k++) order[size_t(k)] = k;
    if (below(4) == 0 && n > 1) std::swap(order[size_t(below(n))], order[size_t(below(n))]);
    for (int k : order) {
        const int at = k * size, z = int(d.size()) - at < size ? int(d.size()) - at : size, odd = below(60);
        Bytes g = {uint8_t(((odd != 0) << 6) | ((odd != 1) << 5) | ((odd != 2) << 4) | (odd == 3 ? 3 + below(5) : type)), uint8_t(rng())};
        if (odd != 1) { g.push_back(uint8_t(((k == n - 1) << 7) | (k >> 8))); g.push_back(uint8_t(k)); }
        if (odd != 2) { g.push_back(0x12); g.push_back(uint8_t(tid >> 8)); g.push_back(uint8_t(tid)); }
        const int says = odd == 4 ? z + 1 : z;
        g.push_back(uint8_t(says >> 8));
        g.push_back(uint8_t(says));
        g.insert(g.end(), d.begin() + at, d.begin() + at + z);
        put_crc(g);
        send_group(g);
        if (below(10) == 0) send_group(g);                             // a repetition
    }
}

static int dir_tid = 1;
static void next_carousel(int directory_capacity, int object_capacity) {
    if (below(3) == 0) dir_tid = 1 + below(5);
    const int n = below(8) ? below(7) : below(300);
    struct Obj { int tid; Bytes body; };
    std::vector<Obj> objs;
    Bytes dir(13, 0);
    for (int i = 0; i < n; i++) {
        const int tid = 100 + below(n > 20 ? 400 : 12), hbytes = 7 + below(below(6) ? 30 : 300);
        const int bbytes = i < 6 ? (below(10) ? below(400) : below(object_capacity + 40)) : below(40);
        Bytes header(static_cast<size_t>(hbytes));
        for (uint8_t &v : header) v = uint8_t(rng());
        const int hsays = below(40) ? hbytes : hbytes - 1 + below(3), bsays = below(30) ? bbytes : bbytes + 1;
        header[0] = uint8_t(bsays >> 20); header[1] = uint8_t(bsays >> 12); header[2] = uint8_t(bsays >> 4);
        header[3] = uint8_t(((bsays & 15) << 4) | (hsays >> 9)); header[4] = uint8_t(hsays >> 1); header[5] = uint8_t(((hsays & 1) << 7) | (header[5] & 0x7F));
        dir.push_back(uint8_t(tid >> 8));
        dir.push_back(uint8_t(tid));
        dir.insert(dir.end(), header.begin(), header.end());
        if (i < 6) {
            Bytes body(static_cast<size_t>(bbytes));
            for (uint8_t &v : body) v = uint8_t(rng());
            objs.push_back({tid, body});
        }
    }
    const int D = int(dir.size()), dsays = below(25) ? D : D + below(3) - 1, nsays = below(25) ? n : n + 1;
    dir[0] = uint8_t((dsays >> 24) | (below(40) ? 0 : 0x80)); dir[1] = uint8_t(dsays >> 16); dir[2] = uint8_t(dsays >> 8); dir[3] = uint8_t(dsays);
    dir[4] = uint8_t(nsays >> 8); dir[5] = uint8_t(nsays);
    dir[6] = uint8_t(rng()); dir[7] = uint8_t(rng()); dir[8] = uint8_t(rng()); dir[9] = uint8_t(rng()); dir[10] = uint8_t(rng());
    if (below(40) == 0) dir[12] = uint8_t(1 + below(200));             // an extension that is not there
    const bool bodies_first = below(4) == 0;
    const int dseg = 1 + below(below(3) ? 200 : directory_capacity + 20);
    if (!bodies_first) send_part(6, dir_tid, dir, dseg > 8191 ? 8191 : dseg);
    // the bodies, interleaved segment by segment now and then
    if (below(3) == 0 && objs.size() > 1) {
        for (int round = 0; round < 4; round++)
            for (const Obj &o : objs) {
                const int size = 1 + int(o.body.size()) / 4;
                const int at = round * size;
                if (at > int(o.body.size()) || (at == int(o.body.size()) && at > 0)) continue;
                const int z = std::min(size, int(o.body.size()) - at);
                const bool last = at + z == int(o.body.size());
                Bytes g = {0x74, 0x00, uint8_t((last << 7)), uint8_t(round), 0x12, uint8_t(o.tid >> 8), uint8_t(o.tid), uint8_t(z >> 8), uint8_t(z)};
                g.insert(g.end(), o.body.begin() + at, o.body.begin() + at + z);
                put_crc(g);
                send_group(g);
            }
    } else {
        for (const Obj &o : objs) send_part(4, o.tid, o.body, 1 + below(below(4) ? 96 : 8191));
    }
    if (bodies_first) send_part(6, dir_tid, dir, dseg > 8191 ? 8191 : dseg);
}

int main(int argc, char **argv) {
    const long frames = argc > 1 ? atol(argv[1]) : 30000;
    car::State *st = static_cast<car::State *>(std::aligned_alloc(16, sizeof(car::State)));
    if (!st) return 2;
    std::memset(st, 0, sizeof *st);
    car::Counters c{}, all{};
    mot::Orders ord;
    car::Call call{};
    uint8_t *arena = nullptr, *slots = nullptr, *directory = nullptr;
    size_t arena_size = 0, slots_size = 0;
    long orders = 0, checked = 0, fresh = 0;
    auto run_orders = [&](const uint8_t *block, int need, int phase) {
        REQUIRE(ord.n >= 0 && ord.n <= mot::MAX_ORDERS);
        const uint32_t body0 = car::body_off(call, 0), pitch = car::round16(uint32_t(call.object_capacity));
        for (int i = 0; i < ord.n; i++) {
            const mot::Order &o = ord.o[i];
            orders++;
            if (o.kind == pkt::ORDER_PACKET) {
                REQUIRE(phase == 1 && i == 0 && o.len > 0 && o.src == 3 && o.src + o.len <= need && uint64_t(o.dst) + uint64_t(o.len) <= uint64_t(mot::GROUP_CAP));
            } else if (o.kind == mot::ORDER_MOVE) {
                REQUIRE(phase == 1 && o.len > 0 && o.src >= 0 && o.src + o.len <= mot::GROUP_CAP && o.dst >= uint32_t(car::DIRECTORY_OFF));
                if (o.dst < body0) {
                    REQUIRE(uint64_t(o.dst) + uint64_t(o.len) <= uint64_t(car::DIRECTORY_OFF) + uint64_t(call.directory_capacity));
                } else {
                    const uint32_t k = pitch ? (o.dst - body0) / pitch : 0;
                    REQUIRE(int(k) < call.assemblies && uint64_t(o.dst) + uint64_t(o.len) <= uint64_t(body0) + uint64_t(k) * pitch + uint64_t(call.object_capacity));
                }
                REQUIRE(uint64_t(o.dst) + uint64_t(o.len) <= arena_size);
            } else if (o.kind == car::ORDER_DIRECTORY) {
                REQUIRE(phase == 2 && o.src == car::DIRECTORY_OFF && o.dst == 0 && o.len >= 13 && o.len <= call.directory_capacity);
            } else if (o.kind == car::ORDER_OBJECT) {
                REQUIRE(phase == 3 && o.len > 0 && o.src >= car::DIRECTORY_OFF && uint64_t(o.src) + uint64_t(o.len) <= arena_size &&
                        uint64_t(o.dst) + uint64_t(o.len) <= slots_size);
            } else {
                REQUIRE(phase == 3 && o.kind == mot::ORDER_RECORD && o.src == 0 && uint64_t(o.dst) + mot::RECORD_BYTES <= slots_size && o.dst % 16 == 0);
            }
            car::execute_order(o, ord, block, arena, directory, slots);
        }
    };
    for (long w = 0; w < frames; w++) {
        if (w % 16 == 0) {                                            // the next call
            car::finish(*st, c);
            for (size_t i = 0; i < sizeof(car::Counters) / 4 - 5; i++) reinterpret_cast<int32_t *>(&all)[i] += reinterpret_cast<int32_t *>(&c)[i];    // (not what describes the directory)
            std::memset(&c, 0, sizeof c);
            if (!arena || below(40) == 0) {                           // other sizes (and what the state says no longer goes with them)
                std::free(arena);
                std::free(directory);
                call.directory_capacity = below(3) ? 16 + below(600) : 16 + below(9000);
                call.assemblies = below(3) ? 1 + below(4) : 1 + below(32);
                call.object_capacity = below(3) ? below(700) : 8191 + below(2000);
                REQUIRE(car::sizes_ok(call.directory_capacity, call.assemblies, call.object_capacity));
                arena_size = size_t(car::arena_bytes(call.directory_capacity, call.assemblies, call.object_capacity));
                arena = static_cast<uint8_t *>(std::malloc(arena_size));
                directory = static_cast<uint8_t *>(std::malloc(size_t(call.directory_capacity)));
                if (!arena || !directory) return 2;
                std::memset(arena, 0xA7, arena_size);
                std::memset(directory, 0xA7, size_t(call.directory_capacity));
            }
            std::free(slots);
            call.max_objects = below(4);
            call.object_stride = uint32_t(16 * (2 + below(below(4) ? 40 : 700)));
            call.deferred = 0;
            slots_size = size_t(call.max_objects) * call.object_stride;
            slots = static_cast<uint8_t *>(std::malloc(slots_size ? slots_size : 1));
            if (!slots) return 2;
            if (below(12) == 0) {
                uint8_t *b = reinterpret_cast<uint8_t *>(st);
                if (below(3) == 0) for (size_t i = 0; i < sizeof *st; i++) b[i] = uint8_t(rng());
                else for (int k = 1 + below(4); k > 0; k--) b[size_t(below(int(sizeof *st)))] ^= uint8_t(1 << below(8));
            }
            const bool had = st->pkt.seen || st->placed || st->dir_valid || st->cur_valid;
            car::sanitize(*st, call.directory_capacity, call.assemblies, call.object_capacity);
            fresh += had && !st->pkt.seen && !st->placed && !st->dir_valid && !st->cur_valid;
            if (below(4) == 0) S = below(3) ? 1 + below(12) : 1 + below(64);
        }
        // the frame: a heap block of exactly 24 S bytes
        uint8_t *frame = static_cast<uint8_t *>(std::malloc(size_t(24 * S)));
        if (!frame) return 2;
        const int how = below(20);
        if (how == 0) {
            for (int i = 0; i < 24 * S; i++) frame[i] = uint8_t(rng());
        } else {
            int pos = 0;
            while (pos < S) {
                if (queue.empty()) next_carousel(call.directory_capacity, call.object_capacity);
                const int kind = below(10);
                Bytes p;
                if (kind == 0) {
                    p = packet(0, nullptr, 0, 1 + below(4), false, false);
                } else if (kind == 1) {
                    uint8_t d[19];
                    for (uint8_t &v : d) v = uint8_t(rng());
                    p = packet(1 + below(1023), d, 19, 1, true, true);
                } else {
                    p = queue.front();
                    if (pos + int(p.size()) / 24 <= S || below(6) == 0) queue.pop_front();
                    else p = packet(0, nullptr, 0, 1, false, false);
                }
                const int n = int(p.size()) < 24 * (S - pos) ? int(p.size()) : 24 * (S - pos);     // (one that overruns is cut off)
                std::memcpy(frame + 24 * pos, p.data(), size_t(n));
                pos += n / 24;
            }
            if (how == 1) for (int k = 1 + below(3); k > 0; k--) frame[below(24 * S)] = uint8_t(rng());
        }
        call.frame = int(w % 16);
        pkt::scan_frame(c.head, frame, S, ADDRESS, 0, [&](int pos, int L) {
            REQUIRE(pos >= 0 && L >= 1 && L <= 4 && pos + L <= S);
            const int need = pkt::packet_read_bytes(L, frame[24 * pos + 2]);
            REQUIRE(need >= 3 && need <= 24 * L - 2);
            uint8_t *block = static_cast<uint8_t *>(std::malloc(size_t(need)));      // what the walk kernel stages, exactly
            if (!block) std::exit(2);
            std::memcpy(block, frame + 24 * pos, size_t(need));
            call.slot = pos;
            const int before = c.objects_written;
            car::follow_packet(*st, c, ord, call, block, L);
            run_orders(block, need, 1);
            if (st->check_pending) {
                REQUIRE(mot::part_full(st->dir) && mot::part_bytes(st->dir) <= call.directory_capacity);
                // the check reads exactly the directory's bytes: a heap block of that size
                const int D = mot::part_bytes(st->dir);
                uint8_t *copy = static_cast<uint8_t *>(std::malloc(size_t(D ? D : 1)));
                if (!copy) std::exit(2);
                std::memcpy(copy, arena + car::DIRECTORY_OFF, size_t(D));
                if (car::check_directory_phase(*st, c, ord, copy)) car::clear_stale(*st, c, call);
                std::free(copy);
                run_orders(block, need, 2);
            }
            REQUIRE(!st->check_pending);
            car::emit_attempt(*st, c, ord, call);
            run_orders(block, need, 3);
            REQUIRE(c.objects_written - before <= 1 && c.objects_written <= call.max_objects);
            for (int k = before; k < c.objects_written; k++) {
                const uint8_t *slot = slots + size_t(k) * call.object_stride;
                int32_t rec[8];
                std::memcpy(rec, slot, sizeof rec);
                const uint8_t *h = slot + mot::RECORD_BYTES;
                REQUIRE(rec[3] >= 7 && rec[4] >= 0 && uint32_t(mot::RECORD_BYTES + rec[3] + rec[4]) <= call.object_stride && rec[5] == call.frame && rec[6] == pos);
                REQUIRE((((h[3] & 0x0F) << 9) | (h[4] << 1) | (h[5] >> 7)) == rec[3] && ((h[0] << 20) | (h[1] << 12) | (h[2] << 4) | (h[3] >> 4)) == rec[4]);
                REQUIRE(rec[7] == st->cur_tid && st->cur_valid);
                checked++;
            }
            std::free(block);
            car::State *copy = static_cast<car::State *>(std::aligned_alloc(16, sizeof(car::State)));
            if (!copy) std::exit(2);
            std::memcpy(copy, st, sizeof *st);
            car::sanitize(*copy, call.directory_capacity, call.assemblies, call.object_capacity);     // what the walk leaves is a record of its own
            REQUIRE(std::memcmp(copy, st, sizeof *st) == 0);
            std::free(copy);
        });
        std::free(frame);
    }
    for (size_t i = 0; i < sizeof(car::Counters) / 4 - 5; i++) reinterpret_cast<int32_t *>(&all)[i] += reinterpret_cast<int32_t *>(&c)[i];    // (not what describes the directory)
    std::free(arena);
    std::free(directory);
    std::free(slots);
    std::free(st);
    std::printf("frames=%ld slots=%d bad=%d followed=%d groups_ok=%d crc_failed=%d header_mode=%d ignored=%d repeated=%d unlisted=%d placed=%d "
                "too_large=%d directories=%d mismatched=%d dir_too_large=%d stale=%d evicted=%d body_mismatched=%d dropped=%d deferred=%d written=%d "
                "fresh=%ld checked=%ld orders=%ld\n",
                frames, all.head.slots, all.head.slots_bad, all.head.packets_followed, all.head.mot.groups_ok, all.head.mot.groups_crc_failed,
                all.groups_header_mode, all.head.mot.groups_ignored_type, all.head.mot.groups_repeated, all.groups_unlisted, all.head.mot.segments_placed,
                all.head.mot.objects_too_large, all.directories_completed, all.directories_mismatched, all.directories_too_large, all.objects_stale,
                all.objects_evicted, all.head.mot.objects_mismatched, all.objects_dropped, all.objects_deferred, all.objects_written, fresh, checked, orders);
    return all.head.cifs == frames ? 0 : 4;
}
