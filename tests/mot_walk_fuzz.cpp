// mot_walk_fuzz.cpp -- include/dabgpu_mot_walk.h on its own, under the host compiler's sanitizers (tests/test_pad_slides.py
// builds this with -fsanitize=address,undefined and runs it): N walks over random access units and over valid ones (MOT
// objects in X-PAD sub-fields of types 1 / 12 / 13) with bytes changed, cut short or lengthened, each copied to the END of
// a heap block of exactly its size; the arena and the slide slots are heap blocks of exactly their size, too.  The copy
// orders the walk returns are executed here as the kernel executes them, every one with its bounds asserted first.  The
// state runs on from walk to walk; a "call" ends every 48 walks (counters and slots start again, the state goes through
// sanitize()); now and then the state is replaced by random bytes, or the arena by one of another size.
#include "dabgpu_mot_walk.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <random>
#include <vector>

namespace mot = dabgpu_mot;
namespace pad = dabgpu_pad;
typedef std::vector<uint8_t> Bytes;

static std::mt19937_64 rng(0xD1DE);
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

// one MOT segment in its MSC data group; now and then something is off
static Bytes group(int type, int tid, int number, bool last, const uint8_t *seg, int z) {
    const int odd = below(24);
    const bool ext = below(4) == 0, seg_flag = odd != 0, ua = odd != 1, tid_flag = odd != 2;
    if (odd == 3) type = 5 + below(3);
    Bytes g = {uint8_t((ext << 7) | ((odd != 4) << 6) | (seg_flag << 5) | (ua << 4) | type), uint8_t(rng())};
    if (ext) { g.push_back(uint8_t(rng())); g.push_back(uint8_t(rng())); }
    if (seg_flag) { g.push_back(uint8_t((last << 7) | (number >> 8))); g.push_back(uint8_t(number)); }
    if (ua) {
        const int extra = below(3) ? 0 : below(14);
        g.push_back(uint8_t((tid_flag << 4) | ((tid_flag ? 2 : 0) + extra - (odd == 5 && extra == 0 ? 1 : 0))));
        if (tid_flag) { g.push_back(uint8_t(tid >> 8)); g.push_back(uint8_t(tid)); }
        for (int i = 0; i < extra; i++) g.push_back(uint8_t(rng()));
    }
    const int says = odd == 6 ? z + 1 : z;
    g.push_back(uint8_t((below(8) << 5) | (says >> 8)));
    g.push_back(uint8_t(says));
    g.insert(g.end(), seg, seg + z);
    put_crc(g);
    if (odd == 7) g[size_t(below(int(g.size())))] ^= uint8_t(1 << below(8));
    return g;
}

static std::deque<std::pair<int, Bytes>> queue;                       // sub-fields waiting to be sent: (type, bytes)
static const int lengths[8] = {4, 6, 8, 12, 16, 24, 32, 48};

// the next object: header and body in segments, groups in any order now and then, each group behind its length indicator
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
    std::vector<Bytes> groups;
    for (int part = 0; part < 2; part++) {
        const Bytes &d = part ? body : header;
        const int size = part ? bseg : hseg, n = d.empty() ? 1 : int((d.size() + size_t(size) - 1) / size_t(size));
        for (int k = 0; k < n; k++) {
            const int at = k * size, z = int(d.size()) - at < size ? int(d.size()) - at : size;
            groups.push_back(group(3 + part, tid, below(40) ? k : k + below(300), k == n - 1 || below(60) == 0, d.data() + at, z - (below(50) == 0 && z > 1)));
        }
    }
    if (below(4) == 0) std::shuffle(groups.begin(), groups.end(), rng);
    if (below(6) == 0 && !groups.empty()) groups.push_back(groups[size_t(below(int(groups.size())))]);
    for (const Bytes &g : groups) {
        if (g.size() >= 16384) continue;
        const int idx = g.size() > 600 ? 7 : below(8);
        if (below(20)) {
            Bytes li = {uint8_t(g.size() >> 8), uint8_t(g.size())};
            put_crc(li);
            if (below(30) == 0) li[3] ^= 1;
            queue.push_back({1, li});
        }
        for (size_t at = 0, k = 0; at < g.size(); at += size_t(lengths[idx]), k++) {
            Bytes part;
            part.resize(size_t(lengths[idx]), 0);
            std::memcpy(part.data(), g.data() + at, g.size() - at < part.size() ? g.size() - at : part.size());
            queue.push_back({k ? 13 : 12, part});
        }
    }
}

// a valid access unit: a data stream element with a variable X-PAD field of up to four waiting sub-fields, then filler
static Bytes valid_au(int body_capacity, bool *ci_less_ok, int *last_type, int *last_len) {
    if (queue.empty()) next_object(body_capacity);
    Bytes x;
    const int want = 1 + below(4);
    std::vector<std::pair<int, Bytes>> take;
    int bytes = 0;
    while (int(take.size()) < want && !queue.empty() && bytes + int(queue.front().second.size()) <= 192) {
        bytes += int(queue.front().second.size());
        take.push_back(queue.front());
        queue.pop_front();
    }
    const bool bare = *ci_less_ok && take.size() == 1 && take[0].first == 13 && *last_type >= 12 && int(take[0].second.size()) == *last_len && below(2);
    if (!bare) {
        if (below(5) == 0 && take.size() < 4) { x.push_back(uint8_t((below(8) << 5) | 2)); }      // a label's sub-field in front
        const size_t dls = x.size();
        for (auto &t : take) {
            int idx = 0;
            while (lengths[idx] != int(t.second.size())) idx++;
            x.push_back(uint8_t((idx << 5) | t.first));
        }
        if (take.size() + dls < 4) x.push_back(0);
        if (dls) x.insert(x.end(), size_t(lengths[x[0] >> 5]), 0x2A);
    }
    for (auto &t : take) x.insert(x.end(), t.second.begin(), t.second.end());
    *ci_less_ok = true;
    *last_type = take.back().first;
    *last_len = int(take.back().second.size());
    const int spare = below(3) == 0 ? below(250) : 0, n = int(x.size()) + 2 + spare;
    Bytes au = {uint8_t(0x80 | (below(16) << 1))};
    if (n >= 255) { au.push_back(255); au.push_back(uint8_t(n - 255)); } else au.push_back(uint8_t(n));
    au.insert(au.end(), size_t(spare), 0);
    for (size_t i = x.size(); i-- > 0;) au.push_back(x[i]);
    au.push_back(uint8_t(2 << 4));
    au.push_back(uint8_t(!bare << 1));
    const int filler = below(40);
    for (int i = 0; i < filler; i++) au.push_back(uint8_t(rng()));
    return au;
}

int main(int argc, char **argv) {
    const long walks = argc > 1 ? atol(argv[1]) : 150000;
    mot::State st;
    std::memset(&st, 0, sizeof st);
    mot::Counters c{}, all{};
    mot::Orders ord;
    mot::Call call{};
    uint8_t *arena = nullptr, *slides = nullptr;
    size_t arena_size = 0, slides_size = 0;
    long slides_seen = 0, malformed = 0, crc_failed = 0, too_large = 0, orders = 0, checked = 0;
    bool ci_less_ok = false;
    int last_type = 0, last_len = 0;
    for (long w = 0; w < walks; w++) {
        if (w % 48 == 0) {                                            // the next call
            for (size_t i = 0; i < sizeof(mot::Counters) / 4; i++) reinterpret_cast<int32_t *>(&all)[i] += reinterpret_cast<int32_t *>(&c)[i];
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
            if (below(20) == 0) {
                uint8_t *b = reinterpret_cast<uint8_t *>(&st);
                if (below(2)) for (size_t i = 0; i < sizeof st; i++) b[i] = uint8_t(rng());
                else for (int k = 1 + below(4); k > 0; k--) b[size_t(below(int(sizeof st)))] ^= uint8_t(1 << below(8));
            }
            mot::sanitize(st, call.body_capacity);
        }
        Bytes au;
        const int how = below(24);
        int len = 0;
        if (how == 0) {
            len = -1;                                                  // lost
            ci_less_ok = false;
        } else if (how < 3) {                                          // random, often with a data stream element in front
            au.resize(size_t(below(3) ? below(40) : below(600)));
            for (uint8_t &v : au) v = uint8_t(rng());
            if (!au.empty() && below(2)) au[0] = uint8_t(0x80 | (au[0] & 0x1F));
        } else {
            au = valid_au(call.body_capacity, &ci_less_ok, &last_type, &last_len);
            if (how == 3) {                                            // changed bytes
                for (int k = 1 + below(3); k > 0 && !au.empty(); k--) au[size_t(below(int(au.size())))] = uint8_t(rng());
            } else if (how == 4) {                                     // cut short
                au.resize(size_t(below(int(au.size()) + 1)));
            } else if (how == 5) {                                     // the count says more
                if (au.size() > 1) au[1] = uint8_t(au[1] + 1 + below(40));
            }
        }
        if (len >= 0) len = int(au.size());
        uint8_t *block = static_cast<uint8_t *>(std::malloc(len > 0 ? size_t(len) : 1));
        if (!block) return 2;
        const uint8_t *at = block + (len > 0 ? 0 : 1);                // an empty unit: the very end of its block
        if (len > 0) std::memcpy(block, au.data(), size_t(len));
        call.superframe = int(w % 48) / 3;
        call.au = int(w % 3);
        const int before = c.slides_written;
        mot::walk_au(st, c, ord, call, at, len);
        REQUIRE(ord.n >= 0 && ord.n <= mot::MAX_ORDERS);
        int records = 0;
        for (int i = 0; i < ord.n; i++) {
            const mot::Order &o = ord.o[i];
            orders++;
            if (o.kind == mot::ORDER_XPAD) {
                REQUIRE(o.len > 0 && o.src < len && o.src - (o.len - 1) >= 0 && uint64_t(o.dst) + uint64_t(o.len) <= uint64_t(mot::GROUP_CAP));
            } else if (o.kind == mot::ORDER_MOVE) {
                REQUIRE(o.len > 0 && o.src >= 0 && o.src + o.len <= mot::GROUP_CAP && o.dst >= uint32_t(mot::HEADER_OFF) && uint64_t(o.dst) + uint64_t(o.len) <= arena_size);
                REQUIRE(o.dst >= uint32_t(mot::BODY_OFF) || o.dst + uint32_t(o.len) <= uint32_t(mot::BODY_OFF));
            } else if (o.kind == mot::ORDER_SLIDE) {
                REQUIRE(o.len > 0 && o.src >= mot::HEADER_OFF && uint64_t(o.src) + uint64_t(o.len) <= arena_size && uint64_t(o.dst) + uint64_t(o.len) <= slides_size);
            } else {
                REQUIRE(o.kind == mot::ORDER_RECORD && o.src == records && o.src < 4 && uint64_t(o.dst) + mot::RECORD_BYTES <= slides_size && o.dst % 16 == 0);
                records++;
            }
            mot::execute(o, ord, at, arena, slides);
        }
        REQUIRE(c.slides_written - before == records && c.slides_written <= call.max_slides);
        // a slide in its slot says what its record says: header_size and body_size of the header core
        for (int k = before; k < c.slides_written; k++) {
            const uint8_t *slot = slides + size_t(k) * call.slide_stride;
            int32_t rec[8];
            std::memcpy(rec, slot, sizeof rec);
            const uint8_t *h = slot + mot::RECORD_BYTES;
            REQUIRE(rec[3] >= 7 && rec[4] >= 0 && uint32_t(mot::RECORD_BYTES + rec[3] + rec[4]) <= call.slide_stride);
            REQUIRE((((h[3] & 0x0F) << 9) | (h[4] << 1) | (h[5] >> 7)) == rec[3] && ((h[0] << 20) | (h[1] << 12) | (h[2] << 4) | (h[3] >> 4)) == rec[4]);
            checked++;
        }
        std::free(block);
        mot::State copy = st;
        mot::sanitize(copy, call.body_capacity);                      // what the walk leaves is a record of its own
        REQUIRE(std::memcmp(&copy, &st, sizeof st) == 0);
    }
    for (size_t i = 0; i < sizeof(mot::Counters) / 4; i++) reinterpret_cast<int32_t *>(&all)[i] += reinterpret_cast<int32_t *>(&c)[i];
    slides_seen = all.slides_written;
    malformed = all.pad_malformed + all.groups_malformed;
    crc_failed = all.groups_crc_failed;
    too_large = all.objects_too_large;
    std::free(arena);
    std::free(slides);
    std::printf("walks=%ld aus=%d lost=%d xpad=%d malformed=%ld lengths_ignored=%d no_length=%d groups_ok=%d crc_failed=%ld ignored_type=%d no_tid=%d "
                "repeated=%d placed=%d early_last=%d completed=%d mismatched=%d too_large=%ld slides=%ld dropped=%d checked=%ld orders=%ld\n",
                walks, all.aus, all.aus_lost, all.aus_with_xpad, malformed, all.lengths_ignored, all.groups_no_length, all.groups_ok, crc_failed,
                all.groups_ignored_type, all.groups_no_transport_id, all.groups_repeated, all.segments_placed, all.segments_early_last,
                all.objects_completed, all.objects_mismatched, too_large, slides_seen, all.slides_dropped, checked, orders);
    return all.aus == walks ? 0 : 4;
}
