// pad_walk_fuzz.cpp -- include/dabgpu_pad_walk.h on its own, under the host compiler's sanitizers (tests/test_pad_labels.py
// builds this with -fsanitize=address,undefined and runs it): N walks over random access units and over valid ones with
// bytes changed, cut short or lengthened, each copied to the END of a heap block of exactly its size, so a read past
// [au, au + len) is a heap overflow.  The state runs on from walk to walk; now and then it is replaced by random bytes
// (a record the walk did not write) and goes through sanitize() as it does at the start of every call.
#include "dabgpu_pad_walk.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

namespace pad = dabgpu_pad;

static std::mt19937_64 rng(0xDAB0);
static int below(int n) { return int(rng() % uint64_t(n)); }

// a data group: text segment, clear, DL Plus or an unknown command
static std::vector<uint8_t> group() {
    std::vector<uint8_t> g;
    const int kind = below(8), toggle = below(2);
    if (kind == 0) {
        g = {uint8_t((toggle << 7) | 0x11), 0};
    } else if (kind == 1) {
        const int n = 1 + below(16);
        g = {uint8_t((toggle << 7) | 0x12), uint8_t(n - 1)};
        for (int i = 0; i < n; i++) g.push_back(uint8_t(rng()));
    } else if (kind == 2) {
        g = {uint8_t(0x10 | (3 + below(12))), uint8_t(rng())};
    } else {
        const int n = 1 + below(16), first = below(2), last = below(2);
        g = {uint8_t((toggle << 7) | (first << 6) | (last << 5) | (n - 1)), uint8_t((first ? 15 : below(8)) << 4)};
        for (int i = 0; i < n; i++) g.push_back(uint8_t(0x20 + below(0x5F)));
    }
    const uint32_t crc = pad::crc16(g.data(), int(g.size()));
    g.push_back(uint8_t(crc >> 8));
    g.push_back(uint8_t(crc));
    return g;
}

// a valid access unit: data stream element with a variable or short X-PAD field carrying (part of) a data group, then filler
static std::vector<uint8_t> valid_au() {
    static std::vector<uint8_t> open;                                  // what is left of the group being sent
    static const int lengths[8] = {4, 6, 8, 12, 16, 24, 32, 48};
    std::vector<uint8_t> x;                                            // logical X-PAD bytes
    int ind = 2, ci = 1;
    const bool start = open.empty();
    if (start) open = group();
    if (below(4) == 0) {                                               // short
        ind = 1;
        ci = start ? 1 : below(2);
        if (ci) x.push_back(start ? 2 : 3);
        while (x.size() < 4) {
            x.push_back(open.empty() ? 0 : open.front());
            if (!open.empty()) open.erase(open.begin());
        }
    } else {
        const int idx = below(8), extra = below(3);
        ci = start ? 1 : below(4) != 0;
        std::vector<uint8_t> body;
        if (ci) {
            if (extra == 1) { x.push_back(uint8_t((1 << 5) | 1)); body.insert(body.end(), 6, 0x11); }
            if (extra == 2) { x.push_back(uint8_t((0 << 5) | 31)); x.push_back(0x42); body.insert(body.end(), 4, 0x22); }
            x.push_back(uint8_t((idx << 5) | (start ? 2 : 3)));
            if (below(2)) x.push_back(0);                              // (not always: then the list runs into the data)
        }
        for (int i = 0; i < lengths[idx]; i++) {
            body.push_back(open.empty() ? 0 : open.front());
            if (!open.empty()) open.erase(open.begin());
        }
        x.insert(x.end(), body.begin(), body.end());
    }
    const int spare = below(3) == 0 ? below(300) : 0, n = int(x.size()) + 2 + spare;
    std::vector<uint8_t> au = {uint8_t(0x80 | (below(16) << 1))};
    if (n >= 255) { au.push_back(255); au.push_back(uint8_t(n - 255)); } else au.push_back(uint8_t(n));
    au.insert(au.end(), size_t(spare), 0);
    for (size_t i = x.size(); i-- > 0;) au.push_back(x[i]);
    au.push_back(uint8_t(ind << 4));
    au.push_back(uint8_t(ci << 1));
    const int filler = below(40);
    for (int i = 0; i < filler; i++) au.push_back(uint8_t(rng()));
    return au;
}

int main(int argc, char **argv) {
    const long walks = argc > 1 ? atol(argv[1]) : 200000;
    pad::State st;
    std::memset(&st, 0, sizeof st);
    pad::Counters c{};
    long labels = 0;
    for (long w = 0; w < walks; w++) {
        std::vector<uint8_t> au;
        const int how = below(16);
        int len = 0;
        if (how == 0) {
            len = -1;                                                  // lost
        } else if (how < 4) {                                          // random, often with a data stream element in front
            au.resize(size_t(below(3) ? below(40) : below(600)));
            for (uint8_t &v : au) v = uint8_t(rng());
            if (!au.empty() && below(2)) au[0] = uint8_t(0x80 | (au[0] & 0x1F));
        } else {
            au = valid_au();
            if (how < 8) {                                             // changed bytes
                for (int k = 1 + below(3); k > 0 && !au.empty(); k--) au[size_t(below(int(au.size())))] = uint8_t(rng());
            } else if (how < 10) {                                     // cut short
                au.resize(size_t(below(int(au.size()) + 1)));
            } else if (how == 10) {                                    // the count says more
                if (au.size() > 1) au[1] = uint8_t(au[1] + 1 + below(40));
            }
        }
        if (len >= 0) len = int(au.size());
        if (below(5000) == 0) {
            uint8_t *b = reinterpret_cast<uint8_t *>(&st);
            for (size_t i = 0; i < sizeof st; i++) b[i] = uint8_t(rng());
            pad::sanitize(st);
        }
        uint8_t *block = static_cast<uint8_t *>(std::malloc(len > 0 ? size_t(len) : 1));
        if (!block) return 2;
        const uint8_t *at = block + (len > 0 ? 0 : 1);                // an empty unit: the very end of its block
        if (len > 0) std::memcpy(block, au.data(), size_t(len));
        const int before = c.labels_completed;
        pad::walk_au(st, c, at, len);
        labels += c.labels_completed - before;
        std::free(block);
        if (st.label.length < 0 || st.label.length > 128 || st.group_have > pad::GROUP_MAX) return 3;
    }
    std::printf("walks=%ld aus=%d lost=%d xpad=%d malformed=%d ignored=%d groups_ok=%d crc_failed=%d labels=%ld changes=%d\n", walks, c.aus,
                c.aus_lost, c.aus_with_xpad, c.pad_malformed, c.fields_ignored, c.groups_ok, c.groups_crc_failed, labels, c.changes);
    return c.aus == walks ? 0 : 4;
}
