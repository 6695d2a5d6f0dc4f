// fig_listing_fuzz.cpp -- include/dabgpu_fig.h on its own, under the host compiler's sanitizers (tests/test_fig_listings.py builds
// this with -fsanitize=address,undefined and runs it): N rounds of the five listings over random bytes and over FIBs of valid FIGs
// with bytes changed, lengths and counts raised and end markers dropped in.  The FIBs and their CRC flags each lie at the END of a
// heap block of exactly their size, and the output is a heap block of exactly `max` entries, so a read outside the batch and a
// write behind `max` entries are heap overflows.  Checked per call: *n within the listing's cap, the order of what was handed
// over, nothing written by a call that reports DABGPU_ERR_CAPACITY or the profile callable's refusal.
#include "dabgpu_fig.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "dabgpu.h"

namespace fig = dabgpu_fig;

static std::mt19937_64 rng(0xF160);
static int below(int n) { return int(rng() % uint64_t(n)); }
typedef std::vector<uint8_t> Bytes;

constexpr uint8_t FILL = 0xA5;
constexpr int REFUSED = -5;

// ids from a small or a large pool: a small one makes duplicates and joins, a large one fills the lists
static int pool = 8;
static int id6() { return below(pool < 64 ? pool : 64); }
static int id12() { return below(pool < 4096 ? pool : 4096); }
static void put_sid(Bytes &b, int pd) {
    const uint32_t sid = (pd ? 0xE0000000u : 0u) + 0x1000u + uint32_t(below(pool));
    for (int q = pd ? 3 : 1; q >= 0; q--) b.push_back(uint8_t(sid >> (8 * q)));
}

// a FIG 0 of the given extension with as many whole entries as fit below `room` bytes (header and length byte included)
static Bytes fig0(int ext, int room) {
    const int pd = below(4) == 0;
    Bytes body;
    for (int tries = 1 + below(12); tries > 0; tries--) {
        Bytes e;
        if (ext == 1) {
            const int id = id6(), start = below(864);
            e = {uint8_t((id << 2) | (start >> 8)), uint8_t(start)};
            if (below(2)) {
                e.push_back(uint8_t((below(8) == 0) << 6 | below(64)));
            } else {
                const int option = below(6) ? below(2) : below(8), size = below(6) ? 4 * (1 + below(20)) : below(1024);
                e.push_back(uint8_t(0x80 | (option << 4) | (below(4) << 2) | (size >> 8)));
                e.push_back(uint8_t(size));
            }
        } else if (ext == 2) {
            put_sid(e, pd);
            const int ncomp = 1 + below(4);
            e.push_back(uint8_t(ncomp));
            for (int c = 0; c < ncomp; c++) {
                const int tmid = below(4);
                if (tmid == 3) {
                    const int scid = id12();
                    e.push_back(uint8_t(0xC0 | (scid >> 6)));
                    e.push_back(uint8_t((scid << 2) | below(4)));
                } else {
                    e.push_back(uint8_t((tmid << 6) | below(64)));
                    e.push_back(uint8_t((id6() << 2) | below(4)));
                }
            }
        } else if (ext == 3) {
            const int scid = id12(), caorg = below(4) == 0, address = below(1024);
            e = {uint8_t(scid >> 4), uint8_t((scid << 4) | caorg), uint8_t((below(2) << 7) | below(64)), uint8_t((id6() << 2) | (address >> 8)),
                 uint8_t(address)};
            if (caorg) e.insert(e.end(), 2, 0x5A);
        } else if (ext == 8) {
            put_sid(e, pd);
            const int extended = below(2);
            e.push_back(uint8_t((extended << 7) | below(4)));
            if (below(2)) {
                const int scid = id12();
                e.push_back(uint8_t(0x80 | (scid >> 8)));
                e.push_back(uint8_t(scid));
            } else {
                e.push_back(uint8_t(((below(6) == 0) << 6) | id6()));
            }
            if (extended) e.push_back(0);
        } else if (ext == 13) {
            put_sid(e, pd);
            const int count = 1 + below(3);
            e.push_back(uint8_t((below(4) << 4) | count));
            for (int a = 0; a < count; a++) {
                const int type = pool > 64 ? below(2048) : below(6), n = below(4) ? 0 : below(6);
                e.push_back(uint8_t(type >> 3));
                e.push_back(uint8_t((type << 5) | n));
                for (int q = 0; q < n; q++) e.push_back(uint8_t(rng()));
            }
        } else {
            e = {uint8_t((id6() << 2) | below(4))};
        }
        if (2 + body.size() + e.size() > size_t(room)) break;
        body.insert(body.end(), e.begin(), e.end());
    }
    Bytes f = {uint8_t(1 + body.size()), uint8_t((below(12) == 0) << 7 | (below(12) == 0) << 6 | (pd << 5) | ext)};
    f.insert(f.end(), body.begin(), body.end());
    return f;
}

// the 30 data bytes of a FIB and its two CRC bytes (which nothing reads: the flags say whether it held)
static void fill_fib(uint8_t *d) {
    static const int exts[8] = {1, 1, 2, 2, 3, 8, 13, 14};
    std::memset(d, 0, 32);
    int at = 0;
    while (at < 28 && below(8)) {
        const Bytes f = below(10) ? fig0(exts[below(8)], 30 - at) : Bytes{uint8_t((1 + below(7)) << 5 | 2), 0x11, 0x22};
        std::memcpy(d + at, f.data(), f.size());
        at += int(f.size());
    }
    if (at < 30) d[at] = 0xFF;
    const int how = below(12);
    if (how == 0) {                                                    // random bytes
        for (int i = 0; i < 32; i++) d[i] = uint8_t(rng());
    } else if (how < 4) {                                              // changed bytes
        for (int k = 1 + below(3); k > 0; k--) d[below(30)] = uint8_t(rng());
    } else if (how == 4) {                                             // a length raised: over the next FIG, or over the end
        const int len = (d[0] & 0x1F) + 1 + below(8);
        d[0] = uint8_t((d[0] & 0xE0) | (len > 31 ? 31 : len));
    } else if (how == 5) {                                             // an end marker or a zero length dropped in
        d[below(30)] = below(2) ? 0xFF : 0x00;
    } else if (how == 6) {                                             // a count or a flag nibble raised
        d[2 + below(28)] |= uint8_t(0x0F << (4 * below(2)));
    }
}

// `bytes` copied to the end of a heap block of exactly that size (none: the very end of a block of one byte)
struct AtEnd {
    uint8_t *block, *p;
    explicit AtEnd(const Bytes &bytes) : block(static_cast<uint8_t *>(std::malloc(bytes.empty() ? 1 : bytes.size()))), p(block + (bytes.empty() ? 1 : 0)) {
        if (!block) std::exit(2);
        if (!bytes.empty()) std::memcpy(block, bytes.data(), bytes.size());
    }
    ~AtEnd() { std::free(block); }
};

static void fail(const char *what, long round) {
    std::printf("fig_listing_fuzz: %s in round %ld\n", what, round);
    std::exit(1);
}

static long n_ok = 0, n_capacity = 0, n_refused = 0, n_entries = 0;

// one listing into exactly `max` entries; less(a, b): the order a successful call hands over (strictly, or equal)
template <class T, class Call, class Less> void run(long round, int max, int cap, Call call, Less less) {
    AtEnd out(Bytes(size_t(max) * sizeof(T), FILL));
    T *o = reinterpret_cast<T *>(out.p);
    int n = -1;
    const int rc = call(o, max, &n);
    if (rc == DABGPU_OK) {
        if (n < 0 || n > cap || n > max) fail("*n outside its range", round);
        for (int i = 1; i < n; i++)
            if (less(o[i], o[i - 1])) fail("entries out of order", round);
        n_ok++;
        n_entries += n;
    } else if (rc == DABGPU_ERR_CAPACITY) {
        if (n <= max || n > cap) fail("DABGPU_ERR_CAPACITY with *n that fits, or above the cap", round);
        n_capacity++;
    } else if (rc == REFUSED) {
        if (n != -1) fail("*n written by a refused call", round);
        n_refused++;
    } else {
        fail("a status no listing has", round);
    }
    const size_t kept = rc == DABGPU_OK ? size_t(n) * sizeof(T) : 0;
    for (size_t i = kept; i < size_t(max) * sizeof(T); i++)
        if (out.p[i] != FILL) fail("bytes written that are not the call's to write", round);
}

int main(int argc, char **argv) {
    const long rounds = argc > 1 ? atol(argv[1]) : 20000;
    for (long r = 0; r < rounds; r++) {
        pool = below(3) == 0 ? 5000 : 4 + below(12);
        const int n_frames = below(8) == 0 ? 0 : below(4) ? 1 + below(3) : 4 + below(6);
        Bytes fibs(size_t(n_frames) * 12 * 32), flags(size_t(n_frames) * 12);
        for (int k = 0; k < n_frames * 12; k++) {
            fill_fib(fibs.data() + size_t(k) * 32);
            flags[size_t(k)] = below(10) ? uint8_t(1 + below(255) * below(2)) : 0;
        }
        const AtEnd fib(fibs), crc(flags);
        const int max = below(4) == 0 ? below(8) : below(301);
        // the profile of an entry, as far as this header is concerned: any descriptor, or a refusal
        const auto profile = [](const fig::Organisation &e, dabgpu_subchannel &sc) {
            if (e.long_form ? e.size % 4 != 0 : e.table_switch) return REFUSED;
            sc.start_address = e.start;
            sc.length = e.long_form ? e.size : 1 + e.index;
            return 0;
        };
        run<dabgpu_subchannel>(r, max, 64, [&](dabgpu_subchannel *o, int m, int *n) { return fig::subchannels(fib.p, crc.p, n_frames, profile, o, m, n); },
                               [](const dabgpu_subchannel &a, const dabgpu_subchannel &b) { return a.start_address < b.start_address; });
        run<dabgpu_audio_component>(r, max, 64, [&](dabgpu_audio_component *o, int m, int *n) { return fig::audio_components(fib.p, crc.p, n_frames, o, m, n); },
                                    [](const dabgpu_audio_component &a, const dabgpu_audio_component &b) { return a.start_address < b.start_address; });
        run<dabgpu_stream_component>(r, max, 64, [&](dabgpu_stream_component *o, int m, int *n) { return fig::stream_components(fib.p, crc.p, n_frames, o, m, n); },
                                     [](const dabgpu_stream_component &a, const dabgpu_stream_component &b) { return a.start_address < b.start_address; });
        run<dabgpu_packet_component>(r, max, 256, [&](dabgpu_packet_component *o, int m, int *n) { return fig::packet_components(fib.p, crc.p, n_frames, o, m, n); },
                                     [](const dabgpu_packet_component &a, const dabgpu_packet_component &b) {
                                         return a.start_address != b.start_address ? a.start_address < b.start_address : a.packet_address < b.packet_address;
                                     });
        run<dabgpu_user_application>(r, max, 256, [&](dabgpu_user_application *o, int m, int *n) { return fig::user_applications(fib.p, crc.p, n_frames, o, m, n); },
                                     [](const dabgpu_user_application &a, const dabgpu_user_application &b) {
                                         if (a.sid != b.sid) return a.sid < b.sid;
                                         if (a.scids != b.scids) return a.scids < b.scids;
                                         return a.ua_type < b.ua_type;
                                     });
    }
    std::printf("rounds=%ld ok=%ld capacity=%ld refused=%ld entries=%ld\n", rounds, n_ok, n_capacity, n_refused, n_entries);
    if (n_ok < rounds || n_capacity < rounds / 20 || n_refused < rounds / 50 || n_entries < 10 * rounds) {
        std::printf("fig_listing_fuzz: the inputs exercise too little\n");
        return 4;
    }
    std::printf("fig_listing_fuzz ok\n");
    return 0;
}
