// dabgpu_pad_api.hip -- the C ABI of the dynamic labels (include/dabgpu.h, "Dynamic labels"): the batch call on device
// memory, its twin on host memory (no context, no GPU: the same walk, include/dabgpu_pad_walk.h) and the label's text as UTF-8.
#include "dabgpu_ctx.hpp"

#include <cstring>

#include "../../include/dabgpu_pad_walk.h"

using namespace dabapi;
namespace pad = dabgpu_pad;

static_assert(sizeof(dabgpu_pad_label) == sizeof(pad::Label) && sizeof(dabgpu_pad_result) == sizeof(pad::Counters),
              "ABI structs mirror the walk's");
static_assert(sizeof(dabgpu_superframe_status) == 64, "the walk reads status rows as 16 words");

size_t dabgpu_pad_state_bytes(void) { return sizeof(pad::State); }

// everything both calls refuse, before anything is done; fills the kernel's table when there is one
static int pad_check(const dabgpu_pad_entry *entries, int n_entries, dabk::PadEntry *table) {
    if (n_entries < 0 || (n_entries > 0 && !entries)) return DABGPU_ERR_ARG;
    const uint64_t sb = sizeof(pad::State);
    for (int i = 0; i < n_entries; i++) {
        const dabgpu_pad_entry &e = entries[i];
        if (e.bitrate_kbps < 8 || e.bitrate_kbps > 512 || e.bitrate_kbps % 8) return DABGPU_ERR_ARG;
        const int s = e.bitrate_kbps / 8;
        if (e.max_superframes < 0 || e.data_stride < size_t(110) * s) return DABGPU_ERR_ARG;
        if (!e.d_data || !e.d_status || !e.d_follow || !e.d_state_out || !e.d_label || !e.d_result) return DABGPU_ERR_ARG;
        if ((addr(e.d_state_in) | addr(e.d_state_out)) & 15) return DABGPU_ERR_ARG;
        if ((addr(e.d_status) | addr(e.d_follow) | addr(e.d_label) | addr(e.d_result)) & 3) return DABGPU_ERR_ARG;
        if (e.d_state_in && overlaps(e.d_state_in, sb, e.d_state_out, sb)) return DABGPU_ERR_ARG;
        if (!table) continue;
        dabk::PadEntry &t = table[i];
        t.data = addr(e.d_data);
        t.data_stride = e.data_stride;
        t.status = addr(e.d_status);
        t.follow = addr(e.d_follow);
        t.state_in = addr(e.d_state_in);
        t.state_out = addr(e.d_state_out);
        t.label = addr(e.d_label);
        t.result = addr(e.d_result);
        t.s = s;
        t.max_superframes = e.max_superframes;
    }
    return DABGPU_OK;
}

int dabgpu_pad_labels_dev(dabgpu_ctx *ctx, const dabgpu_pad_entry *entries, int n_entries, void *stream) {
    if (!ctx) return DABGPU_ERR_ARG;
    // everything is checked before anything is enqueued: a refused call leaves every output as it was
    std::vector<dabk::PadEntry> table(size_t(n_entries > 0 ? n_entries : 0), dabk::PadEntry{});
    const int bad = pad_check(entries, n_entries, table.data());
    if (bad) return bad;
    if (n_entries == 0) return DABGPU_OK;
    const size_t table_bytes = table.size() * sizeof(dabk::PadEntry);
    return launch_entry_table(ctx, STAGE_PAD, table_bytes, stream, [&](void *d_table, size_t slot_bytes, hipStream_t s) {
        return dabk::launch_pad_labels(table.data(), n_entries, d_table, slot_bytes, s);
    });
}

int dabgpu_pad_labels_host(const dabgpu_pad_entry *entries, int n_entries) {
    const int bad = pad_check(entries, n_entries, nullptr);
    if (bad) return bad;
    for (int i = 0; i < n_entries; i++) {
        const dabgpu_pad_entry &e = entries[i];
        pad::State st;
        if (e.d_state_in) std::memcpy(&st, e.d_state_in, sizeof st);
        else std::memset(&st, 0, sizeof st);
        pad::sanitize(st);
        pad::Counters c{};
        int n_sf = e.d_follow->n_superframes;
        n_sf = n_sf < 0 ? 0 : n_sf > e.max_superframes ? e.max_superframes : n_sf;
        pad::walk_superframes(st, c, e.d_data, e.data_stride, reinterpret_cast<const int32_t *>(e.d_status), n_sf, e.bitrate_kbps / 8);
        std::memcpy(e.d_state_out, &st, sizeof st);
        std::memcpy(e.d_label, &st.label, sizeof st.label);
        std::memcpy(e.d_result, &c, sizeof c);
    }
    return DABGPU_OK;
}

// ---------------------------------------------------------------------------- the label as text
int dabgpu_pad_label_utf8(const dabgpu_pad_label *label, char *out, int cap) {
    if (!label || !out || cap < 1 || label->length < 0 || label->length > 128) return DABGPU_ERR_ARG;
    const uint8_t *t = label->text;
    const int n = label->length;
    char text[200];                                                    // 64 UCS-2 characters make at most 192 bytes
    int at = 0;
    auto put = [&](uint32_t v) { text[at++] = char(v); };
    if (label->charset == 15) {
        for (int i = 0; i < n;) {
            const uint8_t b = t[i];
            const int more = b < 0x80 ? 0 : (b >> 5) == 6 ? 1 : (b >> 4) == 14 ? 2 : (b >> 3) == 30 ? 3 : -1;
            if (more < 0 || i + more >= n) return DABGPU_ERR_ARG;
            uint32_t cp = more == 0 ? b : b & (0x3F >> more);
            for (int j = 1; j <= more; j++) {
                if ((t[i + j] >> 6) != 2) return DABGPU_ERR_ARG;
                cp = (cp << 6) | (t[i + j] & 0x3F);
            }
            // no overlong form, no surrogate, nothing above U+10FFFF, no NUL inside a C string
            static const uint32_t least[4] = {0x01, 0x80, 0x800, 0x10000};
            if (cp < least[more] || cp > 0x10FFFF || (cp >= 0xD800 && cp <= 0xDFFF)) return DABGPU_ERR_ARG;
            for (int j = 0; j <= more; j++) put(t[i + j]);
            i += more + 1;
        }
    } else if (label->charset == 6) {
        if (n & 1) return DABGPU_ERR_ARG;
        for (int i = 0; i < n; i += 2) {
            const uint32_t cp = (uint32_t(t[i]) << 8) | t[i + 1];
            if (cp == 0 || (cp >= 0xD800 && cp <= 0xDFFF)) return DABGPU_ERR_ARG;     // (UCS-2 has no surrogate pairs)
            if (cp < 0x80) {
                put(cp);
            } else if (cp < 0x800) {
                put(0xC0 | (cp >> 6));
                put(0x80 | (cp & 0x3F));
            } else {
                put(0xE0 | (cp >> 12));
                put(0x80 | ((cp >> 6) & 0x3F));
                put(0x80 | (cp & 0x3F));
            }
        }
    } else {
        return DABGPU_ERR_PROFILE;
    }
    if (at >= cap) return DABGPU_ERR_CAPACITY;                         // (nothing written)
    std::memcpy(out, text, size_t(at));
    out[at] = 0;
    return at;
}
