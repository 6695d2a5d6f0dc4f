// dabgpu_mp2_api.hip -- the C ABI of following DAB (MPEG layer II) sub-channels (include/dabgpu.h, "Following every DAB
// (MPEG layer II) sub-channel") and of taking their checked frames on to sub-band samples and audio levels: each batch call
// on device memory and its twin on host memory (no context, no GPU: the same code, include/dabgpu_mp2_frame.h and
// include/dabgpu_mp2_audio.h).
#include "dabgpu_ctx.hpp"

#include <cstring>

#include "../../include/dabgpu_mp2_audio.h"
#include "../../include/dabgpu_mp2_frame.h"

using namespace dabapi;
namespace mp2 = dabgpu_mp2;

static_assert(sizeof(dabgpu_mp2_result) == sizeof(mp2::Result), "ABI struct mirrors the header-only code's");
static_assert(DABGPU_MP2_ROW_BYTES == mp2::ROW_BYTES && DABGPU_MP2_PAD_KBPS == mp2::PAD_KBPS, "one row layout");
static_assert(sizeof(dabgpu_superframe_status) == 64 && sizeof(dabgpu_dabplus_follow_result) == 32, "records the PAD calls read");

size_t dabgpu_mp2_carry_bytes(int bitrate_kbps) { return mp2::bitrate_ok(bitrate_kbps) ? size_t(mp2::carry_bytes(bitrate_kbps)) : 0; }

// everything both calls refuse, before anything is done; fills the kernels' table when there is one
static int mp2_check(const dabgpu_mp2_entry *entries, int n_entries, int n_cifs, dabk::Mp2Entry *table) {
    if (n_entries < 0 || n_cifs < 0 || n_cifs > (1 << 28) || (n_entries > 0 && !entries)) return DABGPU_ERR_ARG;
    for (int i = 0; i < n_entries; i++) {
        const dabgpu_mp2_entry &e = entries[i];
        if (!mp2::bitrate_ok(e.bitrate_kbps)) return DABGPU_ERR_ARG;
        if (e.in_stride < size_t(3) * size_t(e.bitrate_kbps)) return DABGPU_ERR_ARG;
        if (n_cifs > 0 && !e.d_in) return DABGPU_ERR_ARG;
        if (!e.d_rows || !e.d_status || !e.d_follow || !e.d_carry_out || !e.d_result) return DABGPU_ERR_ARG;
        if ((addr(e.d_carry_in) | addr(e.d_carry_out)) & 15) return DABGPU_ERR_ARG;
        if ((addr(e.d_status) | addr(e.d_follow) | addr(e.d_result)) & 3) return DABGPU_ERR_ARG;
        const uint64_t cb = uint64_t(mp2::carry_bytes(e.bitrate_kbps));
        if (e.d_carry_in && overlaps(e.d_carry_in, cb, e.d_carry_out, cb)) return DABGPU_ERR_ARG;
        if (!table) continue;
        dabk::Mp2Entry &t = table[i];
        t.in = addr(e.d_in);
        t.carry_in = addr(e.d_carry_in);
        t.carry_out = addr(e.d_carry_out);
        t.rows = addr(e.d_rows);
        t.status = addr(e.d_status);
        t.follow = addr(e.d_follow);
        t.result = addr(e.d_result);
        t.in_stride = e.in_stride;
        t.bitrate = e.bitrate_kbps;
    }
    return DABGPU_OK;
}

int dabgpu_mp2_follow_dev(dabgpu_ctx *ctx, const dabgpu_mp2_entry *entries, int n_entries, int n_cifs, void *stream) {
    if (!ctx) return DABGPU_ERR_ARG;
    // everything is checked before anything is enqueued: a refused call leaves every output as it was
    std::vector<dabk::Mp2Entry> table(size_t(n_entries > 0 ? n_entries : 0), dabk::Mp2Entry{});
    const int bad = mp2_check(entries, n_entries, n_cifs, table.data());
    if (bad) return bad;
    if (n_entries == 0) return DABGPU_OK;
    const size_t table_bytes = dabk::mp2_table_bytes(n_entries);
    return launch_entry_table(ctx, STAGE_MP2, table_bytes, stream, [&](void *d_table, size_t slot_bytes, hipStream_t s) {
        return dabk::launch_mp2_follow(table.data(), n_entries, n_cifs, d_table, slot_bytes, s);
    });
}

int dabgpu_mp2_follow_host(const dabgpu_mp2_entry *entries, int n_entries, int n_cifs) {
    const int bad = mp2_check(entries, n_entries, n_cifs, nullptr);
    if (bad) return bad;
    for (int n = 0; n < n_entries; n++) {
        const dabgpu_mp2_entry &e = entries[n];
        const int B = e.bitrate_kbps, lf = 3 * B;
        mp2::Carry cy = {0, 0, 0};
        if (e.d_carry_in) {
            int32_t h[4];
            std::memcpy(h, e.d_carry_in, sizeof h);
            cy = mp2::read_carry(h[0], h[1], h[2], h[3]);
        }
        const int T = cy.held + n_cifs;
        auto frame = [&](int i) {
            return i < cy.held ? static_cast<const uint8_t *>(e.d_carry_in) + mp2::CARRY_HEADER : e.d_in + size_t(i - cy.held) * e.in_stride;
        };
        auto header = [&](int i) { const uint8_t *f = frame(i); return mp2::header_word(f[0], f[1], f[2], f[3]); };
        int hits1 = 0, votes0[2] = {0, 0};
        for (int i = 0; i < T; i++) {
            const int id = mp2::header_id(header(i), B);
            if (id == 1) hits1++;
            if (id == 0) votes0[i & 1]++;
        }
        const mp2::Plan p = mp2::decide(cy, T, hits1, votes0[0], votes0[1]);
        const int per = mp2::slot_frames(p.rate), L = per * lf, want_id = p.rate == mp2::RATE_48K ? 1 : 0;
        int mode = -1;
        for (int i = p.phase; p.rate != mp2::RATE_NONE && i < T && mode < 0; i += per)
            if (mp2::header_id(header(i), B) == want_id) mode = mp2::header_mode(header(i));
        mp2::Result r = mp2::plan_result(p, B, hits1 + votes0[0] + votes0[1], mode);
        for (int k = 0; k < p.n_rows; k++) {
            mp2::TwoPart tp;
            tp.a = frame(p.phase + per * k);
            tp.b = per == 2 ? frame(p.phase + per * k + 1) : tp.a + lf;
            tp.split = lf;
            int c = 0;
            const int kind = mp2::parse_frame(tp, L, B, want_id, &c);
            r.header_errors += kind == mp2::FRAME_HEADER_ERROR;
            r.frames_no_crc += kind == mp2::FRAME_NO_CRC;
            r.crc_failed += kind == mp2::FRAME_CRC_FAILED;
            const int x = kind == mp2::FRAME_GOOD ? mp2::xpad_bytes(L, c) : -1;
            uint8_t *row = e.d_rows + size_t(k) * mp2::ROW_BYTES;
            for (int j = 0; j < mp2::ROW_BYTES; j++) row[j] = x >= 0 ? mp2::row_byte(tp, L, c, x, j) : 0;
            int32_t st[16];
            for (int w = 0; w < 16; w++) st[w] = mp2::status_word(w, x);
            std::memcpy(e.d_status + k, st, sizeof st);
        }
        // the carry record, whole: header, the held frame, zeros behind it (the held frame may come out of carry_in, which
        // does not overlap carry_out)
        uint8_t *co = static_cast<uint8_t *>(e.d_carry_out);
        const int32_t h[4] = {p.synced, p.kept, p.synced ? p.rate : 0, mp2::CARRY_MAGIC};
        std::memcpy(co, h, sizeof h);
        std::memset(co + mp2::CARRY_HEADER, 0, size_t(mp2::carry_bytes(B) - mp2::CARRY_HEADER));
        if (p.kept) std::memcpy(co + mp2::CARRY_HEADER, frame(p.first_kept), size_t(lf));
        dabgpu_dabplus_follow_result fr;
        std::memset(&fr, 0, sizeof fr);
        fr.n_superframes = p.n_rows; fr.phase = p.phase; fr.synced = p.synced; fr.dropped = p.dropped;
        fr.raw_hits = r.hits; fr.held = p.kept;
        std::memcpy(e.d_follow, &fr, sizeof fr);
        std::memcpy(e.d_result, &r, sizeof r);
    }
    return DABGPU_OK;
}

// ---- sub-band samples and audio levels (include/dabgpu.h, "Layer-II services of a batch: sub-band samples and audio levels")
static_assert(sizeof(dabgpu_mp2_level) == sizeof(mp2::Level) && sizeof(dabgpu_mp2_audio_result) == sizeof(mp2::AudioResult),
              "ABI structs mirror the header-only code's");

// everything both calls refuse, before anything is done; fills the kernels' table when there is one
static int mp2_audio_check(const dabgpu_mp2_audio_entry *entries, int n_entries, int n_cifs, dabk::Mp2AudioEntry *table) {
    if (n_entries < 0 || n_cifs < 0 || n_cifs > (1 << 28) || (n_entries > 0 && !entries)) return DABGPU_ERR_ARG;
    for (int i = 0; i < n_entries; i++) {
        const dabgpu_mp2_audio_entry &e = entries[i];
        if (!mp2::bitrate_ok(e.bitrate_kbps)) return DABGPU_ERR_ARG;
        if (e.in_stride < size_t(3) * size_t(e.bitrate_kbps)) return DABGPU_ERR_ARG;
        if (n_cifs > 0 && !e.d_in) return DABGPU_ERR_ARG;
        if (!e.d_status || !e.d_result || !e.d_levels || !e.d_audio) return DABGPU_ERR_ARG;
        if ((addr(e.d_carry_in) | addr(e.d_subbands)) & 15) return DABGPU_ERR_ARG;
        if ((addr(e.d_status) | addr(e.d_result) | addr(e.d_levels) | addr(e.d_audio)) & 3) return DABGPU_ERR_ARG;
        if (!table) continue;
        dabk::Mp2AudioEntry &t = table[i];
        t.in = addr(e.d_in);
        t.carry_in = addr(e.d_carry_in);
        t.status = addr(e.d_status);
        t.result = addr(e.d_result);
        t.levels = addr(e.d_levels);
        t.subbands = addr(e.d_subbands);
        t.audio = addr(e.d_audio);
        t.in_stride = e.in_stride;
        t.bitrate = e.bitrate_kbps;
    }
    return DABGPU_OK;
}

int dabgpu_mp2_subbands_dev(dabgpu_ctx *ctx, const dabgpu_mp2_audio_entry *entries, int n_entries, int n_cifs, void *stream) {
    if (!ctx) return DABGPU_ERR_ARG;
    // everything is checked before anything is enqueued: a refused call leaves every output as it was
    std::vector<dabk::Mp2AudioEntry> table(size_t(n_entries > 0 ? n_entries : 0), dabk::Mp2AudioEntry{});
    const int bad = mp2_audio_check(entries, n_entries, n_cifs, table.data());
    if (bad) return bad;
    if (n_entries == 0) return DABGPU_OK;
    const size_t table_bytes = dabk::mp2_audio_table_bytes(n_entries);
    return launch_entry_table(ctx, STAGE_MP2_AUDIO, table_bytes, stream, [&](void *d_table, size_t slot_bytes, hipStream_t s) {
        return dabk::launch_mp2_subbands(table.data(), n_entries, n_cifs, d_table, slot_bytes, s);
    });
}

int dabgpu_mp2_subbands_host(const dabgpu_mp2_audio_entry *entries, int n_entries, int n_cifs) {
    const int bad = mp2_audio_check(entries, n_entries, n_cifs, nullptr);
    if (bad) return bad;
    for (int n = 0; n < n_entries; n++) {
        const dabgpu_mp2_audio_entry &e = entries[n];
        const int B = e.bitrate_kbps, lf = 3 * B;
        mp2::AudioResult tally = {};
        mp2::Result res;
        std::memcpy(&res, e.d_result, sizeof res);
        mp2::Carry cy = {0, 0, 0};
        if (e.d_carry_in) {
            int32_t h[4];
            std::memcpy(h, e.d_carry_in, sizeof h);
            cy = mp2::read_carry(h[0], h[1], h[2], h[3]);
        }
        if ((res.id == 0 || res.id == 1) && (res.phase == 0 || res.phase == 1)) {
            const int per = res.id == 1 ? 1 : 2, L = per * lf;
            const int fit = (cy.held + n_cifs - res.phase) / per, frames = res.frames < fit ? res.frames : fit;
            auto frame = [&](int i) {
                return i < cy.held ? static_cast<const uint8_t *>(e.d_carry_in) + mp2::CARRY_HEADER : e.d_in + size_t(i - cy.held) * e.in_stride;
            };
            for (int k = 0; k < frames; k++) {
                mp2::TwoPart tp;
                tp.a = frame(res.phase + per * k);
                tp.b = per == 2 ? frame(res.phase + per * k + 1) : tp.a + lf;
                tp.split = lf;
                int32_t mask;
                std::memcpy(&mask, reinterpret_cast<const int32_t *>(e.d_status + k) + 4, sizeof mask);
                float *v = e.d_subbands ? e.d_subbands + size_t(k) * mp2::FRAME_VALUES : nullptr;
                mp2::Level lv = mp2::empty_level(mp2::AUDIO_NOT_GOOD);
                if (mask == 1) lv = mp2::decode_frame(tp, L, B, res.id, v);
                else if (v) std::memset(v, 0, sizeof(float) * mp2::FRAME_VALUES);
                std::memcpy(e.d_levels + k, &lv, sizeof lv);
                tally.decoded += lv.kind == mp2::AUDIO_DECODED;
                tally.not_good += lv.kind == mp2::AUDIO_NOT_GOOD;
                tally.overrun += lv.kind == mp2::AUDIO_OVERRUN;
                tally.silent += lv.kind == mp2::AUDIO_DECODED && lv.power[0] + lv.power[1] == 0.0f;
            }
        }
        std::memcpy(e.d_audio, &tally, sizeof tally);
    }
    return DABGPU_OK;
}
