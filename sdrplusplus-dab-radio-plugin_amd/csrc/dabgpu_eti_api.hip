// dabgpu_eti_api.hip -- the ETI(NI) entry points of the C ABI (include/dabgpu.h, "ETI(NI) output"): the host-side
// layout and reader, and the device call that turns a decode call's buffers into frames (eti_kernels.hip) -- and, behind
// them, the same for EDI ("EDI output" / "EDI input"; edi_kernels.hip): one file for the contribution formats, which share
// the plan, its checks and the CRC constants.
#include "dabgpu_ctx.hpp"

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>

#include "../../include/dabgpu_edi.h"
#include "../../include/dabgpu_eti_read.h"

using namespace dabapi;

static_assert(sizeof(dabgpu_eti_history) == sizeof(dabk::EtiHistory) && sizeof(dabgpu_eti_status) == sizeof(dabk::EtiStatus),
              "ABI structs mirror the kernels'");
static_assert(offsetof(dabgpu_eti_history, crc_ok) == offsetof(dabk::EtiHistory, crc_ok) &&
              offsetof(dabgpu_eti_history, next_count) == offsetof(dabk::EtiHistory, next_count) &&
              offsetof(dabgpu_eti_history, valid) == offsetof(dabk::EtiHistory, valid), "ABI structs mirror the kernels'");
static_assert(DABGPU_ETI_FRAME_BYTES == dabk::ETI_FRAME_BYTES && DABGPU_ETI_MAX_STREAMS == dabk::ETI_MAX_STREAMS &&
              DABGPU_ETI_FIC_DELAY == dabk::ETI_FIC_DELAY, "ABI constants mirror the kernels'");

namespace {

constexpr int FIC_BYTES = dabk::ETI_FIC_BYTES;

// ---- CRC-16 (x^16 + x^12 + x^5 + 1) as polynomial arithmetic over GF(2)
uint32_t gf_mul(uint32_t a, uint32_t b) {
    uint32_t r = 0;
    for (int i = 15; i >= 0; i--) {
        r <<= 1;
        if (r & 0x10000u) r ^= 0x11021u;
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}

// x^n mod P
uint32_t gf_xpow(unsigned long long n) {
    uint32_t r = 1, sq = 2;
    for (; n; n >>= 1) {
        if (n & 1u) r = gf_mul(r, sq);
        sq = gf_mul(sq, sq);
    }
    return r;
}

// start 0xFFFF, result inverted
uint32_t crc16(const uint8_t *p, size_t n) {
    uint32_t crc = 0xFFFFu;
    for (size_t i = 0; i < n; i++) {
        crc ^= uint32_t(p[i]) << 8;
        for (int b = 0; b < 8; b++) crc = (crc & 0x8000u) ? ((crc << 1) ^ 0x1021u) & 0xFFFFu : (crc << 1) & 0xFFFFu;
    }
    return crc ^ 0xFFFFu;
}

// what dabgpu_eti_layout guarantees, checked again on a plan handed to the device call (it sizes every access of the kernels)
bool plan_consistent(const dabgpu_eti_plan &p) {
    if (p.nst < 0 || p.nst > DABGPU_ETI_MAX_STREAMS || p.header_bytes != 12 + 4 * p.nst) return false;
    bool seen[DABGPU_ETI_MAX_STREAMS] = {};
    int off = 0;
    for (int k = 0; k < p.nst; k++) {
        if (p.order[k] < 0 || p.order[k] >= p.nst || seen[p.order[k]]) return false;
        seen[p.order[k]] = true;
        if (p.bytes[k] <= 0 || p.bytes[k] % 24 || p.bytes[k] > 8 * 1023 || p.offset[k] != off) return false;
        off += p.bytes[k];
    }
    return p.data_bytes == off && p.length == p.header_bytes + FIC_BYTES + off + 8 && p.length <= DABGPU_ETI_FRAME_BYTES &&
           p.fl * 4 + 16 == p.length;
}

}  // namespace

extern "C" {

size_t dabgpu_eti_history_bytes(void) { return sizeof(dabgpu_eti_history); }

int dabgpu_eti_layout(const dabgpu_eti_stream *streams, int n, dabgpu_eti_plan *plan) {
    if (!plan || n < 0 || n > DABGPU_ETI_MAX_STREAMS || (n > 0 && !streams)) return DABGPU_ERR_ARG;
    char used[864] = {};
    for (int i = 0; i < n; i++) {
        const dabgpu_subchannel &sc = streams[i].sc;
        if (streams[i].subchannel_id < 0 || streams[i].subchannel_id > 63) return DABGPU_ERR_ARG;
        if (sc.start_address < 0 || sc.length <= 0 || sc.start_address > 863 || sc.length > 864 - sc.start_address) return DABGPU_ERR_ARG;
        if (sc.bitrate_kbps <= 0 || sc.bitrate_kbps % 8 || sc.bitrate_kbps * 3 / 8 > 1023) return DABGPU_ERR_ARG;
        if (sc.is_uep ? (sc.is_uep != 1 || sc.protection_level < 1 || sc.protection_level > 5)
                      : (sc.protection_level < 1 || sc.protection_level > 4 || sc.eep_type < 0 || sc.eep_type > 1))
            return DABGPU_ERR_ARG;
        for (int cu = sc.start_address; cu < sc.start_address + sc.length; cu++) {
            if (used[cu]) return DABGPU_ERR_ARG;
            used[cu] = 1;
        }
    }
    dabgpu_eti_plan p;
    std::memset(&p, 0, sizeof p);
    p.nst = n;
    for (int k = 0; k < n; k++) p.order[k] = k;
    std::sort(p.order, p.order + n, [&](int a, int b) { return streams[a].sc.start_address < streams[b].sc.start_address; });
    int stl_sum = 0;
    for (int k = 0; k < n; k++) {
        const dabgpu_eti_stream &st = streams[p.order[k]];
        const int stl = st.sc.bitrate_kbps * 3 / 8;
        const int tpl = st.sc.is_uep ? 0x10 | (st.sc.protection_level - 1) : 0x20 | (st.sc.eep_type << 2) | (st.sc.protection_level - 1);
        p.offset[k] = 8 * stl_sum;
        p.bytes[k] = 8 * stl;
        stl_sum += stl;
        uint8_t *stc = p.header + 8 + 4 * k;
        stc[0] = uint8_t((st.subchannel_id << 2) | (st.sc.start_address >> 8));
        stc[1] = uint8_t(st.sc.start_address & 0xff);
        stc[2] = uint8_t((tpl << 2) | (stl >> 8));
        stc[3] = uint8_t(stl & 0xff);
    }
    p.fl = n + 1 + 24 + 2 * stl_sum;
    p.header_bytes = 12 + 4 * n;
    p.data_bytes = 8 * stl_sum;
    p.length = 4 * p.fl + 16;
    if (p.length > DABGPU_ETI_FRAME_BYTES) return DABGPU_ERR_ARG;
    p.header[5] = uint8_t(0x80 | n);
    p.header[6] = uint8_t((1 << 3) | (p.fl >> 8));             // FP = 0, MID = 1
    p.header[7] = uint8_t(p.fl & 0xff);
    p.header[8 + 4 * n] = 0xFF;                                // MNSC
    p.header[9 + 4 * n] = 0xFF;
    *plan = p;
    return DABGPU_OK;
}

int dabgpu_eti_frames_dev(dabgpu_ctx *ctx, const dabgpu_eti_plan *plan, int n_streams, int frames_per_stream,
                          const uint8_t *d_fib, const uint8_t *d_crc_ok, const uint8_t *const *d_out,
                          const dabgpu_eti_history *d_history_in, dabgpu_eti_history *d_history_out,
                          const int32_t *d_cif_start, uint8_t *d_eti, dabgpu_eti_status *d_status, void *stream) {
    if (!ctx || !plan || !d_fib || !d_crc_ok || !d_eti || !d_status || n_streams < 0 || frames_per_stream < 0) return DABGPU_ERR_ARG;
    if (!plan_consistent(*plan) || (plan->nst > 0 && !d_out)) return DABGPU_ERR_ARG;
    if ((addr(d_fib) & 3u) || (addr(d_eti) & 15u) || (addr(d_status) & 7u) || (addr(d_history_in) & 7u) ||
        (addr(d_history_out) & 7u) || (addr(d_cif_start) & 3u))
        return DABGPU_ERR_ARG;
    if (d_history_in && static_cast<const void *>(d_history_in) == static_cast<const void *>(d_history_out)) return DABGPU_ERR_ARG;
    for (int i = 0; i < plan->nst; i++)
        if (!d_out[i] || (addr(d_out[i]) & 7u)) return DABGPU_ERR_ARG;
    if (size_t(n_streams) * size_t(frames_per_stream) * 4u > size_t(0x7fffffff) / 4u) return DABGPU_ERR_ARG;
    if (n_streams == 0 || frames_per_stream == 0) return DABGPU_OK;
    DeviceGuard guard(ctx);

    void *base = nullptr;
    int rc = stage(ctx, STAGE_ETI_COUNTS, size_t(n_streams) * sizeof(int32_t), &base);
    if (rc) return rc;

    dabk::EtiArgs a{};
    const int nst = plan->nst;
    for (int k = 0; k < nst; k++) {
        a.out[k] = d_out[plan->order[k]];
        a.offset[k] = uint16_t(plan->offset[k]);
        a.bytes[k] = uint16_t(plan->bytes[k]);
    }
    // the constant part of the header: the caller's plan is read for its numbers only, the bytes are laid out again
    uint8_t hdr[16 + 4 * DABGPU_ETI_MAX_STREAMS] = {};
    std::memcpy(hdr + 8, plan->header + 8, size_t(4 * nst));
    hdr[5] = uint8_t(0x80 | nst);
    hdr[6] = uint8_t((1 << 3) | (plan->fl >> 8));
    hdr[7] = uint8_t(plan->fl & 0xff);
    hdr[8 + 4 * nst] = 0xFF;
    hdr[9 + 4 * nst] = 0xFF;
    std::memcpy(a.header, hdr, size_t(8 + 4 * nst));
    const int header_crc_bytes = 6 + 4 * nst;                  // FC, STC, MNSC
    a.header_crc0 = uint16_t(crc16(hdr + 4, size_t(header_crc_bytes)));
    a.fct_shift = uint16_t(gf_xpow(8ull * unsigned(header_crc_bytes - 1) + 16));
    a.fp_shift = uint16_t(gf_xpow(8ull * unsigned(header_crc_bytes - 3) + 16));
    const int data_len = FIC_BYTES + plan->data_bytes;         // a multiple of 8
    a.chunk_words = (data_len / 4 + 63) / 64;
    for (int lane = 0; lane < 64; lane++) a.lane_shift[lane] = uint16_t(gf_xpow(32ull * unsigned(a.chunk_words) * unsigned(63 - lane)));
    a.data_init = uint16_t(gf_mul(0xFFFFu, gf_xpow(8ull * unsigned(data_len))));
    a.fib = d_fib;
    a.crc_ok = d_crc_ok;
    a.history_in = reinterpret_cast<const dabk::EtiHistory *>(d_history_in);
    a.base = static_cast<const int32_t *>(base);
    a.eti = d_eti;
    a.status = reinterpret_cast<dabk::EtiStatus *>(d_status);
    a.n_streams = n_streams;
    a.frames_per_stream = frames_per_stream;
    a.nst = nst;
    a.data_bytes = plan->data_bytes;

    dabk::EtiAnchorArgs p{};
    p.fib = d_fib;
    p.crc_ok = d_crc_ok;
    p.history_in = a.history_in;
    p.history_out = reinterpret_cast<dabk::EtiHistory *>(d_history_out);
    p.cif_start = d_cif_start;
    p.base = static_cast<int32_t *>(base);
    p.n_streams = n_streams;
    p.frames_per_stream = frames_per_stream;

    hipStream_t s = pick_stream(ctx, stream);
    ScopedTimer timer(ctx, TIMER_ETI, s);
    HIP_TRY(dabk::launch_eti(p, a, s));
    return DABGPU_OK;
}

int dabgpu_eti_parse(const uint8_t *f, dabgpu_eti_info *info) {
    if (!f || !info) return DABGPU_ERR_ARG;
    dabgpu_eti_info r;
    std::memset(&r, 0, sizeof r);
    const auto done = [&](int code) { *info = r; return code; };
    r.err = f[0];
    r.fct = f[4];
    r.nst = f[5] & 0x7f;
    r.fp = f[6] >> 5;
    r.mid = (f[6] >> 3) & 3;
    r.fl = ((f[6] & 7) << 8) | f[7];
    r.length = 4 * r.fl + 16;
    const bool even = f[1] == 0x07 && f[2] == 0x3A && f[3] == 0xB6, odd = f[1] == 0xF8 && f[2] == 0xC5 && f[3] == 0x49;
    if (!(even || odd) || odd != bool(r.fct & 1) || r.fct >= 250) return done(DABGPU_ETI_BAD_SYNC);
    if (!(f[5] & 0x80) || r.mid != 1 || r.nst > DABGPU_ETI_MAX_STREAMS) return done(DABGPU_ETI_BAD_HEADER);
    int stl_sum = 0;
    for (int k = 0; k < r.nst; k++) {
        const uint8_t *stc = f + 8 + 4 * k;
        r.scid[k] = stc[0] >> 2;
        r.sad[k] = ((stc[0] & 3) << 8) | stc[1];
        r.tpl[k] = stc[2] >> 2;
        r.stl[k] = ((stc[2] & 3) << 8) | stc[3];
        r.offset[k] = 12 + 4 * r.nst + FIC_BYTES + 8 * stl_sum;
        stl_sum += r.stl[k];
    }
    r.fic_offset = 12 + 4 * r.nst;
    if (r.fl != r.nst + 1 + 24 + 2 * stl_sum || r.length > DABGPU_ETI_FRAME_BYTES) return done(DABGPU_ETI_BAD_HEADER);
    const int crc_at = 10 + 4 * r.nst;
    r.header_crc = (f[crc_at] << 8) | f[crc_at + 1];
    const int eof_at = r.fic_offset + FIC_BYTES + 8 * stl_sum;
    r.data_crc = (f[eof_at] << 8) | f[eof_at + 1];
    if (uint32_t(r.header_crc) != crc16(f + 4, size_t(6 + 4 * r.nst))) return done(DABGPU_ETI_BAD_HEADER_CRC);
    if (uint32_t(r.data_crc) != crc16(f + r.fic_offset, size_t(FIC_BYTES + 8 * stl_sum))) return done(DABGPU_ETI_BAD_DATA_CRC);
    return done(DABGPU_OK);
}

}  // extern "C"

// ---- ETI(NI) input (include/dabgpu.h, "ETI(NI) input"; include/dabgpu_eti_read.h) -------------------------------------------
namespace er = dabgpu_eti_read;

static_assert(sizeof(dabgpu_eti_read_status) == sizeof(er::Status) && sizeof(dabgpu_eti_read_result) == sizeof(er::Result) &&
                  sizeof(dabgpu_eti_read_entry) == 80,
              "ABI structs mirror the header's");
static_assert(offsetof(dabgpu_eti_read_status, gap) == offsetof(er::Status, gap) &&
                  offsetof(dabgpu_eti_read_result, tail_bytes) == offsetof(er::Result, tail_bytes),
              "ABI structs mirror the header's");
static_assert(DABGPU_ETI_OTHER_PLAN == er::OTHER_PLAN && DABGPU_ETI_BAD_DATA_CRC == er::BAD_DATA_CRC &&
                  DABGPU_ETI_READ_GAP == er::FLAG_GAP && DABGPU_ETI_READ_FP_BREAK == er::FLAG_FP_BREAK &&
                  DABGPU_ETI_READ_ERR_FIELD == er::FLAG_ERR_FIELD && DABGPU_ETI_READ_FIB_CRC == er::FLAG_FIB_CRC,
              "verdicts and flags");

namespace {

constexpr int32_t ETI_READ_MAX_BYTES = 1 << 30;

// everything both calls refuse, before anything is done; fills the kernels' table when there is one
int eti_read_check(const dabgpu_eti_read_entry *entries, int n_entries, dabk::EtiReadEntry *table) {
    if (n_entries < 0 || (n_entries > 0 && !entries)) return DABGPU_ERR_ARG;
    for (int i = 0; i < n_entries; i++) {
        const dabgpu_eti_read_entry &e = entries[i];
        if (e.n_bytes < 0 || e.n_bytes > ETI_READ_MAX_BYTES || (e.n_bytes > 0 && !e.d_bytes)) return DABGPU_ERR_ARG;
        if (!e.d_state_out || !e.d_result) return DABGPU_ERR_ARG;
        const int max_frames = (e.n_bytes + er::MAX_TAIL) / er::FRAME_BYTES;
        if (max_frames > 0 && (!e.d_fib || !e.d_crc_ok || !e.d_status)) return DABGPU_ERR_ARG;
        if ((addr(e.d_bytes) | addr(e.d_state_in) | addr(e.d_state_out) | addr(e.d_fib) | addr(e.d_status)) & 15) return DABGPU_ERR_ARG;
        if (addr(e.d_result) & 3) return DABGPU_ERR_ARG;
        const uint64_t sb = er::STATE_BYTES;
        if (e.d_state_in && overlaps(e.d_state_in, sb, e.d_state_out, sb)) return DABGPU_ERR_ARG;
        if (e.plan) {
            const dabgpu_eti_plan &p = *e.plan;
            if (!plan_consistent(p)) return DABGPU_ERR_ARG;
            for (int k = 0; k < p.nst; k++) {
                // the STC's own length is what a frame is compared with: it must be what the moves are sized by
                const uint8_t *stc = p.header + 8 + 4 * k;
                if (8 * (((stc[2] & 3) << 8) | stc[3]) != p.bytes[k]) return DABGPU_ERR_ARG;
                if (e.d_out && (addr(e.d_out[k]) & 7)) return DABGPU_ERR_ARG;
            }
        }
    }
    if (!table) return DABGPU_OK;
    for (int i = 0; i < n_entries; i++) {
        const dabgpu_eti_read_entry &e = entries[i];
        dabk::EtiReadEntry &t = table[i];
        t.bytes = addr(e.d_bytes);
        t.state_in = addr(e.d_state_in);
        t.state_out = addr(e.d_state_out);
        t.fib = addr(e.d_fib);
        t.crc_ok = addr(e.d_crc_ok);
        t.status = addr(e.d_status);
        t.result = addr(e.d_result);
        t.n_bytes = e.n_bytes;
        t.max_frames = (e.n_bytes + er::MAX_TAIL) / er::FRAME_BYTES;
        if (!e.plan) continue;
        const dabgpu_eti_plan &p = *e.plan;
        t.has_plan = 1;
        t.nst = p.nst;
        t.fl = p.fl;
        t.data_bytes = FIC_BYTES + p.data_bytes;
        t.chunk_words = (t.data_bytes / 4 + 63) / 64;
        for (int k = 0; k < p.nst; k++) {
            t.out[k] = e.d_out ? addr(e.d_out[p.order[k]]) : 0;
            t.offset[k] = uint16_t(p.offset[k]);
            t.nbytes[k] = uint16_t(p.bytes[k]);
        }
        std::memcpy(t.stc, p.header + 8, size_t(4 * p.nst));
        // the constants of the data CRC depend on the length alone: the entries of a batch mostly share them
        if (i > 0 && table[i - 1].has_plan && table[i - 1].data_bytes == t.data_bytes) {
            std::memcpy(t.lane_shift, table[i - 1].lane_shift, sizeof t.lane_shift);
            t.data_init = table[i - 1].data_init;
            continue;
        }
        for (int lane = 0; lane < 64; lane++) t.lane_shift[lane] = uint16_t(gf_xpow(32ull * unsigned(t.chunk_words) * unsigned(63 - lane)));
        t.data_init = uint16_t(gf_mul(0xFFFFu, gf_xpow(8ull * unsigned(t.data_bytes))));
    }
    return DABGPU_OK;
}

}  // namespace

extern "C" {

size_t dabgpu_eti_read_state_bytes(void) { return size_t(er::STATE_BYTES); }

int dabgpu_eti_read_dev(dabgpu_ctx *ctx, const dabgpu_eti_read_entry *entries, int n_entries, void *stream) {
    if (!ctx) return DABGPU_ERR_ARG;
    // everything is checked before anything is enqueued: a refused call leaves every output as it was
    std::vector<dabk::EtiReadEntry> table(size_t(n_entries > 0 ? n_entries : 0), dabk::EtiReadEntry{});
    const int bad = eti_read_check(entries, n_entries, table.data());
    if (bad) return bad;
    if (n_entries == 0) return DABGPU_OK;
    size_t table_bytes = table.size() * sizeof(dabk::EtiReadEntry) + dabk::eti_read_bases_bytes(n_entries);
    for (const dabk::EtiReadEntry &t : table) table_bytes += dabk::eti_read_scratch_bytes(t.n_bytes);
    return launch_entry_table(ctx, STAGE_ETI_READ, table_bytes, stream, [&](void *d_table, size_t, hipStream_t s) {
        return dabk::launch_eti_read(table.data(), n_entries, d_table, s);
    });
}

int dabgpu_eti_read_host(const dabgpu_eti_read_entry *entries, int n_entries) {
    const int bad = eti_read_check(entries, n_entries, nullptr);
    if (bad) return bad;
    std::vector<uint8_t> s;
    for (int i = 0; i < n_entries; i++) {
        const dabgpu_eti_read_entry &e = entries[i];
        er::Head in{};
        if (e.d_state_in) std::memcpy(&in, e.d_state_in, sizeof in);
        const size_t tail = er::clamp_tail(in.tail_bytes);
        s.resize(tail + size_t(e.n_bytes));
        if (tail) std::memcpy(s.data(), static_cast<const uint8_t *>(e.d_state_in) + er::STATE_HEAD_BYTES, tail);
        if (e.n_bytes) std::memcpy(s.data() + tail, e.d_bytes, size_t(e.n_bytes));
        er::PlanKey key{};
        uint8_t *out[DABGPU_ETI_MAX_STREAMS] = {};
        if (e.plan) {
            key.nst = e.plan->nst;
            key.fl = e.plan->fl;
            std::memcpy(key.stc, e.plan->header + 8, size_t(4 * key.nst));
            for (int k = 0; k < key.nst; k++) out[k] = e.d_out ? e.d_out[e.plan->order[k]] : nullptr;
        }
        er::HostOut o{};
        o.fib = e.d_fib;
        o.crc_ok = e.d_crc_ok;
        o.status = reinterpret_cast<er::Status *>(e.d_status);
        o.result = reinterpret_cast<er::Result *>(e.d_result);
        o.out = out;
        o.offset = e.plan ? e.plan->offset : nullptr;
        o.bytes = e.plan ? e.plan->bytes : nullptr;
        er::read_entry(s.data(), s.size(), in, e.plan ? &key : nullptr, o, static_cast<uint8_t *>(e.d_state_out));
    }
    return DABGPU_OK;
}

}  // extern "C"

// ---- EDI output and input (include/dabgpu.h, "EDI output" / "EDI input"; include/dabgpu_edi.h) ------------------------------
namespace ed = dabgpu_edi;

static_assert(sizeof(dabgpu_edi_read_status) == sizeof(ed::Status) && sizeof(dabgpu_edi_read_result) == sizeof(ed::Result) &&
                  sizeof(dabgpu_edi_read_entry) == sizeof(dabgpu_eti_read_entry),
              "ABI structs mirror the header's");
static_assert(offsetof(dabgpu_edi_read_status, flags) == offsetof(ed::Status, flags) &&
                  offsetof(dabgpu_edi_read_status, tsta) == offsetof(ed::Status, tsta) &&
                  offsetof(dabgpu_edi_read_result, tail_bytes) == offsetof(ed::Result, tail_bytes),
              "ABI structs mirror the header's");
static_assert(DABGPU_EDI_BAD_HEADER == ed::BAD_HEADER && DABGPU_EDI_BAD_CRC == ed::BAD_CRC && DABGPU_EDI_BAD_TAGS == ed::BAD_TAGS &&
                  DABGPU_EDI_NOT_DETI == ed::NOT_DETI && DABGPU_EDI_READ_GAP == ed::FLAG_GAP &&
                  DABGPU_EDI_READ_SEQ_BREAK == ed::FLAG_SEQ_BREAK && DABGPU_EDI_READ_FP_MISMATCH == ed::FLAG_FP_MISMATCH &&
                  DABGPU_EDI_READ_STAT_FIELD == ed::FLAG_STAT_FIELD && DABGPU_EDI_READ_FIB_CRC == ed::FLAG_FIB_CRC &&
                  DABGPU_EDI_READ_NO_FIC == ed::FLAG_NO_FIC && DABGPU_EDI_READ_TIME == ed::FLAG_TIME &&
                  DABGPU_EDI_MAX_PACKET == ed::MAX_PACKET,
              "verdicts, flags and constants");

namespace {

constexpr int32_t EDI_READ_MAX_BYTES = 1 << 30;

// the plan's STC words must say the sizes the plan's moves are made with
bool plan_stc_consistent(const dabgpu_eti_plan &p) {
    if (!plan_consistent(p)) return false;
    for (int k = 0; k < p.nst; k++) {
        const uint8_t *stc = p.header + 8 + 4 * k;
        if (8 * (((stc[2] & 3) << 8) | stc[3]) != p.bytes[k]) return false;
    }
    return true;
}

ed::PlanKey plan_key(const dabgpu_eti_plan &p) {
    ed::PlanKey key{};
    key.nst = p.nst;
    std::memcpy(key.stc, p.header + 8, size_t(4 * p.nst));
    return key;
}

// everything both calls refuse, before anything is done; fills the kernels' table when there is one
int edi_read_check(const dabgpu_edi_read_entry *entries, int n_entries, dabk::EdiReadEntry *table) {
    if (n_entries < 0 || (n_entries > 0 && !entries)) return DABGPU_ERR_ARG;
    for (int i = 0; i < n_entries; i++) {
        const dabgpu_edi_read_entry &e = entries[i];
        if (e.n_bytes < 0 || e.n_bytes > EDI_READ_MAX_BYTES || (e.n_bytes > 0 && !e.d_bytes)) return DABGPU_ERR_ARG;
        if (!e.d_state_out || !e.d_result) return DABGPU_ERR_ARG;
        if (e.plan && !plan_stc_consistent(*e.plan)) return DABGPU_ERR_ARG;
        if (!e.d_fib || !e.d_crc_ok || !e.d_status) return DABGPU_ERR_ARG;            // max_rows is never 0
        if ((addr(e.d_bytes) | addr(e.d_state_in) | addr(e.d_state_out) | addr(e.d_fib) | addr(e.d_status)) & 15) return DABGPU_ERR_ARG;
        if (addr(e.d_result) & 3) return DABGPU_ERR_ARG;
        const uint64_t sb = ed::STATE_BYTES;
        if (e.d_state_in && overlaps(e.d_state_in, sb, e.d_state_out, sb)) return DABGPU_ERR_ARG;
        if (e.plan && e.d_out)
            for (int k = 0; k < e.plan->nst; k++)
                if (addr(e.d_out[k]) & 7) return DABGPU_ERR_ARG;
    }
    if (!table) return DABGPU_OK;
    for (int i = 0; i < n_entries; i++) {
        const dabgpu_edi_read_entry &e = entries[i];
        dabk::EdiReadEntry &t = table[i];
        t.bytes = addr(e.d_bytes);
        t.state_in = addr(e.d_state_in);
        t.state_out = addr(e.d_state_out);
        t.fib = addr(e.d_fib);
        t.crc_ok = addr(e.d_crc_ok);
        t.status = addr(e.d_status);
        t.result = addr(e.d_result);
        t.n_bytes = e.n_bytes;
        t.max_rows = int32_t(ed::max_rows(uint32_t(e.n_bytes), e.plan ? e.plan->nst : 0, e.plan ? e.plan->data_bytes : 0));
        if (!e.plan) continue;
        t.has_plan = 1;
        t.nst = e.plan->nst;
        for (int k = 0; k < t.nst; k++) t.out[k] = e.d_out ? addr(e.d_out[e.plan->order[k]]) : 0;
        std::memcpy(t.stc, e.plan->header + 8, size_t(4 * t.nst));
    }
    return DABGPU_OK;
}

}  // namespace

extern "C" {

int dabgpu_edi_packet_bytes(const dabgpu_eti_plan *plan) {
    if (!plan || !plan_stc_consistent(*plan)) return DABGPU_ERR_ARG;
    return ed::packet_bytes(plan->nst, plan->data_bytes);
}

int dabgpu_edi_frames_dev(dabgpu_ctx *ctx, const dabgpu_eti_plan *plan, int n_streams, int frames_per_stream,
                          const uint8_t *d_fib, const uint8_t *d_crc_ok, const uint8_t *const *d_out,
                          const dabgpu_eti_history *d_history_in, dabgpu_eti_history *d_history_out,
                          const int32_t *d_cif_start, const uint32_t *seq_start, uint8_t *d_edi, size_t stream_stride,
                          dabgpu_eti_status *d_status, void *stream) {
    if (!ctx || !plan || !d_fib || !d_crc_ok || !d_edi || !d_status || n_streams < 0 || frames_per_stream < 0) return DABGPU_ERR_ARG;
    if (!plan_stc_consistent(*plan) || (plan->nst > 0 && !d_out)) return DABGPU_ERR_ARG;
    if ((addr(d_fib) & 3u) || (addr(d_edi) & 15u) || (addr(d_status) & 7u) || (addr(d_history_in) & 7u) ||
        (addr(d_history_out) & 7u) || (addr(d_cif_start) & 3u) || (stream_stride & 15u))
        return DABGPU_ERR_ARG;
    if (d_history_in && static_cast<const void *>(d_history_in) == static_cast<const void *>(d_history_out)) return DABGPU_ERR_ARG;
    for (int i = 0; i < plan->nst; i++)
        if (!d_out[i] || (addr(d_out[i]) & 7u)) return DABGPU_ERR_ARG;
    if (size_t(n_streams) * size_t(frames_per_stream) * 4u > size_t(0x7fffffff) / 4u) return DABGPU_ERR_ARG;
    const int packet = ed::packet_bytes(plan->nst, plan->data_bytes);
    if (packet > dabk::EDI_MAX_WRITER_PACKET || stream_stride < size_t(frames_per_stream) * 4u * size_t(packet)) return DABGPU_ERR_ARG;
    if (n_streams == 0 || frames_per_stream == 0) return DABGPU_OK;
    DeviceGuard guard(ctx);
    hipStream_t s = pick_stream(ctx, stream);

    // the stage area: [n_streams] counts of the pre-pass, then [n_streams] first sequence numbers
    const size_t stage_bytes = size_t(n_streams) * 8u;
    // (growing the area must not race with a launch that still reads the old one)
    if (ctx->stage_bytes[STAGE_EDI] < stage_bytes) HIP_TRY(hipStreamSynchronize(s));
    void *base = nullptr;
    const int rc = stage(ctx, STAGE_EDI, stage_bytes, &base);
    if (rc) return rc;
    uint32_t *d_seq = nullptr;
    if (seq_start) {
        d_seq = static_cast<uint32_t *>(base) + n_streams;
        // through a pageable copy: the transfer has left it when hipMemcpyAsync returns, so the caller may add to seq_start at
        // once, whatever kind of memory it lies in
        const std::vector<uint32_t> seq(seq_start, seq_start + n_streams);
        HIP_TRY(hipMemcpyAsync(d_seq, seq.data(), size_t(n_streams) * 4u, hipMemcpyHostToDevice, s));
    }

    dabk::EdiArgs a{};
    const int nst = plan->nst;
    for (int k = 0; k < nst; k++) {
        a.out[k] = d_out[plan->order[k]];
        a.offset[k] = uint16_t(plan->offset[k]);
        a.bytes[k] = uint16_t(plan->bytes[k]);
    }
    std::memcpy(a.stc, plan->header + 8, size_t(4 * nst));
    const int crc_len = packet - 2;
    a.chunk_bytes = (crc_len + 63) / 64;
    for (int lane = 0; lane < 64; lane++) a.lane_shift[lane] = uint16_t(gf_xpow(8ull * unsigned(a.chunk_bytes) * unsigned(63 - lane)));
    a.crc_init = uint16_t(gf_mul(0xFFFFu, gf_xpow(8ull * unsigned(crc_len))));
    a.fib = d_fib;
    a.crc_ok = d_crc_ok;
    a.history_in = reinterpret_cast<const dabk::EtiHistory *>(d_history_in);
    a.base = static_cast<const int32_t *>(base);
    a.seq_start = d_seq;
    a.edi = d_edi;
    a.status = reinterpret_cast<dabk::EtiStatus *>(d_status);
    a.stream_stride = stream_stride;
    a.n_streams = n_streams;
    a.frames_per_stream = frames_per_stream;
    a.nst = nst;
    a.data_bytes = plan->data_bytes;
    a.packet_bytes = packet;

    dabk::EtiAnchorArgs p{};
    p.fib = d_fib;
    p.crc_ok = d_crc_ok;
    p.history_in = a.history_in;
    p.history_out = reinterpret_cast<dabk::EtiHistory *>(d_history_out);
    p.cif_start = d_cif_start;
    p.base = static_cast<int32_t *>(base);
    p.n_streams = n_streams;
    p.frames_per_stream = frames_per_stream;

    HIP_TRY(dabk::launch_edi(p, a, s));
    return DABGPU_OK;
}

int dabgpu_edi_parse(const uint8_t *packet, size_t len, dabgpu_edi_info *info) {
    if (!packet || !info) return DABGPU_ERR_ARG;
    dabgpu_edi_info r;
    std::memset(&r, 0, sizeof r);
    r.fic_offset = -1;
    r.tsta = 0xFFFFFF;
    const auto done = [&](int code) { *info = r; return code; };
    const ed::PtrPacket g{packet};
    int total = 0;
    if (len < size_t(ed::AF_HEADER_BYTES) || !ed::header_ok(g, total) || size_t(total) != len) return done(DABGPU_EDI_BAD_HEADER);
    r.len = total - ed::AF_OVERHEAD;
    r.length = total;
    r.seq = int32_t(ed::be16(g, 6));
    r.crc = int32_t(ed::be16(g, total - 2));
    if (!ed::crc_ok(g, total)) return done(DABGPU_EDI_BAD_CRC);
    ed::Fields f;
    const int verdict = ed::parse(g, total, f);
    r.n_ptr = f.n_ptr;
    r.n_deti = f.n_deti;
    r.n_other = f.n_other;
    if (verdict == ed::BAD_TAGS) return done(DABGPU_EDI_BAD_TAGS);
    r.atstf = f.atstf;
    r.ficf = f.ficf;
    r.rfudf = f.rfudf;
    r.dlfc = f.dlfc;
    r.stat = f.stat;
    r.mid = f.mid;
    r.fp = f.fp;
    r.mnsc = f.mnsc;
    r.utco = f.utco;
    r.seconds = f.seconds;
    r.tsta = f.tsta;
    r.fic_offset = f.fic_at;
    if (verdict == ed::NOT_DETI) return done(DABGPU_EDI_NOT_DETI);
    r.nst = f.n_est;
    for (int k = 0; k < f.n_est; k++) {
        r.scid[k] = f.sstc[k][0] >> 2;
        r.sad[k] = ((f.sstc[k][0] & 3) << 8) | f.sstc[k][1];
        r.tpl[k] = f.sstc[k][2] >> 2;
        r.stl[k] = f.stl[k];
        r.offset[k] = f.data_at[k];
    }
    return done(DABGPU_OK);
}

int dabgpu_edi_streams_from_packet(const uint8_t *packet, size_t len, dabgpu_eti_stream *streams, int *n) {
    if (!packet || !streams || !n) return DABGPU_ERR_ARG;
    dabgpu_edi_info info;
    if (dabgpu_edi_parse(packet, len, &info) != DABGPU_OK) return DABGPU_ERR_ARG;
    // the est items as the STC words of an ETI(NI) frame: one mapping from TPL / STL to a sub-channel for both formats
    uint8_t frame[8 + 4 * DABGPU_ETI_MAX_STREAMS] = {};
    frame[5] = uint8_t(0x80 | info.nst);
    for (int k = 0; k < info.nst; k++) {
        uint8_t *stc = frame + 8 + 4 * k;
        stc[0] = uint8_t((info.scid[k] << 2) | (info.sad[k] >> 8));
        stc[1] = uint8_t(info.sad[k] & 0xff);
        stc[2] = uint8_t((info.tpl[k] << 2) | (info.stl[k] >> 8));
        stc[3] = uint8_t(info.stl[k] & 0xff);
    }
    return dabgpu_eti_streams_from_frame(frame, streams, n);
}

size_t dabgpu_edi_read_state_bytes(void) { return size_t(ed::STATE_BYTES); }

int dabgpu_edi_read_max_rows(int n_bytes, const dabgpu_eti_plan *plan) {
    if (n_bytes < 0 || n_bytes > EDI_READ_MAX_BYTES || (plan && !plan_stc_consistent(*plan))) return DABGPU_ERR_ARG;
    return int(ed::max_rows(uint32_t(n_bytes), plan ? plan->nst : 0, plan ? plan->data_bytes : 0));
}

int dabgpu_edi_read_dev(dabgpu_ctx *ctx, const dabgpu_edi_read_entry *entries, int n_entries, void *stream) {
    if (!ctx || n_entries > dabk::EDI_READ_MAX_ENTRIES) return DABGPU_ERR_ARG;
    // everything is checked before anything is enqueued: a refused call leaves every output as it was
    std::vector<dabk::EdiReadEntry> table(size_t(n_entries > 0 ? n_entries : 0), dabk::EdiReadEntry{});
    const int bad = edi_read_check(entries, n_entries, table.data());
    if (bad) return bad;
    if (n_entries == 0) return DABGPU_OK;
    size_t table_bytes = (table.size() * sizeof(dabk::EdiReadEntry) + 15) / 16 * 16;
    for (const dabk::EdiReadEntry &t : table) table_bytes += dabk::edi_read_scratch_bytes(t.n_bytes);
    return launch_entry_table(ctx, STAGE_EDI_READ, table_bytes, stream, [&](void *d_table, size_t, hipStream_t s) {
        return dabk::launch_edi_read(table.data(), n_entries, d_table, s);
    });
}

int dabgpu_edi_read_host(const dabgpu_edi_read_entry *entries, int n_entries) {
    const int bad = edi_read_check(entries, n_entries, nullptr);
    if (bad) return bad;
    std::vector<uint8_t> s;
    for (int i = 0; i < n_entries; i++) {
        const dabgpu_edi_read_entry &e = entries[i];
        ed::Head in{};
        if (e.d_state_in) std::memcpy(&in, e.d_state_in, sizeof in);
        const size_t tail = ed::clamp_tail(in.tail_bytes);
        s.resize(tail + size_t(e.n_bytes));
        if (tail) std::memcpy(s.data(), static_cast<const uint8_t *>(e.d_state_in) + ed::STATE_HEAD_BYTES, tail);
        if (e.n_bytes) std::memcpy(s.data() + tail, e.d_bytes, size_t(e.n_bytes));
        ed::PlanKey key{};
        uint8_t *out[DABGPU_ETI_MAX_STREAMS] = {};
        if (e.plan) {
            key = plan_key(*e.plan);
            for (int k = 0; k < key.nst; k++) out[k] = e.d_out ? e.d_out[e.plan->order[k]] : nullptr;
        }
        ed::HostOut o{};
        o.fib = e.d_fib;
        o.crc_ok = e.d_crc_ok;
        o.status = reinterpret_cast<ed::Status *>(e.d_status);
        o.result = reinterpret_cast<ed::Result *>(e.d_result);
        o.out = out;
        ed::read_entry(s.data(), s.size(), in, e.plan ? &key : nullptr, o, static_cast<uint8_t *>(e.d_state_out));
    }
    return DABGPU_OK;
}

}  // extern "C"
