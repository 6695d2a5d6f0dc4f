// dabgpu_decode_api.hip -- the channel-decoder entry points of the C ABI (include/dabgpu.h): FIC, MSC sub-channels,
// whole frames, the one-stream host call, DAB+ super-frames and following DAB+ sub-channels to them, plain Viterbi.
#include "decode_plan.hpp"

#include <algorithm>
#include <cstring>
#include <optional>

#include "../../include/dabgpu_fig.h"
#include "lane_plan.hpp"

using namespace dab;
using namespace dabapi;

namespace {

// THE lane/wave decision.  0: the wave kernels.  1: the lane kernels, if their scratch can be had -- a failed allocation
// falls back to the wave kernels silently.  2: the lane kernels or DABGPU_ERR_NOMEM -- the context forces them
// (DABGPU_FLAG_VITERBI_LANE), or a codeword is too long for the wave kernels' LDS slab (the lane kernels keep their
// survivors in HBM and take any length).  `n_codewords`: a single item's own count; the grouped call's sum.
int lane_policy(const dabgpu_ctx *ctx, long n_codewords, bool too_long) {
    if (too_long || ctx->lane_mode > 0) return 2;
    return (ctx->lane_mode < 0 && n_codewords >= LANE_MIN_CODEWORDS) ? 1 : 0;
}

dabk::LaneItem fic_item(dabgpu_ctx *ctx, const int8_t *d_soft, size_t soft_stride, int n_streams, int frames_per_stream, uint8_t *d_fib,
                        uint8_t *d_crc_ok) {
    dabk::LaneItem it{};
    it.code = ctx->fic.tables(true);
    it.tables = ctx->fic.lane_tables();
    it.args.soft = d_soft;
    it.args.soft_stride = soft_stride;
    it.args.n_streams = n_streams;
    it.args.frames_per_stream = frames_per_stream;
    it.args.out = d_fib;
    it.kind = dabk::LaneItem::FIC;
    it.crc_ok = d_crc_ok;
    return it;
}
dabk::LaneItem msc_item(const DeviceCode *dc, const dabk::MscArgs &a) {
    dabk::LaneItem it{};
    it.code = dc->tables(true);
    it.tables = dc->lane_tables();
    it.args = a;
    it.kind = dabk::LaneItem::SUBCHANNEL;
    return it;
}

// A list of items through the lane kernels (`timer`: TIMER_FIC / TIMER_MSC, or < 0 for none).  Returns 0 when everything
// was enqueued, 1 when the lane kernels do not apply (the caller falls back), < 0 on errors.
//   one item (!by_table)  goes whatever its shape: fused where lane_item_fusable says so, through the prep kernel otherwise
//                         (and always with DABGPU_FLAG_LANE_UNFUSED); `too_long` is its own length
//   several items         all or nothing: every item fusable and the context not unfused, else the caller sends them one
//                         by one; a failed allocation falls back too, so that each item applies the policy to itself; a
//                         too-long codeword among them forces nothing (too_long = false)
//   by_table              (dabgpu_decode_ensembles_dev) as several items, through the device table; no batch-size threshold:
//                         the alternative is not the wave kernels on the whole batch but one small call per stream
// The multi-item forms ask for the timer's parts (forward | traceback | history).
int decode_lane(dabgpu_ctx *ctx, const std::vector<dabk::LaneItem> &items, bool too_long, int timer, bool by_table, void *stream) {
    const int n = int(items.size());
    const bool single = n == 1 && !by_table;
    long total_cw = 0;
    for (const dabk::LaneItem &it : items) {
        if (!dabk::lane_supported(it.code.nsteps)) return 1;
        total_cw += long(it.codewords());
    }
    const int policy = lane_policy(ctx, by_table ? long(LANE_MIN_CODEWORDS) : total_cw, too_long);
    if (policy == 0) return 1;
    if (!single) {
        if (ctx->lane_unfused) return 1;
        for (const dabk::LaneItem &it : items)
            if (!dabk::lane_item_fusable(it)) return 1;
    }
    hipStream_t s = pick_stream(ctx, stream);
    int rc;
    if (!lane_scratch(ctx, dabk::lane_scratch_bytes(items.data(), n, ctx->lane_unfused), s, &rc))
        return rc ? rc : (single && policy == 2) ? DABGPU_ERR_NOMEM : 1;
    dabk::LaneScratch lsc{ctx->d_lane_scratch, ctx->lane_scratch_bytes, ctx->lane_unfused};
    if (by_table) {
        // (a table that cannot be had falls back, as scratch that cannot; a stream that cannot be waited for is an error)
        DeviceTable t;
        const int trc = stage_table(ctx, STAGE_ENSEMBLES, dabk::lane_table_bytes(items.data(), n), s, &t);
        if (trc) return trc == DABGPU_ERR_HIP ? trc : 1;
        lsc.table = t.d;
        lsc.table_bytes = t.bytes;
    }
    std::optional<ScopedTimer> tm;
    if (timer >= 0) tm.emplace(ctx, timer, s);
    bool parts = false;
    const hipError_t e = dabk::launch_lane(items.data(), n, lsc, s, (tm && !single) ? tm->mids() : nullptr, &parts);
    if (tm && parts) tm->mids_recorded();
    return e == hipSuccess ? 0 : DABGPU_ERR_HIP;
}

// one sub-channel in launches of its own (`dc`: its code tables where the caller's plan holds them, else looked up here)
int msc_decode_one(dabgpu_ctx *ctx, const dabgpu_subchannel *sc, DeviceCode *dc, const int8_t *d_soft, size_t soft_stride,
                   int n_streams, int frames_per_stream, const int8_t *d_history_in, int8_t *d_history_out,
                   uint8_t *d_out, void *stream) {
    if (!ctx || !d_soft || !d_out || n_streams < 0 || frames_per_stream < 0) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    if (d_history_in && d_history_in == d_history_out) return DABGPU_ERR_ARG;
    if (soft_stride < size_t(NB_FRAME_BITS) && size_t(n_streams) * frames_per_stream > 1) return DABGPU_ERR_ARG;
    int rc;
    if (!dc && (rc = lookup_code(ctx, sc, &dc))) return rc;
    if (n_streams == 0 || frames_per_stream == 0) return DABGPU_OK;
    const bool too_long = !dabk::viterbi_fits(dc->prof.nsteps);   // above ~800 kbit/s: only the lane kernels hold it
    if (too_long && !dabk::lane_supported(dc->prof.nsteps)) return DABGPU_ERR_CAPACITY;
    const dabk::MscArgs a = msc_args(*sc, d_soft, soft_stride, n_streams, frames_per_stream, d_history_in, d_history_out, d_out);
    if ((rc = decode_lane(ctx, {msc_item(dc, a)}, too_long, TIMER_MSC, false, stream)) <= 0) return rc;
    if (too_long) return DABGPU_ERR_CAPACITY;
    hipStream_t s = pick_stream(ctx, stream);
    ScopedTimer tm(ctx, TIMER_MSC, s);
    HIP_TRY(dabk::launch_msc_decode(dc->tables(true), a, s));
    return DABGPU_OK;
}

// The FIC (d_fib != nullptr) and/or several sub-channels in one grouped lane launch: decode_lane's answer.
int decode_parts_lane(dabgpu_ctx *ctx, uint8_t *d_fib, uint8_t *d_crc_ok, const SubchannelPlan &plan, const int8_t *d_soft,
                   size_t soft_stride, int n_streams, int frames_per_stream, const int8_t *const *d_history_in,
                   int8_t *const *d_history_out, uint8_t *const *d_out, void *stream) {
    if (plan.n + (d_fib ? 1 : 0) < 2 || !d_soft || n_streams <= 0 || frames_per_stream <= 0 || soft_stride < size_t(NB_FRAME_BITS))
        return 1;
    std::vector<dabk::LaneItem> items;
    if (d_fib) items.push_back(fic_item(ctx, d_soft, soft_stride, n_streams, frames_per_stream, d_fib, d_crc_ok));
    for (int i = 0; i < plan.n; i++) {
        items.push_back(msc_item(plan.code[size_t(i)], msc_args(plan.sc[i], d_soft, soft_stride, n_streams, frames_per_stream,
                                                                d_history_in ? d_history_in[i] : nullptr,
                                                                d_history_out ? d_history_out[i] : nullptr, d_out[i])));
        if (items.back().args.hist_in && items.back().args.hist_in == items.back().args.hist_out) return DABGPU_ERR_ARG;
    }
    return decode_lane(ctx, items, false, TIMER_MSC, false, stream);
}

// Sub-channels that do not go through the grouped lane launch.  Small batches (each sub-channel below the lane
// kernels' threshold: the plugin's one frame at a time) go through ONE launch of the wave-per-codeword kernel and one
// for the history rings; anything else is decoded sub-channel by sub-channel.
int decode_subchannels(dabgpu_ctx *ctx, const SubchannelPlan &plan, const int8_t *d_soft, size_t soft_stride, int n_streams,
                       int frames_per_stream, const int8_t *const *d_history_in, int8_t *const *d_history_out,
                       uint8_t *const *d_out, void *stream, uint8_t *d_fib = nullptr, uint8_t *d_crc_ok = nullptr) {
    const long cw_each = long(n_streams) * frames_per_stream * NB_CIFS;
    bool group = plan.n >= 1 && plan.n + (d_fib ? 1 : 0) >= 2 && lane_policy(ctx, cw_each, false) == 0 && d_soft && n_streams > 0 &&
                 frames_per_stream > 0;
    std::vector<dabk::WaveGroupItem> items;
    for (int i = 0; group && i < plan.n; i++) {
        const DeviceCode *dc = plan.code[size_t(i)];
        if (!dabk::wave_group_supported(dc->prof.nsteps)) { group = false; break; }
        dabk::WaveGroupItem it{};
        it.code = dc->tables(true);
        it.args = msc_args(plan.sc[i], d_soft, soft_stride, n_streams, frames_per_stream, d_history_in ? d_history_in[i] : nullptr,
                           d_history_out ? d_history_out[i] : nullptr, d_out[i]);
        if (it.args.hist_in && it.args.hist_in == it.args.hist_out) return DABGPU_ERR_ARG;
        items.push_back(it);
    }
    // the FIC with ONE sub-channel: together only when every codeword is resident at once (the launch then takes as long
    // as the sub-channel alone: 135 -> 101 us per call up to 256 frames); queued up in rounds, two launches are faster
    if (group && plan.n == 1 && !dabk::wave_group_one_round(std::max(items[0].code.nsteps, ctx->fic.prof.nsteps), 2 * cw_each))
        group = false;
    if (group) {
        hipStream_t s = pick_stream(ctx, stream);
        ScopedTimer tm(ctx, TIMER_MSC, s);
        // a small batch's FIC rides along: its four codewords per frame are shorter than any sub-channel's, a launch
        // of their own would only queue up in front
        dabk::WaveFicItem fic{ctx->fic.tables(true), d_soft, soft_stride, n_streams * frames_per_stream, d_fib, d_crc_ok};
        HIP_TRY(dabk::launch_msc_decode_group(items.data(), int(items.size()), s, d_fib ? &fic : nullptr));
        return DABGPU_OK;
    }
    if (d_fib) {
        const int rc = dabgpu_fic_decode_dev(ctx, d_soft, soft_stride, n_streams * frames_per_stream, d_fib, d_crc_ok, stream);
        if (rc) return rc;
    }
    for (int i = 0; i < plan.n; i++) {
        const int rc = msc_decode_one(ctx, &plan.sc[i], plan.code[size_t(i)], d_soft, soft_stride, n_streams, frames_per_stream,
                                      d_history_in ? d_history_in[i] : nullptr, d_history_out ? d_history_out[i] : nullptr,
                                      d_out[i], stream);
        if (rc) return rc;
    }
    return DABGPU_OK;
}

// dabgpu_decode_stream_frames behind its checks (any failure in here: its caller drops every ring)
int decode_stream_frames_body(dabgpu_ctx *ctx, const SubchannelPlan &plan, const int8_t *soft, size_t soft_stride, int n_frames,
                              uint8_t *fib, uint8_t *crc_ok, uint8_t *const *out, dabgpu_ber_count *fic_ber,
                              dabgpu_ber_count *const *msc_ber, dabgpu_mer *mer) {
    const dabgpu_subchannel *sc = plan.sc;
    const int n_subchannels = plan.n;
    // the quality outputs land behind the decoder's results, in the same area and the same download
    const ResultLayout lay(size_t(n_frames), plan, fic_ber != nullptr, msc_ber, mer != nullptr);
    std::vector<const int8_t *> p_hi(n_subchannels, nullptr);
    std::vector<int8_t *> p_ho(n_subchannels, nullptr);
    hipStream_t s = ctx->stream;
    for (int i = 0; i < n_subchannels; i++) {
        // the sub-channel's ring from the call before, or a new (erased) one
        const int k = ctx->sub_history.acquire(sc[i].start_address, sc[i].length, 1, s);
        if (k < 0) return k;
        p_hi[i] = ctx->sub_history.in(k);
        p_ho[i] = ctx->sub_history.out(k);
    }
    const size_t nb_soft = size_t(n_frames - 1) * soft_stride + NB_FRAME_BITS;
    void *d_soft, *d_res;
    int rc;
    if ((rc = stage(ctx, STAGE_SOFT, nb_soft, &d_soft))) return rc;
    if ((rc = stage(ctx, STAGE_RESULT, lay.total, &d_res))) return rc;
    if ((rc = ensure_bounce(ctx, lay.total))) return rc;
    if (injected_failure(ctx)) return DABGPU_ERR_HIP;            // (test hook: the caller's failure path drops every ring)
    // one upload (by a kernel when the soft bits lie in page-locked memory the device can address).  One frame with a
    // handful of sub-channels -- the plugin's call -- sends only what will be read: the FIC and the sub-channels' ranges
    // of the four CIFs (21.5 kB of the 230 kB for one 64 kbit/s service)
    // (every query first: once the upload is enqueued the host only enqueues, and stays ahead of the device)
    void *h_dev = nullptr;
    HIP_TRY(hipHostGetDevicePointer(&h_dev, ctx->h_bounce, 0));
    void *soft_alias = (nb_soft & 15) ? nullptr : device_alias_of_pinned(soft);
    if (soft_alias && !(reinterpret_cast<uintptr_t>(soft_alias) & 15)) {
        std::vector<dabk::CopyPiece> up;
        if (n_frames == 1 && !mer && 1 + NB_CIFS * n_subchannels <= dabk::copy_pieces_max()) {
            char *d = static_cast<char *>(d_soft);
            const char *h = static_cast<const char *>(soft_alias);
            up.push_back(dabk::CopyPiece{d, h, size_t(NB_FIC_BITS)});
            for (int i = 0; i < n_subchannels; i++)
                for (int c = 0; c < NB_CIFS; c++) {
                    const size_t off = size_t(NB_FIC_BITS) + size_t(c) * NB_CIF_BITS + size_t(sc[i].start_address) * CU_BITS;
                    up.push_back(dabk::CopyPiece{d + off, h + off, size_t(sc[i].length) * CU_BITS});
                }
        } else {
            up.push_back(dabk::CopyPiece{d_soft, soft_alias, nb_soft});
        }
        HIP_TRY(dabk::launch_copy_pieces(up.data(), int(up.size()), s));
    } else {
        HIP_TRY(hipMemcpyAsync(d_soft, soft, nb_soft, hipMemcpyHostToDevice, s));
    }
    // the results -- a few hundred bytes per frame -- are written by the decoder's kernels straight into the page-locked
    // landing area (no copy behind them); one synchronisation
    (void)d_res;
    char *res = static_cast<char *>(h_dev);
    std::vector<uint8_t *> p_out(n_subchannels, nullptr);
    for (int i = 0; i < n_subchannels; i++) p_out[i] = reinterpret_cast<uint8_t *>(res + lay.off_out[i]);
    rc = decode_frames_planned(ctx, plan, static_cast<const int8_t *>(d_soft), soft_stride, 1, n_frames, reinterpret_cast<uint8_t *>(res),
                               reinterpret_cast<uint8_t *>(res + lay.off_crc), p_hi.data(), p_ho.data(), p_out.data(), s);
    if (rc) return rc;
    {   // quality of the same frames from the same soft bits and rings (one more launch for the BER, one for the MER)
        std::vector<dabgpu_subchannel> q_sc;
        std::vector<const int8_t *> q_hi;
        std::vector<const uint8_t *> q_out;
        std::vector<dabgpu_ber_count *> q_ber;
        for (int i = 0; i < n_subchannels; i++)
            if (msc_ber && msc_ber[i]) {
                q_sc.push_back(sc[i]);
                q_hi.push_back(p_hi[i]);
                q_out.push_back(p_out[i]);
                q_ber.push_back(reinterpret_cast<dabgpu_ber_count *>(res + lay.off_msc_ber[i]));
            }
        if (fic_ber || !q_sc.empty()) {
            rc = dabgpu_channel_ber_dev(ctx, static_cast<const int8_t *>(d_soft), soft_stride, 1, n_frames,
                                        fic_ber ? reinterpret_cast<const uint8_t *>(res) : nullptr,
                                        reinterpret_cast<dabgpu_ber_count *>(res + lay.off_fic_ber), q_sc.data(), int(q_sc.size()),
                                        q_hi.data(), q_out.data(), q_ber.data(), s);
            if (rc) return rc;
        }
        if (mer && (rc = dabgpu_mer_dev(ctx, static_cast<const int8_t *>(d_soft), soft_stride, n_frames, 0, NB_DATA_SYMBOLS,
                                        reinterpret_cast<dabgpu_mer *>(res + lay.off_mer), s)))
            return rc;
    }
    // one synchronisation: the word behind the landing area's payload
    if ((rc = wait_for_signal(s, SignalWord(ctx, h_dev)))) return rc;
    const char *hb = static_cast<const char *>(ctx->h_bounce);
    std::memcpy(fib, hb, lay.nb_fib);
    std::memcpy(crc_ok, hb + lay.off_crc, lay.nb_crc);
    for (int i = 0; i < n_subchannels; i++) {
        std::memcpy(out[i], hb + lay.off_out[i], lay.out_bytes[i]);
        if (msc_ber && msc_ber[i]) std::memcpy(msc_ber[i], hb + lay.off_msc_ber[i], lay.nb_ber);
    }
    if (fic_ber) std::memcpy(fic_ber, hb + lay.off_fic_ber, lay.nb_ber);
    if (mer) std::memcpy(mer, hb + lay.off_mer, lay.nb_mer);
    ctx->sub_history.commit();                                  // (a sub-channel left out of this call has missed a frame)
    return DABGPU_OK;
}

}  // namespace

int dabapi::decode_frames_planned(dabgpu_ctx *ctx, const SubchannelPlan &plan, const int8_t *d_soft, size_t soft_stride, int n_streams,
                                  int frames_per_stream, uint8_t *d_fib, uint8_t *d_crc_ok, const int8_t *const *d_history_in,
                                  int8_t *const *d_history_out, uint8_t *const *d_out, void *stream) {
    const int g = decode_parts_lane(ctx, d_fib, d_crc_ok, plan, d_soft, soft_stride, n_streams, frames_per_stream, d_history_in,
                                 d_history_out, d_out, stream);
    if (g <= 0) return g;
    // (the FIC goes into the sub-channels' grouped wave launch when there is one, else it gets its own)
    return decode_subchannels(ctx, plan, d_soft, soft_stride, n_streams, frames_per_stream, d_history_in, d_history_out, d_out,
                              stream, d_fib, d_crc_ok);
}

extern "C" {

// ---------------------------------------------------------------------------- FIC
int dabgpu_fic_decode_dev(dabgpu_ctx *ctx, const int8_t *d_soft, size_t soft_stride, int n_frames,
                          uint8_t *d_fib, uint8_t *d_crc_ok, void *stream) {
    if (!ctx || !d_soft || !d_fib || !d_crc_ok || n_frames < 0) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    if (n_frames > 1 && soft_stride < size_t(NB_FIC_BITS)) return DABGPU_ERR_ARG;
    if (n_frames == 0) return DABGPU_OK;
    const int rc = decode_lane(ctx, {fic_item(ctx, d_soft, soft_stride, 1, n_frames, d_fib, d_crc_ok)}, false, TIMER_FIC, false, stream);
    if (rc <= 0) return rc;
    hipStream_t s = pick_stream(ctx, stream);
    ScopedTimer tm(ctx, TIMER_FIC, s);
    HIP_TRY(dabk::launch_fic_decode(ctx->fic.tables(true), d_soft, soft_stride, n_frames, d_fib, d_crc_ok, s));
    return DABGPU_OK;
}

int dabgpu_fic_decode(dabgpu_ctx *ctx, const int8_t *soft, size_t soft_stride, int n_frames, uint8_t *fib,
                      uint8_t *crc_ok) {
    if (!ctx || !soft || !fib || !crc_ok || n_frames < 0) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    if (n_frames == 0) return DABGPU_OK;
    HostCall h(ctx);
    void *d_soft = h.room(STAGE_SOFT, size_t(n_frames - 1) * soft_stride + NB_FIC_BITS);
    void *d_fib = h.room(STAGE_RESULT, size_t(n_frames) * NB_FIBS * 32);
    void *d_ok = h.room(STAGE_AUX, size_t(n_frames) * NB_FIBS);
    h.up(STAGE_SOFT, soft);
    if (h.rc) return h.rc;
    const int rc = dabgpu_fic_decode_dev(ctx, static_cast<const int8_t *>(d_soft), soft_stride, n_frames,
                                         static_cast<uint8_t *>(d_fib), static_cast<uint8_t *>(d_ok), ctx->stream);
    if (rc) return rc;
    h.down(STAGE_RESULT, fib);
    h.down(STAGE_AUX, crc_ok);
    return h.finish();
}

// ---------------------------------------------------------------------------- MSC
int dabgpu_soft_selection(const dabgpu_subchannel *subchannels, int n_subchannels, int with_fic,
                          dabgpu_bit_range *out, int max_out) {
    if (n_subchannels < 0 || (n_subchannels > 0 && !subchannels) || max_out < 0 || (max_out > 0 && !out)) return DABGPU_ERR_ARG;
    int n = 0;
    auto put = [&](int first, int count) {
        if (n < max_out) { out[n].first = first; out[n].count = count; }
        n++;
    };
    if (with_fic) put(0, NB_FIC_BITS);
    for (int i = 0; i < n_subchannels; i++) {
        dab::PunctureProfile prof;
        const int rc = subchannel_profile(&subchannels[i], prof);
        if (rc) return rc;
        for (int c = 0; c < NB_CIFS; c++)
            put(NB_FIC_BITS + c * NB_CIF_BITS + subchannels[i].start_address * 64, subchannels[i].length * 64);
    }
    return n;
}

int dabgpu_uep_subchannel(int table_index, int start_address, dabgpu_subchannel *out) {
    if (!out) return DABGPU_ERR_ARG;
    if (table_index < 0 || table_index >= 64) return DABGPU_ERR_PROFILE;
    const UepProfileRow &r = UEP_TABLE[table_index];
    if (start_address < 0 || start_address + r.size > 864) return DABGPU_ERR_ARG;
    out->start_address = start_address;
    out->length = r.size;
    out->is_uep = 1;
    out->eep_type = 0;
    out->protection_level = r.level;
    out->bitrate_kbps = r.bitrate;
    return DABGPU_OK;
}

int dabgpu_subchannel_bytes(const dabgpu_subchannel *sc) {
    dab::PunctureProfile prof;
    int rc = subchannel_profile(sc, prof);
    if (rc) return rc;
    return (prof.nsteps - 6) / 8;
}

int dabgpu_msc_decode_dev(dabgpu_ctx *ctx, const dabgpu_subchannel *sc, const int8_t *d_soft, size_t soft_stride,
                          int n_streams, int frames_per_stream, const int8_t *d_history_in,
                          int8_t *d_history_out, uint8_t *d_out, void *stream) {
    return msc_decode_one(ctx, sc, nullptr, d_soft, soft_stride, n_streams, frames_per_stream, d_history_in, d_history_out, d_out, stream);
}

int dabgpu_msc_decode(dabgpu_ctx *ctx, const dabgpu_subchannel *sc, const int8_t *soft, size_t soft_stride,
                      int n_streams, int frames_per_stream, const int8_t *history_in, int8_t *history_out,
                      uint8_t *out) {
    if (!ctx || !soft || !out || n_streams < 0 || frames_per_stream < 0) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    const int nbytes = dabgpu_subchannel_bytes(sc);
    if (nbytes < 0) return nbytes;
    const size_t nframes = size_t(n_streams) * frames_per_stream;
    if (nframes == 0) return DABGPU_OK;
    const size_t nb_hist = size_t(n_streams) * 15 * sc->length * CU_BITS;
    HostCall h(ctx);
    void *d_soft = h.room(STAGE_SOFT, (nframes - 1) * soft_stride + NB_FRAME_BITS);
    void *d_out = h.room(STAGE_RESULT, nframes * NB_CIFS * nbytes);
    void *d_hi = h.room(STAGE_WIDE, nb_hist, history_in != nullptr);
    void *d_ho = h.room(STAGE_HISTORY_OUT, nb_hist, history_out != nullptr);
    h.up(STAGE_SOFT, soft);
    h.up(STAGE_WIDE, history_in);
    if (h.rc) return h.rc;
    const int rc = dabgpu_msc_decode_dev(ctx, sc, static_cast<const int8_t *>(d_soft), soft_stride, n_streams,
                                         frames_per_stream, static_cast<const int8_t *>(d_hi), static_cast<int8_t *>(d_ho),
                                         static_cast<uint8_t *>(d_out), ctx->stream);
    if (rc) return rc;
    h.down(STAGE_RESULT, out);
    h.down(STAGE_HISTORY_OUT, history_out);
    return h.finish();
}

int dabgpu_msc_decode_multi_dev(dabgpu_ctx *ctx, const dabgpu_subchannel *sc, int n_subchannels,
                                const int8_t *d_soft, size_t soft_stride, int n_streams, int frames_per_stream,
                                const int8_t *const *d_history_in, int8_t *const *d_history_out,
                                uint8_t *const *d_out, void *stream) {
    if (!ctx || !sc || !d_out || n_subchannels < 0) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    // validate everything before enqueueing anything: profiles, bounds, no overlap inside the CIF
    const SubchannelPlan plan(ctx, sc, n_subchannels, d_out);
    if (plan.rc) return plan.rc;
    const int g = decode_parts_lane(ctx, nullptr, nullptr, plan, d_soft, soft_stride, n_streams, frames_per_stream, d_history_in,
                                 d_history_out, d_out, stream);
    if (g <= 0) return g;                                      // done (0) or a real error (< 0); 1 = not applicable
    return decode_subchannels(ctx, plan, d_soft, soft_stride, n_streams, frames_per_stream, d_history_in, d_history_out, d_out,
                              stream);
}

int dabgpu_decode_frames_dev(dabgpu_ctx *ctx, const int8_t *d_soft, size_t soft_stride, int n_streams,
                             int frames_per_stream, uint8_t *d_fib, uint8_t *d_crc_ok, const dabgpu_subchannel *sc,
                             int n_subchannels, const int8_t *const *d_history_in, int8_t *const *d_history_out,
                             uint8_t *const *d_out, void *stream) {
    if (!ctx || !d_soft || !d_fib || !d_crc_ok || n_streams < 0 || frames_per_stream < 0 || n_subchannels < 0) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    if (n_subchannels > 0 && (!sc || !d_out)) return DABGPU_ERR_ARG;
    if (soft_stride < size_t(NB_FRAME_BITS) && size_t(n_streams) * frames_per_stream > 1) return DABGPU_ERR_ARG;
    const SubchannelPlan plan(ctx, sc, n_subchannels, d_out);
    if (plan.rc) return plan.rc;
    if (n_streams == 0 || frames_per_stream == 0) return DABGPU_OK;
    return decode_frames_planned(ctx, plan, d_soft, soft_stride, n_streams, frames_per_stream, d_fib, d_crc_ok, d_history_in,
                                 d_history_out, d_out, stream);
}

int dabgpu_decode_ensembles_dev(dabgpu_ctx *ctx, const int8_t *d_soft, size_t soft_stride, int n_streams, int frames_per_stream,
                                uint8_t *d_fib, uint8_t *d_crc_ok, const dabgpu_subchannel *sc, const int32_t *sc_first,
                                const int8_t *const *d_history_in, int8_t *const *d_history_out, uint8_t *const *d_out,
                                void *stream) {
    if (!ctx || !d_soft || !sc_first || n_streams < 0 || frames_per_stream < 0 || (d_fib == nullptr) != (d_crc_ok == nullptr))
        return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    if (soft_stride < size_t(NB_FRAME_BITS) && size_t(n_streams) * frames_per_stream > 1) return DABGPU_ERR_ARG;
    // everything is checked before anything is enqueued: a refused call leaves every output as it was
    const EnsemblePlan plan(ctx, sc, sc_first, n_streams, d_out);
    if (plan.rc) return plan.rc;
    for (int i = 0; i < plan.total; i++)
        if (d_history_in && d_history_out && d_history_in[i] && d_history_in[i] == d_history_out[i]) return DABGPU_ERR_ARG;
    if (n_streams == 0 || frames_per_stream == 0) return DABGPU_OK;
    // Everything in one launch through the device table when every stream is whole 64-codeword groups (the other conditions:
    // decode_lane)
    if (frames_per_stream % 16 == 0 && soft_stride >= size_t(NB_FRAME_BITS)) {
        std::vector<dabk::LaneItem> items;
        items.reserve(size_t(plan.total) + 1);
        if (d_fib) items.push_back(fic_item(ctx, d_soft, soft_stride, n_streams, frames_per_stream, d_fib, d_crc_ok));
        for (int s = 0; s < n_streams; s++)
            for (int i = sc_first[s]; i < sc_first[s + 1]; i++)
                items.push_back(msc_item(plan.code[size_t(i)],
                                         msc_args(sc[i], d_soft + size_t(s) * frames_per_stream * soft_stride, soft_stride, 1, frames_per_stream,
                                                  d_history_in ? d_history_in[i] : nullptr, d_history_out ? d_history_out[i] : nullptr, d_out[i])));
        if (items.empty()) return DABGPU_OK;
        const int g = decode_lane(ctx, items, false, TIMER_MSC, true, stream);
        if (g <= 0) return g;
    }
    // any other shape: the same bytes part by part, stream by stream
    for (int s = 0; s < n_streams; s++) {
        const int i0 = sc_first[s], n = plan.count(s);
        const int8_t *soft_s = d_soft + size_t(s) * frames_per_stream * soft_stride;
        const SubchannelPlan sub(ctx, sc + i0, n, d_out + i0);
        if (sub.rc) return sub.rc;
        const int8_t *const *hi = d_history_in ? d_history_in + i0 : nullptr;
        int8_t *const *ho = d_history_out ? d_history_out + i0 : nullptr;
        int rc;
        if (d_fib) {
            rc = decode_frames_planned(ctx, sub, soft_s, soft_stride, 1, frames_per_stream,
                                       d_fib + size_t(s) * frames_per_stream * NB_FIBS * 32,
                                       d_crc_ok + size_t(s) * frames_per_stream * NB_FIBS, hi, ho, d_out + i0, stream);
        } else {
            rc = decode_parts_lane(ctx, nullptr, nullptr, sub, soft_s, soft_stride, 1, frames_per_stream, hi, ho, d_out + i0, stream);
            if (rc > 0) rc = decode_subchannels(ctx, sub, soft_s, soft_stride, 1, frames_per_stream, hi, ho, d_out + i0, stream);
        }
        if (rc) return rc;
    }
    return DABGPU_OK;
}

int dabgpu_fig_subchannels(const uint8_t *fib, const uint8_t *crc_ok, int n_frames, dabgpu_subchannel *out, int max, int *n) {
    if (!fib || !crc_ok || !n || n_frames < 0 || max < 0 || (max > 0 && !out)) return DABGPU_ERR_ARG;
    // the walk: include/dabgpu_fig.h; the profile an entry names: here, where the puncture tables are
    return dabgpu_fig::subchannels(fib, crc_ok, n_frames, [](const dabgpu_fig::Organisation &e, dabgpu_subchannel &sc) {
        if (!e.long_form) return e.table_switch ? int(DABGPU_ERR_PROFILE) : dabgpu_uep_subchannel(e.index, e.start, &sc);
        // the bit rate the size implies: n times the level's capacity units, 8 n (A) or 32 n (B) kbit/s
        static const int CU_A[4] = {12, 8, 6, 4}, CU_B[4] = {27, 21, 18, 15};
        const int unit = e.option ? CU_B[e.level - 1] : CU_A[e.level - 1];
        if (e.size == 0 || e.size % unit) return int(DABGPU_ERR_PROFILE);
        sc = dabgpu_subchannel{e.start, e.size, 0, e.option, e.level, (e.option ? 32 : 8) * (e.size / unit)};
        dab::PunctureProfile prof;
        return subchannel_profile(&sc, prof);
    }, out, max, n);
}

int dabgpu_fig_audio_components(const uint8_t *fib, const uint8_t *crc_ok, int n_frames, dabgpu_audio_component *out, int max,
                                int *n) {
    if (!fib || !crc_ok || !n || n_frames < 0 || max < 0 || (max > 0 && !out)) return DABGPU_ERR_ARG;
    return dabgpu_fig::audio_components(fib, crc_ok, n_frames, out, max, n);
}

int dabgpu_decode_frames(dabgpu_ctx *ctx, const int8_t *soft, size_t soft_stride, int n_streams, int frames_per_stream,
                         uint8_t *fib, uint8_t *crc_ok, const dabgpu_subchannel *sc, int n_subchannels,
                         const int8_t *const *history_in, int8_t *const *history_out, uint8_t *const *out) {
    if (!ctx || !soft || !fib || !crc_ok || n_streams < 0 || frames_per_stream < 0 || n_subchannels < 0) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    if (n_subchannels > 0 && (!sc || !out)) return DABGPU_ERR_ARG;
    const size_t nframes = size_t(n_streams) * frames_per_stream;
    if (nframes == 0) return DABGPU_OK;
    if (soft_stride < size_t(NB_FRAME_BITS) && nframes > 1) return DABGPU_ERR_ARG;
    const SubchannelPlan plan(ctx, sc, n_subchannels, out);
    if (plan.rc) return plan.rc;
    // the result staging buffer: ResultLayout; the history staging buffers: [hist_0 | hist_1 ...]
    const ResultLayout lay(nframes, plan);
    std::vector<size_t> hist_off(n_subchannels), hist_bytes(n_subchannels);
    size_t hist_total = 0;
    for (int i = 0; i < n_subchannels; i++) {
        hist_off[i] = hist_total;
        hist_bytes[i] = size_t(n_streams) * 15 * sc[i].length * CU_BITS;
        hist_total += ResultLayout::al(hist_bytes[i]);
    }
    HostCall h(ctx);
    void *d_soft = h.room(STAGE_SOFT, (nframes - 1) * soft_stride + NB_FRAME_BITS);
    void *d_res = h.room(STAGE_RESULT, lay.total);
    void *d_hi = h.room(STAGE_WIDE, hist_total, hist_total && history_in);
    void *d_ho = h.room(STAGE_HISTORY_OUT, hist_total, hist_total && history_out);
    h.up(STAGE_SOFT, soft);                                                            // the frames go up once
    if (h.rc) return h.rc;
    hipStream_t s = ctx->stream;
    std::vector<const int8_t *> p_hi(n_subchannels, nullptr);
    std::vector<int8_t *> p_ho(n_subchannels, nullptr);
    std::vector<uint8_t *> p_out(n_subchannels, nullptr);
    uint8_t *res = static_cast<uint8_t *>(d_res);
    for (int i = 0; i < n_subchannels; i++) {
        p_out[i] = res + lay.off_out[i];
        if (history_in && history_in[i]) {
            p_hi[i] = reinterpret_cast<const int8_t *>(static_cast<char *>(d_hi) + hist_off[i]);
            HIP_TRY(hipMemcpyAsync(const_cast<int8_t *>(p_hi[i]), history_in[i], hist_bytes[i], hipMemcpyHostToDevice, s));
        }
        if (history_out && history_out[i]) p_ho[i] = reinterpret_cast<int8_t *>(static_cast<char *>(d_ho) + hist_off[i]);
    }
    const int rc = decode_frames_planned(ctx, plan, static_cast<const int8_t *>(d_soft), soft_stride, n_streams, frames_per_stream,
                                         res, res + lay.off_crc, p_hi.data(), p_ho.data(), p_out.data(), s);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(fib, res, lay.nb_fib, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(crc_ok, res + lay.off_crc, lay.nb_crc, hipMemcpyDeviceToHost, s));
    for (int i = 0; i < n_subchannels; i++) {
        HIP_TRY(hipMemcpyAsync(out[i], p_out[i], lay.out_bytes[i], hipMemcpyDeviceToHost, s));
        if (p_ho[i]) HIP_TRY(hipMemcpyAsync(history_out[i], p_ho[i], hist_bytes[i], hipMemcpyDeviceToHost, s));
    }
    return h.finish();                                                                 // one synchronisation
}

int dabgpu_decode_stream_reset(dabgpu_ctx *ctx) {
    if (!ctx) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->sub_history.clear();
    return DABGPU_OK;
}

int dabgpu_decode_stream_frames(dabgpu_ctx *ctx, const int8_t *soft, size_t soft_stride, int n_frames, uint8_t *fib,
                                uint8_t *crc_ok, const dabgpu_subchannel *sc, int n_subchannels, uint8_t *const *out) {
    return dabgpu_decode_stream_frames_quality(ctx, soft, soft_stride, n_frames, fib, crc_ok, sc, n_subchannels, out, nullptr,
                                               nullptr, nullptr);
}

int dabgpu_decode_stream_frames_quality(dabgpu_ctx *ctx, const int8_t *soft, size_t soft_stride, int n_frames, uint8_t *fib,
                                        uint8_t *crc_ok, const dabgpu_subchannel *sc, int n_subchannels, uint8_t *const *out,
                                        dabgpu_ber_count *fic_ber, dabgpu_ber_count *const *msc_ber, dabgpu_mer *mer) {
    if (!ctx || !soft || !fib || !crc_ok || n_frames < 0 || n_subchannels < 0) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    if (n_subchannels > 0 && (!sc || !out)) return DABGPU_ERR_ARG;
    if (n_frames == 0) return DABGPU_OK;
    if (soft_stride < size_t(NB_FRAME_BITS) && n_frames > 1) return DABGPU_ERR_ARG;
    // argument errors are refused before any ring is touched: the kept state survives them
    const SubchannelPlan plan(ctx, sc, n_subchannels, out);
    if (plan.rc) return plan.rc;
    if (mer && n_frames > 1 && (soft_stride & 15)) return DABGPU_ERR_ARG;          // (the MER kernel's 16-byte loads)
    const int rc = decode_stream_frames_body(ctx, plan, soft, soft_stride, n_frames, fib, crc_ok, out, fic_ber, msc_ber, mer);
    if (rc != DABGPU_OK) {
        // A call that failed part-way leaves rings that have missed this frame (and `live` marks on some of them): no
        // ring continues the stream any more.  All of them go; the next call starts every sub-channel from erasures.
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipGetLastError();
        ctx->sub_history.clear();
    }
    return rc;
}

// ---------------------------------------------------------------------------- DAB+ super-frame
static_assert(sizeof(dabgpu_superframe_status) == sizeof(dabk::SuperframeStatus), "ABI struct mirrors the kernel's");

int dabgpu_dabplus_superframes_dev(dabgpu_ctx *ctx, const uint8_t *d_in, size_t in_stride, int n_superframes,
                                   int bitrate_kbps, uint8_t *d_out, dabgpu_superframe_status *d_status,
                                   void *stream) {
    if (!ctx || !d_in || !d_out || !d_status || n_superframes < 0) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    if (bitrate_kbps < 8 || bitrate_kbps % 8 || bitrate_kbps > 512) return DABGPU_ERR_PROFILE;
    const int s = bitrate_kbps / 8;
    if (n_superframes > 1 && in_stride < size_t(120) * s) return DABGPU_ERR_ARG;
    if (n_superframes == 0) return DABGPU_OK;
    HIP_TRY(dabk::launch_dabplus_superframes(d_in, in_stride, n_superframes, s, d_out,
                                             reinterpret_cast<dabk::SuperframeStatus *>(d_status),
                                             pick_stream(ctx, stream)));
    return DABGPU_OK;
}

int dabgpu_dabplus_superframes(dabgpu_ctx *ctx, const uint8_t *in, size_t in_stride, int n_superframes,
                               int bitrate_kbps, uint8_t *out, dabgpu_superframe_status *status) {
    if (!ctx || !in || !out || !status || n_superframes < 0) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    if (bitrate_kbps < 8 || bitrate_kbps % 8 || bitrate_kbps > 512) return DABGPU_ERR_PROFILE;
    const int s = bitrate_kbps / 8;
    if (n_superframes > 1 && in_stride < size_t(120) * s) return DABGPU_ERR_ARG;   // (before any byte of `in` is read)
    if (n_superframes == 0) return DABGPU_OK;
    const size_t nb_in = size_t(n_superframes - 1) * in_stride + size_t(120) * s;
    const size_t nb_out = size_t(n_superframes) * 110 * s;
    // A few super-frames in page-locked buffers (the host mirror's channels hand over ONE, ~1-2 kB in, ~1 kB out): the kernel
    // reads and writes the caller's buffers themselves -- one launch and the watched word instead of three copy-engine
    // transfers and a sleep (~60 -> ~15 us per call; three DAB+ services make 2.4 such calls per frame).
    if (n_superframes <= 8) {
        void *a_in = device_alias_of_pinned(in), *a_out = device_alias_of_pinned(out), *a_st = device_alias_of_pinned(status);
        if (a_in && a_out && a_st && !(reinterpret_cast<uintptr_t>(a_st) & 7)) {
            const int brc = ensure_bounce(ctx, 0);
            if (brc) return brc;
            // the kernel writes the caller's buffers: the word is watched only when they are known to be coherent
            const bool coherent = known_coherent_host(out, nb_out) && known_coherent_host(status, sizeof(dabgpu_superframe_status) * size_t(n_superframes));
            void *h_dev = nullptr;
            HIP_TRY(hipHostGetDevicePointer(&h_dev, ctx->h_bounce, 0));
            hipStream_t st = ctx->stream;
            const SignalWord w(ctx, h_dev);
            if (n_superframes == 1) {
                // ONE super-frame (the host mirror's call) is ONE workgroup: it stores the watched word itself, behind its results
                HIP_TRY(dabk::launch_dabplus_superframes(static_cast<const uint8_t *>(a_in), in_stride, 1, s, static_cast<uint8_t *>(a_out),
                                                         reinterpret_cast<dabk::SuperframeStatus *>(a_st), st, w.dev, w.seq));
                return wait_for_signal(st, w, true, coherent);
            }
            const int rc0 = dabgpu_dabplus_superframes_dev(ctx, static_cast<const uint8_t *>(a_in), in_stride, n_superframes, bitrate_kbps,
                                                           static_cast<uint8_t *>(a_out), static_cast<dabgpu_superframe_status *>(a_st), st);
            if (rc0) return rc0;
            return wait_for_signal(st, w, false, coherent);
        }
    }
    HostCall h(ctx);
    void *d_in = h.room(STAGE_SOFT, nb_in);
    void *d_out = h.room(STAGE_RESULT, nb_out);
    void *d_st = h.room(STAGE_AUX, sizeof(dabgpu_superframe_status) * n_superframes);
    h.up(STAGE_SOFT, in);
    if (h.rc) return h.rc;
    const int rc = dabgpu_dabplus_superframes_dev(ctx, static_cast<const uint8_t *>(d_in), in_stride, n_superframes,
                                                  bitrate_kbps, static_cast<uint8_t *>(d_out),
                                                  static_cast<dabgpu_superframe_status *>(d_st), ctx->stream);
    if (rc) return rc;
    h.down(STAGE_RESULT, out);
    h.down(STAGE_AUX, status);
    return h.finish();
}

// ---------------------------------------------------------------------------- DAB+: following sub-channels
static_assert(sizeof(dabgpu_dabplus_follow_result) == sizeof(dabk::FollowResult), "ABI struct mirrors the kernel's");

static bool follow_bitrate_ok(int bitrate_kbps) { return bitrate_kbps >= 8 && bitrate_kbps <= 512 && bitrate_kbps % 8 == 0; }

size_t dabgpu_dabplus_carry_bytes(int bitrate_kbps) {
    return follow_bitrate_ok(bitrate_kbps) ? dabk::follow_carry_bytes(bitrate_kbps / 8) : 0;
}

int dabgpu_dabplus_follow_dev(dabgpu_ctx *ctx, const dabgpu_dabplus_entry *entries, int n_entries, int n_cifs, void *stream) {
    if (!ctx || n_entries < 0 || n_cifs < 0 || (n_entries > 0 && !entries)) return DABGPU_ERR_ARG;
    // everything is checked before anything is enqueued: a refused call leaves every output as it was
    const int max_sf = (n_cifs + 4) / 5;
    std::vector<dabk::FollowEntry> table(size_t(n_entries), dabk::FollowEntry{});
    for (int i = 0; i < n_entries; i++) {
        const dabgpu_dabplus_entry &e = entries[i];
        if (!follow_bitrate_ok(e.bitrate_kbps)) return DABGPU_ERR_ARG;
        const int s = e.bitrate_kbps / 8;
        if (n_cifs > 0 && !e.d_in) return DABGPU_ERR_ARG;
        if (n_cifs > 1 && e.in_stride < size_t(24) * s) return DABGPU_ERR_ARG;
        if (max_sf > 0 && (!e.d_data || !e.d_status)) return DABGPU_ERR_ARG;
        if (!e.d_carry_out || !e.d_result) return DABGPU_ERR_ARG;
        if ((addr(e.d_carry_in) | addr(e.d_carry_out)) & 15) return DABGPU_ERR_ARG;
        if ((addr(e.d_status) | addr(e.d_result)) & 3) return DABGPU_ERR_ARG;
        const uint64_t cb = dabk::follow_carry_bytes(s);
        if (e.d_carry_in && overlaps(e.d_carry_in, cb, e.d_carry_out, cb)) return DABGPU_ERR_ARG;
        dabk::FollowEntry &t = table[size_t(i)];
        t.in = addr(e.d_in);
        t.carry_in = addr(e.d_carry_in);
        t.carry_out = addr(e.d_carry_out);
        t.data = addr(e.d_data);
        t.status = addr(e.d_status);
        t.result = addr(e.d_result);
        t.in_stride = e.in_stride;
        t.s = s;
    }
    if (n_entries == 0) return DABGPU_OK;
    const size_t table_bytes = dabk::follow_table_bytes(n_entries);
    return launch_entry_table(ctx, STAGE_DABPLUS, table_bytes, stream, [&](void *d_table, size_t slot_bytes, hipStream_t s) {
        return dabk::launch_dabplus_follow(table.data(), n_entries, n_cifs, d_table, slot_bytes, s);
    });
}

// ---------------------------------------------------------------------------- plain Viterbi
int dabgpu_viterbi_dev(dabgpu_ctx *ctx, const int8_t *d_punct, int n_codewords, const uint8_t *mask, int nsteps,
                       uint8_t *d_out_bytes, void *stream) {
    if (!ctx || !d_punct || !mask || !d_out_bytes || n_codewords < 0) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    if (nsteps < 14 || ((nsteps - 6) & 7)) return DABGPU_ERR_ARG;
    const bool too_long = !dabk::viterbi_fits(nsteps);
    if (too_long && !dabk::lane_supported(nsteps)) return DABGPU_ERR_CAPACITY;
    dab::PunctureProfile prof;
    prof.mask.assign(mask, mask + 4 * size_t(nsteps));
    for (uint8_t &f : prof.mask) f = f ? 1 : 0;
    finish_profile(prof);
    if (n_codewords == 0) return DABGPU_OK;
    DeviceCode *dc = nullptr;
    int rc = get_code(ctx, std::move(prof), &dc);
    if (rc) return rc;
    dabk::LaneItem it{};
    it.code = dc->tables(false);
    it.tables = dc->lane_tables();
    it.args.soft = d_punct;
    it.args.out = d_out_bytes;
    it.kind = dabk::LaneItem::PLAIN;
    it.n_plain = n_codewords;
    if ((rc = decode_lane(ctx, {it}, too_long, -1, false, stream)) <= 0) return rc;
    if (too_long) return DABGPU_ERR_CAPACITY;
    HIP_TRY(dabk::launch_viterbi_plain(dc->tables(false), d_punct, n_codewords, d_out_bytes, pick_stream(ctx, stream)));
    return DABGPU_OK;
}

int dabgpu_viterbi(dabgpu_ctx *ctx, const int8_t *punct, int n_codewords, const uint8_t *mask, int nsteps,
                   uint8_t *out_bytes) {
    if (!ctx || !punct || !mask || !out_bytes || n_codewords < 0) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    if (nsteps < 14 || ((nsteps - 6) & 7)) return DABGPU_ERR_ARG;
    if (n_codewords == 0) return DABGPU_OK;
    size_t n_punct = 0;
    for (int i = 0; i < 4 * nsteps; i++) n_punct += mask[i] ? 1 : 0;
    const size_t nb_in = size_t(n_codewords) * n_punct;
    HostCall h(ctx);
    void *d_in = h.room(STAGE_SOFT, nb_in ? nb_in : 1);
    void *d_out = h.room(STAGE_RESULT, size_t(n_codewords) * ((nsteps - 6) / 8));
    if (nb_in) h.up(STAGE_SOFT, punct);                        // (a mask that keeps nothing: no byte of `punct` is read)
    if (h.rc) return h.rc;
    const int rc = dabgpu_viterbi_dev(ctx, static_cast<const int8_t *>(d_in), n_codewords, mask, nsteps,
                                      static_cast<uint8_t *>(d_out), ctx->stream);
    if (rc) return rc;
    h.down(STAGE_RESULT, out_bytes);
    return h.finish();
}

}  // extern "C"