// dabgpu_measure_api.hip -- the measurement entry points of the C ABI (include/dabgpu.h): transmitter identification (TII)
// from the null symbol, channel impulse response (CIR) from the phase reference symbol; their host-side decoders;
// reception quality (MER, pre-Viterbi channel BER) from what the front end and the decoder left on the device.
#include "decode_plan.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

using namespace dab;
using namespace dabapi;

static_assert(sizeof(dabgpu_tii_acc) == sizeof(dabk::TiiRecord), "ABI struct mirrors the kernel's");
static_assert(offsetof(dabgpu_tii_acc, floor) == offsetof(dabk::TiiRecord, floor) &&
              offsetof(dabgpu_tii_acc, frames) == offsetof(dabk::TiiRecord, frames), "ABI struct mirrors the kernel's");
static_assert(sizeof(dabgpu_cir_acc) == sizeof(dabk::CirRecord), "ABI struct mirrors the kernel's");
static_assert(offsetof(dabgpu_cir_acc, carrier) == offsetof(dabk::CirRecord, carrier) &&
              offsetof(dabgpu_cir_acc, frames) == offsetof(dabk::CirRecord, frames), "ABI struct mirrors the kernel's");

namespace {
// both calls: checks, the per-frame records (the caller's or STAGE_TII), the launches
int tii_launch(dabgpu_ctx *ctx, dabk::TiiArgs &a, dabgpu_tii_acc *d_frame, dabgpu_tii_acc *d_acc, void *stream) {
    if ((reinterpret_cast<uintptr_t>(d_acc) & 3u) || (reinterpret_cast<uintptr_t>(d_frame) & 3u)) return DABGPU_ERR_ARG;
    const size_t n_frames = size_t(a.n_streams) * size_t(a.frames_per_stream);
    if (n_frames > size_t(0x7fffffff)) return DABGPU_ERR_ARG;
    if (n_frames == 0) return DABGPU_OK;
    int rc;
    void *rec = d_frame;
    if (!rec && (rc = stage(ctx, STAGE_TII, n_frames * sizeof(dabk::TiiRecord), &rec))) return rc;
    a.frame = static_cast<dabk::TiiRecord *>(rec);
    a.acc = reinterpret_cast<dabk::TiiRecord *>(d_acc);
    hipStream_t s = pick_stream(ctx, stream);
    HIP_TRY(dabk::launch_tii(ctx->d_twiddle, a, s, ctx->iq_format));
    return a.state ? note_state_use(ctx, s) : DABGPU_OK;
}

// both calls: checks, the per-frame records (the caller's or STAGE_CIR), the launches
int cir_launch(dabgpu_ctx *ctx, dabk::CirArgs &a, dabgpu_cir_acc *d_frame, dabgpu_cir_acc *d_acc, void *stream) {
    if ((reinterpret_cast<uintptr_t>(d_acc) & 3u) || (reinterpret_cast<uintptr_t>(d_frame) & 3u)) return DABGPU_ERR_ARG;
    const size_t n_frames = size_t(a.n_streams) * size_t(a.frames_per_stream);
    if (n_frames > size_t(0x7fffffff)) return DABGPU_ERR_ARG;
    if (n_frames == 0) return DABGPU_OK;
    int rc;
    void *rec = d_frame;
    if (!rec && (rc = stage(ctx, STAGE_CIR, n_frames * sizeof(dabk::CirRecord), &rec))) return rc;
    a.frame = static_cast<dabk::CirRecord *>(rec);
    a.acc = reinterpret_cast<dabk::CirRecord *>(d_acc);
    a.prs_qt = ctx->d_prs_qt;
    hipStream_t s = pick_stream(ctx, stream);
    HIP_TRY(dabk::launch_cir(ctx->d_twiddle, a, s, ctx->iq_format));
    return a.state ? note_state_use(ctx, s) : DABGPU_OK;
}
}  // namespace

extern "C" {

// ---------------------------------------------------------------------------- transmitter identification
void dabgpu_tii_default_cfg(dabgpu_tii_cfg *cfg) {
    if (!cfg) return;
    cfg->min_level_db = 3.0f;
    cfg->reserved = 0;
}

int dabgpu_tii_pattern(int p) { return p >= 0 && p < dabk::TII_PATTERNS ? dabk::tii_pattern_mask(p) : -1; }

int dabgpu_tii_frames_dev(dabgpu_ctx *ctx, const void *d_iq, size_t frame_stride, int n_streams, int frames_per_stream,
                          const float *d_freq_offset, dabgpu_tii_acc *d_frame, dabgpu_tii_acc *d_acc, void *stream) {
    if (!ctx || !d_iq || !d_acc || n_streams < 0 || frames_per_stream < 0 || iq_misaligned(ctx, d_iq)) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    if (size_t(n_streams) * size_t(frames_per_stream) > 1 && frame_stride < size_t(NB_NULL_PERIOD)) return DABGPU_ERR_ARG;
    if (!d_freq_offset && n_streams > 0 && frames_per_stream > 0) {
        if (!ctx->d_states) return DABGPU_ERR_ARG;                 // dabgpu_streams_reset first
        if (n_streams > ctx->n_states) return DABGPU_ERR_CAPACITY;
    }
    dabk::TiiArgs a{};
    a.iq = static_cast<const float2 *>(d_iq);
    a.stride = frame_stride;
    a.n_streams = n_streams;
    a.frames_per_stream = frames_per_stream;
    a.freq_offset = d_freq_offset;
    a.state = d_freq_offset ? nullptr : ctx->d_states;
    return tii_launch(ctx, a, d_frame, d_acc, stream);
}

int dabgpu_tii_acquired_dev(dabgpu_ctx *ctx, const void *d_iq, size_t stream_stride, int n_streams, int max_frames,
                            const dabgpu_acquired_frame *d_frames, int timing_margin, dabgpu_tii_acc *d_frame,
                            dabgpu_tii_acc *d_acc, void *stream) {
    if (!ctx || !d_iq || !d_frames || !d_acc || n_streams < 0 || max_frames <= 0 || iq_misaligned(ctx, d_iq)) return DABGPU_ERR_ARG;
    if (timing_margin < 0 || timing_margin > NB_CP || (reinterpret_cast<uintptr_t>(d_frames) & 7u)) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    dabk::TiiArgs a{};
    a.iq = static_cast<const float2 *>(d_iq);
    a.stride = stream_stride;
    a.n_streams = n_streams;
    a.frames_per_stream = max_frames;
    a.acq = reinterpret_cast<const dabk::AcquiredFrame *>(d_frames);
    a.timing_margin = timing_margin;
    return tii_launch(ctx, a, d_frame, d_acc, stream);
}

int dabgpu_tii_decode(const dabgpu_tii_acc *acc, const dabgpu_tii_cfg *cfg, dabgpu_tii_entry *out, int max_out) {
    dabgpu_tii_cfg def;
    dabgpu_tii_default_cfg(&def);
    if (!cfg) cfg = &def;
    if (!acc || max_out < 0 || (max_out > 0 && !out) || !std::isfinite(cfg->min_level_db)) return DABGPU_ERR_ARG;
    if (acc->frames == 0 || !(acc->floor > 0.0f)) return 0;
    const double thr = std::pow(10.0, double(cfg->min_level_db) / 10.0);
    const double noise = 8.0 * double(acc->floor);
    std::vector<dabgpu_tii_entry> found;
    for (int c = 0; c < dabk::TII_COMBS; c++) {
        double level[dabk::TII_POSITIONS];
        int on = 0, n_on = 0;
        for (int b = 0; b < dabk::TII_POSITIONS; b++) {
            level[b] = double(acc->cell[c][b]) / noise - 1.0;
            if (level[b] >= thr) {
                on |= 0x80 >> b;
                n_on++;
            }
        }
        for (int p = 0; p < dabk::TII_PATTERNS; p++) {
            const int m = dabk::tii_pattern_mask(p);
            if ((on & m) != m) continue;
            double sum = 0.0;
            for (int b = 0; b < dabk::TII_POSITIONS; b++)
                if (m & (0x80 >> b)) sum += level[b];
            found.push_back(dabgpu_tii_entry{p, c, float(10.0 * std::log10(sum / 4.0)), n_on > 4 ? DABGPU_TII_AMBIGUOUS : 0});
        }
    }
    std::stable_sort(found.begin(), found.end(), [](const dabgpu_tii_entry &x, const dabgpu_tii_entry &y) {
        return x.level_db > y.level_db;                             // (found in sub_id, main_id order: ties keep it)
    });
    for (size_t i = 0; i < found.size() && i < size_t(max_out); i++) out[i] = found[i];
    return int(found.size());
}

// ---------------------------------------------------------------------------- channel impulse response
void dabgpu_cir_default_cfg(dabgpu_cir_cfg *cfg) {
    if (!cfg) return;
    cfg->min_snr_db = 10.0f;
    cfg->range_db = 25.0f;
}

int dabgpu_cir_frames_dev(dabgpu_ctx *ctx, const void *d_iq, size_t frame_stride, int n_streams, int frames_per_stream,
                          const float *d_freq_offset, dabgpu_cir_acc *d_frame, dabgpu_cir_acc *d_acc, void *stream) {
    if (!ctx || !d_iq || !d_acc || n_streams < 0 || frames_per_stream < 0 || iq_misaligned(ctx, d_iq)) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    if (size_t(n_streams) * size_t(frames_per_stream) > 1 && (frame_stride < size_t(NB_SYM_PERIOD) || (frame_stride & 1u)))
        return DABGPU_ERR_ARG;
    if (!d_freq_offset && n_streams > 0 && frames_per_stream > 0) {
        if (!ctx->d_states) return DABGPU_ERR_ARG;                 // dabgpu_streams_reset first
        if (n_streams > ctx->n_states) return DABGPU_ERR_CAPACITY;
    }
    dabk::CirArgs a{};
    a.iq = static_cast<const float2 *>(d_iq);
    a.stride = frame_stride;
    a.n_streams = n_streams;
    a.frames_per_stream = frames_per_stream;
    a.freq_offset = d_freq_offset;
    a.state = d_freq_offset ? nullptr : ctx->d_states;
    return cir_launch(ctx, a, d_frame, d_acc, stream);
}

int dabgpu_cir_acquired_dev(dabgpu_ctx *ctx, const void *d_iq, size_t stream_stride, int n_streams, int max_frames,
                            const dabgpu_acquired_frame *d_frames, int timing_margin, dabgpu_cir_acc *d_frame,
                            dabgpu_cir_acc *d_acc, void *stream) {
    if (!ctx || !d_iq || !d_frames || !d_acc || n_streams < 0 || max_frames <= 0 || iq_misaligned(ctx, d_iq)) return DABGPU_ERR_ARG;
    if (timing_margin < 0 || timing_margin > NB_CP || (reinterpret_cast<uintptr_t>(d_frames) & 7u)) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    dabk::CirArgs a{};
    a.iq = static_cast<const float2 *>(d_iq);
    a.stride = stream_stride;
    a.n_streams = n_streams;
    a.frames_per_stream = max_frames;
    a.acq = reinterpret_cast<const dabk::AcquiredFrame *>(d_frames);
    a.timing_margin = timing_margin;
    return cir_launch(ctx, a, d_frame, d_acc, stream);
}

int dabgpu_cir_analyse(const dabgpu_cir_acc *acc, const dabgpu_cir_cfg *cfg, dabgpu_cir_report *report,
                       dabgpu_cir_path *out, int max_out) {
    dabgpu_cir_cfg def;
    dabgpu_cir_default_cfg(&def);
    if (!cfg) cfg = &def;
    if (!acc || max_out < 0 || (max_out > 0 && !out) || !std::isfinite(cfg->min_snr_db) || !std::isfinite(cfg->range_db))
        return DABGPU_ERR_ARG;
    constexpr int N = dabk::CIR_TAPS;
    dabgpu_cir_report r{};
    r.frames = acc->frames;
    std::vector<double> p(N);
    double floor = 0.0, peak = 0.0;
    if (acc->frames != 0) {
        const double F = double(acc->frames);
        for (int n = 0; n < N; n++) p[n] = double(acc->tap[n]) / F;
        std::vector<double> sorted(p);
        std::sort(sorted.begin(), sorted.end());
        // the median of a mean of F unit exponentials: what a noise-only tap of a sum over F frames has
        const double m = 1.0 - 1.0 / (3.0 * F) + 8.0 / (405.0 * F * F);
        floor = 0.5 * (sorted[N / 2 - 1] + sorted[N / 2]) / m;
        peak = sorted[N - 1];
        r.floor = float(floor);
        r.peak = float(peak);
    }
    struct Found {
        double delay, power;
    };
    std::vector<Found> found;
    if (acc->frames != 0 && floor > 0.0) {
        const double min_p = std::max(floor * std::pow(10.0, double(cfg->min_snr_db) / 10.0),
                                      peak * std::pow(10.0, -double(cfg->range_db) / 10.0));
        for (int n = 0; n < N; n++) {
            const double pm = p[(n + N - 1) % N], p0 = p[n], pp = p[(n + 1) % N];
            if (!(p0 > pm && p0 >= pp && p0 >= min_p)) continue;
            const double Lm = 10.0 * std::log10(std::max(pm, 1e-30)), L0 = 10.0 * std::log10(std::max(p0, 1e-30)),
                         Lp = 10.0 * std::log10(std::max(pp, 1e-30));
            const double den = Lm - 2.0 * L0 + Lp;
            const double frac = den < 0.0 ? 0.5 * (Lm - Lp) / den : 0.0;
            found.push_back(Found{double(n >= N / 2 ? n - N : n) + frac, p0});
        }
    }
    std::stable_sort(found.begin(), found.end(), [](const Found &x, const Found &y) { return x.delay < y.delay; });
    const int n_paths = int(found.size());
    r.n_paths = n_paths;
    if (n_paths > 0) {
        const double first = found[0].delay;
        double strongest = found[0].delay, best = found[0].power, sum_p = 0.0, sum_pd = 0.0, within = 0.0, beyond = 0.0;
        for (const Found &f : found) {
            if (f.power > best) { best = f.power; strongest = f.delay; }
            sum_p += f.power;
            sum_pd += f.power * f.delay;
            (f.delay - first > double(NB_CP) ? beyond : within) += f.power;
        }
        double spread = 0.0;
        if (n_paths > 1) {
            const double mean = sum_pd / sum_p;
            double var = 0.0;
            for (const Found &f : found) var += f.power * (f.delay - mean) * (f.delay - mean);
            spread = std::sqrt(var / sum_p);
        }
        r.first_delay = float(first);
        r.strongest_delay = float(strongest);
        r.rms_delay_spread = float(spread);
        r.guard_ratio_db = beyond > 0.0 ? float(10.0 * std::log10(within / beyond)) : INFINITY;
        for (int i = 0; i < n_paths && i < max_out; i++) {
            const Found &f = found[i];
            out[i] = dabgpu_cir_path{float(f.delay), float(10.0 * std::log10(f.power / peak)), float(10.0 * std::log10(f.power / floor)),
                                     f.delay - first > double(NB_CP) ? DABGPU_CIR_BEYOND_GUARD : 0};
        }
    }
    if (report) *report = r;
    return n_paths;
}

// ---------------------------------------------------------------------------- reception quality
static_assert(sizeof(dabgpu_mer) == sizeof(dabk::MerSums), "ABI struct mirrors the kernel's");
static_assert(sizeof(dabgpu_ber_count) == 8, "{errors, bits}: one uint2 per codeword");

int dabgpu_mer_dev(dabgpu_ctx *ctx, const int8_t *d_soft, size_t soft_stride, int n_frames, int first_symbol, int n_symbols,
                   dabgpu_mer *d_out, void *stream) {
    if (!ctx || !d_soft || !d_out || n_frames < 0) return DABGPU_ERR_ARG;
    if (first_symbol < 0 || n_symbols < 1 || first_symbol + n_symbols > NB_DATA_SYMBOLS) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    const size_t stride = n_frames > 1 ? soft_stride : 0;     // (one frame: the stride is never used)
    if (n_frames > 1 && stride < size_t(first_symbol + n_symbols) * NB_SYM_BITS) return DABGPU_ERR_ARG;
    if (((reinterpret_cast<uintptr_t>(d_soft) | stride) & 15) || (reinterpret_cast<uintptr_t>(d_out) & 7)) return DABGPU_ERR_ARG;
    if (n_frames == 0) return DABGPU_OK;
    HIP_TRY(dabk::launch_mer(d_soft, stride, n_frames, first_symbol, n_symbols, reinterpret_cast<dabk::MerSums *>(d_out),
                             pick_stream(ctx, stream)));
    return DABGPU_OK;
}

int dabgpu_channel_ber_dev(dabgpu_ctx *ctx, const int8_t *d_soft, size_t soft_stride, int n_streams, int frames_per_stream,
                           const uint8_t *d_fib, dabgpu_ber_count *d_fic, const dabgpu_subchannel *sc, int n_subchannels,
                           const int8_t *const *d_history_in, const uint8_t *const *d_out, dabgpu_ber_count *const *d_msc,
                           void *stream) {
    if (!ctx || !d_soft || n_streams < 0 || frames_per_stream < 0 || n_subchannels < 0) return DABGPU_ERR_ARG;
    if (d_fib && (!d_fic || (reinterpret_cast<uintptr_t>(d_fic) & 7))) return DABGPU_ERR_ARG;
    if (n_subchannels > 0 && (!sc || !d_out || !d_msc)) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    const size_t nframes = size_t(n_streams) * frames_per_stream;
    if (nframes > 1 && soft_stride < size_t(n_subchannels > 0 ? NB_FRAME_BITS : NB_FIC_BITS)) return DABGPU_ERR_ARG;
    // validate everything before enqueueing anything: profiles, bounds, no overlap inside the CIF (as the decode calls)
    std::vector<dabk::BerItem> items;
    if (d_fib) {
        dabk::BerItem it{};
        it.nsteps = ctx->fic.prof.nsteps;
        it.prbs_bytes = ctx->fic.d_prbs;
        it.punct_idx = ctx->fic.d_punct_idx;
        it.args.soft = d_soft;
        it.args.soft_stride = soft_stride;
        it.args.n_streams = n_streams;
        it.args.frames_per_stream = frames_per_stream;
        it.args.out = const_cast<uint8_t *>(d_fib);       // (read only)
        it.is_fic = true;
        it.counts = reinterpret_cast<uint32_t *>(d_fic);
        items.push_back(it);
    }
    const SubchannelPlan plan(ctx, sc, n_subchannels, d_out);
    if (plan.rc) return plan.rc;
    for (int i = 0; i < n_subchannels; i++) {
        if (!d_msc[i] || (reinterpret_cast<uintptr_t>(d_msc[i]) & 7)) return DABGPU_ERR_ARG;
        const DeviceCode *dc = plan.code[size_t(i)];
        dabk::BerItem it{};
        it.nsteps = dc->prof.nsteps;
        it.prbs_bytes = dc->d_prbs;
        it.punct_idx = dc->d_punct_idx;
        it.args = msc_args(sc[i], d_soft, soft_stride, n_streams, frames_per_stream, d_history_in ? d_history_in[i] : nullptr, nullptr,
                           const_cast<uint8_t *>(d_out[i]));    // (read only)
        it.counts = reinterpret_cast<uint32_t *>(d_msc[i]);
        items.push_back(it);
    }
    if (nframes == 0 || items.empty()) return DABGPU_OK;
    HIP_TRY(dabk::launch_channel_ber(items.data(), int(items.size()), pick_stream(ctx, stream)));
    return DABGPU_OK;
}

}  // extern "C"
