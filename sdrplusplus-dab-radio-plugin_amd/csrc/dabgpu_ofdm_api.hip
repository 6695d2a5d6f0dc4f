// dabgpu_ofdm_api.hip -- the front-end entry points of the C ABI (include/dabgpu.h): OFDM demodulation of frames, streams,
// acquired and tracked frames, the FFT stage, PRS synchronisation, acquisition, the one-frame host call.
#include "dabgpu_ctx.hpp"

#include <algorithm>
#include <cstring>

using namespace dab;
using namespace dabapi;

namespace {

// How a launch's frames are cut into runs of consecutive symbols (one run = one item of the launch's queue; 12 wavefronts
// resident per CU take them).  A cut costs one more transform and one more symbol read (the run's differential reference),
// so cuts are made only where they buy balance: as many whole frames as fill the resident wave slots an integer number
// of times go first, uncut; the frames behind them -- which alone would leave most slots idle for the length of a frame --
// are cut into `parts`.  Cost model, in symbol transforms per wave slot: passes x (symbols per item + 1).
// The model counts passes over the wave slots as if they began together.  They do not: the waves take items from a queue
// as they finish, and after the whole frames they finish up to a whole item's length apart, so the launch ends when the
// last of the cut items does.  Shorter ones end it sooner: the frames behind the whole ones are cut into at least
// TAIL_MIN_PARTS.  Measured on 64 x 256 frames (profiles/front_end_queue.md; the model alone says 3): 3 parts 5.272 ms,
// 4 parts 5.252 ms, 6 parts 5.224 ms per launch -- although 6 parts read 0.4 % more than 3.
constexpr int TAIL_MIN_PARTS = 6;
struct RunPlan {
    int uncut_frames, parts;
};
RunPlan plan_runs(const dabgpu_ctx *ctx, int n_frames, int total_syms) {
    if (ctx->ofdm_parts_override > 0 && ctx->ofdm_parts_override <= total_syms) return RunPlan{0, ctx->ofdm_parts_override};
    const long slots = long(ctx->wave_slots);
    auto uniform = [&](long frames, int *best_p) {
        long best_cost = -1;
        *best_p = 1;
        for (int p = 1; p <= total_syms && frames > 0; p++) {
            const long rounds = (frames * p + slots - 1) / slots;
            const long cost = rounds * ((total_syms + p - 1) / p + 1);
            if (best_cost < 0 || cost < best_cost) { best_cost = cost; *best_p = p; }
        }
        return best_cost < 0 ? 0 : best_cost;
    };
    int p_all = 1, p_tail = 1;
    const long cost_all = uniform(n_frames, &p_all);
    const long whole = long(n_frames) / slots * slots;
    const long cost_mixed = whole / slots * (total_syms + 1) + uniform(long(n_frames) - whole, &p_tail);
    if (whole > 0 && cost_mixed < cost_all) return RunPlan{int(whole), std::max(p_tail, TAIL_MIN_PARTS)};
    return RunPlan{0, p_all};
}

dabk::OfdmTables ofdm_tables(const dabgpu_ctx *ctx) { return dabk::OfdmTables{ctx->d_twiddle, ctx->d_bin_of_n, ctx->d_n_of_vj}; }

// The run queue of the next front-end launch on `s` (dabk::RunQueue, QueueRing): the next pair of the stream's ring, which
// is made -- and zeroed on `s`, ahead of the launch -- the first time the stream is seen.
int next_run_queue(dabgpu_ctx *ctx, hipStream_t s, dabk::RunQueue &q) {
    auto it = ctx->run_queues.find(s);
    if (it == ctx->run_queues.end()) {
        // (a caller that keeps making streams: the rings of the ones it has dropped go once nothing can be using them)
        if (ctx->run_queues.size() >= 64) {
            HIP_TRY(hipDeviceSynchronize());
            for (auto &kv : ctx->run_queues) (void)hipFree(kv.second.d_pairs);
            ctx->run_queues.clear();
        }
        QueueRing ring;
        constexpr size_t bytes = sizeof(unsigned) * QUEUE_RING * QUEUE_PAIR_STRIDE;
        if (hipMalloc(reinterpret_cast<void **>(&ring.d_pairs), bytes) != hipSuccess) return DABGPU_ERR_NOMEM;
        if (hipMemsetAsync(ring.d_pairs, 0, bytes, s) != hipSuccess) { (void)hipFree(ring.d_pairs); return DABGPU_ERR_HIP; }
        it = ctx->run_queues.emplace(s, ring).first;
    }
    QueueRing &ring = it->second;
    q.pair = ring.d_pairs + size_t(ring.launches++ % QUEUE_RING) * QUEUE_PAIR_STRIDE;
    q.wave_slots = ctx->wave_slots;
    return DABGPU_OK;
}
dabk::SyncTables sync_tables(const dabgpu_ctx *ctx) {
    return dabk::SyncTables{ctx->d_twiddle, ctx->d_prs_qt, ctx->d_sync_pairs, ctx->n_sync_pairs, ctx->d_sync_fs};
}

// The one fused front-end launch behind every call: `a` arrives with what is particular to the caller (a.spectra set: the
// FFT stage, total_syms = 76; else the demodulation, 75); the tables, the soft-bit selection (demodulation only), the run
// plan and the launch are the same for all.  The timer spans this launch alone: what the stream and tracked calls launch
// behind it (their state updates) stays outside (dabgpu_mean_kernel_ms 0 is the front-end kernel's own time).
int launch_front_end(dabgpu_ctx *ctx, dabk::OfdmArgs &a, int total_syms, TimerSlot timer, hipStream_t s) {
    const dabk::OfdmTables tab = ofdm_tables(ctx);
    if (!a.spectra) a.keep = ctx->d_keep;
    dabk::RunQueue q{};
    const int rc = next_run_queue(ctx, s, q);
    if (rc) return rc;
    ScopedTimer tm(ctx, timer, s);
    const RunPlan plan = plan_runs(ctx, a.n_frames, total_syms);
    a.uncut_frames = plan.uncut_frames;
    HIP_TRY(a.spectra ? dabk::launch_fft_symbols(tab, a, plan.parts, q, s) : dabk::launch_ofdm_demod(tab, a, plan.parts, q, s, ctx->iq_format));
    return DABGPU_OK;
}

// terms a frame contributes to the decision-directed loop's sum (its quality gate scales with them): 256 carriers of
// every data symbol the launch demodulated
int dd_terms_per_frame(const dabgpu_ctx *ctx, const dabk::OfdmArgs &a) {
    return 256 * ((a.keep && !a.dqpsk) ? ctx->keep_symbols : NB_DATA_SYMBOLS);
}

// the alignment a device IQ pointer and its frame stride need
bool iq_unaligned(const dabgpu_ctx *ctx, const void *d_iq, size_t frame_stride) {
    // integer samples: one sample of alignment, any stride (frames at odd sample offsets take the per-sample loads)
    if (ctx->iq_format != dabk::IQ_CF32) return iq_misaligned(ctx, d_iq);
    return (reinterpret_cast<uintptr_t>(d_iq) & 15u) || (frame_stride & 1u);
}

int check_iq(const dabgpu_ctx *ctx, const void *d_iq, size_t frame_stride, int n_frames) {
    if (!d_iq || n_frames < 0) return DABGPU_ERR_ARG;
    if (iq_unaligned(ctx, d_iq, frame_stride)) return DABGPU_ERR_ARG;
    if (n_frames > 1 && frame_stride < size_t(NB_FRAME_SYMBOLS) * NB_SYM_PERIOD) return DABGPU_ERR_ARG;
    return DABGPU_OK;
}

// bytes from the first sample of the first frame to the last of the last
size_t iq_span(size_t frame_stride, int n_frames) {
    return (size_t(n_frames - 1) * frame_stride + size_t(NB_FRAME_SYMBOLS) * NB_SYM_PERIOD) * sizeof(float2);
}

// the soft bits of a host-pointer call back to the caller (`whole_frames`: the call wrote all of them, selection or not)
void download_soft(HostCall &h, int8_t *soft, int n_frames, bool whole_frames) {
    if (h.rc || !h.ctx->d_keep || whole_frames) return h.down(STAGE_SOFT, soft);
    // a selection is active: the kernel wrote only the selected runs of the staging buffer, and only those go
    // back -- the rest of the caller's `soft` stays as it was (one strided copy per run, over all frames)
    const int8_t *d_soft = static_cast<const int8_t *>(h.ctx->d_stage[STAGE_SOFT]);
    for (const dabgpu_bit_range &r : h.ctx->keep_ranges)
        if (hipMemcpy2DAsync(soft + r.first, NB_FRAME_BITS, d_soft + r.first, NB_FRAME_BITS, size_t(r.count), size_t(n_frames),
                             hipMemcpyDeviceToHost, h.ctx->stream) != hipSuccess) {
            h.rc = DABGPU_ERR_HIP;
            return;
        }
}

bool peak_rule_ok(float distance_prob, float first_path_rel) {
    return distance_prob >= 0.f && distance_prob <= 1.f && first_path_rel >= 0.f && first_path_rel <= 1.f;
}

// scratch + argument block of the acquisition kernels (dabgpu_acquire_dev, auto-acquisition of the tracked call)
int acquire_args(dabgpu_ctx *ctx, const void *d_iq, size_t stream_stride, int n_streams, int64_t n_samples,
                 const dabgpu_acquire_cfg &c, int max_frames, dabgpu_acquired_frame *d_out, int32_t *d_counts,
                 hipStream_t s, dabk::AcquireArgs &a) {
    const size_t need = dabk::acquire_scratch_bytes(n_streams, n_samples, max_frames);
    if (ctx->acq_scratch_bytes < need) {
        HIP_TRY(hipStreamSynchronize(s));
        if (ctx->d_acq_scratch) (void)hipFree(ctx->d_acq_scratch);
        ctx->d_acq_scratch = nullptr;
        ctx->acq_scratch_bytes = 0;
        if (hipMalloc(&ctx->d_acq_scratch, need) != hipSuccess) return DABGPU_ERR_NOMEM;
        ctx->acq_scratch_bytes = need;
    }
    a.iq = static_cast<const float2 *>(d_iq);
    a.stream_stride = stream_stride;
    a.n_streams = n_streams;
    a.n_samples = n_samples;
    a.thr_start = c.thr_null_start;
    a.thr_end = c.thr_null_end;
    a.level_chunk = c.level_chunk_blocks;
    a.min_blocks = c.min_null_blocks;
    a.max_coarse = c.max_coarse_carriers;
    a.min_peak_to_mean = c.min_peak_to_mean;
    a.margin = c.timing_margin;
    a.rule.distance_prob = c.impulse_peak_distance_probability;
    a.rule.expected = 0;
    a.rule.first_path_rel = c.first_path_rel;
    a.max_out = max_frames;
    a.l1 = static_cast<float *>(ctx->d_acq_scratch);
    const size_t l1_bytes = (size_t(n_streams) * size_t(n_samples / 64) * sizeof(float) + 255) & ~size_t(255);
    a.cands = reinterpret_cast<int64_t *>(static_cast<char *>(ctx->d_acq_scratch) + l1_bytes);
    a.out = reinterpret_cast<dabk::AcquiredFrame *>(d_out);
    a.counts = d_counts;
    return DABGPU_OK;
}

int track_cfg(const dabgpu_track_cfg *cfg, dabgpu_track_cfg &c) {
    if (cfg) c = *cfg; else dabgpu_track_default_cfg(&c);
    auto unit = [](float v) { return v >= 0.f && v <= 1.f; };
    if (!unit(c.fine_freq_update_beta) || !unit(c.signal_update_beta) || !unit(c.thr_null_start) || !unit(c.drift_beta) ||
        !unit(c.coarse_freq_slow_beta) || !peak_rule_ok(c.impulse_peak_distance_probability, c.first_path_rel) ||
        !(c.min_peak_to_mean >= 0.f) || c.timing_margin < 0 || c.timing_margin > NB_CP || c.max_coarse_carriers < 0 ||
        c.max_coarse_carriers > 1023 || !(c.dd_gate >= 0.f && c.dd_gate <= 1000.f) || c.reserved != 0)
        return DABGPU_ERR_ARG;
    return DABGPU_OK;
}

// What a tracked call launches (tracked_launches): where the streams lie, where the results go, and the riders the
// one-frame call adds.  Value-initialised: everything optional is off.
struct TrackedCall {
    dabk::StreamState *states = nullptr;             // the streams' tracking state (device)
    const void *d_iq = nullptr;                      // [n_streams][stream_stride] cf32
    size_t stream_stride = 0;
    int n_streams = 0;
    int64_t n_samples = 0;                           // samples per stream in this call
    int max_frames = 1;                              // output rows per stream
    int64_t advance = 0;                             // samples the streams move on by after the call
    int fixed_start = 0;                             // the frame starts at sample 0 of its stream (one-frame call)
    int acquiring = 0;                               // ... and is the first after a null detection (coarse search, lock check)
    int8_t *d_soft = nullptr;
    void *d_cyc = nullptr, *d_dd4 = nullptr;         // the fine loop's input: cyclic-prefix correlations, or fourth-power sums
    void *d_dqpsk = nullptr;
    dabgpu_acquired_frame *d_frames = nullptr;
    dabgpu_sync_result *d_sync = nullptr;
    int32_t *d_counts = nullptr;
    const dabk::AcquireArgs *auto_acq = nullptr;     // streams that are not tracking are acquired in the same call
    // riders of the one-frame call: the frame's upload inside the synchronisation launch, the download inside the update's
    const void *upload_from = nullptr;
    size_t upload_bytes = 0;
    const dabk::CopyPiece *down = nullptr;           // n_down (<= 3) pieces
    int n_down = 0;
    dabk::StreamState *state_out = nullptr;          // the new state, written to page-locked memory by the updating workgroup
    bool note_states = true;                         // record the state event behind the call (off: the call synchronises itself)
};

// the three launches of a tracked call on `s`: PRS synchronisation at the predicted positions, demodulation of the frames
// where they lie, state update
int tracked_launches(dabgpu_ctx *ctx, const TrackedCall &k, const dabgpu_track_cfg &c, hipStream_t s) {
    const dabk::SyncTables stab = sync_tables(ctx);
    dabk::TrackArgs t{};
    t.state = k.states;
    t.iq = static_cast<const float2 *>(k.d_iq);
    t.stream_stride = k.stream_stride;
    t.n_streams = k.n_streams;
    t.n_samples = k.n_samples;
    t.max_out = k.max_frames;
    t.margin = c.timing_margin;
    t.min_peak_to_mean = c.min_peak_to_mean;
    t.rule.distance_prob = c.impulse_peak_distance_probability;
    t.rule.first_path_rel = c.first_path_rel;
    t.fixed_start = k.fixed_start;
    t.max_coarse = k.fixed_start ? c.max_coarse_carriers : 0;
    t.acquiring = k.acquiring;
    t.coarse_slow_beta = c.coarse_freq_slow_beta;
    t.out = reinterpret_cast<dabk::AcquiredFrame *>(k.d_frames);
    t.sync_out = reinterpret_cast<dabk::SyncResult *>(k.d_sync);
    if (k.upload_from) {
        // the one-frame call: the frame's upload rides in this launch, and the synchronisation reads its PRS straight
        // from the caller's page-locked buffer meanwhile (TrackArgs::copy_*)
        t.sync_iq = static_cast<const float2 *>(k.upload_from);
        t.copy_dst = static_cast<uint4 *>(const_cast<void *>(k.d_iq));
        t.copy_src = static_cast<const uint4 *>(k.upload_from);
        t.copy_n16 = unsigned(k.upload_bytes >> 4);
    }
    HIP_TRY(dabk::launch_track_sync(stab, t, s, ctx->iq_format));
    // streams that are not tracking: acquired here (their rows of d_frames / d_counts; the pass above left them empty)
    if (k.auto_acq) HIP_TRY(dabk::launch_acquire(stab, *k.auto_acq, s, ctx->iq_format));
    dabk::OfdmArgs a{};
    a.iq = t.iq;
    a.frame_stride = k.stream_stride;
    a.n_frames = k.n_streams * k.max_frames;
    a.soft = k.d_soft;
    a.cyc = static_cast<float2 *>(k.d_cyc);
    a.dd4 = static_cast<float2 *>(k.d_dd4);
    a.dqpsk = static_cast<float2 *>(k.d_dqpsk);
    a.acq = reinterpret_cast<const dabk::AcquiredFrame *>(k.d_frames);
    a.acq_per_stream = k.max_frames;
    int rc = launch_front_end(ctx, a, NB_DATA_SYMBOLS, TIMER_OFDM, s);
    if (rc) return rc;
    dabk::TrackUpdateArgs u{};
    u.state = k.states;
    u.frames = t.out;
    u.cyc = a.cyc ? a.cyc : a.dd4;
    u.dd = a.cyc ? 0 : 1;
    u.iq = t.iq;
    u.stream_stride = k.stream_stride;
    u.n_streams = k.n_streams;
    u.n_samples = k.n_samples;
    u.max_out = k.max_frames;
    u.advance = k.advance;
    u.fine_beta = c.fine_freq_update_beta;
    u.drift_beta = c.drift_beta;
    u.signal_beta = c.signal_update_beta;
    u.thr_null_start = c.thr_null_start;
    u.fixed_start = k.fixed_start;
    u.counts = k.d_counts;
    u.dd_gate = c.dd_gate;
    u.dd_terms_per_frame = dd_terms_per_frame(ctx, a);
    for (int i = 0; i < k.n_down && i < 3; i++) u.down[i] = k.down[i];
    u.state_out = k.state_out;
    // ... and their tracking starts from what the acquisition found (marked 2; the update launch makes it 1)
    if (k.auto_acq)
        HIP_TRY(dabk::launch_track_start(k.states, t.out, k.d_counts, k.n_streams, k.max_frames, k.advance, 1, s));
    HIP_TRY(dabk::launch_track_update(u, s, ctx->iq_format));
    return k.note_states ? note_state_use(ctx, s) : DABGPU_OK;
}
}  // namespace

extern "C" {

// ---------------------------------------------------------------------------- OFDM
int dabgpu_ofdm_demod_frames_dev(dabgpu_ctx *ctx, const void *d_iq, size_t frame_stride, int n_frames,
                                 const float *d_freq_offset, int8_t *d_soft, void *d_cyc, void *d_dqpsk,
                                 void *stream) {
    if (!ctx || !d_soft || (d_dqpsk && cf32_only(ctx))) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    int rc = check_iq(ctx, d_iq, frame_stride, n_frames);
    if (rc) return rc;
    if (reinterpret_cast<uintptr_t>(d_soft) & 15u) return DABGPU_ERR_ARG;
    if (n_frames == 0) return DABGPU_OK;
    dabk::OfdmArgs a{};
    a.iq = static_cast<const float2 *>(d_iq);
    a.frame_stride = frame_stride;
    a.freq_offset = d_freq_offset;
    a.n_frames = n_frames;
    a.soft = d_soft;
    a.cyc = static_cast<float2 *>(d_cyc);
    a.dqpsk = static_cast<float2 *>(d_dqpsk);
    return launch_front_end(ctx, a, NB_DATA_SYMBOLS, TIMER_OFDM, pick_stream(ctx, stream));
}

int dabgpu_ofdm_demod_frames_dd_dev(dabgpu_ctx *ctx, const void *d_iq, size_t frame_stride, int n_frames,
                                    const float *d_freq_offset, int8_t *d_soft, void *d_dd4, void *stream) {
    if (!ctx || !d_soft || !d_dd4) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    int rc = check_iq(ctx, d_iq, frame_stride, n_frames);
    if (rc) return rc;
    if (reinterpret_cast<uintptr_t>(d_soft) & 15u) return DABGPU_ERR_ARG;
    if (n_frames == 0) return DABGPU_OK;
    dabk::OfdmArgs a{};
    a.iq = static_cast<const float2 *>(d_iq);
    a.frame_stride = frame_stride;
    a.freq_offset = d_freq_offset;
    a.n_frames = n_frames;
    a.soft = d_soft;
    a.dd4 = static_cast<float2 *>(d_dd4);
    return launch_front_end(ctx, a, NB_DATA_SYMBOLS, TIMER_OFDM, pick_stream(ctx, stream));
}

int dabgpu_mover_frames_dev(dabgpu_ctx *ctx, const void *d_iq, size_t frame_stride, int n_frames, int8_t *d_soft,
                            int with_prefixes, void *stream) {
    if (!ctx || !d_soft || cf32_only(ctx)) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    int rc = check_iq(ctx, d_iq, frame_stride, n_frames);
    if (rc) return rc;
    if (reinterpret_cast<uintptr_t>(d_soft) & 15u) return DABGPU_ERR_ARG;
    if (n_frames == 0) return DABGPU_OK;
    const RunPlan plan = plan_runs(ctx, n_frames, NB_DATA_SYMBOLS);
    hipStream_t s = pick_stream(ctx, stream);
    dabk::RunQueue q{};
    if ((rc = next_run_queue(ctx, s, q))) return rc;
    HIP_TRY(dabk::launch_geometry_mover(static_cast<const float2 *>(d_iq), frame_stride, n_frames, d_soft, plan.uncut_frames,
                                        plan.parts, with_prefixes != 0, q, s));
    return DABGPU_OK;
}

int dabgpu_ofdm_set_soft_selection(dabgpu_ctx *ctx, const dabgpu_bit_range *ranges, int n_ranges) {
    if (!ctx || n_ranges < 0 || (n_ranges > 0 && !ranges)) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    if (n_ranges == 0) { ctx->d_keep = nullptr; ctx->keep_ranges.clear(); ctx->keep_symbols = NB_DATA_SYMBOLS; return DABGPU_OK; }
    constexpr int CHUNKS_PER_SYMBOL = NB_SYM_BITS / 16;          // 192 = 3 words
    std::vector<unsigned long long> words(size_t(NB_DATA_SYMBOLS) * 3, 0ull);
    for (int r = 0; r < n_ranges; r++) {
        const int first = ranges[r].first, count = ranges[r].count;
        if (first < 0 || count < 0 || (first & 15) || (count & 15) || first > NB_FRAME_BITS - count) return DABGPU_ERR_ARG;
        for (int c = first / 16; c < (first + count) / 16; c++) {
            const int sym = c / CHUNKS_PER_SYMBOL, k = c % CHUNKS_PER_SYMBOL;
            words[size_t(sym) * 3 + (k >> 6)] |= 1ull << (k & 63);
        }
    }
    // kernels already launched keep reading the table they were given: a new selection gets a new table
    if (ctx->keep_tables.size() >= 256) {
        HIP_TRY(hipDeviceSynchronize());
        for (void *p : ctx->keep_tables) (void)hipFree(p);
        ctx->keep_tables.clear();
        ctx->d_keep = nullptr;
    }
    void *d = nullptr;
    if (hipMalloc(&d, words.size() * sizeof(words[0])) != hipSuccess) return DABGPU_ERR_NOMEM;
    if (hipMemcpy(d, words.data(), words.size() * sizeof(words[0]), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(d);
        return DABGPU_ERR_HIP;
    }
    ctx->keep_tables.push_back(d);
    ctx->d_keep = static_cast<const unsigned long long *>(d);
    ctx->keep_symbols = 0;
    for (int l = 0; l < NB_DATA_SYMBOLS; l++)
        if (words[size_t(l) * 3] | words[size_t(l) * 3 + 1] | words[size_t(l) * 3 + 2]) ctx->keep_symbols++;
    // the same selection as merged byte runs, for the host-pointer call's copy-back
    ctx->keep_ranges.clear();
    for (int c = 0; c < NB_FRAME_BITS / 16; c++) {
        if (!(words[size_t(c / CHUNKS_PER_SYMBOL) * 3 + ((c % CHUNKS_PER_SYMBOL) >> 6)] >> ((c % CHUNKS_PER_SYMBOL) & 63) & 1ull)) continue;
        if (!ctx->keep_ranges.empty() && ctx->keep_ranges.back().first + ctx->keep_ranges.back().count == 16 * c)
            ctx->keep_ranges.back().count += 16;
        else
            ctx->keep_ranges.push_back(dabgpu_bit_range{16 * c, 16});
    }
    return DABGPU_OK;
}

int dabgpu_fft_symbols_dev(dabgpu_ctx *ctx, const void *d_iq, size_t frame_stride, int n_frames,
                           const float *d_freq_offset, void *d_spectra, void *stream) {
    if (!ctx || !d_spectra || cf32_only(ctx)) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    int rc = check_iq(ctx, d_iq, frame_stride, n_frames);
    if (rc) return rc;
    if (n_frames == 0) return DABGPU_OK;
    dabk::OfdmArgs a{};
    a.iq = static_cast<const float2 *>(d_iq);
    a.frame_stride = frame_stride;
    a.freq_offset = d_freq_offset;
    a.n_frames = n_frames;
    a.spectra = static_cast<float2 *>(d_spectra);
    return launch_front_end(ctx, a, NB_FRAME_SYMBOLS, TIMER_FFT, pick_stream(ctx, stream));
}

// host-pointer variants: stage through device buffers on the context stream (HostCall)
int dabgpu_ofdm_demod_frames(dabgpu_ctx *ctx, const float *iq, size_t frame_stride, int n_frames,
                             const float *freq_offset, int8_t *soft, float *cyc, float *dqpsk) {
    if (ctx && cf32_only(ctx)) return DABGPU_ERR_ARG;
    if (!ctx || !iq || !soft || n_frames < 0) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    if (n_frames == 0) return DABGPU_OK;
    HostCall h(ctx);
    void *d_iq = h.room(STAGE_IQ, iq_span(frame_stride, n_frames));
    void *d_soft = h.room(STAGE_SOFT, size_t(n_frames) * NB_FRAME_BITS);
    void *d_fo = h.room(STAGE_AUX, sizeof(float) * n_frames, freq_offset != nullptr);
    void *d_cyc = h.room(STAGE_RESULT, size_t(n_frames) * NB_FRAME_SYMBOLS * sizeof(float2), cyc != nullptr);
    void *d_dq = h.room(STAGE_WIDE, size_t(n_frames) * NB_DATA_SYMBOLS * NB_CARRIERS * sizeof(float2), dqpsk != nullptr);
    h.up(STAGE_IQ, iq);
    h.up(STAGE_AUX, freq_offset);
    if (h.rc) return h.rc;
    const int rc = dabgpu_ofdm_demod_frames_dev(ctx, d_iq, frame_stride, n_frames, static_cast<const float *>(d_fo),
                                                static_cast<int8_t *>(d_soft), d_cyc, d_dq, ctx->stream);
    if (rc) return rc;
    download_soft(h, soft, n_frames, dqpsk != nullptr);
    h.down(STAGE_RESULT, cyc);
    h.down(STAGE_WIDE, dqpsk);
    return h.finish();
}

// ---------------------------------------------------------------------------- closed-loop stream call
int dabgpu_ofdm_demod_streams_dev(dabgpu_ctx *ctx, const void *d_iq, size_t frame_stride, int n_streams,
                                  int frames_per_stream, float fine_freq_update_beta, int8_t *d_soft, void *d_cyc,
                                  void *d_dqpsk, void *stream) {
    if (!ctx || !d_soft || n_streams < 0 || frames_per_stream < 0 || (d_dqpsk && cf32_only(ctx))) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    if (n_streams > ctx->n_states) return DABGPU_ERR_CAPACITY;   // dabgpu_streams_reset first
    if (!(fine_freq_update_beta >= 0.f && fine_freq_update_beta <= 1.f)) return DABGPU_ERR_ARG;
    if (size_t(n_streams) * size_t(frames_per_stream) > size_t(0x7fffffff) / NB_DATA_SYMBOLS) return DABGPU_ERR_ARG;
    const int n_frames = n_streams * frames_per_stream;
    int rc = check_iq(ctx, d_iq, frame_stride, n_frames);
    if (rc) return rc;
    if (reinterpret_cast<uintptr_t>(d_soft) & 15u) return DABGPU_ERR_ARG;
    if (n_frames == 0) return DABGPU_OK;
    hipStream_t s = pick_stream(ctx, stream);
    // No correlation output asked for: the loop's input stays in the library's scratch -- the correlations, or, once the
    // caller has switched the loop to decision-directed (dabgpu_set_stream_loop), the fourth-power sums of the
    // differential symbols: then the cyclic prefixes are not read at all, 17 % fewer bytes for an HBM-bound kernel.
    const bool dd = d_cyc == nullptr && ctx->loop_dd;
    void *d_dd = nullptr;
    if (dd && (rc = stage(ctx, STAGE_LOOP, size_t(n_frames) * NB_FRAME_SYMBOLS * sizeof(float2), &d_dd))) return rc;
    if (!dd && !d_cyc && (rc = stage(ctx, STAGE_LOOP, size_t(n_frames) * NB_FRAME_SYMBOLS * sizeof(float2), &d_cyc))) return rc;
    dabk::OfdmArgs a{};
    a.iq = static_cast<const float2 *>(d_iq);
    a.frame_stride = frame_stride;
    a.n_frames = n_frames;
    a.soft = d_soft;
    a.cyc = static_cast<float2 *>(d_cyc);
    a.dd4 = static_cast<float2 *>(d_dd);
    a.dqpsk = static_cast<float2 *>(d_dqpsk);
    a.state = ctx->d_states;
    a.frames_per_stream = frames_per_stream;
    if ((rc = launch_front_end(ctx, a, NB_DATA_SYMBOLS, TIMER_OFDM, s))) return rc;
    HIP_TRY(dabk::launch_stream_update(ctx->d_states, dd ? a.dd4 : a.cyc, a.iq, frame_stride, n_streams, frames_per_stream,
                                       fine_freq_update_beta, ctx->thr_null_start, ctx->signal_beta, dd ? 1 : 0, ctx->dd_gate,
                                       dd_terms_per_frame(ctx, a), s, ctx->iq_format));
    return note_state_use(ctx, s);
}

int dabgpu_ofdm_demod_streams(dabgpu_ctx *ctx, const float *iq, size_t frame_stride, int n_streams,
                              int frames_per_stream, float fine_freq_update_beta, int8_t *soft, float *cyc,
                              float *dqpsk) {
    if (!ctx || !iq || !soft || n_streams < 0 || frames_per_stream < 0 || cf32_only(ctx)) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    if (size_t(n_streams) * size_t(frames_per_stream) > size_t(0x7fffffff) / NB_DATA_SYMBOLS) return DABGPU_ERR_ARG;
    const int n_frames = n_streams * frames_per_stream;
    if (n_frames == 0) return DABGPU_OK;
    HostCall h(ctx);
    void *d_iq = h.room(STAGE_IQ, iq_span(frame_stride, n_frames));
    void *d_soft = h.room(STAGE_SOFT, size_t(n_frames) * NB_FRAME_BITS);
    void *d_cyc = h.room(STAGE_RESULT, size_t(n_frames) * NB_FRAME_SYMBOLS * sizeof(float2));
    void *d_dq = h.room(STAGE_WIDE, size_t(n_frames) * NB_DATA_SYMBOLS * NB_CARRIERS * sizeof(float2), dqpsk != nullptr);
    h.up(STAGE_IQ, iq);
    if (h.rc) return h.rc;
    const int rc = dabgpu_ofdm_demod_streams_dev(ctx, d_iq, frame_stride, n_streams, frames_per_stream, fine_freq_update_beta,
                                                 static_cast<int8_t *>(d_soft), d_cyc, d_dq, ctx->stream);
    if (rc) return rc;
    download_soft(h, soft, n_frames, dqpsk != nullptr);
    h.down(STAGE_RESULT, cyc);
    h.down(STAGE_WIDE, dqpsk);
    return h.finish();
}

int dabgpu_fft_symbols(dabgpu_ctx *ctx, const float *iq, size_t frame_stride, int n_frames,
                       const float *freq_offset, float *spectra) {
    if (!ctx || !iq || !spectra || n_frames < 0 || cf32_only(ctx)) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    if (n_frames == 0) return DABGPU_OK;
    HostCall h(ctx);
    void *d_iq = h.room(STAGE_IQ, iq_span(frame_stride, n_frames));
    void *d_sp = h.room(STAGE_WIDE, size_t(n_frames) * NB_FRAME_SYMBOLS * NB_FFT * sizeof(float2));
    void *d_fo = h.room(STAGE_AUX, sizeof(float) * n_frames, freq_offset != nullptr);
    h.up(STAGE_IQ, iq);
    h.up(STAGE_AUX, freq_offset);
    if (h.rc) return h.rc;
    const int rc = dabgpu_fft_symbols_dev(ctx, d_iq, frame_stride, n_frames, static_cast<const float *>(d_fo), d_sp, ctx->stream);
    if (rc) return rc;
    h.down(STAGE_WIDE, spectra);
    return h.finish();
}

// ---------------------------------------------------------------------------- PRS sync
static_assert(sizeof(dabgpu_sync_result) == sizeof(dabk::SyncResult), "ABI struct mirrors the kernel's");

int dabgpu_sync_prs_dev(dabgpu_ctx *ctx, const void *d_iq, size_t frame_stride, int n_frames,
                        const float *d_freq_offset, int max_coarse, dabgpu_sync_result *d_out, void *stream) {
    if (!ctx || !d_iq || !d_out || n_frames < 0 || max_coarse < 0 || max_coarse > 1023) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    if (iq_unaligned(ctx, d_iq, frame_stride)) return DABGPU_ERR_ARG;
    if (n_frames > 1 && frame_stride < size_t(NB_SYM_PERIOD)) return DABGPU_ERR_ARG;
    if (n_frames == 0) return DABGPU_OK;
    HIP_TRY(dabk::launch_prs_sync(sync_tables(ctx), static_cast<const float2 *>(d_iq), frame_stride, n_frames, d_freq_offset,
                                  max_coarse, reinterpret_cast<dabk::SyncResult *>(d_out), pick_stream(ctx, stream), ctx->iq_format));
    return DABGPU_OK;
}

int dabgpu_sync_prs(dabgpu_ctx *ctx, const float *iq, size_t frame_stride, int n_frames, const float *freq_offset,
                    int max_coarse, dabgpu_sync_result *out) {
    if (!ctx || !iq || !out || n_frames < 0 || cf32_only(ctx)) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    if (n_frames == 0) return DABGPU_OK;
    HostCall h(ctx);
    void *d_iq = h.room(STAGE_IQ, (size_t(n_frames - 1) * frame_stride + NB_SYM_PERIOD) * sizeof(float2));
    void *d_out = h.room(STAGE_RESULT, sizeof(dabgpu_sync_result) * n_frames);
    void *d_fo = h.room(STAGE_AUX, sizeof(float) * n_frames, freq_offset != nullptr);
    h.up(STAGE_IQ, iq);
    h.up(STAGE_AUX, freq_offset);
    if (h.rc) return h.rc;
    const int rc = dabgpu_sync_prs_dev(ctx, d_iq, frame_stride, n_frames, static_cast<const float *>(d_fo), max_coarse,
                                       static_cast<dabgpu_sync_result *>(d_out), ctx->stream);
    if (rc) return rc;
    h.down(STAGE_RESULT, out);
    return h.finish();
}

// ---------------------------------------------------------------------------- acquisition
void dabgpu_acquire_default_cfg(dabgpu_acquire_cfg *cfg) {
    if (!cfg) return;
    cfg->thr_null_start = 0.35f;
    cfg->thr_null_end = 0.75f;
    cfg->min_null_blocks = 30;
    cfg->max_coarse_carriers = 200;
    cfg->min_peak_to_mean = 30.0f;
    cfg->timing_margin = 64;
    cfg->impulse_peak_distance_probability = 0.15f;
    cfg->first_path_rel = 0.25f;
    cfg->level_chunk_blocks = 256;
    cfg->reserved = 0;
}

int dabgpu_acquire_dev(dabgpu_ctx *ctx, const void *d_iq, size_t stream_stride, int n_streams, int64_t n_samples,
                       const dabgpu_acquire_cfg *cfg, int max_frames, dabgpu_acquired_frame *d_out, int32_t *d_counts,
                       void *stream) {
    static_assert(sizeof(dabgpu_acquired_frame) == 32 && sizeof(dabk::AcquiredFrame) == 32, "acquired-frame layout");
    if (!ctx || !d_iq || !d_out || !d_counts || n_streams < 0 || max_frames <= 0 || n_samples < 0) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    if (iq_misaligned(ctx, d_iq)) return DABGPU_ERR_ARG;
    if (n_streams > 1 && stream_stride < size_t(n_samples)) return DABGPU_ERR_ARG;
    dabgpu_acquire_cfg c;
    if (cfg) c = *cfg; else dabgpu_acquire_default_cfg(&c);
    if (c.max_coarse_carriers < 0 || c.max_coarse_carriers > 1023 || c.min_null_blocks < 1 || c.timing_margin < 0 ||
        c.timing_margin > NB_CP || !(c.thr_null_start > 0.f) || !(c.thr_null_end >= c.thr_null_start) ||
        !peak_rule_ok(c.impulse_peak_distance_probability, c.first_path_rel) ||
        (c.level_chunk_blocks != 0 && (c.level_chunk_blocks < 64 || c.level_chunk_blocks > 16384 ||
                                       (c.level_chunk_blocks & (c.level_chunk_blocks - 1)))))
        return DABGPU_ERR_ARG;
    if (n_streams == 0) return DABGPU_OK;
    hipStream_t s = pick_stream(ctx, stream);
    int rc2;
    if (n_samples < 64) {                                      // nothing to search: no frames anywhere
        HIP_TRY(hipMemsetAsync(d_counts, 0, sizeof(int32_t) * n_streams, s));
        HIP_TRY(hipMemsetAsync(d_out, 0, sizeof(dabgpu_acquired_frame) * size_t(n_streams) * max_frames, s));
        return DABGPU_OK;
    }
    dabk::AcquireArgs a{};
    if ((rc2 = acquire_args(ctx, d_iq, stream_stride, n_streams, n_samples, c, max_frames, d_out, d_counts, s, a))) return rc2;
    HIP_TRY(dabk::launch_acquire(sync_tables(ctx), a, s, ctx->iq_format));
    return DABGPU_OK;
}

int dabgpu_acquire(dabgpu_ctx *ctx, const float *iq, size_t stream_stride, int n_streams, int64_t n_samples,
                   const dabgpu_acquire_cfg *cfg, int max_frames, dabgpu_acquired_frame *out, int32_t *counts) {
    if (!ctx || !iq || !out || !counts || n_streams < 0 || max_frames <= 0 || n_samples < 0 || cf32_only(ctx)) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    if (n_streams == 0) return DABGPU_OK;
    if (n_streams > 1 && stream_stride < size_t(n_samples)) return DABGPU_ERR_ARG;
    // a capture is as large as the caller makes it: its device copy is allocated for the call, not kept
    const size_t nb_iq = (size_t(n_streams - 1) * stream_stride + size_t(n_samples)) * sizeof(float2);
    const size_t nb_out = sizeof(dabgpu_acquired_frame) * size_t(n_streams) * max_frames;
    void *d_iq = nullptr, *d_out = nullptr, *d_cnt = nullptr;
    hipStream_t s = ctx->stream;
    int rc = DABGPU_OK;
    if (hipMalloc(&d_iq, std::max<size_t>(nb_iq, 16)) != hipSuccess || hipMalloc(&d_out, nb_out) != hipSuccess ||
        hipMalloc(&d_cnt, sizeof(int32_t) * n_streams) != hipSuccess)
        rc = DABGPU_ERR_NOMEM;
    if (!rc && hipMemcpyAsync(d_iq, iq, nb_iq, hipMemcpyHostToDevice, s) != hipSuccess) rc = DABGPU_ERR_HIP;
    if (!rc)
        rc = dabgpu_acquire_dev(ctx, d_iq, stream_stride, n_streams, n_samples, cfg, max_frames,
                                static_cast<dabgpu_acquired_frame *>(d_out), static_cast<int32_t *>(d_cnt), s);
    if (!rc && (hipMemcpyAsync(out, d_out, nb_out, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipMemcpyAsync(counts, d_cnt, sizeof(int32_t) * n_streams, hipMemcpyDeviceToHost, s) != hipSuccess))
        rc = DABGPU_ERR_HIP;
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = DABGPU_ERR_HIP;
    if (d_iq) (void)hipFree(d_iq);
    if (d_out) (void)hipFree(d_out);
    if (d_cnt) (void)hipFree(d_cnt);
    return rc;
}

int dabgpu_ofdm_demod_acquired_dev(dabgpu_ctx *ctx, const void *d_iq, size_t stream_stride, int n_streams,
                                   int max_frames, const dabgpu_acquired_frame *d_frames, int8_t *d_soft, void *d_cyc,
                                   void *d_dqpsk, void *stream) {
    if (!ctx || !d_iq || !d_frames || !d_soft || n_streams < 0 || max_frames <= 0 || (d_dqpsk && cf32_only(ctx))) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    if (iq_misaligned(ctx, d_iq) || (reinterpret_cast<uintptr_t>(d_soft) & 15u)) return DABGPU_ERR_ARG;
    if (n_streams == 0) return DABGPU_OK;
    if (size_t(n_streams) * size_t(max_frames) > size_t(0x7fffffff) / NB_DATA_SYMBOLS) return DABGPU_ERR_ARG;
    dabk::OfdmArgs a{};
    a.iq = static_cast<const float2 *>(d_iq);
    a.frame_stride = stream_stride;
    a.n_frames = n_streams * max_frames;
    a.soft = d_soft;
    a.cyc = static_cast<float2 *>(d_cyc);
    a.dqpsk = static_cast<float2 *>(d_dqpsk);
    a.acq = reinterpret_cast<const dabk::AcquiredFrame *>(d_frames);
    a.acq_per_stream = max_frames;
    return launch_front_end(ctx, a, NB_DATA_SYMBOLS, TIMER_OFDM, pick_stream(ctx, stream));
}

// ---------------------------------------------------------------------------- timing tracking
void dabgpu_track_default_cfg(dabgpu_track_cfg *cfg) {
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->fine_freq_update_beta = 0.9f;
    cfg->signal_update_beta = 0.95f;
    cfg->thr_null_start = 0.35f;
    cfg->min_peak_to_mean = 100.0f;
    cfg->impulse_peak_distance_probability = 0.15f;
    cfg->first_path_rel = 0.25f;
    cfg->drift_beta = 0.5f;
    cfg->coarse_freq_slow_beta = 0.1f;
    cfg->timing_margin = 64;
    cfg->max_coarse_carriers = 204;
    cfg->decision_directed = 0;         // the reference's estimator (cyclic-prefix correlations); 1 = this library's own, opt-in
    cfg->auto_acquire = 0;
    cfg->dd_gate = 2.5f;
}

int dabgpu_track_start_dev(dabgpu_ctx *ctx, const dabgpu_acquired_frame *d_frames, const int32_t *d_counts, int n_streams,
                           int max_frames, int64_t advance, int only_lost, void *stream) {
    if (!ctx || !d_frames || !d_counts || n_streams < 0 || max_frames <= 0 || advance < 0) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    if (n_streams > ctx->n_states) return DABGPU_ERR_CAPACITY;   // dabgpu_streams_reset first
    if (n_streams == 0) return DABGPU_OK;
    hipStream_t s = pick_stream(ctx, stream);
    HIP_TRY(dabk::launch_track_start(ctx->d_states, reinterpret_cast<const dabk::AcquiredFrame *>(d_frames), d_counts, n_streams,
                                     max_frames, advance, only_lost ? 1 : 0, s));
    if (only_lost) {
        // (tracking = 2 marks "started in this call" for the tracked call's own use; a stand-alone start has no update
        // launch behind it: turn the marks into 1 here)
        dabk::TrackUpdateArgs u{};
        u.state = ctx->d_states;
        u.n_streams = n_streams;
        u.max_out = 1;
        u.fixed_start = 0;
        u.settle_only = 1;
        HIP_TRY(dabk::launch_track_update(u, s));
    }
    return note_state_use(ctx, s);
}

int dabgpu_ofdm_demod_tracked_dev(dabgpu_ctx *ctx, const void *d_iq, size_t stream_stride, int n_streams,
                                  int64_t n_samples, int max_frames, int64_t advance, const dabgpu_track_cfg *cfg,
                                  int8_t *d_soft, void *d_cyc, void *d_dqpsk, dabgpu_acquired_frame *d_frames,
                                  int32_t *d_counts, void *stream) {
    if (!ctx || !d_iq || !d_soft || !d_frames || !d_counts || n_streams < 0 || max_frames <= 0 || n_samples < 0 || advance < 0 ||
        (d_dqpsk && cf32_only(ctx)))
        return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    if (iq_misaligned(ctx, d_iq) || (reinterpret_cast<uintptr_t>(d_soft) & 15u)) return DABGPU_ERR_ARG;
    if (n_streams > 1 && stream_stride < size_t(n_samples)) return DABGPU_ERR_ARG;
    if (n_streams > ctx->n_states) return DABGPU_ERR_CAPACITY;   // dabgpu_streams_reset first
    if (size_t(n_streams) * size_t(max_frames) > size_t(0x7fffffff) / NB_DATA_SYMBOLS) return DABGPU_ERR_ARG;
    dabgpu_track_cfg c;
    int rc = track_cfg(cfg, c);
    if (rc) return rc;
    if (n_streams == 0) return DABGPU_OK;
    hipStream_t s = pick_stream(ctx, stream);
    // (no correlation output asked for: the loop's input stays in the library's scratch -- the cyclic-prefix correlations by
    // default, as the reference's loop; cfg.decision_directed: the fourth-power sums, the cyclic prefixes are not read -- see
    // the stream call; acquisition leaves the fine offset well inside that estimator's range)
    void *d_dd = nullptr;
    if (!d_cyc && (rc = stage(ctx, STAGE_LOOP, size_t(n_streams) * max_frames * NB_FRAME_SYMBOLS * sizeof(float2), c.decision_directed ? &d_dd : &d_cyc)))
        return rc;
    dabk::AcquireArgs acq{};
    if (c.auto_acquire && n_samples >= 64) {
        dabgpu_acquire_cfg ac;
        dabgpu_acquire_default_cfg(&ac);
        ac.thr_null_start = c.thr_null_start;
        ac.max_coarse_carriers = c.max_coarse_carriers;
        ac.timing_margin = c.timing_margin;
        ac.impulse_peak_distance_probability = c.impulse_peak_distance_probability;
        ac.first_path_rel = c.first_path_rel;
        if ((rc = acquire_args(ctx, d_iq, stream_stride, n_streams, n_samples, ac, max_frames, d_frames, d_counts, s, acq))) return rc;
        acq.skip_tracked = ctx->d_states;
    }
    TrackedCall k;
    k.states = ctx->d_states;
    k.d_iq = d_iq;
    k.stream_stride = stream_stride;
    k.n_streams = n_streams;
    k.n_samples = n_samples;
    k.max_frames = max_frames;
    k.advance = advance;
    k.d_soft = d_soft;
    k.d_cyc = d_cyc;
    k.d_dd4 = d_dd;
    k.d_dqpsk = d_dqpsk;
    k.d_frames = d_frames;
    k.d_counts = d_counts;
    k.auto_acq = (c.auto_acquire && n_samples >= 64) ? &acq : nullptr;
    return tracked_launches(ctx, k, c, s);
}

int dabgpu_ofdm_demod_stream_frame(dabgpu_ctx *ctx, int stream_index, const float *iq, int acquiring,
                                   const dabgpu_track_cfg *cfg, int8_t *soft, float *dqpsk, dabgpu_frame_result *result) {
    if (!ctx || !iq || !soft || !result || stream_index < 0 || stream_index >= ctx->n_states || cf32_only(ctx)) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    dabgpu_track_cfg c;
    int rc = track_cfg(cfg, c);
    if (rc) return rc;
    constexpr size_t nb_iq = size_t(NB_FRAME_SYMBOLS) * NB_SYM_PERIOD * sizeof(float2);
    constexpr size_t nb_dq = size_t(NB_DATA_SYMBOLS) * NB_CARRIERS * sizeof(float2);
    auto al = [](size_t v) { return (v + 255) & ~size_t(255); };
    // one result block: soft bits | acquired frame | sync result | state  (| constellation, in a buffer of its own)
    const size_t off_fr = al(NB_FRAME_BITS), off_sy = off_fr + al(sizeof(dabgpu_acquired_frame)),
                 off_st = off_sy + al(sizeof(dabgpu_sync_result)), nb_res = off_st + al(sizeof(dabk::StreamState));
    void *d_iq, *d_res, *d_cyc = nullptr, *d_dd = nullptr, *d_dq = nullptr;
    if ((rc = stage(ctx, STAGE_IQ, nb_iq, &d_iq))) return rc;
    if ((rc = stage(ctx, STAGE_SOFT, nb_res, &d_res))) return rc;
    // the fine loop's input: the 76 cyclic-prefix correlations (the reference's estimator, the default), or -- opt-in,
    // cfg->decision_directed -- the fourth-power sums
    if ((rc = stage(ctx, STAGE_LOOP, NB_FRAME_SYMBOLS * sizeof(float2), c.decision_directed ? &d_dd : &d_cyc))) return rc;
    if (dqpsk && (rc = stage(ctx, STAGE_WIDE, nb_dq, &d_dq))) return rc;
    if ((rc = ensure_bounce(ctx, nb_res))) return rc;
    if ((rc = wait_state_use(ctx))) return rc;
    if (injected_failure(ctx)) return DABGPU_ERR_HIP;            // (test hook: a device call that fails before any launch)
    hipStream_t s = ctx->stream;
    char *res = static_cast<char *>(d_res);
    // one upload: by a kernel when the frame lies in page-locked memory the device can address (the host mirror's does)
    static_assert(nb_iq % 16 == 0 && NB_FRAME_BITS % 16 == 0, "whole 16-byte words");
    // (every query first: once the upload is enqueued the host only enqueues, and stays ahead of the device)
    void *h_dev = nullptr;
    HIP_TRY(hipHostGetDevicePointer(&h_dev, ctx->h_bounce, 0));
    void *iq_alias = device_alias_of_pinned(iq), *soft_alias = device_alias_of_pinned(soft);
    if ((reinterpret_cast<uintptr_t>(iq_alias) | reinterpret_cast<uintptr_t>(soft_alias)) & 15) iq_alias = soft_alias = nullptr;
    if (!iq_alias) HIP_TRY(hipMemcpyAsync(d_iq, iq, nb_iq, hipMemcpyHostToDevice, s));
    dabk::StreamState *st = ctx->d_states + stream_index;
    // Page-locked buffers (the host mirror's): the 1.55 MB upload is the longest single piece of the call (37 us), and the
    // PRS synchronisation (20 us) only needs the frame's first symbol -- so the upload rides in the synchronisation's own
    // launch: its extra workgroups copy the frame while the first one reads its 20 kB straight from the caller's buffer.
    // The call ends in its own synchronisation, so no state event is recorded (an event record between two launches
    // cost 5.6 us of idle device).  Measured and rejected on the way (profiles/r05_frame_path.md): the synchronisation
    // on a second stream (the cross-stream event: 11 us of idle device), soft bits written by the demodulation launch
    // straight into the caller's buffer (the launch 3.4 us slower, the copy behind it only 1.6 us shorter).
    // ... and the download rides in the LAST launch (the state update's): soft bits (straight into the caller's buffer when
    // that is page-locked too: no copy by the CPU afterwards), frame and sync records; the updating workgroup writes the
    // new state to the landing area itself.  Three launches per call: upload + synchronisation, demodulation, update + download.
    static_assert(sizeof(dabk::StreamState) % 16 == 0, "the state goes out in 16-byte words");
    char *hd = static_cast<char *>(h_dev);
    // ... and the constellation, when a display asks for it and its buffer is coherent page-locked memory (the host mirror's
    // is): 0.9 MB more in the same launch instead of a copy-engine transfer and a sleep behind it
    void *dq_alias = (dqpsk && known_coherent_host(dqpsk, nb_dq)) ? device_alias_of_pinned(dqpsk) : nullptr;
    if (reinterpret_cast<uintptr_t>(dq_alias) & 15) dq_alias = nullptr;
    const dabk::CopyPiece down[3] = {{soft_alias ? soft_alias : static_cast<void *>(hd), d_res, size_t(NB_FRAME_BITS)},
                                     {hd + off_fr, res + off_fr, off_st - off_fr},
                                     {dq_alias, d_dq, dq_alias ? nb_dq : 0}};
    TrackedCall k;
    k.states = st;
    k.d_iq = d_iq;
    k.stream_stride = nb_iq / sizeof(float2);
    k.n_streams = 1;
    k.n_samples = int64_t(nb_iq / sizeof(float2));
    k.fixed_start = 1;
    k.acquiring = acquiring ? 1 : 0;
    k.d_soft = reinterpret_cast<int8_t *>(res);
    k.d_cyc = d_cyc;
    k.d_dd4 = d_dd;
    k.d_dqpsk = d_dq;
    k.d_frames = reinterpret_cast<dabgpu_acquired_frame *>(res + off_fr);
    k.d_sync = reinterpret_cast<dabgpu_sync_result *>(res + off_sy);
    k.upload_from = iq_alias;
    k.upload_bytes = iq_alias ? nb_iq : 0;
    k.down = down;
    k.n_down = 3;
    k.state_out = reinterpret_cast<dabk::StreamState *>(hd + off_st);
    k.note_states = false;
    if ((rc = tracked_launches(ctx, k, c, s))) return rc;
    if (dqpsk && !dq_alias) {
        HIP_TRY(hipMemcpyAsync(dqpsk, d_dq, nb_dq, hipMemcpyDeviceToHost, s));           // (the constellation into any other memory:
        HIP_TRY(hipStreamSynchronize(s));                                                // a copy-engine transfer ends the usual way)
    } else {
        // one synchronisation: the word behind the landing area's payload (the area is at least nb_res + 64 bytes)
        // (the soft bits may have gone straight into the caller's buffer: the word is watched only when that buffer is coherent)
        if ((rc = wait_for_signal(s, SignalWord(ctx, hd), false, !soft_alias || known_coherent_host(soft, NB_FRAME_BITS)))) return rc;
    }
    ctx->ev_states_pending = false;
    const char *hb = static_cast<const char *>(ctx->h_bounce);
    if (!soft_alias) std::memcpy(soft, hb, NB_FRAME_BITS);
    dabgpu_acquired_frame fr;
    std::memcpy(&fr, hb + off_fr, sizeof(fr));
    std::memcpy(&result->sync, hb + off_sy, sizeof(result->sync));
    dabk::StreamState hs;
    std::memcpy(&hs, hb + off_st, sizeof(hs));
    result->flags = fr.flags;
    result->reserved = 0;
    stats_of(hs, &result->stats);
    return DABGPU_OK;
}

}  // extern "C"
