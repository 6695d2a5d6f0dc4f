// dabgpu_api.hip -- the C ABI of libdabgpu (include/dabgpu.h): version, parameters and reference tables, context and its
// device tables, staging, host memory, timing, sample format, stream state.  (Front end, synchronisation, acquisition,
// tracking: dabgpu_ofdm_api.hip; TII and CIR: dabgpu_measure_api.hip; channel decoder: dabgpu_decode_api.hip; ETI(NI):
// dabgpu_eti_api.hip; frame buffers: dabgpu_placement.hip; host-fed ring: dabgpu_pipeline.hip.)  No CPU fallback: without a
// gfx950 device dabgpu_create fails with DABGPU_ERR_NODEVICE and every compute entry point needs a context.
#include "dabgpu_ctx.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <utility>

using namespace dab;
using namespace dabapi;

namespace {

// allocations of dabgpu_host_alloc: coherent page-locked memory (known_coherent_host); process-wide, any thread
std::mutex g_host_mutex;
std::vector<std::pair<const char *, size_t>> g_host_ranges;

template <class T>
int upload(T **dst, const std::vector<T> &src) {
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(dst), src.size() * sizeof(T)));
    HIP_TRY(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return DABGPU_OK;
}

int build_device_code(DeviceCode &dc) {
    std::vector<uint16_t> pos;
    pos.reserve(dc.prof.n_punct);
    for (size_t i = 0; i < dc.prof.mask.size(); i++)
        if (dc.prof.mask[i]) pos.push_back(uint16_t(i));
    if (int(pos.size()) != dc.prof.n_punct) return DABGPU_ERR_PROFILE;
    int rc = DABGPU_OK;
    if (dabk::viterbi_fits(dc.prof.nsteps)) {                  // (only the wave-per-codeword kernels read this table)
        // ... and behind it, for codewords of 96 k + 6 steps, where each 96-step chunk's punctured bits begin (CodeTables)
        const int n_punct = dc.prof.n_punct, nsteps = dc.prof.nsteps;
        if (nsteps >= 102 && (nsteps - 6) % 96 == 0) {
            const int k = (nsteps - 6) / 96;
            pos.resize(size_t(dabk::code_chunk_table_offset(n_punct)), 0);
            for (int c = 0; c <= k; c++) {
                int below = 0;
                while (below < n_punct && int(pos[size_t(below)]) < 4 * 96 * c) below++;
                pos.push_back(uint16_t(below));
            }
            pos.push_back(uint16_t(n_punct));
        }
        if ((rc = upload(&dc.d_mother_pos, pos))) return rc;
    }
    std::vector<int32_t> pidx(dc.prof.mask.size(), -1);
    for (size_t i = 0, j = 0; i < dc.prof.mask.size(); i++)
        if (dc.prof.mask[i]) pidx[i] = int32_t(j++);
    if ((rc = upload(&dc.d_punct_idx, pidx))) return rc;
    {
        std::vector<int32_t> desc, tiles;
        dabk::build_lane_fused_tables(dc.prof.mask.data(), dc.prof.nsteps, desc, tiles);
        if ((rc = upload(&dc.d_fused_desc, desc))) return rc;
        if ((rc = upload(&dc.d_fused_tiles, tiles))) return rc;
    }
    return upload(&dc.d_prbs, dab::make_prbs_bytes((dc.prof.nsteps - 6 + 7) / 8));
}
// twiddles in both orders, the carrier maps, the wave kernel's register map
int build_front_end_tables(dabgpu_ctx *ctx) {
    int rc;
    std::vector<float2> tw(NB_FFT + 64 + 512);
    for (int m = 0; m < NB_FFT; m++) {
        const double a = -2.0 * M_PI * double(m) / double(NB_FFT);
        tw[m] = make_float2(float(std::cos(a)), float(std::sin(a)));
    }
    // ... and the same values again in the order the synchronisation's block FFT reads them (fft_common.hpp TWC8_OFF / TWC64_OFF)
    for (int r = 0; r < 8; r++) {
        for (int k = 0; k < 8; k++) tw[NB_FFT + r * 8 + k] = tw[32 * r * k];
        for (int k = 0; k < 64; k++) tw[NB_FFT + 64 + r * 64 + k] = tw[4 * r * k];
    }
    if ((rc = upload(&ctx->d_twiddle, tw))) return rc;
    const std::vector<int32_t> mapper = make_mapper();
    std::vector<uint16_t> bins(NB_CARRIERS);
    for (int n = 0; n < NB_CARRIERS; n++) bins[n] = uint16_t(carrier_bin(mapper[n]));
    if ((rc = upload(&ctx->d_bin_of_n, bins))) return rc;
    // wave kernel: lane v ends each symbol holding bins v + 64*m; carrier register j <-> m = j (j<12) or j+8;
    // lane 0 register 0 holds bin 768 instead of DC
    std::vector<int> n_of_bin(NB_FFT, -1);
    for (int n = 0; n < NB_CARRIERS; n++) n_of_bin[bins[n]] = n;
    // layout [12][64] dwords: dword (jj, v) = n(2jj, v) | n(2jj+1, v) << 16
    std::vector<uint16_t> nvj(24 * 64);
    bool ok = true;
    for (int j = 0; j < 24; j++)
        for (int v = 0; v < 64; v++) {
            int bin = v + 64 * (j < 12 ? j : j + 8);
            if (j == 0 && v == 0) bin = 768;
            if (n_of_bin[bin] < 0) ok = false;
            nvj[((j >> 1) * 64 + v) * 2 + (j & 1)] = uint16_t(n_of_bin[bin] < 0 ? 0 : n_of_bin[bin]);
        }
    if (!ok) return DABGPU_ERR_PROFILE;
    return upload(&ctx->d_n_of_vj, nvj);
}

// synchronisation tables: PRS quarter turns, the adjacent-carrier pair list and its spectrum
int build_sync_tables(dabgpu_ctx *ctx) {
    int rc;
    const std::vector<int8_t> qt = make_prs_quarter_turns();
    std::vector<uint16_t> pairs;
    for (int b = 0; b + 1 < NB_FFT; b++)
        if (qt[b] >= 0 && qt[b + 1] >= 0) pairs.push_back(uint16_t(b | (((qt[b + 1] - qt[b]) & 3) << 11)));
    ctx->n_sync_pairs = int(pairs.size());
    if ((rc = upload(&ctx->d_prs_qt, qt))) return rc;
    if ((rc = upload(&ctx->d_sync_pairs, pairs))) return rc;
    // spectrum of S[b] = j^s on the pair bins: a 2048-point radix-2 FFT in double on the host (once per context)
    std::vector<double> fr(NB_FFT, 0.0), fi(NB_FFT, 0.0);
    static const double SR[4] = {1, 0, -1, 0}, SI[4] = {0, 1, 0, -1};
    for (uint16_t pr : pairs) {
        int b = pr & 2047, rev = 0;
        for (int bit = 0; bit < 11; bit++) rev |= ((b >> bit) & 1) << (10 - bit);      // bit-reversed input order
        fr[rev] = SR[pr >> 11];
        fi[rev] = SI[pr >> 11];
    }
    for (int len = 2; len <= NB_FFT; len <<= 1) {
        const double ang = -2.0 * M_PI / double(len);
        for (int i = 0; i < NB_FFT; i += len)
            for (int j = 0; j < len / 2; j++) {
                const double wr = std::cos(ang * j), wi = std::sin(ang * j);
                const int p0 = i + j, p1 = i + j + len / 2;
                const double tr = fr[p1] * wr - fi[p1] * wi, ti = fr[p1] * wi + fi[p1] * wr;
                fr[p1] = fr[p0] - tr; fi[p1] = fi[p0] - ti;
                fr[p0] += tr; fi[p0] += ti;
            }
    }
    std::vector<float2> fs(NB_FFT);
    for (int m = 0; m < NB_FFT; m++) fs[m] = make_float2(float(fr[m]), float(fi[m]));
    return upload(&ctx->d_sync_fs, fs);
}

int build_fic_code(dabgpu_ctx *ctx) {
    ctx->fic.prof = make_fic_profile();
    if (ctx->fic.prof.nsteps != NB_FIC_STEPS || ctx->fic.prof.n_punct != NB_FIC_GROUP_BITS) return DABGPU_ERR_PROFILE;
    return build_device_code(ctx->fic);
}

// The Timer behind a caller's `which` (dabgpu.h numbers them) and, in *part, which stretch of it: -1 the whole call,
// 0 / 1 / 2 the forward pass | traceback | history copy of TIMER_MSC's grouped lane decode.  nullptr: no such number.
Timer *timer_of(dabgpu_ctx *ctx, int which, int *part) {
    *part = which >= WHICH_MSC_FORWARD && which <= WHICH_MSC_HISTORY ? which - WHICH_MSC_FORWARD : -1;
    if (which < 0 || which > WHICH_MOD_SYMBOLS) return nullptr;
    if (which == WHICH_MOD_ENCODE || which == WHICH_MOD_SYMBOLS) return &ctx->timers[which == WHICH_MOD_ENCODE ? TIMER_MOD_ENCODE : TIMER_MOD_SYMBOLS];
    return &ctx->timers[*part >= 0 ? TIMER_MSC : which == WHICH_ETI ? TIMER_ETI : which];
}
}  // namespace

namespace dabapi {

void free_device_code(DeviceCode &dc) {
    if (dc.d_mother_pos) (void)hipFree(dc.d_mother_pos);
    if (dc.d_prbs) (void)hipFree(dc.d_prbs);
    if (dc.d_punct_idx) (void)hipFree(dc.d_punct_idx);
    if (dc.d_fused_desc) (void)hipFree(dc.d_fused_desc);
    if (dc.d_fused_tiles) (void)hipFree(dc.d_fused_tiles);
    dc.d_fused_desc = dc.d_fused_tiles = nullptr;
    dc.d_punct_idx = nullptr;
    dc.d_mother_pos = nullptr;
    dc.d_prbs = nullptr;
}

int get_code(dabgpu_ctx *ctx, dab::PunctureProfile &&prof, DeviceCode **out) {
    auto it = ctx->codes.find(prof.mask);
    if (it == ctx->codes.end()) {
        auto dc = std::make_unique<DeviceCode>();
        dc->prof = std::move(prof);
        int rc = build_device_code(*dc);
        if (rc) { free_device_code(*dc); return rc; }
        it = ctx->codes.emplace(dc->prof.mask, std::move(dc)).first;
    }
    *out = it->second.get();
    return DABGPU_OK;
}

int stage(dabgpu_ctx *ctx, StageSlot slot, size_t bytes, void **out) {
    if (ctx->stage_bytes[slot] < bytes) {
        if (ctx->d_stage[slot]) (void)hipFree(ctx->d_stage[slot]);
        ctx->d_stage[slot] = nullptr;
        ctx->stage_bytes[slot] = 0;
        if (hipMalloc(&ctx->d_stage[slot], bytes) != hipSuccess) return DABGPU_ERR_NOMEM;
        ctx->stage_bytes[slot] = bytes;
    }
    *out = ctx->d_stage[slot];
    return DABGPU_OK;
}

bool known_coherent_host(const void *host, size_t bytes) {
    const char *p = static_cast<const char *>(host);
    std::lock_guard<std::mutex> lock(g_host_mutex);
    for (const auto &r : g_host_ranges)
        if (p >= r.first && p + bytes <= r.first + r.second) return true;
    return false;
}

int ensure_bounce(dabgpu_ctx *ctx, size_t bytes) {
    if (ctx->h_bounce_bytes >= bytes + 64) return DABGPU_OK;
    if (ctx->h_bounce) (void)hipHostFree(ctx->h_bounce);
    ctx->h_bounce = nullptr;
    ctx->h_bounce_bytes = 0;
    const size_t want = std::max<size_t>(bytes + 64, 256);
    if (hipHostMalloc(&ctx->h_bounce, want, hipHostMallocCoherent) != hipSuccess) {
        (void)hipGetLastError();
        ctx->h_bounce = nullptr;
        return DABGPU_ERR_NOMEM;
    }
    ctx->h_bounce_bytes = want;
    std::memset(ctx->h_bounce, 0, want);
    return DABGPU_OK;
}

void *device_alias_of_pinned(const void *host) {
    hipPointerAttribute_t at{};
    if (!host || hipPointerGetAttributes(&at, host) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return at.type == hipMemoryTypeHost ? at.devicePointer : nullptr;
}

// The stream states are read and written by launches on whatever stream the caller passed: remember the most recent
// one, so that the host-side accessors can wait for exactly that work.
int note_state_use(dabgpu_ctx *ctx, hipStream_t s) {
    if (!ctx->ev_states && hipEventCreateWithFlags(&ctx->ev_states, hipEventDisableTiming) != hipSuccess) return DABGPU_ERR_HIP;
    HIP_TRY(hipEventRecord(ctx->ev_states, s));
    ctx->ev_states_pending = true;
    return DABGPU_OK;
}
int wait_state_use(dabgpu_ctx *ctx) {
    if (ctx->ev_states_pending) {
        HIP_TRY(hipEventSynchronize(ctx->ev_states));
        ctx->ev_states_pending = false;
    }
    return DABGPU_OK;
}

void stats_of(const dabk::StreamState &st, dabgpu_stats *out) {
    // READING_SYMBOLS / FINDING_NULL_POWER_DIP (a tracked stream that lost every frame of a call is searching again)
    out->state = (st.total_frames_read > 0 && !(st.tracking == 0 && st.next_frame_start != 0.0)) ? 4 : 0;
    out->fine_freq_offset = st.fine_freq_offset;
    out->coarse_freq_offset = st.coarse_freq_offset;
    out->net_freq_offset = st.fine_freq_offset + st.coarse_freq_offset;
    out->signal_average = st.signal_average;
    out->total_frames_read = st.total_frames_read;
    out->total_frames_desync = st.total_frames_desync;
    out->last_fine_error = st.last_fine_error;
    out->tracking = st.tracking;
    out->last_time_offset = st.last_time_offset;
    out->next_frame_start = st.next_frame_start;
    out->drift = st.drift;
    out->last_peak_to_mean = st.last_peak_to_mean;
    out->loop_gated = st.loop_gated;
    out->reserved = 0;
}
}  // namespace dabapi

static_assert(sizeof(dabgpu_stream_state) == 64 && sizeof(dabk::StreamState) == 64, "stream state layout");
static_assert(offsetof(dabgpu_stream_state, next_frame_start) == offsetof(dabk::StreamState, next_frame_start) &&
              offsetof(dabgpu_stream_state, drift) == offsetof(dabk::StreamState, drift), "stream state layout");

extern "C" {

int dabgpu_abi_version(void) { return DABGPU_ABI_VERSION; }

const char *dabgpu_strerror(int status) {
    switch (status) {
    case DABGPU_OK: return "ok";
    case DABGPU_ERR_ARG: return "invalid argument";
    case DABGPU_ERR_HIP: return "HIP runtime error";
    case DABGPU_ERR_NOMEM: return "out of memory";
    case DABGPU_ERR_NODEVICE: return "no gfx950 device available (libdabgpu has no CPU fallback)";
    case DABGPU_ERR_PROFILE: return "unsupported transmission mode or protection profile";
    case DABGPU_ERR_CAPACITY: return "request exceeds context capacity";
    default: return "unknown status";
    }
}

int dabgpu_get_ofdm_params(int mode, dabgpu_ofdm_params *out) {
    if (!out) return DABGPU_ERR_ARG;
    if (mode != 1) return DABGPU_ERR_PROFILE;
    out->nb_frame_symbols = NB_FRAME_SYMBOLS;
    out->nb_symbol_period = NB_SYM_PERIOD;
    out->nb_null_period = NB_NULL_PERIOD;
    out->nb_fft = NB_FFT;
    out->nb_cyclic_prefix = NB_CP;
    out->nb_data_carriers = NB_CARRIERS;
    out->freq_carrier_spacing = 1000;
    out->nb_frame_samples = NB_FRAME_SAMPLES;
    return DABGPU_OK;
}

int dabgpu_get_dab_params(int mode, dabgpu_dab_params *out) {
    if (!out) return DABGPU_ERR_ARG;
    if (mode != 1) return DABGPU_ERR_PROFILE;
    out->nb_frame_bits = NB_FRAME_BITS;
    out->nb_symbols = NB_DATA_SYMBOLS;
    out->nb_fic_symbols = NB_FIC_SYMBOLS;
    out->nb_msc_symbols = NB_DATA_SYMBOLS - NB_FIC_SYMBOLS;
    out->nb_sym_bits = NB_SYM_BITS;
    out->nb_fic_bits = NB_FIC_BITS;
    out->nb_msc_bits = NB_FRAME_BITS - NB_FIC_BITS;
    out->nb_fibs = NB_FIBS;
    out->nb_cifs = NB_CIFS;
    out->nb_fib_bits = 256;
    out->nb_fib_cif_bits = NB_FIC_GROUP_BITS;
    out->nb_fibs_per_cif = NB_FIBS / NB_CIFS;
    out->nb_cif_bits = NB_CIF_BITS;
    return DABGPU_OK;
}

int dabgpu_get_prs_reference(int mode, float *out, int nb_fft) {
    if (!out || nb_fft != NB_FFT) return DABGPU_ERR_ARG;
    if (mode != 1) return DABGPU_ERR_PROFILE;
    static const float RE[4] = {1.f, 0.f, -1.f, 0.f}, IM[4] = {0.f, 1.f, 0.f, -1.f};
    const std::vector<int8_t> q = make_prs_quarter_turns();
    for (int b = 0; b < NB_FFT; b++) {
        out[2 * b] = q[b] < 0 ? 0.f : RE[q[b]];
        out[2 * b + 1] = q[b] < 0 ? 0.f : IM[q[b]];
    }
    return DABGPU_OK;
}

int dabgpu_get_mapper_reference(int32_t *out, int nb_data_carriers, int nb_fft) {
    if (!out || nb_data_carriers != NB_CARRIERS || nb_fft != NB_FFT) return DABGPU_ERR_ARG;
    const std::vector<int32_t> m = make_mapper();
    if (int(m.size()) != NB_CARRIERS) return DABGPU_ERR_PROFILE;
    std::memcpy(out, m.data(), sizeof(int32_t) * NB_CARRIERS);
    return DABGPU_OK;
}

int dabgpu_create(const dabgpu_cfg *cfg, dabgpu_ctx **out) {
    if (!cfg || !out) return DABGPU_ERR_ARG;
    *out = nullptr;
    if (cfg->transmission_mode != 1) return DABGPU_ERR_PROFILE;
    constexpr int KNOWN_FLAGS = DABGPU_FLAG_VITERBI_WAVE | DABGPU_FLAG_VITERBI_LANE | DABGPU_FLAG_LANE_UNFUSED | DABGPU_FLAG_TEST_ONE_DOMAIN;
    if ((cfg->flags & ~KNOWN_FLAGS) || ((cfg->flags & DABGPU_FLAG_VITERBI_WAVE) && (cfg->flags & DABGPU_FLAG_VITERBI_LANE)))
        return DABGPU_ERR_ARG;
    if (cfg->ofdm_symbol_runs < 0 || cfg->ofdm_symbol_runs > NB_DATA_SYMBOLS) return DABGPU_ERR_ARG;
    if (cfg->reserved[0] || cfg->reserved[1] || cfg->reserved[2]) return DABGPU_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return DABGPU_ERR_NODEVICE;
    if (cfg->device < 0 || cfg->device >= ndev) return DABGPU_ERR_ARG;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess) return DABGPU_ERR_HIP;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return DABGPU_ERR_NODEVICE;
    dabgpu_ctx *ctx = new (std::nothrow) dabgpu_ctx();
    if (!ctx) return DABGPU_ERR_NOMEM;
    ctx->device = cfg->device;
    DeviceGuard guard(ctx);
    ctx->max_frames = cfg->max_frames;
    ctx->ofdm_parts_override = cfg->ofdm_symbol_runs;
    ctx->lane_mode = (cfg->flags & DABGPU_FLAG_VITERBI_LANE) ? 1 : (cfg->flags & DABGPU_FLAG_VITERBI_WAVE) ? 0 : -1;
    ctx->lane_unfused = (cfg->flags & DABGPU_FLAG_LANE_UNFUSED) != 0;
    ctx->test_one_domain = (cfg->flags & DABGPU_FLAG_TEST_ONE_DOMAIN) != 0;
    ctx->wave_slots = prop.multiProcessorCount > 0 ? prop.multiProcessorCount * 12 : 3072;   // 3 workgroups x 4 waves per CU
    int rc = DABGPU_OK;
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) rc = DABGPU_ERR_HIP;
    if (!rc && (dabk::init_viterbi_kernel_attributes() != hipSuccess || dabk::init_lane_kernel_attributes() != hipSuccess))
        rc = DABGPU_ERR_HIP;
    if (!rc) rc = build_front_end_tables(ctx);
    if (!rc) rc = build_sync_tables(ctx);
    if (!rc) rc = build_fic_code(ctx);
    if (rc) { dabgpu_destroy(ctx); return rc; }
    *out = ctx;
    return DABGPU_OK;
}

void dabgpu_destroy(dabgpu_ctx *ctx) {
    if (!ctx) return;
    {
    DeviceGuard guard(ctx);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->d_states) (void)hipFree(ctx->d_states);
    ctx->sub_history.clear();
    if (ctx->h_bounce) (void)hipHostFree(ctx->h_bounce);
    if (ctx->d_twiddle) (void)hipFree(ctx->d_twiddle);
    if (ctx->d_bin_of_n) (void)hipFree(ctx->d_bin_of_n);
    if (ctx->d_n_of_vj) (void)hipFree(ctx->d_n_of_vj);
    for (auto &kv : ctx->run_queues) (void)hipFree(kv.second.d_pairs);
    if (ctx->d_prs_qt) (void)hipFree(ctx->d_prs_qt);
    if (ctx->d_sync_pairs) (void)hipFree(ctx->d_sync_pairs);
    if (ctx->d_sync_fs) (void)hipFree(ctx->d_sync_fs);
    free_device_code(ctx->fic);
    for (auto &kv : ctx->codes) free_device_code(*kv.second);
    for (void *p : ctx->d_stage) if (p) (void)hipFree(p);
    if (ctx->d_lane_scratch) (void)hipFree(ctx->d_lane_scratch);
    if (ctx->d_acq_scratch) (void)hipFree(ctx->d_acq_scratch);
    if (ctx->d_mod_tables) (void)hipFree(ctx->d_mod_tables);
    for (void *p : ctx->keep_tables) (void)hipFree(p);
    for (Timer &t : ctx->timers)
        for (int i = 0; i < TIMER_RING; i++) {
            if (t.start[i]) (void)hipEventDestroy(t.start[i]);
            if (t.stop[i]) (void)hipEventDestroy(t.stop[i]);
            for (hipEvent_t e : t.mid[i])
                if (e) (void)hipEventDestroy(e);
        }
    pipeline_destroy(ctx);
    arena_destroy(ctx);
    if (ctx->ev_states) (void)hipEventDestroy(ctx->ev_states);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    }
    delete ctx;
}

void *dabgpu_host_alloc(size_t bytes) {
    void *p = nullptr;
    if (bytes == 0) return nullptr;
    // coherent page-locked memory, asked for by name (the runtime's default can be switched by its environment)
    if (hipHostMalloc(&p, bytes, hipHostMallocCoherent) == hipSuccess) {
        std::lock_guard<std::mutex> lock(g_host_mutex);
        g_host_ranges.emplace_back(static_cast<const char *>(p), bytes);
        return p;
    }
    (void)hipGetLastError();
    // (not registered: the one-frame calls then end in a stream synchronisation instead of the watched word)
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}

void dabgpu_host_free(void *p) {
    if (!p) return;
    {
        std::lock_guard<std::mutex> lock(g_host_mutex);
        for (size_t i = 0; i < g_host_ranges.size(); i++)
            if (g_host_ranges[i].first == p) { g_host_ranges[i] = g_host_ranges.back(); g_host_ranges.pop_back(); break; }
    }
    (void)hipHostFree(p);
}

int dabgpu_test_fail_frame_call(dabgpu_ctx *ctx, int nth) {
    if (!ctx || nth < 0) return DABGPU_ERR_ARG;
    ctx->test_fail_in = nth;
    return DABGPU_OK;
}

int dabgpu_sync(dabgpu_ctx *ctx) {
    if (!ctx) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DABGPU_OK;
}

void *dabgpu_stream(dabgpu_ctx *ctx) { return ctx ? reinterpret_cast<void *>(ctx->stream) : nullptr; }

int dabgpu_set_timing(dabgpu_ctx *ctx, int enable) {
    if (!ctx) return DABGPU_ERR_ARG;
    ctx->timing = enable != 0;
    for (Timer &t : ctx->timers) t.recorded = 0;               // a new measurement starts
    return DABGPU_OK;
}

int dabgpu_last_kernel_ms(dabgpu_ctx *ctx, int which, float *ms) {
    if (!ctx || !ms) return DABGPU_ERR_ARG;
    int part;
    Timer *t = timer_of(ctx, which, &part);
    if (!t || part >= 0) return DABGPU_ERR_ARG;                 // (the parts are read as means only)
    DeviceGuard guard(ctx);
    if (t->recorded == 0) return DABGPU_ERR_ARG;
    const int i = int((t->recorded - 1) % TIMER_RING);
    HIP_TRY(hipEventSynchronize(t->stop[i]));
    HIP_TRY(hipEventElapsedTime(ms, t->start[i], t->stop[i]));
    return DABGPU_OK;
}

int dabgpu_mean_kernel_ms(dabgpu_ctx *ctx, int which, float *mean_ms, int *launches) {
    if (!ctx || !mean_ms) return DABGPU_ERR_ARG;
    int part;
    Timer *tp = timer_of(ctx, which, &part);
    if (!tp) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    Timer &t = *tp;
    const int n = int(std::min<long>(t.recorded, TIMER_RING));
    double sum = 0.0;
    int used = 0;
    for (int k = 0; k < n; k++) {
        const int i = int((t.recorded - 1 - k) % TIMER_RING);
        if (part >= 0 && !t.has_mid[i]) continue;
        float ms = 0.f;
        HIP_TRY(hipEventSynchronize(t.stop[i]));
        hipEvent_t a = part <= 0 ? t.start[i] : t.mid[i][part - 1], b = part < 0 || part == 2 ? t.stop[i] : t.mid[i][part];
        HIP_TRY(hipEventElapsedTime(&ms, a, b));
        sum += double(ms);
        used++;
    }
    if (used == 0) return DABGPU_ERR_ARG;
    *mean_ms = float(sum / used);
    if (launches) *launches = used;
    return DABGPU_OK;
}

// ---------------------------------------------------------------------------- sample formats
int dabgpu_set_iq_format(dabgpu_ctx *ctx, int format) {
    if (!ctx || !dabk::iq_format_valid(format)) return DABGPU_ERR_ARG;
    if (ctx->pipe) return DABGPU_ERR_ARG;                       // the ring's staging slots are sized for the format it opened with
    ctx->iq_format = format;
    return DABGPU_OK;
}

int dabgpu_get_iq_format(const dabgpu_ctx *ctx) { return ctx ? ctx->iq_format : DABGPU_ERR_ARG; }


int dabgpu_streams_reset(dabgpu_ctx *ctx, int n_streams) {
    if (!ctx || n_streams < 0) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    int wrc = wait_state_use(ctx);
    if (wrc) return wrc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (n_streams > ctx->n_states) {
        if (ctx->d_states) (void)hipFree(ctx->d_states);
        ctx->d_states = nullptr;
        ctx->n_states = 0;
        if (hipMalloc(reinterpret_cast<void **>(&ctx->d_states), sizeof(dabk::StreamState) * size_t(n_streams)) != hipSuccess)
            return DABGPU_ERR_NOMEM;
    }
    ctx->n_states = n_streams;
    if (n_streams > 0) HIP_TRY(hipMemset(ctx->d_states, 0, sizeof(dabk::StreamState) * size_t(n_streams)));
    return DABGPU_OK;
}

dabgpu_stream_state *dabgpu_stream_states(dabgpu_ctx *ctx) {
    return ctx ? reinterpret_cast<dabgpu_stream_state *>(ctx->d_states) : nullptr;
}

int dabgpu_set_stream_offsets(dabgpu_ctx *ctx, int stream_index, const float *fine, const float *coarse) {
    if (!ctx || stream_index < 0 || stream_index >= ctx->n_states) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    int wrc = wait_state_use(ctx);
    if (wrc) return wrc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    dabk::StreamState *st = ctx->d_states + stream_index;
    if (fine) HIP_TRY(hipMemcpy(&st->fine_freq_offset, fine, sizeof(float), hipMemcpyHostToDevice));
    if (coarse) HIP_TRY(hipMemcpy(&st->coarse_freq_offset, coarse, sizeof(float), hipMemcpyHostToDevice));
    // a re-seeded stream pulls in again: the decision-directed loop's gate forgets the branch it was holding
    const int32_t pulling_in[2] = {dabk::DD_NO_BRANCH, dabk::DD_NO_BRANCH};
    static_assert(offsetof(dabk::StreamState, dd_pending) == offsetof(dabk::StreamState, dd_branch) + 4, "branch, pending adjacent");
    if (fine || coarse) HIP_TRY(hipMemcpy(&st->dd_branch, pulling_in, sizeof(pulling_in), hipMemcpyHostToDevice));
    return DABGPU_OK;
}


int dabgpu_get_stats(dabgpu_ctx *ctx, int stream_index, dabgpu_stats *out) {
    if (!ctx || !out || stream_index < 0 || stream_index >= ctx->n_states) return DABGPU_ERR_ARG;
    DeviceGuard guard(ctx);
    int wrc = wait_state_use(ctx);
    if (wrc) return wrc;
    dabk::StreamState st;
    HIP_TRY(hipMemcpyAsync(&st, ctx->d_states + stream_index, sizeof(st), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    stats_of(st, out);
    return DABGPU_OK;
}

int dabgpu_set_stream_loop(dabgpu_ctx *ctx, float signal_update_beta, float thr_null_start, int decision_directed) {
    if (!ctx || !(signal_update_beta >= 0.f && signal_update_beta <= 1.f) || !(thr_null_start >= 0.f && thr_null_start <= 1.f))
        return DABGPU_ERR_ARG;
    ctx->signal_beta = signal_update_beta;
    ctx->thr_null_start = thr_null_start;
    ctx->loop_dd = decision_directed != 0;
    return DABGPU_OK;
}

int dabgpu_set_loop_gate(dabgpu_ctx *ctx, float dd_gate) {
    if (!ctx || !(dd_gate >= 0.f && dd_gate <= 1000.f)) return DABGPU_ERR_ARG;
    ctx->dd_gate = dd_gate;
    return DABGPU_OK;
}

}  // extern "C"
