// dabgpu_ctx.hpp -- the context behind the opaque dabgpu_ctx handle and the helpers the translation units of the C ABI
// share (dabgpu_api.hip: context, tables, timing, stream state; dabgpu_ofdm_api.hip: front end, synchronisation,
// acquisition, tracking; dabgpu_measure_api.hip: TII, CIR, reception quality; dabgpu_decode_api.hip: channel decoder;
// dabgpu_eti_api.hip: ETI(NI) output; dabgpu_pad_api.hip: dynamic labels; dabgpu_mod_api.hip: ETI(NI) to IQ; dabgpu_placement.hip: frame buffers;
// dabgpu_pipeline.hip: the host-fed ring; decode_plan.hpp: what the decoder's entry points share).  Internal to libdabgpu.
#pragma once
#include "../../include/dabgpu.h"

#include <hip/hip_runtime.h>

#include <chrono>
#include <map>
#include <memory>
#include <vector>

#include "dab_tables.hpp"
#include "kernels.hpp"
#include "iq_load.hpp"

namespace dabapi {

struct DeviceCode {
    dab::PunctureProfile prof;
    uint16_t *d_mother_pos = nullptr;
    uint8_t *d_prbs = nullptr;
    int32_t *d_punct_idx = nullptr;      // [4*nsteps] punctured index of each mother bit, -1 = erased (lane kernels)
    int32_t *d_fused_desc = nullptr, *d_fused_tiles = nullptr;   // fused lane forward pass (build_lane_fused_tables)
    dabk::LaneTables lane_tables() const { return dabk::LaneTables{d_punct_idx, d_fused_desc, d_fused_tiles}; }
    dabk::CodeTables tables(bool descramble) const {
        const bool chunked = d_mother_pos && prof.nsteps >= 102 && (prof.nsteps - 6) % 96 == 0;
        return dabk::CodeTables{d_mother_pos, prof.n_punct, prof.nsteps, descramble ? d_prbs : nullptr,
                                chunked ? d_mother_pos + dabk::code_chunk_table_offset(prof.n_punct) : nullptr};
    }
};

// hipEvent pairs around the most recent launches of one kernel family (a ring: the launches are asynchronous, so
// the pairs can only be read back after the stream has caught up)
constexpr int TIMER_RING = 32;
struct Timer {
    hipEvent_t start[TIMER_RING] = {}, stop[TIMER_RING] = {};
    // the grouped lane decode is two kernels (+ the history copy) inside one timed call: two more events split it into
    // forward pass | traceback | history (dabgpu_mean_kernel_ms 4 / 5 / 6 read TIMER_MSC through them)
    hipEvent_t mid[TIMER_RING][2] = {};
    bool has_mid[TIMER_RING] = {};
    long recorded = 0;                   // launches timed since timing was switched on
};

// ctx->timers, and what dabgpu_last_kernel_ms / dabgpu_mean_kernel_ms call them (dabgpu.h): the first four by their own
// numbers, the parts of TIMER_MSC's grouped lane decode as 4 / 5 / 6 (_mean_ only), the ETI launches as 7, the modulator's encoder (with its pre-pass) and symbol kernel as 8 / 9
enum TimerSlot { TIMER_OFDM = 0, TIMER_FIC = 1, TIMER_MSC = 2, TIMER_FFT = 3, TIMER_ETI = 4, TIMER_MOD_ENCODE = 5, TIMER_MOD_SYMBOLS = 6, TIMER_SLOTS };
enum { WHICH_MSC_FORWARD = 4, WHICH_MSC_TRACEBACK = 5, WHICH_MSC_HISTORY = 6, WHICH_ETI = 7, WHICH_MOD_ENCODE = 8, WHICH_MOD_SYMBOLS = 9 };

// ctx->d_stage.  The first six are shared by role across the host-pointer entry points (two buffers of one call never
// share one); the rest belong to one family of calls each.  One caller stream at a time per context (dabgpu.h, conventions).
enum StageSlot {
    STAGE_IQ = 0,           // samples going up
    STAGE_SOFT = 1,         // soft bits: the front end's result, the decoder's input (DAB+ / plain Viterbi: their input bytes;
                            // the one-frame call: its whole result block)
    STAGE_AUX = 2,          // one small item per frame: frequency offsets going up; CRC flags, super-frame status coming down
    STAGE_RESULT = 3,       // the call's result: correlations, sync results, FIBs, decoded bytes
    STAGE_WIDE = 4,         // the large optional buffer: constellation, spectra; de-interleaver history going up
    STAGE_HISTORY_OUT = 5,  // de-interleaver history coming down
    STAGE_LOOP = 6,         // the stream / tracked / frame calls' own loop input (correlations or decision-directed sums)
    STAGE_TII = 7,          // the TII calls' per-frame records
    STAGE_CIR = 8,          // the CIR calls'
    STAGE_ETI_COUNTS = 9,   // the ETI call's per-stream CIF counts
    STAGE_MOD_CODED = 10,   // the modulator's coded records, one per ETI frame
    STAGE_MOD_CUM = 11,     // ... and running quarter turns, one pair of bit planes per data symbol
    STAGE_ENSEMBLES = 12,   // dabgpu_decode_ensembles_dev: the entry table of the ragged grouped lane launch
    STAGE_DABPLUS = 13,     // dabgpu_dabplus_follow_dev: the entry table and the plans of the align / follow launches
    STAGE_PAD = 14,         // dabgpu_pad_labels_dev: the entry table
    STAGE_MOT = 15,         // dabgpu_mot_slides_dev: the entry table
    STAGE_MP2 = 16,         // dabgpu_mp2_follow_dev: the entry table and the plans of the rate / frame launches
    STAGE_MP2_AUDIO = 17,   // dabgpu_mp2_subbands_dev: the entry table
    STAGE_PACKET = 18,      // dabgpu_packet_slides_dev: the entry table and the scan records of the scan / walk launches
    STAGE_PACKET_FEC = 19,  // dabgpu_packet_fec_dev: the entry table, the marks, the accepted frames and their counts
    STAGE_PACKET_FEC_ERASURES = 20,  // dabgpu_packet_fec_erasures_dev: the same, and a word of suspect bits per window frame
    STAGE_PACKET_CAROUSEL = 21,      // dabgpu_packet_carousel_dev: the entry table, what it adds per entry, the scan records
    STAGE_PACKET_GROUPS = 22,        // dabgpu_packet_groups_dev: the scan's table, this call's table, the scan records
    STAGE_ETI_READ = 23,             // dabgpu_eti_read_dev: the entry table, the candidate bitmaps and the row lists
    STAGE_EDI = 24,                  // dabgpu_edi_frames_dev: per stream the CIF count of the pre-pass and the first sequence number
    STAGE_EDI_READ = 25,             // dabgpu_edi_read_dev: the entry table and the two bitmaps of every entry
    STAGE_PFT = 26,                  // dabgpu_pft_fragments_dev: the first Pseq of every stream
    STAGE_PFT_READ = 27,             // dabgpu_pft_read_dev: the entry table, the two bitmaps and the fill launch's arena of every entry
    STAGE_DMB = 28,                  // dabgpu_dmb_follow_dev: the entry table, the sync launch's words and packet starts of every entry
    STAGE_SLOTS
};

struct Pipeline;                         // dabgpu_pipeline.hip

// The {next, done} pairs of the front end's run queue (dabk::RunQueue), a ring per stream the context's front-end calls
// have been enqueued on: launches on one stream run in order, so a stream's launches may share its ring; launches on
// different streams may be in flight together and never share a pair.  A launch takes the ring's next pair.  Zeroed when
// the ring is made; every launch leaves its pair zeroed (the kernel's last wave), so no call clears anything.
constexpr int QUEUE_RING = 8;
constexpr int QUEUE_PAIR_STRIDE = 32;    // in 32-bit words: a pair per 128-byte line
struct QueueRing {
    unsigned *d_pairs = nullptr;
    unsigned launches = 0;
};

// The de-interleaver rings of the sub-channels a state-keeping call decodes (dabgpu_decode_stream_frames: one stream;
// dabgpu_pipe_submit: n_streams of them), kept on the device between calls and double-buffered: [n_streams][15][bits] a
// side.  A call acquires the ring of every sub-channel it lists, decodes from in() to out() and commits.  A ring that
// misses a call no longer continues its streams: commit drops it, and a later call starts that sub-channel from erasures
// (this also bounds the set over any number of reconfigurations).  A call that fails after its first acquire leaves
// rings that have missed this frame: its caller clears the set.
struct HistoryRings {
    struct Ring {
        int start_address, length, n_streams;
        int8_t *buf[2];
        int cur;
        bool live;                       // acquired by the current call
    };
    std::vector<Ring> rings;
    // the ring of (start, length, n_streams) from the call before, or a new one whose input side is erased on `s`: its
    // index for in() / out(), or DABGPU_ERR_* (< 0)
    int acquire(int start_address, int length, int n_streams, hipStream_t s) {
        int k = -1;
        for (size_t j = 0; j < rings.size(); j++)
            if (rings[j].start_address == start_address && rings[j].length == length && rings[j].n_streams == n_streams) k = int(j);
        if (k < 0) {
            Ring r{};
            r.start_address = start_address;
            r.length = length;
            r.n_streams = n_streams;
            const size_t bytes = size_t(n_streams) * 15 * size_t(length) * dab::CU_BITS;
            if (hipMalloc(reinterpret_cast<void **>(&r.buf[0]), bytes) != hipSuccess) return DABGPU_ERR_NOMEM;
            if (hipMalloc(reinterpret_cast<void **>(&r.buf[1]), bytes) != hipSuccess) { (void)hipFree(r.buf[0]); return DABGPU_ERR_NOMEM; }
            k = int(rings.size());
            rings.push_back(r);
            if (hipMemsetAsync(r.buf[0], 0, bytes, s) != hipSuccess) return DABGPU_ERR_HIP;
        }
        rings[size_t(k)].live = true;
        return k;
    }
    const int8_t *in(int k) const { return rings[size_t(k)].buf[rings[size_t(k)].cur]; }
    int8_t *out(int k) const { return rings[size_t(k)].buf[rings[size_t(k)].cur ^ 1]; }
    // the call went through: what it wrote is the next call's input; the rings it left out go
    // (`busy`: a stream whose work may still use them, waited for before the first one is freed)
    void commit(hipStream_t busy = nullptr) {
        size_t kept = 0;
        bool dropped = false;
        for (Ring &r : rings) {
            if (r.live) { r.live = false; r.cur ^= 1; rings[kept++] = r; continue; }
            if (busy && !dropped) (void)hipStreamSynchronize(busy);
            dropped = true;
            (void)hipFree(r.buf[0]);
            (void)hipFree(r.buf[1]);
        }
        rings.resize(kept);
    }
    void clear() {
        for (Ring &r : rings) { (void)hipFree(r.buf[0]); (void)hipFree(r.buf[1]); }
        rings.clear();
    }
};

// The domain-aware frame buffers of a context live inside TWO address ranges, both reserved by the first such allocation
// and given back by dabgpu_destroy only (dabgpu_placement.hip): `probe` is where physical chunks are mapped while their
// HBM domains are found, `pair` is where the pair handed to the caller is mapped.  (Two, not one: access rights are only
// ever set on a span that begins at the base of a reservation -- the one use of the virtual-memory API that was never
// seen to fail on this runtime.)
struct Arena {
    char *probe = nullptr, *pair = nullptr;
    size_t probe_bytes = 0, pair_bytes = 0;
    struct Piece {
        size_t off, bytes;               // offset inside `pair`, mapped bytes
        hipMemGenericAllocationHandle_t h;
    };
    std::vector<Piece> pieces;           // live mappings of the pair handed out (empty: the arena is idle)
    void *d_iq = nullptr, *d_soft = nullptr;
};

}  // namespace dabapi

struct dabgpu_ctx {
    int device = 0;
    int max_frames = 0;
    hipStream_t stream = nullptr;
    float2 *d_twiddle = nullptr;
    uint16_t *d_bin_of_n = nullptr;
    uint16_t *d_n_of_vj = nullptr;
    std::map<hipStream_t, dabapi::QueueRing> run_queues;   // front-end run queues, by stream (dabapi::QueueRing)
    int8_t *d_prs_qt = nullptr;
    uint16_t *d_sync_pairs = nullptr;
    int n_sync_pairs = 0;
    float2 *d_sync_fs = nullptr;         // FFT of the PRS's adjacent-carrier differential (coarse search by FFT)
    dabapi::DeviceCode fic;
    std::map<std::vector<uint8_t>, std::unique_ptr<dabapi::DeviceCode>> codes;   // keyed by puncture mask
    // ... and found again by the sub-channel's descriptor (form, profile, level, bit rate, size) without building the
    // 4 x (24 x bitrate + 6) flags of its puncture mask first: the plugin's per-frame decode call built it three times
    // per sub-channel (validation, grouping, code look-up), ~10 us of host time in front of and between its launches
    std::map<uint64_t, dabapi::DeviceCode *> code_by_descriptor;
    void *d_stage[dabapi::STAGE_SLOTS] = {};             // grown on demand (dabapi::stage), freed by dabgpu_destroy
    size_t stage_bytes[dabapi::STAGE_SLOTS] = {};
    bool timing = false;
    dabapi::Timer timers[dabapi::TIMER_SLOTS];
    int ofdm_parts_override = 0;
    const unsigned long long *d_keep = nullptr;          // current soft-bit selection table ([75][3] words) or nullptr
    std::vector<void *> keep_tables;                     // every table handed to a kernel so far (freed on destroy)
    void *d_acq_scratch = nullptr;       // block norms + candidates of dabgpu_acquire
    size_t acq_scratch_bytes = 0;
    void *d_lane_scratch = nullptr;      // work buffers of the codeword-per-lane Viterbi
    size_t lane_scratch_bytes = 0;
    int lane_mode = -1;                  // 1 = DABGPU_FLAG_VITERBI_LANE, 0 = DABGPU_FLAG_VITERBI_WAVE, -1 by batch size
    bool lane_unfused = false;           // DABGPU_FLAG_LANE_UNFUSED
    bool test_one_domain = false;        // DABGPU_FLAG_TEST_ONE_DOMAIN (dabgpu_placement.hip)
    int test_fail_in = 0;                // dabgpu_test_fail_frame_call: one-frame calls left until one reports DABGPU_ERR_HIP
    int wave_slots = 3072;               // resident OFDM wavefronts: 12 per CU
    std::vector<dabgpu_bit_range> keep_ranges;           // the current selection, merged, for the host-pointer copy-back
    dabk::StreamState *d_states = nullptr;               // per-stream tracking state (dabgpu_streams_reset)
    int n_states = 0;
    hipEvent_t ev_states = nullptr;      // recorded behind the last launch that reads or writes d_states, on ITS stream
    bool ev_states_pending = false;
    float thr_null_start = 0.35f;        // desync threshold of the stream call (null_l1_search.thresh_null_start)
    float signal_beta = 0.95f;           // signal_l1.update_beta of the stream call
    bool loop_dd = false;                // stream call without a correlation buffer: decision-directed fine loop
    float dd_gate = 2.5f;                // decision-directed loop: quality gate (dabgpu_set_loop_gate, dabk::dd_loop_error)
    int keep_symbols = 75;               // data symbols per frame the current selection demodulates (75: no selection)
    dabapi::HistoryRings sub_history;    // dabgpu_decode_stream_frames: the stream's sub-channels
    void *h_bounce = nullptr;            // page-locked landing area of that call's single download (+ 64 bytes: the
    size_t h_bounce_bytes = 0;           // word wait_for_signal watches sits behind the payload)
    unsigned long long signal_seq = 0;   // number of the last one-frame call that ended through wait_for_signal
    dabapi::Arena arena;                 // dabgpu_alloc_frame_buffers(DABGPU_PLACE_DOMAINS)
    dabapi::Pipeline *pipe = nullptr;    // dabgpu_pipe_open
    int iq_format = 0;                   // DABGPU_IQ_* of the samples the device-pointer calls read (dabgpu_set_iq_format)
    void *d_mod_tables = nullptr;        // dabgpu_modulate_eti_dev: PRBS bytes, bin -> data index, the TII null symbol (made on first use)
    int mod_tii_main = -2, mod_tii_sub = -2;             // the transmitter whose null symbol the table holds
};

namespace dabapi {

// Makes the context's device current for the duration of an entry point and restores the caller's afterwards:
// allocations, copies and launches of a context must never land on whatever device the calling thread last used.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(const dabgpu_ctx *ctx) {
        if (ctx && hipGetDevice(&prev) == hipSuccess && prev != ctx->device) switched = hipSetDevice(ctx->device) == hipSuccess;
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

#define HIP_TRY(expr)                               \
    do {                                            \
        hipError_t e_ = (expr);                     \
        if (e_ != hipSuccess) return DABGPU_ERR_HIP; \
    } while (0)

struct ScopedTimer {
    dabgpu_ctx *ctx;
    int which;
    hipStream_t s;
    ScopedTimer(dabgpu_ctx *c, int w, hipStream_t st) : ctx(c), which(w), s(st) {
        if (ctx->timing) {
            Timer &t = ctx->timers[which];
            const int i = int(t.recorded % TIMER_RING);
            if (!t.start[i]) { (void)hipEventCreate(&t.start[i]); (void)hipEventCreate(&t.stop[i]); }
            t.has_mid[i] = false;
            (void)hipEventRecord(t.start[i], s);
        }
    }
    // the two events a launch sequence may record between its kernels (nullptr while timing is off); when it has recorded
    // both it says so with mids_recorded(): only then does this call count for the timer's parts
    hipEvent_t *mids() {
        if (!ctx->timing) return nullptr;
        Timer &t = ctx->timers[which];
        for (hipEvent_t &e : t.mid[int(t.recorded % TIMER_RING)])
            if (!e && hipEventCreate(&e) != hipSuccess) return nullptr;
        return t.mid[int(t.recorded % TIMER_RING)];
    }
    void mids_recorded() { ctx->timers[which].has_mid[int(ctx->timers[which].recorded % TIMER_RING)] = true; }
    ~ScopedTimer() {
        if (ctx->timing) {
            Timer &t = ctx->timers[which];
            (void)hipEventRecord(t.stop[int(t.recorded % TIMER_RING)], s);
            t.recorded++;
        }
    }
};

// The end of a one-frame call (dabgpu_ofdm_demod_stream_frame, dabgpu_decode_stream_frames): ~55 us of device work are in
// flight and the caller can do nothing until they are done.  hipStreamSynchronize puts the thread to sleep and pays the
// wake-up; instead a one-thread launch behind the call's last kernel stores the call's number into a word of the page-locked
// landing area and the host watches that word -- for at most SIGNAL_SPIN_US (no frame call takes that long on an idle
// device; a core is never held longer), then it sleeps on the stream after all.
// `w`: the two addresses of the word and this call's number.
// (already_signalled: the last kernel of the call stores the word itself -- a single-workgroup launch can)
// results_coherent: the kernels of these calls write their results straight into page-locked HOST memory, and
// a watched word orders nothing for memory the device does not write coherently: HIP guarantees host visibility of kernel
// writes to hipHostRegister'ed or non-coherent allocations only at a stream / event synchronisation.  The word is watched
// only when every such buffer is KNOWN to be coherent -- the context's own landing area and buffers from dabgpu_host_alloc
// (known_coherent_host) -- and the call ends in hipStreamSynchronize otherwise.
constexpr long SIGNAL_SPIN_US = 200;
// the watched word: the last 64 bytes of the landing area (ensure_bounce first), and the number of the call that takes it.
// `h_dev`: the address the device reaches ctx->h_bounce under.
struct SignalWord {
    volatile unsigned long long *host;
    unsigned long long *dev;
    unsigned long long seq;
    SignalWord(dabgpu_ctx *ctx, void *h_dev)
        : host(reinterpret_cast<volatile unsigned long long *>(static_cast<char *>(ctx->h_bounce) + ctx->h_bounce_bytes - 64)),
          dev(reinterpret_cast<unsigned long long *>(static_cast<char *>(h_dev) + ctx->h_bounce_bytes - 64)), seq(++ctx->signal_seq) {}
};
inline int wait_for_signal(hipStream_t s, const SignalWord &w, bool already_signalled = false, bool results_coherent = true) {
    if (!results_coherent) return hipStreamSynchronize(s) == hipSuccess ? DABGPU_OK : DABGPU_ERR_HIP;
    if (!already_signalled && dabk::launch_signal(w.dev, w.seq, s) != hipSuccess) return DABGPU_ERR_HIP;
    const auto give_up = std::chrono::steady_clock::now() + std::chrono::microseconds(SIGNAL_SPIN_US);
    for (;;) {
        for (int i = 0; i < 64; i++) {
            if (*w.host == w.seq) {
                __atomic_thread_fence(__ATOMIC_ACQUIRE);
                return DABGPU_OK;
            }
#if defined(__x86_64__) || defined(__i386__)
            __builtin_ia32_pause();
#endif
        }
        if (std::chrono::steady_clock::now() >= give_up) break;
    }
    return hipStreamSynchronize(s) == hipSuccess ? DABGPU_OK : DABGPU_ERR_HIP;
}

// dabgpu_test_fail_frame_call: true exactly once, on the armed one-frame call
inline bool injected_failure(dabgpu_ctx *ctx) {
    return ctx->test_fail_in > 0 && --ctx->test_fail_in == 0;
}

inline hipStream_t pick_stream(dabgpu_ctx *ctx, void *stream) {
    return stream ? reinterpret_cast<hipStream_t>(stream) : ctx->stream;
}

// the calls that read cf32 only (host-pointer calls, the FFT stage, the mover, a constellation output)
inline bool cf32_only(const dabgpu_ctx *ctx) { return ctx->iq_format != dabk::IQ_CF32; }
// a device IQ pointer must hold one complex sample of the context's format at its alignment
inline bool iq_misaligned(const dabgpu_ctx *ctx, const void *d_iq) {
    return (reinterpret_cast<uintptr_t>(d_iq) & (dabk::iq_sample_bytes(ctx->iq_format) - 1)) != 0;
}

// defined in dabgpu_api.hip
// the slot, grown to at least `bytes` (what it held is gone when it grows)
int stage(dabgpu_ctx *ctx, StageSlot slot, size_t bytes, void **out);
int get_code(dabgpu_ctx *ctx, dab::PunctureProfile &&prof, DeviceCode **out);
void free_device_code(DeviceCode &dc);
// the address the device reaches page-locked host memory under (hipHostMalloc / hipHostRegister: dabgpu_host_alloc), or
// nullptr for any other pointer
void *device_alias_of_pinned(const void *host);
// [host, host + bytes) lies inside one allocation of dabgpu_host_alloc (coherent page-locked memory: a kernel's writes to it
// are visible to a host that watched a word the kernel stored afterwards)
bool known_coherent_host(const void *host, size_t bytes);
// the context's page-locked landing area (coherent), at least `bytes` + the 64 bytes of the watched word, zeroed when (re)allocated
int ensure_bounce(dabgpu_ctx *ctx, size_t bytes);
int note_state_use(dabgpu_ctx *ctx, hipStream_t s);
int wait_state_use(dabgpu_ctx *ctx);
void stats_of(const dabk::StreamState &st, dabgpu_stats *out);
// defined in dabgpu_placement.hip / dabgpu_pipeline.hip: what dabgpu_destroy calls
void arena_destroy(dabgpu_ctx *ctx);
void pipeline_destroy(dabgpu_ctx *ctx);

// The transfers of a host-pointer entry point through the staging slots, on the context's stream: the call asks for
// every slot it uses (room), fills the ones that carry input (up), runs its device-pointer twin on ctx->stream, copies
// the results back (down) and waits (finish).  A slot's size is stated once, to room().  The first failure stays in `rc`
// and turns every later step into a no-op, as the early return it stands for would.
struct HostCall {
    dabgpu_ctx *ctx;
    int rc = DABGPU_OK;
    size_t bytes[STAGE_LOOP] = {};                             // of the six shared slots, where this call asked for them
    explicit HostCall(dabgpu_ctx *c) : ctx(c) {}
    // (`wanted` = false: an optional buffer the caller did not pass takes no slot and stays nullptr)
    void *room(StageSlot slot, size_t n, bool wanted = true) {
        void *d = nullptr;
        if (wanted && !rc && !(rc = stage(ctx, slot, n, &d))) bytes[slot] = n;
        return d;
    }
    void up(StageSlot slot, const void *host) { copy(ctx->d_stage[slot], host, slot, hipMemcpyHostToDevice); }
    void down(StageSlot slot, void *host) { copy(host, ctx->d_stage[slot], slot, hipMemcpyDeviceToHost); }
    int finish() {
        if (!rc && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = DABGPU_ERR_HIP;
        return rc;
    }
    // (a null host pointer or a slot this call did not ask for: nothing to copy)
    void copy(void *dst, const void *src, StageSlot slot, hipMemcpyKind kind) {
        if (rc || !dst || !src || !bytes[slot]) return;
        if (hipMemcpyAsync(dst, src, bytes[slot], kind, ctx->stream) != hipSuccess) rc = DABGPU_ERR_HIP;
    }
};

// The device table of an entry-table call -- the `_dev` calls that take a list of entries, check all of it, build the kernels'
// table on the host and launch over it -- in the staging slot of its family, at least `bytes` long, for launches on `s`.
// stage() frees a slot that has to grow, and growing the table must not race with a launch that still reads the old one: a
// slot that is too small waits for `s` first (one caller stream at a time per context: dabgpu.h, conventions).
struct DeviceTable {
    void *d = nullptr;
    size_t bytes = 0;                    // the slot's size: what a launch may use behind its own tables
};
inline int stage_table(dabgpu_ctx *ctx, StageSlot slot, size_t bytes, hipStream_t s, DeviceTable *out) {
    if (ctx->stage_bytes[slot] < bytes) HIP_TRY(hipStreamSynchronize(s));
    const int rc = stage(ctx, slot, bytes, &out->d);
    out->bytes = ctx->stage_bytes[slot];
    return rc;
}
// ... and the end of such a call, behind its checks (argument errors, no entries, DABGPU_ERR_CAPACITY: nothing before here
// touches HIP): the context's device, the caller's stream, the table, then launch(d_table, slot_bytes, s) -> hipError_t.
template <class Launch> int launch_entry_table(dabgpu_ctx *ctx, StageSlot slot, size_t bytes, void *stream, Launch launch) {
    DeviceGuard guard(ctx);
    hipStream_t s = pick_stream(ctx, stream);
    DeviceTable t;
    const int rc = stage_table(ctx, slot, bytes, s, &t);
    if (rc) return rc;
    HIP_TRY(launch(t.d, t.bytes, s));
    return DABGPU_OK;
}

// what every *_check compares: an address as a number, and whether [a, a + a_bytes) and [b, b + b_bytes) share a byte
inline uint64_t addr(const void *p) { return uint64_t(reinterpret_cast<uintptr_t>(p)); }
inline bool overlaps(const void *a, uint64_t a_bytes, const void *b, uint64_t b_bytes) {
    return addr(a) < addr(b) + b_bytes && addr(b) < addr(a) + a_bytes;
}

// No capacity unit of the CIF used twice (and none outside it): the state-keeping entry points (dabgpu_decode_stream_frames,
// dabgpu_pipe_submit) key their de-interleaver rings by (start, size), so a sub-channel listed twice would share one ring --
// both entries reading and writing the same pair of buffers, the ring flipped twice -- and the NEXT call would continue from
// a stale buffer.  Checked before any ring is touched: a refused call leaves the kept state as it was.
inline bool subchannels_disjoint(const dabgpu_subchannel *sc, int n) {
    char used[864] = {};
    for (int i = 0; i < n; i++) {
        if (sc[i].start_address < 0 || sc[i].length <= 0 || sc[i].start_address + sc[i].length > 864) return false;
        for (int cu = sc[i].start_address; cu < sc[i].start_address + sc[i].length; cu++) {
            if (used[cu]) return false;
            used[cu] = 1;
        }
    }
    return true;
}

// The codeword-per-lane Viterbi pays once a launch has enough codewords to give every SIMD a wave (one wave =
// 64 codewords; its single-wave latency equals the wave-per-codeword kernels' time at ~24k codewords).
constexpr int LANE_MIN_CODEWORDS = 24576;

}  // namespace dabapi
