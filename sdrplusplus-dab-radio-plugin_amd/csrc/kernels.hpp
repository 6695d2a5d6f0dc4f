// kernels.hpp -- launch interfaces of the hand-written gfx950 kernels (internal to libdabgpu).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>
#include <cstddef>
#include <cstdint>

#include "wave_plan.hpp"

namespace dabk {

// ---- OFDM front end (ofdm_kernels.hip) -------------------------------------
struct OfdmTables {
    const float2 *twiddle;     // [2048] exp(-2*pi*i*m/2048)
    const uint16_t *bin_of_n;  // [1536] FFT bin of data index n (mapper folded with carrier->bin)
    const uint16_t *n_of_vj;   // [12][64][2] data index of carrier registers 2jj, 2jj+1 of lane v (wave kernel)
};

// The run queue of ONE front-end launch.  A launch has at most wave_slots / 4 workgroups, all resident; each wave starts on
// the item of its own number and takes every further one from pair[0]; pair[1] counts the waves that have left, and the
// last one zeroes both words again.  `pair` must be zero when the launch starts, and no other launch that may run at the
// same time may be given the same pair.
struct RunQueue {
    unsigned *pair;
    int wave_slots;            // wavefronts of this kernel the device holds at once (12 per CU)
};

// Per-stream tracking state kept in device memory between launches (== dabgpu_stream_state, 64 bytes): the
// frequency offsets OFDM_Demod shows through GetFineFrequencyOffset / GetCoarseFrequencyOffset
// (/root/reference/src/render_radio_block.cpp:202-207), its frame counters, and -- what RUNNING_FINE_TIME_SYNC
// maintains frame by frame (:196) -- where the stream's next frame starts.
struct StreamState {
    float fine_freq_offset;    // cycles/sample, within +-0.5 carrier
    float coarse_freq_offset;  // cycles/sample, whole carriers
    float signal_average;      // mean |re|+|im| of the stream's most recent frame
    float last_fine_error;     // residual the most recent update measured, cycles/sample
    int32_t total_frames_read;
    int32_t total_frames_desync;
    int32_t tracking;          // 1: next_frame_start is valid (set by track_start, cleared when every frame of a call is lost)
    int32_t last_time_offset;  // impulse-response peak position of the most recent frame relative to its predicted one, samples
    double next_frame_start;   // first sample (PRS prefix minus margin) of the next frame, relative to the NEXT capture
    float drift;               // samples per frame by which the frame period differs from 196608
    float last_peak_to_mean;
    // decision-directed fine loop (dd_loop_error below)
    int32_t loop_gated;        // calls whose fourth-power estimate was not used as it came (quality gate, branch hold)
    int32_t dd_branch;         // branch k of the most recent accepted estimate (residual = e_dd + k / (4 2552))
    int32_t dd_pending;        // a one-step departure from branch 0 seen once (DD_NO_BRANCH: none)
    int32_t reserved;
};

struct OfdmArgs {
    const float2 *iq;          // frame f at iq + f*frame_stride (first PRS sample)
    size_t frame_stride;       // complex samples
    const float *freq_offset;  // [n_frames] or nullptr
    int n_frames;
    int8_t *soft;              // [n_frames][230400]
    float2 *cyc;               // [n_frames][76] or nullptr
    // decision-directed frequency error (no cyclic prefix is read): [n_frames][76]; the sum of a frame's entries 1..75 =
    // sum over its data symbols and a fixed subset of 256 carriers (the ones nearest the centre) of (X_l conj X_{l-1})^4 (a run's total in the entry
    // of its last symbol, zeros in its others); entry 0 is never written.  Ignored when cyc is set.
    float2 *dd4 = nullptr;
    float2 *dqpsk;             // [n_frames][75][1536] or nullptr
    float2 *spectra;           // FFT-only mode: [n_frames][76][2048]
    // acquired mode (acq != nullptr): frame f belongs to stream f / acq_per_stream, which starts at
    // iq + stream*frame_stride; its first sample and frequency correction come from acq[f]; frames whose
    // flags are not 3 produce all-zero (erased) soft bits
    const struct AcquiredFrame *acq = nullptr;
    int acq_per_stream = 1;
    // soft-bit selection: [75][3] words, bit k of symbol s = write its 16-byte chunk k; nullptr = write everything
    const unsigned long long *keep = nullptr;
    // stream mode (state != nullptr): frame f belongs to stream f / frames_per_stream and is corrected by that
    // stream's fine + coarse offset; freq_offset is ignored
    const StreamState *state = nullptr;
    int frames_per_stream = 0;
    // the first `uncut_frames` frames of the launch are ONE run each (no symbol is transformed twice); only the frames
    // behind them -- the ones that would otherwise leave most of the chip idle at the end of the launch -- are cut
    // into `parts` runs
    int uncut_frames = 0;
};

// fused A2..A6.  Frames behind the first a.uncut_frames are cut into `parts` contiguous runs of data symbols (1..75);
// a run re-reads the symbol before it as differential reference.
//
// iq_format (IQ_*, iq_load.hpp; every launcher that reads samples takes it): a.iq / the iq pointers then hold the caller's
// integer samples; strides and starts stay in complex samples.  The integer formats take the fused kernel without a
// constellation output only, and the tracking pass in batch mode without a riding upload (hipErrorInvalidValue otherwise).
hipError_t launch_ofdm_demod(const OfdmTables &t, const OfdmArgs &a, int parts, const RunQueue &q, hipStream_t s, int iq_format = 0);
// A2+A3 only; parts in 1..76.
hipError_t launch_fft_symbols(const OfdmTables &t, const OfdmArgs &a, int parts, const RunQueue &q, hipStream_t s);
// Fine-frequency loop and counters of the stream call, after the demodulation launch on the same stream:
// per stream, fine -= beta * mean(arg cyc[frame][symbol]) / (2*pi*2048), wrapped to +-half a carrier; frame count;
// L1 level of the stream's last frame (first 4096 samples) into the running average, counted as a desync when it
// is below thr_null_start times the average so far.
// noise-like floats in [0.5, 1) with random signs: timing probes must not run on zeros (they move ~6 % faster)
hipError_t launch_fill_noise(void *p, size_t bytes, hipStream_t s);
// Copies done by a kernel instead of the copy engine, for page-locked host memory the device can address: behind (or in
// front of) the kernels of a one-frame call such a copy starts at once, where an engine copy costs ~8 us of hand-over on
// either side.  Up to three pieces per launch; sizes multiples of 16, pointers 16-byte aligned (hipErrorInvalidValue
// otherwise); a piece of 0 bytes is skipped.
struct CopyPiece {
    void *dst;
    const void *src;
    size_t bytes;
};
hipError_t launch_copy_pieces(const CopyPiece *pieces, int n, hipStream_t s);   // n <= copy_pieces_max()
// one thread stores `value` to `flag` (page-locked host memory, through its device alias): enqueued behind a call's last
// launch it tells a host that is watching the word that everything before it on the stream is done and visible
hipError_t launch_signal(unsigned long long *flag, unsigned long long value, hipStream_t s);
int copy_pieces_max();
// reads `in` and writes `out` at the same time (streaming, both whole): the launch is slower when the two buffers
// share an HBM domain -- what the placement helpers time
hipError_t launch_placement_probe(const void *in, size_t in_bytes, void *out, size_t out_bytes, hipStream_t s);
// the fused front end's loads and stores without its arithmetic, same grid, queue, run structure and occupancy (dabgpu_mover_frames_dev)
hipError_t launch_geometry_mover(const float2 *iq, size_t frame_stride, int n_frames, int8_t *soft, int uncut_frames, int parts,
                                 bool prefixes, const RunQueue &q, hipStream_t s);
// dd != 0: `cyc` holds the front end's dd4 output instead; the error is angle(-sum of all entries l >= 1) / (4 * 2 pi * 2552)
// (dd_gate, dd_terms_per_frame: see dd_loop_error / TrackUpdateArgs)
hipError_t launch_stream_update(StreamState *state, const float2 *cyc, const float2 *iq, size_t frame_stride,
                                int n_streams, int frames_per_stream, float beta, float thr_null_start, float signal_beta,
                                int dd, float dd_gate, int dd_terms_per_frame, hipStream_t s, int iq_format = 0);

// ---- synchronisation on the PRS (sync_kernels.hip) -----------------------------
struct SyncTables {
    const float2 *twiddle;     // [2048 + 576]: natural order, then the block FFT's compact tables (fft_common.hpp TW_TOTAL)
    const int8_t *prs_qt;      // [2048] quarter turns of the PRS per bin, -1 = not a carrier
    const uint16_t *pairs;     // [n_pairs] adjacent carrier pairs: bin | ((qt[bin+1]-qt[bin])&3) << 11
    int n_pairs;
    const float2 *pair_spectrum;   // [2048] FFT of S[b] = R[b+1] conj R[b] on carrier pairs (0 elsewhere): coarse search by FFT
};
struct SyncResult {            // == dabgpu_sync_result
    int32_t coarse_carriers;
    int32_t time_offset;
    float peak_to_mean;
    float coarse_peak_to_mean;
};
hipError_t launch_prs_sync(const SyncTables &t, const float2 *iq, size_t frame_stride, int n_frames,
                           const float *freq_offset, int max_coarse, SyncResult *out, hipStream_t s, int iq_format = 0);

// Which tap of the channel impulse response a frame is aligned to (impulse_peak_distance_probability,
// /root/reference/src/render_radio_block.cpp:225):
//   score[n] = |h[n]|^2 * w(n)^2,  w(n) = 1 - (1 - distance_prob) * |t(n) - expected| / 2552,  t(n) the signed offset
//   peak = first maximum of the score;  peak_to_mean uses the unweighted |h[peak]|^2
//   first_path_rel > 0: the earliest tap within a cyclic prefix (504 samples) before the peak whose power is at least
//   max(first_path_rel * |h[peak]|^2, 16 * mean) replaces it -- the window is aligned to the first significant
//   path, so that a stronger late echo still falls inside the prefix.  0 = the reference's rule (weighted maximum).
struct PeakRule {
    float distance_prob = 1.0f;
    int expected = 0;
    float first_path_rel = 0.0f;
};

// ---- acquisition on unaligned captures (sync_kernels.hip) ----------------------
struct AcquiredFrame {         // == dabgpu_acquired_frame (32 bytes)
    int64_t start;             // first sample the demodulator treats as PRS cyclic prefix, relative to the stream
    float freq_offset;         // fine_offset - coarse_carriers/2048: what the demodulator applies
    int32_t coarse_carriers;
    float fine_offset;
    float peak_to_mean;
    float coarse_peak_to_mean;
    int32_t flags;             // bit 0 locked, bit 1 whole frame inside the capture
};
struct AcquireArgs {
    const float2 *iq;          // stream s at iq + s*stream_stride
    size_t stream_stride;      // complex samples
    int n_streams;
    int64_t n_samples;         // per stream
    float thr_start, thr_end;  // null-symbol dip thresholds relative to the (local) mean block L1
    int level_chunk;           // blocks per chunk of the local level estimate (power of two, 64..16384); 0 = capture mean
    const double *chunk_mean;  // scratch [n_streams][ceil(nb / level_chunk)], set by launch_acquire
    int min_blocks;            // shortest dip (64-sample blocks) accepted as a null symbol
    int max_coarse;            // carriers
    float min_peak_to_mean;
    int margin;                // samples the FFT windows are kept inside the cyclic prefix
    PeakRule rule;
    int max_out;               // frames per stream
    float *l1;                 // scratch [n_streams][n_samples/64]
    int64_t *cands;            // scratch [n_streams][max_out]
    AcquiredFrame *out;        // [n_streams][max_out]; entries >= counts[s] get flags 0, start -1
    int32_t *counts;           // [n_streams]
    // auto-acquisition inside a tracked call: streams whose state says tracking == 1 are left alone entirely (nothing
    // read, nothing written -- their rows of `out` and `counts` belong to the tracking pass)
    const StreamState *skip_tracked = nullptr;
};
size_t acquire_scratch_bytes(int n_streams, int64_t n_samples, int max_out);
hipError_t launch_acquire(const SyncTables &t, const AcquireArgs &a, hipStream_t s, int iq_format = 0);

// ---- per-stream timing tracking (sync_kernels.hip) -------------------------------
// Batch mode (fixed_start = 0): frame slot i of stream s is predicted from the stream's state at
//   p_i = next_frame_start + (j0 + i) * (196608 + drift),  j0 = frames that would start before the capture (missed),
// synchronised on its PRS at llrint(p_i) (impulse response with the state's net frequency offset applied, PeakRule)
// and written as an AcquiredFrame for the demodulator; slots whose frame (+512 samples) does not fit the capture, and
// every slot of a stream that is not tracking, get flags 0 / start -1.
// Frame mode (fixed_start = 1; the host mirror's one frame per call): the frame is the stream's first 76*2552 samples
// as the host assembled it (max_out = 1, start stays 0); max_coarse > 0 also runs the whole-carrier search:
// acquiring != 0 SETS the state's coarse offset from it (the search then runs with the fine offset alone), otherwise a
// residual of k carriers moves it by coarse_slow_beta * k; bit 1 of flags = the window lies inside the prefix
// (0 <= time offset <= 488).
struct TrackArgs {
    StreamState *state;
    const float2 *iq;          // stream s at iq + s*stream_stride
    size_t stream_stride;
    int n_streams;
    int64_t n_samples;
    int max_out;
    int margin;
    float min_peak_to_mean;
    PeakRule rule;             // expected is set to `margin` by the launcher
    int fixed_start;
    int max_coarse;
    int acquiring;
    float coarse_slow_beta;
    AcquiredFrame *out;        // [n_streams][max_out]
    SyncResult *sync_out;      // [n_streams][max_out] or nullptr
    // an upload riding in the same launch (the one-frame call): extra workgroups copy copy_n16 16-byte words from copy_src
    // (page-locked host memory) to copy_dst while the first ones synchronise on `sync_iq` -- the PRS read straight from
    // the host buffer -- so the 20 us of the synchronisation disappear inside the 37 us of the upload without a second
    // stream (a cross-stream event costs ~11 us on this runtime: profiles/r05_frame_path.md)
    const float2 *sync_iq = nullptr;     // where the synchronisation reads its samples (nullptr: `iq`)
    uint4 *copy_dst = nullptr;
    const uint4 *copy_src = nullptr;
    unsigned copy_n16 = 0;
    int copy_blocks = 0;                 // set by the launcher
};
hipError_t launch_track_sync(const SyncTables &t, const TrackArgs &a, hipStream_t s, int iq_format = 0);

// After the demodulation of those frames, one workgroup per stream:
//   fine loop   fine -= beta * mean(arg cyc) / (2 pi 2048) over the locked frames, wrapped to +-half a carrier
//   timing      residuals r_i = start_i - p_i of the n locked frames; with n >= 2 a least-squares line
//               r = alpha + slope*i, drift += drift_beta * min(1, n/4) * slope; with n = 1: alpha = r, slope = 0 and
//               (one slot per call only) drift += drift_beta/8 * r;
//               next_frame_start = p(count) + alpha + slope*count - advance
//               (count = frame slots inside the capture, p(count) with the OLD drift)
//   counters    total_frames_read += locked, total_frames_desync += missed + unlocked; no locked frame at all in a
//               call that had frames: tracking = 0
//   level       L1 mean of the first 4096 samples of the last locked frame into the running average
//               (signal_beta * average + (1 - signal_beta) * level); a level below thr_null_start * average counts one
//               more desync and leaves the average alone
//   counts[s]   = count
// The decision-directed fine-frequency error of a call (restated by oracle.dd_loop_error).
//   (sx, sy)  sum of u^4 over the call's differential symbols (unit magnitude each), n_terms of them
//   e_cp      mean angle of the call's PRS cyclic-prefix correlations / (2 pi 2048): the same residual, coarser, but
//             unambiguous within half a carrier
// The fourth-power estimate e_dd = angle(-sum) / (4 2 pi 2552) repeats every 1 / (4 2552) cycles per sample (0.2 carriers);
// e_cp picks its branch k.  Two things can make that wrong, and both are gated:
//   quality   |sum| is compared with what n_terms random unit phasors add up to (sqrt(n_terms)): below `gate` times that
//             (2.5 by default; 0 = off) the sum carries no usable phase -- single frames below ~3 dB SNR, an empty selection
//             -- and the call takes e_cp alone: unbiased, coarser.  (At s = |sum| / sqrt(n_terms) the estimate's spread
//             is 0.0225 / s carriers; a single PRS prefix has ~0.008-0.012 at 3-0 dB: the two cross near s = 2-3, and a
//             pure-noise sum exceeds 2.5 once in 500 calls.  profiles/r04_loop_gate.txt has the table: 8 was too
//             cautious -- at 3 dB it threw away an estimate twice as good as the prefix's.)
//   branch    a stream that was locked (previous branch 0: residual inside +-0.1 carriers) and now asks for branch +-1
//             has, far more often than a real 200 Hz jump between two calls, a PRS prefix hit by a fade or an impulse:
//             the departure must be seen on two consecutive calls before it is believed; the first time the branch is
//             held at 0.  (While a stream pulls in -- previous branch not 0, or its first call -- everything is believed.)
// Either gate counts in state.loop_gated.
constexpr int32_t DD_NO_BRANCH = 0x7fffffff;
__host__ __device__ inline float dd_loop_error(double sx, double sy, float e_cp, double n_terms, float gate, bool first_call,
                                               StreamState &st) {
    const double mag2 = sx * sx + sy * sy;
    if (!(n_terms > 0.0) || mag2 < double(gate) * double(gate) * n_terms) {
        st.loop_gated += 1;
        st.dd_pending = DD_NO_BRANCH;
        st.dd_branch = int32_t(rintf(e_cp * (4.0f * 2552.0f)));
        return e_cp;
    }
    const float e_dd = float(atan2(-sy, -sx) / (4.0 * 6.283185307179586 * 2552.0));
    int32_t k = int32_t(rintf((e_cp - e_dd) * (4.0f * 2552.0f)));
    if (!first_call && st.dd_branch == 0 && (k == 1 || k == -1) && st.dd_pending != k) {
        st.dd_pending = k;
        st.loop_gated += 1;
        k = 0;
    } else {
        st.dd_pending = DD_NO_BRANCH;
    }
    st.dd_branch = k;
    return e_dd + float(k) * (1.0f / (4.0f * 2552.0f));
}

struct TrackUpdateArgs {
    StreamState *state;
    const AcquiredFrame *frames;
    const float2 *cyc;         // [n_streams*max_out][76]
    int dd = 0;                // cyc holds dd4 sums (see OfdmArgs::dd4)
    const float2 *iq;
    size_t stream_stride;
    int n_streams;
    int64_t n_samples;
    int max_out;
    int64_t advance;           // samples between the first sample of this capture and of the next one
    float fine_beta, drift_beta, signal_beta, thr_null_start;
    int fixed_start;
    int32_t *counts;           // [n_streams] or nullptr
    int settle_only = 0;       // only turn "started in this call" marks (tracking == 2) into 1
    float dd_gate = 2.5f;      // dd_loop_error's quality gate
    int dd_terms_per_frame = 19200;   // unit terms one frame adds to the sums (256 carriers x the symbols that are demodulated)
    // the one-frame call's download riding in this launch: workgroups behind the n_streams updating ones copy `down` (what
    // the launches before this one produced: soft bits, frame and sync records); the updating workgroup writes the new state
    // to `state_out` as well (page-locked host memory) -- one launch instead of two at the end of the call
    CopyPiece down[3] = {{nullptr, nullptr, 0}, {nullptr, nullptr, 0}, {nullptr, nullptr, 0}};   // (the third: the constellation, when asked for)
    StreamState *state_out = nullptr;
    int copy_blocks = 0;       // set by the launcher
};
hipError_t launch_track_update(const TrackUpdateArgs &a, hipStream_t s, int iq_format = 0);
// Start tracking from an acquisition result (dabgpu_acquire_dev on the same capture): per stream, a least-squares line
// through the starts of the locked frames against their frame number round((start - first)/196608) gives the drift
// (0 with fewer than 4 locked frames); next_frame_start = start_last + 196608 + drift - advance; fine offset = mean of
// the locked frames', coarse = the last locked frame's; tracking = 1 (0 when no frame locked).
// only_lost != 0: streams that are tracking keep their state; the others start with tracking = 2 ("started in this
// call"), which the track_update launch behind it turns into 1 without touching anything else.
hipError_t launch_track_start(StreamState *state, const AcquiredFrame *frames, const int32_t *counts, int n_streams,
                              int max_out, int64_t advance, int only_lost, hipStream_t s);

// ---- DAB+ audio super-frame (dabplus_kernels.hip) ------------------------------
struct SuperframeStatus {      // == dabgpu_superframe_status
    int32_t firecode_ok;
    int32_t rs_corrected;
    int32_t rs_uncorrectable;
    int32_t num_aus;
    int32_t au_crc_mask;
    int32_t au_start[8];
    int32_t reserved[3];
};
// `done_flag` (optional, ONE super-frame only): the launch's single workgroup stores `done_seq` there behind its results --
// the word a host thread watches (dabgpu_ctx.hpp wait_for_signal) -- instead of a launch of its own behind the kernel
hipError_t launch_dabplus_superframes(const uint8_t *in, size_t in_stride, int n_superframes, int s, uint8_t *out,
                                      SuperframeStatus *status, hipStream_t stream, unsigned long long *done_flag = nullptr,
                                      unsigned long long done_seq = 0);

// Following DAB+ sub-channels to super-frames (dabgpu_dabplus_follow_dev): one entry per followed sub-channel, uploaded
// as a table; the align kernel (one wave per entry) finds each entry's phase from the raw Fire check of every logical
// frame, writes its plan behind the table, the result record and the carry record; the follow kernel (one workgroup per
// possible super-frame) decodes the super-frames the plans name.  No host synchronisation in between.
struct alignas(16) FollowEntry {
    uint64_t in;               // [n_cifs][in_stride] logical frames of 24 s bytes
    uint64_t carry_in;         // carry record or 0: 16-byte header {synced, held, 0, 0}, then 4 frames of 24 s bytes
    uint64_t carry_out;
    uint64_t data;             // [(n_cifs + 4) / 5][110 s]
    uint64_t status;           // [(n_cifs + 4) / 5] SuperframeStatus
    uint64_t result;           // one FollowResult
    uint64_t in_stride;
    int32_t s;                 // bitrate / 8
    int32_t reserved;
};
struct alignas(16) FollowPlan {
    int32_t phase, n_superframes, held, reserved;
};
struct FollowResult {          // == dabgpu_dabplus_follow_result
    int32_t n_superframes, phase, synced, dropped, raw_hits, held, reserved[2];
};
constexpr size_t FOLLOW_CARRY_HEADER = 16;
inline size_t follow_carry_bytes(int s) { return (FOLLOW_CARRY_HEADER + size_t(4) * 24 * size_t(s) + 15) & ~size_t(15); }
// bytes of device memory the table and the plans take (16-byte aligned)
size_t follow_table_bytes(int n_entries);
// `entries`: HOST array (copied to d_table on `stream` before the kernels); every pointer checked by the caller
hipError_t launch_dabplus_follow(const FollowEntry *entries, int n_entries, int n_cifs, void *d_table, size_t table_bytes,
                                 hipStream_t stream);

// ---- dynamic labels from PAD (pad_kernels.hip) -----------------------------------
// dabgpu_pad_labels_dev: one entry per followed DAB+ sub-channel, uploaded as a table; one wave per entry walks the access
// units the follow call left on the device (include/dabgpu_pad_walk.h is the walk) and writes the state record, the label
// and the counters.  n_superframes is read from the follow call's result record on the device.
struct alignas(16) PadEntry {
    uint64_t data;             // [max_superframes][data_stride], rows of 110 s bytes
    uint64_t data_stride;
    uint64_t status;           // [max_superframes] SuperframeStatus
    uint64_t follow;           // one FollowResult
    uint64_t state_in;         // dabgpu_pad::State or 0
    uint64_t state_out;
    uint64_t label;            // dabgpu_pad::Label
    uint64_t result;           // dabgpu_pad::Counters
    int32_t s;                 // bitrate / 8
    int32_t max_superframes;
    int32_t reserved[2];
};
// `entries`: HOST array (copied to d_table on `stream` before the kernel); every pointer checked by the caller
hipError_t launch_pad_labels(const PadEntry *entries, int n_entries, void *d_table, size_t table_bytes, hipStream_t stream);

// ---- slideshow objects from X-PAD (mot_kernels.hip) -------------------------------
// dabgpu_mot_slides_dev: the same table idea; one wave per entry runs the control walk of include/dabgpu_mot_walk.h in
// lane 0 and executes its copy orders with all 64 lanes.
struct alignas(16) MotEntry {
    uint64_t data;             // [max_superframes][data_stride], rows of 110 s bytes
    uint64_t data_stride;
    uint64_t status;           // [max_superframes] SuperframeStatus
    uint64_t follow;           // one FollowResult
    uint64_t state_in;         // dabgpu_mot::State or 0
    uint64_t state_out;
    uint64_t arena;            // dabgpu_mot::arena_bytes(body_capacity), updated in place
    uint64_t slides;           // [max_slides][slide_stride]
    uint64_t result;           // dabgpu_mot::Counters
    uint32_t slide_stride;
    int32_t max_slides;
    int32_t body_capacity;
    int32_t s;                 // bitrate / 8
    int32_t max_superframes;
    int32_t reserved;
};
// `entries`: HOST array (copied to d_table on `stream` before the kernel); every pointer checked by the caller
hipError_t launch_mot_slides(const MotEntry *entries, int n_entries, void *d_table, size_t table_bytes, hipStream_t stream);

// ---- following layer-II sub-channels (mp2_kernels.hip) ----------------------------
// dabgpu_mp2_follow_dev: one entry per followed DAB (MPEG layer II) sub-channel, uploaded as a table; the rate kernel (one
// wave per entry) checks every logical frame's header, chooses sampling rate and pairing phase, writes the entry's plan
// behind the table, both result records and the carry record; the frame kernel (one lane per frame, 64 frames a workgroup)
// checks header and ISO CRC and lifts the PAD into rows (include/dabgpu_mp2_frame.h is the contract and the code).
struct alignas(16) Mp2Entry {
    uint64_t in;               // [n_cifs][in_stride] logical frames of 3 B bytes
    uint64_t carry_in;         // carry record or 0
    uint64_t carry_out;
    uint64_t rows;             // [n_cifs + 1][220]
    uint64_t status;           // [n_cifs + 1] SuperframeStatus
    uint64_t follow;           // one FollowResult
    uint64_t result;           // one dabgpu_mp2::Result
    uint64_t in_stride;
    int32_t bitrate;           // B, kbit/s
    int32_t reserved[3];
};
struct alignas(16) Mp2Plan {
    int32_t rate, phase, n_rows, held;
};
size_t mp2_table_bytes(int n_entries);
// `entries`: HOST array (copied to d_table on `stream` before the kernels); every pointer checked by the caller
hipError_t launch_mp2_follow(const Mp2Entry *entries, int n_entries, int n_cifs, void *d_table, size_t table_bytes, hipStream_t stream);

// ---- layer-II frames to sub-band samples and audio levels (mp2_audio_kernels.hip) --
// dabgpu_mp2_subbands_dev, behind the follow call: one wave per checked frame decodes bit allocation, SCFSI, scale factors
// and samples a lane per cell (include/dabgpu_mp2_audio.h is the contract and the code); rows, rate and phase are read on the
// device from what the follow call wrote.
struct alignas(16) Mp2AudioEntry {
    uint64_t in;               // [n_cifs][in_stride] logical frames of 3 B bytes
    uint64_t carry_in;         // the carry record the follow call read, or 0
    uint64_t status;           // [n_cifs + 1] SuperframeStatus the follow call wrote
    uint64_t result;           // one dabgpu_mp2::Result the follow call wrote
    uint64_t levels;           // [n_cifs + 1] dabgpu_mp2::Level
    uint64_t subbands;         // 0, or [n_cifs + 1][2][36][32] float
    uint64_t audio;            // one dabgpu_mp2::AudioResult
    uint64_t in_stride;
    int32_t bitrate;           // B, kbit/s
    int32_t reserved[3];
};
size_t mp2_audio_table_bytes(int n_entries);
// `entries`: HOST array (copied to d_table on `stream` before the kernels); every pointer checked by the caller
hipError_t launch_mp2_subbands(const Mp2AudioEntry *entries, int n_entries, int n_cifs, void *d_table, size_t table_bytes, hipStream_t stream);

// ---- packet-mode MOT services to slides (packet_kernels.hip) -----------------------
// dabgpu_packet_slides_dev: one entry per (sub-channel, packet address), uploaded as a table; the scan kernel (one lane per
// 24-byte slot, 64 / S frames a wave) checks every candidate packet's CRC, resolves each frame's chain and writes one scan
// record per frame behind the table; the walk kernel (one wave per entry) sums the records' counters, runs the control walk
// of include/dabgpu_packet_walk.h in lane 0 over the followed packets alone and executes its copy orders with all 64 lanes.
struct alignas(16) PacketEntry {
    uint64_t in;               // [n_cifs][in_stride] logical frames of 24 s bytes
    uint64_t in_stride;
    uint64_t state_in;         // dabgpu_packet::State or 0
    uint64_t state_out;
    uint64_t arena;            // dabgpu_mot::arena_bytes(body_capacity), updated in place
    uint64_t slides;           // [max_slides][slide_stride]
    uint64_t result;           // dabgpu_packet::Counters
    uint64_t records;          // [n_cifs] scan records of packet_record_words(s) words (filled in by the launch)
    uint32_t slide_stride;
    int32_t max_slides;
    int32_t body_capacity;
    int32_t s;                 // bitrate / 8
    int32_t address;
    int32_t fec;
    int32_t reserved[2];
};
// A scan record: word 0 = followed packets n, word 1 = FEC | bad << 8 | padding << 16 | other << 24 (each <= 64), words 2, 3
// zero, then n words pos | L << 8 | h0 << 16 | h2 << 24 (room for s)
__host__ __device__ inline int packet_record_words(int s) { return 4 + s; }
// what dabgpu_packet_carousel_dev adds to an entry (its walk is the same kernel body with another sink; PacketEntry's slides,
// slide_stride, max_slides and body_capacity are then d_objects, object_stride, max_objects and object_capacity, its arena
// dabgpu_carousel::arena_bytes(...), its state dabgpu_carousel::State, its result dabgpu_carousel::Counters)
struct alignas(16) CarouselExtra {
    uint64_t directory;        // [directory_capacity]
    int32_t directory_capacity;
    int32_t assemblies;
};
// carousel: the table also holds a CarouselExtra per entry, between the entries and the records
size_t packet_table_bytes(const PacketEntry *entries, int n_entries, int n_cifs, bool carousel);
// workgroups of the scan launch; 0 = nothing to scan
uint64_t packet_scan_blocks(const PacketEntry *entries, int n_entries, int n_cifs);
// `entries`: HOST array (its `records` are set here; copied to d_table on `stream` before the kernels); every pointer checked
// by the caller.  extras: NULL = the slides walk; else [n_entries] (HOST) and the carousel walk
hipError_t launch_packet_walk(PacketEntry *entries, const CarouselExtra *extras, int n_entries, int n_cifs, void *d_table,
                              size_t table_bytes, hipStream_t stream);
// the carousel's walk launch alone, on the uploaded table (packet_carousel_kernels.hip; called by launch_packet_walk)
hipError_t launch_carousel_walk(const PacketEntry *d_table, const CarouselExtra *d_extras, int n_entries, int n_cifs, hipStream_t stream);

// ---- data groups of any packet-mode component (packet_groups_kernels.hip) -----------
// dabgpu_packet_groups_dev: the scan launch above as it stands (on a PacketEntry table of which it reads in, in_stride, s,
// address, fec and records), then one workgroup of PACKET_GROUPS_CHUNK lanes per entry: a lane per followed packet, the
// steps of include/dabgpu_data_groups.h as segmented scans, chunk by chunk with a carry.
constexpr int PACKET_GROUPS_CHUNK = 256;   // followed packets a workgroup takes at a time
struct alignas(16) PacketGroupsEntry {
    uint64_t state_in;         // dabgpu_groups::State or 0
    uint64_t state_out;
    uint64_t bytes;            // [bytes_capacity]
    uint64_t groups;           // [max_groups] dabgpu_groups::Record
    uint64_t result;           // dabgpu_groups::Counters
    int32_t bytes_capacity;
    int32_t max_groups;
    int32_t mode;
    int32_t keep_repeats;
    int32_t reserved[2];
};
static_assert(sizeof(PacketGroupsEntry) == 64, "an entry of the table in the stage area");
// the scan launch alone on an uploaded table whose `records` are set: what launch_packet_walk enqueues in front of its walk
// (`entries`: the HOST copy, for the grid)
hipError_t launch_packet_scan(const PacketEntry *d_table, const PacketEntry *entries, int n_entries, int n_cifs, hipStream_t stream);
// the table: [n_entries] PacketEntry, [n_entries] PacketGroupsEntry, then the scan records
size_t packet_groups_table_bytes(const PacketEntry *entries, int n_entries, int n_cifs);
// `scan`, `entries`: HOST arrays (scan[i].records is set here; both are copied to d_table on `stream` before the two launches)
hipError_t launch_packet_groups(PacketEntry *scan, const PacketGroupsEntry *entries, int n_entries, int n_cifs, void *d_table,
                                size_t table_bytes, hipStream_t stream);

// ---- RS(204,188) correction of packet-mode FEC frames (packet_fec_kernels.hip) ------
// dabgpu_packet_fec_dev and dabgpu_packet_fec_erasures_dev: one entry per sub-channel, uploaded as a table with its scratch
// records behind it.  Four launches: move (the carried and the new frames to the output and the new state record; a mark per
// new slot), accept (one wave per entry: candidate ends by ballot, the accept chain in order, the new record's head), correct
// (one workgroup per accepted frame: 16 syndromes of 12 rows on all lanes, then Berlekamp-Massey / Chien / Forney for the rows
// that need it, corrected bytes written back) and tally (one wave per entry sums the frames' counts into the result).
// include/dabgpu_packet_fec.h.
// With `erasures`, move also scans every arriving frame's slots (packet CRCs) into a word of suspect bits per window frame;
// accept carries the last D frames' bits on in the new head; correct goes on, for the rows the errors-only rule leaves, to
// errata decoding over the frame's erased columns; tally writes the wider record.  include/dabgpu_packet_fec_erasures.h.
struct alignas(16) PacketFecEntry {
    uint64_t in;               // [n_cifs][in_stride] logical frames of 24 s bytes
    uint64_t in_stride;
    uint64_t out;              // [n_cifs][out_stride]
    uint64_t out_stride;
    uint64_t state_in;         // dabgpu_packet_fec::state_bytes(s) or 0
    uint64_t state_out;
    uint64_t result;           // dabgpu_packet_fec::Counters; erasures: ErasureCounters
    // these four: filled in by the launch
    uint64_t marks;            // [8 + n_cifs s] bytes: the record's tail, then a mark per new slot
    uint64_t accepted;         // [16 + max_frames] words: count, 0 (erasures: suspect new slots), 2 x 0, the call's Counters; accepted ends
    uint64_t counts;           // [max_frames][8] words: FrameCounts, 3 x 0
                               // (erasures: [max_frames][12] words: ErasureFrameCounts, with suspects, beyond erasures, 2 x 0)
    uint64_t suspects;         // 0 (erasures: [delay(s) + n_cifs] 64-bit words: a suspect bit per slot of every window frame)
    int32_t s;
    int32_t max_frames;        // dabgpu_packet_fec::max_frames(s, n_cifs)
};
static_assert(sizeof(PacketFecEntry) == 96, "an entry of the table in the stage area");
size_t packet_fec_table_bytes(const PacketFecEntry *entries, int n_entries, int n_cifs, bool erasures);
// workgroups of the largest launch
uint64_t packet_fec_blocks(const PacketFecEntry *entries, int n_entries, int n_cifs);
// `entries`: HOST array (its scratch addresses and max_frames are set here; copied to d_table on `stream` before the kernels);
// every pointer checked by the caller
hipError_t launch_packet_fec(PacketFecEntry *entries, int n_entries, int n_cifs, bool erasures, void *d_table, size_t table_bytes,
                             hipStream_t stream);

// ---- T-DMB stream-mode sub-channels to TS packets (dmb_kernels.hip) -----------------
// dabgpu_dmb_follow_dev: one entry per sub-channel, uploaded as a table with its scratch behind it.  Three launches: sync (a
// workgroup per entry, a lane per phase: run counters, the locks of the call, the start of every packet the call emits, the
// new record's head, run counters and carried bytes), packets (a workgroup per emitted packet: the de-interleaving gather,
// 16 syndromes across the lanes, Berlekamp-Massey / Chien / Forney where needed, 188 bytes and a record out) and continuity
// (a workgroup per entry: a lane per packet in chunks of 256, the counter table and the census in LDS, the result and the
// rest of the new record).  include/dabgpu_dmb.h.
constexpr int DMB_SYNC_WORDS = 16;   // count, dropped, sync_hits, locks, lock_losses, locked, phase, 0 ...
struct alignas(16) DmbEntry {
    uint64_t in;               // [n_cifs][in_stride] logical frames of 3 kbps bytes
    uint64_t in_stride;
    uint64_t ts;               // [capacity][188]
    uint64_t records;          // [capacity] dabgpu_dmb::Record
    uint64_t state_in;         // dabgpu_dmb::STATE_BYTES or 0
    uint64_t state_out;
    uint64_t result;           // dabgpu_dmb::Result
    uint64_t sync;             // filled in by the launch: [DMB_SYNC_WORDS + max_packets] words: the sync launch's counts, then
                               // every emitted packet's start, counted from 2448 bytes before the call's first byte
    int32_t kbps;
    int32_t max_packets;       // dabgpu_dmb::new_packets(kbps, n_cifs): the most the call completes
    int32_t capacity;          // room in ts / records, packets; what does not fit is deferred into the new state record
};
static_assert(sizeof(DmbEntry) == 80, "an entry of the table in the stage area");
constexpr int DMB_MAX_ENTRIES = 65535;
size_t dmb_table_bytes(const DmbEntry *entries, int n_entries);
// workgroups of the largest launch (256 lanes each: DMB_MAX_BLOCKS keeps the launch's thread count below 2^32)
constexpr uint64_t DMB_MAX_BLOCKS = (uint64_t(1) << 24) - 1;
uint64_t dmb_blocks(const DmbEntry *entries, int n_entries);
// `entries`: HOST array (sync is set here; copied to d_table on `stream` before the kernels); every pointer checked by the caller
hipError_t launch_dmb(DmbEntry *entries, int n_entries, int n_cifs, void *d_table, size_t table_bytes, hipStream_t stream);

// ---- channel decoder (viterbi_kernels.hip) ---------------------------------
struct CodeTables {
    const uint16_t *mother_pos;  // [n_punct] mother-bit position of punctured bit i
    int n_punct;
    int nsteps;                  // trellis steps (info bits + 6)
    const uint8_t *prbs_bytes;   // [(nsteps-6)/8] energy-dispersal bytes, or nullptr = no descramble
    // codewords of 96 k + 6 steps (the rot kernel's): [k + 2] -- chunk_first[c] = punctured bits whose mother position lies
    // below step 96 c (c <= k), chunk_first[k + 1] = n_punct: the punctured bits of the 96-step chunk c are
    // [chunk_first[c], chunk_first[c + 1]), the last entry's the six tail steps'.  nullptr for other lengths.
    const uint16_t *chunk_first = nullptr;
};
// where build_device_code puts the chunk table: behind the positions, in the same allocation
__host__ __device__ inline int code_chunk_table_offset(int n_punct) { return (n_punct + 7) & ~7; }

// A8..A11: FIC of n_frames frames.
hipError_t launch_fic_decode(const CodeTables &c, const int8_t *soft, size_t soft_stride, int n_frames,
                             uint8_t *fib, uint8_t *crc_ok, hipStream_t s);
// A9 on contiguous punctured codewords.
hipError_t launch_viterbi_plain(const CodeTables &c, const int8_t *punct, int n_codewords, uint8_t *out,
                                hipStream_t s);
// A12: one subchannel, time de-interleave fused into the fetch.
struct MscArgs {
    const int8_t *soft;
    size_t soft_stride;
    int n_streams;
    int frames_per_stream;
    int start_bit;             // start_address * 64
    int nbits;                 // length * 64 (== n_punct)
    const int8_t *hist_in;     // [n_streams][15][nbits] or nullptr
    int8_t *hist_out;          // [n_streams][15][nbits] or nullptr
    uint8_t *out;              // [n_streams][frames*4][(nsteps-6)/8]
};
hipError_t launch_msc_decode(const CodeTables &c, const MscArgs &a, hipStream_t s);
// Small batches of a whole multiplex: every sub-channel's codewords in one launch of the wave-per-codeword kernel and
// all history rings in a second one (instead of one pair of launches per sub-channel).  nsteps must pass
// wave_group_supported() (every DAB profile does).
struct WaveGroupItem {
    CodeTables code;
    MscArgs args;
};
// the FIC of the same frames, decoded by the same launch (nullptr = not)
struct WaveFicItem {
    CodeTables code;
    const int8_t *soft;
    size_t soft_stride;
    int n_frames;
    uint8_t *fib, *crc_ok;
};
// (wave_group_supported: wave_plan.hpp)
// true when `n_waves` codewords whose longest takes `max_nsteps` trellis steps are all resident at once (LDS per wave x
// waves <= the chip's LDS): a grouped launch then finishes with its longest codeword instead of queueing kinds up
bool wave_group_one_round(int max_nsteps, long n_waves);
hipError_t launch_msc_decode_group(const WaveGroupItem *items, int n, hipStream_t s, const WaveFicItem *fic = nullptr);

// ---- large-batch variant: one codeword per lane (viterbi_lane_kernels.hip, lane_plan.hpp) ----
// (lane_supported: wave_plan.hpp)
// per-profile tables of the lane kernels: punct_idx [4*nsteps] (punctured index of each mother bit, -1 = erased);
// fused_desc [4*nsteps] and fused_tiles [2*ceil(nsteps/24)] from build_lane_fused_tables (may be null: prep path)
struct LaneTables {
    const int32_t *punct_idx;
    const int32_t *fused_desc;
    const int32_t *fused_tiles;
};
void build_lane_fused_tables(const uint8_t *mask, int nsteps, std::vector<int32_t> &desc, std::vector<int32_t> &tiles);
// What one launch decodes: a sub-channel (every field of args), the FIC of the same frames (args.soft / soft_stride /
// n_streams / frames_per_stream, args.out = the FIBs, crc_ok) or plain codewords (args.soft = the first one, code.n_punct
// bytes each; args.out; n_plain of them).
struct LaneItem {
    enum Kind { SUBCHANNEL, FIC, PLAIN };
    CodeTables code;
    LaneTables tables;
    MscArgs args;
    Kind kind;
    uint8_t *crc_ok;           // FIC: CRC flag per FIB
    int n_plain;               // PLAIN: codewords
    size_t codewords() const { return kind == PLAIN ? size_t(n_plain) : size_t(args.n_streams) * args.frames_per_stream * 4; }
};
// The work buffer of a launch and, for the device-table transport, where the entry table goes (device memory, 16-byte
// aligned, at least lane_table_bytes(); uploaded on the launch's stream).
struct LaneScratch {
    void *base;
    size_t bytes;
    bool unfused = false;      // DABGPU_FLAG_LANE_UNFUSED: depuncture in a pass of its own (lane_prep_kernel)
    void *table = nullptr;
    size_t table_bytes = 0;
};
// lane_plan.hpp states which items take the fused forward pass (lane_item_fusable) and how many bytes of LaneScratch a
// list needs (lane_scratch_bytes).
size_t lane_table_bytes(const LaneItem *items, int n);
// THE launch of the lane kernels.  Every item must pass lane_supported(nsteps) and have a 4-byte aligned output.
//   A list whose items all pass lane_item_fusable (and !sc.unfused): ONE forward and ONE traceback launch per transport
//   unit -- by value in the kernel arguments (at most 16 entries per launch, longer lists in several), or, with sc.table,
//   any number of entries through a table in device memory, dispatched longest codeword first.  (ONE such item that is the
//   FIC or plain codewords: its forward pass is the same body on a 64-row window, lane_forward_fused_kernel.)
//   ONE item that does not (or sc.unfused): lane_prep_kernel, lane_forward_kernel, the traceback on a pack of one.
//   Anything else is hipErrorInvalidValue.
// The history rings (args.hist_out of the sub-channel items) are written behind the last traceback.
// mid (optional, timing only): two events, recorded behind the forward pass and behind the traceback -- only when the whole
// list went out as one forward and one traceback launch; *mid_recorded says whether they were.
hipError_t launch_lane(const LaneItem *items, int n, const LaneScratch &sc, hipStream_t s, hipEvent_t *mid = nullptr,
                       bool *mid_recorded = nullptr);
// Dynamic-LDS request (>= lds) that makes every CU hold the same number of workgroups of a `grid`-workgroup
// launch when at most `o_cap` fit per CU otherwise (the dispatcher fills CUs greedily).
size_t balanced_lds_bytes(unsigned grid, size_t lds, unsigned o_cap);
// history ring update alone (used by both MSC variants)
hipError_t launch_msc_history(const MscArgs &a, hipStream_t s);

// ---- reception quality (quality_kernels.hip) ----------------------------------
// MER of the differential constellation from the soft bits, per frame: data symbols [first_symbol, first_symbol + n_symbols)
// of frame f (at soft + f*stride); out[f] = {sum (a+b)^2, sum (a-b)^2, carriers counted, 0} with a = |soft[n]|,
// b = |soft[1536 + n]| of a symbol's carrier n, carriers whose pair is (0, 0) (erased) left out (== dabgpu_mer)
struct MerSums {
    uint64_t signal, error;
    int32_t carriers, reserved;
};
hipError_t launch_mer(const int8_t *soft, size_t stride, int n_frames, int first_symbol, int n_symbols, MerSums *out,
                      hipStream_t s);
// Channel bit errors by re-encoding: per codeword the decoded bytes (args.out for a sub-channel, the FIBs for the FIC) are
// scrambled again, run through the mother code and compared with the hard decisions of the soft bytes the decoder read
// (soft_source.hpp) for every mother bit the profile keeps; counts[g] = {errors, bits} (bits: soft byte != 0).  Sub-channel
// items take args.soft / soft_stride / n_streams / frames_per_stream / start_bit / nbits / hist_in / out; the FIC item
// args.soft / soft_stride / n_streams / frames_per_stream / out (= FIBs).  Up to ber_group_max() items per launch (longer
// lists are chunked).
struct BerItem {
    int nsteps;
    const uint8_t *prbs_bytes;
    const int32_t *punct_idx;  // LaneTables::punct_idx of the profile
    MscArgs args;
    bool is_fic;
    uint32_t *counts;          // [n_codewords][2]
};
hipError_t launch_channel_ber(const BerItem *items, int n, hipStream_t s);
int ber_group_max();

// ---- transmitter identification from the null symbol (tii_kernels.hip) --------
// EN 300 401 section 14.8, Mode I.  Comb c (sub-identifier, 0..23) and position b (0..7) own the carrier pairs
// k = B + 2c + 48b, k + 1 for the four bases B; pattern p (main identifier, 0..69) switches on four of the eight positions.
// The carrier bases and which bit of a pattern is b = 0 are the two conventions the tests cannot pin against the standard:
// both live here, and only here (tests/tii_reference.py restates them).
constexpr int TII_COMBS = 24, TII_POSITIONS = 8, TII_CELLS = TII_COMBS * TII_POSITIONS, TII_PATTERNS = 70;
__host__ __device__ constexpr int tii_base(int q) { return q < 2 ? -768 + 384 * q : 384 * q - 767; }   // -768 -384 1 385
// pattern p = the p-th 8-bit value with four bits set, ascending; bit 7 - b is position b
__host__ __device__ constexpr int tii_pattern_mask(int p) {
    for (int v = 0, i = 0; v < 256; v++)
        if (__builtin_popcount(unsigned(v)) == 4 && i++ == p) return v;
    return -1;
}
// The window: 2048 samples centred in the null symbol, [-2352, -304) relative to the first sample of the PRS prefix; the
// noise floor: mean power of the bins 776 <= |k| <= 927 (outside the ensemble, inside the guard band to the next block).
constexpr int TII_WIN_BEGIN = 2352, TII_FLOOR_LO = 776, TII_FLOOR_HI = 927;
struct TiiRecord {             // == dabgpu_tii_acc (784 bytes): per frame, or a stream's running sums
    float cell[TII_CELLS];     // [c][b]: power of the cell's 8 carriers
    float floor;               // mean power of a noise bin
    int32_t frames;
    int32_t reserved[2];
};
struct TiiArgs {
    const float2 *iq;          // context's sample format
    size_t stride;             // frame (frame calls) or stream (acquired calls) stride, complex samples
    int n_streams, frames_per_stream;
    const float *freq_offset;  // frame calls: [n_frames] cycles/sample, or nullptr: the stream states
    const struct StreamState *state;
    const AcquiredFrame *acq;  // acquired calls: [n_streams][frames_per_stream]
    int timing_margin;         // acquired calls: PRS prefix = start + timing_margin
    TiiRecord *frame;          // [n_frames] per-frame records
    TiiRecord *acc;            // [n_streams] += the stream's frames, in frame order
};
hipError_t launch_tii(const float2 *twiddle, const TiiArgs &a, hipStream_t s, int iq_format);

// ---- channel impulse response from the phase reference symbol (cir_kernels.hip) --------
// Window: the 2048 samples [504, 2552) after the first sample of the PRS prefix (the front end's).  Hann taper
// w(k) = 0.5 + 0.5 cos(pi k / 769) over the 1536 carriers, whose sum is exactly 768.
constexpr int CIR_WIN_BEGIN = 504, CIR_TAPS = 2048, CIR_CARRIERS = 1536;
struct CirRecord {             // == dabgpu_cir_acc (14 352 bytes): per frame, or a stream's running sums
    float tap[CIR_TAPS];       // |h[n]|^2
    float carrier[CIR_CARRIERS];  // (1536 / 2048^2) |X_k|^2, k = -768..-1, 1..768
    int32_t frames;
    int32_t reserved[3];
};
struct CirArgs {
    const float2 *iq;          // context's sample format
    size_t stride;             // frame (frame calls) or stream (acquired calls) stride, complex samples
    int n_streams, frames_per_stream;
    const float *freq_offset;  // frame calls: [n_frames] cycles/sample, or nullptr: the stream states
    const struct StreamState *state;
    const AcquiredFrame *acq;  // acquired calls: [n_streams][frames_per_stream]
    int timing_margin;         // acquired calls: PRS prefix = start + timing_margin
    const int8_t *prs_qt;      // [2048] quarter turns of the PRS per bin, -1 = not a carrier
    CirRecord *frame;          // [n_frames] per-frame records
    CirRecord *acc;            // [n_streams] += the stream's frames, in frame order
};
hipError_t launch_cir(const float2 *twiddle, const CirArgs &a, hipStream_t s, int iq_format);

// ---- ETI(NI) output (eti_kernels.hip) ---------------------------------------
constexpr int ETI_FRAME_BYTES = 6144;
constexpr int ETI_MAX_STREAMS = 64;
constexpr int ETI_FIC_DELAY = 15;
constexpr int ETI_FIC_BYTES = 96;
constexpr int ETI_CIF_COUNTS = 5000;
struct EtiHistory {            // == dabgpu_eti_history (1504 bytes)
    uint8_t fib[ETI_FIC_DELAY][ETI_FIC_BYTES];
    uint8_t crc_ok[ETI_FIC_DELAY][3];
    uint8_t pad[3];
    int32_t next_count, valid, reserved[2];
};
struct EtiStatus {             // == dabgpu_eti_status
    uint16_t cif_count;
    uint8_t flags, fib_ok;
    uint16_t length, reserved;
};
// Everything a call's frames share, by value in the kernel arguments (~1.4 KB)
struct EtiArgs {
    const uint8_t *out[ETI_MAX_STREAMS];       // sub-channel k of the FRAME (plan order): [n_streams][n_cif][bytes[k]]
    uint16_t offset[ETI_MAX_STREAMS];          // byte offset of its data behind the FIC
    uint16_t bytes[ETI_MAX_STREAMS];
    uint32_t header[2 + ETI_MAX_STREAMS];      // frame bytes 0 .. 8 + 4 nst as little-endian words (ERR, FSYNC, FCT, FP = 0)
    uint16_t lane_shift[64];                   // x^(8 C (63 - lane)) mod P: moves a lane's chunk CRC to the end of the data
    const uint8_t *fib, *crc_ok;
    const EtiHistory *history_in;
    const int32_t *base;                       // [n_streams] count of the call's first CIF | no-anchor << 16 (pre-pass)
    uint8_t *eti;
    EtiStatus *status;
    int n_streams, frames_per_stream;
    int nst, data_bytes;
    int chunk_words;                           // C / 4: 32-bit words of FIC + data every lane folds
    uint16_t header_crc0;                      // header CRC (finished) with FCT = FP = 0
    uint16_t fct_shift, fp_shift;              // x^(8 (Lh - 1) + 16), x^(8 (Lh - 3) + 16) mod P: a byte's way to the header's end
    uint16_t data_init;                        // 0xFFFF x^(8 L) mod P: the start value's way through FIC + data
};
struct EtiAnchorArgs {
    const uint8_t *fib, *crc_ok;
    const EtiHistory *history_in;
    EtiHistory *history_out;
    const int32_t *cif_start;
    int32_t *base;
    int n_streams, frames_per_stream;
};
hipError_t launch_eti(const EtiAnchorArgs &p, const EtiArgs &a, hipStream_t s);
// the pre-pass alone (the EDI writer's first launch)
hipError_t launch_eti_anchor(const EtiAnchorArgs &p, hipStream_t s);

// ---- EDI output (edi_kernels.hip; include/dabgpu_edi.h) ------------------------
constexpr int EDI_MAX_WRITER_PACKET = 6640;    // what a plan that fits an ETI frame can need (6620), a multiple of 16
// Everything a call's packets share, by value in the kernel arguments (~1.4 KB)
struct EdiArgs {
    const uint8_t *out[ETI_MAX_STREAMS];       // sub-channel k of the PACKET (plan order): [n_streams][n_cif][bytes[k]]
    uint16_t offset[ETI_MAX_STREAMS];          // byte offset of its data among the sub-channels' data
    uint16_t bytes[ETI_MAX_STREAMS];
    uint8_t stc[4 * ETI_MAX_STREAMS];          // the plan's STC words
    uint16_t lane_shift[64];                   // x^(8 chunk_bytes (63 - lane)) mod P
    const uint8_t *fib, *crc_ok;
    const EtiHistory *history_in;
    const int32_t *base;                       // [n_streams] what the anchor pre-pass left
    const uint32_t *seq_start;                 // [n_streams] DEVICE, or nullptr = 0
    uint8_t *edi;
    EtiStatus *status;
    unsigned long long stream_stride;
    int n_streams, frames_per_stream;
    int nst, data_bytes;
    int packet_bytes;
    int chunk_bytes;                           // bytes of the packet in front of its CRC every lane folds
    uint16_t crc_init;                         // 0xFFFF x^(8 (packet_bytes - 2)) mod P
};
hipError_t launch_edi(const EtiAnchorArgs &p, const EdiArgs &a, hipStream_t s);

// ---- EDI input (edi_read_kernels.hip; include/dabgpu_edi.h) --------------------
constexpr int EDI_READ_SPAN = 4096;            // byte positions a workgroup of the check launch judges
constexpr int EDI_READ_MAX_ENTRIES = 65535;    // (the check launch's grid has an entry per y)
// One entry of the table in device memory (addresses as integers)
struct EdiReadEntry {
    uint64_t bytes, state_in, state_out, fib, crc_ok, status, result;
    uint64_t good;                             // scratch: bit q % 64 of word q / 64 = C(q) of the contract
    uint64_t open;                             // scratch: ... = H(q) and the packet is incomplete
    uint64_t out[ETI_MAX_STREAMS];             // stream k of the PACKET (plan order): [max_rows][8 STL], 0 = not wanted
    int32_t n_bytes, max_rows, has_plan, nst;
    uint8_t stc[4 * ETI_MAX_STREAMS];          // the plan's STC words
};
// positions an entry's S can have, whatever its state's tail holds, and the words of one bitmap over them
inline size_t edi_read_positions(int n_bytes) { return size_t(n_bytes) + 8191u; }
inline size_t edi_read_bitmap_words(int n_bytes) { return (edi_read_positions(n_bytes) + 63) / 64; }
// scratch an entry needs behind the table: its two bitmaps (bytes, a multiple of 16)
inline size_t edi_read_scratch_bytes(int n_bytes) { return (2 * edi_read_bitmap_words(n_bytes) * 8 + 15) / 16 * 16; }
// entries: the host's table with everything but good and open filled in (this fills them); d_table: n_entries *
// sizeof(EdiReadEntry) + the sum of edi_read_scratch_bytes, 16-byte aligned
hipError_t launch_edi_read(EdiReadEntry *entries, int n_entries, void *d_table, hipStream_t s);

// ---- EDI PFT layer, writer (pft_kernels.hip; include/dabgpu_pft.h) --------------
// Everything a call's packets share, by value in the kernel arguments: the fields of dabgpu_pft::Layout the kernel reads
struct PftArgs {
    const uint8_t *af;                         // [n_streams] at in_stride: n_packets AF packets of packet_bytes back to back
    uint8_t *pf;                               // [n_streams] at out_stride: n_packets * stream_bytes
    unsigned long long in_stride, out_stride;
    const uint32_t *pseq_start;                // [n_streams] DEVICE
    int32_t packet_bytes, fec, addr, chunks, rs_k, rs_z, block_bytes, fcount, plen, header_bytes, stream_bytes;
    uint32_t source, dest;
};
hipError_t launch_pft(const PftArgs &a, int n_streams, int n_packets, hipStream_t s);

// ---- EDI PFT layer, reader (pft_read_kernels.hip; include/dabgpu_pft.h) ---------
constexpr int PFT_READ_SPAN = 4096;            // byte positions a workgroup of the check launch judges
constexpr int PFT_READ_MAX_ENTRIES = 65535;    // (the check and fill launches' grids have an entry per y)
constexpr int PFT_READ_MAX_TAIL = 8211;        // == dabgpu_pft::MAX_TAIL
constexpr int PFT_READ_MAX_BLOCK = 10496;      // == dabgpu_pft::MAX_BLOCK
// One entry of the table in device memory (addresses as integers)
struct PftReadEntry {
    uint64_t bytes, state_in, state_out, out, records, result;
    uint64_t good;                             // scratch: bit q % 64 of word q / 64 = T(q) of the contract
    uint64_t stop;                             // scratch: H(q) with an incomplete fragment, or U(q): the walk ends there
    uint64_t arena;                            // scratch: per group the fill launch works on, its received map and fragments
    int32_t n_bytes, flags;
    uint32_t max_records, arena_bytes;
};
inline size_t pft_read_positions(int n_bytes) { return size_t(n_bytes) + size_t(PFT_READ_MAX_TAIL); }
inline size_t pft_read_bitmap_words(int n_bytes) { return (pft_read_positions(n_bytes) + 63) / 64; }
// A group the fill launch works on holds a fragment with FEC (16 header bytes and its payload) in S, or is one of the two
// carried: 32 map bytes and its payload are at most twice its bytes in S, or 32 + PFT_READ_MAX_BLOCK
inline size_t pft_read_arena_bytes(int n_bytes) { return (2 * (32 + size_t(PFT_READ_MAX_BLOCK)) + 2 * pft_read_positions(n_bytes) + 15) / 16 * 16; }
// scratch an entry needs behind the table: its two bitmaps and its arena (bytes, a multiple of 16)
inline size_t pft_read_scratch_bytes(int n_bytes) { return (2 * pft_read_bitmap_words(n_bytes) * 8 + 15) / 16 * 16 + pft_read_arena_bytes(n_bytes); }
// entries: the host's table with everything but good, stop, arena and arena_bytes filled in (this fills them); d_table:
// n_entries * sizeof(PftReadEntry) + the sum of pft_read_scratch_bytes, 16-byte aligned
hipError_t launch_pft_read(PftReadEntry *entries, int n_entries, void *d_table, hipStream_t s);

// ---- ETI(NI) input (eti_read_kernels.hip) -------------------------------------
constexpr int ETI_READ_SCAN_SPAN = 8192;       // byte positions a workgroup of the scan judges
constexpr int ETI_READ_ROW_WAVES = 4;          // rows (waves) per workgroup of the check launch
constexpr int ETI_READ_LIST_HEAD = 4;          // words in front of a row list: rows, where the tail begins, skipped, resyncs
// One entry of the table in device memory (addresses as integers; ~1.3 KB)
struct EtiReadEntry {
    uint64_t bytes, state_in, state_out, fib, crc_ok, status, result;
    uint64_t bitmap;                           // scratch: bit q % 64 of word q / 64 = position q of S is a candidate
    uint64_t rows;                             // scratch: ETI_READ_LIST_HEAD words, then the offset in S of every row
    uint64_t out[ETI_MAX_STREAMS];             // stream k of the FRAME (plan order): [max_frames][bytes[k]], 0 = not wanted
    int32_t n_bytes, max_frames, bitmap_words, has_plan;
    int32_t nst, fl;                           // the plan's
    int32_t data_bytes;                        // FIC + streams of the plan: what its data CRC covers
    int32_t chunk_words;                       // 32-bit words of them a lane folds
    uint32_t row_base, scan_base;              // the entry's first wave of the check launch, first workgroup of the scan
    uint16_t offset[ETI_MAX_STREAMS], nbytes[ETI_MAX_STREAMS];
    uint16_t lane_shift[64];                   // x^(32 chunk_words (63 - lane)) mod P
    uint16_t data_init, pad[3];                // 0xFFFF x^(8 data_bytes) mod P
    uint8_t stc[4 * ETI_MAX_STREAMS];          // the plan's STC words
};
// scratch an entry needs behind the table: its bitmap, then its row list (bytes, a multiple of 8)
inline size_t eti_read_scratch_bytes(int n_bytes) {
    const size_t words = (size_t(n_bytes) + 63) / 64, rows = (size_t(n_bytes) + 6143) / 6144;
    return words * 8 + ((ETI_READ_LIST_HEAD + rows) * 4 + 15) / 16 * 16;
}
// behind the entries the table holds their scan_base and row_base once more, packed ([n_entries] words each): a wave finds
// its entry from one coalesced load of them instead of a chain of dependent loads through the entries
inline size_t eti_read_bases_bytes(int n_entries) { return (size_t(n_entries) * 8 + 15) / 16 * 16; }
// entries: the host's table with everything but bitmap, rows, row_base and scan_base filled in (this fills them);
// d_table: n_entries * sizeof(EtiReadEntry) + eti_read_bases_bytes + the sum of eti_read_scratch_bytes, 16-byte aligned
hipError_t launch_eti_read(EtiReadEntry *entries, int n_entries, void *d_table, hipStream_t s);

// ---- modulator: ETI(NI) frames to Mode-I IQ (mod_kernels.hip) -----------------
// One ETI frame's coded bits ("coded record"): the 2304 punctured FIC bits of its three FIBs, then the 55 296 bits of its
// CIF BEFORE time interleaving (every sub-channel's punctured codeword at 64 SAD, zeros elsewhere), bit i in bit i % 32
// of word i / 32.
constexpr int MOD_FIC_WORDS = 72, MOD_CIF_WORDS = 1728, MOD_CODED_WORDS = MOD_FIC_WORDS + MOD_CIF_WORDS;
constexpr int MOD_DEPTH = 15;                  // CIFs the time interleaver looks back
constexpr int MOD_SYM_WORDS = 96;              // the 3072 bits of one data symbol
constexpr int MOD_ITEMS = 77;                  // null symbol, PRS, 75 data symbols
constexpr int MOD_PRBS_BYTES = 511;            // the energy-dispersal sequence repeats after 511 bits, so after 511 bytes too
constexpr int MOD_BAD_INPUT = 1, MOD_MISALIGNED = 2;
struct ModState {              // == dabgpu_mod_state (103 680 bytes): the CIF parts of the last 15 coded records, oldest first
    uint32_t cif[MOD_DEPTH][MOD_CIF_WORDS];
};
struct ModStatus {             // == dabgpu_mod_status
    uint32_t flags;
    uint8_t refused, reserved[3];
};
struct ModCode {               // one codeword of an ETI frame: up to four runs of 128-bit blocks, then the tail
    uint16_t in_offset, in_bytes;              // where its bytes are in the frame
    uint16_t out_word;                         // first word of its punctured bits in the coded record
    uint16_t blocks[4];
    uint8_t pi[4];
};
struct ModTables {
    const uint8_t *prbs;       // [511] energy-dispersal bytes
    const int16_t *n_of_bin;   // [2048] data index n of FFT bin b, -1 = not a carrier
    const int8_t *prs_qt;      // [2048] quarter turns of the PRS per bin
    const float2 *twiddle;     // SyncTables::twiddle
    const float2 *null_symbol; // [2656] the TII null symbol at gain 1, or nullptr = zeros
};
struct ModArgs {               // by value in the kernel arguments (~1.7 KB)
    ModCode code[1 + ETI_MAX_STREAMS];         // [0] the FIC, then the plan's streams
    uint32_t header[2 + ETI_MAX_STREAMS];      // the plan's frame bytes 0 .. 8 + 4 nst as little-endian words
    int n_codes, nst;
    const uint8_t *eti;        // [n_streams][n_cif][6144]
    const ModState *state_in;
    ModState *state_out;
    uint32_t *coded;           // [n_streams][n_cif][MOD_CODED_WORDS]
    uint32_t *cum;             // [n_frames][75][96]: per data symbol the running sum of the quarter turns, low bits | high bits
    float2 *iq;
    size_t frame_stride;
    ModStatus *status;
    float gain;
    int n_streams, frames_per_stream;
};
// two launches each; `symbols` follows `encode` on the same stream
hipError_t launch_mod_encode(const ModTables &t, const ModArgs &a, hipStream_t s);
hipError_t launch_mod_symbols(const ModTables &t, const ModArgs &a, hipStream_t s);
// the null symbol of transmitter (main p, sub c) at gain 1 into out[2656]
hipError_t launch_mod_tii(const int8_t *prs_qt, int main_id, int sub_id, float2 *out, hipStream_t s);

// Let every kernel that takes dynamic LDS use the whole 160 KB of a CU: set once per context creation (on the
// context's device) instead of per launch.
hipError_t init_viterbi_kernel_attributes();
hipError_t init_lane_kernel_attributes();

// (viterbi_wave_lds_bytes, viterbi_fits: wave_plan.hpp)

}  // namespace dabk
