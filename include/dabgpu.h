/*
 * dabgpu.h -- C ABI of the MI355X-native DAB Mode-I receive chain (libdabgpu.so).
 *
 * This is the drop-in boundary for the ONE hot path of the SDR++ DAB plugin: the
 * OFDM front end and the channel decoder that sit behind Radio_Block / OFDM_Demod /
 * BasicRadio.  Every entry point names the reference interface it replaces
 * (file:line under /root/reference).  The DSP those interfaces front lives in git
 * submodules that are empty in the reference snapshot, so the citations are the
 * plugin's call sites.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types, no exceptions.
 *   - return 0 (DABGPU_OK) or a negative dabgpu_status; dabgpu_strerror() explains.
 *   - `_dev` entry points take DEVICE pointers and a hipStream_t passed as void*
 *     (NULL = the context's own stream); they only enqueue work.  The variants
 *     without `_dev` take HOST pointers, copy, run and synchronise.
 *   - the context's own stream is NON-BLOCKING (hipStreamNonBlocking): it is not
 *     ordered behind the null stream or any other.  Device buffers handed to a
 *     `_dev` call with stream == NULL must already hold their data (and no fill of
 *     an output buffer may still be running); a caller that produces them on a
 *     stream of its own passes THAT stream.
 *   - the caller owns every buffer; a context is thread-compatible (one caller
 *     at a time per context), contexts are independent.
 *   - work enqueued through ONE context must be stream-ordered: the entry points
 *     share per-context work buffers (decoder scratch, the stream / tracked / frame
 *     calls' loop input, the stream states), so AT MOST ONE caller stream may be in
 *     flight per context -- two calls on different streams need an event between
 *     them (or two contexts, as the host mirror uses: one for OFDM_Demod, one for
 *     BasicRadio).
 *   - soft bits are int8: +127 = logical 1, -127 = logical 0, 0 = erased
 *     (`viterbi_bit_t`, /root/reference/src/radio_block.h:19).  They are
 *     level-free: scaling cf32 samples of unit mean power by 2^k leaves every
 *     soft bit unchanged for -52 <= k <= 56 (measured; the quantiser's 1e-30
 *     floor and float32's range end it).
 *   - the library REQUIRES a gfx950 device for everything except the table
 *     getters; there is no CPU fallback.
 */
#ifndef DABGPU_H
#define DABGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DABGPU_ABI_VERSION 6   /* 6: every closed-loop call defaults to the reference's cyclic-prefix estimator (dabgpu_track_cfg.decision_directed */
                               /*    defaults to 0 and the frame call honours it); 5: one frame-buffer allocator, host-fed ring, loop gate           */

typedef enum dabgpu_status {
    DABGPU_OK = 0,
    DABGPU_ERR_ARG = -1,       /* null / out-of-range argument              */
    DABGPU_ERR_HIP = -2,       /* a HIP runtime call failed                 */
    DABGPU_ERR_NOMEM = -3,     /* device or host allocation failed          */
    DABGPU_ERR_NODEVICE = -4,  /* no gfx950 device visible                  */
    DABGPU_ERR_PROFILE = -5,   /* unsupported transmission mode / profile   */
    DABGPU_ERR_CAPACITY = -6   /* request exceeds what the context was sized for */
} dabgpu_status;

/* ------------------------------------------------------------------------ */
/* A0: constant parameter blocks.                                            */
/* Replaces get_DAB_OFDM_params(mode)   /root/reference/src/radio_block.cpp:12 */
/*          get_dab_parameters(mode)    /root/reference/src/radio_block.cpp:13 */
/* Only transmission mode 1 is supported (radio_block.cpp:9).                 */
/* ------------------------------------------------------------------------ */
typedef struct dabgpu_ofdm_params {
    int32_t nb_frame_symbols;     /* 76  */
    int32_t nb_symbol_period;     /* 2552 */
    int32_t nb_null_period;       /* 2656 */
    int32_t nb_fft;               /* 2048 */
    int32_t nb_cyclic_prefix;     /* 504 */
    int32_t nb_data_carriers;     /* 1536 */
    int32_t freq_carrier_spacing; /* 1000 Hz */
    int32_t nb_frame_samples;     /* 196608 */
} dabgpu_ofdm_params;

typedef struct dabgpu_dab_params {
    int32_t nb_frame_bits;    /* 230400 */
    int32_t nb_symbols;       /* 75 data symbols */
    int32_t nb_fic_symbols;   /* 3 */
    int32_t nb_msc_symbols;   /* 72 */
    int32_t nb_sym_bits;      /* 3072 */
    int32_t nb_fic_bits;      /* 9216 */
    int32_t nb_msc_bits;      /* 221184 */
    int32_t nb_fibs;          /* 12 */
    int32_t nb_cifs;          /* 4 */
    int32_t nb_fib_bits;      /* 256 */
    int32_t nb_fib_cif_bits;  /* 2304: one punctured FIC group */
    int32_t nb_fibs_per_cif;  /* 3 */
    int32_t nb_cif_bits;      /* 55296 */
} dabgpu_dab_params;

int dabgpu_get_ofdm_params(int transmission_mode, dabgpu_ofdm_params *out);
int dabgpu_get_dab_params(int transmission_mode, dabgpu_dab_params *out);

/* A0': replaces get_DAB_PRS_reference(mode, span<complex<float>>[nb_fft])
 * /root/reference/src/radio_block.cpp:18-19.  out = nb_fft interleaved (re,im). */
int dabgpu_get_prs_reference(int transmission_mode, float *out_cf32, int nb_fft);
/* A0': replaces get_DAB_mapper_ref(span<int>[nb_data_carriers], nb_fft)
 * /root/reference/src/radio_block.cpp:20-21. */
int dabgpu_get_mapper_reference(int32_t *out, int nb_data_carriers, int nb_fft);

/* ------------------------------------------------------------------------ */
/* Context                                                                   */
/* ------------------------------------------------------------------------ */
typedef struct dabgpu_ctx dabgpu_ctx;

typedef struct dabgpu_cfg {
    int32_t device;          /* HIP device ordinal                                    */
    int32_t max_frames;      /* largest n_frames any call will pass (scratch sizing)  */
    int32_t transmission_mode; /* must be 1                                           */
    int32_t flags;           /* DABGPU_FLAG_*                                         */
    int32_t ofdm_symbol_runs;  /* front end: cut every frame into this many runs of    */
                             /* consecutive symbols (one wavefront each), 1..75;      */
                             /* 0 = chosen from the batch size                        */
    int32_t reserved[3];     /* must be 0                                             */
} dabgpu_cfg;

/* Which kernels decode (results are identical; the default picks by batch size).  Meant for tests and timing. */
#define DABGPU_FLAG_NONE 0
#define DABGPU_FLAG_VITERBI_WAVE  (1 << 0) /* channel decoder: one wavefront per codeword, always (codewords    */
                                           /* above ~680 kbit/s do not fit its LDS slab: those go per lane)      */
#define DABGPU_FLAG_VITERBI_LANE  (1 << 1) /* one codeword per lane wherever the length allows, any batch size */
#define DABGPU_FLAG_LANE_UNFUSED  (1 << 2) /* lane decoder: separate depuncture pass before the forward pass   */
/* Test hooks (tests/ only; they change no result, they force a branch that hardware takes rarely): */
#define DABGPU_FLAG_TEST_ONE_DOMAIN (1 << 30) /* dabgpu_alloc_frame_buffers(DABGPU_PLACE_DOMAINS): the check of the  */
                                           /* placed pair is taken as 1.00 (a box whose chunks share one domain)   */

/* Replaces the construction in Radio_Block::Radio_Block
 * (/root/reference/src/radio_block.cpp:11-22: params + PRS + mapper + OFDM_Demod). */
int  dabgpu_create(const dabgpu_cfg *cfg, dabgpu_ctx **out);
void dabgpu_destroy(dabgpu_ctx *ctx);
const char *dabgpu_strerror(int status);
int  dabgpu_abi_version(void);
/* Entry points make cfg.device current for the duration of the call and restore the caller's device afterwards: a
 * process may hold contexts on several GPUs. */
/* block until everything enqueued on the context's own stream has finished */
int  dabgpu_sync(dabgpu_ctx *ctx);
/* the context's own hipStream_t (as void*) */
void *dabgpu_stream(dabgpu_ctx *ctx);

/* Page-locked host memory for the host-pointer entry points: buffers obtained here are copied to and from the
 * device by DMA at the full link rate, pageable ones go through the runtime's bounce buffers (measured on the
 * pool's PCIe Gen5 link: see DESIGN.md section 5).  Any host pointer is accepted everywhere; this is an
 * optimisation for callers that own their buffers, e.g. the host mirror's frame and soft-bit buffers. */
void *dabgpu_host_alloc(size_t bytes);
void dabgpu_host_free(void *p);
/* (The one-frame calls -- dabgpu_ofdm_demod_stream_frame, dabgpu_decode_stream_frames, dabgpu_dabplus_superframes -- let
 * their kernels write results straight into page-locked caller buffers and end on a watched word instead of a stream
 * synchronisation ONLY for buffers obtained here, which are coherent; results written into any other page-locked memory
 * (hipHostRegister, non-coherent allocations) are followed by hipStreamSynchronize: HIP promises host visibility of kernel
 * writes to such memory only there.) */

/* Test hook (tests/ only; changes no result): the nth one-frame call of this context from now on
 * (dabgpu_ofdm_demod_stream_frame or dabgpu_decode_stream_frames, whichever the context serves) returns DABGPU_ERR_HIP
 * before any launch, once; 0 disarms.  What the host mirror must survive: /root/reference/src/radio_block.cpp:27, 37
 * (the two Process calls run on threads nobody can throw to). */
int dabgpu_test_fail_frame_call(dabgpu_ctx *ctx, int nth);

/* Device buffers for a batch user's IQ samples ([n_frames][frame_stride] cf32, frame_stride >= 196608 samples; buffers of
 * integer samples, dabgpu_set_iq_format, are plain device allocations of the caller's) and
 * soft bits ([n_frames][230400] int8).  Any device buffer is accepted by the _dev entry points; this call exists for
 * callers that own their buffers and want them placed for the front end.
 *   placement  DABGPU_PLACE_PLAIN    two hipMallocs.
 *              DABGPU_PLACE_DOMAINS  MI355X's HBM behaves as three domains of 96 GB, and a launch that reads its
 *                samples from the domain it writes its soft bits to runs up to ~10 % slower than one whose two streams
 *                lie apart (profiles/r02_hbm_domains.txt; against a plain pair the front end
 *                gained 0.8-3.9 % in six of six trials, profiles/r04_placement_ab.txt).  Physical memory is taken in
 *                chunks through the virtual-memory API (1 GiB for the samples, 256 MiB for the soft bits; never more
 *                than 1.5 x the pair's size held during set-up), every chunk's domain is found with a small data
 *                mover (two passes, ~40-110 ms), the IQ buffer is mapped over chunks of the most plentiful domain(s)
 *                and every 256 MiB of the soft-bit buffer over a chunk whose domain differs from the ~1.7 GiB of
 *                samples read WHILE it is written; the chunks left over go back.  All of it happens inside two
 *                address ranges per context (one to probe in, one for the pair), reserved by the first such call and
 *                released by dabgpu_destroy: one domain-aware pair per context at a time.  The call then CHECKS its
 *                own result (report->pair_over_same_domain) and, where the pair behaves as one domain -- a box whose
 *                virtual-memory chunks all come from one: the worst case, 2-9 % of the boxes seen --, gives it back
 *                and allocates a plain pair instead: the caller never has to compare.  That case, a second request
 *                while the first pair is alive, a request larger than the range was reserved for, buffers below
 *                ~4 GiB, a device without the virtual-memory API or without room, and any failure on the way all end
 *                in a PLAIN pair (report->method = 0, report->fallback_reason says why).  A set-up call: it
 *                synchronises, takes ~0.1-0.2 s and leaves noise in both buffers.
 * Returns an error only when the plain allocation fails too.  Release with dabgpu_free_frame_buffers (both pointers of
 * a domain-aware pair together). */
#define DABGPU_PLACE_PLAIN   0
#define DABGPU_PLACE_DOMAINS 1
/* report->fallback_reason */
#define DABGPU_PLAIN_REQUESTED    0  /* DABGPU_PLACE_PLAIN was asked for                                   */
#define DABGPU_PLAIN_SIZE         1  /* too small for the domains to matter, or more chunks than are handled */
#define DABGPU_PLAIN_NO_VMM       2  /* the virtual-memory API refused (reserve / map / set access)          */
#define DABGPU_PLAIN_NO_ROOM      3  /* free memory does not hold the chunks                                  */
#define DABGPU_PLAIN_ARENA_BUSY   4  /* the context's domain-aware pair is still alive                        */
#define DABGPU_PLAIN_ARENA_SMALL  5  /* larger than the address range the context reserved on its first call   */
#define DABGPU_PLAIN_PROBE_FAILED 6  /* a probe launch or its timing failed                                    */
#define DABGPU_PLAIN_ONE_DOMAIN   7  /* the placed pair's own check read >= 0.985 (it behaves as one domain: the   */
                                     /* worst case); it was given back and two plain allocations made instead;   */
                                     /* pair_over_same_domain, n_domains, domains describe the pair given back    */
typedef struct dabgpu_placement_report {
    int32_t method;             /* 0 = plain hipMalloc pair, 1 = domain-aware pair                              */
    int32_t fallback_reason;    /* method 0: DABGPU_PLAIN_*                                                     */
    int32_t n_chunks;           /* physical chunks taken during set-up                                         */
    int32_t iq_chunks, soft_chunks;   /* chunks (of either size) each buffer is mapped over                    */
    int32_t n_domains;          /* distinct HBM domains seen among the chunks (1..3)                           */
    int32_t conflicts;          /* per mille of the soft bits that are written beside reads from their own domain */
    int32_t runtime_error;      /* fallback after a failed runtime call: stage * 1000 + hipError_t (stage 1 reserve, */
                                /* 2 create, 3 map, 4 set access, 5 unmap, 6 memory info, 7 / 8 map / set access   */
                                /* of the pair); else 0                                                             */
    uint64_t chunk_bytes;
    uint64_t setup_peak_bytes;  /* device memory held at the peak of the set-up (<= 1.5 x the pair)            */
    float classify_ms;          /* time spent finding the domains                                              */
    float pair_over_same_domain; /* check of the result: a mover reading 3/4 of the samples' first chunk and writing */
                                /* the start of the soft-bit buffer, over the same mover writing into the last 1/4 */
                                /* of that chunk instead (same domain by construction): ~0.9 when the two buffers  */
                                /* lie apart, ~1.0 when they do not (0 = not measured).  A domain-aware pair is   */
                                /* only ever handed out below 0.985; at or above it the pair goes back and the    */
                                /* call ends in a plain pair (DABGPU_PLAIN_ONE_DOMAIN): the caller decides nothing */
    char domains[100];          /* one letter per chunk in allocation order: 'A' 'B' 'C' for the 1 GiB chunks, */
                                /* 'a' 'b' 'c' for the 256 MiB ones; NUL-terminated, cut at 95                  */
    char iq_map[72];            /* the chunks of the IQ buffer in address order, same letters                  */
    char soft_map[28];          /* the chunks of the soft-bit buffer in address order                          */
} dabgpu_placement_report;
int dabgpu_alloc_frame_buffers(dabgpu_ctx *ctx, int n_frames, size_t frame_stride, int placement, void **d_iq,
                               int8_t **d_soft, dabgpu_placement_report *report);
int dabgpu_free_frame_buffers(dabgpu_ctx *ctx, void *d_iq, int8_t *d_soft);

/* The ceiling the front end is measured against: a pure data mover of the front end's own geometry on the caller's
 * buffers -- per frame the useful 2048 samples of each of the 76 symbols (+ the PRS's prefix; with_prefixes != 0: the
 * whole 2552-sample periods, what a launch that produces the cyclic-prefix correlations reads) in, 230400 bytes out,
 * one wavefront per run of symbols cut exactly as dabgpu_ofdm_demod_frames_dev cuts the same batch, streaming
 * accesses, the same LDS footprint (occupancy) -- and no arithmetic.  Overwrites d_soft with meaningless bytes.
 * Time it with events on `stream`; bench.py reports it as roofline.mover_same_geometry_ms. */
/* (cf32 only: DABGPU_ERR_ARG on a context set to another sample format, dabgpu_set_iq_format.) */
int dabgpu_mover_frames_dev(dabgpu_ctx *ctx, const void *d_iq, size_t frame_stride, int n_frames, int8_t *d_soft,
                            int with_prefixes, void *stream);

/* ------------------------------------------------------------------------ */
/* Sample formats of the device-pointer calls (per context; cf32 by default). */
/* ------------------------------------------------------------------------ */
#define DABGPU_IQ_CF32 0  /* interleaved float32 I,Q -- the default, what every call reads unless told otherwise */
#define DABGPU_IQ_CS16 1  /* interleaved int16 I,Q                                                             */
#define DABGPU_IQ_CS8  2  /* interleaved int8 I,Q (HackRF)                                                     */
#define DABGPU_IQ_CU8  3  /* interleaved uint8 I,Q, value = u - 127.5 (rtl_sdr)                                */
/* Sets the format the context's device-pointer calls read their d_iq in; DABGPU_ERR_ARG for an unknown value, or while
 * the context has an open ring (dabgpu_pipe_open sizes its staging slots for the format it finds).
 * The value contract: the kernels convert right after the load, before any arithmetic and without scaling, to
 *   float(i), float(q)            (cs16, cs8)
 *   float(u) - 127.5f             (cu8; exact)
 * so every output -- soft bits, cyclic-prefix correlations, decision-directed sums, stream states, sync results, acquired
 * frames and counts, decoded bytes -- is bit for bit what the cf32 path gives on a cf32 buffer holding the same values.
 * The quantiser and every threshold are relative, so no scale is needed; signal_average (stream states, dabgpu_get_stats)
 * is then in the format's units.  Strides, starts and offsets stay in complex samples.  d_iq needs one complex sample of
 * alignment (4 bytes cs16, 2 bytes cs8 / cu8) and frame_stride may be odd (frames at odd sample offsets are read sample by
 * sample).
 * Reading the format: dabgpu_ofdm_demod_frames_dev, dabgpu_ofdm_demod_frames_dd_dev, dabgpu_ofdm_demod_streams_dev (both
 * loops), dabgpu_sync_prs_dev, dabgpu_acquire_dev, dabgpu_ofdm_demod_acquired_dev, dabgpu_ofdm_demod_tracked_dev (auto_acquire
 * included) and the ring (dabgpu_pipe_*), with or without a soft-bit selection and a d_cyc buffer.
 * Refusing any format but cf32 with DABGPU_ERR_ARG, nothing enqueued: the host-pointer calls (their `const float *` is cf32),
 * dabgpu_ofdm_demod_stream_frame, dabgpu_fft_symbols[_dev], dabgpu_mover_frames_dev, and any call given d_dqpsk != NULL.
 * dabgpu_alloc_frame_buffers sizes cf32 buffers: integer IQ buffers are plain device allocations.
 * dabgpu_get_iq_format returns the context's format (DABGPU_ERR_ARG for a NULL context). */
int dabgpu_set_iq_format(dabgpu_ctx *ctx, int format);
int dabgpu_get_iq_format(const dabgpu_ctx *ctx);

/* ------------------------------------------------------------------------ */
/* A2..A6: OFDM front end on time-aligned frames.                             */
/* Replaces the READING_SYMBOLS work of OFDM_Demod::Process                    */
/*   /root/reference/src/dab_module.cpp:25 (call), src/radio_block.cpp:22 (ctor) */
/* up to the payload of the On_OFDM_Frame callback (src/radio_block.cpp:25).   */
/*                                                                            */
/* iq           cf32; frame f starts (first PRS sample, i.e. after the null    */
/*              symbol) at iq + f*frame_stride complex samples; 76*2552        */
/*              samples are read per frame.  Must be 16-byte aligned and        */
/*              frame_stride even.  The _dev call reads the context's sample    */
/*              format (dabgpu_set_iq_format: then one sample of alignment, any */
/*              stride, no dqpsk); the host call cf32 only.                     */
/* freq_offset  [n_frames] correction in cycles/sample applied as               */
/*              x[n]*exp(+j*2*pi*f*n) (the sum the reference shows as           */
/*              GetNetFrequencyOffset(), src/render_radio_block.cpp:204).       */
/*              Exactly: f is quantised to a 32-bit phase step                  */
/*              dphi = llrint(f*2^32) mod 2^32 (ties to even), and sample n,    */
/*              counted from the frame's first sample (n = 0 at the PRS         */
/*              prefix, prefixes included), is multiplied by                    */
/*              exp(+j*2*pi*frac(n*dphi/2^32)).  The same holds for the stream  */
/*              states' fine + coarse offset (added in float32) and an acquired */
/*              frame's freq_offset.                                            */
/*              NULL = no correction.                                           */
/* soft         [n_frames][230400] int8 (frame bits in transmission order)      */
/* cyc          optional [n_frames][76] cf32: cyclic-prefix correlations        */
/*              sum conj(y[i])*y[i+2048]; their mean angle / (2*pi*2048) is the */
/*              fine frequency error (fine_freq_update_beta loop,               */
/*              src/render_radio_block.cpp:216).                                */
/* dqpsk        optional [n_frames][75][1536] cf32 differential symbols in      */
/*              carrier order -768..768 (GetFrameDataVec(),                     */
/*              src/render_radio_block.cpp:109).                                */
/* ------------------------------------------------------------------------ */
int dabgpu_ofdm_demod_frames_dev(dabgpu_ctx *ctx, const void *d_iq, size_t frame_stride, int n_frames,
                                 const float *d_freq_offset, int8_t *d_soft, void *d_cyc, void *d_dqpsk,
                                 void *stream);
int dabgpu_ofdm_demod_frames(dabgpu_ctx *ctx, const float *iq, size_t frame_stride, int n_frames,
                             const float *freq_offset, int8_t *soft, float *cyc, float *dqpsk);
/* (Serves the fine-frequency loop whose state the GUI reads -- GetFineFrequencyOffset, fine_freq_update_beta,
 * /root/reference/src/render_radio_block.cpp:202, :216 -- with an estimator of this library's own.)
 * The same front end reading ONE cyclic prefix per frame instead of 76 (the prefixes are 20 % of the samples, and the
 * kernel is bound by the bytes it moves), with the decision-directed frequency-error sums a loop needs instead of the
 * cyclic-prefix correlations:
 *   dd4  [n_frames][76] cf32; the SUM of entries 1..75 of a frame = sum over its 75 data symbols and 256 of each
 *        symbol's carriers (FFT bins v + 64 m, v < 64, m in {0, 1, 30, 31}, bin 0 replaced by 768) of u^4, u = the
 *        differential symbol X_l conj X_{l-1} divided by its magnitude (every term has magnitude 1 whatever the level of
 *        the input; |sum| / 19200 is a lock quality between 0 and 1).  How the sum is spread over the entries depends on
 *        how the launch cut the frame into runs: a run's total sits in the entry of its last symbol, its other entries
 *        are 0.  Whatever two bits a differential symbol carries, its fourth power is -exp(j 4 theta) with theta =
 *        2 pi * (residual offset, cycles per sample) * 2552: angle(-sum) / (4 * 2 pi * 2552) is the residual modulo
 *        1 / (4 * 2552) (0.2 carriers).
 *        Entry 0 of a frame = the cyclic-prefix correlation of its PRS (symbol 0; the one prefix that IS read, 0.3 % of
 *        the frame): angle / (2 pi 2048) is the same residual, coarser but unambiguous within half a carrier -- it picks
 *        the branch: residual = e_dd + k / (4 * 2552), k = round((e_cp - e_dd) * 4 * 2552).
 * OPT-IN everywhere: every closed-loop entry point runs the reference's loop (cyclic-prefix correlations) unless told
 * otherwise -- the tracked and frame calls through dabgpu_track_cfg.decision_directed = 1, the stream call and the ring after
 * dabgpu_set_stream_loop(..., decision_directed = 1) -- and only when the caller does not ask for the correlations
 * (d_cyc == NULL). */
int dabgpu_ofdm_demod_frames_dd_dev(dabgpu_ctx *ctx, const void *d_iq, size_t frame_stride, int n_frames,
                                    const float *d_freq_offset, int8_t *d_soft, void *d_dd4, void *stream);

/* ------------------------------------------------------------------------ */
/* Closed-loop front end: per-stream tracking state kept in device memory.    */
/* Replaces the fine-frequency loop of OFDM_Demod and the scalars the GUI      */
/* reads from it: GetFineFrequencyOffset / GetCoarseFrequencyOffset /          */
/* GetNetFrequencyOffset / GetSignalAverage / GetTotalFramesRead /             */
/* GetTotalFramesDesync and fine_freq_update_beta                              */
/*   (/root/reference/src/render_radio_block.cpp:202-207, :216).               */
/*                                                                            */
/* A context owns `n_streams` states (dabgpu_streams_reset).  The stream call  */
/* demodulates frames_per_stream consecutive frames of every stream with the   */
/* stream's current fine + coarse offset -- no host-supplied frequency -- and  */
/* then, on the device and in stream order, moves the fine offset by           */
/* -beta * (mean angle of the frames' cyclic-prefix correlations)/(2*pi*2048), */
/* kept within +-half a carrier; the next call uses the new value.  Frame      */
/* (s, f) starts at iq + (s*frames_per_stream + f)*frame_stride.               */
/* cyc may be NULL: the library keeps what the loop needs in its own scratch --  */
/* the correlations, or (dabgpu_set_stream_loop(.., decision_directed = 1)) the  */
/* dd4 sums, in which case only the PRS's cyclic prefix is read.                  */
/* ------------------------------------------------------------------------ */
typedef struct dabgpu_stream_state {      /* DEVICE memory, 64 bytes */
    float fine_freq_offset;               /* cycles/sample, within +-0.5/2048                     */
    float coarse_freq_offset;             /* cycles/sample (whole carriers: -k/2048)              */
    float signal_average;                 /* running mean of |re|+|im| per sample                 */
    float last_fine_error;                /* residual the most recent call measured, cycles/sample */
    int32_t total_frames_read;
    int32_t total_frames_desync;          /* frames lost: level below thresh_null_start x average, PRS not found, */
                                          /* or (tracked calls) begun before the capture did                      */
    int32_t tracking;                     /* tracked calls: 1 = next_frame_start is valid                         */
    int32_t last_time_offset;             /* tracked calls: where the most recent frame's impulse-response peak    */
                                          /* sat relative to the predicted position, samples                       */
    double next_frame_start;              /* first sample of the next frame (PRS prefix minus timing_margin),      */
                                          /* relative to the first sample of the NEXT capture                      */
    float drift;                          /* samples per frame the frame period differs from 196608                */
    float last_peak_to_mean;              /* impulse-response peak / mean of the most recent frame                 */
    int32_t loop_gated;                   /* decision-directed loop: calls whose fourth-power estimate was gated    */
                                          /* (quality below the gate: the PRS prefix alone was used; or a one-step  */
                                          /* branch departure held back) -- see dabgpu_set_loop_gate                */
    int32_t dd_branch;                    /* branch of the most recent accepted estimate, units of 0.2 carriers     */
    int32_t dd_pending;                   /* a one-step departure from branch 0 seen once (0x7fffffff: none)        */
    int32_t reserved;
} dabgpu_stream_state;

typedef struct dabgpu_stats {             /* HOST copy with the derived fields the GUI prints */
    int32_t state;                        /* OFDM_Demod::State value: 0 before the first frame (and after a tracked */
                                          /* stream lost every frame of a call), 4 = READING_SYMBOLS               */
    float fine_freq_offset;
    float coarse_freq_offset;
    float net_freq_offset;
    float signal_average;
    int32_t total_frames_read;
    int32_t total_frames_desync;
    float last_fine_error;
    int32_t tracking;
    int32_t last_time_offset;
    double next_frame_start;
    float drift;
    float last_peak_to_mean;
    int32_t loop_gated;                   /* see dabgpu_stream_state                                                */
    int32_t reserved;
} dabgpu_stats;

/* (re)create the context's stream states, all zero */
int dabgpu_streams_reset(dabgpu_ctx *ctx, int n_streams);
/* the states in device memory ([n_streams]), e.g. to seed them from a kernel of the caller's; NULL before a reset */
dabgpu_stream_state *dabgpu_stream_states(dabgpu_ctx *ctx);
/* host-side setter (synchronises the context stream): NULL = leave that offset as it is.  The host mirror stores the
 * coarse offset found at acquisition here (is_coarse_freq_correction, src/render_radio_block.cpp:215). */
int dabgpu_set_stream_offsets(dabgpu_ctx *ctx, int stream_index, const float *fine, const float *coarse);
/* (Reads d_iq in the context's sample format, dabgpu_set_iq_format; d_dqpsk needs cf32.  The host call: cf32 only.) */
int dabgpu_ofdm_demod_streams_dev(dabgpu_ctx *ctx, const void *d_iq, size_t frame_stride, int n_streams,
                                  int frames_per_stream, float fine_freq_update_beta, int8_t *d_soft, void *d_cyc,
                                  void *d_dqpsk, void *stream);
int dabgpu_ofdm_demod_streams(dabgpu_ctx *ctx, const float *iq, size_t frame_stride, int n_streams,
                              int frames_per_stream, float fine_freq_update_beta, int8_t *soft, float *cyc,
                              float *dqpsk);
/* the seven scalars of src/render_radio_block.cpp:192-207 for one stream.  Ordering: the states are read and written
 * by the stream calls on whatever stream those were given; dabgpu_get_stats, dabgpu_set_stream_offsets and
 * dabgpu_streams_reset first wait (on the host) for the most recent such call to finish, wherever it ran. */
int dabgpu_get_stats(dabgpu_ctx *ctx, int stream_index, dabgpu_stats *out);
/* signal_l1.update_beta (src/render_radio_block.cpp:235) and null_l1_search.thresh_null_start (:226-233) of the stream
 * calls' level average and desync count (defaults 0.95 / 0.35), and which estimator the fine-frequency loop of
 * dabgpu_ofdm_demod_streams_dev runs on when the caller passes no correlation buffer (d_cyc == NULL):
 *   decision_directed == 0 (default)  the cyclic-prefix correlations, kept in the library's scratch: pulls in from
 *                                     +-half a carrier, as the reference's loop does
 *   decision_directed != 0            the dd4 sums of dabgpu_ofdm_demod_frames_dd_dev: of the 76 cyclic prefixes of a frame
 *                                     only the PRS's is read (17 % fewer bytes); it resolves the sums' 0.2-carrier
 *                                     ambiguity, so this loop, too, pulls in from +-half a carrier and may run from
 *                                     the first call on.  Off by default: the drop-in path keeps the reference's
 *                                     data flow; this one is the library's own, opt-in. */
int dabgpu_set_stream_loop(dabgpu_ctx *ctx, float signal_update_beta, float thr_null_start, int decision_directed);
/* The decision-directed loop checks its own estimate before it moves (stream call here; tracked and frame calls:
 * dabgpu_track_cfg.dd_gate).  With S = the call's sum of unit fourth powers over n terms:
 *   quality  |S| < dd_gate * sqrt(n) -- what n random phases add up to, times the gate (2.5 by default): the sum carries no
 *            usable phase (single frames below ~3 dB SNR, nothing selected) and the call takes the cyclic-prefix
 *            estimate of its PRSs alone -- unbiased, coarser; 0 switches this gate off.
 *   branch   a stream whose previous residual lay inside +-0.1 carriers and whose PRS prefix now asks for the branch one
 *            step (0.2 carriers) away is believed only when the next call asks again; the first time the branch is held.
 * Either event counts in loop_gated (dabgpu_get_stats).  The loop on the cyclic-prefix correlations -- the reference's
 * estimator, fine_freq_update_beta at /root/reference/src/render_radio_block.cpp:216 -- has no such ambiguity and no gate. */
int dabgpu_set_loop_gate(dabgpu_ctx *ctx, float dd_gate);

/* Soft-bit selection (batch receivers that decode the FIC and a few sub-channels and never look at the rest of the
 * frame): from the next call on, dabgpu_ofdm_demod_frames[_dev], dabgpu_ofdm_demod_streams[_dev] and
 * dabgpu_ofdm_demod_acquired_dev of this context write only the listed parts of each frame's 230400 soft bits and leave the other bytes of `soft` untouched -- in
 * device memory and, for the host-pointer call, in the caller's host buffer (only the selected ranges are copied
 * back).  Symbols that carry no selected bit and are not the differential reference of one that does are not
 * transformed at all (their cyclic-prefix correlation is still produced when `cyc` is asked for).  The reference's
 * OFDM_Demod always emits whole frames (/root/reference/src/radio_block.cpp:25); its BasicRadio then reads the
 * FIC and the selected sub-channels only (:42) -- this moves that choice in front of the 230 kB store.
 *   ranges    frame-bit coordinates [first, first+count), both multiples of 16, inside 0..230400
 *   n_ranges  0 = write everything again (the default)
 * Calls with a constellation output (dqpsk != NULL) ignore the selection.  Not to be changed while a demodulation
 * call of this context is still running on some stream.
 * dabgpu_soft_selection writes the ranges of the FIC (with_fic != 0) and of the given sub-channels (4 CIFs each)
 * to `out` and returns how many there are (more than max_out = nothing written beyond max_out), or a negative
 * status for a bad sub-channel. */
struct dabgpu_subchannel;             /* defined with the MSC entry points below */
typedef struct dabgpu_bit_range {
    int32_t first;
    int32_t count;
} dabgpu_bit_range;
int dabgpu_ofdm_set_soft_selection(dabgpu_ctx *ctx, const dabgpu_bit_range *ranges, int n_ranges);
int dabgpu_soft_selection(const struct dabgpu_subchannel *subchannels, int n_subchannels, int with_fic,
                          dabgpu_bit_range *out, int max_out);

/* A2+A3 alone (the unfused "FFT stage"): frequency-corrected 2048-point forward
 * FFT of the useful part of each of the 76 symbols.  Replaces the FFTW3f plan the
 * reference links (/root/reference/CMakeLists.txt:55-64).
 * spectra  [n_frames][76][2048] cf32, unnormalised, natural bin order. */
/* (cf32 only: DABGPU_ERR_ARG on a context set to another sample format, dabgpu_set_iq_format.) */
int dabgpu_fft_symbols_dev(dabgpu_ctx *ctx, const void *d_iq, size_t frame_stride, int n_frames,
                           const float *d_freq_offset, void *d_spectra, void *stream);
int dabgpu_fft_symbols(dabgpu_ctx *ctx, const float *iq, size_t frame_stride, int n_frames,
                       const float *freq_offset, float *spectra);

/* ------------------------------------------------------------------------ */
/* Frame synchronisation on the phase reference symbol.      */
/* Replaces the RUNNING_COARSE_FREQ_SYNC and RUNNING_FINE_TIME_SYNC work of    */
/* OFDM_Demod (/root/reference/src/render_radio_block.cpp:195-196) and its     */
/* knobs is_coarse_freq_correction / max_coarse_freq_correction_norm /         */
/* impulse_peak_threshold_db (:213-231).                                       */
/*                                                                            */
/* iq            candidate f starts at iq + f*frame_stride: the caller's guess */
/*               of the FIRST sample of the PRS cyclic prefix; 2552 samples    */
/*               are read.  16-byte aligned, frame_stride even.                */
/* freq_offset   [n] correction applied before the search (NULL = none)        */
/* max_coarse    search range in carriers, 0..1023                             */
/* out[f].coarse_carriers  integer carrier offset k of the signal: apply       */
/*               -k/2048 cycles/sample as coarse correction                    */
/* out[f].time_offset      the PRS useful part starts at candidate + 504 +     */
/*               time_offset samples (signed, -1024..1023)                     */
/* out[f].peak_to_mean     impulse-response peak / mean power (threshold it    */
/*               like impulse_peak_threshold_db)                               */
/* out[f].coarse_peak_to_mean  same for the coarse correlation                 */
/* A window whose correlation (or impulse response) is zero everywhere -- an   */
/* all-zero window -- gives coarse_carriers 0 (time_offset 0) and ratio 0, so   */
/* it fails every positive threshold and never carries a NaN into a stream's   */
/* state.  The results are the same bit for bit for any 2^k scaling of the     */
/* input: the correlations are normalised by a power of two before squaring.   */
/* ------------------------------------------------------------------------ */
typedef struct dabgpu_sync_result {
    int32_t coarse_carriers;
    int32_t time_offset;
    float peak_to_mean;
    float coarse_peak_to_mean;
} dabgpu_sync_result;

/* (Reads d_iq in the context's sample format, dabgpu_set_iq_format.  The host call: cf32 only.) */
int dabgpu_sync_prs_dev(dabgpu_ctx *ctx, const void *d_iq, size_t frame_stride, int n_frames,
                        const float *d_freq_offset, int max_coarse, dabgpu_sync_result *d_out, void *stream);
int dabgpu_sync_prs(dabgpu_ctx *ctx, const float *iq, size_t frame_stride, int n_frames, const float *freq_offset,
                    int max_coarse, dabgpu_sync_result *out);

/* ------------------------------------------------------------------------ */
/* Acquisition on unaligned captures: everything OFDM_Demod   */
/* does before READING_SYMBOLS -- FINDING_NULL_POWER_DIP, READING_NULL_AND_PRS, */
/* RUNNING_COARSE_FREQ_SYNC, RUNNING_FINE_TIME_SYNC                            */
/* (/root/reference/src/render_radio_block.cpp:193-196; knobs                  */
/* thresh_null_start/end, max_coarse_freq_correction_norm,                     */
/* impulse_peak_threshold_db at :213-235) -- for whole captures at once.        */
/*                                                                            */
/* iq       stream s = iq + s*stream_stride complex samples, n_samples each;    */
/*          any 8-byte aligned position (no frame alignment assumed)            */
/* out      [n_streams][max_frames]: one entry per null symbol found whose      */
/*          frame lies inside the capture, in time order; entries past          */
/*          counts[s] have flags 0 and start -1                                 */
/*   start            first sample of the PRS cyclic prefix minus               */
/*                    cfg.timing_margin, relative to the stream                 */
/*   freq_offset      correction to hand to the demodulator, cycles/sample      */
/*                    (= fine_offset - coarse_carriers/2048)                    */
/*   fine_offset      from the cyclic prefix of the PRS, (-0.5..0.5]/2048       */
/*   flags            bit 0: impulse peak_to_mean >= cfg.min_peak_to_mean       */
/*                    bit 1: all 76 symbols lie inside the capture              */
/* dabgpu_ofdm_demod_acquired_dev demodulates exactly those frames (A2..A6 as   */
/* dabgpu_ofdm_demod_frames): soft [n_streams*max_frames][230400]; entries      */
/* whose flags are not 3 give all-zero (erased) soft bits.                      */
/* ------------------------------------------------------------------------ */
typedef struct dabgpu_acquire_cfg {
    float thr_null_start;        /* dip begins below this fraction of the mean block L1 norm (0.35) */
    float thr_null_end;          /* and ends above this one (0.75)                                   */
    int32_t min_null_blocks;     /* shortest dip, in 64-sample blocks, taken for a null symbol (30)  */
    int32_t max_coarse_carriers; /* coarse search range (200)                                        */
    float min_peak_to_mean;      /* lock threshold on the impulse response (30 = 14.8 dB)            */
    int32_t timing_margin;       /* samples the FFT windows are kept inside the cyclic prefix (64)   */
    /* which tap of the channel impulse response a frame is aligned to:                                  */
    float impulse_peak_distance_probability; /* taps are scored |h|^2 w^2, w = 1 - (1 - p) |offset - expected| / 2552 */
                                 /* (src/render_radio_block.cpp:225; 0.15; 1 = unweighted)           */
    float first_path_rel;        /* > 0: the earliest tap within 504 samples before the scored peak  */
                                 /* with at least max(rel x peak power, 16 x mean) replaces it, so   */
                                 /* that a stronger LATE echo still falls inside the cyclic prefix   */
                                 /* (0.25 = -6 dB); 0 = the scored peak itself, the reference's rule */
    int32_t level_chunk_blocks;  /* the null thresholds follow the LOCAL level: mean block norm over    */
                                 /* chunks of this many 64-sample blocks, averaged over chunks c-2..c+2 */
                                 /* (power of two, 64..16384; 256 = 8 ms chunks, a 40 ms window) -- the   */
                                 /* batch counterpart of the reference's running average                */
                                 /* (signal_l1.update_beta, :235); 0 = the mean of the whole capture     */
    int32_t reserved;
} dabgpu_acquire_cfg;

typedef struct dabgpu_acquired_frame {
    int64_t start;
    float freq_offset;
    int32_t coarse_carriers;
    float fine_offset;
    float peak_to_mean;
    float coarse_peak_to_mean;
    int32_t flags;
} dabgpu_acquired_frame;

void dabgpu_acquire_default_cfg(dabgpu_acquire_cfg *cfg);
/* (dabgpu_acquire_dev and dabgpu_ofdm_demod_acquired_dev read d_iq in the context's sample format, dabgpu_set_iq_format;
 * d_dqpsk needs cf32.  The host call dabgpu_acquire: cf32 only.) */
int dabgpu_acquire_dev(dabgpu_ctx *ctx, const void *d_iq, size_t stream_stride, int n_streams, int64_t n_samples,
                       const dabgpu_acquire_cfg *cfg, int max_frames, dabgpu_acquired_frame *d_out, int32_t *d_counts,
                       void *stream);
int dabgpu_acquire(dabgpu_ctx *ctx, const float *iq, size_t stream_stride, int n_streams, int64_t n_samples,
                   const dabgpu_acquire_cfg *cfg, int max_frames, dabgpu_acquired_frame *out, int32_t *counts);
int dabgpu_ofdm_demod_acquired_dev(dabgpu_ctx *ctx, const void *d_iq, size_t stream_stride, int n_streams,
                                   int max_frames, const dabgpu_acquired_frame *d_frames, int8_t *d_soft, void *d_cyc,
                                   void *d_dqpsk, void *stream);

/* ------------------------------------------------------------------------ */
/* Timing tracking: what OFDM_Demod's RUNNING_FINE_TIME_SYNC state does on     */
/* every frame once locked (/root/reference/src/render_radio_block.cpp:196;    */
/* knobs impulse_peak_threshold_db, impulse_peak_distance_probability,         */
/* :224-225) -- for batches of streams, with the position kept on the device.  */
/*                                                                            */
/* A stream is acquired ONCE (dabgpu_acquire_dev on its first capture, then     */
/* dabgpu_track_start_dev).  Every later capture goes through                  */
/* dabgpu_ofdm_demod_tracked_dev alone: per stream, the frames the state        */
/* predicts inside the capture (start_i = next_frame_start + i*(196608+drift)) */
/* are synchronised on their own PRS (impulse response -> exact start, lock),   */
/* demodulated where they lie with the stream's fine + coarse offset, and the   */
/* state is moved on: fine-frequency loop (on the cyclic-prefix correlations, as  */
/* the reference's; cfg.decision_directed = 1 and d_cyc == NULL: on the dd4 sums), */
/* next_frame_start and drift from a line through the measured starts.         */
/*   n_samples  samples per stream in this capture                             */
/*   advance    the next capture of every stream will begin this many samples   */
/*              after this one began.  Frames are only taken whole (+512        */
/*              samples), so consecutive captures must overlap by at least one  */
/*              frame + 512 + the drift: advance <= n_samples - 197632.         */
/*   frames     [n_streams][max_frames] as dabgpu_acquire_dev writes them        */
/*              (flags 3 = demodulated); counts[s] = frame slots of stream s     */
/*              that lay inside the capture.  soft / cyc / dqpsk as             */
/*              dabgpu_ofdm_demod_acquired_dev (slots without a locked frame:    */
/*              erased soft bits).  cyc may be NULL (cfg.decision_directed       */
/*              then chooses what the fine loop runs on).                        */
/* A stream none of whose frames locked in a call stops tracking (state 0 in     */
/* dabgpu_get_stats): acquire it again -- or set cfg.auto_acquire and the next   */
/* call does (then the very first call needs no dabgpu_acquire_dev either).      */
/* ------------------------------------------------------------------------ */
typedef struct dabgpu_track_cfg {
    float fine_freq_update_beta;              /* 0.9                                                   */
    float signal_update_beta;                 /* signal_l1.update_beta, 0.95                           */
    float thr_null_start;                     /* 0.35                                                  */
    float min_peak_to_mean;                   /* impulse_peak_threshold_db as a power ratio (100)      */
    float impulse_peak_distance_probability;  /* 0.15, see dabgpu_acquire_cfg                          */
    float first_path_rel;                     /* 0.25, see dabgpu_acquire_cfg                          */
    float drift_beta;                         /* share of a measured drift error taken per call (0.5)  */
    float coarse_freq_slow_beta;              /* frame call: see below (0.1)                           */
    int32_t timing_margin;                    /* 64 (batch calls); the frame call uses the host's own   */
    int32_t max_coarse_carriers;              /* frame call and auto-acquisition: whole-carrier search */
                                              /* range, 0 = off (204)                                  */
    int32_t decision_directed;                /* 0 (default) = the fine loop runs on the cyclic-prefix */
                                              /* correlations, the reference's estimator               */
                                              /* (fine_freq_update_beta, render_radio_block.cpp:216);   */
                                              /* 1 = tracked / frame call with d_cyc == NULL: on the    */
                                              /* dd4 sums, only the PRS's cyclic prefix is read -- this */
                                              /* library's own estimator, opt-in (ABI v6; v5: default 1) */
    int32_t auto_acquire;                     /* tracked call: != 0 = streams that are not tracking    */
                                              /* (never acquired, or lost) are ACQUIRED inside the     */
                                              /* call -- null-symbol search + PRS on their capture as  */
                                              /* dabgpu_acquire_dev does, their frames demodulated     */
                                              /* with the others', their tracking started; streams     */
                                              /* that are tracking cost nothing extra.  One call does  */
                                              /* everything from the first capture on (0)              */
    float dd_gate;                            /* decision-directed loop: quality gate, see             */
                                              /* dabgpu_set_loop_gate (2.5; 0 = off)                   */
    int32_t reserved;                         /* must be 0                                             */
} dabgpu_track_cfg;
void dabgpu_track_default_cfg(dabgpu_track_cfg *cfg);
/* only_lost != 0: streams that are tracking keep their state (re-acquisition of the lost ones beside them) */
int dabgpu_track_start_dev(dabgpu_ctx *ctx, const dabgpu_acquired_frame *d_frames, const int32_t *d_counts, int n_streams,
                           int max_frames, int64_t advance, int only_lost, void *stream);
/* (Reads d_iq in the context's sample format, dabgpu_set_iq_format, auto_acquire included; d_dqpsk needs cf32.) */
int dabgpu_ofdm_demod_tracked_dev(dabgpu_ctx *ctx, const void *d_iq, size_t stream_stride, int n_streams,
                                  int64_t n_samples, int max_frames, int64_t advance, const dabgpu_track_cfg *cfg,
                                  int8_t *d_soft, void *d_cyc, void *d_dqpsk, dabgpu_acquired_frame *d_frames,
                                  int32_t *d_counts, void *stream);

/* One frame of one stream from host memory, everything in ONE call: what OFDM_Demod does between "76 symbols are in
 * the buffer" and the On_OFDM_Frame callback (RUNNING_COARSE_FREQ_SYNC / RUNNING_FINE_TIME_SYNC / READING_SYMBOLS,
 * /root/reference/src/render_radio_block.cpp:195-197; src/radio_block.cpp:25).  One upload of the frame; on the
 * device: synchronisation on the PRS, the coarse-offset update, demodulation with the stream's offsets, fine loop,
 * counters, level; one download of {soft bits, sync result, statistics}; one synchronisation.
 *   iq         76 * 2552 cf32 as the caller assembled them: iq[0] is its guess of the first PRS prefix sample,
 *              `cfg->timing_margin` samples early.  Any host memory; page-locked buffers (dabgpu_host_alloc) aligned to
 *              16 bytes -- `iq` and `soft` both -- are read / written by kernels in line with the others (no copy-engine
 *              hand-over, no copy by the CPU afterwards): ~10 % less time per call
 *   acquiring  != 0: first frame after a null-symbol detection -- the stream's fine offset is set from this PRS's own
 *              cyclic prefix (so that already this frame is demodulated with it) and the whole-carrier offset found on
 *              this PRS is STORED as its coarse offset (cfg->max_coarse_carriers > 0); 0: a residual of k carriers
 *              moves the coarse offset by coarse_freq_slow_beta * k
 *   result->flags  bit 0 = PRS found (peak_to_mean >= min_peak_to_mean), bit 1 = the FFT windows lie inside the
 *              cyclic prefix (0 <= sync.time_offset <= 488); only a frame with both is demodulated (others: erased
 *              soft bits, counted as desync)
 *   dqpsk      optional [75][1536] cf32 (GetFrameDataVec) */
typedef struct dabgpu_frame_result {
    dabgpu_sync_result sync;
    int32_t flags;
    int32_t reserved;
    dabgpu_stats stats;
} dabgpu_frame_result;
/* (cf32 only: DABGPU_ERR_ARG on a context set to another sample format, dabgpu_set_iq_format.) */
int dabgpu_ofdm_demod_stream_frame(dabgpu_ctx *ctx, int stream_index, const float *iq, int acquiring,
                                   const dabgpu_track_cfg *cfg, int8_t *soft, float *dqpsk, dabgpu_frame_result *result);

/* ------------------------------------------------------------------------ */
/* A7..A11: FIC.  Replaces the FIC branch of BasicRadio::Process              */
/*   /root/reference/src/radio_block.cpp:42 (call), :60 (ctor).               */
/* soft      frame f's bits start at soft + f*soft_stride; the first 9216 are  */
/*           the FIC (4 groups of 2304).                                       */
/* fib       [n_frames][12][32] bytes (30 data + CRC16), energy dispersal       */
/*           removed                                                           */
/* crc_ok    [n_frames][12] 1 = CRC matches                                    */
/* ------------------------------------------------------------------------ */
int dabgpu_fic_decode_dev(dabgpu_ctx *ctx, const int8_t *d_soft, size_t soft_stride, int n_frames,
                          uint8_t *d_fib, uint8_t *d_crc_ok, void *stream);
int dabgpu_fic_decode(dabgpu_ctx *ctx, const int8_t *soft, size_t soft_stride, int n_frames,
                      uint8_t *fib, uint8_t *crc_ok);

/* ------------------------------------------------------------------------ */
/* A12: one MSC subchannel.  Replaces the per-subchannel branch of             */
/* BasicRadio::Process (/root/reference/src/radio_block.cpp:42); the           */
/* descriptor mirrors the Subchannel entity the GUI prints                     */
/* (/root/reference/src/render_formatters.cpp:9-25).  Any size up to a         */
/* sub-channel that fills the CIF (864 capacity units).                        */
/* ------------------------------------------------------------------------ */
typedef struct dabgpu_subchannel {
    int32_t start_address;   /* first capacity unit (0..863)                  */
    int32_t length;          /* size in capacity units                        */
    int32_t is_uep;          /* 0 = EEP (long form), 1 = UEP (short form)     */
    int32_t eep_type;        /* EEP: 0 = A, 1 = B                             */
    int32_t protection_level;/* EEP 1..4; UEP 1..5                            */
    int32_t bitrate_kbps;    /* EEP: multiple of 8 (A) / 32 (B); UEP: one of  */
                             /* the 14 rates of the protection profile table  */
} dabgpu_subchannel;

/* UEP sub-channels are announced by an index into the standard's table of 64 protection profiles
 * (FIG 0/1 short form, `uep_prot_index` in the reference's Subchannel entity,
 * /root/reference/src/render_formatters.cpp:9-25): fills bit rate, level and size from it. */
int dabgpu_uep_subchannel(int table_index, int start_address, dabgpu_subchannel *out);

/* bytes one CIF of this subchannel decodes to (bitrate*3), or <0 */
int dabgpu_subchannel_bytes(const dabgpu_subchannel *sc);

/* n_streams independent ensembles, frames_per_stream consecutive frames each;
 * frame (s,f) is at soft + (s*frames_per_stream+f)*soft_stride.
 * history_in / history_out  [n_streams][15][length*64] int8: the subchannel's bits of the
 *           15 CIFs before / at the end of this call (time de-interleaver state, 16-CIF
 *           depth).  history_in may be NULL (treated as erasures); they must not alias.
 * out       [n_streams][frames_per_stream*4][bitrate*3] bytes; entry t is the logical
 *           frame completed by CIF t, i.e. the one transmitted 15 CIFs earlier. */
int dabgpu_msc_decode_dev(dabgpu_ctx *ctx, const dabgpu_subchannel *sc, const int8_t *d_soft,
                          size_t soft_stride, int n_streams, int frames_per_stream,
                          const int8_t *d_history_in, int8_t *d_history_out, uint8_t *d_out, void *stream);
int dabgpu_msc_decode(dabgpu_ctx *ctx, const dabgpu_subchannel *sc, const int8_t *soft,
                      size_t soft_stride, int n_streams, int frames_per_stream,
                      const int8_t *history_in, int8_t *history_out, uint8_t *out);

/* Whole-ensemble variant: decode `n_subchannels` subchannels of the same frames in one
 * call (all on one stream; EEP-A, EEP-B and UEP profiles).  Per subchannel i:
 *   history_in[i] / history_out[i]   as above, may be NULL pointers inside the arrays
 *   out[i]                           [n_streams][frames_per_stream*4][bitrate_i*3]
 * The three pointer arrays are HOST arrays of DEVICE pointers.  Subchannels must not overlap in the CIF. */
int dabgpu_msc_decode_multi_dev(dabgpu_ctx *ctx, const dabgpu_subchannel *sc, int n_subchannels,
                                const int8_t *d_soft, size_t soft_stride, int n_streams, int frames_per_stream,
                                const int8_t *const *d_history_in, int8_t *const *d_history_out,
                                uint8_t *const *d_out, void *stream);

/* A7..A12 in one call: what BasicRadio::Process does with a frame (/root/reference/src/radio_block.cpp:42) --
 * the FIC and every listed sub-channel -- for a whole batch of frames.  Arguments as dabgpu_fic_decode_dev and
 * dabgpu_msc_decode_multi_dev.  Large batches whose streams are a multiple of 16 frames long put the FIC and all
 * sub-channels through one pair of launches (their codewords then share the machine instead of queueing up behind
 * each other); any other shape is decoded part by part with the same results. */
int dabgpu_decode_frames_dev(dabgpu_ctx *ctx, const int8_t *d_soft, size_t soft_stride, int n_streams,
                             int frames_per_stream, uint8_t *d_fib, uint8_t *d_crc_ok, const dabgpu_subchannel *sc,
                             int n_subchannels, const int8_t *const *d_history_in, int8_t *const *d_history_out,
                             uint8_t *const *d_out, void *stream);

/* ------------------------------------------------------------------------ */
/* A batch of DIFFERENT ensembles (a monitoring receiver, a band scan): every  */
/* stream has its own multiplex -- its own number of sub-channels, start       */
/* addresses, sizes and protection profiles.                                    */
/*                                                                            */
/* dabgpu_decode_ensembles_dev  dabgpu_decode_frames_dev with one sub-channel   */
/*            list PER STREAM.  Streams that are a multiple of 16 frames long,   */
/*            with the alignment a grouped launch wants (soft bits, history in   */
/*            on 16 bytes, outputs on 4), put the FIC of all frames and every     */
/*            (stream, sub-channel) pair through ONE forward and ONE traceback     */
/*            launch, whatever their number, and all history rings through a       */
/*            third; any other shape is decoded part by part, stream by stream,     */
/*            with the same results.  Checks and status codes per stream as         */
/*            dabgpu_decode_frames_dev; everything is checked before anything is     */
/*            enqueued, so a refused call leaves every output as it was.              */
/* dabgpu_fig_subchannels  (host) the list to pass for one stream, read from the  */
/*            FIBs an earlier call decoded: FIC pass with no entries, this        */
/*            function per stream, then the call with the plans                    */
/*            (INTEGRATION.md section 13).                                        */
/* ------------------------------------------------------------------------ */
/* n_streams ensembles, each with ITS OWN sub-channel list, in one call.
 * sc        all lists one after the other (HOST); stream s owns entries sc_first[s] .. sc_first[s+1]-1
 * sc_first  [n_streams + 1] (HOST), sc_first[0] = 0, non-decreasing; a stream may own no entry (FIC only);
 *           at most 64 entries per stream
 * per entry j of stream s (HOST arrays of DEVICE pointers, sc_first[n_streams] long):
 *   d_history_in[j] / d_history_out[j]   [15][length_j*64] int8, as dabgpu_msc_decode_dev for ONE stream; the arrays or
 *                                        single pointers may be NULL (in: erasures); in != out
 *   d_out[j]                             [frames_per_stream*4][bitrate_j*3]
 * d_fib / d_crc_ok as dabgpu_decode_frames_dev, or both NULL (sub-channels only).
 * Entries of ONE stream must not overlap in the CIF; entries of different streams may use the same capacity units. */
int dabgpu_decode_ensembles_dev(dabgpu_ctx *ctx, const int8_t *d_soft, size_t soft_stride, int n_streams,
                                int frames_per_stream, uint8_t *d_fib, uint8_t *d_crc_ok,
                                const dabgpu_subchannel *sc, const int32_t *sc_first,
                                const int8_t *const *d_history_in, int8_t *const *d_history_out,
                                uint8_t *const *d_out, void *stream);

/* host only: the sub-channel organisation (FIG 0/1, current configuration, C/N = 0) found in CRC-clean FIBs of ONE
 * ensemble, sorted by start address, each sub-channel once; short form through dabgpu_uep_subchannel, long form
 * option 0 = EEP-A / 1 = EEP-B with the bit rate its size and level imply (a reserved option is passed over).
 * fib [n_frames][12][32], crc_ok [n_frames][12].  *n receives the count;
 * DABGPU_ERR_CAPACITY if max is too small, DABGPU_ERR_PROFILE if an announced pair names no profile. */
int dabgpu_fig_subchannels(const uint8_t *fib, const uint8_t *crc_ok, int n_frames, dabgpu_subchannel *out, int max, int *n);

/* host only: which of those sub-channels carry audio, and which kind -- what the reference lists per service before it
 * shows a DAB+ channel's flags (/root/reference/src/render_radio_block.cpp:414-437 are drawn for the sub-channels whose
 * component says ASCTy 63).  FIG 0/2 (clause 6.3.1), both P/D forms, current configuration of this ensemble (C/N = 0,
 * OE = 0): the MSC stream audio components (TMId = 0), joined through FIG 0/1 to the start address the entries of
 * dabgpu_fig_subchannels carry.  Each SubChId once (its first component), sorted by start address; a component whose
 * sub-channel the same FIBs have not announced (or announce with a reserved long-form option) is left out.
 * *n receives the count; DABGPU_ERR_CAPACITY if max is too small (nothing written). */
typedef struct dabgpu_audio_component {
    uint32_t sid;               /* 16-bit (P/D = 0) or 32-bit (P/D = 1) service identifier */
    int32_t subchid;
    int32_t start_address;      /* CU, as dabgpu_subchannel.start_address                 */
    int32_t ascty;              /* 0 = DAB (MPEG layer II), 63 = DAB+ (HE-AAC super-frames) */
    int32_t primary;            /* P/S flag                                                */
    int32_t reserved[3];
} dabgpu_audio_component;
int dabgpu_fig_audio_components(const uint8_t *fib, const uint8_t *crc_ok, int n_frames, dabgpu_audio_component *out, int max,
                                int *n);

/* Host-pointer form for the plugin's one-frame-at-a-time use (BasicRadio::Process, src/radio_block.cpp:42): the
 * frames are uploaded ONCE, the FIC and every sub-channel are decoded from that copy, the results come back in one
 * batch of copies, one synchronisation.  history_in / history_out / out are HOST arrays of HOST pointers. */
int dabgpu_decode_frames(dabgpu_ctx *ctx, const int8_t *soft, size_t soft_stride, int n_streams, int frames_per_stream,
                         uint8_t *fib, uint8_t *crc_ok, const dabgpu_subchannel *sc, int n_subchannels,
                         const int8_t *const *history_in, int8_t *const *history_out, uint8_t *const *out);

/* The same for ONE stream fed frame after frame, as the plugin does: the time de-interleaver state of every listed
 * sub-channel stays on the device between calls (keyed by start address and size; a sub-channel seen for the first
 * time starts from erasures, and so does one that was left out of the previous call: a ring that misses a frame no
 * longer continues the stream and is dropped), so a call is one upload of the soft bits, the decode, one download of
 * all results.
 * dabgpu_decode_stream_reset drops the kept state (Radio_Block::reset_radio). */
int dabgpu_decode_stream_frames(dabgpu_ctx *ctx, const int8_t *soft, size_t soft_stride, int n_frames, uint8_t *fib,
                                uint8_t *crc_ok, const dabgpu_subchannel *sc, int n_subchannels, uint8_t *const *out);
int dabgpu_decode_stream_reset(dabgpu_ctx *ctx);

/* ------------------------------------------------------------------------ */
/* Reception quality ("Reception quality"): two figures from   */
/* what the front end and the decoder already left on the device, for every    */
/* front-end entry point and every decoder.                                     */
/*                                                                            */
/* MER  of the quantised differential constellation, per frame, equal-weighted  */
/*      over carriers: with a = |soft[n]|, b = |soft[1536 + n]| of carrier n of  */
/*      a data symbol, signal = sum (a+b)^2, error = sum (a-b)^2 over the       */
/*      carriers whose pair is not (0, 0) (erased).  MER in dB =                */
/*      10 log10(signal / error) (+inf when error is 0).  Not channel SNR: the   */
/*      phase error of the differential symbol, which saturates at high SNR      */
/*      through the quantiser's truncation.                                      */
/* BER  before the Viterbi decoder, per codeword: the decoded bits are          */
/*      scrambled and encoded again, punctured as the profile says and compared  */
/*      with the hard decisions of the soft bits the decoder read; erased bits   */
/*      are not counted.  A codeword the decoder got wrong re-encodes to other   */
/*      bits than were sent, and its count is then too low (the FIB CRC shows    */
/*      it for the FIC).                                                         */
/* ------------------------------------------------------------------------ */
typedef struct dabgpu_mer {      /* per frame, 24 bytes */
    uint64_t signal;             /* sum (|re|+|im|)^2 over counted carriers           */
    uint64_t error;              /* sum (|re|-|im|)^2                                  */
    int32_t  carriers;           /* carriers counted (not erased)                      */
    int32_t  reserved;
} dabgpu_mer;

typedef struct dabgpu_ber_count {  /* per codeword */
    uint32_t errors;             /* kept mother bits whose soft bit has the wrong sign */
    uint32_t bits;               /* kept mother bits with a soft bit != 0              */
} dabgpu_ber_count;

/* MER of data symbols [first_symbol, first_symbol + n_symbols) (within 0..74) of n_frames frames (frame f's soft bits
 * at d_soft + f*soft_stride, as the front end wrote them) -> d_out[n_frames].  d_soft and soft_stride multiples of 16
 * bytes, d_out of 8.  Symbols 0..2 (the FIC) are the cheap figure of a monitor; with a soft-bit selection
 * (dabgpu_ofdm_set_soft_selection) only selected symbols hold what the front end wrote. */
int dabgpu_mer_dev(dabgpu_ctx *ctx, const int8_t *d_soft, size_t soft_stride, int n_frames, int first_symbol, int n_symbols,
                   dabgpu_mer *d_out, void *stream);

/* Channel BER of a decode call that has been enqueued before it on the same stream (dabgpu_decode_frames_dev,
 * dabgpu_fic_decode_dev, dabgpu_msc_decode_dev / _multi_dev): the same soft bits, frame shape, sub-channels and history_in.
 *   d_fib     that call's FIBs, or NULL: no FIC count;  d_fic [n_streams*frames_per_stream][4], one per FIC codeword
 *             (3 FIBs)
 *   d_out[i]  sub-channel i's decoded bytes;  d_msc[i] [n_streams][frames_per_stream*4], aligned with d_out: entry t
 *             counts logical frame t - 15, whose bits lie in CIFs t-15..t (with d_history_in NULL the first 15 entries
 *             of a stream count only the bits of this call's CIFs)
 * Pointer arrays are HOST arrays of DEVICE pointers (d_history_in may be NULL, and so may its entries); sub-channels must
 * not overlap.  One launch for the FIC and up to 16 sub-channels. */
int dabgpu_channel_ber_dev(dabgpu_ctx *ctx, const int8_t *d_soft, size_t soft_stride, int n_streams, int frames_per_stream,
                           const uint8_t *d_fib, dabgpu_ber_count *d_fic, const dabgpu_subchannel *sc, int n_subchannels,
                           const int8_t *const *d_history_in, const uint8_t *const *d_out, dabgpu_ber_count *const *d_msc,
                           void *stream);

/* dabgpu_decode_stream_frames with the quality of the same frames, in the same batch of downloads and behind the same
 * synchronisation (the de-interleaver rings this call reads live inside the context: a caller could not count the
 * sub-channels' BER afterwards).  HOST outputs, each NULL = not computed:
 *   fic_ber     [n_frames][4]
 *   msc_ber[i]  [n_frames*4] for sub-channel i (the array NULL, or single entries NULL)
 *   mer         [n_frames], all 75 data symbols (the whole frame is uploaded then, not only the ranges the decode reads)
 * With every quality output NULL this IS dabgpu_decode_stream_frames. */
int dabgpu_decode_stream_frames_quality(dabgpu_ctx *ctx, const int8_t *soft, size_t soft_stride, int n_frames, uint8_t *fib,
                                        uint8_t *crc_ok, const dabgpu_subchannel *sc, int n_subchannels, uint8_t *const *out,
                                        dabgpu_ber_count *fic_ber, dabgpu_ber_count *const *msc_ber, dabgpu_mer *mer);

/* ------------------------------------------------------------------------ */
/* Transmitter identification (TII, EN 300 401 section 14.8, Mode I): which   */
/* transmitters of a single-frequency network are received, and how strongly,  */
/* from the combs they put into the null symbol.  Comb c (sub-identifier,       */
/* 0..23) and position b (0..7) own the carrier pairs k = B + 2c + 48b, k + 1   */
/* for B in {-768, -384, 1, 385}; pattern p (main identifier, 0..69) switches  */
/* on four of the eight positions (dabgpu_tii_pattern: bit 7 - b = position b). */
/*                                                                            */
/* Per frame the 2048 samples [-2352, -304) before the first sample of the PRS  */
/* prefix are corrected in frequency and transformed; with P(k) = |X_k|^2:      */
/*   cell[c][b]  sum of P over the 8 carriers of (c, b)                         */
/*   floor       mean P over the noise bins 776 <= |k| <= 927                   */
/* The calls ADD each stream's frames, in frame order, to d_acc[stream] (zero   */
/* it to start; no atomics: the sums repeat bit for bit).  d_frame, when not    */
/* NULL, receives every frame's own record ([n_streams][frames_per_stream],     */
/* frames = 1, or 0 for a skipped slot, whose sums are 0).  d_iq is read in the */
/* context's sample format (dabgpu_set_iq_format); the records are the same    */
/* for every format holding the same values.                                    */
/*                                                                            */
/* dabgpu_tii_frames_dev    frame (s, f) as the front end has it: its PRS      */
/*            prefix at d_iq + (s*frames_per_stream + f)*frame_stride (>= 2656  */
/*            when there is more than one frame); the caller guarantees the      */
/*            2656 samples before every frame are readable.  d_freq_offset       */
/*            [n_frames] cycles/sample as dabgpu_ofdm_demod_frames_dev takes it,  */
/*            or NULL: each stream's fine + coarse offset from the context's      */
/*            stream states, what dabgpu_ofdm_demod_streams_dev would apply if    */
/*            enqueued next (DABGPU_ERR_ARG without stream states,                */
/*            DABGPU_ERR_CAPACITY for more streams than there are states).        */
/* dabgpu_tii_acquired_dev  the slots dabgpu_acquire_dev / _tracked_dev wrote    */
/*            ([n_streams][max_frames]) with their start and freq_offset; the    */
/*            PRS prefix is at start + timing_margin (the margin the slots were   */
/*            found with, 0..504).  Counted: flags == 3 and the window inside the  */
/*            capture (start + timing_margin >= 2352); other slots add nothing.   */
/* dabgpu_tii_decode        host only (no context, no device): level(c, b) =    */
/*            cell / (8 floor) - 1, the estimated SNR of a TII carrier; a cell is */
/*            on at level >= 10^(min_level_db / 10).  A pattern whose four cells  */
/*            are on is an entry {p, c, 10 log10(mean of its four levels),        */
/*            AMBIGUOUS when its comb has more than four cells on}.  Entries by    */
/*            level descending (ties: sub_id, then main_id ascending).  Returns    */
/*            how many there are (none for frames == 0 or floor <= 0; nothing      */
/*            written beyond max_out), DABGPU_ERR_ARG for a NULL acc, a NULL out   */
/*            with max_out > 0, max_out < 0 or a min_level_db that is not finite. */
/*            cfg NULL = the defaults.                                           */
/* Refusals (DABGPU_ERR_ARG / _CAPACITY) enqueue nothing and leave the outputs   */
/* untouched.  The tables restate the standard from memory: the pattern bit     */
/* order and the bases are not checked against it.   */
/* ------------------------------------------------------------------------ */
typedef struct dabgpu_tii_acc {   /* DEVICE memory, 784 bytes: a stream's sums, or one frame's record */
    float cell[24][8];            /* sum over frames of the cell energies                             */
    float floor;                  /* sum over frames of the mean noise-bin power                      */
    int32_t frames;               /* frames added                                                     */
    int32_t reserved[2];          /* left as they are by the calls; 0 in per-frame records            */
} dabgpu_tii_acc;

typedef struct dabgpu_tii_cfg {
    float min_level_db;           /* a cell is on at this TII-carrier SNR or more (3.0) */
    int32_t reserved;             /* 0 */
} dabgpu_tii_cfg;

#define DABGPU_TII_AMBIGUOUS 1    /* the comb has more than four cells on (e.g. two transmitters share the sub-identifier) */
typedef struct dabgpu_tii_entry {
    int32_t main_id;              /* pattern p, 0..69     */
    int32_t sub_id;               /* comb c, 0..23        */
    float level_db;               /* 10 log10(mean level) */
    int32_t flags;                /* DABGPU_TII_*         */
} dabgpu_tii_entry;

void dabgpu_tii_default_cfg(dabgpu_tii_cfg *cfg);
/* the 8-bit mask of pattern p (bit 7 - b = position b), -1 outside 0..69 */
int dabgpu_tii_pattern(int p);
int dabgpu_tii_frames_dev(dabgpu_ctx *ctx, const void *d_iq, size_t frame_stride, int n_streams, int frames_per_stream,
                          const float *d_freq_offset, dabgpu_tii_acc *d_frame, dabgpu_tii_acc *d_acc, void *stream);
int dabgpu_tii_acquired_dev(dabgpu_ctx *ctx, const void *d_iq, size_t stream_stride, int n_streams, int max_frames,
                            const dabgpu_acquired_frame *d_frames, int timing_margin, dabgpu_tii_acc *d_frame,
                            dabgpu_tii_acc *d_acc, void *stream);
int dabgpu_tii_decode(const dabgpu_tii_acc *acc, const dabgpu_tii_cfg *cfg, dabgpu_tii_entry *out, int max_out);

/* ------------------------------------------------------------------------ */
/* Channel impulse response (CIR, Mode I) from the phase reference symbol:    */
/* where the paths of a single-frequency network arrive and how strongly.     */
/*                                                                            */
/* Per frame the 2048 samples [504, 2552) after the first sample of the PRS   */
/* prefix (the front end's window) are corrected in frequency as the TII      */
/* calls do (nco(n, round(f 2^32)), n from the window start) and transformed  */
/* (X, unnormalised).  Over the 1536 carriers k = -768..768, k != 0, with the */
/* Hann taper w(k) = 0.5 + 0.5 cos(pi k / 769), S = sum of w (= 768) and the   */
/* PRS R (dabgpu_get_prs_reference):                                          */
/*   h[n]       = sqrt(1536) / (2048 S) sum_k w(k) X[k] conj R[k]             */
/*                exp(+2 pi i k n / 2048),  n = 0..2047                       */
/*   tap[n]     = |h[n]|^2  (a path of gain g at integer delay d, unit mean    */
/*                sample power: tap[d] = |g|^2)                               */
/*   carrier[i] = (1536 / 2048^2) |X[k]|^2, untapered, i = 0..1535 for         */
/*                k = -768..-1, 1..768 (1.0 on a flat unit-gain channel)       */
/* Tap n is the delay from the window start; n >= 1024 reads as n - 2048      */
/* (arrivals before the timing reference).  The taper keeps the sidelobes of   */
/* a path off the sample grid from reading as echoes.                          */
/* The calls ADD each stream's frames, in frame order, to d_acc[stream] (zero */
/* it to start; no atomics: the sums repeat bit for bit, with or without       */
/* d_frame).  d_frame, when not NULL, receives every frame's own record        */
/* ([n_streams][frames_per_stream], frames = 1, or an all-zero record for a    */
/* skipped slot); NULL needs no scratch from the caller.  d_iq is read in the  */
/* context's sample format (dabgpu_set_iq_format); the records are the same    */
/* for every format holding the same values.                                   */
/*                                                                            */
/* dabgpu_cir_frames_dev    frame (s, f) has its PRS prefix at d_iq +         */
/*            (s*frames_per_stream + f)*frame_stride (even and >= 2552 when    */
/*            there is more than one frame); the caller guarantees the 2552    */
/*            samples from every prefix are readable.  d_freq_offset           */
/*            [n_frames] cycles/sample, whole-carrier part included, as        */
/*            dabgpu_ofdm_demod_frames_dev takes it, or NULL: each stream's     */
/*            fine + coarse offset from the context's stream states            */
/*            (DABGPU_ERR_ARG without stream states, DABGPU_ERR_CAPACITY for   */
/*            more streams than there are states).                            */
/* dabgpu_cir_acquired_dev  the slots dabgpu_acquire_dev / _tracked_dev wrote  */
/*            ([n_streams][max_frames]) with their start and freq_offset; the  */
/*            PRS prefix is at start + timing_margin (0..504).  Counted:       */
/*            flags == 3 and start + timing_margin >= 0; other slots add       */
/*            nothing.                                                        */
/* dabgpu_cir_analyse       host only (no context, no device), on            */
/*            p[n] = tap[n] / frames:                                         */
/*            floor = median(p) / m(F), F = frames, m(F) = 1 - 1/(3F) +         */
/*              8/(405 F^2) (the median of a mean of F unit exponentials; the  */
/*              median is the mean of the 1024th and 1025th smallest p);       */
/*            peak = max p.  Tap n (indices circular) is a path when           */
/*              p[n] > p[n-1], p[n] >= p[n+1], p[n] >= floor 10^(min_snr_db/10) */
/*              and p[n] >= peak 10^(-range_db/10).  Its delay is the signed   */
/*              tap plus 0.5 (L- - L+) / (L- - 2 L0 + L+) on                  */
/*              L = 10 log10(max(p, 1e-30)); level_db = 10 log10(p[n] / peak), */
/*              snr_db = 10 log10(p[n] / floor); BEYOND_GUARD when             */
/*              delay - first_delay > 504.  Paths by delay ascending.          */
/*            report (may be NULL): rms_delay_spread weighted by the paths'    */
/*              p (0 for one path); guard_ratio_db = 10 log10 of the power of  */
/*              the paths within 504 samples of the first over the power of    */
/*              those beyond (+inf when none is beyond); with no paths every   */
/*              field after peak is 0.  Returns the number of paths (none for   */
/*              frames == 0 or floor <= 0; nothing written beyond max_out),    */
/*              DABGPU_ERR_ARG for a NULL acc, a NULL out with max_out > 0,    */
/*              max_out < 0 or a cfg value that is not finite.  cfg NULL = the */
/*              defaults.                                                     */
/* Refusals (DABGPU_ERR_ARG / _CAPACITY) enqueue nothing and leave the outputs   */
/* untouched.                                      */
/* ------------------------------------------------------------------------ */
typedef struct dabgpu_cir_acc {   /* DEVICE memory, 14 352 bytes: a stream's sums, or one frame's record */
    float tap[2048];              /* sum over frames of |h[n]|^2                                         */
    float carrier[1536];          /* sum over frames of the normalised |X_k|^2                           */
    int32_t frames;               /* frames added                                                        */
    int32_t reserved[3];          /* left as they are by the calls; 0 in per-frame records               */
} dabgpu_cir_acc;

typedef struct dabgpu_cir_cfg {
    float min_snr_db;             /* a path stands this far above the noise floor (10.0)      */
    float range_db;               /* and no further than this below the strongest tap (25.0)  */
} dabgpu_cir_cfg;

typedef struct dabgpu_cir_report {
    int32_t frames, n_paths;
    float floor, peak;            /* per-frame mean tap power: noise floor estimate, strongest tap      */
    float first_delay, strongest_delay, rms_delay_spread;   /* samples                                   */
    float guard_ratio_db;         /* power of paths within 504 samples of the first / power beyond      */
} dabgpu_cir_report;

#define DABGPU_CIR_BEYOND_GUARD 1 /* the path arrives more than 504 samples (the guard interval) after the first */
typedef struct dabgpu_cir_path {
    float delay;                  /* samples from the window start, signed, interpolated */
    float level_db;               /* relative to the strongest tap                       */
    float snr_db;                 /* relative to the noise floor                         */
    int32_t flags;                /* DABGPU_CIR_*                                        */
} dabgpu_cir_path;

void dabgpu_cir_default_cfg(dabgpu_cir_cfg *cfg);
int dabgpu_cir_frames_dev(dabgpu_ctx *ctx, const void *d_iq, size_t frame_stride, int n_streams, int frames_per_stream,
                          const float *d_freq_offset, dabgpu_cir_acc *d_frame, dabgpu_cir_acc *d_acc, void *stream);
int dabgpu_cir_acquired_dev(dabgpu_ctx *ctx, const void *d_iq, size_t stream_stride, int n_streams, int max_frames,
                            const dabgpu_acquired_frame *d_frames, int timing_margin, dabgpu_cir_acc *d_frame,
                            dabgpu_cir_acc *d_acc, void *stream);
int dabgpu_cir_analyse(const dabgpu_cir_acc *acc, const dabgpu_cir_cfg *cfg, dabgpu_cir_report *report,
                       dabgpu_cir_path *out, int max_out);

/* ------------------------------------------------------------------------ */
/* ETI(NI) output: what a decode call left on the  */
/* device, written as one 6144-byte ETI(NI) frame per 24 ms CIF -- the FIC of   */
/* that CIF, the sub-channel table and every listed sub-channel's bytes, the    */
/* header and the data each under a CRC -- ready to be downloaded or written to */
/* a file as it is.  All multi-bit fields big-endian, MSB first:               */
/*   0   1  ERR    0xFF all three FIBs passed their CRC, 0xE1 otherwise,        */
/*                 0x00 warm-up frame                                          */
/*   1   3  FSYNC  07 3A B6 (FCT even) / F8 C5 49 (FCT odd)                    */
/*   4   1  FCT    CIF count modulo 250                                        */
/*   5   1  FICF (1 bit) = 1, NST (7) = number of streams                      */
/*   6   2  FP (3) = CIF count modulo 8, MID (2) = 1, FL (11) = NST + 1 + 24 +  */
/*                 2 * sum STL                                                 */
/*   8   4 NST  STC per stream: SCID (6), SAD (10), TPL (6), STL (10) =         */
/*                 bitrate_kbps * 3 / 8; streams by ascending SAD              */
/*   ..  2  MNSC = FFFF;   2  CRC over bytes 4 .. end of MNSC                  */
/*   ..  96 FIC: the CIF's three FIBs as the FIC decoder wrote them            */
/*   ..  8 STL per stream: its bytes of this CIF as the MSC decoder wrote them */
/*   ..  2  CRC over FIC + stream bytes;  2  RFU = FFFF;  4  TIST = FFFFFFFF    */
/*   ..  0x55 up to 6144                                                       */
/* TPL: UEP 0x10 | (level - 1); EEP 0x20 | (eep_type << 2) | (level - 1).  Both */
/* CRCs are the FIB's (x^16 + x^12 + x^5 + 1, start FFFF, inverted).           */
/*                                                                            */
/* Alignment.  A frame carries the FIC and the sub-channel bytes of the SAME    */
/* transmitted CIF.  Entry t of a sub-channel's decoder output is the logical   */
/* frame transmitted at CIF t - 15 of the call, and the FIC is not interleaved: */
/* output frame t = FIC of CIF t - 15 + every sub-channel's entry t.  The FIC   */
/* of a call's last 15 CIFs waits in a per-stream history record               */
/* (dabgpu_eti_history) for the next call, exactly as the de-interleaver state   */
/* does: d_history_in / d_history_out [n_streams] records, 8-byte aligned, must */
/* not alias; d_history_in may be NULL, and an all-zero record means the same   */
/* (a stream that starts here).  Frames whose CIF lies before the start of the  */
/* stream are WARM-UP frames: written, well-formed, both CRCs right, ERR = 0x00, */
/* a zero FIC, DABGPU_ETI_WARMUP in their status.                               */
/*                                                                            */
/* CIF count.  Per stream and call the ANCHOR is the first CIF of the call whose */
/* first FIB passed its CRC and begins with FIG 0/0 (05 00 EId EId, 5 bits of    */
/* the upper count, 8 of the lower); CIF c of the call then counts              */
/* count(anchor) + c - anchor modulo 5000 (upper modulo 20, lower modulo 250),   */
/* the CIFs of the history included.  Without an anchor the call's first CIF    */
/* continues the history's count, or is 0 without a history                     */
/* (DABGPU_ETI_NO_ANCHOR on every frame of that stream and call).  A frame whose  */
/* own first FIB is valid, begins with FIG 0/0 and says another count keeps the   */
/* anchored one and gets DABGPU_ETI_COUNT_MISMATCH (a reconfigured or spliced     */
/* stream).  d_cif_start, when not NULL, is [n_streams]: an entry >= 0 is the     */
/* count of that stream's first CIF of this call and overrides anchor and history */
/* (modulo 5000); a negative entry leaves the stream to the rule above.           */
/*                                                                            */
/* dabgpu_eti_layout   host only (no context, no device).  Validates n          */
/*            sub-channels, orders them by start address and builds the part of   */
/*            the header every frame of a call shares.  DABGPU_ERR_ARG for        */
/*            n > 64, an id outside 0..63, a size outside the CIF, overlapping     */
/*            sub-channels, a bit rate that is not a positive multiple of 8 (or    */
/*            above 2728: STL has 10 bits), a level outside 1..4 (EEP) / 1..5      */
/*            (UEP), an eep_type outside 0..1, or a frame longer than 6144 bytes.  */
/*            The sub-channel's size and protection are NOT held to its bit rate   */
/*            here (the decode call does that).  n = 0 is a frame with the FIC only. */
/* dabgpu_eti_frames_dev   after a decode call on the same stream (d_fib          */
/*            [n_streams*frames_per_stream][12][32], d_crc_ok [..][12], d_out[i]    */
/*            [n_streams][frames_per_stream*4][bitrate_i*3] exactly as it wrote    */
/*            them).  d_out is a HOST array of plan->nst DEVICE pointers (8-byte    */
/*            aligned) in the order the sub-channels were given to                  */
/*            dabgpu_eti_layout -- the decode call's order; plan->order maps the    */
/*            frame's streams to it.  Writes d_eti [n_streams][frames_per_stream*4] */
/*            [6144] (16-byte aligned) and d_status [n_streams][frames_per_stream*4] */
/*            (8-byte aligned).  Two launches, no synchronisation.  A refused call   */
/*            (DABGPU_ERR_ARG) enqueues nothing.                                     */
/* dabgpu_eti_parse    host only.  Checks one 6144-byte frame -- FSYNC and its      */
/*            parity, FICF, MID, FL against the STC, the length, both CRCs -- and    */
/*            gives its parts.  Returns DABGPU_OK, DABGPU_ERR_ARG for a NULL         */
/*            argument, or a positive DABGPU_ETI_BAD_* (info is filled as far as the  */
/*            check that failed).  ERR, MNSC, RFU, TIST and the padding are not       */
/*            judged.                                                                */
/* ------------------------------------------------------------------------ */
#define DABGPU_ETI_FRAME_BYTES 6144
#define DABGPU_ETI_MAX_STREAMS 64
#define DABGPU_ETI_FIC_DELAY 15        /* CIFs a stream's FIC waits for its sub-channels */

typedef struct dabgpu_eti_stream {
    int32_t subchannel_id;             /* SCID, 0..63 (FIG 0/1) */
    dabgpu_subchannel sc;
} dabgpu_eti_stream;

typedef struct dabgpu_eti_plan {
    int32_t nst;                       /* streams per frame                                          */
    int32_t fl;                        /* FL: 32-bit words of STC + MNSC/CRC + FIC + stream data     */
    int32_t header_bytes;              /* 12 + 4 nst: bytes before the FIC                           */
    int32_t data_bytes;                /* sum of the streams' bytes per CIF                          */
    int32_t length;                    /* 4 fl + 16: bytes before the 0x55 padding                   */
    int32_t reserved[3];               /* 0                                                          */
    int32_t order[DABGPU_ETI_MAX_STREAMS];   /* order[k]: index, in the caller's list, of stream k    */
    int32_t offset[DABGPU_ETI_MAX_STREAMS];  /* byte offset of stream k's data behind the FIC          */
    int32_t bytes[DABGPU_ETI_MAX_STREAMS];   /* 8 STL of stream k = bitrate * 3                        */
    uint8_t header[16 + 4 * DABGPU_ETI_MAX_STREAMS]; /* bytes 0 .. header_bytes - 1 with ERR, FSYNC,   */
                                       /* FCT, FP and the CRC left 0                                 */
} dabgpu_eti_plan;

#define DABGPU_ETI_WARMUP         1    /* the CIF lies before the start of the stream: zero FIC, ERR = 0x00 */
#define DABGPU_ETI_FIB_CRC        2    /* one of the three FIBs failed its CRC                              */
#define DABGPU_ETI_NO_ANCHOR      4    /* no FIG 0/0 in this call: the count runs on from the history or 0   */
#define DABGPU_ETI_COUNT_MISMATCH 8    /* the frame's own FIG 0/0 says another count                         */
typedef struct dabgpu_eti_status {     /* per frame, 8 bytes */
    uint16_t cif_count;                /* upper * 250 + lower, 0..4999                               */
    uint8_t  flags;                    /* DABGPU_ETI_*                                               */
    uint8_t  fib_ok;                   /* bit j = FIB j passed its CRC                               */
    uint16_t length;                   /* bytes before the padding                                   */
    uint16_t reserved;                 /* 0                                                          */
} dabgpu_eti_status;

typedef struct dabgpu_eti_history {    /* DEVICE memory, per stream, 1504 bytes */
    uint8_t fib[DABGPU_ETI_FIC_DELAY][96];    /* the FIC groups of the call's last 15 CIFs, oldest first    */
    uint8_t crc_ok[DABGPU_ETI_FIC_DELAY][3];  /* their CRC flags                                            */
    uint8_t pad[3];
    int32_t next_count;                /* CIF count of the first CIF of the next call                */
    int32_t valid;                     /* how many of the 15 slots hold a CIF (the newest ones); 0:  */
                                       /* nothing here, next_count included                          */
                                       /* A record the library did not write is read like this: valid */
                                       /* below 0 counts as 0, above 15 as 15; next_count is taken as  */
                                       /* an unsigned 32-bit number modulo 5000 (-1 counts as 2295).   */
                                       /* No value of either makes a call read outside the record.     */
    int32_t reserved[2];
} dabgpu_eti_history;

#define DABGPU_ETI_BAD_SYNC       1    /* FSYNC is neither pattern, or not the one FCT's parity asks for */
#define DABGPU_ETI_BAD_HEADER     2    /* FICF, MID, NST or FL do not fit each other or the frame        */
#define DABGPU_ETI_BAD_HEADER_CRC 3
#define DABGPU_ETI_BAD_DATA_CRC   4
typedef struct dabgpu_eti_info {
    int32_t err, fct, fp, mid, nst, fl;
    int32_t length;                    /* 4 fl + 16                                                  */
    int32_t fic_offset;                /* where the 96 FIC bytes begin                               */
    int32_t header_crc, data_crc;      /* as stored in the frame                                     */
    int32_t reserved[2];
    int32_t scid[DABGPU_ETI_MAX_STREAMS], sad[DABGPU_ETI_MAX_STREAMS], tpl[DABGPU_ETI_MAX_STREAMS],
            stl[DABGPU_ETI_MAX_STREAMS];
    int32_t offset[DABGPU_ETI_MAX_STREAMS];  /* where stream k's 8 stl bytes begin in the frame       */
} dabgpu_eti_info;

int dabgpu_eti_layout(const dabgpu_eti_stream *streams, int n, dabgpu_eti_plan *plan);
size_t dabgpu_eti_history_bytes(void);     /* sizeof(dabgpu_eti_history) */
int dabgpu_eti_frames_dev(dabgpu_ctx *ctx, const dabgpu_eti_plan *plan, int n_streams, int frames_per_stream,
                          const uint8_t *d_fib, const uint8_t *d_crc_ok, const uint8_t *const *d_out,
                          const dabgpu_eti_history *d_history_in, dabgpu_eti_history *d_history_out,
                          const int32_t *d_cif_start, uint8_t *d_eti, dabgpu_eti_status *d_status, void *stream);
int dabgpu_eti_parse(const uint8_t *frame, dabgpu_eti_info *info);

/* ------------------------------------------------------------------------ */
/* ETI(NI) to IQ: the way back.  n_streams         */
/* ensembles of frames_per_stream transmission frames each; ensemble s gives    */
/* 4 * frames_per_stream ETI frames d_eti[s][t][6144] laid out as above, and    */
/* transmission frame f is made of ETI frames 4f .. 4f + 3:                      */
/*   FIC   the 96 FIC bytes of ETI frame 4f + j are codeword j: energy          */
/*         dispersal, the K = 7 rate-1/4 mother code with six tail bits, the     */
/*         FIC puncturing (2304 bits); four codewords = the first 9216 bits.     */
/*   MSC   a sub-channel's 8 STL bytes of ETI frame r: energy dispersal, the     */
/*         mother code, its EEP-A / EEP-B / UEP puncturing, zero padding to       */
/*         64 * size bits = coded[r].  Bit i of the sub-channel in the CIF of     */
/*         ETI frame t is coded[t - D(i mod 16)][i], D = 0 8 4 12 2 10 6 14 1 9   */
/*         5 13 3 11 7 15, t counted from the start of the stream ACROSS calls;   */
/*         a frame before the start gives 0.  The sub-channel lies at CIF bits    */
/*         64 SAD ..; every other CIF bit is 0.  CIF j follows the FIC at bit     */
/*         9216 + 55296 j.                                                        */
/*   OFDM  75 blocks of 3072 bits; block l - 1 gives q_n = ((1 - 2 p_n) +        */
/*         j (1 - 2 p_(n+1536))) / sqrt 2 on carrier k_n of the frequency         */
/*         interleaver, z_l = z_(l-1) q with z_0 the phase reference symbol;      */
/*         every symbol is the inverse FFT at unit mean power behind its 504      */
/*         prefix samples.  The frame: 2656 null samples, the PRS, 75 data        */
/*         symbols = 196 608 cf32 samples, times cfg->gain.                        */
/*   null  zeros, or with cfg->tii_main (0..69) and cfg->tii_sub (0..23) set the   */
/*         TII symbol of that transmitter (its 32 carriers with the PRS's phase,   */
/*         extended cyclically over the 2656 samples).                             */
/* An ETI frame is TAKEN when its FSYNC is one of the two patterns and its         */
/* FICF/NST, MID/FL and STC words are the plan's; any other frame is modulated     */
/* as 96 zero FIC bytes and zero stream bytes and named in the status.  CRCs are   */
/* not checked here (dabgpu_eti_parse does, on the host).  A transmission frame    */
/* whose first ETI frame has FP mod 4 != 0 is flagged and modulated all the same.  */
/*                                                                                */
/* dabgpu_eti_streams_from_frame   host only.  The list dabgpu_eti_layout takes,    */
/*            read back from one frame's STC (in the frame's order): SCID, start    */
/*            address, bit rate from STL, protection from TPL, the size from the    */
/*            EEP profile or the UEP table row.  streams holds 64 entries, *n       */
/*            receives NST.  DABGPU_ERR_ARG for NST > 64 or a TPL/STL pair that      */
/*            names no profile.                                                      */
/* dabgpu_mod_default_cfg   gain 1, tii_main = tii_sub = -1 (a null symbol of zeros). */
/* dabgpu_mod_state_bytes   size of the per-stream device record that carries the    */
/*            time interleaver from call to call (what the next call needs of the    */
/*            last 15 CIFs).  All zero = a stream that starts.                        */
/* dabgpu_modulate_eti_dev   plan and streams: what dabgpu_eti_layout gave and took   */
/*            (every sub-channel's size must be its profile's).  d_eti 16-byte        */
/*            aligned.  d_state_in / d_state_out [n_streams] records, either may be    */
/*            NULL (in: the streams start here), 16-byte aligned, not the same.        */
/*            d_iq [n_streams*frames_per_stream] frames, frame_stride complex samples  */
/*            apart (>= 196608, even), 16-byte aligned; samples between frames are not */
/*            touched.  d_status [n_streams*frames_per_stream], 8-byte aligned.         */
/*            Four launches (five when the TII table changes), no synchronisation;     */
/*            a refused call (DABGPU_ERR_ARG / DABGPU_ERR_PROFILE) enqueues nothing.    */
/* ------------------------------------------------------------------------ */
#define DABGPU_MOD_BAD_INPUT  1        /* at least one of the four ETI frames was not taken      */
#define DABGPU_MOD_MISALIGNED 2        /* FP of the first ETI frame is not a multiple of 4       */
typedef struct dabgpu_mod_status {     /* per transmission frame, 8 bytes */
    uint32_t flags;                    /* DABGPU_MOD_*                                               */
    uint8_t  refused;                  /* bit j = ETI frame 4f + j was not taken                     */
    uint8_t  reserved[3];              /* 0                                                          */
} dabgpu_mod_status;

typedef struct dabgpu_mod_cfg {
    float   gain;                      /* every sample is multiplied by it                           */
    int32_t tii_main, tii_sub;         /* main 0..69 and sub 0..23 identifier, or both -1            */
    int32_t reserved;                  /* 0                                                          */
} dabgpu_mod_cfg;

typedef struct dabgpu_mod_state dabgpu_mod_state;    /* DEVICE memory, opaque, dabgpu_mod_state_bytes() each */

int dabgpu_eti_streams_from_frame(const uint8_t *frame, dabgpu_eti_stream *streams, int *n);
void dabgpu_mod_default_cfg(dabgpu_mod_cfg *cfg);
size_t dabgpu_mod_state_bytes(void);
int dabgpu_modulate_eti_dev(dabgpu_ctx *ctx, const dabgpu_eti_plan *plan, const dabgpu_eti_stream *streams,
                            const dabgpu_mod_cfg *cfg, int n_streams, int frames_per_stream, const uint8_t *d_eti,
                            const dabgpu_mod_state *d_state_in, dabgpu_mod_state *d_state_out, float *d_iq,
                            size_t frame_stride, dabgpu_mod_status *d_status, void *stream);

/* ------------------------------------------------------------------------ */
/* ETI(NI) input: ETI(NI) byte streams read back   */
/* into what the decode call leaves -- FIBs with CRC flags and every            */
/* sub-channel's logical frames -- so that the FIG functions and every follow   */
/* call (d_in / in_stride) run on a recording or a multiplexer's output as they  */
/* do behind the channel decoder.  A batch of entries, each a stream with its    */
/* own multiplex.  The input is a BYTE STREAM: cut anywhere, bytes missing in    */
/* the middle.  The contract -- stream, verdicts, candidates, the walk, rows,    */
/* status, state -- is written out in include/dabgpu_eti_read.h, which the       */
/* kernels, the host twin and the host mirror all run.  In short, per entry:     */
/*   S = the state's carried tail (0..6143 bytes) + the n_bytes new bytes; at    */
/*   most max_frames = (6143 + n_bytes) / 6144 rows.  A position is a CANDIDATE  */
/*   when FSYNC, its parity against FCT, the header fields and the header CRC    */
/*   hold.  From p = 0: a candidate gives a row and p += 6144; otherwise the walk */
/*   resynchronises on the next candidate (skipped, resyncs).  What is left      */
/*   (at most 6143 bytes) is the new tail and is judged again by the next call.   */
/*   Row r with verdict 0 is TAKEN: its FIC to d_fib[r], the three FIB CRC flags  */
/*   (computed here, the FIC decoder's rule) to d_crc_ok[r], stream k's bytes to  */
/*   d_out[k][r] for every d_out[k] that is not NULL (the caller's order, as      */
/*   dabgpu_eti_frames_dev takes it through plan->order).  A row whose data CRC    */
/*   fails (4) or whose NST, FL or STC differ from the plan's                     */
/*   (DABGPU_ETI_OTHER_PLAN) keeps its place in time with zero FIC, flags and     */
/*   stream rows: the follow calls see a lost frame.  Rows behind the emitted      */
/*   count are not written.  plan NULL is the discovery pass: only the FIC is      */
/*   extracted; dabgpu_eti_streams_from_frame reads the multiplex from a taken     */
/*   frame, whose offset in S is in its status.                                    */
/* Frames missing by FCT are NOT replaced by zero rows: after byte loss the         */
/* entries of a call emit different row counts (status gap says how many frames     */
/* are missing in front of a row).                                                  */
/*                                                                                */
/* dabgpu_eti_read_state_bytes   size of the per-entry state record (a head with    */
/*            the tail length, the last row's FCT and FP and the running totals,     */
/*            then the tail).  All zero = a stream that starts.  Written whole.  A    */
/*            record the library did not write makes no call read outside it (a      */
/*            tail length above 6143 counts as 6143).                                 */
/* dabgpu_eti_read_dev   entries: HOST array.  d_bytes 16-byte aligned (NULL with     */
/*            n_bytes 0), no byte outside [d_bytes, d_bytes + n_bytes) is read.       */
/*            d_state_in (or NULL) / d_state_out 16-byte aligned and not the same.     */
/*            d_fib [max_frames][3][32] and d_status 16-byte aligned, d_result 4-,      */
/*            every d_out[k] 8-byte aligned; d_out is a HOST array of plan->nst DEVICE  */
/*            pointers or NULL.  plan: what dabgpu_eti_layout gave, or NULL.  Four      */
/*            launches, no synchronisation, no global atomic.  Everything is checked    */
/*            before anything is enqueued: a refused call (DABGPU_ERR_ARG) writes       */
/*            nothing.                                                                  */
/* dabgpu_eti_read_host   the same on host pointers (no context, no device): the        */
/*            serial walk of the same header.                                           */
/* ------------------------------------------------------------------------ */
#define DABGPU_ETI_OTHER_PLAN     5    /* a verdict beside DABGPU_ETI_BAD_*: a good frame of another multiplex */
#define DABGPU_ETI_READ_GAP       1    /* status flags: gap != 0                                               */
#define DABGPU_ETI_READ_FP_BREAK  2    /* FP is not the previous row's FP + 1 modulo 8                          */
#define DABGPU_ETI_READ_ERR_FIELD 4    /* ERR is not 0xFF (the writer's warm-up frames included)                */
#define DABGPU_ETI_READ_FIB_CRC   8    /* a taken row with a FIB that failed its CRC                            */

typedef struct dabgpu_eti_read_status { /* per row, 16 bytes */
    uint32_t offset;                   /* of the frame in S                                          */
    uint8_t  verdict;                  /* 0, DABGPU_ETI_BAD_DATA_CRC or DABGPU_ETI_OTHER_PLAN         */
    uint8_t  fct, fp, err;             /* the header's                                               */
    uint8_t  fib_ok;                   /* bit j = FIB j passed its CRC (0 unless taken)              */
    uint8_t  gap;                      /* (FCT - (previous row's FCT + 1)) mod 250; 0 for the first  */
    uint8_t  flags;                    /* DABGPU_ETI_READ_*                                          */
    uint8_t  reserved;                 /* 0                                                          */
    uint32_t reserved2;                /* 0                                                          */
} dabgpu_eti_read_status;

typedef struct dabgpu_eti_read_result { /* per entry and call, 48 bytes */
    uint32_t rows, taken;              /* rows emitted; of them with verdict 0                       */
    uint32_t bad_data_crc, other_plan; /* ... with verdict 4, 5                                      */
    uint32_t skipped, resyncs;         /* bytes stepped over; times the walk had to search           */
    uint32_t gap_sum;                  /* sum of the rows' gaps                                      */
    uint32_t fib_errors;               /* FIBs of taken rows that failed their CRC                   */
    uint32_t tail_bytes;               /* held in the new state                                      */
    uint32_t reserved[3];              /* 0                                                          */
} dabgpu_eti_read_result;

typedef struct dabgpu_eti_read_entry {
    const uint8_t *d_bytes;            /* the new bytes                                              */
    int32_t n_bytes;                   /* 0 .. 2^30                                                  */
    int32_t reserved;                  /* 0                                                          */
    const dabgpu_eti_plan *plan;       /* HOST; NULL = discovery                                     */
    uint8_t *const *d_out;             /* HOST array [plan->nst] of DEVICE pointers, or NULL         */
    const void *d_state_in;            /* or NULL                                                    */
    void *d_state_out;
    uint8_t *d_fib;                    /* [max_frames][3][32]                                        */
    uint8_t *d_crc_ok;                 /* [max_frames][3]                                            */
    dabgpu_eti_read_status *d_status;  /* [max_frames]                                               */
    dabgpu_eti_read_result *d_result;
} dabgpu_eti_read_entry;

size_t dabgpu_eti_read_state_bytes(void);
int dabgpu_eti_read_dev(dabgpu_ctx *ctx, const dabgpu_eti_read_entry *entries, int n_entries, void *stream);
int dabgpu_eti_read_host(const dabgpu_eti_read_entry *entries, int n_entries);

/* ------------------------------------------------------------------------ */
/* EDI output: the decode call's buffers written   */
/* as EDI -- ETSI TS 102 693 over the AF layer of TS 102 821 -- one AF packet    */
/* per CIF.  The format is stated as known, a line per field, at the top of      */
/* include/dabgpu_edi.h; parity with other EDI tools is not pinned.  A packet is  */
/*   10 AF header ("AF", LEN, SEQ, AR = 0x90, PT = 'T')                           */
/*   16 "*ptr" item naming "DETI";  110 "deti" item: dlfc, STAT, MID = 1, FP,      */
/*      MNSC = FFFF and the 96 FIC bytes (no time stamp)                          */
/*   11 + 8 STL per stream: "est" n, SCID / SAD / TPL, its bytes of this CIF,      */
/*      streams by ascending SAD as in the ETI frame                              */
/*   zero padding to a payload of a multiple of 8 bytes;  2 CRC (the FIB's rule)   */
/* so a plan's packet has one size, 12 + 8 k bytes.  Everything the ETI writer     */
/* decides is decided here by the same device code: the FIC delay of 15 CIFs and   */
/* dabgpu_eti_history -- a history one writer left continues the other --, warm-up,  */
/* the FIG 0/0 anchor, d_cif_start, COUNT_MISMATCH, dabgpu_eti_status with length =  */
/* the packet's bytes); STAT is the byte the ETI writer puts into ERR.  The CIF      */
/* count travels whole: dlfc = 0 .. 4999.                                          */
/*                                                                                */
/* dabgpu_edi_packet_bytes   host only: the size of the plan's packet, or           */
/*            DABGPU_ERR_ARG for a plan dabgpu_eti_layout did not make.             */
/* dabgpu_edi_frames_dev   the arguments of dabgpu_eti_frames_dev, and: seq_start    */
/*            a HOST array [n_streams] or NULL (= 0): packet t of stream s gets SEQ   */
/*            seq_start[s] + t modulo 65536 (the caller adds 4 frames_per_stream      */
/*            per call, and may do so as soon as the call has returned, whatever      */
/*            memory the array lies in: it is copied before the call returns); the    */
/*            output is a byte stream per ensemble, the call's                        */
/*            4 frames_per_stream packets back to back from d_edi + s stream_stride   */
/*            (d_edi and stream_stride 16-byte aligned, stream_stride >=              */
/*            4 frames_per_stream packet bytes), ready for one write().  Bytes         */
/*            behind a stream's packets are not touched.  Two launches, no             */
/*            synchronisation (the first call on a context, or one with more streams   */
/*            than any before, waits for the stream once while its stage area grows).  */
/*            A refused call (DABGPU_ERR_ARG) enqueues nothing.                        */
/* dabgpu_edi_parse   host only.  Checks one AF packet of exactly len bytes -- header, */
/*            CRC, the TAG items, what makes it a DETI packet -- and gives its parts.   */
/*            Returns DABGPU_OK, DABGPU_ERR_ARG for a NULL argument, or a positive      */
/*            DABGPU_EDI_* (info is filled as far as the check that failed).            */
/* dabgpu_edi_streams_from_packet   host only.  The list dabgpu_eti_layout takes, read   */
/*            from a DETI packet's est items by dabgpu_eti_streams_from_frame's own      */
/*            mapping from TPL / STL to a sub-channel.  DABGPU_ERR_ARG for a packet      */
/*            dabgpu_edi_parse does not pass or a TPL / STL pair that names no profile.  */
/* ------------------------------------------------------------------------ */
#define DABGPU_EDI_MAX_PACKET 8192     /* header and CRC included: what the reader takes for a packet */
#define DABGPU_EDI_BAD_HEADER 1        /* "AF", LEN against len and MAX_PACKET, AR, PT                  */
#define DABGPU_EDI_BAD_CRC    2
#define DABGPU_EDI_BAD_TAGS   3        /* malformed: an item overruns, a deti / est / *ptr of a wrong length, a count out of range */
#define DABGPU_EDI_NOT_DETI   4        /* well formed, but not exactly one deti, est numbers not 1..N once each, or a foreign *ptr */

typedef struct dabgpu_edi_info {
    int32_t len;                       /* LEN: the payload's bytes                                   */
    int32_t length;                    /* 12 + len                                                   */
    int32_t seq, crc;                  /* as stored in the packet                                    */
    int32_t n_ptr, n_deti, n_other;    /* items of these names (n_other: names stepped over)         */
    int32_t atstf, ficf, rfudf;        /* the deti item's flags                                      */
    int32_t dlfc;                      /* 250 FCTH + FCT                                             */
    int32_t stat, mid, fp, mnsc;
    int32_t utco, tsta;                /* when atstf (tsta 0xFFFFFF otherwise)                       */
    uint32_t seconds;
    int32_t fic_offset;                /* where the 96 FIC bytes begin in the packet, -1 without     */
    int32_t nst;                       /* est items (of a DETI packet)                               */
    int32_t reserved[4];
    int32_t scid[DABGPU_ETI_MAX_STREAMS], sad[DABGPU_ETI_MAX_STREAMS], tpl[DABGPU_ETI_MAX_STREAMS],
            stl[DABGPU_ETI_MAX_STREAMS];     /* of est k + 1                                          */
    int32_t offset[DABGPU_ETI_MAX_STREAMS];  /* where its 8 stl bytes begin in the packet             */
} dabgpu_edi_info;

int dabgpu_edi_packet_bytes(const dabgpu_eti_plan *plan);
int dabgpu_edi_frames_dev(dabgpu_ctx *ctx, const dabgpu_eti_plan *plan, int n_streams, int frames_per_stream,
                          const uint8_t *d_fib, const uint8_t *d_crc_ok, const uint8_t *const *d_out,
                          const dabgpu_eti_history *d_history_in, dabgpu_eti_history *d_history_out,
                          const int32_t *d_cif_start, const uint32_t *seq_start, uint8_t *d_edi, size_t stream_stride,
                          dabgpu_eti_status *d_status, void *stream);
int dabgpu_edi_parse(const uint8_t *packet, size_t len, dabgpu_edi_info *info);
int dabgpu_edi_streams_from_packet(const uint8_t *packet, size_t len, dabgpu_eti_stream *streams, int *n);

/* ------------------------------------------------------------------------ */
/* EDI input: AF packet byte streams -- a TCP        */
/* capture, a file -- read back into what the decode call leaves, as the ETI(NI)  */
/* reader does, on the device or on host memory.  The contract -- stream, H and C, the walk, what   */
/* is judged how, rows, status, state -- is written out in include/dabgpu_edi.h.   */
/* In short, per entry: S = the state's carried tail (0..8191 bytes) + the         */
/* n_bytes new bytes.  A position holds a packet when its ten header bytes are      */
/* plausible, the packet lies inside S and its CRC holds; the walk steps from       */
/* packet to packet and searches for the next one where there is none (skipped,     */
/* resyncs), never trusting the LEN of a packet whose CRC fails.  A CRC-good         */
/* packet that is malformed (bad_tags), not a DETI packet (not_deti) or of another   */
/* multiplex than the plan's (other_plan) is counted and gives no row.  Every other  */
/* is row r: its FIC to d_fib[r] (zero with DABGPU_EDI_READ_NO_FIC), the three FIB    */
/* CRC flags computed here to d_crc_ok[r], stream k's bytes to d_out[k][r] for every   */
/* d_out[k] that is not NULL (the caller's order, through plan->order).  plan NULL     */
/* is the discovery pass: every DETI packet is a row, only FIC and status leave;        */
/* dabgpu_edi_streams_from_packet reads the multiplex from a row's packet (offset and   */
/* length in its status).  What is left (below 8192 bytes) is the new tail.  CIFs       */
/* missing by dlfc are NOT replaced by zero rows: status gap says how many are           */
/* missing in front of a row, exactly (modulo 5000), and SEQ_BREAK that packets are.     */
/*                                                                                     */
/* dabgpu_edi_read_max_rows   rows one entry can emit: (8191 + n_bytes) / m with m the     */
/*            smallest packet that gives a row, 26 in discovery and                       */
/*            26 + sum(11 + 8 STL) with a plan.  Its outputs hold this many.  Never 0.     */
/*            DABGPU_ERR_ARG for n_bytes outside 0 .. 2^30 or a plan dabgpu_eti_layout      */
/*            did not make.                                                                */
/* dabgpu_edi_read_state_bytes   size of the per-entry state record (a head of 96 bytes,     */
/*            then 8192 tail bytes).  All zero = a stream that starts.  Written whole.  A     */
/*            record the library did not write makes no call read outside it.                */
/* dabgpu_edi_read_dev   entries: HOST array (at most 65535) with the fields of                  */
/*            dabgpu_eti_read_entry and the same alignments (d_bytes, the states, d_fib,          */
/*            d_status 16 bytes; d_result 4; every d_out[k] 8), d_state_in and d_state_out not     */
/*            overlapping, d_fib / d_crc_ok / d_status never NULL; d_out a HOST array of           */
/*            plan->nst DEVICE pointers or NULL.  No byte outside [d_bytes, d_bytes + n_bytes)      */
/*            is read.  Two launches -- every position's header test and the CRCs of the hits,      */
/*            then a wave per entry that walks, judges and moves -- no synchronisation (but once     */
/*            while the stage area grows), no global atomic.  Everything is checked before           */
/*            anything is enqueued: a refused call (DABGPU_ERR_ARG) writes nothing.  A stream that    */
/*            is header-plausible every 10 bytes costs at most n / 10 CRCs of at most 8 KB each:      */
/*            the bound is stated, not optimised.                                                     */
/* dabgpu_edi_read_host   the same on host pointers (no context, no device): the serial walk of        */
/*            the same header.                                                                        */
/* ------------------------------------------------------------------------ */
#define DABGPU_EDI_READ_GAP         1  /* status flags: gap != 0                                               */
#define DABGPU_EDI_READ_SEQ_BREAK   2  /* SEQ is not the previous CRC-good packet's + 1                         */
#define DABGPU_EDI_READ_FP_MISMATCH 4  /* FP != dlfc mod 8                                                      */
#define DABGPU_EDI_READ_STAT_FIELD  8  /* STAT is not 0xFF (the writer's warm-up packets included)              */
#define DABGPU_EDI_READ_FIB_CRC    16  /* a FIB of the row failed its CRC                                       */
#define DABGPU_EDI_READ_NO_FIC     32  /* FICF = 0: the row's FIC and flags are zero                            */
#define DABGPU_EDI_READ_TIME       64  /* ATSTF = 1: utco, seconds and tsta are the packet's                    */

typedef struct dabgpu_edi_read_status { /* per row, 32 bytes */
    uint32_t offset;                   /* of the packet in S                                         */
    uint16_t length;                   /* 12 + LEN                                                   */
    uint16_t dlfc;                     /* 0 .. 4999                                                  */
    uint16_t seq;
    uint16_t gap;                      /* (dlfc - (previous row's dlfc + 1)) mod 5000; 0 for the first */
    uint8_t  fp, stat, mid;            /* the deti item's                                            */
    uint8_t  fib_ok;                   /* bit j = FIB j passed its CRC                               */
    uint8_t  flags;                    /* DABGPU_EDI_READ_*                                          */
    uint8_t  utco;
    uint8_t  reserved[2];              /* 0                                                          */
    uint32_t seconds, tsta;            /* 0 / 0xFFFFFF without DABGPU_EDI_READ_TIME                  */
    uint32_t reserved2;                /* 0                                                          */
} dabgpu_edi_read_status;

typedef struct dabgpu_edi_read_result { /* per entry and call, 48 bytes */
    uint32_t rows;                     /* rows emitted                                               */
    uint32_t not_deti, bad_tags, other_plan; /* CRC-good packets that gave no row                    */
    uint32_t skipped, resyncs;         /* bytes stepped over; stretches of them                      */
    uint32_t gap_sum;                  /* sum of the rows' gaps                                      */
    uint32_t fib_errors;               /* FIBs of rows with a FIC that failed their CRC              */
    uint32_t tail_bytes;               /* held in the new state                                      */
    uint32_t reserved[3];              /* 0                                                          */
} dabgpu_edi_read_result;

typedef struct dabgpu_edi_read_entry {
    const uint8_t *d_bytes;            /* the new bytes                                              */
    int32_t n_bytes;                   /* 0 .. 2^30                                                  */
    int32_t reserved;                  /* 0                                                          */
    const dabgpu_eti_plan *plan;       /* NULL = discovery                                           */
    uint8_t *const *d_out;             /* array [plan->nst] of pointers, or NULL                     */
    const void *d_state_in;            /* or NULL                                                    */
    void *d_state_out;
    uint8_t *d_fib;                    /* [max_rows][3][32]                                          */
    uint8_t *d_crc_ok;                 /* [max_rows][3]                                              */
    dabgpu_edi_read_status *d_status;  /* [max_rows]                                                 */
    dabgpu_edi_read_result *d_result;
} dabgpu_edi_read_entry;

size_t dabgpu_edi_read_state_bytes(void);
int dabgpu_edi_read_max_rows(int n_bytes, const dabgpu_eti_plan *plan);
int dabgpu_edi_read_dev(dabgpu_ctx *ctx, const dabgpu_edi_read_entry *entries, int n_entries, void *stream);
int dabgpu_edi_read_host(const dabgpu_edi_read_entry *entries, int n_entries);

/* ------------------------------------------------------------------------ */
/* EDI PFT layer: EDI over UDP or multicast.  Every    */
/* AF packet travels as PF fragments (TS 102 821), usually with Reed-Solomon        */
/* RS(255,207) parity over interleaved chunks so that whole datagrams may be lost.   */
/* The writer cuts the AF packets dabgpu_edi_frames_dev leaves into fragments; the    */
/* reader puts fragment byte streams (datagram payloads concatenated by the caller,    */
/* or a file) back together into the AF packet byte streams dabgpu_edi_read_dev         */
/* takes.  The format as known, the layout rule and the reader's whole contract --       */
/* stream, walk, groups and the horizon, closing, records, state -- are written out in   */
/* include/dabgpu_pft.h; parity with other EDI tools is not pinned.                        */
/*                                                                                        */
/* dabgpu_pft_layout   host only.  How packets of packet_bytes (12 .. 8192) are cut:       */
/*            with fec, fragments sized so that any m of a packet's may be lost            */
/*            (s0 = min(48 c / (m + 1), max_payload), f = ceil(B / s0), s = ceil(B / f));     */
/*            without, fragments of max_payload bytes.  addr: fragments carry Source and       */
/*            Dest.  guaranteed_losses is exact.  DABGPU_ERR_ARG for what the rule refuses      */
/*            (info is not written).                                                           */
/* dabgpu_pft_fragments_dev   d_af: n_packets AF packets of layout->packet_bytes back to         */
/*            back per stream, stream s at d_af + s * in_stride (what dabgpu_edi_frames_dev        */
/*            leaves); pseq_start: HOST array [n_streams] or NULL (= 0), the first packet's         */
/*            Pseq per stream -- the caller adds n_packets to it after the call, the kernel           */
/*            wraps modulo 65536.  Stream s's fragments leave back to back from d_pf +                */
/*            s * out_stride, layout->stream_bytes per packet.  A workgroup per packet: parity         */
/*            with a lane per (chunk, parity byte), fragments by the interleave rule.  d_af and         */
/*            d_pf 16-byte aligned, strides multiples of 16, in_stride >= n_packets *                    */
/*            packet_bytes, out_stride >= n_packets * stream_bytes, no overlap; a layout                  */
/*            dabgpu_pft_layout did not make, or anything else here, is DABGPU_ERR_ARG and                 */
/*            nothing is enqueued or written.  One launch, no synchronisation (but once while the           */
/*            stage area grows).                                                                            */
/* dabgpu_pft_fragments_host   the same on host pointers, serially (no context, no device).                   */
/* dabgpu_pft_read_state_bytes / _out_bytes / _max_records   sizes of an entry's state record                  */
/*            (a head, the two open groups, the tail; all zero = a stream that starts), its output              */
/*            (29216 + n_bytes: nothing can run out of room) and its records                                    */
/*            (2 + (8211 + n_bytes) / 15).  The latter two are 0 for n_bytes outside 0 .. 2^30.                  */
/* dabgpu_pft_read_dev   entries: HOST array (at most 65535).  Per entry, in short: S = the carried               */
/*            tail + the new bytes; fragments are taken where a plausible header (HCRC) and its                    */
/*            payload lie inside S, bytes between them are skipped and counted; fragments join                      */
/*            the group of their Pseq, open only at 1 and 2 above the horizon; a complete group                     */
/*            is emitted, in Pseq order; a group that the horizon passes, or FLUSH closes, is                       */
/*            filled by erasure-only RS decoding where every chunk misses at most 48 bytes, and                      */
/*            LOST otherwise.  Packets leave back to back in d_out, a record per closed group in                      */
/*            d_records.  d_bytes, the states and d_out 16-byte aligned, d_records and d_result 4;                    */
/*            d_state_in and d_state_out not overlapping.  Three launches -- every position's header                  */
/*            test, a wave per entry that walks and moves, a workgroup per emitted packet that                         */
/*            fills and checks -- no synchronisation (but once while the stage area grows), no                          */
/*            global atomic.  Everything is checked before anything is enqueued: a refused call                         */
/*            (DABGPU_ERR_ARG) writes nothing.  The walk is one serial step per fragment and entry:                      */
/*            stated, not optimised.                                                                                    */
/* dabgpu_pft_read_host   the same on host pointers (no context, no device): the serial reader of                        */
/*            the same header.                                                                                          */
/* To chain into dabgpu_edi_read_dev, result.out_bytes has to reach the host in between (one 4-byte                        */
/* copy): the EDI entry's n_bytes is a host field.                                                                         */
/* ------------------------------------------------------------------------ */
#define DABGPU_PFT_FEC          1      /* record flags: the group's fragments carry RSk / RSz                 */
#define DABGPU_PFT_ADDR         2      /* ... Source / Dest                                                    */
#define DABGPU_PFT_RECOVERED    4      /* fragments were missing and every chunk was filled                     */
#define DABGPU_PFT_INCONSISTENT 8      /* a filled chunk fails one of its 48 syndromes: a received byte was wrong */
#define DABGPU_PFT_LOST        16      /* nothing emitted, length 0                                             */
#define DABGPU_PFT_AF_OK       32      /* the emitted bytes are one AF packet whose CRC holds                   */
#define DABGPU_PFT_FLUSHED     64      /* closed by DABGPU_PFT_READ_FLUSH                                       */
#define DABGPU_PFT_READ_FLUSH   1      /* entry flag: close every open group at the call's end                  */

typedef struct dabgpu_pft_layout_info { /* 64 bytes */
    int32_t packet_bytes, fec, m, max_payload, addr;   /* as given                                   */
    int32_t chunks, rs_k, rs_z, block_bytes;           /* c, k, z, B (0 without fec)                 */
    int32_t fcount, plen;                              /* f, s                                       */
    int32_t header_bytes;                              /* 14 + 2 fec + 4 addr                        */
    int32_t stream_bytes;                              /* all fragments of one packet                */
    int32_t guaranteed_losses;
    int32_t reserved[2];                               /* 0                                          */
} dabgpu_pft_layout_info;

typedef struct dabgpu_pft_read_record { /* per closed group that held a fragment, 32 bytes */
    uint32_t offset;                   /* of the packet in the call's output                         */
    uint16_t length;                   /* l; 0 = LOST                                                */
    uint16_t pseq, fcount, received;
    uint16_t plen;                     /* s                                                          */
    uint8_t  rs_k, rs_z, chunks;       /* 0 without FEC                                              */
    uint8_t  max_erasures;             /* the worst chunk's erased positions (255 = that or more)    */
    uint16_t flags;                    /* DABGPU_PFT_*                                               */
    uint16_t source, dest;
    uint32_t reserved[2];              /* 0                                                          */
} dabgpu_pft_read_record;

typedef struct dabgpu_pft_read_result { /* per entry and call, 64 bytes */
    uint32_t records, packets, lost, recovered;
    uint32_t fragments, duplicates, mismatched, late;
    uint32_t unsupported, missing, skipped, resyncs;
    uint32_t out_bytes, tail_bytes, chunks_filled, bytes_filled;
} dabgpu_pft_read_result;

typedef struct dabgpu_pft_read_entry {
    const uint8_t *d_bytes;            /* the new bytes                                              */
    int32_t n_bytes;                   /* 0 .. 2^30                                                  */
    int32_t flags;                     /* DABGPU_PFT_READ_FLUSH or 0                                 */
    const void *d_state_in;            /* or NULL                                                    */
    void *d_state_out;
    uint8_t *d_out;                    /* [dabgpu_pft_read_out_bytes(n_bytes)]                       */
    dabgpu_pft_read_record *d_records; /* [dabgpu_pft_read_max_records(n_bytes)]                     */
    dabgpu_pft_read_result *d_result;
} dabgpu_pft_read_entry;

int dabgpu_pft_layout(int packet_bytes, int fec, int m, int max_payload, int addr, dabgpu_pft_layout_info *info);
int dabgpu_pft_fragments_dev(dabgpu_ctx *ctx, const dabgpu_pft_layout_info *layout, int n_streams, int n_packets, const uint8_t *d_af,
                             size_t in_stride, const uint32_t *pseq_start, uint32_t source, uint32_t dest, uint8_t *d_pf, size_t out_stride,
                             void *stream);
int dabgpu_pft_fragments_host(const dabgpu_pft_layout_info *layout, int n_streams, int n_packets, const uint8_t *af, size_t in_stride,
                              const uint32_t *pseq_start, uint32_t source, uint32_t dest, uint8_t *pf, size_t out_stride);
size_t dabgpu_pft_read_state_bytes(void);
size_t dabgpu_pft_read_out_bytes(int n_bytes);
int dabgpu_pft_read_max_records(int n_bytes);
int dabgpu_pft_read_dev(dabgpu_ctx *ctx, const dabgpu_pft_read_entry *entries, int n_entries, void *stream);
int dabgpu_pft_read_host(const dabgpu_pft_read_entry *entries, int n_entries);

/* ------------------------------------------------------------------------ */
/* The host-fed ring: dabgpu_ofdm_demod_frames + dabgpu_decode_frames for a    */
/* caller whose samples start in HOST memory (files, a network), pipelined.    */
/* The reference runs these two stages on two threads with a 2-frame ring       */
/* between them (/root/reference/src/radio_block.cpp:23-44: the On_OFDM_Frame   */
/* callback writes, the radio thread reads and calls BasicRadio::Process); here  */
/* the ring is `slots` device staging sets and three engines work at once: the   */
/* upload of batch k+1, the kernels of batch k, the download of batch k-1.       */
/*                                                                            */
/* dabgpu_pipe_open   slots 2..8 (3 keeps all three engines busy); max_frames =   */
/*            the largest n_streams * frames_per_stream a submit will carry;       */
/*            frame_stride of the host IQ ([n][frame_stride] complex samples of the */
/*            context's format, dabgpu_set_iq_format, which the ring records and    */
/*            sizes its staging slots for; frame f's first PRS sample at            */
/*            iq + f*frame_stride, 76*2552 samples read).  One ring per context.    */
/* dabgpu_pipe_submit enqueues ONE batch and returns at once: the samples go up,    */
/*            are demodulated -- with freq_offset[n_frames] as                       */
/*            dabgpu_ofdm_demod_frames does, or (freq_offset == NULL) closed loop on   */
/*            the context's stream states as dabgpu_ofdm_demod_streams does, cyclic-   */
/*            prefix or decision-directed per dabgpu_set_stream_loop -- and decoded     */
/*            as dabgpu_decode_frames does (FIC + the listed sub-channels); fib,         */
/*            crc_ok, out[i] ([n_streams][frames_per_stream*4][bitrate*3]) and, when      */
/*            soft != NULL, the soft bits come down.  Batches are processed in the        */
/*            order submitted and CONTINUE their streams: the time de-interleaver of       */
/*            every sub-channel stays on the device between submits (keyed by start         */
/*            address, size and n_streams; a sub-channel seen for the first time, or left    */
/*            out of the previous batch, starts from erasures; dabgpu_pipe_reset drops        */
/*            them all).  Every host buffer must stay valid and untouched until                */
/*            dabgpu_pipe_wait(ticket) returns; buffers from dabgpu_host_alloc move at          */
/*            the link rate (pageable memory works, through the runtime's bounce buffers         */
/*            and without overlap).  A submit that finds every slot busy first waits for           */
/*            the oldest batch to leave the device.                                                */
/* dabgpu_pipe_wait   blocks until that batch's results are in the caller's buffers.               */
/* Kernels run on the context's own stream: the synchronous entry points of the same context         */
/* stay ordered with the ring (and wait behind it).                                                   */
/* ------------------------------------------------------------------------ */
int dabgpu_pipe_open(dabgpu_ctx *ctx, int slots, int max_frames, size_t frame_stride);
int dabgpu_pipe_submit(dabgpu_ctx *ctx, const void *iq, int n_streams, int frames_per_stream, const float *freq_offset,
                       float fine_freq_update_beta, const dabgpu_subchannel *sc, int n_subchannels, int8_t *soft,
                       uint8_t *fib, uint8_t *crc_ok, uint8_t *const *out, int64_t *ticket);
int dabgpu_pipe_wait(dabgpu_ctx *ctx, int64_t ticket);
int dabgpu_pipe_reset(dabgpu_ctx *ctx);
int dabgpu_pipe_close(dabgpu_ctx *ctx);

/* ------------------------------------------------------------------------ */
/* DAB+ audio super-frame: Fire code, RS(120,110), AU CRC.    */
/* Replaces the checks the reference reports as the "Firecode / RS / AU"       */
/* flags and GetSuperFrameHeader()                                             */
/*   (/root/reference/src/render_radio_block.cpp:414-437).                     */
/*                                                                            */
/* in        super-frame f = 5 consecutive logical frames of a DAB+ subchannel */
/*           (the bytes dabgpu_msc_decode produces) = 15*bitrate bytes,        */
/*           starting at in + f*in_stride.  The caller finds the alignment by   */
/*           trying the 5 possible logical-frame offsets until firecode_ok      */
/*           (a batch: dabgpu_dabplus_follow_dev below finds and keeps it).     */
/* out       [n][110*s] corrected data part (s = bitrate/8)                    */
/* status[f] firecode_ok (after RS), rs_corrected bytes, rs_uncorrectable       */
/*           codewords (of s), num_aus (0 when the Fire code fails),            */
/*           au_crc_mask (bit a = access unit a passes its CRC16),              */
/*           au_start[0..num_aus] byte offsets into `out`                       */
/* ------------------------------------------------------------------------ */
typedef struct dabgpu_superframe_status {
    int32_t firecode_ok;
    int32_t rs_corrected;
    int32_t rs_uncorrectable;
    int32_t num_aus;
    int32_t au_crc_mask;
    int32_t au_start[8];
    int32_t reserved[3];
} dabgpu_superframe_status;

int dabgpu_dabplus_superframes_dev(dabgpu_ctx *ctx, const uint8_t *d_in, size_t in_stride, int n_superframes,
                                   int bitrate_kbps, uint8_t *d_out, dabgpu_superframe_status *d_status,
                                   void *stream);
int dabgpu_dabplus_superframes(dabgpu_ctx *ctx, const uint8_t *in, size_t in_stride, int n_superframes,
                               int bitrate_kbps, uint8_t *out, dabgpu_superframe_status *status);

/* ------------------------------------------------------------------------ */
/* Following every DAB+ sub-channel of a batch to super-frames on the device:  */
/* alignment, carry between calls, then the checks above -- what stands        */
/* behind the "Firecode / RS / AU" flags and the super-frame header of every    */
/* DAB+ service the reference shows                                            */
/*   (/root/reference/src/render_radio_block.cpp:414-437)                       */
/* for a monitoring receiver that decodes many ensembles per call              */
/* (dabgpu_decode_ensembles_dev).                    */
/*                                                                            */
/* One entry per followed sub-channel; one call takes the n_cifs logical        */
/* frames every entry's decode call produced (its d_out[j]) and two launches:   */
/* one wave per entry finds the phase, one workgroup per super-frame decodes.   */
/*                                                                            */
/* The contract of one entry in one call.  F = the `held` frames of carry_in    */
/* followed by the n_cifs new ones, T = held + n_cifs.  Frame i is a RAW HIT    */
/* when its first 11 bytes, uncorrected, are not all zero and the Fire code     */
/* over bytes 2..10 equals bytes 0..1.  votes[r] = hits at i = r (mod 5),       */
/* raw_hits = their sum.  The phase p: with a synced carry 0, unless a residue   */
/* has strictly more votes than residue 0 -- then, and with a carry that is      */
/* not synced, the smallest residue with the maximum, if that is > 0; else no    */
/* phase.  No phase: n_superframes = 0, phase = -1, carry_out holds the last     */
/* min(4, T) frames with synced = 0, dropped = the rest.  With a phase:          */
/* n_superframes = (T - p) / 5, super-frame k = frames p + 5k .. p + 5k + 4,      */
/* dropped = p, carry_out holds the 0..4 frames from p + 5 n_superframes on,      */
/* synced = 1 iff votes[p] > 0 or n_superframes = 0.  Every emitted super-frame   */
/* gets exactly what dabgpu_dabplus_superframes_dev gives for the same 120 s      */
/* bytes (RS, then the Fire code, then the AU table and CRCs): d_data[k] and      */
/* d_status[k], k < n_superframes; rows beyond are not written.  A super-frame    */
/* whose header has byte errors is decoded where the votes of the others put      */
/* it, and comes out firecode_ok after RS.                                        */
/*                                                                            */
/* The search reads the raw header because an RS pass at all five phases costs   */
/* five times the kernel; one phase per entry per call is enough because the     */
/* CIFs of a call are contiguous by construction.  The limit: a call none of     */
/* whose start frames has a clean raw header finds no phase (or keeps the one    */
/* it was on), however well RS would have repaired them.                         */
/* ------------------------------------------------------------------------ */
typedef struct dabgpu_dabplus_follow_result {
    int32_t n_superframes;      /* emitted by this call                                             */
    int32_t phase;              /* p, or -1 = none                                                   */
    int32_t synced;             /* what carry_out says                                               */
    int32_t dropped;            /* frames of F that belong to no super-frame and are not carried      */
    int32_t raw_hits;
    int32_t held;               /* frames in carry_out, 0..4                                          */
    int32_t reserved[2];
} dabgpu_dabplus_follow_result;

typedef struct dabgpu_dabplus_entry {       /* HOST array, one per followed sub-channel; every pointer DEVICE memory */
    const uint8_t *d_in;        /* [n_cifs][in_stride] logical frames: the d_out[j] of the decode calls            */
    size_t in_stride;           /* >= bitrate*3                                                                    */
    int32_t bitrate_kbps;       /* multiple of 8, 8 .. 512 (the range of dabgpu_dabplus_superframes_dev)           */
    const void *d_carry_in;     /* dabgpu_dabplus_carry_bytes(bitrate) bytes on a 16-byte boundary, or NULL = fresh */
                                /* start; an all-zero record is a fresh start too (as is one whose held is not 0..4) */
    void *d_carry_out;          /* same size and alignment; != d_carry_in; overlaps nothing else of the call        */
                                /* (written whole: header, held frames, zeros behind them)                         */
    uint8_t *d_data;            /* [(n_cifs+4)/5][110*s]                                                           */
    dabgpu_superframe_status *d_status;      /* [(n_cifs+4)/5]                                                     */
    dabgpu_dabplus_follow_result *d_result;  /* one record                                                         */
} dabgpu_dabplus_entry;

/* bytes of one carry record: a 16-byte header {int32 synced, held, 0, 0} and 4 logical frames of bitrate*3 bytes, rounded
 * up to 16; 0 for a bit rate the follow call refuses */
size_t dabgpu_dabplus_carry_bytes(int bitrate_kbps);

/* entries [n_entries] (HOST), any mix of bit rates; n_cifs logical frames per entry (frames_per_stream * 4 of the decode
 * call).  Everything is checked before anything is enqueued, so a refused call leaves every output as it was:
 * DABGPU_ERR_ARG for a NULL context or table, negative counts, a bit rate outside 8 .. 512 or no multiple of 8,
 * in_stride < bitrate*3 (with more than one frame), a NULL pointer other than d_carry_in (d_in may be NULL with
 * n_cifs = 0, d_data / d_status with n_cifs = 0), a carry record off its 16-byte boundary, d_carry_in and d_carry_out that
 * are equal or overlap, d_status or d_result off a 4-byte boundary.  No host synchronisation, no host-pointer twin: the
 * one-frame path of the plugin stays on dabgpu_dabplus_superframes. */
int dabgpu_dabplus_follow_dev(dabgpu_ctx *ctx, const dabgpu_dabplus_entry *entries, int n_entries, int n_cifs, void *stream);

/* ------------------------------------------------------------------------ */
/* Dynamic labels: the text every followed DAB+ service shows ("now playing"),  */
/* from the programme-associated data (PAD) of its access units -- what the     */
/* reference prints as channel.GetDynamicLabel() for every audio channel        */
/*   (/root/reference/src/render_radio_block.cpp:425-427, 470-472).             */
/* PAD travels in a data stream element, the first syntactic element of the     */
/* access unit, byte-aligned: no AAC is decoded.  Runs behind                   */
/* dabgpu_dabplus_follow_dev on the same stream, on what that call left on the   */
/* device.  One wave per entry, one launch.          */
/*                                                                              */
/* Not read here: X-PAD application types 1, 12, 13 are stepped over (the         */
/* slideshow call below reads them); DL Plus tags (the command's CRC is           */
/* checked, its body dropped).  No audio is decoded.  (Layer-II frames reach      */
/* this call through dabgpu_mp2_follow_dev below.)                                */
/* Charset 0 (EBU Latin) labels come out as bytes; no table translates them.      */
/*                                                                              */
/* THE CONTRACT of one entry in one call (EN 300 401 clauses 7.4.2 - 7.4.5,       */
/* TS 102 563 clause 5.4, every ambiguity decided; one implementation,            */
/* include/dabgpu_pad_walk.h, serves the kernel, the host twin and the mirror).   */
/*                                                                              */
/* Order and loss.  n = n_superframes of d_follow, clamped to 0 ..                */
/* max_superframes.  Access units (AUs) are visited super-frame k = 0 .. n-1,      */
/* then a = 0 .. num_aus-1 (num_aus above 7 counts as 7).  Every visited AU        */
/* counts in aus.  A super-frame with firecode_ok == 0 or num_aus <= 0 is visited   */
/* as ONE lost AU (how many it carried is not known).  Else AU a is LOST when bit   */
/* a of au_crc_mask is clear, or when b = au_start[a], e = au_start[a+1] are not     */
/* 0 <= b, b + 2 < e <= 110 s.  A lost AU counts in aus_lost and drops the           */
/* continuation context and any open data group.                                    */
/*                                                                              */
/* Locating PAD.  len = e - b - 2 (without the AU CRC).  len < 2 or                */
/* (au[0] >> 5) != 4: no PAD, nothing changes.  Else n = au[1], the payload p       */
/* begins at o = 2; if au[1] == 255 then n += au[2], o = 3.  n < 2 or o + n > len    */
/* (an escape with len == 2 included): pad_malformed++, context and group           */
/* dropped.  F-PAD = p[n-2], p[n-1].  (p[n-2] >> 6) != 0: nothing changes.           */
/* ind = (p[n-2] >> 4) & 3, ci = (p[n-1] >> 1) & 1; ind 0 or 3: nothing changes.      */
/* X-PAD logical byte i = p[n-3-i], avail = n - 2 of them.  An AU that delivers       */
/* at least one sub-field counts in aus_with_xpad.                                    */
/*                                                                              */
/* Short X-PAD (ind 1): avail < 4 is malformed.  With ci: byte 0 is a content         */
/* indicator (CI), type = & 0x1F, then 3 data bytes; it counts as a list of one        */
/* sub-field of length 4.  Without: 4 data bytes of the continued type.                */
/* Variable X-PAD (ind 2), with ci: up to four CI bytes, length index >> 5 into         */
/* {4, 6, 8, 12, 16, 24, 32, 48}, type & 0x1F; type 0 ends the list (its byte is         */
/* consumed); type 31 consumes one more byte (the extended type) and its sub-field       */
/* is skipped by length; the sub-fields follow in list order; a CI or extended-type      */
/* byte at or beyond avail, or list plus sub-fields longer than avail: malformed,        */
/* nothing of the field is used.  The list first sets the continued type to none.        */
/* Without ci: one sub-field of the continued type, as long as the last sub-field         */
/* of the most recent list, clamped to avail.                                             */
/* Continued type: 3 after a sub-field of type 2 or 3, 13 after 12 or 13, none after      */
/* anything else.  A CI-less field with no continued type counts in fields_ignored        */
/* and delivers nothing.  Types other than 2 and 3 are skipped.                           */
/*                                                                              */
/* DLS data group.  A type-2 sub-field drops an open group and opens a new one; a          */
/* type-3 sub-field appends to an open one and is ignored without.  Bytes are taken         */
/* one by one.  With 2 bytes the length is known: b0 = T(1) F(1) L(1) C(1) field1(4),        */
/* b1 = field2(4) field3(4).  C = 0: 2 + (field1 + 1) + 2.  C = 1, field1 = 1 (clear): 4.     */
/* C = 1, field1 = 2 (DL Plus): 2 + (field3 + 1) + 2.  Any other command: the group is         */
/* dropped, commands_ignored++.  With all its bytes the group closes; what is left of           */
/* the sub-field is ignored.  CRC: the FIB's (CCITT 0x1021, start 0xFFFF, complemented)          */
/* over all but the last two bytes, sent big-endian: groups_ok++ or groups_crc_failed++.          */
/* A DL Plus group with a good CRC counts in groups_ok and in commands_ignored.                   */
/*                                                                              */
/* Segments.  A text group (C = 0) with F = 1 is segment 0 and field2 its charset; else            */
/* its number is field2 & 7.  L marks the last segment (of several, the most recent).               */
/* A T that differs from the assembly's empties the assembly and becomes its T.  A                   */
/* segment overwrites its slot.  When segment 0, a last segment m and every one between               */
/* are there: the label is their concatenation (at most 128 bytes), labels_completed++;                */
/* if length, charset or bytes differ from the current label it is replaced and                        */
/* changes++; toggle = T either way; the assembly is emptied, T kept.  A clear command                  */
/* empties the assembly and zeroes the label record; changes++ if its length was not 0.                 */
/* Text bytes behind length are 0.                                                                     */
/*                                                                              */
/* The state record (context, open group, assembly, current label) is opaque; a record                  */
/* this library did not write (a field out of its range) is a fresh start.                              */
/* ------------------------------------------------------------------------ */
typedef struct dabgpu_pad_label {
    int32_t length;             /* 0 .. 128                                                           */
    int32_t charset;            /* 0 .. 15 (EN 300 401 clause 5.2.2.2: 15 = UTF-8, 6 = UCS-2, 0 = EBU Latin) */
    int32_t toggle;             /* T of the label completed last                                      */
    int32_t reserved;
    uint8_t text[128];
} dabgpu_pad_label;

typedef struct dabgpu_pad_result {          /* counts of THIS call */
    int32_t aus, aus_lost, aus_with_xpad, pad_malformed, fields_ignored;
    int32_t groups_ok, groups_crc_failed, commands_ignored, labels_completed, changes;
    int32_t reserved[6];
} dabgpu_pad_result;

typedef struct dabgpu_pad_entry {           /* HOST array, one per followed sub-channel; every pointer DEVICE memory */
    const uint8_t *d_data;      /* the follow entry's d_data: [max_superframes] rows of >= 110*s bytes          */
    size_t data_stride;         /* >= 110*s                                                                    */
    const dabgpu_superframe_status *d_status;     /* the follow entry's d_status                                */
    const dabgpu_dabplus_follow_result *d_follow; /* its d_result: n_superframes is READ ON THE DEVICE           */
    int32_t bitrate_kbps;       /* multiple of 8, 8 .. 512                                                      */
    int32_t max_superframes;    /* rows that exist; n_superframes is clamped to it                               */
    const void *d_state_in;     /* dabgpu_pad_state_bytes() on a 16-byte boundary; NULL or all zero = fresh start */
    void *d_state_out;          /* same size and alignment; != d_state_in, no overlap                            */
    dabgpu_pad_label *d_label;  /* the label after this call (also kept in the state)                            */
    dabgpu_pad_result *d_result;
} dabgpu_pad_entry;

size_t dabgpu_pad_state_bytes(void);

/* entries [n_entries] (HOST).  No host synchronisation: n_superframes is read on the device, behind the follow call on
 * the same stream.  Everything is checked before anything is enqueued, so a refused call leaves every output as it was:
 * DABGPU_ERR_ARG for a NULL context or table, a negative count, a bit rate outside 8 .. 512 or no multiple of 8, a negative
 * max_superframes, data_stride < 110*s, a NULL pointer other than d_state_in, a state record off its 16-byte boundary,
 * d_state_in and d_state_out that are equal or overlap, d_status, d_follow, d_label or d_result off a 4-byte boundary. */
int dabgpu_pad_labels_dev(dabgpu_ctx *ctx, const dabgpu_pad_entry *entries, int n_entries, void *stream);
/* the same table with HOST pointers, the same checks, the same walk: no context, no GPU */
int dabgpu_pad_labels_host(const dabgpu_pad_entry *entries, int n_entries);
/* The label's text as a NUL-terminated UTF-8 string in out[cap]: -> its length in bytes (>= 0).  Charset 15 (UTF-8: copied
 * after validation -- no stray or missing continuation byte, overlong form, surrogate, code point above U+10FFFF, or NUL)
 * and charset 6 (UCS-2 big-endian; an odd length, a surrogate or a NUL is refused).  DABGPU_ERR_PROFILE for any other
 * charset, DABGPU_ERR_ARG for text that is not valid in its charset, a NULL pointer, cap < 1 or a length outside 0 .. 128,
 * DABGPU_ERR_CAPACITY when cap is too small for the text and its NUL.  A refused call writes nothing. */
int dabgpu_pad_label_utf8(const dabgpu_pad_label *label, char *out, int cap);

/* ------------------------------------------------------------------------ */
/* Slideshow: the MOT objects every followed DAB+ service sends in X-PAD -- what  */
/* the reference shows in the "Slideshow" tab of every audio channel              */
/*   (its src/render_radio_block.cpp:309-382, 589-593).                           */
/* Runs behind dabgpu_dabplus_follow_dev on the same stream, beside                */
/* dabgpu_pad_labels_dev, on the same inputs.  One     */
/* wave per entry, one launch.  The X-PAD field walk (locating PAD, F-PAD, short   */
/* and variable X-PAD, the CI list, continuation, the continued type) is the        */
/* label call's, the same code (include/dabgpu_pad_walk.h, walk_fields); the sink   */
/* is include/dabgpu_mot_walk.h.  Counters aus .. fields_ignored mean what they     */
/* mean there.                                                                      */
/*                                                                                */
/* Not read: FIG 0/13 user application signalling (X-PAD types 12 / 13 are taken    */
/* as MOT as given); MOT directory mode (data group types 6, 7); scrambled bodies   */
/* (type 5) and CA parameters.  The image is not decoded; the device does not look    */
/* at the content type.  (MOT in packet mode: dabgpu_packet_slides_dev, below.)       */
/*                                                                                */
/* THE CONTRACT of one entry in one call (EN 300 401 clauses 5.3.3, 7.4.5.1;          */
/* EN 301 234 clauses 5.1, 5.2, 6.1; every ambiguity decided).                        */
/*                                                                                */
/* Order and loss: exactly the label call's.  A lost AU or a malformed PAD drops      */
/* the continued type, an armed length and any open X-PAD data group.  It does        */
/* not drop the object assembly.                                                      */
/*                                                                                */
/* Type 1 (data group length indicator).  A sub-field of fewer than 4 bytes (the       */
/* 3 bytes of short X-PAD with a CI): lengths_ignored++.  Else bytes 0, 1 = rfa(2)     */
/* length(14), bytes 2, 3 = the FIB's CRC over bytes 0, 1, big-endian: good arms        */
/* next_length = length, lengths_ok++; bad: lengths_ignored++, nothing changes.         */
/*                                                                                */
/* Type 12 drops an open group and consumes the armed length: none armed:               */
/* groups_no_length++, no group; a length below 4: groups_malformed++, no group;         */
/* else a group of that many bytes opens.  Type 13 appends to an open group and is       */
/* ignored without one.  Of a sub-field, min(its length, what the group lacks) bytes     */
/* are taken; the rest is padding.  With all its bytes the group closes.                 */
/*                                                                                */
/* Closing a group (b0 = its first byte; end = length - 2), first match wins:             */
/*   CRC flag (b0 & 0x40) clear, or CRC (the FIB's, over all but the last two bytes,      */
/*     sent big-endian) bad                              -> groups_crc_failed++           */
/*   data group type (b0 & 0x0F) not 3 (MOT header) or 4 (body) -> groups_ignored_type++  */
/*   o = 2, + 2 with the extension flag (b0 & 0x80)                                       */
/*   segment flag (b0 & 0x20) clear, or o + 2 > end      -> groups_malformed++            */
/*   last = bit 7, number n = 15 bits of the two bytes at o; o += 2                        */
/*   user access flag (b0 & 0x10) clear                  -> groups_no_transport_id++      */
/*   o + 1 > end                                         -> groups_malformed++            */
/*   ua = byte at o; o += 1; transport id flag (ua & 0x10) clear -> groups_no_transport_id++ */
/*   li = ua & 0x0F; li < 2 or o + li + 2 > end          -> groups_malformed++            */
/*   transport id = 16 bits at o; o += li (the end-user address is stepped over)            */
/*   z = 13 bits of the two bytes at o (MOT segmentation header); o += 2                    */
/*   z != end - o                                        -> groups_malformed++            */
/*   else groups_ok++ and the segment (part = header | body, id, n, last, z bytes) is used. */
/* Continuity and repetition indices and the repetition count are not looked at.            */
/*                                                                                */
/* Assembly: one object per entry.  For a used segment, first match wins:                    */
/*   id equals the id of the object completed last      -> groups_repeated++, dropped       */
/*   no assembly, or id differs from the assembly's: the assembly is emptied, id is its id   */
/*   the assembly is marked too large                    -> dropped                          */
/*   n >= 32 (header) / 256 (body)                       -> objects_too_large++, marked      */
/*   not last: z == 0, or the part's segment size S is known and z != S, or the part's last  */
/*     segment is known and n >= it                      -> groups_malformed++               */
/*   last: n > 0 and S not known                         -> segments_early_last++, dropped   */
/*   last: a last segment of another number or length is known, or S known and z > S, or a   */
/*     segment above n is present                        -> groups_malformed++               */
/*   at = n * S (S = z for the first non-last segment; 0 when not known).  at + z beyond      */
/*     1024 (header) / body_capacity (body)              -> objects_too_large++, marked      */
/*   S is set (not last) or the last segment and its length noted; then segment n present:    */
/*     segments_repeated++, not overwritten; else placed at `at`: segments_placed++.          */
/* Marked too large, the object is ignored until the transport id changes.                     */
/*                                                                                */
/* Completion, when segments 0 .. last of header AND body are present.  The header core        */
/* is the first 7 header bytes: body_size(28) header_size(13) content_type(6) subtype(9).      */
/* Fewer than 7 header bytes, header_size != assembled header bytes or body_size !=             */
/* assembled body bytes: objects_mismatched++, the assembly is emptied (no id).  Else            */
/* objects_completed++, the id becomes that of the object completed last, the assembly is        */
/* emptied, and the object goes to slot slides_written of THIS call:                             */
/* d_slides + slot * slide_stride holds a dabgpu_mot_slide, the header bytes, the body bytes;    */
/* slides_written++.  No slot left (max_slides) or 32 + header + body > slide_stride:            */
/* slides_dropped++ instead.  Bytes of a slot behind the object, and slots not written, are       */
/* left as they were.                                                                            */
/*                                                                                */
/* The state record is opaque; a record this library did not write for an arena of this           */
/* size is a fresh start.  The arena belongs to the state: the same memory, untouched by          */
/* anyone else, goes into the next call.                                                         */
/* ------------------------------------------------------------------------ */
typedef struct dabgpu_mot_slide {           /* in front of every slide in its slot */
    int32_t transport_id;
    int32_t content_type, content_subtype;  /* of the header core; 2 = image (subtype 1 JFIF, 3 PNG)                 */
    int32_t header_bytes, body_bytes;       /* the MOT header follows the record, the body follows the header          */
    int32_t superframe, au;                 /* where in this call the object completed                                 */
    int32_t reserved;
} dabgpu_mot_slide;

typedef struct dabgpu_mot_result {          /* counts of THIS call */
    int32_t aus, aus_lost, aus_with_xpad, pad_malformed, fields_ignored;
    int32_t lengths_ok, lengths_ignored, groups_no_length;
    int32_t groups_ok, groups_crc_failed, groups_ignored_type, groups_no_transport_id, groups_malformed, groups_repeated;
    int32_t segments_placed, segments_repeated, segments_early_last;
    int32_t objects_completed, objects_mismatched, objects_too_large;
    int32_t slides_written, slides_dropped;
    int32_t xpad_bytes;                     /* X-PAD bytes taken into data groups                                      */
    int32_t object_bytes;                   /* bytes placed into the assembly plus bytes written to slots               */
    int32_t reserved[8];
} dabgpu_mot_result;

typedef struct dabgpu_mot_entry {           /* HOST array, one per followed sub-channel; every pointer DEVICE memory */
    const uint8_t *d_data;      /* as dabgpu_pad_entry                                                          */
    size_t data_stride;
    const dabgpu_superframe_status *d_status;
    const dabgpu_dabplus_follow_result *d_follow;
    int32_t bitrate_kbps;
    int32_t max_superframes;
    const void *d_state_in;     /* dabgpu_mot_state_bytes() on a 16-byte boundary; NULL or all zero = fresh start */
    void *d_state_out;          /* same size and alignment; != d_state_in, no overlap                            */
    void *d_arena;              /* 16-byte boundary; updated in place                                            */
    size_t arena_bytes;         /* >= dabgpu_mot_arena_bytes(0); what is beyond it is body_capacity (at most 256 * 8191) */
    uint8_t *d_slides;          /* [max_slides] slots, 16-byte boundary; may be NULL with max_slides == 0          */
    size_t slide_stride;        /* a multiple of 16, >= 32                                                       */
    int32_t max_slides;         /* max_slides * slide_stride < 2^31                                              */
    int32_t reserved;
    dabgpu_mot_result *d_result;
} dabgpu_mot_entry;

size_t dabgpu_mot_state_bytes(void);
/* the smallest arena for objects whose body has up to body_capacity bytes (0 for more than 256 * 8191) */
size_t dabgpu_mot_arena_bytes(size_t body_capacity);

/* entries [n_entries] (HOST).  No host synchronisation: n_superframes is read on the device, behind the follow call on
 * the same stream.  Everything is checked before anything is enqueued, so a refused call leaves every output as it was:
 * DABGPU_ERR_ARG for a NULL context or table, a negative count, a bit rate outside 8 .. 512 or no multiple of 8, a negative
 * max_superframes, data_stride < 110*s, a NULL pointer other than d_state_in (and d_slides with max_slides == 0), a state
 * record, the arena or d_slides off its 16-byte boundary, d_state_in and d_state_out that are equal or overlap, d_status,
 * d_follow or d_result off a 4-byte boundary, arena_bytes < dabgpu_mot_arena_bytes(0), a negative max_slides, and with
 * max_slides > 0 a slide_stride below 32 or no multiple of 16, or max_slides * slide_stride >= 2^31. */
int dabgpu_mot_slides_dev(dabgpu_ctx *ctx, const dabgpu_mot_entry *entries, int n_entries, void *stream);
/* the same table with HOST pointers, the same checks, the same walk: no context, no GPU */
int dabgpu_mot_slides_host(const dabgpu_mot_entry *entries, int n_entries);

/* The MOT header of a slide (EN 301 234 clause 6, TS 101 499 clause 6.2), host side. */
typedef struct dabgpu_mot_text {
    int32_t length;             /* -1: the parameter is not there; else 0 .. 255                                 */
    uint8_t bytes[256];         /* bytes behind length are zero                                                  */
} dabgpu_mot_text;

typedef struct dabgpu_mot_header {
    int32_t body_size, header_size, content_type, content_subtype;        /* the header core                    */
    int32_t n_params, n_unknown;    /* parameters in the header extension; those of them not named below          */
    int32_t name_charset;           /* ContentName 0x0C: the charset nibble of its first byte; -1 = no name        */
    int32_t has_trigger, trigger_now;   /* TriggerTime 0x05; now: its validity bit is clear                        */
    uint32_t trigger_time;          /* its first four bytes, big-endian                                            */
    int32_t has_expire, expire_now; /* ExpireTime 0x04, likewise                                                   */
    uint32_t expire_time;
    int32_t has_category, category_id, slide_id;                            /* CategoryID/SlideID 0x25            */
    dabgpu_mot_text name, category_title /* 0x26 */, click_through_url /* 0x27 */, alternative_location_url /* 0x28 */;
} dabgpu_mot_header;

/* header[n]: n must equal the core's header_size.  Parameters by PLI: 0 no data, 1 one byte, 2 four bytes, 3 a length of
 * 7 bits, or of 15 when the first length byte's top bit is set.  Unknown parameters are stepped over by length.  Of a
 * parameter that comes twice the later one holds.  DABGPU_ERR_ARG for NULL, n < 7, header_size != n, a parameter that
 * runs past the header, a ContentName without its charset byte, a time of fewer than 4 bytes, a CategoryID/SlideID of
 * fewer than 2; DABGPU_ERR_CAPACITY for a text longer than 255 bytes.  A refused call writes nothing. */
int dabgpu_mot_header_parse(const uint8_t *header, int n, dabgpu_mot_header *out);

/* ------------------------------------------------------------------------ */
/* Following every DAB (MPEG layer II) sub-channel of a batch to checked frames  */
/* and their PAD on the device -- what stands behind the audio parameters and    */
/* the dynamic label the reference shows for a layer-II channel                   */
/*   (/root/reference/src/render_radio_block.cpp:439-486).                        */
/* The other audio kind of dabgpu_fig_audio_components (ascty == 0).  One entry   */
/* per followed sub-channel; one call takes the n_cifs logical frames every       */
/* entry's decode call produced and two launches: one wave per entry finds the    */
/* sampling rate and the pairing phase, then one lane per frame checks header     */
/* and ISO CRC and whole waves lift the PAD into rows.  The rows, their status    */
/* and d_follow are what dabgpu_pad_labels_dev and dabgpu_mot_slides_dev read:     */
/* point their entries at d_rows / d_status / d_follow with bitrate_kbps =         */
/* DABGPU_MP2_PAD_KBPS, data_stride >= DABGPU_MP2_ROW_BYTES and max_superframes    */
/* = n_cifs + 1, in the same table as the DAB+ entries. */
/*                                                                              */
/* THE CONTRACT -- header, ISO CRC, ScF-CRC bytes, the PAD row, rate and phase,    */
/* the carry record -- stands at the top of include/dabgpu_mp2_frame.h, the one     */
/* implementation the kernels, the host twin and the host mirror run.  In short:    */
/* a frame with a valid header and a good ISO CRC over bit allocation and SCFSI     */
/* becomes one pseudo access unit whose data stream element holds its X-PAD and     */
/* F-PAD (au_crc_mask = 1); any other slot is one lost access unit                  */
/* (au_crc_mask = 0, a row of zeros).  Frames without the ISO CRC (protection       */
/* bit 1) are counted and deliver no PAD.  The ScF-CRC bytes are stepped over, not   */
/* checked.  No audio is decoded here: dabgpu_mp2_subbands_dev below takes the       */
/* GOOD frames on to sub-band samples and audio levels.                             */
/* ------------------------------------------------------------------------ */
#define DABGPU_MP2_ROW_BYTES 220
#define DABGPU_MP2_PAD_KBPS 16

typedef struct dabgpu_mp2_result {
    int32_t id;                 /* 1 = MPEG-1 (48 kHz), 0 = LSF (24 kHz), -1 = no rate found                 */
    int32_t sample_rate;        /* 48000, 24000 or 0                                                         */
    int32_t bitrate_kbps;       /* the entry's, 0 with no rate                                               */
    int32_t mode;               /* 0 stereo, 1 joint stereo, 2 dual channel, 3 single channel; -1 = no valid header seen */
    int32_t phase;              /* first frame of F that starts a row; -1 = no rate                           */
    int32_t held;               /* logical frames in carry_out, 0 or 1                                        */
    int32_t synced;             /* what carry_out says                                                       */
    int32_t hits;               /* valid headers of either ID among the frames of F                           */
    /* counts of THIS call */
    int32_t frames;             /* rows emitted = header_errors + frames_no_crc + crc_failed + good frames     */
    int32_t header_errors, crc_failed, frames_no_crc;
    int32_t dropped;            /* logical frames of F that belong to no row and are not carried               */
    int32_t reserved[3];
} dabgpu_mp2_result;

typedef struct dabgpu_mp2_entry {           /* HOST array, one per followed sub-channel; every pointer DEVICE memory */
    const uint8_t *d_in;        /* [n_cifs][in_stride] logical frames: the d_out[j] of the decode calls            */
    size_t in_stride;           /* >= bitrate*3                                                                    */
    int32_t bitrate_kbps;       /* multiple of 8, 8 .. 384                                                         */
    const void *d_carry_in;     /* dabgpu_mp2_carry_bytes(bitrate) bytes on a 16-byte boundary, or NULL = fresh start; */
                                /* a record this library did not write (all zero included) is a fresh start too     */
    void *d_carry_out;          /* same size and alignment; != d_carry_in; overlaps nothing else of the call        */
    uint8_t *d_rows;            /* [n_cifs + 1][DABGPU_MP2_ROW_BYTES]                                              */
    dabgpu_superframe_status *d_status;      /* [n_cifs + 1]                                                       */
    dabgpu_dabplus_follow_result *d_follow;  /* one record: n_superframes = rows emitted, phase, synced, dropped,   */
                                             /* raw_hits = hits, held -- what the PAD entries' d_follow points at   */
    dabgpu_mp2_result *d_result;             /* one record                                                         */
} dabgpu_mp2_entry;

/* bytes of one carry record: a 16-byte header and one logical frame of bitrate*3 bytes, rounded up to 16; 0 for a bit
 * rate the follow call refuses */
size_t dabgpu_mp2_carry_bytes(int bitrate_kbps);

/* entries [n_entries] (HOST), any mix of bit rates; n_cifs logical frames per entry.  Everything is checked before anything
 * is enqueued, so a refused call leaves every output as it was: DABGPU_ERR_ARG for a NULL context or table, negative counts,
 * n_cifs above 2^28 (frame indices and row offsets stay within 32 bits),
 * a bit rate outside 8 .. 384 or no multiple of 8, in_stride < bitrate*3, a NULL pointer other than d_carry_in (d_in may be
 * NULL with n_cifs = 0), a carry record off its 16-byte boundary, d_carry_in and d_carry_out that are equal or overlap,
 * d_status, d_follow or d_result off a 4-byte boundary.  No host synchronisation. */
int dabgpu_mp2_follow_dev(dabgpu_ctx *ctx, const dabgpu_mp2_entry *entries, int n_entries, int n_cifs, void *stream);
/* the same table with HOST pointers, the same checks, the same code: no context, no GPU */
int dabgpu_mp2_follow_host(const dabgpu_mp2_entry *entries, int n_entries, int n_cifs);

/* ------------------------------------------------------------------------ */
/* Layer-II services of a batch: sub-band samples and audio levels -- whether    */
/* audio is on a layer-II channel and how loud, the question behind the           */
/* reference's layer-II channel view (its src/render_radio_block.cpp:439-486).    */
/* Behind dabgpu_mp2_follow_dev on the same stream, with no host synchronisation:  */
/* every checked (GOOD) frame of every followed entry goes through the whole      */
/* layer-II decoder except its last stage -- bit allocation, SCFSI, scale factors, */
/* sample unpacking with the grouped code words, requantisation and scaling to     */
/* the 36 x 32 sub-band samples of each channel -- one wave per frame, a lane per   */
/* cell.  Each row of the follow call gets a level record (power and peak per      */
/* channel); the sub-band samples themselves are optional.  The row count, the     */
/* rate and the phase are read on the device from d_result, the held half of a     */
/* 24 kHz frame from d_carry_in; rows at or beyond `frames` are not written.        */
/*                                                                              */
/* THE CONTRACT -- classes, SCFSI, scale factors, grouping, the value of a sample, */
/* the end of the audio, the level record -- stands at the top of                   */
/* include/dabgpu_mp2_audio.h, the one implementation the kernel, the host twin     */
/* and the host mirror run.  The polyphase synthesis to PCM is NOT part of this     */
/* (it needs the 512-tap window of ISO 11172-3 table B.3): power and peak are        */
/* SUB-BAND-DOMAIN figures, where a full-scale sinusoid has a sub-band amplitude     */
/* of about 1; how they map to PCM dBFS is a convention nobody here has measured.    */
/* Silence is power == 0, or a threshold the caller chooses.                         */
/* ------------------------------------------------------------------------ */
typedef struct dabgpu_mp2_level {
    int32_t kind;               /* 0 decoded, 1 not a GOOD frame, 2 overrun: the audio would run into the ScF-CRC or the PAD */
    int32_t channels;           /* 1 or 2; 0 when kind != 0 (as everything below)                            */
    int32_t cells;              /* active (sub-band, channel) cells                                          */
    int32_t scf63;              /* scale-factor indices sent that are the forbidden 63 (factor 0)            */
    float power[2];             /* per channel: the sum of v^2 over its 36 x 32 values                       */
    float peak[2];              /* per channel: max |v|, exact                                               */
} dabgpu_mp2_level;

typedef struct dabgpu_mp2_audio_result {
    int32_t decoded, not_good, overrun;     /* rows of this call by kind; their sum = the follow call's frames */
    int32_t silent;                         /* decoded frames with power[0] + power[1] == 0                    */
    int32_t reserved[4];
} dabgpu_mp2_audio_result;

typedef struct dabgpu_mp2_audio_entry {     /* HOST array, one per followed sub-channel; every pointer DEVICE memory */
    const uint8_t *d_in;        /* the follow entry's d_in                                                         */
    size_t in_stride;           /* >= bitrate*3                                                                    */
    int32_t bitrate_kbps;       /* multiple of 8, 8 .. 384                                                         */
    const void *d_carry_in;     /* the record the FOLLOW call READ (NULL as there), on a 16-byte boundary           */
    const dabgpu_superframe_status *d_status;    /* what the follow call wrote: au_crc_mask says GOOD              */
    const dabgpu_mp2_result *d_result;           /* what the follow call wrote: id, phase, frames                  */
    dabgpu_mp2_level *d_levels;                  /* [n_cifs + 1]                                                   */
    float *d_subbands;          /* NULL, or [n_cifs + 1][2][36][32] (channel, sample, sub-band) on a 16-byte boundary */
    dabgpu_mp2_audio_result *d_audio;            /* one record, written whole by this call                         */
} dabgpu_mp2_audio_entry;

/* entries [n_entries] (HOST), any mix of bit rates; n_cifs as in the follow call.  Everything is checked before anything is
 * enqueued, so a refused call leaves every output as it was: DABGPU_ERR_ARG for a NULL context or table, negative counts,
 * n_cifs above 2^28, a bit rate outside 8 .. 384 or no multiple of 8, in_stride < bitrate*3, a NULL pointer other than
 * d_carry_in and d_subbands (d_in may be NULL with n_cifs = 0), d_carry_in or d_subbands off a 16-byte boundary, d_status,
 * d_result, d_levels or d_audio off a 4-byte boundary.  No host synchronisation. */
int dabgpu_mp2_subbands_dev(dabgpu_ctx *ctx, const dabgpu_mp2_audio_entry *entries, int n_entries, int n_cifs, void *stream);
/* the same table with HOST pointers, the same checks, the same code: no context, no GPU */
int dabgpu_mp2_subbands_host(const dabgpu_mp2_audio_entry *entries, int n_entries, int n_cifs);

/* ------------------------------------------------------------------------ */
/* Packet-mode MOT services of a batch, to their slides, on the device -- what  */
/* the reference renders for a data packet channel                              */
/*   (its src/render_radio_block.cpp:533, 538-540, 592-593).                    */
/* The third kind of service component beside DAB+ and layer II: TMId = 3.       */
/* dabgpu_fig_packet_components (host) lists them; the caller picks those with   */
/* DSCTy 60 (MOT) and DG flag 0 and gives one entry per (sub-channel, packet     */
/* address) to dabgpu_packet_slides_dev, which runs behind                       */
/* dabgpu_decode_ensembles_dev on the same stream, on the n_cifs logical frames  */
/* that call wrote.  Two launches: a scan (one lane  */
/* per 24-byte slot: packet CRCs, the chain of packets of every frame, a list    */
/* of the followed ones) and a walk (one wave per entry: data groups, then the   */
/* slideshow call's own closing, assembly and slot code).  The contract and the  */
/* code are include/dabgpu_packet_walk.h.                                        */
/*                                                                            */
/* Reed-Solomon RS(204,188) correction of FEC frames is a call of its own in      */
/* front of this one, dabgpu_packet_fec_dev (below): this call recognises and     */
/* counts FEC packets and reads what that one wrote, unchanged.  MOT directory    */
/* mode (data group type 6) is dabgpu_packet_carousel_dev (below); the data      */
/* groups of non-MOT components (TPEG, SPI, Journaline) and FIG 0/13 user        */
/* application signalling are dabgpu_packet_groups_dev and                       */
/* dabgpu_fig_user_applications (below).  Not done: compressed directories       */
/* (type 7); conditional access.                                                 */
/*                                                                            */
/* THE CONTRACT of one entry in one call (EN 300 401 clauses 5.3.2, 5.3.3; every  */
/* ambiguity decided).                                                           */
/*                                                                            */
/* A logical frame of a sub-channel with bit rate R has 3 R bytes: S = R / 8      */
/* slots of 24 bytes.  Packets do not straddle frames.  Scan of one frame:        */
/* pos = 0; while pos < S, with h0 h1 h2 the bytes at 24 pos:                     */
/*   L = (h0 >> 6) + 1 slots; addr = ((h0 & 3) << 8) | h1.  First match wins:     */
/*   1. fec non-zero, addr == 1022, L == 1: packets_fec++, pos += 1 (no packet    */
/*      CRC in these 24 bytes; not checked)                                       */
/*   2. pos + L > S: slots_bad++, pos += 1                                        */
/*   3. the FIB's CRC over the first 24 L - 2 bytes (x^16 + x^12 + x^5 + 1,       */
/*      register all ones, complemented, sent big-endian) is not the last two:    */
/*      slots_bad++, pos += 1 (the scan resynchronises at the next slot and does  */
/*      not trust a length it could not check)                                    */
/*   4. a good packet, pos += L: addr == 0: packets_padding++; addr != address:   */
/*      packets_other++; else packets_followed++, and it is followed.             */
/*                                                                            */
/* Followed packets, in frame and position order: ci = (h0 >> 4) & 3,             */
/* first = (h0 >> 3) & 1, last = (h0 >> 2) & 1, cmd = h2 >> 7, udl = h2 & 0x7F.   */
/* "Dropped": an open group is forgotten and groups_unfinished++ (nothing when     */
/* none is open).                                                                 */
/*   a. a followed packet was seen before (this call or an earlier one) and       */
/*      ci != (prev + 1) & 3: continuity_breaks++, dropped.  Then prev = ci.       */
/*   b. udl > 24 L - 5: packets_malformed++, dropped; next packet.                 */
/*   c. cmd: packets_command++; next packet (an open group stays).                 */
/*   d. first: dropped; a new group opens empty, groups_opened++.  Not first and   */
/*      none open: packets_orphan++; next packet.                                  */
/*   e. have + udl > 16384: groups_too_long++, the group is forgotten (it is not   */
/*      counted unfinished); next packet.                                          */
/*   f. the udl bytes from offset 3 are appended; group_bytes += udl.              */
/*   g. last: have < 4: mot.groups_malformed++, the group is forgotten.  Else the   */
/*      group closes with length = have by "Closing a group" and "Assembly" of      */
/*      dabgpu_mot_slides_dev, word for word (CRC flag clear: groups_crc_failed).   */
/* A completed object goes to its slot as there: a dabgpu_mot_slide whose           */
/* superframe = the index of the logical frame in this call and au = the slot       */
/* position of the closing packet, then header and body.                            */
/*                                                                            */
/* cifs = n_cifs, slots = n_cifs S.  Of the embedded dabgpu_mot_result the fields    */
/* only PAD gives (aus .. fields_ignored, lengths_*, groups_no_length, xpad_bytes)   */
/* stay 0.  The state record is opaque (all zero = a fresh start; a record this      */
/* library did not write for an arena of this size is one) and goes with the arena   */
/* from call to call: a group or an object may span any number of calls.  No frame   */
/* is carried.                                                                      */
/* ------------------------------------------------------------------------ */
typedef struct dabgpu_packet_component {
    uint32_t sid; int32_t scid;            /* FIG 0/2 TMId = 3: SCId(12) P/S(1) CA(1)                      */
    int32_t subchid, start_address;        /* FIG 0/3 SubChId joined through FIG 0/1                        */
    int32_t packet_address;                /* FIG 0/3, 10 bits                                              */
    int32_t dscty, dg_flag;                /* FIG 0/3: DSCTy(6) (60 = MOT), DG flag (0 = data groups used)  */
    int32_t fec_scheme;                    /* FIG 0/14 for that SubChId (2 bits), 0 if none seen            */
    int32_t primary, reserved[3];
} dabgpu_packet_component;

/* host only, the sister of dabgpu_fig_audio_components: the packet-mode components (FIG 0/2 TMId = 3, both P/D forms) of
 * CRC-clean FIBs of ONE ensemble, current configuration of this ensemble (C/N = 0, OE = 0), joined through their SCId to
 * FIG 0/3 -- SCId(12) Rfa(3) CAOrg flag(1), DG flag(1) Rfu(1) DSCTy(6), SubChId(6) packet address(10), CAOrg(16) only when
 * its flag is set -- through the SubChId to FIG 0/1 (the start address) and to FIG 0/14 -- entries of SubChId(6) FEC
 * scheme(2).  Sorted by (start address, packet address); each (SubChId, packet address) once (its first component); a
 * component whose FIG 0/3 or whose sub-channel the same FIBs have not announced is left out.  *n receives the count;
 * DABGPU_ERR_CAPACITY if max is too small (nothing written). */
int dabgpu_fig_packet_components(const uint8_t *fib, const uint8_t *crc_ok, int n_frames, dabgpu_packet_component *out, int max,
                                 int *n);

typedef struct dabgpu_packet_result {       /* counts of THIS call */
    int32_t cifs, slots, slots_bad;
    int32_t packets_fec, packets_padding, packets_other, packets_followed;
    int32_t continuity_breaks, packets_malformed, packets_command, packets_orphan;
    int32_t groups_opened, groups_unfinished, groups_too_long;
    int32_t group_bytes;                    /* useful bytes taken into data groups                              */
    int32_t reserved;
    dabgpu_mot_result mot;                  /* from the closed group on                                         */
} dabgpu_packet_result;

typedef struct dabgpu_packet_entry {        /* HOST array, one per (sub-channel, packet address); every pointer DEVICE memory */
    const uint8_t *d_in;        /* [n_cifs][in_stride] logical frames of 3 * bitrate_kbps bytes, any alignment; several
                                 * entries may name the same frames                                               */
    size_t in_stride;           /* >= 3 * bitrate_kbps                                                           */
    int32_t bitrate_kbps;       /* a multiple of 8 in 8 .. 512                                                   */
    int32_t address;            /* the packet address followed, 1 .. 1023                                        */
    int32_t fec;                /* non-zero: the sub-channel carries FEC packets (the component's fec_scheme)    */
    int32_t reserved;
    const void *d_state_in;     /* dabgpu_packet_state_bytes() on a 16-byte boundary; NULL or all zero = fresh start */
    void *d_state_out;          /* same size and alignment; != d_state_in, no overlap                            */
    void *d_arena;              /* as dabgpu_mot_entry: 16-byte boundary, updated in place                       */
    size_t arena_bytes;         /* >= dabgpu_mot_arena_bytes(0); what is beyond it is body_capacity              */
    uint8_t *d_slides;          /* [max_slides] slots, 16-byte boundary; may be NULL with max_slides == 0          */
    size_t slide_stride;        /* a multiple of 16, >= 32                                                       */
    int32_t max_slides;         /* max_slides * slide_stride < 2^31                                              */
    int32_t reserved2;
    dabgpu_packet_result *d_result;
} dabgpu_packet_entry;

size_t dabgpu_packet_state_bytes(void);

/* entries [n_entries] (HOST).  No host synchronisation.  Everything is checked before anything is enqueued, so a refused call
 * leaves every output as it was: DABGPU_ERR_ARG for a NULL context or table, a negative count, n_cifs outside 0 .. 2^24, a
 * bit rate outside 8 .. 512 or no multiple of 8, in_stride < 3 * bitrate_kbps, an address outside 1 .. 1023, a NULL d_in with
 * n_cifs > 0, a NULL pointer other than d_in, d_state_in (and d_slides with max_slides == 0), and for the state records, the
 * arena, the slots and d_result what dabgpu_mot_slides_dev refuses; DABGPU_ERR_CAPACITY for a table whose scan would need
 * 2^31 or more workgroups (n_entries times the frames of a call over the frames a wave takes, 64 / S). */
int dabgpu_packet_slides_dev(dabgpu_ctx *ctx, const dabgpu_packet_entry *entries, int n_entries, int n_cifs, void *stream);
/* the same table with HOST pointers, the same checks, the same code: no context, no GPU */
int dabgpu_packet_slides_host(const dabgpu_packet_entry *entries, int n_entries, int n_cifs);

/* ------------------------------------------------------------------------ */
/* FEC frames of packet-mode sub-channels: RS(204,188) correction on the device  */
/* (EN 300 401 clause 5.3.5; the reference has no FEC code at all).               */
/* dabgpu_packet_fec_dev runs on the same stream between                          */
/* dabgpu_decode_ensembles_dev and dabgpu_packet_slides_dev, one entry per        */
/* sub-channel whose component has fec_scheme 1: it   */
/* finds the FEC frames in the logical frames, corrects them and writes logical   */
/* frames that the slides call reads unchanged -- there the caller names d_out as */
/* d_in and keeps fec non-zero; `superframe` of a slide then counts delayed       */
/* frames.  The contract and the code are include/dabgpu_packet_fec.h.            */
/*                                                                            */
/* Not provided: correction of the FEC packets' own bytes in the output; FEC      */
/* schemes other than 1.  This call does not use a failed packet CRC as an        */
/* erasure: dabgpu_packet_fec_erasures_dev (below) does.                          */
/*                                                                            */
/* THE CONTRACT of one entry in one call (every ambiguity decided; where this     */
/* text and the standard's wording could part, this text governs).                */
/*                                                                            */
/* Slots.  Bit rate R: S = R / 8 slots of 24 bytes per logical frame, numbered    */
/* g = 0, 1, ... from a fresh start, across frames and calls.                     */
/*                                                                            */
/* FEC frame.  103 consecutive slots: 94 of application data, A[0..2255] in       */
/* stream order, then 9 FEC packets.  A slot is MARK c when (h0 >> 6) == 0,       */
/* (((h0 & 3) << 8) | h1) == 1022 and c = (h0 >> 2) & 15 is at most 8.            */
/* P[0..197] = bytes 2..23 of the nine FEC packets; P[0..191] is the RS data      */
/* table, P[192..197] is ignored.  Row r (0..11): cw_r[c] = A[12 c + r], c < 188; */
/* cw_r[188 + j] = P[12 j + r], j < 16.  GF(2^8), x^8 + x^4 + x^3 + x^2 + 1,      */
/* alpha = 2; generator prod_{i=0..15} (x + alpha^i); cw_r[0] is the coefficient  */
/* of x^203 (RS(255,239) shortened by 51 leading zeros);                          */
/* S_k = sum_c cw_r[c] alpha^(k (203 - c)), k = 0..15.                            */
/*                                                                            */
/* Finding frames.  No phase is assumed, no lock is kept.  A frame ENDS at slot q  */
/* when at least 7 of the slots q - 8 + i (i = 0..8) are mark i (slots before the  */
/* fresh start are no mark; marks are taken from the bytes as received).           */
/* Candidates in ascending q: first slot q - 102 below 0: frames_cut++; else first */
/* slot at or before the end of the last accepted frame: frames_overlapping++;     */
/* neither is processed.  Else accepted: frames++, processed in the call in which  */
/* its last slot arrives.                                                          */
/*                                                                            */
/* Correction.  Bounded distance, errors only, per row: if a codeword lies within  */
/* Hamming distance 8 of the received 204 bytes (every differing position inside   */
/* the 204; it is unique) the row's 188 data bytes become that codeword's:         */
/* rows_corrected++, bytes_corrected += differing data positions,                  */
/* parity_bytes_corrected += the others.  A codeword as received: rows_clean++.    */
/* Otherwise the row stays as received: rows_uncorrectable++.  The FEC packets     */
/* themselves are written out as received.                                         */
/*                                                                            */
/* Delay.  Output lags input by D = ceil(102 / S) frames (102 at 8 kbit/s, 2 at    */
/* 512): output frame f of a call is stream frame F0 + f - D, F0 the frames seen   */
/* since the fresh start.  Stream frames below 0 are S copies of the padding       */
/* packet 0C 00 00, 19 x 00, CRC (address 0, one slot; packets_padding there).     */
/* The state record is opaque -- F0, the last accepted end, the marks of the last  */
/* 8 slots, the last D frames, corrected where their frame has ended --            */
/* dabgpu_packet_fec_state_bytes(bitrate) of it (at most 3664).  NULL, all zero or */
/* a record this library did not write for this bit rate: a fresh start.  The      */
/* result of a stream does not depend on where it is cut into calls (n_cifs below  */
/* D and n_cifs = 0 included).                                                     */
/* ------------------------------------------------------------------------ */
typedef struct dabgpu_packet_fec_result {   /* counts of THIS call */
    int32_t cifs, slots, marks;             /* n_cifs, n_cifs S, the marks among those slots                    */
    int32_t frames, frames_cut, frames_overlapping;
    int32_t rows_clean, rows_corrected, rows_uncorrectable;
    int32_t bytes_corrected;                /* data positions                                                   */
    int32_t parity_bytes_corrected;
    int32_t reserved;
} dabgpu_packet_fec_result;

typedef struct dabgpu_packet_fec_entry {    /* HOST array, one per sub-channel; every pointer DEVICE memory */
    const uint8_t *d_in;        /* [n_cifs][in_stride] logical frames of 3 * bitrate_kbps bytes, any alignment     */
    size_t in_stride;           /* >= 3 * bitrate_kbps                                                           */
    int32_t bitrate_kbps;       /* a multiple of 8 in 8 .. 512                                                   */
    int32_t reserved;
    uint8_t *d_out;             /* [n_cifs][out_stride], any alignment, no overlap with d_in                     */
    size_t out_stride;          /* >= 3 * bitrate_kbps                                                           */
    const void *d_state_in;     /* dabgpu_packet_fec_state_bytes() on a 16-byte boundary; NULL = fresh start       */
    void *d_state_out;          /* same size and alignment; != d_state_in, no overlap                            */
    dabgpu_packet_fec_result *d_result;
} dabgpu_packet_fec_entry;

/* bytes of the state record of a sub-channel of this bit rate; 0 for a bit rate the call refuses */
size_t dabgpu_packet_fec_state_bytes(int bitrate_kbps);
/* D, the frames the output lags the input; -1 for a bit rate the call refuses */
int dabgpu_packet_fec_delay(int bitrate_kbps);

/* entries [n_entries] (HOST).  No host synchronisation.  Everything is checked before anything is enqueued, so a refused call
 * leaves every output as it was: DABGPU_ERR_ARG for what dabgpu_packet_slides_dev refuses for the same fields (a NULL context
 * or table, a negative count, n_cifs outside 0 .. 2^24, a bit rate outside 8 .. 512 or no multiple of 8, in_stride <
 * 3 * bitrate_kbps, a NULL d_in with n_cifs > 0, a NULL d_state_out or d_result, a state record off a 16-byte boundary,
 * d_result off a 4-byte boundary), out_stride < 3 * bitrate_kbps, a NULL d_out with n_cifs > 0, d_out overlapping d_in of the
 * same entry, d_state_out equal to or overlapping d_state_in; DABGPU_ERR_CAPACITY for a table whose largest launch would need
 * 2^31 or more workgroups. */
int dabgpu_packet_fec_dev(dabgpu_ctx *ctx, const dabgpu_packet_fec_entry *entries, int n_entries, int n_cifs, void *stream);
/* the same table with HOST pointers, the same checks, the same code: no context, no GPU */
int dabgpu_packet_fec_host(const dabgpu_packet_fec_entry *entries, int n_entries, int n_cifs);

/* ------------------------------------------------------------------------ */
/* ... with failed packet CRCs as erasures.  A second pair of calls beside the    */
/* one above, which stays as it is; INTEGRATION.md section 21 says which to       */
/* choose.  The contract is the section "Erasures" of                             */
/* include/dabgpu_packet_fec.h, the code include/dabgpu_packet_fec_erasures.h.    */
/*                                                                            */
/* Suspect slots.  Each logical frame is scanned when it arrives, on its bytes as  */
/* received, by steps 1-4 of the packet scan (dabgpu_packet_slides_dev above, fec  */
/* non-zero): a slot that scan counts as slots_bad is SUSPECT; a slot covered by a */
/* good packet or taken as an FEC packet is not; padding frames below stream       */
/* frame 0 have none.                                                              */
/*                                                                            */
/* Erased columns.  Suspect slot i (0..93) of an accepted frame's data table       */
/* erases columns 2i and 2i + 1 of every row: the set E, f = |E|.  Parity columns  */
/* are never erased.                                                               */
/*                                                                            */
/* A row: 1. a codeword: rows_clean++.  2. Else the errors-only rule above, with   */
/* its counters: what the other call corrects, this one corrects identically.      */
/* 3. Else, if 2 <= f <= 16, the codeword that equals the received row outside E   */
/* except in at most e positions -- e = 0 whenever f <= 16, e >= 1 only when       */
/* 2 e + f <= 14 (it is unique): the row's data bytes become that codeword's,      */
/* rows_erasure_corrected++, erased_bytes_changed += the changed positions in E,   */
/* erasure_other_bytes_corrected += those outside E, data and parity.  4. Else     */
/* rows_uncorrectable++ and the row stays as received.                             */
/*                                                                            */
/* The state record has the size of the other call's                               */
/* (dabgpu_packet_fec_state_bytes) and also carries the suspect bits of the        */
/* carried slots; a record of one call is a fresh start for the other.             */
/*                                                                            */
/* Not provided: correction of the FEC packets' own bytes in the output; erasure   */
/* of parity columns (the FEC packets carry no CRC); FEC schemes other than 1.     */
/* ------------------------------------------------------------------------ */
typedef struct dabgpu_packet_fec_erasure_result {   /* counts of THIS call */
    int32_t cifs, slots, marks;             /* these twelve: as dabgpu_packet_fec_result                        */
    int32_t frames, frames_cut, frames_overlapping;
    int32_t rows_clean, rows_corrected, rows_uncorrectable;
    int32_t bytes_corrected;
    int32_t parity_bytes_corrected;
    int32_t reserved;
    int32_t slots_suspect;                  /* among the call's new slots                                       */
    int32_t frames_with_suspects;           /* accepted frames with f >= 2                                      */
    int32_t frames_beyond_erasures;         /* of those, f > 16: step 3 is closed to their rows                 */
    int32_t rows_erasure_corrected;         /* by step 3                                                        */
    int32_t erased_bytes_changed;           /* positions in E                                                   */
    int32_t erasure_other_bytes_corrected;  /* positions outside E, data and parity                             */
    int32_t reserved2[2];
} dabgpu_packet_fec_erasure_result;

typedef struct dabgpu_packet_fec_erasure_entry {    /* the fields of dabgpu_packet_fec_entry, one by one */
    const uint8_t *d_in;
    size_t in_stride;
    int32_t bitrate_kbps;
    int32_t reserved;
    uint8_t *d_out;
    size_t out_stride;
    const void *d_state_in;     /* dabgpu_packet_fec_state_bytes() on a 16-byte boundary; NULL = fresh start       */
    void *d_state_out;
    dabgpu_packet_fec_erasure_result *d_result;
} dabgpu_packet_fec_erasure_entry;

/* entries [n_entries] (HOST).  No host synchronisation.  Refuses what dabgpu_packet_fec_dev refuses, with the same codes,
 * everything checked before anything is enqueued. */
int dabgpu_packet_fec_erasures_dev(dabgpu_ctx *ctx, const dabgpu_packet_fec_erasure_entry *entries, int n_entries, int n_cifs, void *stream);
/* the same table with HOST pointers, the same checks, the same code: no context, no GPU */
int dabgpu_packet_fec_erasures_host(const dabgpu_packet_fec_erasure_entry *entries, int n_entries, int n_cifs);

/* ------------------------------------------------------------------------ */
/* Packet-mode MOT directory carousels of a batch, to their objects, on the     */
/* device.  Station logos and programme guides (SPI) are sent in MOT directory   */
/* mode (EN 301 234 clause 7.2): a directory object (data group type 6) lists    */
/* every object's transport id and MOT header, and only bodies (type 4) follow.  */
/* A second pair of calls beside dabgpu_packet_slides_*: one entry per            */
/* (sub-channel, packet address), behind dabgpu_decode_ensembles_dev on the same  */
/* stream (and behind either FEC call where there is one), on the same logical    */
/* frames.  Two launches: the scan of                 */
/* dabgpu_packet_slides_dev, unchanged, and a walk (one wave per entry).  The     */
/* contract and the code are include/dabgpu_mot_carousel.h.  The counters of      */
/* either call tell which mode a component speaks: groups_header_mode here,       */
/* groups_ignored_type there.                                                     */
/*                                                                              */
/* Not done: compressed directories (type 7; counted), conditional access,        */
/* decoding of SPI/EPG content, directory extension parameters (their bytes are   */
/* in d_directory at extension_offset), directory mode in X-PAD.  (FIG 0/13:      */
/* dabgpu_fig_user_applications, below.)                                          */
/* ------------------------------------------------------------------------ */
/*
 * THE CONTRACT of one entry (a sub-channel and one packet address) in one call, every ambiguity decided.
 *
 * Frames, packets, groups.  The scan of a frame (steps 1-4) and steps a-g of the followed packets are those of
 * dabgpu_packet_walk.h, word for word, with the same counters in the head of the result (a dabgpu_packet_result; of its
 * embedded dabgpu_mot_result the fields groups_ok .. groups_repeated, segments_*, objects_completed, objects_mismatched,
 * objects_too_large and object_bytes count here, the others stay 0).  A closed group goes through "Closing a group" of
 * dabgpu_mot_slides_dev, word for word, up to the type test, which here is:
 *   type 4: a body segment; type 6: a directory segment; type 3: groups_header_mode++; type 7:
 *   groups_compressed_directory++; any other: groups_ignored_type++.
 * Types 4 and 6 then pass the rest of "Closing a group" (segment flag .. z != end - o; groups_ok++).
 *
 * Placing a segment into the directory or into a body assembly follows "Assembly" of dabgpu_mot_slides_dev from
 * "n >= ..." on, word for word: at most 256 segments for both kinds, at most directory_capacity bytes for the directory and
 * object_capacity for a body.  A segment that is present is not overwritten, so a part may become full by a repetition:
 * segment 0 placed as a non-last segment of S bytes and sent again as the last segment with z <= S bytes makes a part of one
 * segment.  Its length is then what the last-segment group said, z, and its bytes are the first z of those placed first.
 *
 * Directory: one buffer.  For a type-6 segment of transport id t, first match wins:
 *   t equals the current (complete, valid) directory's id -> groups_repeated++, dropped
 *   there is a current directory, or no directory under assembly, or t differs from the id under assembly: the current
 *     directory and its index are forgotten, the delivered marks are cleared, the directory assembly is emptied and takes
 *     t.  Body assemblies are kept.
 *   the assembly is marked too large -> dropped (until the id changes)
 *   else the segment is placed.
 * Directory check: when segments 0 .. last are present, behind the copy that places the last one, the directory of D bytes
 * is checked.  First match wins:
 *   1. D < 13, or the low 30 bits of bytes 0-3 (big-endian) != D         -> directories_mismatched++
 *   2. byte 0 bit 7 (compression) set                                   -> directories_mismatched++
 *   3. N = bytes 4, 5; period = bytes 6-8; segment size = 13 bits of bytes 9, 10; X = bytes 11, 12; o = 13 + X
 *   4. o > D                                                             -> directories_mismatched++
 *   5. N > 256                                                           -> directories_too_large++
 *   6. for i < N: o + 9 > D -> mismatched.  tid = 2 bytes at o; the 7 bytes behind it are the header core: body_size(28)
 *      header_size(13) content_type(6) subtype(9).  header_size < 7 or o + 2 + header_size > D -> mismatched.  Index entry
 *      i = (tid, o + 2, header_size, body_size, type, subtype); o += 2 + header_size.
 *   7. o != D                                                            -> directories_mismatched++
 * On a failure the assembly is emptied and there is no current directory.  Else directories_completed++, it is current (the
 * assembly is emptied, the bytes stay where they are), its D bytes go to d_directory (object_bytes += D), and every body
 * assembly whose id is not in the index is emptied, objects_stale++ each.  A transport id listed twice means its lowest i.
 * directory_id, directory_bytes, directory_objects, directory_period and directory_segment_size of the result describe the
 * directory that is current at the end of the call (also one merely carried in from the state); without one directory_id
 * is -1 and the others 0.
 *
 * Bodies.  A type-4 segment of id t:
 *   1. with a current directory: t not listed -> groups_unlisted++, dropped; t listed and delivered -> groups_repeated++,
 *      dropped.  Without one every body is taken (bodies may arrive before their directory).
 *   2. it goes to the assembly that holds t, else to the lowest-numbered empty one, else the assembly whose stamp is oldest
 *      (lowest number on a tie) is emptied, objects_evicted++, and takes t.  The stamp: a 32-bit count of placed body
 *      segments is kept in the state; an assembly that takes an id is stamped with the count, and with the count after
 *      each of its placed segments; age = (count - stamp) mod 2^32.
 *   3. the assembly is marked too large -> dropped; else the segment is placed (object_bytes += z).
 *
 * Emission: one attempt behind every followed packet, after its orders (and the directory check's) have been executed.
 * Without a current directory nothing.  Else the lowest-numbered assembly that is full (segments 0 .. last) and whose id the
 * directory lists, entry e.  First match wins:
 *   assembled bytes != e's body_size             -> objects_mismatched++, emptied, not marked delivered
 *   32 + header_size + bytes > object_stride     -> objects_dropped++, marked delivered, emptied (object_stride as the entry
 *                                                   gives it, also with max_objects == 0)
 *   objects_written == max_objects               -> objects_deferred++, once per call per assembly; it stays as it is
 *   else slot objects_written of THIS call receives a dabgpu_mot_carousel_object record -- transport_id, content_type,
 *     content_subtype, header_bytes, body_bytes, frame = index of the logical frame in this call, slot = slot position of
 *     the packet this attempt follows, directory_id --, then e's header bytes from the directory, then the body;
 *     objects_written++, objects_completed++, object_bytes += header + body, marked delivered, emptied.
 * A call without followed packets emits nothing.
 *
 * State and arena.  The state record has a fixed size: the packet state, the directory part, 32 body parts, the index of 256
 * entries, the delivered bits, the counts.  All zero = a fresh start; a record this code did not write for exactly these
 * directory_capacity, assemblies and object_capacity is one.  The arena: group buffer [0, 16384) | directory
 * [16384, + directory_capacity rounded up to 16) | K bodies of object_capacity rounded up to 16 each.  It belongs to the
 * state; a group, a directory or an object may span any number of calls, cut anywhere.
 */
typedef struct dabgpu_mot_carousel_object {  /* in front of every object in its slot */
    int32_t transport_id;
    int32_t content_type, content_subtype;  /* of the header core in the directory                                    */
    int32_t header_bytes, body_bytes;       /* the MOT header follows the record, the body follows the header          */
    int32_t frame, slot;                    /* where in this call the object was emitted                               */
    int32_t directory_id;                   /* transport id of the directory that listed it                            */
} dabgpu_mot_carousel_object;

typedef struct dabgpu_packet_carousel_result {  /* counts of THIS call */
    dabgpu_packet_result head;              /* the scan, the followed packets, and from the closed group on            */
    int32_t groups_header_mode, groups_compressed_directory, groups_unlisted;
    int32_t directories_completed, directories_mismatched, directories_too_large;
    int32_t objects_stale, objects_evicted, objects_dropped, objects_deferred, objects_written;
    int32_t directory_id;                   /* of the current directory at the end of the call, -1 = none              */
    int32_t directory_bytes, directory_objects, directory_period, directory_segment_size;
} dabgpu_packet_carousel_result;

typedef struct dabgpu_packet_carousel_entry {   /* HOST array, one per (sub-channel, packet address); every pointer DEVICE memory */
    const uint8_t *d_in;        /* as dabgpu_packet_entry, field by field, down to arena_bytes                    */
    size_t in_stride;
    int32_t bitrate_kbps;
    int32_t address;
    int32_t fec;
    int32_t assemblies;         /* K = 1 .. 32 bodies under assembly at once                                     */
    const void *d_state_in;     /* dabgpu_packet_carousel_state_bytes() on a 16-byte boundary; NULL or all zero = fresh start */
    void *d_state_out;          /* same size and alignment; != d_state_in, no overlap                            */
    void *d_arena;              /* 16-byte boundary, updated in place                                            */
    size_t arena_bytes;         /* >= dabgpu_packet_carousel_arena_bytes(directory_capacity, assemblies, object_capacity) */
    uint8_t *d_objects;         /* [max_objects] slots, 16-byte boundary; may be NULL with max_objects == 0        */
    size_t object_stride;       /* a multiple of 16, >= 32                                                       */
    int32_t max_objects;        /* max_objects * object_stride < 2^31                                            */
    int32_t object_capacity;    /* bytes of a body, per assembly: 0 .. 256 * 8191                                */
    uint8_t *d_directory;       /* [directory_capacity], 16-byte boundary: the bytes of every directory that becomes
                                 * current in this call (the last one wins); else left as it was                 */
    int32_t directory_capacity; /* 16 .. 2^20                                                                    */
    int32_t reserved;
    dabgpu_packet_carousel_result *d_result;
} dabgpu_packet_carousel_entry;

size_t dabgpu_packet_carousel_state_bytes(void);
/* the smallest arena for these sizes (0 for sizes outside their ranges) */
size_t dabgpu_packet_carousel_arena_bytes(int directory_capacity, int assemblies, int object_capacity);

/* entries [n_entries] (HOST).  No host synchronisation.  Everything is checked before anything is enqueued, so a refused call
 * leaves every output as it was: DABGPU_ERR_ARG for what dabgpu_packet_slides_dev refuses for the same fields (d_objects,
 * object_stride and max_objects for d_slides, slide_stride and max_slides), for directory_capacity, assemblies or
 * object_capacity outside their ranges, arena_bytes below dabgpu_packet_carousel_arena_bytes(...), a NULL d_directory or one
 * off its 16-byte boundary; DABGPU_ERR_CAPACITY as there. */
int dabgpu_packet_carousel_dev(dabgpu_ctx *ctx, const dabgpu_packet_carousel_entry *entries, int n_entries, int n_cifs, void *stream);
/* the same table with HOST pointers, the same checks, the same code: no context, no GPU */
int dabgpu_packet_carousel_host(const dabgpu_packet_carousel_entry *entries, int n_entries, int n_cifs);

typedef struct dabgpu_mot_directory {       /* the fixed part of a MOT directory */
    int32_t objects;            /* N                                                                             */
    int32_t period;             /* CarouselPeriod, tenths of a second; 0 = undefined                             */
    int32_t segment_size;       /* 0 = not fixed                                                                 */
    int32_t extension_offset, extension_bytes;      /* the directory extension: 13, X                            */
    int32_t directory_bytes;
    int32_t reserved[2];
} dabgpu_mot_directory;

typedef struct dabgpu_mot_directory_object {
    int32_t transport_id;
    int32_t header_offset, header_bytes;    /* where its MOT header lies in the directory: for dabgpu_mot_header_parse  */
    int32_t body_bytes, content_type, content_subtype;      /* of its header core                                       */
    int32_t reserved[2];
} dabgpu_mot_directory_object;

/* host only: the directory check of the contract above (rules 1-7) over dir[n], as d_directory holds it.  info and
 * out[0 .. *n_out) are written on DABGPU_OK alone: DABGPU_ERR_ARG for a NULL pointer (out may be NULL with max == 0), a
 * negative n or max, or a directory the check refuses; DABGPU_ERR_CAPACITY for more objects than max. */
int dabgpu_mot_directory_parse(const uint8_t *dir, int n, dabgpu_mot_directory *info, dabgpu_mot_directory_object *out, int max,
                               int *n_out);

/* ------------------------------------------------------------------------ */
/* Data groups of ANY packet-mode service component of a batch, on the device:  */
/* TPEG, SPI/EPG, Journaline, filecasting, transparent data channels.  A third   */
/* pair of calls beside dabgpu_packet_slides_* and dabgpu_packet_carousel_*: one */
/* entry per (sub-channel, packet address), behind dabgpu_decode_ensembles_dev   */
/* on the same stream (and behind either FEC call where there is one), on the    */
/* same logical frames.  Mode 0 gives every MSC data  */
/* group (EN 300 401 clause 5.3.3.1) with its header fields read, its CRC         */
/* checked and repeats recognised; mode 1 (the component's DG flag is 1) gives    */
/* the packets' useful bytes as one stream.  Two launches: the scan of            */
/* dabgpu_packet_slides_dev, unchanged, and one workgroup per entry with a lane   */
/* per followed packet (segmented scans, no serial walk).  The contract and the   */
/* code are include/dabgpu_data_groups.h.  dabgpu_fig_user_applications (host)    */
/* says from FIG 0/13 which application a component's data is for.                */
/*                                                                              */
/* Not done: interpreting the content of any application; conditional access.    */
/* ------------------------------------------------------------------------ */
/*
 * THE CONTRACT of one entry (a sub-channel and one packet address) in one call, every ambiguity decided.
 *
 * The scan of a frame (rules 1-4) and steps a-e of "Followed packets" are dabgpu_packet_walk.h's, word for word, with its
 * counters: cifs, slots, slots_bad, packets_*, continuity_breaks, groups_opened, groups_unfinished, groups_too_long,
 * group_bytes.  The cap on a group is 16384 bytes.
 *
 * MODE 0 (the component's DG flag is 0: data groups are used).
 *   f. the udl bytes from offset 3 are appended; group_bytes += udl.
 *   g. last: the group closes with n = have bytes, groups_closed++, and no group is open.  First match wins:
 *        n < 4                                              -> groups_malformed++   (as the slides call decides)
 *        b0 = byte 0: extension flag 0x80, CRC flag 0x40, segment flag 0x20, user access flag 0x10, type = b0 & 0x0F;
 *        byte 1: continuity = high nibble, repetition = low nibble.
 *        CRC flag set and the CRC (the packet CRC's polynomial, start and complement) over bytes 0 .. n - 3 is not bytes
 *          n - 2, n - 1 (big-endian)                        -> groups_crc_failed++  (the CRC is judged before the headers,
 *                                                              as in "Closing a group" of the slideshow contract)
 *        end = n - 2 with the CRC flag, else n; o = 2
 *        extension flag: o + 2 > end -> groups_malformed++; extension = the 16 bits at o; o += 2
 *        segment flag:   o + 2 > end -> groups_malformed++; segment = the 16 bits at o (last(1) number(15)); o += 2
 *        user access flag: o + 1 > end -> groups_malformed++; ua = byte at o; o += 1; li = ua & 0x0F;
 *          transport-id flag (ua & 0x10) set and li < 2 -> groups_malformed++; o + li > end -> groups_malformed++;
 *          transport id = the 16 bits at o when its flag is set; the end user address is the other li - 2 (or li) bytes;
 *          o += li
 *        the group is ACCEPTED: data field = bytes o .. end - 1 (it may be empty).  CRC flag clear: groups_no_crc++.
 *
 * Repeats.  An accepted group is a repeat when the latest earlier accepted group of the same type on this entry (this call
 * or an earlier one, emitted or not) has the same continuity index: groups_repeated++ (whatever keep_repeats says).  With
 * keep_repeats == 0 it is not emitted; otherwise it is, with DG_REPEAT in its flags.
 *
 * Emission.  The groups to emit (accepted, and not a repeat unless repeats are kept) are numbered i = 0, 1, ... in closing
 * order within THIS call; offset_i = the sum over j < i of length_j rounded up to 16 (held at 2^31 once it reaches it).
 * Group i is emitted iff i < max_groups and offset_i + length_i <= bytes_capacity: groups_emitted++, bytes_emitted +=
 * length_i, its n bytes at d_bytes + offset_i and record i at d_groups + i; else groups_no_room++.  The emitted groups are
 * therefore a prefix of the groups to emit.  Records beyond the emitted ones and bytes outside the emitted groups are not
 * written.
 *
 * MODE 1 (DG flag 1: no data groups).  Steps a, b, c as above, except that nothing is ever open: a break leaves a record
 * (below) instead of dropping.  A packet that passes them contributes its udl bytes to one stream; first and last are not
 * looked at.  at = the sum of udl of the contributing packets before it in THIS call.  It is emitted (its bytes at d_bytes +
 * at, bytes_emitted += udl) iff at + udl <= bytes_capacity; else bytes_no_room += udl.  Every continuity break is numbered
 * i = 0, 1, ... within this call; with i < max_groups record i is {offset = at of the packet that broke, length 0, cif, slot,
 * flags = DG_BREAK, every other field 0} and groups_emitted++, else groups_no_room++.  The other groups_* counters stay 0,
 * group_bytes too.
 * An open group in the state record is forgotten without a count.
 *
 * The state record: seen, prev, open, have, the CRC register over the open group (not complemented), the last continuity
 * index per type (16 bytes and a mask), and the open group's bytes (16384; zero behind `have`).  All zero = a fresh start; a
 * record this code did not write is a fresh start, and no value in it makes a call read or write outside the record.  A
 * stream may be cut into calls anywhere; a group may span any number of calls.
 */
#define DABGPU_DG_EXTENSION    1
#define DABGPU_DG_CRC          2    /* a CRC was present, and it was good */
#define DABGPU_DG_SEGMENT      4
#define DABGPU_DG_USER_ACCESS  8
#define DABGPU_DG_TRANSPORT_ID 16
#define DABGPU_DG_REPEAT       32
#define DABGPU_DG_BREAK        64   /* mode 1: a continuity break lies at `offset` of the stream */

typedef struct dabgpu_data_group {          /* 32 bytes */
    int32_t offset, length;                 /* where the whole group lies in d_bytes, and its bytes                     */
    int32_t cif;                            /* index in this call of the frame of the closing packet                    */
    uint8_t slot;                           /* slot position of the closing packet                                      */
    uint8_t type, continuity, repetition;   /* from bytes 0 and 1                                                       */
    uint16_t flags;                         /* DABGPU_DG_*; bits 8-11: the bytes of the end user address                */
    uint16_t extension;                     /* the extension field, 0 without one                                       */
    int32_t segment;                        /* -1, or the 16-bit segment field: last(1) number(15)                      */
    int32_t transport_id;                   /* -1, or the id                                                            */
    uint16_t data_offset, data_length;      /* the data field inside the group                                          */
} dabgpu_data_group;

typedef struct dabgpu_packet_groups_result {    /* counts of THIS call */
    int32_t cifs, slots, slots_bad;
    int32_t packets_fec, packets_padding, packets_other, packets_followed;
    int32_t continuity_breaks, packets_malformed, packets_command, packets_orphan;
    int32_t groups_opened, groups_unfinished, groups_too_long;
    int32_t group_bytes;
    int32_t groups_closed, groups_malformed, groups_crc_failed, groups_no_crc;
    int32_t groups_repeated, groups_emitted, groups_no_room;
    int32_t bytes_emitted, bytes_no_room;
    int32_t reserved[4];
} dabgpu_packet_groups_result;

typedef struct dabgpu_packet_groups_entry {    /* HOST array, one per (sub-channel, packet address); every pointer DEVICE memory */
    const uint8_t *d_in;        /* as dabgpu_packet_entry, field by field, down to fec                           */
    size_t in_stride;
    int32_t bitrate_kbps;
    int32_t address;
    int32_t fec;
    int32_t mode;               /* 0: data groups; 1: no data groups, the useful bytes as a stream               */
    int32_t keep_repeats;       /* mode 0: non-zero = a repeat is emitted, with DABGPU_DG_REPEAT                  */
    int32_t reserved;
    const void *d_state_in;     /* dabgpu_packet_groups_state_bytes() on a 16-byte boundary; NULL or all zero = fresh start */
    void *d_state_out;          /* same size and alignment; != d_state_in, no overlap                            */
    uint8_t *d_bytes;           /* [bytes_capacity], 16-byte boundary; may be NULL with bytes_capacity == 0       */
    dabgpu_data_group *d_groups;/* [max_groups], 4-byte boundary; may be NULL with max_groups == 0                */
    int32_t bytes_capacity;     /* 0 .. 2^31 - 1                                                                 */
    int32_t max_groups;         /* >= 0                                                                          */
    dabgpu_packet_groups_result *d_result;
} dabgpu_packet_groups_entry;

size_t dabgpu_packet_groups_state_bytes(void);
/* the followed packets the kernel takes at a time (its seams lie at multiples of this; for tests and sizing only) */
int dabgpu_packet_groups_chunk(void);

/* entries [n_entries] (HOST).  No host synchronisation.  Everything is checked before anything is enqueued, so a refused call
 * leaves every output as it was: DABGPU_ERR_ARG for what dabgpu_packet_slides_dev refuses for d_in, in_stride, bitrate_kbps,
 * address, n_cifs, the two state records and d_result; for a mode other than 0 or 1, a negative bytes_capacity or max_groups,
 * a NULL d_bytes with bytes_capacity > 0 or one off its 16-byte boundary, a NULL d_groups with max_groups > 0 or one off its
 * 4-byte boundary.  DABGPU_ERR_CAPACITY as there, and for n_cifs * 3 * bitrate_kbps >= 2^31 (the stream offsets of a call are
 * int32). */
int dabgpu_packet_groups_dev(dabgpu_ctx *ctx, const dabgpu_packet_groups_entry *entries, int n_entries, int n_cifs, void *stream);
/* the same table with HOST pointers, the same checks, the same code: no context, no GPU */
int dabgpu_packet_groups_host(const dabgpu_packet_groups_entry *entries, int n_entries, int n_cifs);

typedef struct dabgpu_user_application {
    uint32_t sid; int32_t scids;            /* FIG 0/13: SId, SCIdS                                          */
    int32_t ua_type;                        /* user application type, 11 bits.  Registered in TS 101 756:    */
                                            /*   0x002 MOT slideshow                                         */
                                            /*   0x004 TPEG                                                  */
                                            /*   0x007 SPI (programme guide, logos)                          */
                                            /*   0x00D filecasting                                           */
                                            /*   0x44A Journaline                                            */
    int32_t tmid_packet;                    /* 1: FIG 0/8 joins it to a packet-mode component (an SCId); 0: to a sub-channel, or
                                             * the same FIBs carry no FIG 0/8 for it                         */
    int32_t subchid, scid, packet_address;  /* -1 where the same FIBs do not say                             */
    int32_t data_length;                    /* 0 .. 23 bytes of user application data                        */
    uint8_t data[23];
    uint8_t reserved;
} dabgpu_user_application;

/* host only, the sister of dabgpu_fig_packet_components: the user applications (FIG 0/13) of CRC-clean FIBs of ONE ensemble,
 * current configuration of this ensemble (C/N = 0, OE = 0).  The FIG is a sequence of entries: SId (16 bits with P/D = 0, 32
 * with P/D = 1), SCIdS(4) number of user applications(4), and per application type(11) data length(5) and that many bytes
 * (an entry or an application cut off by the FIG's end ends the FIG).  Each (SId, SCIdS, type) is reported once, its first.
 * It is joined through FIG 0/8 (SId, Ext(1) Rfa(3) SCIdS(4), then L/S(1): 0 = MSC/FIC flag(1) SubChId(6), 1 = Rfa(3) SCId(12);
 * an Rfa byte behind it with Ext) to its component -- the first FIG 0/8 of that (SId, SCIdS), wherever it lies among the
 * FIBs; a short-form entry whose MSC/FIC flag is 1 names a FIDC, not a sub-channel, and is passed over as if absent -- and
 * for a packet-mode component on through FIG 0/3 to its subchid and packet_address.  Sorted by (sid, scids, ua_type).  *n
 * receives the count; DABGPU_ERR_CAPACITY if max is too small (nothing written).  The types are not interpreted.  At most
 * 256 applications, 256 FIG 0/8 entries and 256 FIG 0/3 entries are kept, the first ones; what lies beyond is passed over. */
int dabgpu_fig_user_applications(const uint8_t *fib, const uint8_t *crc_ok, int n_frames, dabgpu_user_application *out, int max,
                                 int *n);

/* ------------------------------------------------------------------------ */
/* A9 on its own: batched punctured soft Viterbi (K=7, rate 1/4).             */
/* Replaces the `viterbi` package (/root/reference/CMakeLists.txt:53-54).     */
/* punct     [n_codewords][n_punct] int8 punctured soft bits                   */
/* mask      HOST pointer, 4*nsteps flags (1 = transmitted)                    */
/* out_bits  [n_codewords][(nsteps-6)/8] bytes, MSB first, NOT descrambled     */
/*                                                                            */
/* A DIAGNOSTIC entry point: no call of the reference's path reaches it (the  */
/* FIC and every sub-channel go through dabgpu_fic_decode* / dabgpu_msc_decode* */
/* / dabgpu_decode_*frames*, whose codewords all have nsteps = 96 k + 6 and run */
/* on viterbi_rot_kernel or the lane kernels).  Lengths that are NOT 96 k + 6  */
/* are decoded by a fourth implementation, viterbi_wave_kernel, which no DAB    */
/* profile uses and which exists for this call alone: it lets the tests hold    */
/* the decoder to an exhaustive maximum-likelihood search on short codewords    */
/* (tests/test_gpu_parity.py) and tools/decoder_fuzz.py hold all implementations */
/* to each other.  Not tuned, not part of any measured figure.                  */
/* ------------------------------------------------------------------------ */
int dabgpu_viterbi_dev(dabgpu_ctx *ctx, const int8_t *d_punct, int n_codewords, const uint8_t *mask,
                       int nsteps, uint8_t *d_out_bytes, void *stream);
int dabgpu_viterbi(dabgpu_ctx *ctx, const int8_t *punct, int n_codewords, const uint8_t *mask,
                   int nsteps, uint8_t *out_bytes);

/* ------------------------------------------------------------------------ */
/* T-DMB: stream-mode data sub-channels (FIG 0/2, TMId 1, DSCTy 24) to checked  */
/* MPEG-2 TS packets, on the device (ETSI TS 102 427).  One entry per (stream,   */
/* stream-mode sub-channel), behind dabgpu_decode_ensembles_dev,                 */
/* dabgpu_eti_read_dev or dabgpu_edi_read_dev on the same stream, on the logical  */
/* frames those calls leave.  Three launches whatever */
/* the number of entries: sync (a workgroup per entry, a lane per phase), gather  */
/* and RS(204,188) (a workgroup per packet), continuity (a workgroup per entry).  */
/* The contract, every ambiguity decided, and the code are include/dabgpu_dmb.h:  */
/* sync search over all 204 phases (lock after 5 sync bytes 204 apart, loss after */
/* 8 misses), the 12-branch convolutional de-interleaver as a gather              */
/* x[i] = y[s + 204 (i mod 12) + i], the outer code of dabgpu_packet_fec_dev,     */
/* continuity counters of all 8192 PIDs and a census of the first 32.  The output */
/* of a stream does not depend on where it is cut into calls.                     */
/*                                                                              */
/* With less room than dabgpu_dmb_max_packets the packets that do not fit wait in   */
/* the state record (up to 64) and come out first in the next call.                */
/*                                                                              */
/* Not provided: anything inside the TS; erasure decoding.                         */
/* ------------------------------------------------------------------------ */
#define DABGPU_DSCTY_MPEG2_TS 24            /* TS 101 756 table 2: MPEG-2 transport stream (T-DMB) */
#define DABGPU_DMB_TS_BYTES 188
#define DABGPU_DMB_CENSUS 32
#define DABGPU_DMB_DEFER_ROOM 64
enum { DABGPU_DMB_AS_RECEIVED = 0, DABGPU_DMB_CORRECTED = 1, DABGPU_DMB_UNCORRECTABLE = 2 };
#define DABGPU_DMB_EXEMPT 1                 /* record flag: discontinuity_indicator set in an adaptation field of length >= 1 */

typedef struct dabgpu_dmb_record {          /* one emitted TS packet */
    uint8_t status;                         /* DABGPU_DMB_AS_RECEIVED / _CORRECTED / _UNCORRECTABLE (then byte 1 |= 0x80 in d_ts) */
    uint8_t corrected_data, corrected_parity;
    uint8_t byte3;                          /* transport_scrambling_control << 6 | adaptation_field_control << 4 | continuity_counter */
    uint16_t pid;
    uint8_t flags;                          /* DABGPU_DMB_EXEMPT */
    uint8_t reserved;
    uint32_t position;                      /* of the packet's first byte in the sub-channel's byte stream, modulo 2^32 */
    uint32_t reserved2;
} dabgpu_dmb_record;

typedef struct dabgpu_dmb_result {          /* counts of THIS call, then where the stream stands */
    int32_t cifs, bytes;
    int32_t sync_hits;                      /* sync bytes found where the lock looked for them */
    int32_t locks, lock_losses;
    int32_t packets_emitted, packets_clean, packets_corrected, packets_uncorrectable;
    int32_t packets_dropped;                /* of a lock that was lost before they were complete */
    int32_t bytes_corrected, parity_bytes_corrected;
    int32_t discontinuities, duplicates;
    int32_t locked, phase;                  /* at the end of the call; phase = lock position mod 204, -1 unlocked */
    int32_t pids, pids_overflowed;          /* cumulative: census entries in use; distinct PIDs that found it full */
    int32_t packets_deferred;               /* waiting in d_state_out: the next call emits them first                */
    int32_t packets_lost;                   /* of this call: beyond max_packets and beyond the 64 the record holds   */
} dabgpu_dmb_result;

typedef struct dabgpu_dmb_census_entry {    /* cumulative, since the fresh start */
    uint16_t pid, reserved;
    uint32_t packets, discontinuities, duplicates, scrambled;
} dabgpu_dmb_census_entry;

typedef struct dabgpu_dmb_entry {           /* HOST array, one per sub-channel; every pointer DEVICE memory */
    const uint8_t *d_in;        /* [n_cifs][in_stride] logical frames of 3 * bitrate_kbps bytes, any alignment     */
    size_t in_stride;           /* >= 3 * bitrate_kbps                                                           */
    int32_t bitrate_kbps;       /* a multiple of 8 in 8 .. 1824                                                  */
    int32_t max_packets;        /* room in d_ts and d_records, >= 0; dabgpu_dmb_max_packets() holds everything   */
    uint8_t *d_ts;              /* [max_packets][188], 16-byte boundary: the emitted packets back to back         */
    dabgpu_dmb_record *d_records; /* [max_packets], 16-byte boundary                                             */
    const void *d_state_in;     /* dabgpu_dmb_state_bytes() on a 16-byte boundary; NULL = fresh start            */
    void *d_state_out;          /* same size and alignment; != d_state_in, no overlap                            */
    dabgpu_dmb_result *d_result;
} dabgpu_dmb_entry;

/* bytes of a state record (any bit rate) */
size_t dabgpu_dmb_state_bytes(void);
/* the most packets a call of n_cifs frames can emit: ceil(3 * bitrate_kbps * n_cifs / 204) that it completes and the
 * DABGPU_DMB_DEFER_ROOM an earlier call may have deferred; -1 for what the call refuses.  With less room only the first
 * max_packets are emitted (packets, records, counts by status, continuity and census: all at emission); the next up to
 * DABGPU_DMB_DEFER_ROOM wait in d_state_out and are emitted first by the next call (packets_deferred); the rest are
 * packets_lost.  While nothing is lost the output of a stream does not depend on the room given either. */
int dabgpu_dmb_max_packets(int bitrate_kbps, int n_cifs);
/* the census of a state record on HOST memory (NULL, all zero or foreign: none): up to DABGPU_DMB_CENSUS entries into
 * `census`, in the order the PIDs first appeared; returns how many, or DABGPU_ERR_ARG */
int dabgpu_dmb_state_census(const void *state, int bitrate_kbps, dabgpu_dmb_census_entry *census);

/* host only, the sister of dabgpu_fig_audio_components and dabgpu_fig_packet_components: the stream-mode data components
 * (FIG 0/2 TMId = 1, both P/D forms: DSCTy(6), SubChId(6), P/S(1), CA flag(1)) of CRC-clean FIBs of ONE ensemble, current
 * configuration of this ensemble (C/N = 0, OE = 0), joined through the SubChId to FIG 0/1 for the start address -- which is
 * also what joins a component to its dabgpu_subchannel among the entries of dabgpu_fig_subchannels.  Sorted by start
 * address; each SubChId once (its first component); a component whose sub-channel the same FIBs have not announced is left
 * out.  Components are reported, not judged: dscty == DABGPU_DSCTY_MPEG2_TS is what dabgpu_dmb_follow_dev is for, whether
 * another DSCTy is followed is the caller's choice.  *n receives the count; DABGPU_ERR_CAPACITY if max is too small (nothing
 * written). */
typedef struct dabgpu_stream_component {
    uint32_t sid;               /* 16-bit (P/D = 0) or 32-bit (P/D = 1) service identifier */
    int32_t subchid;
    int32_t start_address;      /* CU, as dabgpu_subchannel.start_address                 */
    int32_t dscty;              /* TS 101 756 table 2; 24 = MPEG-2 transport stream        */
    int32_t primary;            /* P/S flag                                                */
    int32_t ca;                 /* CA flag                                                 */
    int32_t reserved[2];
} dabgpu_stream_component;
int dabgpu_fig_stream_components(const uint8_t *fib, const uint8_t *crc_ok, int n_frames, dabgpu_stream_component *out, int max,
                                 int *n);

/* host only: the programmes of a buffer of TS packets [n_packets][188] (ISO/IEC 13818-1 clauses 2.4.4.3 and 2.4.4.8), as
 * dabgpu_dmb_follow_dev leaves them in d_ts.  PAT sections (PID 0, table_id 0) and the PMT sections (table_id 2) of the PIDs the
 * PAT names are assembled through pointer_field and continuation packets (adaptation fields skipped; a packet with the
 * transport_error_indicator set, or a continuity counter out of order, ends the section being assembled), checked with
 * CRC-32/MPEG-2 (a section that fails counts in crc_errors and is ignored) and taken when current_next_indicator is set.
 * Listed: programme numbers with their PMT PID in PAT order (programme 0 names the network PID and is no programme), and per
 * programme whose PMT was seen: PCR PID, whether an IOD descriptor (tag 0x1D) stands in its programme info, and the
 * elementary streams (stream_type, PID) in PMT order.  A later section of the same table replaces the earlier one.  Nothing
 * of SL, OD, BIFS or the video is interpreted.  Programmes beyond DABGPU_TS_MAX_PROGRAMS and streams beyond
 * DABGPU_TS_MAX_STREAMS are counted in n_programs / n_streams but not stored.  DABGPU_ERR_ARG for a NULL pointer or a
 * negative count. */
#define DABGPU_TS_MAX_PROGRAMS 16
#define DABGPU_TS_MAX_STREAMS 16
typedef struct dabgpu_ts_program {
    int32_t program_number, pmt_pid;
    int32_t pmt_seen;                       /* a PMT section of this programme checked; the fields below are valid  */
    int32_t pcr_pid, iod_present, n_streams;
    int32_t stream_type[DABGPU_TS_MAX_STREAMS], stream_pid[DABGPU_TS_MAX_STREAMS];
} dabgpu_ts_program;
typedef struct dabgpu_ts_info {
    int32_t transport_stream_id;            /* -1: no PAT seen                                                      */
    int32_t network_pid;                    /* -1: none named                                                       */
    int32_t n_programs;
    int32_t pat_sections, pmt_sections;     /* sections that checked                                                */
    int32_t crc_errors;
    int32_t reserved[2];
    dabgpu_ts_program programs[DABGPU_TS_MAX_PROGRAMS];
} dabgpu_ts_info;
int dabgpu_ts_programs(const uint8_t *ts, int n_packets, dabgpu_ts_info *info);

/* entries [n_entries] (HOST).  No host synchronisation.  Everything is checked before anything is enqueued, so a refused call
 * leaves every output as it was: DABGPU_ERR_ARG for a NULL context or table, a negative count, n_cifs outside 0 .. 2^16, a bit
 * rate outside 8 .. 1824 or no multiple of 8, in_stride < 3 * bitrate_kbps, a NULL d_in with n_cifs > 0, a negative
 * max_packets, a NULL d_ts or d_records with max_packets > 0, a NULL d_state_out or d_result, d_ts, d_records or
 * a state record off a 16-byte boundary, d_result off a 4-byte boundary, d_state_out equal to or overlapping d_state_in;
 * DABGPU_ERR_CAPACITY for more than 65535 entries, or when n_entries times the largest entry's ceil(3 * bitrate_kbps * n_cifs /
 * 204) reaches 2^24 (a workgroup of 256 lanes per packet: the launch's thread count stays below 2^32). */
int dabgpu_dmb_follow_dev(dabgpu_ctx *ctx, const dabgpu_dmb_entry *entries, int n_entries, int n_cifs, void *stream);
/* the same table with HOST pointers, the same checks, the serial code of include/dabgpu_dmb.h: no context, no GPU */
int dabgpu_dmb_follow_host(const dabgpu_dmb_entry *entries, int n_entries, int n_cifs);

/* ------------------------------------------------------------------------ */
/* Timing helper: duration (ms) of the launches of each kernel family,         */
/* measured with hipEvents on the launch stream, around the kernel launch       */
/* alone, while dabgpu_set_timing(ctx,1) is on (every call to it starts a new   */
/* measurement).  which: 0 = ofdm front end, 1 = fic (alone), 2 = msc / grouped */
/* decode (dabgpu_decode_frames*: the FIC is part of the grouped launch),        */
/* 3 = fft stage.  _last_ = the most recent launch; _mean_ = the mean over the  */
/* launches since timing was switched on (at most the last 32) and how many     */
/* that were.  Both wait for the launches they read.  _mean_ only: 4 / 5 / 6 =  */
/* the parts of 2 when it was the grouped codeword-per-lane launch (batches of  */
/* >= 24 576 codewords): forward pass | traceback | de-interleaver history copy */
/* (DABGPU_ERR_ARG when no timed call took that path).  A call has these parts  */
/* only when its whole list went out as ONE forward and ONE traceback launch:   */
/* dabgpu_decode_frames* / dabgpu_msc_decode_multi_dev with at most 16 entries  */
/* (the FIC is one), or dabgpu_decode_ensembles_dev through its table.  A longer */
/* list is several launch pairs: it counts for 2 and is passed over by 4 / 5 / 6. */
/* 7 (both calls) = the ETI launches of dabgpu_eti_frames_dev.                  */
/* 8 / 9 (both calls) = dabgpu_modulate_eti_dev: the encoder with its pre-pass | */
/* the symbol kernel.                                                           */
/* ------------------------------------------------------------------------ */
int dabgpu_set_timing(dabgpu_ctx *ctx, int enable);
int dabgpu_last_kernel_ms(dabgpu_ctx *ctx, int which, float *ms);
int dabgpu_mean_kernel_ms(dabgpu_ctx *ctx, int which, float *mean_ms, int *launches);

#ifdef __cplusplus
}
#endif
#endif
