// decode_plan.hpp -- what the channel-decoder entry points (dabgpu_decode_api.hip, the channel BER of dabgpu_measure_api.hip,
// the ring of dabgpu_pipeline.hip) state once: a sub-channel list checked and resolved to its code tables, the kernels'
// arguments for one entry, the lane kernels' work buffer, the packed result block.  Internal to libdabgpu.
#pragma once
#include "dabgpu_ctx.hpp"

namespace dabapi {

inline int subchannel_profile(const dabgpu_subchannel *sc, dab::PunctureProfile &prof) {
    if (!sc) return DABGPU_ERR_ARG;
    int size_cu = 0;
    if (sc->is_uep) {
        if (!dab::make_uep_profile(dab::uep_table_index(sc->bitrate_kbps, sc->protection_level), prof, size_cu)) return DABGPU_ERR_PROFILE;
    } else if (!dab::make_eep_profile(sc->eep_type, sc->protection_level, sc->bitrate_kbps, prof, size_cu)) {
        return DABGPU_ERR_PROFILE;
    }
    if (size_cu != sc->length) return DABGPU_ERR_PROFILE;
    if (sc->start_address < 0 || sc->start_address + sc->length > 864) return DABGPU_ERR_ARG;
    return DABGPU_OK;
}

// the sub-channel's code tables through the context's descriptor cache (see dabgpu_ctx::code_by_descriptor); the same
// checks and status codes as subchannel_profile
inline int lookup_code(dabgpu_ctx *ctx, const dabgpu_subchannel *sc, DeviceCode **out) {
    if (!sc) return DABGPU_ERR_ARG;
    const uint64_t key = (uint64_t(sc->is_uep != 0) << 63) | (uint64_t(uint32_t(sc->eep_type) & 0xFu) << 56) |
                         (uint64_t(uint32_t(sc->protection_level) & 0xFFu) << 48) | (uint64_t(uint32_t(sc->bitrate_kbps) & 0xFFFFFFu) << 16) |
                         uint64_t(uint32_t(sc->length) & 0xFFFFu);
    // (the key holds the fields masked: only a descriptor whose fields fit their masks may use -- or fill -- the cache)
    const bool in_range = sc->eep_type >= 0 && sc->eep_type <= 15 && sc->protection_level >= 0 && sc->protection_level <= 255 &&
                          sc->bitrate_kbps >= 0 && sc->bitrate_kbps <= 0xFFFFFF && sc->length >= 0 && sc->length <= 0xFFFF;
    auto it = in_range ? ctx->code_by_descriptor.find(key) : ctx->code_by_descriptor.end();
    if (it == ctx->code_by_descriptor.end()) {
        dab::PunctureProfile prof;
        int rc = subchannel_profile(sc, prof);
        if (rc) return rc;
        // a length no decoder holds gets no device tables (they would stay allocated for the context's lifetime)
        if (!dabk::viterbi_fits(prof.nsteps) && !dabk::lane_supported(prof.nsteps)) return DABGPU_ERR_CAPACITY;
        DeviceCode *dc = nullptr;
        if ((rc = get_code(ctx, std::move(prof), &dc))) return rc;
        // (ctx->codes only ever grows until dabgpu_destroy frees it: the pointers kept here stay valid for the context's life)
        if (in_range) ctx->code_by_descriptor[key] = dc;
        *out = dc;
        return DABGPU_OK;
    }
    if (sc->start_address < 0 || sc->start_address + sc->length > 864) return DABGPU_ERR_ARG;
    *out = it->second;
    return DABGPU_OK;
}

// A sub-channel list checked and resolved, once per entry point and before anything is enqueued or any kept state is
// touched: every entry's descriptor and output pointer in list order (lookup_code's status, DABGPU_ERR_ARG for a null
// pointer), then no capacity unit used twice (subchannels_disjoint).  `rc` is the call's status; when it is DABGPU_OK
// the bodies take each entry's code tables and sizes from here.  (n >= 0 is the caller's check.)
struct SubchannelPlan {
    const dabgpu_subchannel *sc;
    int n;
    std::vector<DeviceCode *> code;
    int rc = DABGPU_OK;
    template <class T>
    SubchannelPlan(dabgpu_ctx *ctx, const dabgpu_subchannel *sc_, int n_, T *const *out) : sc(sc_), n(n_), code(size_t(n_), nullptr) {
        if (n > 0 && (!sc || !out)) rc = DABGPU_ERR_ARG;
        for (int i = 0; !rc && i < n; i++)
            if (!(rc = lookup_code(ctx, &sc[i], &code[size_t(i)])) && !out[i]) rc = DABGPU_ERR_ARG;
        if (!rc && !subchannels_disjoint(sc, n)) rc = DABGPU_ERR_ARG;
    }
    // decoded bytes of entry i: per CIF, and of `n_frames` frames
    size_t cif_bytes(int i) const { return size_t(code[size_t(i)]->prof.nsteps - 6) / 8; }
    size_t out_bytes(int i, size_t n_frames) const { return n_frames * dab::NB_CIFS * cif_bytes(i); }
};

// The ragged counterpart: n_streams lists one after the other, stream s owning entries first[s] .. first[s + 1] - 1
// (dabgpu_decode_ensembles_dev).  The same checks and status codes per stream, in stream order, before anything is
// enqueued: the shape of `first` (starts at 0, never decreases, at most MAX_PER_STREAM entries a stream), then every entry's
// descriptor and output pointer, then no capacity unit used twice INSIDE a stream -- different streams are different
// ensembles and may use the same units.  Codes come through lookup_code, so the descriptor cache is shared.
struct EnsemblePlan {
    static constexpr int MAX_PER_STREAM = 64;     // what a multiplex can announce (FIG 0/1: 6-bit SubChId)
    const dabgpu_subchannel *sc;
    const int32_t *first;
    int n_streams;
    int total = 0;
    std::vector<DeviceCode *> code;
    int rc = DABGPU_OK;
    template <class T>
    EnsemblePlan(dabgpu_ctx *ctx, const dabgpu_subchannel *sc_, const int32_t *first_, int n_streams_, T *const *out)
        : sc(sc_), first(first_), n_streams(n_streams_) {
        if (!first || first[0] != 0) { rc = DABGPU_ERR_ARG; return; }
        for (int s = 0; s < n_streams; s++)
            if (first[s + 1] < first[s] || first[s + 1] - first[s] > MAX_PER_STREAM) { rc = DABGPU_ERR_ARG; return; }
        total = first[n_streams];
        if (total > 0 && (!sc || !out)) { rc = DABGPU_ERR_ARG; return; }
        code.assign(size_t(total), nullptr);
        for (int s = 0; !rc && s < n_streams; s++) {
            for (int i = first[s]; !rc && i < first[s + 1]; i++)
                if (!(rc = lookup_code(ctx, &sc[i], &code[size_t(i)])) && !out[i]) rc = DABGPU_ERR_ARG;
            if (!rc && !subchannels_disjoint(sc + first[s], count(s))) rc = DABGPU_ERR_ARG;
        }
    }
    int count(int s) const { return first[s + 1] - first[s]; }
};

// the decode / history / BER kernels' arguments for one sub-channel of a batch of frames
inline dabk::MscArgs msc_args(const dabgpu_subchannel &sc, const int8_t *d_soft, size_t soft_stride, int n_streams, int frames_per_stream,
                              const int8_t *hist_in, int8_t *hist_out, uint8_t *out) {
    dabk::MscArgs a{};
    a.soft = d_soft;
    a.soft_stride = soft_stride;
    a.n_streams = n_streams;
    a.frames_per_stream = frames_per_stream;
    a.start_bit = sc.start_address * dab::CU_BITS;
    a.nbits = sc.length * dab::CU_BITS;
    a.hist_in = hist_in;
    a.hist_out = hist_out;
    a.out = out;
    return a;
}

// The lane kernels' work buffer (ctx->d_lane_scratch), grown to at least `need` bytes; what it held is gone when it grows.
// Returns whether the buffer is there.  When it is not, *rc is DABGPU_ERR_HIP if the stream failed and DABGPU_OK if the
// device had no room: what that means is the caller's policy.
inline bool lane_scratch(dabgpu_ctx *ctx, size_t need, hipStream_t s, int *rc) {
    *rc = DABGPU_OK;
    if (ctx->lane_scratch_bytes >= need) return true;
    // growing the buffer must not race with work still using the old one
    if (hipStreamSynchronize(s) != hipSuccess) { *rc = DABGPU_ERR_HIP; return false; }
    if (ctx->d_lane_scratch) (void)hipFree(ctx->d_lane_scratch);
    ctx->d_lane_scratch = nullptr;
    ctx->lane_scratch_bytes = 0;
    if (hipMalloc(&ctx->d_lane_scratch, need) != hipSuccess) { ctx->d_lane_scratch = nullptr; return false; }
    ctx->lane_scratch_bytes = need;
    return true;
}

// The packed result block of the frame calls: [fib | crc | out_0 | out_1 ... (| fic ber | msc ber of the entries that ask
// for one ... | mer)], every part on a 256-byte boundary.  Offsets in bytes from the block's start; the FIBs are at 0.
struct ResultLayout {
    static size_t al(size_t v) { return (v + 255) & ~size_t(255); }
    size_t nb_fib, nb_crc, nb_ber, nb_mer;            // bytes of the FIBs, the CRC flags, one BER block, the MER block
    size_t off_crc, off_fic_ber = 0, off_mer = 0, total;
    std::vector<size_t> off_out, out_bytes, off_msc_ber;   // per entry of the plan (off_msc_ber: 0 where none is wanted)
    ResultLayout(size_t n_frames, const SubchannelPlan &plan, bool fic_ber = false, dabgpu_ber_count *const *msc_ber = nullptr,
                 bool mer = false)
        : nb_fib(n_frames * dab::NB_FIBS * 32), nb_crc(n_frames * dab::NB_FIBS), nb_ber(n_frames * dab::NB_CIFS * sizeof(dabgpu_ber_count)),
          nb_mer(n_frames * sizeof(dabgpu_mer)), off_crc(al(nb_fib)), total(al(nb_fib) + al(nb_crc)), off_out(size_t(plan.n)),
          out_bytes(size_t(plan.n)), off_msc_ber(size_t(plan.n), 0) {
        auto take = [this](size_t bytes) { const size_t off = total; total += al(bytes); return off; };
        for (int i = 0; i < plan.n; i++) off_out[size_t(i)] = take(out_bytes[size_t(i)] = plan.out_bytes(i, n_frames));
        if (fic_ber) off_fic_ber = take(nb_ber);
        for (int i = 0; i < plan.n; i++)
            if (msc_ber && msc_ber[i]) off_msc_ber[size_t(i)] = take(nb_ber);
        if (mer) off_mer = take(nb_mer);
    }
};

// dabgpu_decode_frames_dev behind its checks, for the entry points that have built the plan themselves (defined in
// dabgpu_decode_api.hip): at least one frame, a stride that holds it, no null pointer
int decode_frames_planned(dabgpu_ctx *ctx, const SubchannelPlan &plan, const int8_t *d_soft, size_t soft_stride, int n_streams,
                          int frames_per_stream, uint8_t *d_fib, uint8_t *d_crc_ok, const int8_t *const *d_history_in,
                          int8_t *const *d_history_out, uint8_t *const *d_out, void *stream);

}  // namespace dabapi
