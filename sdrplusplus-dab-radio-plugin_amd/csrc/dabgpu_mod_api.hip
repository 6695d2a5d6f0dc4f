// dabgpu_mod_api.hip -- the modulator's entry points of the C ABI (include/dabgpu.h, "ETI(NI) to IQ"): the stream list read
// back from a frame, the configuration, and the device call that turns ETI(NI) frames into Mode-I IQ (mod_kernels.hip).
#include "dabgpu_ctx.hpp"

#include <cstddef>
#include <cstring>
#include <vector>

using namespace dabapi;

static_assert(sizeof(dabgpu_mod_status) == sizeof(dabk::ModStatus) && offsetof(dabgpu_mod_status, refused) == offsetof(dabk::ModStatus, refused),
              "ABI structs mirror the kernels'");
static_assert(DABGPU_MOD_BAD_INPUT == dabk::MOD_BAD_INPUT && DABGPU_MOD_MISALIGNED == dabk::MOD_MISALIGNED, "ABI constants mirror the kernels'");

namespace {

// d_mod_tables: PRBS bytes | bin -> data index | the TII null symbol
constexpr size_t TAB_PRBS = 0, TAB_N_OF_BIN = 512, TAB_NULL = TAB_N_OF_BIN + 2 * dab::NB_FFT;
constexpr size_t TAB_BYTES = TAB_NULL + sizeof(float2) * dab::NB_NULL_PERIOD;
static_assert(TAB_NULL % 16 == 0, "the null symbol is read in 16-byte words");

int ensure_tables(dabgpu_ctx *ctx) {
    if (ctx->d_mod_tables) return DABGPU_OK;
    std::vector<uint8_t> h(TAB_NULL, 0);
    const std::vector<uint8_t> prbs = dab::make_prbs_bytes(dabk::MOD_PRBS_BYTES);
    std::memcpy(h.data() + TAB_PRBS, prbs.data(), prbs.size());
    int16_t *n_of_bin = reinterpret_cast<int16_t *>(h.data() + TAB_N_OF_BIN);
    for (int b = 0; b < dab::NB_FFT; b++) n_of_bin[b] = -1;
    const std::vector<int32_t> mapper = dab::make_mapper();
    for (int n = 0; n < dab::NB_CARRIERS; n++) n_of_bin[dab::carrier_bin(mapper[size_t(n)])] = int16_t(n);
    void *d = nullptr;
    if (hipMalloc(&d, TAB_BYTES) != hipSuccess) return DABGPU_ERR_NOMEM;
    if (hipMemcpy(d, h.data(), h.size(), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(d);
        return DABGPU_ERR_HIP;
    }
    ctx->d_mod_tables = d;
    ctx->mod_tii_main = ctx->mod_tii_sub = -2;
    return DABGPU_OK;
}

// the runs of 128-bit blocks of a sub-channel's profile and its size in capacity units
bool subchannel_runs(const dabgpu_subchannel &sc, dabk::ModCode &code, int &size_cu) {
    std::memset(code.blocks, 0, sizeof code.blocks);
    std::memset(code.pi, 0, sizeof code.pi);
    if (sc.is_uep) {
        const int idx = sc.is_uep == 1 ? dab::uep_table_index(sc.bitrate_kbps, sc.protection_level) : -1;
        if (idx < 0) return false;
        const dab::UepProfileRow &r = dab::UEP_TABLE[idx];
        for (int i = 0; i < 4; i++) {
            code.blocks[i] = uint16_t(r.L[i]);
            code.pi[i] = uint8_t(r.PI[i]);
        }
        size_cu = r.size;
        return true;
    }
    int L1, L2, P1, P2;
    if (!dab::eep_runs(sc.eep_type, sc.protection_level, sc.bitrate_kbps, L1, L2, P1, P2, size_cu) || size_cu > 864) return false;
    code.blocks[0] = uint16_t(L1);
    code.blocks[1] = uint16_t(L2);
    code.pi[0] = uint8_t(P1);
    code.pi[1] = uint8_t(P2);
    return true;
}

}  // namespace

extern "C" {

int dabgpu_eti_streams_from_frame(const uint8_t *f, dabgpu_eti_stream *streams, int *n) {
    if (!f || !streams || !n) return DABGPU_ERR_ARG;
    const int nst = f[5] & 0x7f;
    if (nst > DABGPU_ETI_MAX_STREAMS) return DABGPU_ERR_ARG;
    for (int k = 0; k < nst; k++) {
        const uint8_t *stc = f + 8 + 4 * k;
        const int tpl = stc[2] >> 2, stl = ((stc[2] & 3) << 8) | stc[3];
        dabgpu_eti_stream st;
        std::memset(&st, 0, sizeof st);
        st.subchannel_id = stc[0] >> 2;
        st.sc.start_address = ((stc[0] & 3) << 8) | stc[1];
        if (stl == 0 || stl % 3) return DABGPU_ERR_ARG;        // 8 STL bytes = bit rate * 3, the bit rate a multiple of 8
        st.sc.bitrate_kbps = stl / 3 * 8;
        if ((tpl & 0x38) == 0x10) {                            // UEP: 0 1 0 level:3, the size from the table row
            st.sc.is_uep = 1;
            st.sc.protection_level = (tpl & 7) + 1;
        } else if ((tpl & 0x30) == 0x20 && ((tpl >> 2) & 3) <= 1) {   // EEP: 1 option:3 level:2, option A or B
            st.sc.eep_type = (tpl >> 2) & 3;
            st.sc.protection_level = (tpl & 3) + 1;
        } else {
            return DABGPU_ERR_ARG;
        }
        dabk::ModCode code;
        int size_cu = 0;
        if (!subchannel_runs(st.sc, code, size_cu) || st.sc.start_address + size_cu > 864) return DABGPU_ERR_ARG;
        st.sc.length = size_cu;
        streams[k] = st;
    }
    *n = nst;
    return DABGPU_OK;
}

void dabgpu_mod_default_cfg(dabgpu_mod_cfg *cfg) {
    if (!cfg) return;
    cfg->gain = 1.0f;
    cfg->tii_main = -1;
    cfg->tii_sub = -1;
    cfg->reserved = 0;
}

size_t dabgpu_mod_state_bytes(void) { return sizeof(dabk::ModState); }

int dabgpu_modulate_eti_dev(dabgpu_ctx *ctx, const dabgpu_eti_plan *plan, const dabgpu_eti_stream *streams,
                            const dabgpu_mod_cfg *cfg, int n_streams, int frames_per_stream, const uint8_t *d_eti,
                            const dabgpu_mod_state *d_state_in, dabgpu_mod_state *d_state_out, float *d_iq,
                            size_t frame_stride, dabgpu_mod_status *d_status, void *stream) {
    if (!ctx || !plan || !d_eti || !d_iq || !d_status || n_streams < 0 || frames_per_stream < 0) return DABGPU_ERR_ARG;
    const int nst = plan->nst;
    if (nst < 0 || nst > DABGPU_ETI_MAX_STREAMS || (nst > 0 && !streams)) return DABGPU_ERR_ARG;
    if (plan->header_bytes != 12 + 4 * nst || plan->fl < 0 || plan->fl > 0x7ff) return DABGPU_ERR_ARG;
    dabgpu_mod_cfg c;
    dabgpu_mod_default_cfg(&c);
    if (cfg) c = *cfg;
    const bool tii = c.tii_main >= 0 || c.tii_sub >= 0;
    if (tii ? (c.tii_main < 0 || c.tii_main >= dabk::TII_PATTERNS || c.tii_sub < 0 || c.tii_sub >= dabk::TII_COMBS)
            : (c.tii_main != -1 || c.tii_sub != -1))
        return DABGPU_ERR_ARG;
    if (!(c.gain == c.gain)) return DABGPU_ERR_ARG;
    if ((addr(d_eti) & 15u) || (addr(d_iq) & 15u) || (addr(d_status) & 7u) || (addr(d_state_in) & 15u) || (addr(d_state_out) & 15u))
        return DABGPU_ERR_ARG;
    if (frame_stride < size_t(dab::NB_FRAME_SAMPLES) || (frame_stride & 1u)) return DABGPU_ERR_ARG;
    if (d_state_in && static_cast<const void *>(d_state_in) == static_cast<const void *>(d_state_out)) return DABGPU_ERR_ARG;
    if (size_t(n_streams) * size_t(frames_per_stream) > size_t(0x7fffffff) / size_t(dabk::MOD_ITEMS)) return DABGPU_ERR_ARG;

    // the frame as the plan lays it out: the header every ETI frame is held to, and where each codeword's bytes are
    dabk::ModArgs a{};
    uint8_t hdr[16 + 4 * DABGPU_ETI_MAX_STREAMS] = {};
    hdr[5] = uint8_t(0x80 | nst);
    hdr[6] = uint8_t((1 << 3) | (plan->fl >> 8));
    hdr[7] = uint8_t(plan->fl & 0xff);
    a.code[0].in_offset = uint16_t(plan->header_bytes);
    a.code[0].in_bytes = uint16_t(dabk::ETI_FIC_BYTES);
    a.code[0].out_word = 0;
    a.code[0].blocks[0] = 21;
    a.code[0].blocks[1] = 3;
    a.code[0].pi[0] = 16;
    a.code[0].pi[1] = 15;
    char used[864] = {};
    int off = 0;
    for (int k = 0; k < nst; k++) {
        const int i = plan->order[k];
        if (i < 0 || i >= nst) return DABGPU_ERR_ARG;
        const dabgpu_eti_stream &st = streams[i];
        const dabgpu_subchannel &sc = st.sc;
        dabk::ModCode &code = a.code[1 + k];
        int size_cu = 0;
        if (!subchannel_runs(sc, code, size_cu)) return DABGPU_ERR_PROFILE;
        if (sc.length != size_cu || sc.start_address < 0 || sc.start_address + size_cu > 864) return DABGPU_ERR_PROFILE;
        if (st.subchannel_id < 0 || st.subchannel_id > 63) return DABGPU_ERR_ARG;
        for (int cu = sc.start_address; cu < sc.start_address + size_cu; cu++) {
            if (used[cu]) return DABGPU_ERR_ARG;
            used[cu] = 1;
        }
        const int bytes = sc.bitrate_kbps * 3, stl = bytes / 8;
        if (plan->offset[k] != off || plan->bytes[k] != bytes || stl > 1023) return DABGPU_ERR_ARG;
        const int tpl = sc.is_uep ? 0x10 | (sc.protection_level - 1) : 0x20 | (sc.eep_type << 2) | (sc.protection_level - 1);
        uint8_t *stc = hdr + 8 + 4 * k;
        stc[0] = uint8_t((st.subchannel_id << 2) | (sc.start_address >> 8));
        stc[1] = uint8_t(sc.start_address & 0xff);
        stc[2] = uint8_t((tpl << 2) | (stl >> 8));
        stc[3] = uint8_t(stl & 0xff);
        code.in_offset = uint16_t(plan->header_bytes + dabk::ETI_FIC_BYTES + off);
        code.in_bytes = uint16_t(bytes);
        code.out_word = uint16_t(dabk::MOD_FIC_WORDS + 2 * sc.start_address);
        off += bytes;
    }
    if (plan->data_bytes != off || plan->length != plan->header_bytes + dabk::ETI_FIC_BYTES + off + 8 ||
        plan->length > DABGPU_ETI_FRAME_BYTES || plan->fl * 4 + 16 != plan->length)
        return DABGPU_ERR_ARG;
    std::memcpy(a.header, hdr, size_t(8 + 4 * nst));
    if (n_streams == 0 || frames_per_stream == 0) return DABGPU_OK;
    DeviceGuard guard(ctx);

    int rc = ensure_tables(ctx);
    if (rc) return rc;
    const size_t n_frames = size_t(n_streams) * size_t(frames_per_stream);
    void *coded = nullptr, *cum = nullptr;
    if ((rc = stage(ctx, STAGE_MOD_CODED, n_frames * 4 * dabk::MOD_CODED_WORDS * sizeof(uint32_t), &coded))) return rc;
    if ((rc = stage(ctx, STAGE_MOD_CUM, n_frames * dab::NB_DATA_SYMBOLS * dabk::MOD_SYM_WORDS * sizeof(uint32_t), &cum))) return rc;

    char *tab = static_cast<char *>(ctx->d_mod_tables);
    dabk::ModTables t{};
    t.prbs = reinterpret_cast<const uint8_t *>(tab + TAB_PRBS);
    t.n_of_bin = reinterpret_cast<const int16_t *>(tab + TAB_N_OF_BIN);
    t.prs_qt = ctx->d_prs_qt;
    t.twiddle = ctx->d_twiddle;
    t.null_symbol = tii ? reinterpret_cast<const float2 *>(tab + TAB_NULL) : nullptr;

    a.n_codes = nst + 1;
    a.nst = nst;
    a.eti = d_eti;
    a.state_in = reinterpret_cast<const dabk::ModState *>(d_state_in);
    a.state_out = reinterpret_cast<dabk::ModState *>(d_state_out);
    a.coded = static_cast<uint32_t *>(coded);
    a.cum = static_cast<uint32_t *>(cum);
    a.iq = reinterpret_cast<float2 *>(d_iq);
    a.frame_stride = frame_stride;
    a.status = reinterpret_cast<dabk::ModStatus *>(d_status);
    a.gain = c.gain;
    a.n_streams = n_streams;
    a.frames_per_stream = frames_per_stream;

    hipStream_t s = pick_stream(ctx, stream);
    if (tii && (ctx->mod_tii_main != c.tii_main || ctx->mod_tii_sub != c.tii_sub)) {
        ctx->mod_tii_main = ctx->mod_tii_sub = -2;
        HIP_TRY(dabk::launch_mod_tii(ctx->d_prs_qt, c.tii_main, c.tii_sub, reinterpret_cast<float2 *>(tab + TAB_NULL), s));
        ctx->mod_tii_main = c.tii_main;
        ctx->mod_tii_sub = c.tii_sub;
    }
    {
        ScopedTimer timer(ctx, TIMER_MOD_ENCODE, s);
        HIP_TRY(dabk::launch_mod_encode(t, a, s));
    }
    ScopedTimer timer(ctx, TIMER_MOD_SYMBOLS, s);
    HIP_TRY(dabk::launch_mod_symbols(t, a, s));
    return DABGPU_OK;
}

}  // extern "C"
