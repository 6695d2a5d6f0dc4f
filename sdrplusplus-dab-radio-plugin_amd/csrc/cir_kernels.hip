// cir_kernels.hip -- channel impulse response (CIR) from the phase reference symbol (PRS), Mode I.
//
// Per frame, with X = FFT2048(nco * x[504 .. 2552)) relative to the first sample of the PRS prefix (the front end's window)
// and, over the 1536 carriers k = -768..768, k != 0, a Hann taper w(k) = 0.5 + 0.5 cos(pi k / 769) (sum S = 768):
//   h[n]       = sqrt(1536) / (2048 S) * sum_k w(k) X[k] conj R[k] exp(+2 pi i k n / 2048)
//   tap[n]     = |h[n]|^2                        (a path of gain g at integer delay d on unit sample power: tap[d] = |g|^2)
//   carrier[i] = 1536 / 2048^2 * |X[k]|^2        (i = 0..1535 for k = -768..-1, 1..768: 1.0 on a flat unit channel)
// one 256-thread workgroup per frame.  The inverse is a second forward transform: |IFFT(Y)| = |FFT(conj Y)| / 2048, with
// the 1/2048 folded into the scale of Y.  R is a fourth root of unity, so Y is swaps and negations of X times w.  A second
// pass adds each stream's records to its accumulator in frame order (no float atomics: the sums repeat bit for bit).
#include <type_traits>

#include "kernels.hpp"
#include "dab_tables.hpp"
#include "fft_common.hpp"
#include "iq_load.hpp"

namespace dabk {

using namespace dab;

namespace {

static_assert(sizeof(CirRecord) == 14352, "CirRecord mirrors dabgpu_cir_acc");
static_assert(CIR_CARRIERS == NB_CARRIERS && CIR_TAPS == NB_FFT && CIR_WIN_BEGIN == NB_CP, "Mode I");
constexpr int CIR_SUM_WORDS = CIR_TAPS + CIR_CARRIERS;         // the floats an accumulator adds, then the frame count
constexpr int CIR_ACC_WG = 256;
constexpr int CIR_ACC_BLOCKS = (CIR_SUM_WORDS + 1 + CIR_ACC_WG - 1) / CIR_ACC_WG;
// sqrt(1536) / (2048 * 768): the taper's sum and the inverse transform's 1/2048 folded into Y; and 1536 / 2048^2
constexpr float CIR_Y_SCALE = float(39.191835884530846 / (2048.0 * 768.0));
constexpr float CIR_CARRIER_SCALE = float(1536.0 / (2048.0 * 2048.0));

__device__ __forceinline__ float cir_power(float2 z) { return z.x * z.x + z.y * z.y; }

// conj(X * (-j)^q) = conj(X conj R) for R = j^q
__device__ __forceinline__ float2 cir_conj_rot(float2 v, int q) {
    switch (q & 3) {
    case 0: return make_float2(v.x, -v.y);
    case 1: return make_float2(v.y, v.x);
    case 2: return make_float2(-v.x, v.y);
    default: return make_float2(-v.y, -v.x);
    }
}

template <int FMT>
__global__ __launch_bounds__(WG) void cir_frame_kernel(const float2 *tw, CirArgs a) {
    __shared__ float2 t1[NB_FFT];
    __shared__ float2 x[NB_FFT];
    const int tid = threadIdx.x, frame = blockIdx.x;
    constexpr int FAM = iq_family(FMT);
    const IqSrc<FAM> iq0 = iq_src<FAM>(a.iq, FMT);
    CirRecord *rec = a.frame + frame;
    IqSrc<FAM> win;
    uint32_t dphi;
    if (a.acq) {
        // a slot of the acquisition / tracking calls: counted when locked and whole, its PRS prefix inside the capture
        const AcquiredFrame m = a.acq[frame];
        const int64_t p0 = m.start + a.timing_margin;
        if ((m.flags & 3) != 3 || p0 < 0) {
            float *w = reinterpret_cast<float *>(rec);
            for (int i = tid; i < int(sizeof(CirRecord) / 4); i += WG) w[i] = 0.0f;
            return;
        }
        win = iq0 + size_t(frame / a.frames_per_stream) * a.stride + p0 + CIR_WIN_BEGIN;
        dphi = uint32_t(__double2ll_rn(double(m.freq_offset) * 4294967296.0));
    } else {
        win = iq0 + size_t(frame) * a.stride + CIR_WIN_BEGIN;
        if (a.state) {
            // what the stream call would apply to this frame (ofdm_kernels.hip, frame_dphi)
            const StreamState st = a.state[frame / a.frames_per_stream];
            dphi = uint32_t(__double2ll_rn(double(st.fine_freq_offset + st.coarse_freq_offset) * 4294967296.0));
        } else {
            dphi = dphi_of(a.freq_offset, frame);
        }
    }
    {
        float2 v[8];
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const int n = tid + r * WG;
            float2 s = win[n];
            // the rotation's rounding spelled out (iq_load.hpp, mul_rn): every format forms the same values
            if (dphi != 0u) {
                const float2 w = nco(uint32_t(n), dphi);
                s = make_float2(fmaf(w.x, s.x, -mul_rn(w.y, s.y)), fmaf(w.y, s.x, mul_rn(w.x, s.y)));
            }
            v[r] = s;
        }
        block_fft2048(v, t1, x, tw, tw + TWC8_OFF, tw + TWC64_OFF, tid);
    }
    // bin b = tid + 256 r: the carrier's power to the record, conj(w X conj R) (0 off the carriers) into the second transform
    {
        float2 v[8];
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const int b = tid + r * WG;
            const int q = a.prs_qt[b];
            const float2 X = x[b];
            float2 y = make_float2(0.0f, 0.0f);
            if (q >= 0) {
                const int k = b < NB_FFT / 2 ? b : b - NB_FFT;
                rec->carrier[k < 0 ? k + NB_CARRIERS / 2 : k + NB_CARRIERS / 2 - 1] = CIR_CARRIER_SCALE * cir_power(X);
                const float w = CIR_Y_SCALE * fmaf(0.5f, cospif(float(k) * (1.0f / 769.0f)), 0.5f);
                const float2 c = cir_conj_rot(X, q);
                y = make_float2(w * c.x, w * c.y);
            }
            v[r] = y;
        }
        block_fft2048(v, t1, x, tw, tw + TWC8_OFF, tw + TWC64_OFF, tid);
    }
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int n = tid + r * WG;
        rec->tap[n] = cir_power(x[n]);
    }
    if (tid == 0) {
        rec->frames = 1;
        rec->reserved[0] = 0;
        rec->reserved[1] = 0;
        rec->reserved[2] = 0;
    }
}

// acc[s] += records of stream s, frame by frame; thread i of block (s, by) owns word by * 256 + i (2048 taps, 1536
// carriers, the frame count)
constexpr int CIR_ACC_BATCH = 16;
__global__ __launch_bounds__(CIR_ACC_WG) void cir_accumulate_kernel(const CirRecord *frame, int frames_per_stream, CirRecord *acc) {
    const int s = blockIdx.x, i = blockIdx.y * CIR_ACC_WG + threadIdx.x;
    if (i > CIR_SUM_WORDS) return;
    const float *src = reinterpret_cast<const float *>(frame + size_t(s) * frames_per_stream) + i;
    float *dst = reinterpret_cast<float *>(acc + s) + i;
    constexpr int W = int(sizeof(CirRecord) / 4);
    if (i == CIR_SUM_WORDS) {
        int n = __float_as_int(*dst);
        for (int f = 0; f < frames_per_stream; f++) n += __float_as_int(src[size_t(f) * W]);
        *dst = __int_as_float(n);
        return;
    }
    float sum = *dst;
    for (int f0 = 0; f0 < frames_per_stream; f0 += CIR_ACC_BATCH) {
        // the loads of a batch in flight together, the adds in frame order
        float v[CIR_ACC_BATCH];
#pragma unroll
        for (int u = 0; u < CIR_ACC_BATCH; u++) v[u] = f0 + u < frames_per_stream ? src[size_t(f0 + u) * W] : 0.0f;
#pragma unroll
        for (int u = 0; u < CIR_ACC_BATCH; u++)
            if (f0 + u < frames_per_stream) sum += v[u];
    }
    *dst = sum;
}

}  // namespace

hipError_t launch_cir(const float2 *twiddle, const CirArgs &a, hipStream_t s, int iq_format) {
    if (a.n_streams <= 0 || a.frames_per_stream <= 0) return hipSuccess;
    if (!a.iq || !a.frame || !a.acc || !a.prs_qt || !twiddle) return hipErrorInvalidValue;
    const unsigned n_frames = unsigned(a.n_streams) * unsigned(a.frames_per_stream);
    switch (iq_format) {
    case IQ_CF32: hipLaunchKernelGGL(cir_frame_kernel<IQ_CF32>, dim3(n_frames), dim3(WG), 0, s, twiddle, a); break;
    case IQ_CS16: hipLaunchKernelGGL(cir_frame_kernel<IQ_CS16>, dim3(n_frames), dim3(WG), 0, s, twiddle, a); break;
    case IQ_CS8: hipLaunchKernelGGL(cir_frame_kernel<IQ_CS8>, dim3(n_frames), dim3(WG), 0, s, twiddle, a); break;
    case IQ_CU8: hipLaunchKernelGGL(cir_frame_kernel<IQ_CU8>, dim3(n_frames), dim3(WG), 0, s, twiddle, a); break;
    default: return hipErrorInvalidValue;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cir_accumulate_kernel, dim3(unsigned(a.n_streams), CIR_ACC_BLOCKS), dim3(CIR_ACC_WG), 0, s, a.frame,
                       a.frames_per_stream, a.acc);
    return hipGetLastError();
}

}  // namespace dabk
