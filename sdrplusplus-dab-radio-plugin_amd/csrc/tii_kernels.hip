// tii_kernels.hip -- transmitter identification (TII, EN 300 401 section 14.8) from the null symbol.
//
// Each transmitter of a single-frequency network puts a comb of carrier pairs into the null symbol: comb c (its
// sub-identifier) and four of eight positions b (pattern p, its main identifier; kernels.hpp has the tables).  Per frame:
//   X    = FFT2048(nco * x[-2352 .. -304))    relative to the first sample of the PRS prefix: the window sits in the middle
//                                              of the 2656-sample null symbol, 304 samples clear of the previous symbol's
//                                              echoes and of the PRS, so a later transmitter stays clean to ~300 samples
//   cell[c][b] = sum of |X_k|^2 over the 8 carriers of (c, b)
//   floor      = mean |X_k|^2 over the noise bins 776 <= |k| <= 927
// one 256-thread workgroup per frame (the LDS Stockham of fft_common.hpp), written as a per-frame record.  A second pass
// adds each stream's records to its accumulator in frame order, one workgroup per stream: no float atomics, the sums repeat
// bit for bit.  The whole-carrier offset moves the comb, so the frame's frequency correction is applied before the FFT.
#include <type_traits>

#include "kernels.hpp"
#include "dab_tables.hpp"
#include "fft_common.hpp"
#include "iq_load.hpp"

namespace dabk {

using namespace dab;

namespace {

static_assert(sizeof(TiiRecord) == 784, "TiiRecord mirrors dabgpu_tii_acc");
constexpr int TII_WORDS = TII_CELLS + 2;     // the floats and the frame count an accumulator adds (not `reserved`)

__device__ __forceinline__ float power(float2 z) { return z.x * z.x + z.y * z.y; }

template <int FMT>
__global__ __launch_bounds__(WG) void tii_frame_kernel(const float2 *tw, TiiArgs a) {
    __shared__ float2 t1[NB_FFT];
    __shared__ float2 x[NB_FFT];
    __shared__ float red[WG / 64];
    const int tid = threadIdx.x, frame = blockIdx.x;
    constexpr int FAM = iq_family(FMT);
    const IqSrc<FAM> iq0 = iq_src<FAM>(a.iq, FMT);
    TiiRecord *rec = a.frame + frame;
    IqSrc<FAM> win;
    uint32_t dphi;
    if (a.acq) {
        // a slot of the acquisition / tracking calls: counted when locked, whole, and its window inside the capture
        const AcquiredFrame m = a.acq[frame];
        const int64_t w0 = m.start + a.timing_margin - TII_WIN_BEGIN;
        if ((m.flags & 3) != 3 || w0 < 0) {
            float *w = reinterpret_cast<float *>(rec);
            for (int i = tid; i < int(sizeof(TiiRecord) / 4); i += WG) w[i] = 0.0f;
            return;
        }
        win = iq0 + size_t(frame / a.frames_per_stream) * a.stride + w0;
        dphi = uint32_t(__double2ll_rn(double(m.freq_offset) * 4294967296.0));
    } else {
        win = iq0 + size_t(frame) * a.stride - TII_WIN_BEGIN;
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
    // cells: thread c*8 + b sums its 8 carriers, bases in order, k before k + 1
    if (tid < TII_CELLS) {
        const int c = tid >> 3, b = tid & 7;
        float s = 0.0f;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int k = tii_base(q) + 2 * c + 48 * b;
            s += power(x[k & (NB_FFT - 1)]);
            s += power(x[(k + 1) & (NB_FFT - 1)]);
        }
        rec->cell[tid] = s;
    }
    // floor: bins +k and -k per thread, a fixed reduction tree (DPP inside a wave, the four waves in order)
    constexpr int N_SIDE = TII_FLOOR_HI - TII_FLOOR_LO + 1;
    static_assert(N_SIDE <= WG, "one noise bin pair per thread");
    float p = 0.0f;
    if (tid < N_SIDE) p = power(x[TII_FLOOR_LO + tid]) + power(x[NB_FFT - TII_FLOOR_LO - tid]);
    p = wave_sum(p, tid & 63);
    if ((tid & 63) == 0) red[tid >> 6] = p;
    __syncthreads();
    if (tid == 0) {
        rec->floor = (((red[0] + red[1]) + red[2]) + red[3]) / float(2 * N_SIDE);
        rec->frames = 1;
        rec->reserved[0] = 0;
        rec->reserved[1] = 0;
    }
}

// acc[s] += records of stream s, frame by frame; thread i owns word i (192 cells, the floor, the frame count)
constexpr int ACC_BATCH = 16;
__global__ __launch_bounds__(256) void tii_accumulate_kernel(const TiiRecord *frame, int frames_per_stream, TiiRecord *acc) {
    const int s = blockIdx.x, i = threadIdx.x;
    if (i >= TII_WORDS) return;
    const float *src = reinterpret_cast<const float *>(frame + size_t(s) * frames_per_stream) + i;
    float *dst = reinterpret_cast<float *>(acc + s) + i;
    constexpr int W = int(sizeof(TiiRecord) / 4);
    if (i == TII_CELLS + 1) {
        int n = __float_as_int(*dst);
        for (int f = 0; f < frames_per_stream; f++) n += __float_as_int(src[size_t(f) * W]);
        *dst = __int_as_float(n);
        return;
    }
    float sum = *dst;
    for (int f0 = 0; f0 < frames_per_stream; f0 += ACC_BATCH) {
        // the loads of a batch in flight together, the adds in frame order
        float v[ACC_BATCH];
#pragma unroll
        for (int u = 0; u < ACC_BATCH; u++) v[u] = f0 + u < frames_per_stream ? src[size_t(f0 + u) * W] : 0.0f;
#pragma unroll
        for (int u = 0; u < ACC_BATCH; u++)
            if (f0 + u < frames_per_stream) sum += v[u];
    }
    *dst = sum;
}

}  // namespace

hipError_t launch_tii(const float2 *twiddle, const TiiArgs &a, hipStream_t s, int iq_format) {
    if (a.n_streams <= 0 || a.frames_per_stream <= 0) return hipSuccess;
    if (!a.iq || !a.frame || !a.acc || !twiddle) return hipErrorInvalidValue;
    const unsigned n_frames = unsigned(a.n_streams) * unsigned(a.frames_per_stream);
    switch (iq_format) {
    case IQ_CF32: hipLaunchKernelGGL(tii_frame_kernel<IQ_CF32>, dim3(n_frames), dim3(WG), 0, s, twiddle, a); break;
    case IQ_CS16: hipLaunchKernelGGL(tii_frame_kernel<IQ_CS16>, dim3(n_frames), dim3(WG), 0, s, twiddle, a); break;
    case IQ_CS8: hipLaunchKernelGGL(tii_frame_kernel<IQ_CS8>, dim3(n_frames), dim3(WG), 0, s, twiddle, a); break;
    case IQ_CU8: hipLaunchKernelGGL(tii_frame_kernel<IQ_CU8>, dim3(n_frames), dim3(WG), 0, s, twiddle, a); break;
    default: return hipErrorInvalidValue;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tii_accumulate_kernel, dim3(unsigned(a.n_streams)), dim3(256), 0, s, a.frame, a.frames_per_stream, a.acc);
    return hipGetLastError();
}

}  // namespace dabk
