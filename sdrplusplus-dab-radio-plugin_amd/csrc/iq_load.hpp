// iq_load.hpp -- complex samples in the caller's format (dabgpu_set_iq_format), read as float2 right after the load.
//
// The kernels work on exactly these values: float(i), float(q) for cs16 and cs8; float(u) - 127.5f for cu8, formed as the
// signed byte u ^ 0x80 (= u - 128) plus 0.5 -- exact, so cs8 and cu8 share one loader (the flip and the offset are constants
// in every instantiation: the kernels take the format as a template argument).
// No scaling: every later step is scale-free (relative quantiser, relative thresholds), so a buffer of integers gives the
// bits a cf32 buffer holding the same values gives.
//
// IqSrc<FAM> is what a kernel indexes in complex samples: for cf32 the plain `const float2 *` the kernels have always
// used (their code does not change), for the integer families a small pointer object with the same arithmetic.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "mem_stream.hpp"

namespace dabk {

// == DABGPU_IQ_*
constexpr int IQ_CF32 = 0, IQ_CS16 = 1, IQ_CS8 = 2, IQ_CU8 = 3;
// loader families (cs8 and cu8 differ only in the flip and the offset)
constexpr int IQF_F32 = 0, IQF_I16 = 1, IQF_I8 = 2;

__host__ __device__ constexpr int iq_family(int fmt) { return fmt == IQ_CS16 ? IQF_I16 : (fmt == IQ_CS8 || fmt == IQ_CU8) ? IQF_I8 : IQF_F32; }
__host__ __device__ constexpr size_t iq_sample_bytes(int fmt) { return fmt == IQ_CS16 ? 4 : (fmt == IQ_CS8 || fmt == IQ_CU8) ? 2 : 8; }
inline bool iq_format_valid(int fmt) { return fmt >= IQ_CF32 && fmt <= IQ_CU8; }

namespace detail {
__device__ __forceinline__ float s16lo(uint32_t v) { return float(int32_t(v << 16) >> 16); }
__device__ __forceinline__ float s16hi(uint32_t v) { return float(int32_t(v) >> 16); }
template <int B> __device__ __forceinline__ float s8(uint32_t v, float off) { return float(int32_t(v << (24 - 8 * B)) >> 24) + off; }
__device__ __forceinline__ uint32_t ld_nt_u32(const uint32_t *p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ uint32_t ld_nt_u16(const uint16_t *p) { return __builtin_nontemporal_load(p); }
}  // namespace detail

// interleaved int16 I, Q (4 bytes per sample)
struct IqPtr16 {
    const uint32_t *p;
    __device__ IqPtr16 operator+(int64_t n) const { return IqPtr16{p + n}; }
    __device__ IqPtr16 operator-(int64_t n) const { return IqPtr16{p - n}; }
    __device__ float2 cvt(uint32_t v) const { return make_float2(detail::s16lo(v), detail::s16hi(v)); }
    __device__ float2 operator[](int64_t i) const { return cvt(p[i]); }
    __device__ float2 ld(int64_t i) const { return cvt(detail::ld_nt_u32(p + i)); }           // streaming, one sample
    // samples i, i+1 as one 8-byte load: the pair must be 8-byte aligned (pair_aligned of the frame, even i)
    __device__ void ld2(int64_t i, float2 &a, float2 &b) const {
        const uint2 v = ld_stream(reinterpret_cast<const uint2 *>(p + i));
        a = cvt(v.x);
        b = cvt(v.y);
    }
    __device__ bool pair_aligned() const { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }
};

// interleaved 8-bit I, Q (2 bytes per sample): value = int8(byte ^ flip) + off (cs8: 0, 0; cu8: 0x80, 0.5)
struct IqPtr8 {
    const uint16_t *p;
    uint32_t flip;             // 0 or 0x80808080
    float off;                 // 0 or 0.5
    __device__ IqPtr8 operator+(int64_t n) const { return IqPtr8{p + n, flip, off}; }
    __device__ IqPtr8 operator-(int64_t n) const { return IqPtr8{p - n, flip, off}; }
    __device__ float2 cvt(uint32_t v) const {
        v ^= flip;
        return make_float2(detail::s8<0>(v, off), detail::s8<1>(v, off));
    }
    __device__ float2 operator[](int64_t i) const { return cvt(uint32_t(p[i])); }
    __device__ float2 ld(int64_t i) const { return cvt(uint32_t(detail::ld_nt_u16(p + i))); }
    // samples i, i+1 as one 4-byte load (4-byte aligned pair)
    __device__ void ld2(int64_t i, float2 &a, float2 &b) const {
        const uint32_t v = detail::ld_nt_u32(reinterpret_cast<const uint32_t *>(p + i)) ^ flip;
        a = make_float2(detail::s8<0>(v, off), detail::s8<1>(v, off));
        b = make_float2(detail::s8<2>(v, off), detail::s8<3>(v, off));
    }
    __device__ bool pair_aligned() const { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
};

// Exact rounding for the few sums of products the integer instantiations form straight from their samples.  The compiler
// contracts `a * b + c * d` into one fma, and WHICH product it fuses depends on what produced the operands (a load in the
// cf32 instantiations, a conversion here): the integer paths spell out, with these, the rounding the cf32 instantiations
// are compiled to, so that they stay bit-exact with them (tests/test_iq_formats.py).
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

template <int FAM>
using IqSrc = typename std::conditional<FAM == IQF_F32, const float2 *,
                                        typename std::conditional<FAM == IQF_I16, IqPtr16, IqPtr8>::type>::type;

// the kernels' float2 * argument, read in format `fmt` (of family FAM)
template <int FAM>
__device__ __forceinline__ IqSrc<FAM> iq_src(const float2 *p, int fmt) {
    if constexpr (FAM == IQF_F32) {
        return p;
    } else if constexpr (FAM == IQF_I16) {
        return IqPtr16{reinterpret_cast<const uint32_t *>(p)};
    } else {
        const bool u8 = fmt == IQ_CU8;
        return IqPtr8{reinterpret_cast<const uint16_t *>(p), u8 ? 0x80808080u : 0u, u8 ? 0.5f : 0.0f};
    }
}

}  // namespace dabk
