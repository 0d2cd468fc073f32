// Device-side helpers that more than one kernel file needs (included by the .hip files only): the register vector types, element and 16-byte
// vector access to fp32-or-fp16 buffers, and a few arithmetic idioms.  A helper with a single user stays in that user's file.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ie {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef long i64x2 __attribute__((ext_vector_type(2)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// Word 3 of a buffer resource, the flags argument of __builtin_amdgcn_make_buffer_rsrc: DATA_FORMAT (bits 18:15) = 4, a 32-bit element, and
// every other field 0: raw addressing (no swizzle, no index stride, no typed-format conversion), offsets range-checked against num_records bytes
constexpr int kBufferRsrcFlags = 0x00020000;

// one element of a buffer that holds floats (f16 == 0) or halfs behind the same typed pointer (TensorArg::p)
__device__ __forceinline__ float ld_any(const float* p, int f16, int64_t i) {
    return f16 ? float(reinterpret_cast<const _Float16*>(p)[i]) : p[i];
}
__device__ __forceinline__ void st_any(float* p, int f16, int64_t i, float v) {
    if (f16) reinterpret_cast<_Float16*>(p)[i] = _Float16(v);
    else p[i] = v;
}

// 16 bytes of consecutive elements (4 floats / 8 halfs, 16-byte aligned) <-> floats
template <typename T>
__device__ __forceinline__ void load16(const T* p, float* d);
template <>
__device__ __forceinline__ void load16<float>(const float* p, float* d) {
    const float4 x = *reinterpret_cast<const float4*>(p);
    d[0] = x.x; d[1] = x.y; d[2] = x.z; d[3] = x.w;
}
template <>
__device__ __forceinline__ void load16<_Float16>(const _Float16* p, float* d) {
    const h8 x = *reinterpret_cast<const h8*>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = float(x[i]);
}
template <typename T>
__device__ __forceinline__ void store16(T* p, const float* v);
template <>
__device__ __forceinline__ void store16<float>(float* p, const float* v) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
template <>
__device__ __forceinline__ void store16<_Float16>(_Float16* p, const float* v) {
    h8 o;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = _Float16(v[i]);
    *reinterpret_cast<h8*>(p) = o;
}

// sum over the LANES lanes of a group (a power of two <= 64, groups aligned inside the wave); every lane of the wave takes part
template <int LANES>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int m = LANES / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, LANES);
    return v;
}

// 2^x as the bare v_exp_f32 (exp2f wraps the instruction in a rescaling for results in the denormal range)
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// Wave-uniform n / d on the scalar unit: mg = floor(2^32 / d) (2^32 - 1 for d == 1) undershoots the quotient by at most one.
__device__ __forceinline__ unsigned udiv_uniform(unsigned n, unsigned d, unsigned mg) {
    unsigned q = __umulhi(n, mg);
    if (n - q * d >= d) ++q;
    return q;
}

constexpr float kE4m3Max = 448.0f;

// four floats -> four e4m3 bytes (round to nearest even; the inputs are clamped to the finite range first, so nothing overflows
// into the NaN encoding)
__device__ __forceinline__ unsigned pack4_e4m3(float a, float b, float c, float d) {
    a = __builtin_fminf(__builtin_fmaxf(a, -kE4m3Max), kE4m3Max);
    b = __builtin_fminf(__builtin_fmaxf(b, -kE4m3Max), kE4m3Max);
    c = __builtin_fminf(__builtin_fmaxf(c, -kE4m3Max), kE4m3Max);
    d = __builtin_fminf(__builtin_fmaxf(d, -kE4m3Max), kE4m3Max);
    int p = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    p = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, p, true);
    return unsigned(p);
}
__device__ __forceinline__ void unpack4_e4m3(unsigned p, float* v) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(int(p), false), hi = __builtin_amdgcn_cvt_pk_f32_fp8(int(p), true);
    v[0] = lo[0]; v[1] = lo[1]; v[2] = hi[0]; v[3] = hi[1];
}

}  // namespace ie
