// What the KV-cache kernel files share (included by kernels_decode.hip, kernels_decode_h.hip and kernels_extend_w.hip only): the block size, the
// addressing of a step's qkv rows and rope tables, the clamped lengths of a resident cache, the key bias, and the launchers of the half-cache forms
// and of the wide-head extend tile that kernels_decode.hip's dispatch hands over to.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"

namespace ie {

constexpr int kDecodeBlock = 256;

// the table row of token l of image n: the token's own id pos[n pos_sn + l] (a negative position counts from the end), l without pos, clamped into the table
__device__ __forceinline__ int64_t rope_row(const DecodeArgs& a, int64_t n, int l) {
    int64_t r = l;
    if (a.pos) {
        const int64_t p = a.pos[n * a.pos_sn + l];
        r = p < 0 ? p + a.rope_rows : p;
    }
    return r < 0 ? 0 : (r >= a.rope_rows ? a.rope_rows - 1 : r);
}

// element e of the head whose row starts at element `rb` of the qkv buffer, rotated at table row r (cos null: as it is)
template <typename T>
__device__ __forceinline__ float rotated(const DecodeArgs& a, int64_t rb, int64_t r, int e, bool rope) {
    const T* p = reinterpret_cast<const T*>(a.in.p);
    const float x = float(p[rb + int64_t(e) * a.in.sc]);
    if (!rope) return x;
    const int hh = a.head_dim / 2, pe = e < hh ? e + hh : e - hh;
    const float xp = float(p[rb + int64_t(pe) * a.in.sc]);
    const int64_t t = r * a.head_dim + e;
    return fmaf(x, a.rope_cos[t], (e < hh ? -xp : xp) * a.rope_sin[t]);
}

// the first element of k (which = 1) or v (which = 2) of K / V head kvh of token (n, l) in the qkv buffer; which = 0: of query head kvh
__device__ __forceinline__ int64_t qkv_base(const DecodeArgs& a, int64_t n, int l, int which, int head) {
    const int64_t D = int64_t(a.heads) * a.head_dim, Dkv = int64_t(a.kv_heads) * a.head_dim;
    const int64_t col = (which == 0 ? 0 : (which == 1 ? D : D + Dkv)) + int64_t(head) * a.head_dim;
    return n * a.in.sn + int64_t(l) * a.in.sw + col * a.in.sc;
}

// In place: image n's valid rows and the tokens this step appends, clamped so that whatever the two arrays hold no kernel leaves the cache:
// 0 <= len <= cache_rows, 0 <= c <= min(new_len, cache_rows - len)
struct Resident { int len, c; };
__device__ __forceinline__ Resident resident(const DecodeArgs& a, int64_t n) {
    const int rows = int(a.cache_rows);
    int len = a.lens[n], c = a.news[n];
    len = len < 0 ? 0 : (len > rows ? rows : len);
    c = c > a.new_len ? a.new_len : c;
    c = c > rows - len ? rows - len : c;
    return {len, c < 0 ? 0 : c};
}

// the bias of key j of image n, and the image's largest bias where it is small enough to be taken out of every score exactly (0 otherwise)
__device__ __forceinline__ float key_bias(const DecodeArgs& a, int64_t n, int j) { return (1.f - float(a.mask[n * a.mask_sn + j])) * a.mask_value; }

// kernels_decode_h.hip, for a step that kernels_decode.hip has found eligible (DecodeArgs::cache_f16): the append of the step's new rows to a half
// cache, and tile 4 of a decode step over one (the combine launch behind it where splits > 1 stays the caller's)
hipError_t LaunchKvAppendRowsHalf(const DecodeArgs& a, hipStream_t stream);
hipError_t LaunchDecodeHalf(const DecodeArgs& a, hipStream_t stream);
// kernels_extend_w.hip, for an extend step at head_dim 128 that kernels_decode.hip has found eligible: tile 6 over `present` or the resident cache, fp32
// or half (the append in front of it and the combine launch behind it stay the caller's), and its registration for more than 64 KiB of LDS
hipError_t LaunchExtendWide(const DecodeArgs& a, hipStream_t stream);
hipError_t InitKernelsExtendWide();

}  // namespace ie
