// KV cache for generation with Llama-class graphs on gfx950: the append of a step's new K / V rows to the cache and the one-token decode attention.
//
// The cache tensors are fp32 in every precision and dense [N][Hkv][rows][hd] (kernels.h DecodeArgs): `past` with P rows comes in, `present` with
// P + L rows goes out.  A decode step (L = 1) is a bandwidth problem: the arithmetic is 2 FMAs per cached element and query head, so the kernels
// are arranged around reading the cache once at the HBM rate.
//
//   kv_append_kernel<T, V>               one lane per V consecutive floats of `present` (V = 4: 16-byte vectors; V = 1: a head dim that is no
//                                        multiple of 4).  Rows < P: the past row, bit for bit.  Row P + l: k of token l after the rotary embedding
//                                        (x cos + rotate_half(x) sin at the table row pos[n] + l, fp32 arithmetic as AttnArgs describes it) resp. v of
//                                        token l, converted to fp32.  Without a past (a prefill with a cache) it writes all L rows.
//   attention_decode_generic_kernel<T>   tile 0: one wave per (image, query head) over `present`, which a kv_append launch wrote.  Lane l owns the head
//                                        elements l, l + 64, ...; per key one wave reduction gives the score, the online softmax runs in every lane
//                                        alike.  Any hd <= 512, any P, with or without a mask: the route for whatever tile 4 declines, and the cross-check.
//   attention_decode_kernel<T, HD, G>    tile 4: a workgroup = (image, K / V head, key split s of S), four waves.  A key row is HD / 4 lanes of 16 bytes, so a
//                                        wave takes 256 / HD keys and the workgroup DecodeKeyTile(HD) keys per iteration, contiguous in the cache.  The lane
//                                        that loads a K / V vector stores it into `present` (the Concat costs no pass of its own), multiplies it with the
//                                        same slice of the g <= G query rows of its group, which it holds in registers, and a reduction over the HD / 4
//                                        lanes of the key gives the g scores: every cached element is loaded by one lane of one workgroup, once, for all
//                                        g query heads.  Every key slot keeps an online softmax (m, l, o) per query head in registers; the slots of the
//                                        workgroup are merged through LDS at the end.  The last split rotates and appends the new row and attends to it.
//                                        S == 1: the workgroup writes the token row.  S > 1: it writes (m, l, o[hd]) per query head into the workspace and
//   attention_decode_combine_kernel<T>   adds the S records of a query head in split order.  No atomics: the result is bit-identical from run to run.
//
// Scores, statistics and accumulation are fp32.  The key-mask bias (1 - float(mask[n, j])) * c is added to the scaled score in fp32 and the sum clamped
// at -FLT_MAX, as the MASK forms of kernels_attn.hip keep it finite: the running maximum starts at -FLT_MAX too, so a split (or a whole row) whose
// keys are all masked has m = -FLT_MAX, l = its key count and o = the plain sum of its V rows; next to a split with a real score its weight
// exp(-FLT_MAX - M) is exactly 0, and a fully masked row comes out as the uniform average of V, which is what the graph's own sum gives.
// The VALU dot-product form was chosen over MFMA 16x16x4 on padded query rows because g <= 8 rows would leave half or more of every MFMA idle.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_util.h"
#include "kernels.h"
#include "launch_util.h"

namespace ie {
namespace {

constexpr int kDecodeBlock = 256;
constexpr float kFltMax = 3.402823466e+38f;
constexpr float kMaskShiftMax = 16777216.f;

// the table row of token l of image n: pos[n] + l (a negative position counts from the end), clamped into the table
__device__ __forceinline__ int64_t rope_row(const DecodeArgs& a, int64_t n, int l) {
    int64_t r = l;
    if (a.pos) {
        const int64_t p = a.pos[n];
        r += p < 0 ? p + a.rope_rows : p;
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

template <typename T, int V>
__global__ __launch_bounds__(kDecodeBlock) void kv_append_kernel(const DecodeArgs a, const int64_t total) {
    const int64_t i = int64_t(blockIdx.x) * kDecodeBlock + threadIdx.x;      // vector i of present: ((n Hkv + kvh) rows + row) hd / V + ev
    if (i >= total) return;
    const int hd = a.head_dim, P = a.past_len, rows = P + a.new_len, vpr = hd / V;
    const int ev = int(i % vpr);
    const int row = int((i / vpr) % rows);
    const int64_t nh = i / (int64_t(vpr) * rows);      // n Hkv + kvh
    const int kvh = int(nh % a.kv_heads);
    const int64_t n = nh / a.kv_heads;
    const int64_t o = i * V;
    if (row < P) {
        const int64_t s = (nh * P + row) * hd + int64_t(ev) * V;
        if constexpr (V == 4) {
            *reinterpret_cast<float4*>(a.present_k + o) = *reinterpret_cast<const float4*>(a.past_k + s);
            *reinterpret_cast<float4*>(a.present_v + o) = *reinterpret_cast<const float4*>(a.past_v + s);
        } else {
            a.present_k[o] = a.past_k[s];
            a.present_v[o] = a.past_v[s];
        }
        return;
    }
    const int l = row - P;
    const bool rope = a.rope_cos != nullptr;
    const int64_t r = rope ? rope_row(a, n, l) : 0;
    const int64_t kb = qkv_base(a, n, l, 1, kvh), vb = qkv_base(a, n, l, 2, kvh);
    float k[V], v[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        k[j] = rotated<T>(a, kb, r, ev * V + j, rope);
        v[j] = float(reinterpret_cast<const T*>(a.in.p)[vb + int64_t(ev * V + j) * a.in.sc]);
    }
    if constexpr (V == 4) {
        *reinterpret_cast<float4*>(a.present_k + o) = make_float4(k[0], k[1], k[2], k[3]);
        *reinterpret_cast<float4*>(a.present_v + o) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        a.present_k[o] = k[0];
        a.present_v[o] = v[0];
    }
}

// the bias of key j of image n, and the image's largest bias where it is small enough to be taken out of every score exactly (0 otherwise)
__device__ __forceinline__ float key_bias(const DecodeArgs& a, int64_t n, int j) { return (1.f - float(a.mask[n * a.mask_sn + j])) * a.mask_value; }

// rows = N * heads, one wave each
template <typename T>
__global__ __launch_bounds__(kDecodeBlock) void attention_decode_generic_kernel(const DecodeArgs a, const int64_t rows) {
    constexpr int kChunks = kDecodeMaxHeadDim / 64;
    const int lane = int(threadIdx.x) % 64;
    const int64_t row = int64_t(blockIdx.x) * (kDecodeBlock / 64) + threadIdx.x / 64;
    if (row >= rows) return;                       // wave-uniform
    const int hd = a.head_dim, Lk = a.past_len + 1;
    const int h = int(row % a.heads);
    const int64_t n = row / a.heads;
    const int kvh = h / (a.heads / a.kv_heads);
    const float* K = a.present_k + (n * a.kv_heads + kvh) * int64_t(Lk) * hd;
    const float* Vp = a.present_v + (n * a.kv_heads + kvh) * int64_t(Lk) * hd;
    const bool rope = a.rope_cos != nullptr;
    const int64_t r = rope ? rope_row(a, n, 0) : 0;
    const int64_t qb = qkv_base(a, n, 0, 0, h);
    float q[kChunks], acc[kChunks];
#pragma unroll
    for (int c = 0; c < kChunks; ++c) {
        const int e = c * 64 + lane;
        q[c] = e < hd ? rotated<T>(a, qb, r, e, rope) * a.scale : 0.f;
        acc[c] = 0.f;
    }
    float shift = 0.f;
    if (a.mask) {
        float bm = -kFltMax;
        for (int j = lane; j < Lk; j += 64) bm = fmaxf(bm, key_bias(a, n, j));
#pragma unroll
        for (int x = 32; x >= 1; x >>= 1) bm = fmaxf(bm, __shfl_xor(bm, x, 64));
        shift = fabsf(bm) <= kMaskShiftMax ? bm : 0.f;
    }
    float m = -kFltMax, l = 0.f;
    for (int j = 0; j < Lk; ++j) {
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < kChunks; ++c) {
            const int e = c * 64 + lane;
            if (e < hd) s = fmaf(q[c], K[int64_t(j) * hd + e], s);
        }
#pragma unroll
        for (int x = 32; x >= 1; x >>= 1) s += __shfl_xor(s, x, 64);
        if (a.mask) s = fmaxf(s + (key_bias(a, n, j) - shift), -kFltMax);
        const float mn = fmaxf(m, s), al = __expf(m - mn), p = __expf(s - mn);
        l = l * al + p;
#pragma unroll
        for (int c = 0; c < kChunks; ++c) {
            const int e = c * 64 + lane;
            if (e < hd) acc[c] = fmaf(p, Vp[int64_t(j) * hd + e], acc[c] * al);
        }
        m = mn;
    }
    T* out = reinterpret_cast<T*>(a.out.p);
    const int64_t ob = n * a.out.sn + int64_t(h) * hd * a.out.sc;
#pragma unroll
    for (int c = 0; c < kChunks; ++c) {
        const int e = c * 64 + lane;
        if (e < hd) out[ob + int64_t(e) * a.out.sc] = T(acc[c] / l);
    }
}

__device__ __forceinline__ float dot4(const float4 a, const float4 b) { return fmaf(a.x, b.x, fmaf(a.y, b.y, fmaf(a.z, b.z, a.w * b.w))); }

// grid = (splits, Hkv, N)
template <typename T, int HD, int G>
__global__ __launch_bounds__(kDecodeBlock) void attention_decode_kernel(const DecodeArgs a) {
    constexpr int LPK = HD / 4;                    // lanes of one key row
    constexpr int KPW = 64 / LPK;                  // key slots of a wave
    constexpr int KT = 4 * KPW;                    // keys of the workgroup per iteration (kernels.h DecodeKeyTile)
    constexpr int NS = 4 * KPW;                    // key slots of the workgroup, each with its own online softmax
    static_assert(KT == DecodeKeyTile(HD), "kernels.h DecodeKeyTile");
    __shared__ float s_ml[NS][G][2];
    __shared__ float s_o[NS][G][HD];
    const int S = int(gridDim.x), sp = int(blockIdx.x), kvh = int(blockIdx.y);
    const int64_t n = blockIdx.z;
    const int lane = int(threadIdx.x) % 64, wave = int(threadIdx.x) / 64;
    const int sub = lane / LPK, el = lane % LPK, slot = wave * KPW + sub;
    const int g = a.heads / a.kv_heads, P = a.past_len, Lk = P + 1;
    const int tiles = (Lk + KT - 1) / KT, per = (tiles + S - 1) / S;
    const int k0 = sp * per * KT, k1 = min(Lk, (sp + 1) * per * KT);      // this split's keys (none where per * S overshoots)
    const bool rope = a.rope_cos != nullptr;
    const int64_t r = rope ? rope_row(a, n, 0) : 0;
    // the lane's slice of the g query rows, rotated and scaled
    float4 q[G];
#pragma unroll
    for (int gi = 0; gi < G; ++gi) {
        q[gi] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (gi < g) {
            const int64_t qb = qkv_base(a, n, 0, 0, kvh * g + gi);
            q[gi] = make_float4(rotated<T>(a, qb, r, el * 4, rope) * a.scale, rotated<T>(a, qb, r, el * 4 + 1, rope) * a.scale,
                                rotated<T>(a, qb, r, el * 4 + 2, rope) * a.scale, rotated<T>(a, qb, r, el * 4 + 3, rope) * a.scale);
        }
    }
    float m[G], l[G];
    float4 o[G];
#pragma unroll
    for (int gi = 0; gi < G; ++gi) { m[gi] = -kFltMax; l[gi] = 0.f; o[gi] = make_float4(0.f, 0.f, 0.f, 0.f); }
    const int64_t nh = n * a.kv_heads + kvh;
    const float* pk = a.past_k + nh * int64_t(P) * HD;
    const float* pv = a.past_v + nh * int64_t(P) * HD;
    float* ok = a.present_k + nh * int64_t(Lk) * HD;
    float* ov = a.present_v + nh * int64_t(Lk) * HD;
    // the K / V vectors of a cached row; the next iteration's are requested before this iteration's arithmetic, so their latency lies under it
    auto load_row = [&](int j, float4& kx, float4& vx) {
        kx = *reinterpret_cast<const float4*>(pk + int64_t(j) * HD + el * 4);
        vx = *reinterpret_cast<const float4*>(pv + int64_t(j) * HD + el * 4);
    };
    float4 kn = make_float4(0.f, 0.f, 0.f, 0.f), vn = kn;
    if (k0 + slot < k1 && k0 + slot < P) load_row(k0 + slot, kn, vn);
    for (int jb = k0; jb < k1; jb += KT) {         // workgroup-uniform
        const int j = jb + slot;
        const bool valid = j < k1;
        float4 kx = kn, vx = vn;                   // (a slot past the split's end keeps stale finite values: its scores are never used)
        if (j + KT < k1 && j + KT < P) load_row(j + KT, kn, vn);
        if (valid) {
            if (j >= P) {                          // the new row: k rotated, v as it is, both fp32
                const int64_t kb = qkv_base(a, n, 0, 1, kvh), vb = qkv_base(a, n, 0, 2, kvh);
                const T* p = reinterpret_cast<const T*>(a.in.p);
                kx = make_float4(rotated<T>(a, kb, r, el * 4, rope), rotated<T>(a, kb, r, el * 4 + 1, rope), rotated<T>(a, kb, r, el * 4 + 2, rope),
                                 rotated<T>(a, kb, r, el * 4 + 3, rope));
                vx = make_float4(float(p[vb + int64_t(el * 4) * a.in.sc]), float(p[vb + int64_t(el * 4 + 1) * a.in.sc]), float(p[vb + int64_t(el * 4 + 2) * a.in.sc]),
                                 float(p[vb + int64_t(el * 4 + 3) * a.in.sc]));
            }
            *reinterpret_cast<float4*>(ok + int64_t(j) * HD + el * 4) = kx;
            *reinterpret_cast<float4*>(ov + int64_t(j) * HD + el * 4) = vx;
        }
        const float bias = valid && a.mask ? key_bias(a, n, j) : 0.f;
#pragma unroll
        for (int gi = 0; gi < G; ++gi) {
            float s = group_sum<LPK>(dot4(q[gi], kx));
            if (valid && gi < g) {
                if (a.mask) s = fmaxf(s + bias, -kFltMax);
                const float mn = fmaxf(m[gi], s), al = __expf(m[gi] - mn), p = __expf(s - mn);
                l[gi] = l[gi] * al + p;
                o[gi].x = fmaf(p, vx.x, o[gi].x * al);
                o[gi].y = fmaf(p, vx.y, o[gi].y * al);
                o[gi].z = fmaf(p, vx.z, o[gi].z * al);
                o[gi].w = fmaf(p, vx.w, o[gi].w * al);
                m[gi] = mn;
            }
        }
    }
    // merge the workgroup's key slots: (m, l) and o of every slot and query head through LDS, then one thread per (query head, element)
#pragma unroll
    for (int gi = 0; gi < G; ++gi) {
        if (el == 0) { s_ml[slot][gi][0] = m[gi]; s_ml[slot][gi][1] = l[gi]; }
        *reinterpret_cast<float4*>(&s_o[slot][gi][el * 4]) = o[gi];
    }
    __syncthreads();
    for (int idx = int(threadIdx.x); idx < g * HD; idx += kDecodeBlock) {
        const int gi = idx / HD, e = idx % HD;
        float M = -kFltMax;
#pragma unroll
        for (int t = 0; t < NS; ++t) M = fmaxf(M, s_ml[t][gi][0]);
        float Lsum = 0.f, O = 0.f;
#pragma unroll
        for (int t = 0; t < NS; ++t) {
            const float w = __expf(s_ml[t][gi][0] - M);
            Lsum = fmaf(s_ml[t][gi][1], w, Lsum);
            O = fmaf(s_o[t][gi][e], w, O);
        }
        const int h = kvh * g + gi;
        if (S == 1) {
            reinterpret_cast<T*>(a.out.p)[n * a.out.sn + (int64_t(h) * HD + e) * a.out.sc] = T(O / Lsum);
        } else {                                   // record (n, h, split): m, l, o[HD]
            float* rec = a.workspace + ((n * a.heads + h) * S + sp) * int64_t(HD + 2);
            if (e == 0) { rec[0] = M; rec[1] = Lsum; }
            rec[2 + e] = O;
        }
    }
}

// one thread per (image, query head, element): the S records of the head in split order
template <typename T>
__global__ __launch_bounds__(kDecodeBlock) void attention_decode_combine_kernel(const DecodeArgs a, const int64_t total) {
    const int64_t i = int64_t(blockIdx.x) * kDecodeBlock + threadIdx.x;
    if (i >= total) return;
    const int hd = a.head_dim, S = a.splits;
    const int e = int(i % hd);
    const int64_t nh = i / hd;                     // n heads + h
    const float* rec = a.workspace + nh * S * int64_t(hd + 2);
    float M = -kFltMax;
    for (int s = 0; s < S; ++s) M = fmaxf(M, rec[int64_t(s) * (hd + 2)]);
    float L = 0.f, O = 0.f;
    for (int s = 0; s < S; ++s) {
        const float* rs = rec + int64_t(s) * (hd + 2);
        const float w = __expf(rs[0] - M);
        L = fmaf(rs[1], w, L);
        O = fmaf(rs[2 + e], w, O);
    }
    const int64_t n = nh / a.heads, h = nh % a.heads;
    reinterpret_cast<T*>(a.out.p)[n * a.out.sn + (h * hd + e) * a.out.sc] = T(O / L);
}

bool cache_ok(const DecodeArgs& a) {
    return a.in.p && a.present_k && a.present_v && a.heads >= 1 && a.kv_heads >= 1 && a.heads % a.kv_heads == 0 && a.head_dim >= 1 && a.past_len >= 0 && a.new_len >= 1 &&
           a.in.w == a.new_len && !a.in.f8 && (a.past_len == 0 || (a.past_k && a.past_v)) && (!a.rope_cos || (a.rope_sin && a.rope_rows >= 1 && a.head_dim % 2 == 0)) &&
           int64_t(a.in.c) == int64_t(a.heads + 2 * a.kv_heads) * a.head_dim;
}

template <typename T, int HD>
hipError_t launch_decode_g(const DecodeArgs& a, hipStream_t stream) {
    const dim3 grid(unsigned(a.splits), unsigned(a.kv_heads), unsigned(a.in.n));
    const int g = a.heads / a.kv_heads;
    if (g == 1) hipLaunchKernelGGL((attention_decode_kernel<T, HD, 1>), grid, dim3(kDecodeBlock), 0, stream, a);
    else if (g == 2) hipLaunchKernelGGL((attention_decode_kernel<T, HD, 2>), grid, dim3(kDecodeBlock), 0, stream, a);
    else if (g <= 4) hipLaunchKernelGGL((attention_decode_kernel<T, HD, 4>), grid, dim3(kDecodeBlock), 0, stream, a);
    else hipLaunchKernelGGL((attention_decode_kernel<T, HD, 8>), grid, dim3(kDecodeBlock), 0, stream, a);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_decode(const DecodeArgs& a, hipStream_t stream) {
    const hipError_t e = a.head_dim == 32 ? launch_decode_g<T, 32>(a, stream) : (a.head_dim == 64 ? launch_decode_g<T, 64>(a, stream) : launch_decode_g<T, 128>(a, stream));
    if (e != hipSuccess || a.splits == 1) return e;
    const int64_t total = int64_t(a.in.n) * a.heads * a.head_dim;
    hipLaunchKernelGGL((attention_decode_combine_kernel<T>), dim3(unsigned((total + kDecodeBlock - 1) / kDecodeBlock)), dim3(kDecodeBlock), 0, stream, a, total);
    return hipGetLastError();
}

}  // namespace

bool KvAppendEligible(const DecodeArgs& a) {
    if (!cache_ok(a)) return false;
    const int64_t total = int64_t(a.in.n) * a.kv_heads * (int64_t(a.past_len) + a.new_len) * a.head_dim;
    return total / kDecodeBlock < (int64_t(1) << 31);
}

hipError_t LaunchKvAppend(const DecodeArgs& a, hipStream_t stream) {
    if (!KvAppendEligible(a)) return hipErrorInvalidValue;
    if (a.in.n == 0) return hipSuccess;
    const int64_t floats = int64_t(a.in.n) * a.kv_heads * (int64_t(a.past_len) + a.new_len) * a.head_dim;
    const bool vec = a.head_dim % 4 == 0 && Aligned16(a.present_k) && Aligned16(a.present_v) && (a.past_len == 0 || (Aligned16(a.past_k) && Aligned16(a.past_v)));
    const int64_t total = vec ? floats / 4 : floats;
    const dim3 grid(unsigned((total + kDecodeBlock - 1) / kDecodeBlock));
    if (vec) {
        if (a.in.f16) hipLaunchKernelGGL((kv_append_kernel<_Float16, 4>), grid, dim3(kDecodeBlock), 0, stream, a, total);
        else hipLaunchKernelGGL((kv_append_kernel<float, 4>), grid, dim3(kDecodeBlock), 0, stream, a, total);
    } else {
        if (a.in.f16) hipLaunchKernelGGL((kv_append_kernel<_Float16, 1>), grid, dim3(kDecodeBlock), 0, stream, a, total);
        else hipLaunchKernelGGL((kv_append_kernel<float, 1>), grid, dim3(kDecodeBlock), 0, stream, a, total);
    }
    return hipGetLastError();
}

bool AttentionDecodeEligible(const DecodeArgs& a, int tile) {
    if (!cache_ok(a) || !a.out.p || a.out.f8 || a.in.f16 != a.out.f16 || a.new_len != 1 || a.past_len < 1 || a.head_dim > kDecodeMaxHeadDim) return false;
    if (int64_t(a.out.c) != int64_t(a.heads) * a.head_dim) return false;
    if (tile == 0) return true;
    if (tile != kAttnDecodeTile) return false;
    if (!DecodeFastFits(a.head_dim, a.heads, a.kv_heads, a.mask != nullptr, a.mask_value)) return false;
    if (!Aligned16(a.past_k) || !Aligned16(a.past_v) || !Aligned16(a.present_k) || !Aligned16(a.present_v)) return false;
    const int64_t keys = int64_t(a.past_len) + 1, tiles = (keys + DecodeKeyTile(a.head_dim) - 1) / DecodeKeyTile(a.head_dim);
    if (a.splits < 1 || a.splits > kDecodeMaxSplits || a.splits > tiles || a.kv_heads > 65535 || a.in.n > 65535) return false;
    return a.splits == 1 || (a.workspace && DecodeWorkspaceFloats(a.in.n, a.heads, a.head_dim, a.splits) <= a.workspace_floats);
}

// tile 0 attends over `present` as a kv_append launch left it; tile 4 copies, appends and attends in one launch (plus the combine)
hipError_t LaunchAttentionDecode(const DecodeArgs& a, int tile, hipStream_t stream) {
    if (!AttentionDecodeEligible(a, tile)) return hipErrorInvalidValue;
    if (a.in.n == 0) return hipSuccess;
    if (tile == 0) {
        const int64_t rows = int64_t(a.in.n) * a.heads;
        const int64_t blocks = (rows + kDecodeBlock / 64 - 1) / (kDecodeBlock / 64);
        if (blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
        if (a.in.f16) hipLaunchKernelGGL((attention_decode_generic_kernel<_Float16>), dim3(unsigned(blocks)), dim3(kDecodeBlock), 0, stream, a, rows);
        else hipLaunchKernelGGL((attention_decode_generic_kernel<float>), dim3(unsigned(blocks)), dim3(kDecodeBlock), 0, stream, a, rows);
        return hipGetLastError();
    }
    return a.in.f16 ? launch_decode<_Float16>(a, stream) : launch_decode<float>(a, stream);
}

}  // namespace ie
