// KV cache for generation with Llama-class graphs on gfx950: the append of a step's new K / V rows to the cache, the one-token decode attention and the
// attention of an extend step (several new tokens over a cache).
//
// The cache tensors are fp32 in every precision and dense [N][Hkv][rows][hd] (kernels.h DecodeArgs): `past` with P rows comes in, `present` with
// P + L rows goes out.  A decode step (L = 1) is a bandwidth problem: the arithmetic is 2 FMAs per cached element and query head, so the kernels
// are arranged around reading the cache once at the HBM rate.
//
//   kv_append_kernel<T, V>               one lane per V consecutive floats of `present` (V = 4: 16-byte vectors; V = 1: a head dim that is no
//                                        multiple of 4).  Rows < P: the past row, bit for bit.  Row P + l: k of token l after the rotary embedding
//                                        (x cos + rotate_half(x) sin at the token's table row pos[n][l], fp32 arithmetic as AttnArgs describes it) resp. v of
//                                        token l, converted to fp32.  Without a past (a prefill with a cache) it writes all L rows.
//   attention_decode_generic_kernel<T>   tile 0: one wave per (image, query head) over `present`, which a kv_append launch wrote.  Lane l owns the head
//                                        elements l, l + 64, ...; per key one wave reduction gives the score, the online softmax runs in every lane
//                                        alike.  Any hd <= 512, any P, with or without a mask: the route for whatever tile 4 declines, and the cross-check.
//   attention_extend_generic_kernel<T>   tile 0 of an extend step (a past and Lq >= 2 new tokens): the same wave per (image, query head, new token i) over the
//                                        first P + i + 1 rows of `present`: the chunk is causal by chunk index, q is rotated at its token's own table row.
//   attention_extend_kernel<T, HD>       tile 5 of an extend step, behind the kv_append launch: a workgroup = (image, K / V head, 128 query rows of the head
//                                        group, key split) stages `present` through LDS in chunks and runs tile 1's MFMA softmax with the key mask and the
//                                        chunk's causal limit (described at the kernel); S > 1: attention_extend_combine_kernel<T> adds the split records.
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
// In place (DecodeArgs::cache_rows > 0: the model is bound to a resident cache): past and present are one storage with its own row stride, the
// image's valid length len and the tokens c it appends come from two device arrays, and nothing of the cache is copied.
//   kv_append_rows_kernel<T, V>          writes the rotated k and the v of the tokens i < c at the rows len + i and touches nothing else.
//   attention_inplace_generic_kernel<T>  tile 0 of a decode and of an extend step: the wave of the generic kernels over the rows the token may see.
//   attention_decode_kernel<.., true>    tile 4 without the `present` store: the key loop covers [0, len), one workgroup writes row len from registers.
//   attention_extend_kernel<.., true>    tile 5 behind the kv_append_rows launch, its causal limit counted from len.
//
// Scores, statistics and accumulation are fp32.  The key-mask bias (1 - float(mask[n, j])) * c is added to the scaled score in fp32 and the sum clamped
// at -FLT_MAX, as the MASK forms of kernels_attn.hip keep it finite: the running maximum starts at -FLT_MAX too, so a split (or a whole row) whose
// keys are all masked has m = -FLT_MAX, l = its key count and o = the plain sum of its V rows; next to a split with a real score its weight
// exp(-FLT_MAX - M) is exactly 0, and a fully masked row comes out as the uniform average of V, which is what the graph's own sum gives.
// The VALU dot-product form was chosen over MFMA 16x16x4 on padded query rows because g <= 8 rows would leave half or more of every MFMA idle.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "attn_mfma.h"
#include "kernels.h"
#include "launch_util.h"

namespace ie {
namespace {

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

// In place: one lane per V consecutive floats of the step's new rows [N][Hkv][new_len][hd].  Token l < c of image n: k after the rotary embedding and v
// go to row len + l of the cache (kv_append_kernel's arithmetic); a token l >= c and every other row of the cache: untouched
template <typename T, int V>
__global__ __launch_bounds__(kDecodeBlock) void kv_append_rows_kernel(const DecodeArgs a, const int64_t total) {
    const int64_t i = int64_t(blockIdx.x) * kDecodeBlock + threadIdx.x;      // ((n Hkv + kvh) new_len + l) hd / V + ev
    if (i >= total) return;
    const int hd = a.head_dim, vpr = hd / V;
    const int ev = int(i % vpr);
    const int l = int((i / vpr) % a.new_len);
    const int64_t nh = i / (int64_t(vpr) * a.new_len);      // n Hkv + kvh
    const int kvh = int(nh % a.kv_heads);
    const int64_t n = nh / a.kv_heads;
    const Resident rs = resident(a, n);
    if (l >= rs.c) return;
    const int64_t o = (nh * a.cache_rows + rs.len + l) * hd + int64_t(ev) * V;
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

// One wave of tile 0: query head h of token i of image n over the first Lk rows of its K / V head at K / Vp.  The first `biased` of them carry their mask
// column's bias (the new rows of a resident cache carry none: their columns are of the prefix of ones); the shift is the largest bias among the keys the
// query sees.  ZERO_EMPTY: a row with nothing visible (l = 0) comes out as zeros, and the row is scaled by 1 / l instead of divided by l
template <typename T, bool ZERO_EMPTY>
__device__ __forceinline__ void attend_wave(const DecodeArgs& a, int64_t n, int h, int i, const float* K, const float* Vp, int Lk, int biased) {
    constexpr int kChunks = kDecodeMaxHeadDim / 64;
    const int lane = int(threadIdx.x) % 64;
    const int hd = a.head_dim;
    const bool rope = a.rope_cos != nullptr;
    const int64_t r = rope ? rope_row(a, n, i) : 0;
    const int64_t qb = qkv_base(a, n, i, 0, h);
    float q[kChunks], acc[kChunks];
#pragma unroll
    for (int c = 0; c < kChunks; ++c) {
        const int e = c * 64 + lane;
        q[c] = e < hd ? rotated<T>(a, qb, r, e, rope) * a.scale : 0.f;
        acc[c] = 0.f;
    }
    float shift = 0.f;
    if (a.mask) {
        float bm = Lk > biased ? 0.f : -kFltMax;   // (a visible key without a bias has the bias 0)
        for (int j = lane; j < biased; j += 64) bm = fmaxf(bm, key_bias(a, n, j));
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
        if (a.mask) s = fmaxf(s + ((j < biased ? key_bias(a, n, j) : 0.f) - shift), -kFltMax);
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
    const int64_t ob = n * a.out.sn + int64_t(i) * a.out.sw + int64_t(h) * hd * a.out.sc;
    [[maybe_unused]] const float inv = l > 0.f ? 1.f / l : 0.f;
#pragma unroll
    for (int c = 0; c < kChunks; ++c) {
        const int e = c * 64 + lane;
        if (e >= hd) continue;
        if constexpr (ZERO_EMPTY) out[ob + int64_t(e) * a.out.sc] = T(acc[c] * inv);
        else out[ob + int64_t(e) * a.out.sc] = T(acc[c] / l);
    }
}

// tile 0 over `present` as a kv_append launch wrote it, `rows` rows per K / V head: every visible key carries its bias, and the new one is always visible
template <typename T>
__device__ __forceinline__ void attend_present(const DecodeArgs& a, int64_t n, int h, int i, int Lk, int rows) {
    const int64_t kv = (n * a.kv_heads + h / (a.heads / a.kv_heads)) * int64_t(rows) * a.head_dim;
    attend_wave<T, false>(a, n, h, i, a.present_k + kv, a.present_v + kv, Lk, Lk);
}

// rows = N * heads, one wave each: a decode step sees all P + 1 rows
template <typename T>
__global__ __launch_bounds__(kDecodeBlock) void attention_decode_generic_kernel(const DecodeArgs a, const int64_t rows) {
    const int64_t row = int64_t(blockIdx.x) * (kDecodeBlock / 64) + threadIdx.x / 64;
    if (row >= rows) return;                       // wave-uniform
    attend_present<T>(a, row / a.heads, int(row % a.heads), 0, a.past_len + 1, a.past_len + 1);
}

// rows = N * heads * Lq, one wave per (image, query head, new token i), the token fastest: key j is visible to token i iff j <= P + i, the first
// P + i + 1 of the P + Lq rows, the rest being the chunk's future
template <typename T>
__global__ __launch_bounds__(kDecodeBlock) void attention_extend_generic_kernel(const DecodeArgs a, const int64_t rows) {
    const int64_t row = int64_t(blockIdx.x) * (kDecodeBlock / 64) + threadIdx.x / 64;
    if (row >= rows) return;                       // wave-uniform
    const int Lq = a.new_len, i = int(row % Lq);
    const int64_t nh = row / Lq;
    attend_present<T>(a, nh / a.heads, int(nh % a.heads), i, a.past_len + i + 1, a.past_len + Lq);
}

// In place, tile 0 of a decode step (new_len = 1) and of an extend step alike: rows = N * heads * new_len, one wave per (image, query head, new token i), the
// token fastest, over the resident cache a kv_append_rows launch has appended to.  The wave walks the rows [0, len + min(i, c - 1)] and no other: a
// row below len carries its mask column's bias, a new row none; a token with nothing visible writes zeros
template <typename T>
__global__ __launch_bounds__(kDecodeBlock) void attention_inplace_generic_kernel(const DecodeArgs a, const int64_t rows) {
    const int64_t row = int64_t(blockIdx.x) * (kDecodeBlock / 64) + threadIdx.x / 64;
    if (row >= rows) return;                       // wave-uniform
    const int Lq = a.new_len, i = int(row % Lq);
    const int64_t nh = row / Lq, n = nh / a.heads;
    const int h = int(nh % a.heads);
    const Resident rs = resident(a, n);
    const int64_t kv = (n * a.kv_heads + h / (a.heads / a.kv_heads)) * a.cache_rows * a.head_dim;
    attend_wave<T, true>(a, n, h, i, a.present_k + kv, a.present_v + kv, rs.len + (i < rs.c ? i : rs.c - 1) + 1, rs.len);
}

__device__ __forceinline__ float dot4(const float4 a, const float4 b) { return fmaf(a.x, b.x, fmaf(a.y, b.y, fmaf(a.z, b.z, a.w * b.w))); }

// grid = (splits, Hkv, N).  INPLACE: the form of a step bound to a resident cache, which is read where it lives and of which nothing is stored again.  The S
// splits share the image's len cached keys in whole key tiles at run time (the grid is the plan's: a split beyond them has no keys and writes
// (-FLT_MAX, 0, 0), which the combine weights with exactly 0); no workgroup reads a row at or beyond len, so the one row that is written (row len, by
// one workgroup, from registers) is read by nobody in this launch
template <typename T, int HD, int G, bool INPLACE = false>
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
    const int g = a.heads / a.kv_heads;
    Resident rs = {0, 0};
    if constexpr (INPLACE) rs = resident(a, n);
    const int P = INPLACE ? rs.len : a.past_len, Lk = INPLACE ? P : P + 1;      // in place: the cached keys alone, the new one comes from registers below
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
    const float* pk = a.past_k + nh * (INPLACE ? a.cache_rows : int64_t(P)) * HD;
    const float* pv = a.past_v + nh * (INPLACE ? a.cache_rows : int64_t(P)) * HD;
    float* ok = a.present_k + nh * (INPLACE ? a.cache_rows : int64_t(Lk)) * HD;
    float* ov = a.present_v + nh * (INPLACE ? a.cache_rows : int64_t(Lk)) * HD;
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
        if constexpr (!INPLACE) if (valid) {
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
    if constexpr (INPLACE) {
        // the split that holds the last cached key (none cached: the last split) owns the new row: every lane builds its slice of it, slot 0 stores it
        // at row len and attends to it.  c == 0 (a padded token, or a full cache): nothing is stored, the key is not visible
        const int owner = tiles > 0 ? (tiles - 1) / per : S - 1;
        if (sp == owner) {                         // workgroup-uniform
            const int64_t kb = qkv_base(a, n, 0, 1, kvh), vb = qkv_base(a, n, 0, 2, kvh);
            const T* p = reinterpret_cast<const T*>(a.in.p);
            const float4 kx = make_float4(rotated<T>(a, kb, r, el * 4, rope), rotated<T>(a, kb, r, el * 4 + 1, rope), rotated<T>(a, kb, r, el * 4 + 2, rope),
                                          rotated<T>(a, kb, r, el * 4 + 3, rope));
            const float4 vx = make_float4(float(p[vb + int64_t(el * 4) * a.in.sc]), float(p[vb + int64_t(el * 4 + 1) * a.in.sc]), float(p[vb + int64_t(el * 4 + 2) * a.in.sc]),
                                          float(p[vb + int64_t(el * 4 + 3) * a.in.sc]));
            const bool mine = slot == 0 && rs.c > 0;
            if (mine) {
                *reinterpret_cast<float4*>(ok + int64_t(P) * HD + el * 4) = kx;
                *reinterpret_cast<float4*>(ov + int64_t(P) * HD + el * 4) = vx;
            }
#pragma unroll
            for (int gi = 0; gi < G; ++gi) {
                const float s = group_sum<LPK>(dot4(q[gi], kx));
                if (mine && gi < g) {
                    const float mn = fmaxf(m[gi], s), al = __expf(m[gi] - mn), pr = __expf(s - mn);
                    l[gi] = l[gi] * al + pr;
                    o[gi].x = fmaf(pr, vx.x, o[gi].x * al);
                    o[gi].y = fmaf(pr, vx.y, o[gi].y * al);
                    o[gi].z = fmaf(pr, vx.z, o[gi].z * al);
                    o[gi].w = fmaf(pr, vx.w, o[gi].w * al);
                    m[gi] = mn;
                }
                // nothing visible at all (no cached key, no new one): the weight 1 on a zero row keeps the token's output finite, and next to a real
                // maximum the record's weight is exactly 0
                if (slot == 0 && P == 0 && rs.c == 0) l[gi] = 1.f;
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

// Tile 5 of an extend step.  grid = (row blocks x S, Hkv, N), dynamic LDS = ExtendLdsBytes(HD, half); runs behind the kv_append launch and reads K / V
// from the fp32 `present` only.  A workgroup is (image, K / V head, block of 128 query rows, key split): the query rows of the group enumerate (new token
// i, head-in-group r) as row = i g + r, so a wave's 32 rows (one per lane column, tile 1's orientation: S^T = K Q^T, O^T += V^T P^T with MFMA 32x32x2f32 /
// 32x32x16_f16) have visible-key limits P + i that grow with the row.  K and V of the K / V head pass through LDS in chunks of kAttnChunkKeys keys,
// converted to T where they enter it, the chunk's key biases (units of log2, clamped at -FLT_MAX) beside them: every `present` element is read from
// HBM once per (image, K / V head, row block, split), never once per query head.
// Masking: a key-masked key keeps its clamped bias and the running maximum starts at -FLT_MAX, so a tile, chunk or split of masked keys leaves with
// weight exactly 0 next to a real score (tile 4's rule); a causally hidden key (key > P + i; the padded keys of the last tile are such) is -inf and is
// tested only in the key tiles that reach beyond P + (the wave's first token); a lane with nothing visible in a tile keeps its finite maximum.
// EVERY wave takes part in EVERY barrier (tile 3's rule): a wave whose rows lie beyond g Lq, or that is past its last tile (the one that holds P + its
// last token), keeps staging and waiting and only skips the key tiles.
// S > 1: split s takes the key tiles [s per, (s + 1) per) of ceil((P + Lq) / 32), cut at the row block's last visible key, and writes (m, l, o[HD]) per
// query row into the workspace, record ((n H + h) Lq + i) S + s; a split with nothing visible for a row writes (-FLT_MAX, 0, 0).
// INPLACE: behind a kv_append_rows launch, over the resident cache with its own row stride.  The image's len and c come
// from the device arrays, so every limit above counts from len instead of P: token i sees the rows <= len + min(i, c - 1), of which a row below len
// carries its mask column's bias and a new row none; the splits share the len + c rows that exist; rows at or beyond len + c are never read, those that
// fall into a staged chunk are zeros in LDS as the padded keys are.  All of this is uniform over the workgroup (len and c belong to the image), so the
// barrier rule holds as it stands.  A row with nothing visible at all (c = 0 over an empty cache) takes the weight 1 on its zero sum in split 0
template <typename T, int HD, bool INPLACE = false>
__global__ __launch_bounds__(kDecodeBlock) void attention_extend_kernel(const DecodeArgs a) {
    constexpr bool F16 = sizeof(T) == 2;
    constexpr int V = 16 / int(sizeof(T));         // elements per 16-byte vector
    constexpr int RS = HD + V;                     // LDS row stride in elements
    constexpr int HH = HD / 2;                     // head-dim elements one lane half supplies to QK^T
    constexpr int KC = kAttnChunkKeys;
    constexpr int VPR = HD / 4;                    // float4s of a `present` row
    static_assert(KC % 32 == 0, "whole key tiles per chunk");
    extern __shared__ __attribute__((aligned(16))) unsigned char extend_smem[];
    T* Ks = reinterpret_cast<T*>(extend_smem);
    T* Vs = Ks + size_t(KC) * RS;
    float* Bs = reinterpret_cast<float*>(Vs + size_t(KC) * RS);
    const int S = a.splits, rb = int(blockIdx.x) / S, sp = int(blockIdx.x) % S, kvh = int(blockIdx.y);
    const int64_t n = blockIdx.z;
    int len = a.past_len, app = a.new_len;         // the rows in front of the chunk and the tokens that append
    if constexpr (INPLACE) { const Resident rs = resident(a, n); len = rs.len; app = rs.c; }
    const int g = a.heads / a.kv_heads, P = len, Lq = a.new_len, R = g * Lq, Lk = INPLACE ? P + app : P + Lq;
    const int wave = int(threadIdx.x) / 64, lane = int(threadIdx.x) % 64, col = lane & 31, hf = lane >> 5;
    const int q0 = rb * 128 + wave * 32;
    const bool live = q0 < R;                      // wave-uniform
    const int row = q0 + col < R ? q0 + col : R - 1;
    const int tok = row / g, h = kvh * g + row % g;
    auto seen = [app](int t) { return INPLACE && t >= app ? app - 1 : t; };      // the new rows token t sees beyond its cached ones, less one
    const int lim = P + seen(tok);                 // this lane's last visible key
    const int first_tok = (q0 < R ? q0 : R - 1) / g, last_tok = (q0 + 31 < R ? q0 + 31 : R - 1) / g;
    const int wave_end = live ? P + seen(last_tok) + 1 : 0;      // the wave's keys: [0, wave_end)
    const int free_end = P + seen(first_tok) + 1;                // keys below it are visible to every row of the wave
    const int wg_end = P + seen((rb * 128 + 127 < R ? rb * 128 + 127 : R - 1) / g) + 1;
    const int per = ((Lk + 31) / 32 + S - 1) / S;
    const int kbeg = sp * per * 32, kend = wg_end < (sp + 1) * per * 32 ? wg_end : (sp + 1) * per * 32;      // the workgroup's keys (none: kbeg >= kend)

    // this lane's half of its Q row, rotated at its token's own table row (the lane halves are the two rope halves); halfs are rounded once, here
    float4 q4[F16 ? 1 : HH / 4];
    h8 q8[F16 ? HH / 8 : 1];
    {
        const T* qh = reinterpret_cast<const T*>(a.in.p) + n * a.in.sn + int64_t(tok) * a.in.sw + h * HD;
        const bool rope = a.rope_cos != nullptr;
        const int64_t t = rope ? rope_row(a, n, tok) * HD + hf * HH : 0;
        float qf[HH];
#pragma unroll
        for (int k = 0; k < HH; ++k) {
            const float x = float(qh[hf * HH + k]);
            qf[k] = x;
            if (rope) {
                const float xp = float(qh[(1 - hf) * HH + k]);
                qf[k] = fmaf(x, a.rope_cos[t + k], (hf ? xp : -xp) * a.rope_sin[t + k]);
            }
        }
        if constexpr (F16) {
#pragma unroll
            for (int k = 0; k < HH; ++k) q8[k / 8][k % 8] = _Float16(qf[k]);
        } else {
#pragma unroll
            for (int k = 0; k < HH / 4; ++k) q4[k] = make_float4(qf[4 * k], qf[4 * k + 1], qf[4 * k + 2], qf[4 * k + 3]);
        }
    }
    f32x16 o0, o1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
    float m = -kFltMax, lsum = 0.f;
    const float sl2 = a.scale * kLog2e;            // scores in units of log2: exp(x) = exp2(x * log2 e)
    const float* pk = a.present_k + (n * a.kv_heads + kvh) * (INPLACE ? a.cache_rows : int64_t(Lk)) * HD;
    const float* pv = a.present_v + (n * a.kv_heads + kvh) * (INPLACE ? a.cache_rows : int64_t(Lk)) * HD;

    for (int c0 = kbeg; c0 < kend; c0 += KC) {     // (the bounds are the workgroup's: every wave runs every iteration)
        const int rows = kend - c0 < KC ? (kend - c0 + 31) / 32 * 32 : KC;
        for (int idx = int(threadIdx.x); idx < rows * VPR; idx += kDecodeBlock) {
            const int lr = idx / VPR, cv = idx % VPR, key = c0 + lr;
            float4 kx = make_float4(0.f, 0.f, 0.f, 0.f), vx = kx;                         // rows past P + Lq: zeros (a zero probability times them stays zero)
            if (key < Lk) {
                kx = *reinterpret_cast<const float4*>(pk + int64_t(key) * HD + cv * 4);
                vx = *reinterpret_cast<const float4*>(pv + int64_t(key) * HD + cv * 4);
            }
            if constexpr (F16) {
                h4 kh, vh;
                kh[0] = _Float16(kx.x); kh[1] = _Float16(kx.y); kh[2] = _Float16(kx.z); kh[3] = _Float16(kx.w);
                vh[0] = _Float16(vx.x); vh[1] = _Float16(vx.y); vh[2] = _Float16(vx.z); vh[3] = _Float16(vx.w);
                *reinterpret_cast<h4*>(Ks + lr * RS + cv * 4) = kh;
                *reinterpret_cast<h4*>(Vs + lr * RS + cv * 4) = vh;
            } else {
                *reinterpret_cast<float4*>(Ks + lr * RS + cv * 4) = kx;
                *reinterpret_cast<float4*>(Vs + lr * RS + cv * 4) = vx;
            }
        }
        for (int j = int(threadIdx.x); j < rows; j += kDecodeBlock)
            Bs[j] = c0 + j < (INPLACE ? P : Lk) ? fmaxf(key_bias(a, n, c0 + j) * kLog2e, -kFltMax) : 0.f;      // (a padded key is causally hidden from every row)
        __syncthreads();
        const int cend = c0 + rows < wave_end ? c0 + rows : wave_end;
        for (int key0 = c0; key0 < cend; key0 += 32) {
            const T* Kt = Ks + (key0 - c0) * RS;
            const T* Vt = Vs + (key0 - c0) * RS;
            const float* Bt = Bs + (key0 - c0);
            f32x16 s;
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = 0.f;
            const T* krow = Kt + col * RS + hf * HH;
            if constexpr (F16) {
#pragma unroll
                for (int k = 0; k < HH; k += 8) s = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const h8*>(krow + k), q8[k / 8], s, 0, 0, 0);
            } else {
#pragma unroll
                for (int k = 0; k < HH; k += 4) {
                    const float4 kf = *reinterpret_cast<const float4*>(krow + k);
                    s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.x, q4[k / 4].x, s, 0, 0, 0);
                    s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.y, q4[k / 4].y, s, 0, 0, 0);
                    s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.z, q4[k / 4].z, s, 0, 0, 0);
                    s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.w, q4[k / 4].w, s, 0, 0, 0);
                }
            }
            const bool edge = key0 + 32 > free_end;        // wave-uniform: this tile reaches beyond what the wave's first token sees
            float mx = -__builtin_huge_valf();
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int kt = (r & 3) + 8 * (r >> 2) + 4 * hf;
                const float b = fmaxf(fmaf(s[r], sl2, Bt[kt]), -kFltMax);
                s[r] = edge && key0 + kt > lim ? -__builtin_huge_valf() : b;
                mx = fmaxf(mx, s[r]);
            }
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float mn = fmaxf(m, mx);             // finite: m starts at -FLT_MAX
            const float alpha = fast_exp2(m - mn);
            m = mn;
            float ps = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s[r] = fast_exp2(s[r] - mn);
                ps += s[r];
                o0[r] *= alpha;
                if constexpr (HD == 64) o1[r] *= alpha;
            }
            lsum = fmaf(lsum, alpha, ps);              // this lane half's share of the row sum
            if constexpr (F16) {
#pragma unroll
                for (int st = 0; st < 2; ++st) {
                    h8 pb, va0, va1;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int kt = 16 * st + 8 * (j >> 2) + 4 * hf + (j & 3);
                        pb[j] = _Float16(s[8 * st + j]);
                        va0[j] = Vt[kt * RS + col];
                        if constexpr (HD == 64) va1[j] = Vt[kt * RS + 32 + col];
                    }
                    o0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(va0, pb, o0, 0, 0, 0);
                    if constexpr (HD == 64) o1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(va1, pb, o1, 0, 0, 0);
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int kt = (r & 3) + 8 * (r >> 2) + 4 * hf;
                    o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(float(Vt[kt * RS + col]), s[r], o0, 0, 0, 0);
                    if constexpr (HD == 64) o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(float(Vt[kt * RS + 32 + col]), s[r], o1, 0, 0, 0);
                }
            }
        }
        __syncthreads();                           // the next chunk overwrites the rows
    }

    lsum += __shfl_xor(lsum, 32, 64);
    if constexpr (INPLACE) if (lim < 0 && sp == 0) lsum = 1.f;      // nothing visible at all: zeros, finite
    if (q0 + col >= R) return;                     // behind the last barrier
    // registers 4 j ... 4 j + 3 of o0 (o1: + 32) are the output columns 8 j + 4 hf ... of this lane's query row
    if (S == 1) {
        T* orow = reinterpret_cast<T*>(a.out.p) + n * a.out.sn + int64_t(tok) * a.out.sw + h * HD;
        const float inv = 1.f / lsum;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e0 = 8 * j + 4 * hf;
            if constexpr (F16) {
                h4 x, y;
#pragma unroll
                for (int t = 0; t < 4; ++t) { x[t] = _Float16(o0[4 * j + t] * inv); y[t] = _Float16(o1[4 * j + t] * inv); }
                *reinterpret_cast<h4*>(orow + e0) = x;
                if constexpr (HD == 64) *reinterpret_cast<h4*>(orow + 32 + e0) = y;
            } else {
                *reinterpret_cast<float4*>(orow + e0) = make_float4(o0[4 * j] * inv, o0[4 * j + 1] * inv, o0[4 * j + 2] * inv, o0[4 * j + 3] * inv);
                if constexpr (HD == 64) *reinterpret_cast<float4*>(orow + 32 + e0) = make_float4(o1[4 * j] * inv, o1[4 * j + 1] * inv, o1[4 * j + 2] * inv, o1[4 * j + 3] * inv);
            }
        }
        return;
    }
    float* rec = a.workspace + (((n * a.heads + h) * Lq + tok) * S + sp) * int64_t(HD + 2);
    if (hf == 0) { rec[0] = m; rec[1] = lsum; }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e0 = 8 * j + 4 * hf;
        *reinterpret_cast<float2*>(rec + 2 + e0) = make_float2(o0[4 * j], o0[4 * j + 1]);
        *reinterpret_cast<float2*>(rec + 2 + e0 + 2) = make_float2(o0[4 * j + 2], o0[4 * j + 3]);
        if constexpr (HD == 64) {
            *reinterpret_cast<float2*>(rec + 2 + 32 + e0) = make_float2(o1[4 * j], o1[4 * j + 1]);
            *reinterpret_cast<float2*>(rec + 2 + 32 + e0 + 2) = make_float2(o1[4 * j + 2], o1[4 * j + 3]);
        }
    }
}

// one thread per (image, query head, new token, element): the S records of the row in split order (m in units of log2).  A split with nothing visible
// for the row has (-FLT_MAX, 0, 0): its weight next to a real maximum is exactly 0, and it adds nothing either way
template <typename T>
__global__ __launch_bounds__(kDecodeBlock) void attention_extend_combine_kernel(const DecodeArgs a, const int64_t total) {
    const int64_t i = int64_t(blockIdx.x) * kDecodeBlock + threadIdx.x;
    if (i >= total) return;
    const int hd = a.head_dim, S = a.splits, Lq = a.new_len;
    const int e = int(i % hd);
    const int64_t nhi = i / hd;                    // (n heads + h) Lq + token
    const float* rec = a.workspace + nhi * S * int64_t(hd + 2);
    float M = -kFltMax;
    for (int s = 0; s < S; ++s) M = fmaxf(M, rec[int64_t(s) * (hd + 2)]);
    float L = 0.f, O = 0.f;
    for (int s = 0; s < S; ++s) {
        const float* rs = rec + int64_t(s) * (hd + 2);
        const float w = fast_exp2(rs[0] - M);
        L = fmaf(rs[1], w, L);
        O = fmaf(rs[2 + e], w, O);
    }
    const int64_t tok = nhi % Lq, nh = nhi / Lq, n = nh / a.heads, h = nh % a.heads;
    reinterpret_cast<T*>(a.out.p)[n * a.out.sn + tok * a.out.sw + (h * hd + e) * a.out.sc] = T(O / L);
}

// in place: both arrays, one storage for past and present, and a capacity that is the graph's P (a prefill with a cache: at least its L rows), so that
// every mask column below len exists
bool inplace_ok(const DecodeArgs& a) {
    if (a.cache_rows == 0) return true;
    return a.lens && a.news && a.past_k == a.present_k && a.past_v == a.present_v && a.cache_rows < (int64_t(1) << 31) &&
           (a.past_len > 0 ? a.cache_rows == a.past_len : a.cache_rows >= a.new_len);
}

bool cache_ok(const DecodeArgs& a) {
    return a.in.p && a.present_k && a.present_v && a.heads >= 1 && a.kv_heads >= 1 && a.heads % a.kv_heads == 0 && a.head_dim >= 1 && a.past_len >= 0 && a.new_len >= 1 &&
           a.in.w == a.new_len && !a.in.f8 && (a.past_len == 0 || (a.past_k && a.past_v)) && (!a.rope_cos || (a.rope_sin && a.rope_rows >= 1 && a.head_dim % 2 == 0)) &&
           int64_t(a.in.c) == int64_t(a.heads + 2 * a.kv_heads) * a.head_dim && inplace_ok(a);
}

template <typename T, int HD, bool INPLACE>
hipError_t launch_decode_g(const DecodeArgs& a, hipStream_t stream) {
    const dim3 grid(unsigned(a.splits), unsigned(a.kv_heads), unsigned(a.in.n));
    const int g = a.heads / a.kv_heads;
    if (g == 1) hipLaunchKernelGGL((attention_decode_kernel<T, HD, 1, INPLACE>), grid, dim3(kDecodeBlock), 0, stream, a);
    else if (g == 2) hipLaunchKernelGGL((attention_decode_kernel<T, HD, 2, INPLACE>), grid, dim3(kDecodeBlock), 0, stream, a);
    else if (g <= 4) hipLaunchKernelGGL((attention_decode_kernel<T, HD, 4, INPLACE>), grid, dim3(kDecodeBlock), 0, stream, a);
    else hipLaunchKernelGGL((attention_decode_kernel<T, HD, 8, INPLACE>), grid, dim3(kDecodeBlock), 0, stream, a);
    return hipGetLastError();
}

template <typename T, int HD>
hipError_t launch_decode_hd(const DecodeArgs& a, hipStream_t stream) {
    return a.cache_rows > 0 ? launch_decode_g<T, HD, true>(a, stream) : launch_decode_g<T, HD, false>(a, stream);
}

template <typename T>
hipError_t launch_decode(const DecodeArgs& a, hipStream_t stream) {
    const hipError_t e = a.head_dim == 32 ? launch_decode_hd<T, 32>(a, stream) : (a.head_dim == 64 ? launch_decode_hd<T, 64>(a, stream) : launch_decode_hd<T, 128>(a, stream));
    if (e != hipSuccess || a.splits == 1) return e;
    const int64_t total = int64_t(a.in.n) * a.heads * a.head_dim;
    hipLaunchKernelGGL((attention_decode_combine_kernel<T>), dim3(unsigned((total + kDecodeBlock - 1) / kDecodeBlock)), dim3(kDecodeBlock), 0, stream, a, total);
    return hipGetLastError();
}

template <typename T, int HD>
hipError_t launch_extend(const DecodeArgs& a, hipStream_t stream) {
    const int64_t rblocks = (int64_t(a.heads / a.kv_heads) * a.new_len + 127) / 128;
    const dim3 grid(unsigned(rblocks * a.splits), unsigned(a.kv_heads), unsigned(a.in.n));
    if (a.cache_rows > 0) attention_extend_kernel<T, HD, true><<<grid, dim3(kDecodeBlock), size_t(ExtendLdsBytes(HD, sizeof(T) == 2)), stream>>>(a);
    else attention_extend_kernel<T, HD><<<grid, dim3(kDecodeBlock), size_t(ExtendLdsBytes(HD, sizeof(T) == 2)), stream>>>(a);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess || a.splits == 1) return e;
    const int64_t total = int64_t(a.in.n) * a.heads * a.new_len * a.head_dim;
    hipLaunchKernelGGL((attention_extend_combine_kernel<T>), dim3(unsigned((total + kDecodeBlock - 1) / kDecodeBlock)), dim3(kDecodeBlock), 0, stream, a, total);
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
    const bool inplace = a.cache_rows > 0;         // the new rows alone
    const int64_t floats = int64_t(a.in.n) * a.kv_heads * (inplace ? int64_t(a.new_len) : int64_t(a.past_len) + a.new_len) * a.head_dim;
    const bool vec = a.head_dim % 4 == 0 && Aligned16(a.present_k) && Aligned16(a.present_v) && (a.past_len == 0 || (Aligned16(a.past_k) && Aligned16(a.past_v)));
    const int64_t total = vec ? floats / 4 : floats;
    const dim3 grid(unsigned((total + kDecodeBlock - 1) / kDecodeBlock));
    if (inplace) {
        if (vec) {
            if (a.in.f16) hipLaunchKernelGGL((kv_append_rows_kernel<_Float16, 4>), grid, dim3(kDecodeBlock), 0, stream, a, total);
            else hipLaunchKernelGGL((kv_append_rows_kernel<float, 4>), grid, dim3(kDecodeBlock), 0, stream, a, total);
        } else {
            if (a.in.f16) hipLaunchKernelGGL((kv_append_rows_kernel<_Float16, 1>), grid, dim3(kDecodeBlock), 0, stream, a, total);
            else hipLaunchKernelGGL((kv_append_rows_kernel<float, 1>), grid, dim3(kDecodeBlock), 0, stream, a, total);
        }
        return hipGetLastError();
    }
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
    if (!cache_ok(a) || !a.out.p || a.out.f8 || a.in.f16 != a.out.f16 || a.past_len < 1 || a.head_dim > kDecodeMaxHeadDim) return false;
    if (int64_t(a.out.c) != int64_t(a.heads) * a.head_dim || (a.new_len > 1 && a.out.w != a.new_len)) return false;
    if (tile == 0) return true;
    if (a.new_len > 1) {                           // an extend step: tile 5 alone
        if (tile != kAttnExtendTile || !ExtendFastFits(a.head_dim, a.heads, a.kv_heads, a.mask != nullptr, a.mask_value)) return false;
        const int V = a.in.f16 ? 8 : 4;
        if (!VecViewOk(a.in, V) || !VecViewOk(a.out, V) || !Aligned16(a.present_k) || !Aligned16(a.present_v) || (a.rope_cos && (!Aligned16(a.rope_cos) || !Aligned16(a.rope_sin)))) return false;
        const int64_t rows = int64_t(a.heads / a.kv_heads) * a.new_len, tiles = (int64_t(a.past_len) + a.new_len + 31) / 32;
        if (a.splits < 1 || a.splits > kDecodeMaxSplits || a.splits > tiles || (rows + 127) / 128 * a.splits >= (int64_t(1) << 31) || a.kv_heads > 65535 || a.in.n > 65535) return false;
        if (int64_t(a.in.n) * a.heads * a.new_len * a.head_dim / kDecodeBlock >= (int64_t(1) << 31) || !KvAppendEligible(a)) return false;
        return a.splits == 1 || (a.workspace && ExtendWorkspaceFloats(a.in.n, a.heads, a.head_dim, a.splits, a.new_len) <= a.workspace_floats);
    }
    if (tile != kAttnDecodeTile) return false;
    if (!DecodeFastFits(a.head_dim, a.heads, a.kv_heads, a.mask != nullptr, a.mask_value)) return false;
    if (!Aligned16(a.past_k) || !Aligned16(a.past_v) || !Aligned16(a.present_k) || !Aligned16(a.present_v)) return false;
    const int64_t keys = int64_t(a.past_len) + 1, tiles = (keys + DecodeKeyTile(a.head_dim) - 1) / DecodeKeyTile(a.head_dim);
    if (a.splits < 1 || a.splits > kDecodeMaxSplits || a.splits > tiles || a.kv_heads > 65535 || a.in.n > 65535) return false;
    return a.splits == 1 || (a.workspace && DecodeWorkspaceFloats(a.in.n, a.heads, a.head_dim, a.splits) <= a.workspace_floats);
}

// tile 0 attends over `present` as a kv_append launch left it (new_len > 1: the extend kernel); tile 4 copies, appends and attends in one launch (plus the combine)
hipError_t LaunchAttentionDecode(const DecodeArgs& a, int tile, hipStream_t stream) {
    if (!AttentionDecodeEligible(a, tile)) return hipErrorInvalidValue;
    if (a.in.n == 0) return hipSuccess;
    if (tile == 0) {
        const int64_t rows = int64_t(a.in.n) * a.heads * a.new_len;
        const int64_t blocks = (rows + kDecodeBlock / 64 - 1) / (kDecodeBlock / 64);
        if (blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
        if (a.cache_rows > 0) {                    // in place: one kernel for a decode and an extend step, behind the kv_append_rows launch
            if (a.in.f16) hipLaunchKernelGGL((attention_inplace_generic_kernel<_Float16>), dim3(unsigned(blocks)), dim3(kDecodeBlock), 0, stream, a, rows);
            else hipLaunchKernelGGL((attention_inplace_generic_kernel<float>), dim3(unsigned(blocks)), dim3(kDecodeBlock), 0, stream, a, rows);
            return hipGetLastError();
        }
        if (a.new_len > 1) {
            if (a.in.f16) hipLaunchKernelGGL((attention_extend_generic_kernel<_Float16>), dim3(unsigned(blocks)), dim3(kDecodeBlock), 0, stream, a, rows);
            else hipLaunchKernelGGL((attention_extend_generic_kernel<float>), dim3(unsigned(blocks)), dim3(kDecodeBlock), 0, stream, a, rows);
            return hipGetLastError();
        }
        if (a.in.f16) hipLaunchKernelGGL((attention_decode_generic_kernel<_Float16>), dim3(unsigned(blocks)), dim3(kDecodeBlock), 0, stream, a, rows);
        else hipLaunchKernelGGL((attention_decode_generic_kernel<float>), dim3(unsigned(blocks)), dim3(kDecodeBlock), 0, stream, a, rows);
        return hipGetLastError();
    }
    if (tile == kAttnExtendTile) {                 // the append first: tile 5 reads K and V from `present` only
        if (const hipError_t e = LaunchKvAppend(a, stream); e != hipSuccess) return e;
        if (a.in.f16) return a.head_dim == 32 ? launch_extend<_Float16, 32>(a, stream) : launch_extend<_Float16, 64>(a, stream);
        return a.head_dim == 32 ? launch_extend<float, 32>(a, stream) : launch_extend<float, 64>(a, stream);
    }
    return a.in.f16 ? launch_decode<_Float16>(a, stream) : launch_decode<float>(a, stream);
}

hipError_t InitKernelsDecode() {
    const void* const kernels[] = {
        reinterpret_cast<const void*>(&attention_extend_kernel<float, 32>), reinterpret_cast<const void*>(&attention_extend_kernel<float, 64>),
        reinterpret_cast<const void*>(&attention_extend_kernel<_Float16, 32>), reinterpret_cast<const void*>(&attention_extend_kernel<_Float16, 64>),
        reinterpret_cast<const void*>(&attention_extend_kernel<float, 32, true>), reinterpret_cast<const void*>(&attention_extend_kernel<float, 64, true>),
        reinterpret_cast<const void*>(&attention_extend_kernel<_Float16, 32, true>), reinterpret_cast<const void*>(&attention_extend_kernel<_Float16, 64, true>),
    };
    for (const void* k : kernels)
        if (const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, int(kAttnLdsBudget)); e != hipSuccess) return e;
    return hipSuccess;
}

}  // namespace ie
