// Tile 6 of an extend step on gfx950: several new tokens over a KV cache at head dim 128, the head of the Llama-class models.
// kernels_decode.hip finds the step eligible, launches the append in front of this kernel and the combine behind it; what is here is the kernel, the
// choice of its wave form and its registration for more than 64 KiB of LDS.
//
// Tile 6 of an extend step.  grid = (row blocks x S, Hkv, N), dynamic LDS = ExtendWideLdsBytes(HD, half); runs behind the kv_append launch and reads K / V
// from the fp32 `present` only.  A workgroup is (image, K / V head, block of 128 / KW query rows, key split): the query rows of the group enumerate (new
// token i, head-in-group r) as row = i g + r, so a wave's 32 rows (one per lane column, tile 1's orientation: S^T = K Q^T, O^T += V^T P^T with MFMA 32x32x2f32 /
// 32x32x16_f16) have visible-key limits P + i that grow with the row.  K and V of the K / V head pass through LDS in chunks of kAttnWideChunkKeys keys,
// converted to T where they enter it, the chunk's key biases (units of log2, clamped at -FLT_MAX) beside them: every `present` element is read from
// HBM once per (image, K / V head, row block, split), never once per query head.
// WAVES (what tile 5 does not have): the four waves are 4 / KW row waves by KW key waves, wave = row wave * KW + key wave.  A row wave owns 32 query rows;
// its KW key waves hold the same rows' Q and take the 32-key tiles of every staged chunk round-robin (tile t of the chunk to key wave t % KW), each with
// its own (m, l, O).  After the last chunk the partials of the key waves 1 ... KW - 1 go to the chunk's LDS region, lane by lane, and behind one barrier
// key wave 0 adds them in key-wave order with the usual rescale; a key wave that saw nothing holds (-FLT_MAX, 0, 0) and its weight is exactly 0 (or 1
// on zeros).  The order is fixed, so two runs are bit-identical.  KW is the launcher's: 4 for R = g Lq <= 32 rows, 2 for R <= 64, else 1.
// REGISTERS: a lane keeps its half of its Q row (HD / 2 elements: the two lane halves are the two rope halves) and the HD / 32 accumulators f32x16.
// Masking: a key-masked key keeps its clamped bias and the running maximum starts at -FLT_MAX, so a tile, chunk, key wave or split of masked keys leaves
// with weight exactly 0 next to a real score (tile 4's rule); a causally hidden key (key > P + i; the padded keys of the last tile are such) is -inf and is
// tested only in the key tiles that reach beyond P + (the wave's first token); a lane with nothing visible in a tile keeps its finite maximum.
// EVERY wave takes part in EVERY barrier (tile 3's rule): a wave whose rows lie beyond g Lq, a key wave without a tile in the chunk, or one that is past
// its last tile (the one that holds P + its last token), keeps staging and waiting and only skips the key tiles.  The stores of `out` and of the
// records come behind the last barrier, from key wave 0 alone.
// S > 1: split s takes the key tiles [s per, (s + 1) per) of ceil((P + Lq) / 32), cut at the row block's last visible key, and writes (m, l, o[HD]) per
// query row into the workspace, record ((n H + h) Lq + i) S + s; a split with nothing visible for a row writes (-FLT_MAX, 0, 0).
// INPLACE: behind a kv_append_rows launch, over the resident cache with its own row stride.  The image's len and c come
// from the device arrays, so every limit above counts from len instead of P: token i sees the rows <= len + min(i, c - 1), of which a row below len
// carries its mask column's bias and a new row none; the splits share the len + c rows that exist; rows at or beyond len + c are never read, those that
// fall into a staged chunk are zeros in LDS as the padded keys are.  All of this is uniform over the workgroup (len and c belong to the image), so the
// barrier rule holds as it stands.  A row with nothing visible at all (c = 0 over an empty cache) takes the weight 1 on its zero sum in split 0, key wave 0
// KVH (a half cache, T = half, in place only): a cached row goes HBM -> LDS as HD / 8 16-byte vectors with no conversion, into the same
// rows at the same stride; everything behind the staging is the same code
#include <hip/hip_runtime.h>

#include <cstdint>

#include "attn_mfma.h"
#include "decode_util.h"
#include "kernels.h"

namespace ie {
namespace {

template <typename T, int HD, int KW, bool INPLACE = false, bool KVH = false>
__global__ __launch_bounds__(kDecodeBlock) void attention_extend_wide_kernel(const DecodeArgs a) {
    constexpr bool F16 = sizeof(T) == 2;
    constexpr int V = 16 / int(sizeof(T));         // elements per 16-byte vector
    constexpr int RS = HD + V;                     // LDS row stride in elements
    constexpr int HH = HD / 2;                     // head-dim elements one lane half supplies to QK^T
    constexpr int NA = HD / 32;                    // accumulators: o[j] holds the output columns 32 j ... 32 j + 31
    constexpr int KC = kAttnWideChunkKeys;
    constexpr int VPR = KVH ? HD / 8 : HD / 4;     // 16-byte vectors of a `present` row
    constexpr int RB = 128 / KW;                   // query rows of a workgroup
    constexpr int MS = (2 + 16 * NA) * 64;         // floats of one key wave's partial in LDS: m, l and the accumulator registers, lane fastest
    static_assert(HD == 128 && (KW == 1 || KW == 2 || KW == 4), "the wide head: 4 / KW row waves by KW key waves");
    static_assert(KC % (32 * 4) == 0, "whole key tiles per chunk, the same number for every key wave");
    static_assert(!KVH || (F16 && INPLACE), "a half cache is resident and serves half models");
    static_assert(int64_t(4 / KW) * (KW - 1) * MS * 4 <= ExtendWideLdsBytes(HD, true), "the key waves' partials fit the chunk's region");
    extern __shared__ __attribute__((aligned(16))) unsigned char extend_wide_smem[];
    T* Ks = reinterpret_cast<T*>(extend_wide_smem);
    T* Vs = Ks + size_t(KC) * RS;
    float* Bs = reinterpret_cast<float*>(Vs + size_t(KC) * RS);
    const int S = a.splits, rb = int(blockIdx.x) / S, sp = int(blockIdx.x) % S, kvh = int(blockIdx.y);
    const int64_t n = blockIdx.z;
    int len = a.past_len, app = a.new_len;         // the rows in front of the chunk and the tokens that append
    if constexpr (INPLACE) { const Resident rs = resident(a, n); len = rs.len; app = rs.c; }
    const int g = a.heads / a.kv_heads, P = len, Lq = a.new_len, R = g * Lq, Lk = INPLACE ? P + app : P + Lq;
    const int wave = int(threadIdx.x) / 64, lane = int(threadIdx.x) % 64, col = lane & 31, hf = lane >> 5;
    const int rw = wave / KW, kw = wave % KW;      // row wave and key wave
    const int q0 = rb * RB + rw * 32;
    const bool live = q0 < R;                      // wave-uniform
    const int row = q0 + col < R ? q0 + col : R - 1;
    const int tok = row / g, h = kvh * g + row % g;
    auto seen = [app](int t) { return INPLACE && t >= app ? app - 1 : t; };      // the new rows token t sees beyond its cached ones, less one
    const int lim = P + seen(tok);                 // this lane's last visible key
    const int first_tok = (q0 < R ? q0 : R - 1) / g, last_tok = (q0 + 31 < R ? q0 + 31 : R - 1) / g;
    const int wave_end = live ? P + seen(last_tok) + 1 : 0;      // the row wave's keys: [0, wave_end)
    const int free_end = P + seen(first_tok) + 1;                // keys below it are visible to every row of the wave
    const int wg_end = P + seen((rb * RB + RB - 1 < R ? rb * RB + RB - 1 : R - 1) / g) + 1;
    const int per = ((Lk + 31) / 32 + S - 1) / S;
    const int kbeg = sp * per * 32, kend = wg_end < (sp + 1) * per * 32 ? wg_end : (sp + 1) * per * 32;      // the workgroup's keys (none: kbeg >= kend)

    // this lane's half of its Q row as 16-byte vectors, rotated at its token's own table row (the lane halves are the two rope halves) in fp32; halfs
    // are rounded once, here.  The KW key waves of a row wave hold the same rows
    float4 q4[F16 ? 1 : HH / 4];
    h8 q8[F16 ? HH / 8 : 1];
    {
        const T* qh = reinterpret_cast<const T*>(a.in.p) + n * a.in.sn + int64_t(tok) * a.in.sw + h * HD;
        const bool rope = a.rope_cos != nullptr;
        const int64_t t = rope ? rope_row(a, n, tok) * HD + hf * HH : 0;
#pragma unroll
        for (int k = 0; k < HH / V; ++k) {
            uint4 x = *reinterpret_cast<const uint4*>(qh + hf * HH + V * k);
            if (rope) x = rope_vec<T>(x, *reinterpret_cast<const uint4*>(qh + (1 - hf) * HH + V * k), a.rope_cos + t + V * k, a.rope_sin + t + V * k, hf ? 1.f : -1.f);
            if constexpr (F16) q8[k] = __builtin_bit_cast(h8, x);
            else q4[k] = __builtin_bit_cast(float4, x);
        }
    }
    f32x16 o[NA];
#pragma unroll
    for (int j = 0; j < NA; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[j][r] = 0.f;
    float m = -kFltMax, lsum = 0.f;
    const float sl2 = a.scale * kLog2e;            // scores in units of log2: exp(x) = exp2(x * log2 e)
    constexpr int KVW = KVH ? 2 : 1;               // cache elements per float of the typed pointer
    const float* pk = a.present_k + (n * a.kv_heads + kvh) * (INPLACE ? a.cache_rows : int64_t(Lk)) * HD / KVW;
    const float* pv = a.present_v + (n * a.kv_heads + kvh) * (INPLACE ? a.cache_rows : int64_t(Lk)) * HD / KVW;

    for (int c0 = kbeg; c0 < kend; c0 += KC) {     // (the bounds are the workgroup's: every wave runs every iteration)
        const int rows = kend - c0 < KC ? (kend - c0 + 31) / 32 * 32 : KC;
        // four vectors of K and of V per thread are requested before the first of them is stored (tile 5's half staging, here in both forms): the
        // chunk of a short split is a handful of vectors per thread, and one at a time would pay the memory latency for each
        for (int base = int(threadIdx.x); base < rows * VPR; base += 4 * kDecodeBlock) {
            uint4 kx[4], vx[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = base + u * kDecodeBlock, lr = idx / VPR, cv = idx % VPR, key = c0 + lr;
                kx[u] = make_uint4(0u, 0u, 0u, 0u);                                       // rows past P + Lq: zeros (a zero probability times them stays zero)
                vx[u] = kx[u];
                if (idx < rows * VPR && key < Lk) {
                    kx[u] = *reinterpret_cast<const uint4*>(pk + (int64_t(key) * HD / KVW + cv * 4));
                    vx[u] = *reinterpret_cast<const uint4*>(pv + (int64_t(key) * HD / KVW + cv * 4));
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = base + u * kDecodeBlock, lr = idx / VPR, cv = idx % VPR;
                if (idx >= rows * VPR) continue;
                if constexpr (F16 && !KVH) {       // fp32 `present` in fp16 mode: converted once, here
                    const float4 kf = __builtin_bit_cast(float4, kx[u]), vf = __builtin_bit_cast(float4, vx[u]);
                    h4 kh, vh;
                    kh[0] = _Float16(kf.x); kh[1] = _Float16(kf.y); kh[2] = _Float16(kf.z); kh[3] = _Float16(kf.w);
                    vh[0] = _Float16(vf.x); vh[1] = _Float16(vf.y); vh[2] = _Float16(vf.z); vh[3] = _Float16(vf.w);
                    *reinterpret_cast<h4*>(Ks + lr * RS + cv * 4) = kh;
                    *reinterpret_cast<h4*>(Vs + lr * RS + cv * 4) = vh;
                } else {
                    *reinterpret_cast<uint4*>(Ks + lr * RS + cv * V) = kx[u];
                    *reinterpret_cast<uint4*>(Vs + lr * RS + cv * V) = vx[u];
                }
            }
        }
        if (int(threadIdx.x) < rows) {
            const int j = int(threadIdx.x);
            Bs[j] = c0 + j < (INPLACE ? P : Lk) ? fmaxf(key_bias(a, n, c0 + j) * kLog2e, -kFltMax) : 0.f;      // (a padded key is causally hidden from every row)
        }
        __syncthreads();
        const int cend = c0 + rows < wave_end ? c0 + rows : wave_end;
        for (int key0 = c0 + kw * 32; key0 < cend; key0 += KW * 32) {      // this key wave's tiles of the chunk
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
#pragma unroll
                for (int j = 0; j < NA; ++j) o[j][r] *= alpha;
            }
            lsum = fmaf(lsum, alpha, ps);              // this lane half's share of the row sum
            if constexpr (F16) {
#pragma unroll
                for (int st = 0; st < 2; ++st) {
                    h8 pb;
#pragma unroll
                    for (int j = 0; j < 8; ++j) pb[j] = _Float16(s[8 * st + j]);
#pragma unroll
                    for (int jo = 0; jo < NA; ++jo) {
                        h8 va;
#pragma unroll
                        for (int j = 0; j < 8; ++j) va[j] = Vt[(16 * st + 8 * (j >> 2) + 4 * hf + (j & 3)) * RS + 32 * jo + col];
                        o[jo] = __builtin_amdgcn_mfma_f32_32x32x16_f16(va, pb, o[jo], 0, 0, 0);
                    }
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int kt = (r & 3) + 8 * (r >> 2) + 4 * hf;
#pragma unroll
                    for (int jo = 0; jo < NA; ++jo) o[jo] = __builtin_amdgcn_mfma_f32_32x32x2f32(float(Vt[kt * RS + 32 * jo + col]), s[r], o[jo], 0, 0, 0);
                }
            }
        }
        __syncthreads();                           // the next chunk (or the partials below) overwrites the rows
    }

    // the key waves of a row wave meet: lane by lane (a lane of key wave w holds the same query row and the same output columns as that lane of key
    // wave 0), in key-wave order.  m is the same in both lane halves, l is still the lane half's share
    if constexpr (KW > 1) {
        float* Ms = reinterpret_cast<float*>(extend_wide_smem) + size_t(rw) * (KW - 1) * MS + lane;
        if (kw != 0) {
            float* mine = Ms + size_t(kw - 1) * MS;
            mine[0] = m;
            mine[64] = lsum;
#pragma unroll
            for (int j = 0; j < NA; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) mine[(2 + 16 * j + r) * 64] = o[j][r];
        }
        __syncthreads();
        if (kw == 0) {
            for (int w = 1; w < KW; ++w) {
                const float* theirs = Ms + size_t(w - 1) * MS;
                const float m2 = theirs[0], mn = fmaxf(m, m2);
                const float wa = fast_exp2(m - mn), wb = fast_exp2(m2 - mn);      // (-FLT_MAX next to a real maximum: exactly 0)
                m = mn;
                lsum = fmaf(lsum, wa, theirs[64] * wb);
#pragma unroll
                for (int j = 0; j < NA; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[j][r] = fmaf(o[j][r], wa, theirs[(2 + 16 * j + r) * 64] * wb);
            }
        }
    }

    lsum += __shfl_xor(lsum, 32, 64);
    if constexpr (INPLACE) if (lim < 0 && sp == 0) lsum = 1.f;      // nothing visible at all: zeros, finite
    if (kw != 0 || q0 + col >= R) return;          // behind the last barrier
    // registers 4 j ... 4 j + 3 of o[jo] are the output columns 32 jo + 8 j + 4 hf ... of this lane's query row
    if (S == 1) {
        T* orow = reinterpret_cast<T*>(a.out.p) + n * a.out.sn + int64_t(tok) * a.out.sw + h * HD;
        const float inv = 1.f / lsum;
#pragma unroll
        for (int jo = 0; jo < NA; ++jo)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e0 = 32 * jo + 8 * j + 4 * hf;
                if constexpr (F16) {
                    h4 x;
#pragma unroll
                    for (int t = 0; t < 4; ++t) x[t] = _Float16(o[jo][4 * j + t] * inv);
                    *reinterpret_cast<h4*>(orow + e0) = x;
                } else {
                    *reinterpret_cast<float4*>(orow + e0) = make_float4(o[jo][4 * j] * inv, o[jo][4 * j + 1] * inv, o[jo][4 * j + 2] * inv, o[jo][4 * j + 3] * inv);
                }
            }
        return;
    }
    float* rec = a.workspace + (((n * a.heads + h) * Lq + tok) * S + sp) * int64_t(HD + 2);
    if (hf == 0) { rec[0] = m; rec[1] = lsum; }
#pragma unroll
    for (int jo = 0; jo < NA; ++jo)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e0 = 32 * jo + 8 * j + 4 * hf;
            *reinterpret_cast<float2*>(rec + 2 + e0) = make_float2(o[jo][4 * j], o[jo][4 * j + 1]);
            *reinterpret_cast<float2*>(rec + 2 + e0 + 2) = make_float2(o[jo][4 * j + 2], o[jo][4 * j + 3]);
        }
}

template <typename T, int KW>
hipError_t launch_wide(const DecodeArgs& a, hipStream_t stream) {
    constexpr bool F16 = sizeof(T) == 2;
    constexpr int RB = 128 / KW;
    const int64_t rblocks = (int64_t(a.heads / a.kv_heads) * a.new_len + RB - 1) / RB;
    const dim3 grid(unsigned(rblocks * a.splits), unsigned(a.kv_heads), unsigned(a.in.n));
    const size_t lds = size_t(ExtendWideLdsBytes(128, F16));
    if constexpr (F16) {
        if (a.cache_f16) {
            attention_extend_wide_kernel<T, 128, KW, true, true><<<grid, dim3(kDecodeBlock), lds, stream>>>(a);
            return hipGetLastError();
        }
    }
    if (a.cache_rows > 0) attention_extend_wide_kernel<T, 128, KW, true><<<grid, dim3(kDecodeBlock), lds, stream>>>(a);
    else attention_extend_wide_kernel<T, 128, KW><<<grid, dim3(kDecodeBlock), lds, stream>>>(a);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_wide_kw(const DecodeArgs& a, hipStream_t stream) {
    const int kw = ExtendWideKeyWaves(int64_t(a.heads / a.kv_heads) * a.new_len);
    return kw == 4 ? launch_wide<T, 4>(a, stream) : (kw == 2 ? launch_wide<T, 2>(a, stream) : launch_wide<T, 1>(a, stream));
}

template <typename T, int KW>
hipError_t init_wide() {
    constexpr bool F16 = sizeof(T) == 2;           // (the half-cache form serves half models only)
    const void* const kernels[] = {
        reinterpret_cast<const void*>(&attention_extend_wide_kernel<T, 128, KW>),
        reinterpret_cast<const void*>(&attention_extend_wide_kernel<T, 128, KW, true>),
        reinterpret_cast<const void*>(&attention_extend_wide_kernel<T, 128, KW, true, F16>),
    };
    for (const void* k : kernels)
        if (const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, int(kAttnLdsBudget)); e != hipSuccess) return e;
    return hipSuccess;
}

}  // namespace

hipError_t LaunchExtendWide(const DecodeArgs& a, hipStream_t stream) {
    if (a.head_dim != 128 || (a.cache_f16 && !a.in.f16)) return hipErrorInvalidValue;
    return a.in.f16 ? launch_wide_kw<_Float16>(a, stream) : launch_wide_kw<float>(a, stream);
}

hipError_t InitKernelsExtendWide() {
    hipError_t e = init_wide<float, 1>();
    if (e == hipSuccess) e = init_wide<float, 2>();
    if (e == hipSuccess) e = init_wide<float, 4>();
    if (e == hipSuccess) e = init_wide<_Float16, 1>();
    if (e == hipSuccess) e = init_wide<_Float16, 2>();
    if (e == hipSuccess) e = init_wide<_Float16, 4>();
    return e;
}

}  // namespace ie
