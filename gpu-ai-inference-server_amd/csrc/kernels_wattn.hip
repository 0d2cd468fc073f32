// Attention inside (shifted) windows of a channels-last map, and patch merging (Swin-class graphs) on gfx950.
//
//   out[pixel(i), h * hd + e] = sum_j softmax_j(scale * q_i . k_j + bias[h][i][j] + mask[window][i][j]) * v[j, e]
//
// The operand is the qkv map the qkv Linear wrote ([N, H, W, 3 D]: a pixel's row holds q | k | v, head h at columns h * hd); the result goes straight
// into the map the projection Linear reads.  torch.roll, the window partition, its reverse and the roll back are index arithmetic: token t of
// window (wy, wx) is the pixel ((wy wh + t / ww + sh) mod H, (wx ww + t % ww + sw) mod W) of the unrolled map, for the loads and for the stores.
// Scores, softmax statistics and accumulation are fp32 in both element types; the softmax subtracts the row maximum; no score reaches memory.
// Tables (kernels.h WinAttnArgs): [.][Lp][Lp] with the query index fastest, -inf in the bias rows of the padded keys.
//
//   window_attention_generic_kernel      tile 0: one wave per (image, window, head, query row), as attention_generic_kernel.  Any window, shift, hd,
//                                        pitch, offset, float or half.  The fallback and the cross-check.
//   window_attention_mfma_kernel<T, 32>  tile 1: one wave per (image, window, head) problem, four problems per workgroup, heads fastest so the
//                                        waves of a workgroup read neighbouring columns of the same pixel rows.  Each wave gathers the K and V rows
//                                        of its window into its own LDS slice (rows past L zero, row stride hd + one 16-byte vector as in
//                                        kernels_attn.hip), then walks the one or two blocks of 32 queries.
//
// Tile 1 computes the scores swapped (S^T = K . Q^T) and feeds P^T to the second product from its registers, with the wave and in the operand orders
// of attn_mfma.h (Q, both products and the store are AttnWave's).  Softmax form: TWO-PASS over a whole row held in registers.  L <= 64 is at most two 32-key tiles = 32 score
// registers per lane, which fit beside Q (16) and O (16); the maximum is taken over the complete row before any exponential, so there is no
// running maximum, no rescale of O and sum, and half the exponentials of the online form on a second tile.  Padded keys carry -inf from the bias
// table (no compare in the kernel); padded queries are computed from the last row and never stored.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "attn_mfma.h"
#include "kernels.h"
#include "launch_util.h"

namespace ie {
namespace {

constexpr int kWinBlock = 256;
constexpr int kWinWaves = kWinBlock / 64;

// the map pixel (y, x) of token t of window (wy, wx)
__device__ __forceinline__ void tok_yx(const WinAttnArgs& a, int wy, int wx, int t, int& y, int& x) {
    const int ty = t / a.ww, tx = t - ty * a.ww;
    y = wy * a.wh + ty + a.sh;         // sh < wh <= H: one wrap at most
    x = wx * a.ww + tx + a.sw;
    if (y >= a.in.h) y -= a.in.h;
    if (x >= a.in.w) x -= a.in.w;
}

// the same for t < 64 without an integer division: inv_ww = 1 / ww; (t + 0.5) / ww is at least 0.5 / ww >= 1 / 128 away from every integer
__device__ __forceinline__ void tok_yx_fast(const WinAttnArgs& a, float inv_ww, int wy, int wx, int t, int& y, int& x) {
    const int ty = int((float(t) + 0.5f) * inv_ww), tx = t - ty * a.ww;
    y = wy * a.wh + ty + a.sh;
    x = wx * a.ww + tx + a.sw;
    if (y >= a.in.h) y -= a.in.h;
    if (x >= a.in.w) x -= a.in.w;
}

// rows = N * nW * heads * L query rows, one wave each
__global__ __launch_bounds__(kWinBlock) void window_attention_generic_kernel(const WinAttnArgs a, const int64_t rows) {
    const int lane = int(threadIdx.x) % 64;
    const int64_t row = int64_t(blockIdx.x) * kWinWaves + threadIdx.x / 64;
    if (row >= rows) return;                       // wave-uniform
    const int L = a.wh * a.ww, Lp = (L + 31) / 32 * 32, hd = a.head_dim, D = a.heads * hd;
    const int nww = a.in.w / a.ww, nW = (a.in.h / a.wh) * nww;
    const int i = int(row % L);
    const int h = int((row / L) % a.heads);
    const int win = int((row / (int64_t(L) * a.heads)) % nW);
    const int64_t n = row / (int64_t(L) * a.heads * nW);
    const int wy = win / nww, wx = win % nww;
    int qy, qx;
    tok_yx(a, wy, wx, i, qy, qx);
    const int64_t ib = n * a.in.sn + int64_t(h) * hd * a.in.sc;
    const int64_t qb = ib + int64_t(qy) * a.in.sh + int64_t(qx) * a.in.sw;
    const int64_t ob = n * a.out.sn + int64_t(qy) * a.out.sh + int64_t(qx) * a.out.sw + int64_t(h) * hd * a.out.sc;
    const float* bias = a.bias + int64_t(h) * Lp * Lp + i;
    const float* mask = a.mask ? a.mask + int64_t(win) * Lp * Lp + i : nullptr;
    auto key_base = [&](int j) {
        int y, x;
        tok_yx(a, wy, wx, j, y, x);
        return ib + int64_t(y) * a.in.sh + int64_t(x) * a.in.sw + int64_t(D) * a.in.sc;
    };
    auto score = [&](int j) {
        const int64_t kb = key_base(j);
        float s = 0.f;
        for (int e = 0; e < hd; ++e) s = fmaf(ld_any(a.in.p, a.in.f16, qb + int64_t(e) * a.in.sc), ld_any(a.in.p, a.in.f16, kb + int64_t(e) * a.in.sc), s);
        s = s * a.scale + bias[int64_t(j) * Lp];
        return mask ? s + mask[int64_t(j) * Lp] : s;
    };
    float m = -__builtin_huge_valf();
    for (int j = lane; j < L; j += 64) m = fmaxf(m, score(j));
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) m = fmaxf(m, __shfl_xor(m, x, 64));
    for (int e0 = 0; e0 < hd; e0 += 64) {
        const int e = e0 + lane;
        float l = 0.f, acc = 0.f;
        for (int j0 = 0; j0 < L; j0 += 64) {
            const int j = j0 + lane;
            const float p = j < L ? expf(score(j) - m) : 0.f;
            l += p;
            const int cnt = L - j0 < 64 ? L - j0 : 64;
            for (int t = 0; t < cnt; ++t) {
                const float pj = __shfl(p, t, 64);
                if (e < hd) acc = fmaf(pj, ld_any(a.in.p, a.in.f16, key_base(j0 + t) + int64_t(D + e) * a.in.sc), acc);
            }
        }
#pragma unroll
        for (int x = 32; x >= 1; x >>= 1) l += __shfl_xor(l, x, 64);
        if (e < hd) st_any(a.out.p, a.out.f16, ob + int64_t(e) * a.out.sc, acc / l);
    }
}

// dynamic LDS of the MFMA kernel: per wave the K and V rows of one window, Lp rows of hd + one vector
constexpr int64_t WinAttnLdsBytes(int64_t Lp, int hd, bool f16) { return kWinWaves * 2 * Lp * (int64_t(hd) * (f16 ? 2 : 4) + 16); }

// grid = ceil(problems / 4) workgroups, problem = ((n * nW + window) * heads + head); dynamic LDS = WinAttnLdsBytes(Lp, HD, half)
template <typename T, int HD>
__global__ __launch_bounds__(kWinBlock) void window_attention_mfma_kernel(const WinAttnArgs a, const int64_t problems) {
    constexpr int V = 16 / int(sizeof(T));         // elements per 16-byte vector
    constexpr int RS = HD + V;                     // LDS row stride in elements
    constexpr int HH = HD / 2;                     // head-dim elements one lane half supplies to QK^T
    constexpr int VPR = HD / V;                    // vectors per K / V row
    static_assert(HD == 32, "one 32-column output block per query");
    extern __shared__ __attribute__((aligned(16))) unsigned char wattn_smem[];
    const int L = a.wh * a.ww, Lp = (L + 31) / 32 * 32, D = a.heads * HD;
    const int wave = int(threadIdx.x) / 64, lane = int(threadIdx.x) % 64, col = lane & 31, hf = lane >> 5;
    T* Ks = reinterpret_cast<T*>(wattn_smem) + size_t(wave) * 2 * Lp * RS;
    T* Vs = Ks + size_t(Lp) * RS;
    const int64_t prob = int64_t(blockIdx.x) * kWinWaves + wave;
    const bool live = prob < problems;             // wave-uniform; a dead wave only meets the barrier
    const int nww = a.in.w / a.ww, nW = (a.in.h / a.wh) * nww;
    const int h = int(prob % a.heads);
    const int win = int((prob / a.heads) % nW);
    const int64_t n = prob / (int64_t(a.heads) * nW);
    const int wy = win / nww, wx = win % nww;
    const T* base = reinterpret_cast<const T*>(a.in.p) + n * a.in.sn + h * HD;      // pixel (y, x): + y * sh + x * sw; q at + 0, k at + D, v at + 2 D

    const float inv_ww = 1.f / float(a.ww);
    if (live) {
        // all the window's loads are issued before the first LDS store: one memory latency per wave, not one per group of rows
        constexpr int RPI = 64 / VPR;              // rows one pass of the wave covers
        constexpr int NIT = kWinAttnMaxTokens / RPI;
        const int cv = lane % VPR;
        uint4 kv[NIT], vv[NIT];
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int row = it * RPI + lane / VPR;
            kv[it] = make_uint4(0u, 0u, 0u, 0u);                                          // rows past L: zeros (their probability is exp2(-inf) = 0)
            vv[it] = kv[it];
            if (row < L) {
                int y, x;
                tok_yx_fast(a, inv_ww, wy, wx, row, y, x);
                const T* r = base + int64_t(y) * a.in.sh + int64_t(x) * a.in.sw + cv * V;
                kv[it] = *reinterpret_cast<const uint4*>(r + D);
                vv[it] = *reinterpret_cast<const uint4*>(r + 2 * D);
            }
        }
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int row = it * RPI + lane / VPR;
            if (row < Lp) {
                *reinterpret_cast<uint4*>(Ks + row * RS + cv * V) = kv[it];
                *reinterpret_cast<uint4*>(Vs + row * RS + cv * V) = vv[it];
            }
        }
    }
    __syncthreads();
    if (!live) return;

    const float sl2 = a.scale * kLog2e;            // scores in units of log2: exp(x) = exp2(x * log2 e)
    const float* bias = a.bias + int64_t(h) * Lp * Lp;
    const float* mask = a.mask ? a.mask + int64_t(win) * Lp * Lp : nullptr;
    const bool two = Lp > 32;                      // a second key tile (wave-uniform)

    for (int q0 = 0; q0 < L; q0 += 32) {
        const int qi = q0 + col < L ? q0 + col : L - 1;
        int qy, qx;
        tok_yx_fast(a, inv_ww, wy, wx, qi, qy, qx);
        const T* qrow = base + int64_t(qy) * a.in.sh + int64_t(qx) * a.in.sw + hf * HH;
        AttnWave<T, HD> w;                         // this lane's half of its Q row, one accumulator block; no running maximum: w.m is not used
        w.init(qrow, 0.f);

        // pass 1: the whole score row (one or two 32-key tiles), bias and mask added in registers, then its maximum
        f32x16 s[2];                               // (s[1] stays unset without a second key tile: both passes skip it)
        float mx = -__builtin_huge_valf();
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
            if (kt == 1 && !two) continue;
            // the tile's 16 bias (and mask) values per lane, requested ahead of the MFMAs that hide their latency; the 32 lanes of a half read 32
            // consecutive floats per key
            float bm[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) bm[r] = bias[(32 * kt + (r & 3) + 8 * (r >> 2) + 4 * hf) * Lp + q0 + col];      // -inf on a padded key
            if (mask) {
#pragma unroll
                for (int r = 0; r < 16; ++r) bm[r] += mask[(32 * kt + (r & 3) + 8 * (r >> 2) + 4 * hf) * Lp + q0 + col];
            }
            s[kt] = w.template qk_tile<RS>(Ks + 32 * kt * RS, col, hf);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s[kt][r] = fmaf(s[kt][r], sl2, bm[r] * kLog2e);
                mx = fmaxf(mx, s[kt][r]);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));      // finite: key 0 is real

        // pass 2: probabilities, their sum, and O^T += V^T . P^T from the registers the probabilities are in
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
            if (kt == 1 && !two) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s[kt][r] = fast_exp2(s[kt][r] - mx);
                w.lsum += s[kt][r];
            }
            w.template pv_tile<RS>(Vs + 32 * kt * RS, s[kt], col, hf);
        }
        w.lsum += __shfl_xor(w.lsum, 32, 64);
        if (q0 + col >= L) continue;               // a padded query: no exchange follows in this iteration
        w.store(reinterpret_cast<T*>(a.out.p) + n * a.out.sn + int64_t(qy) * a.out.sh + int64_t(qx) * a.out.sw + h * HD, hf);
    }
}

template <typename T, int HD>
hipError_t launch_mfma(const WinAttnArgs& a, hipStream_t stream) {
    const int64_t problems = int64_t(a.in.n) * (a.in.h / a.wh) * (a.in.w / a.ww) * a.heads;
    const int64_t blocks = (problems + kWinWaves - 1) / kWinWaves;
    if (blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
    const size_t lds = size_t(WinAttnLdsBytes(WinAttnPaddedTokens(int64_t(a.wh) * a.ww), HD, sizeof(T) == 2));
    window_attention_mfma_kernel<T, HD><<<dim3(unsigned(blocks)), dim3(kWinBlock), lds, stream>>>(a, problems);
    return hipGetLastError();
}

constexpr int kMergeBlock = 256;

// per: V-element groups per input pixel (C / V); total = N * OH * OW * 4 * per.  V == 1 reads and writes either element type
template <typename T, int V>
__global__ __launch_bounds__(kMergeBlock) void patch_merge_kernel(const PatchMergeArgs a, const int per, const int64_t total) {
    const int64_t g = int64_t(blockIdx.x) * kMergeBlock + threadIdx.x;
    if (g >= total) return;
    const int c = int(g % per) * V;
    int64_t r = g / per;
    const int k = int(r % 4);
    r /= 4;
    const int x = int(r % a.out.w);
    r /= a.out.w;
    const int y = int(r % a.out.h);
    const int64_t n = r / a.out.h;
    const int64_t si = n * a.in.sn + int64_t(2 * y + (k & 1)) * a.in.sh + int64_t(2 * x + (k >> 1)) * a.in.sw + int64_t(c) * a.in.sc;
    const int64_t di = n * a.out.sn + int64_t(y) * a.out.sh + int64_t(x) * a.out.sw + (int64_t(k) * a.in.c + c) * a.out.sc;
    if constexpr (V > 1) *reinterpret_cast<uint4*>(reinterpret_cast<T*>(a.out.p) + di) = *reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(a.in.p) + si);
    else st_any(a.out.p, a.out.f16, di, ld_any(a.in.p, a.in.f16, si));
}

template <typename T, int V>
hipError_t launch_merge(const PatchMergeArgs& a, hipStream_t stream) {
    const int per = a.in.c / V;
    const int64_t total = int64_t(a.out.n) * a.out.h * a.out.w * 4 * per;
    const int64_t blocks = (total + kMergeBlock - 1) / kMergeBlock;
    if (blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
    if (total == 0) return hipSuccess;
    patch_merge_kernel<T, V><<<dim3(unsigned(blocks)), dim3(kMergeBlock), 0, stream>>>(a, per, total);
    return hipGetLastError();
}

}  // namespace

bool WindowAttentionEligible(const WinAttnArgs& a, int tile) {
    if (tile < 0 || tile >= kNumWinAttnTiles || !a.in.p || !a.out.p || !a.bias || a.heads < 1 || a.head_dim < 1 || a.wh < 1 || a.ww < 1) return false;
    const int64_t D = int64_t(a.heads) * a.head_dim;
    if (a.in.f8 || a.out.f8 || a.in.c != 3 * D || a.out.c != D || a.in.n != a.out.n || a.in.h != a.out.h || a.in.w != a.out.w || a.in.h < 1 || a.in.w < 1) return false;
    if (a.in.h % a.wh || a.in.w % a.ww || a.sh < 0 || a.sw < 0 || a.sh >= a.wh || a.sw >= a.ww) return false;      // (every pixel index the kernels form stays inside the map)
    if (tile == 0) return true;
    const int V = a.out.f16 ? 8 : 4;
    // (the offsets are in the base pointers: their alignment stands for the offset condition)
    // stricter than VecViewOk alone: RowsDense is the layer-norm tiles' condition, taken over with them; the MFMA kernel addresses by sn / sh / sw and
    // would run without it, but the tile keeps accepting exactly the views it was tested on
    return a.in.f16 == a.out.f16 && VecViewOk(a.in, V) && RowsDense(a.in) && VecViewOk(a.out, V) && RowsDense(a.out) &&
           WinAttnMfmaFits(int64_t(a.wh) * a.ww, a.head_dim, a.out.f16 != 0, a.in.c, a.in.sw, 0, a.out.c, a.out.sw, 0);
}

hipError_t LaunchWindowAttention(const WinAttnArgs& a, int tile, hipStream_t stream) {
    if (!WindowAttentionEligible(a, tile)) return hipErrorInvalidValue;
    if (a.in.n == 0) return hipSuccess;
    if (tile == 0) {
        const int64_t rows = int64_t(a.in.n) * a.in.h * a.in.w * a.heads;      // one per (pixel, head)
        const int64_t blocks = (rows + kWinWaves - 1) / kWinWaves;
        if (blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
        hipLaunchKernelGGL(window_attention_generic_kernel, dim3(unsigned(blocks)), dim3(kWinBlock), 0, stream, a, rows);
        return hipGetLastError();
    }
    return a.out.f16 ? launch_mfma<_Float16, 32>(a, stream) : launch_mfma<float, 32>(a, stream);
}

hipError_t InitKernelsWattn() {
    const int lds = int(WinAttnLdsBytes(kWinAttnMaxTokens, 32, false));
    hipError_t e;
    if ((e = hipFuncSetAttribute(reinterpret_cast<const void*>(&window_attention_mfma_kernel<float, 32>), hipFuncAttributeMaxDynamicSharedMemorySize, lds)) != hipSuccess) return e;
    if ((e = hipFuncSetAttribute(reinterpret_cast<const void*>(&window_attention_mfma_kernel<_Float16, 32>), hipFuncAttributeMaxDynamicSharedMemorySize, lds)) != hipSuccess) return e;
    return hipSuccess;
}

hipError_t LaunchPatchMerge(const PatchMergeArgs& a, hipStream_t stream) {
    if (!a.in.p || !a.out.p || a.in.f8 || a.out.f8 || a.in.c < 1 || a.in.h % 2 || a.in.w % 2 || a.out.h != a.in.h / 2 || a.out.w != a.in.w / 2 || a.out.c != 4 * a.in.c ||
        a.in.n != a.out.n)
        return hipErrorInvalidValue;
    const int V = a.out.f16 ? 8 : 4;
    const bool vec = a.in.sc == 1 && a.out.sc == 1 && PatchMergeVec(a.in.f16 != 0, a.out.f16 != 0, a.in.c, a.in.sw, 0, a.out.sw, 0) && a.in.sh % V == 0 && a.in.sn % V == 0 &&
                     a.out.sh % V == 0 && a.out.sn % V == 0 && Aligned16(a.in.p) && Aligned16(a.out.p);
    if (vec) return a.out.f16 ? launch_merge<_Float16, 8>(a, stream) : launch_merge<float, 4>(a, stream);
    return launch_merge<float, 1>(a, stream);
}

}  // namespace ie
