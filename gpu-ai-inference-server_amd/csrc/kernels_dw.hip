// Depthwise convolution (group == Cin == Cout; MobileNet-class graphs) on gfx950.
//
// Bandwidth-bound VALU work, no MFMA: a 3x3 depthwise conv does 9 MACs per output element against 8 bytes of traffic in fp32.
//
//   conv_dw_kernel<T, K, S, PX>   the fast path: NHWC, every lane owns one 16-byte channel vector (4 floats / 8 halfs) and a run of PX
//                                 output pixels along W.  Per filter row the lane loads the (PX - 1) * S + K input vectors its outputs
//                                 need ONCE and slides the K-tap window through registers, so an input element is loaded about kh times
//                                 per output row pass instead of kh * kw times.  The lane's folded weights, bias and prologue constants are
//                                 loaded once (9 x 16 B of weights for 3x3 fp32) and stay in registers while the lane walks pixel groups
//                                 grid-stride.  Consecutive lanes take consecutive channel vectors of one pixel: 16 B per lane, coalesced.
//                                 Accumulation is fp32 in both element types (float2 pairs: v_pk_fma_f32).
//   conv_dw_generic_kernel        one thread per output element: any k <= 7, any stride / padding / C, NCHW or NHWC input, mixed element
//                                 types (an fp16 plan's fp32 graph input).  Every depthwise conv the planner accepts runs on one of the two.
//
// Padding taps contribute 0 (explicit bounds): the prologue (folded pre-activation BN, ReLU, ReLU6's upper bound) applies to in-range taps only,
// as the ONNX graph pads the prologue's OUTPUT.  Epilogue: + bias (+ residual), ReLU, then the Clip bounds.
// Fused activations (sigmoid / hardsigmoid / SiLU / hardswish: MobileNetV3, EfficientNet) close the prologue (pre_act, after pre_hi) and the
// epilogue (act, after the clamp).  The fast kernel takes them only in its ACT instantiations, so the graphs without them run the same code as before.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "device_util.h"
#include "kernels.h"
#include "launch_util.h"

namespace ie {
namespace {

constexpr int kDwBlock = 256;

__device__ __forceinline__ bool finite_lo(float lo) { return lo > -__builtin_huge_valf(); }
__device__ __forceinline__ bool finite_hi(float hi) { return hi < __builtin_huge_valf(); }

// ApplyAct without control flow (the fast kernel's unrolled loops): g = hard ? clamp(a*x + b, 0, 1) : sigmoid(x), then x * g (silu / hardswish)
// or g; kind 0 = identity.  kind is uniform; both branches are selects.
__device__ __forceinline__ float act_sel(int kind, float a, float b, float x) {
    const bool hard = kind == 2 || kind == 4, mul = kind == 3 || kind == 4;
    const float h = fminf(fmaxf(fmaf(a, x, b), 0.f), 1.f);
    const float sg = 1.f / (1.f + __expf(-x));
    const float g = hard ? h : sg;
    const float y = mul ? x * g : g;
    return kind == 0 ? x : (kind == 5 ? fmaxf(x, 0.f) : y);
}

// groups = N * OH * ceil(OW / PX) pixel groups; the grid holds cvn * nslots lanes, lane (slot, cv) walks groups slot, slot + nslots, ...
template <typename T, int K, int S, int PX, bool ACT>
__global__ __launch_bounds__(kDwBlock) void conv_dw_kernel(const DwArgs a, const int cvn, const int owg, const int64_t groups, const int64_t nslots) {
    constexpr int V = 16 / int(sizeof(T));
    constexpr int KK = K * K;
    constexpr int NIN = (PX - 1) * S + K;         // input vectors one filter row of PX outputs touches
    constexpr bool WREG = V * KK <= 100;          // 5x5 halfs (200 floats) re-read their row of weights from L1 instead
    const int64_t t = int64_t(blockIdx.x) * kDwBlock + threadIdx.x;
    if (t >= int64_t(cvn) * nslots) return;
    const int cv = int(t % cvn);
    const int c0 = cv * V;
    const int64_t slot = t / cvn;

    // ---- per-lane constants: weights [V][KK] are contiguous in the blob (c0 * KK floats = a multiple of 16 B), bias, prologue ----
    const float* __restrict__ wg = a.w + int64_t(c0) * KK;
    float wr[WREG ? V * KK : 1];
    if constexpr (WREG) {
#pragma unroll
        for (int i = 0; i < V * KK / 4; ++i) {
            const float4 q = reinterpret_cast<const float4*>(wg)[i];
            wr[4 * i] = q.x; wr[4 * i + 1] = q.y; wr[4 * i + 2] = q.z; wr[4 * i + 3] = q.w;
        }
    }
    float bias[V], ps[V], pt[V];
#pragma unroll
    for (int v = 0; v < V; ++v) { bias[v] = 0.f; ps[v] = 1.f; pt[v] = 0.f; }
    if (a.bias) { load16<float>(a.bias + c0, bias); if constexpr (V == 8) load16<float>(a.bias + c0 + 4, bias + 4); }
    const bool pre = a.pre_scale != nullptr || (ACT && a.pre_act != 0);
    if (pre) {
        load16<float>(a.pre_scale + c0, ps); load16<float>(a.pre_shift + c0, pt);
        if constexpr (V == 8) { load16<float>(a.pre_scale + c0 + 4, ps + 4); load16<float>(a.pre_shift + c0 + 4, pt + 4); }
    }
    const bool pre_relu = a.pre_relu != 0, pre_clip = finite_hi(a.pre_hi);
    const float pre_hi = a.pre_hi;

    const T* __restrict__ in = reinterpret_cast<const T*>(a.in.p);
    T* __restrict__ out = reinterpret_cast<T*>(a.out.p);
    const T* __restrict__ res = reinterpret_cast<const T*>(a.res.p);
    const int OH = a.out.h, OW = a.out.w, H = a.in.h, W = a.in.w;

    for (int64_t g = slot; g < groups; g += nslots) {
        const int gx = int(g % owg);
        const int64_t r = g / owg;
        const int oy = int(r % OH);
        const int n = int(r / OH);
        const int ox0 = gx * PX;
        const int ix0 = ox0 * S - a.pl;
        f32x2 acc[PX][V / 2];
#pragma unroll
        for (int p = 0; p < PX; ++p)
#pragma unroll
            for (int v = 0; v < V / 2; ++v) acc[p][v] = f32x2{0.f, 0.f};
#pragma unroll
        for (int ky = 0; ky < K; ++ky) {
            const int iy = oy * S - a.pt + ky;
            if (iy < 0 || iy >= H) continue;
            const T* row = in + int64_t(n) * a.in.sn + int64_t(iy) * a.in.sh + c0;
            float x[NIN][V];
#pragma unroll
            for (int j = 0; j < NIN; ++j) {
                const int ix = ix0 + j;
                if (ix >= 0 && ix < W) {
                    load16<T>(row + int64_t(ix) * a.in.sw, x[j]);
                    if (pre) {
#pragma unroll
                        for (int v = 0; v < V; ++v) {
                            float y = x[j][v] * ps[v] + pt[v];
                            if (pre_relu) y = fmaxf(y, 0.f);
                            if (pre_clip) y = fminf(y, pre_hi);
                            if constexpr (ACT) y = act_sel(a.pre_act, a.pre_act_a, a.pre_act_b, y);
                            x[j][v] = y;
                        }
                    }
                } else {
#pragma unroll
                    for (int v = 0; v < V; ++v) x[j][v] = 0.f;
                }
            }
            float wrow[V * K];
#pragma unroll
            for (int v = 0; v < V; ++v)
#pragma unroll
                for (int kx = 0; kx < K; ++kx) {
                    if constexpr (WREG) wrow[v * K + kx] = wr[v * KK + ky * K + kx];
                    else wrow[v * K + kx] = wg[v * KK + ky * K + kx];
                }
#pragma unroll
            for (int p = 0; p < PX; ++p)
#pragma unroll
                for (int kx = 0; kx < K; ++kx)
#pragma unroll
                    for (int v = 0; v < V / 2; ++v) {
                        const f32x2 wv = {wrow[(2 * v) * K + kx], wrow[(2 * v + 1) * K + kx]};
                        const f32x2 xv = {x[p * S + kx][2 * v], x[p * S + kx][2 * v + 1]};
                        acc[p][v] = __builtin_elementwise_fma(wv, xv, acc[p][v]);
                    }
        }
#pragma unroll
        for (int p = 0; p < PX; ++p) {
            const int ox = ox0 + p;
            if (ox >= OW) break;
            float o[V], rv[V];
#pragma unroll
            for (int v = 0; v < V / 2; ++v) { o[2 * v] = acc[p][v].x + bias[2 * v]; o[2 * v + 1] = acc[p][v].y + bias[2 * v + 1]; }
            if (res) {
                load16<T>(res + int64_t(n) * a.res.sn + int64_t(oy) * a.res.sh + int64_t(ox) * a.res.sw + c0, rv);
#pragma unroll
                for (int v = 0; v < V; ++v) o[v] += rv[v];
            }
#pragma unroll
            for (int v = 0; v < V; ++v) {
                if (a.relu) o[v] = fmaxf(o[v], 0.f);
                if (finite_lo(a.lo)) o[v] = fmaxf(o[v], a.lo);
                if (finite_hi(a.hi)) o[v] = fminf(o[v], a.hi);
                if constexpr (ACT) o[v] = act_sel(a.act, a.act_a, a.act_b, o[v]);
            }
            store16<T>(out + int64_t(n) * a.out.sn + int64_t(oy) * a.out.sh + int64_t(ox) * a.out.sw + c0, o);
        }
    }
}

__global__ __launch_bounds__(kDwBlock) void conv_dw_generic_kernel(const DwArgs a, const int64_t total) {
    const int64_t idx = int64_t(blockIdx.x) * kDwBlock + threadIdx.x;
    if (idx >= total) return;
    const int C = a.out.c;
    const int c = int(idx % C);
    int64_t m = idx / C;
    const int ox = int(m % a.out.w); m /= a.out.w;
    const int oy = int(m % a.out.h);
    const int n = int(m / a.out.h);
    const float s = a.pre_scale ? a.pre_scale[c] : 1.f, sh = a.pre_scale ? a.pre_shift[c] : 0.f;
    const float* w = a.w + int64_t(c) * a.kh * a.kw;
    const int64_t base = int64_t(n) * a.in.sn + int64_t(c) * a.in.sc;
    float acc = 0.f;
    for (int ky = 0; ky < a.kh; ++ky) {
        const int iy = oy * a.sh - a.pt + ky;
        if (iy < 0 || iy >= a.in.h) continue;
        for (int kx = 0; kx < a.kw; ++kx) {
            const int ix = ox * a.sw - a.pl + kx;
            if (ix < 0 || ix >= a.in.w) continue;
            float x = ld_any(a.in.p, a.in.f16, base + int64_t(iy) * a.in.sh + int64_t(ix) * a.in.sw);
            if (a.pre_scale) {
                x = x * s + sh;
                if (a.pre_relu) x = fmaxf(x, 0.f);
                if (finite_hi(a.pre_hi)) x = fminf(x, a.pre_hi);
            }
            if (a.pre_act) x = ApplyAct(a.pre_act, a.pre_act_a, a.pre_act_b, x);
            acc = fmaf(w[ky * a.kw + kx], x, acc);
        }
    }
    float o = acc + (a.bias ? a.bias[c] : 0.f);
    if (a.res.p) o += ld_any(a.res.p, a.res.f16, int64_t(n) * a.res.sn + int64_t(oy) * a.res.sh + int64_t(ox) * a.res.sw + int64_t(c) * a.res.sc);
    if (a.relu) o = fmaxf(o, 0.f);
    if (finite_lo(a.lo)) o = fmaxf(o, a.lo);
    if (finite_hi(a.hi)) o = fminf(o, a.hi);
    if (a.act) o = ApplyAct(a.act, a.act_a, a.act_b, o);
    const int64_t oi = int64_t(n) * a.out.sn + int64_t(oy) * a.out.sh + int64_t(ox) * a.out.sw + c;
    if (a.out.f16) reinterpret_cast<_Float16*>(a.out.p)[oi] = _Float16(o);
    else a.out.p[oi] = o;
}

constexpr int kDwPx[kNumConvDwTiles] = {1, 1, 2, 4};      // output pixels per lane of each tile (tile 0: the generic kernel)

template <typename T, int K, int S, bool ACT>
hipError_t launch_fast(const DwArgs& a, int px, hipStream_t stream) {
    constexpr int V = 16 / int(sizeof(T));
    px = DwLanePixels(px, V == 8, K, S, ACT);
    const int cvn = a.out.c / V;
    const int owg = (a.out.w + px - 1) / px;
    const int64_t groups = int64_t(a.out.n) * a.out.h * owg;
    // lanes: every channel vector of up to ~2048 lanes per CU x 256 CUs worth of pixel groups; the rest is walked grid-stride (the
    // lane's weights stay in registers)
    const int64_t nslots = std::max<int64_t>(1, std::min<int64_t>(groups, (int64_t(256) * 2048 + cvn - 1) / cvn));
    const int64_t blocks = (int64_t(cvn) * nslots + kDwBlock - 1) / kDwBlock;
    if (blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
    const dim3 grid = dim3(unsigned(blocks)), block = dim3(kDwBlock);
    constexpr bool kPx2 = DwLanePixels(2, V == 8, K, S, ACT) == 2, kPx4 = DwLanePixels(4, V == 8, K, S, ACT) == 4;
    if (px == 1) conv_dw_kernel<T, K, S, 1, ACT><<<grid, block, 0, stream>>>(a, cvn, owg, groups, nslots);
    else if constexpr (!kPx2) return hipErrorInvalidValue;
    else if (px == 2) conv_dw_kernel<T, K, S, 2, ACT><<<grid, block, 0, stream>>>(a, cvn, owg, groups, nslots);
    else if constexpr (kPx4) conv_dw_kernel<T, K, S, 4, ACT><<<grid, block, 0, stream>>>(a, cvn, owg, groups, nslots);
    return hipGetLastError();
}

template <typename T, bool ACT>
hipError_t launch_fast_a(const DwArgs& a, int px, hipStream_t stream) {
    if (a.kh == 3) return a.sh == 1 ? launch_fast<T, 3, 1, ACT>(a, px, stream) : launch_fast<T, 3, 2, ACT>(a, px, stream);
    return a.sh == 1 ? launch_fast<T, 5, 1, ACT>(a, px, stream) : launch_fast<T, 5, 2, ACT>(a, px, stream);
}
template <typename T>
hipError_t launch_fast_t(const DwArgs& a, int px, hipStream_t stream) {
    return a.act || a.pre_act ? launch_fast_a<T, true>(a, px, stream) : launch_fast_a<T, false>(a, px, stream);
}

}  // namespace

bool ConvDwEligible(const DwArgs& a, int tile) {
    if (tile < 0 || tile >= kNumConvDwTiles || !a.w || !a.in.p || !a.out.p) return false;
    if (a.in.f8 || a.out.f8 || a.res.f8 || a.in.c != a.out.c || a.out.sc != 1 || a.kh < 1 || a.kw < 1 || a.kh > 7 || a.kw > 7) return false;
    if (a.pre_scale && !a.pre_shift) return false;
    if (tile == 0) return true;
    if (a.act > 5 || a.pre_act > 5) return false;      // act_sel knows the sigmoid family and ReLU: a fused GELU runs on the generic kernel
    const int V = a.out.f16 ? 8 : 4;
    return a.kh == a.kw && (a.kh == 3 || a.kh == 5) && a.sh == a.sw && (a.sh == 1 || a.sh == 2) && a.in.f16 == a.out.f16 && VecViewOk(a.in, V) &&
           VecViewOk(a.out, V) && (!a.res.p || (a.res.f16 == a.out.f16 && VecViewOk(a.res, V))) && Aligned16(a.w) && (!a.bias || Aligned16(a.bias)) &&
           (!a.pre_scale || (Aligned16(a.pre_scale) && Aligned16(a.pre_shift)));
}

hipError_t LaunchConvDw(const DwArgs& a, int tile, hipStream_t stream) {
    if (!ConvDwEligible(a, tile)) return hipErrorInvalidValue;
    if (int64_t(a.out.n) * a.out.h * a.out.w * a.out.c == 0) return hipSuccess;
    if (tile == 0) {
        const int64_t total = int64_t(a.out.n) * a.out.h * a.out.w * a.out.c;
        const int64_t blocks = (total + kDwBlock - 1) / kDwBlock;
        if (blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
        hipLaunchKernelGGL(conv_dw_generic_kernel, dim3(unsigned(blocks)), dim3(kDwBlock), 0, stream, a, total);
        return hipGetLastError();
    }
    return a.out.f16 ? launch_fast_t<_Float16>(a, kDwPx[tile], stream) : launch_fast_t<float>(a, kDwPx[tile], stream);
}

}  // namespace ie
