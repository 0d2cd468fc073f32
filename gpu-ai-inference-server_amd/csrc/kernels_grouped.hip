// Grouped convolution (1 < group, not depthwise: ResNeXt, RegNet) on gfx950.
//
//   conv_grouped_kernel<T, CPG, OPB, GPB, PX>   the fast path: NHWC.  A wave owns one block of OCB = OPB * GPB output channels (GPB whole groups,
//                                 or a slice of one group) for 64 * PX output pixels; lane l takes pixels l, l + 64, ...  The block's weights are
//                                 the same for every lane, so they are scalar loads that feed the VALU straight from SGPRs; every lane loads
//                                 the ICB = CPG * GPB input channels of its groups at each tap in 16-byte vectors and multiplies them into
//                                 OCB fp32 accumulators per pixel (fp32: fma; fp16: v_dot2_f32_f16 on channel pairs against the half mirror of
//                                 the weights).  Consecutive waves of a workgroup take consecutive channel blocks of the same pixels, so a
//                                 pixel's channels are read by one CU.  No LDS, no atomics: the sum order is fixed (taps, then channels).
//   conv_grouped_generic_kernel   one thread per output element: any group, k <= 7, any stride / padding / channel count, NCHW or NHWC input,
//                                 mixed element types (an fp16 plan's fp32 graph input).  Every grouped conv the planner accepts runs on it.
//
// Padding taps contribute 0; the prologue (folded pre-activation BN, ReLU, bound, activation) applies to in-range taps only.  Epilogue: + bias
// (+ residual), ReLU, Clip bounds, activation: the depthwise kernels' order (kernels_dw.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "device_util.h"
#include "kernels.h"
#include "launch_util.h"

namespace ie {
namespace {

constexpr int kGrpBlock = 256;     // 4 waves

// GELU: the activation codes above 5 (kernels.h ApplyAct) are compiled in; the fast kernel leaves them out (ConvGroupedEligible keeps such steps off it)
template <bool GELU>
__device__ __forceinline__ float prologue(const GroupedArgs& a, int c, float x) {
    if (a.pre_scale) {
        x = x * a.pre_scale[c] + a.pre_shift[c];
        if (a.pre_relu) x = fmaxf(x, 0.f);
        if (a.pre_hi < __builtin_huge_valf()) x = fminf(x, a.pre_hi);
    }
    if (a.pre_act) x = GELU ? ApplyAct(a.pre_act, a.pre_act_a, a.pre_act_b, x) : ApplyActBasic(a.pre_act, a.pre_act_a, a.pre_act_b, x);
    return x;
}

template <bool GELU>
__device__ __forceinline__ float epilogue(const GroupedArgs& a, float o) {
    if (a.relu) o = fmaxf(o, 0.f);
    if (a.lo > -__builtin_huge_valf()) o = fmaxf(o, a.lo);
    if (a.hi < __builtin_huge_valf()) o = fminf(o, a.hi);
    if (a.act) o = GELU ? ApplyAct(a.act, a.act_a, a.act_b, o) : ApplyActBasic(a.act, a.act_a, a.act_b, o);
    return o;
}

// nb channel blocks x ptiles pixel tiles of 64 * PX pixels; wave w of the grid takes block w % nb of tile w / nb
template <typename T, int CPG, int OPB, int GPB, int PX>
__global__ __launch_bounds__(kGrpBlock) void conv_grouped_kernel(const GroupedArgs a, const int nb, const int64_t waves, const int opg) {
    constexpr int V = 16 / int(sizeof(T));
    constexpr int OCB = OPB * GPB, ICB = CPG * GPB;
    constexpr bool DOT = sizeof(T) == 2 && CPG % 2 == 0;      // fp16 channel pairs on v_dot2_f32_f16
    constexpr int XR = DOT ? ICB / 2 : ICB;                   // input registers per pixel
    const int64_t wave = int64_t(blockIdx.x) * (kGrpBlock / 64) + __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6);
    if (wave >= waves) return;
    const int lane = int(threadIdx.x) & 63;
    const int cb = __builtin_amdgcn_readfirstlane(int(wave % nb));
    const int64_t pt = wave / nb;
    const int o0 = cb * OCB;
    const int i0 = (o0 / opg) * CPG;                          // GPB > 1: opg == OPB, the block's groups are consecutive
    const int OH = a.out.h, OW = a.out.w, H = a.in.h, W = a.in.w;
    const int64_t M = int64_t(a.out.n) * OH * OW;

    const T* __restrict__ in = reinterpret_cast<const T*>(a.in.p);
    T* __restrict__ out = reinterpret_cast<T*>(a.out.p);
    const T* __restrict__ res = reinterpret_cast<const T*>(a.res.p);

    int pn[PX], py[PX], px[PX];
    bool pv[PX];
#pragma unroll
    for (int p = 0; p < PX; ++p) {
        const int64_t m = pt * (64 * PX) + p * 64 + lane;
        pv[p] = m < M;
        const int64_t mm = pv[p] ? m : 0;
        px[p] = int(mm % OW);
        py[p] = int((mm / OW) % OH);
        pn[p] = int(mm / (int64_t(OW) * OH));
    }
    float acc[PX][OCB];
#pragma unroll
    for (int p = 0; p < PX; ++p)
#pragma unroll
        for (int j = 0; j < OCB; ++j) acc[p][j] = 0.f;
    const bool pre = a.pre_scale != nullptr || a.pre_act != 0;
    const int KK = a.kh * a.kw;

    for (int ky = 0; ky < a.kh; ++ky) {
        for (int kx = 0; kx < a.kw; ++kx) {
            const int tap = ky * a.kw + kx;
            float xf[DOT ? 1 : PX][DOT ? 1 : XR];
            h2 xh[DOT ? PX : 1][DOT ? XR : 1];
#pragma unroll
            for (int p = 0; p < PX; ++p) {
                const int iy = py[p] * a.sh - a.pt + ky, ix = px[p] * a.sw - a.pl + kx;
                float v[ICB];
                if (pv[p] && iy >= 0 && iy < H && ix >= 0 && ix < W) {
                    const T* src = in + int64_t(pn[p]) * a.in.sn + int64_t(iy) * a.in.sh + int64_t(ix) * a.in.sw + i0;
#pragma unroll
                    for (int q = 0; q < ICB / V; ++q) load16(src + q * V, v + q * V);
                    if (pre) {
#pragma unroll
                        for (int c = 0; c < ICB; ++c) v[c] = prologue<false>(a, i0 + c, v[c]);
                    }
                } else {
#pragma unroll
                    for (int c = 0; c < ICB; ++c) v[c] = 0.f;
                }
                if constexpr (DOT) {
#pragma unroll
                    for (int c = 0; c < XR; ++c) xh[p][c] = h2{_Float16(v[2 * c]), _Float16(v[2 * c + 1])};
                } else {
#pragma unroll
                    for (int c = 0; c < XR; ++c) xf[p][c] = v[c];
                }
            }
            // output j of the block (group j / OPB of the block) reads the block's input channels [(j / OPB) * CPG, + CPG)
#pragma unroll
            for (int j = 0; j < OCB; ++j) {
                const int64_t wrow = (int64_t(o0 + j) * KK + tap) * CPG;
                if constexpr (DOT) {
                    const h2* wj = reinterpret_cast<const h2*>(static_cast<const _Float16*>(a.w16) + wrow);
#pragma unroll
                    for (int c = 0; c < CPG / 2; ++c) {
                        const h2 w2 = wj[c];
#pragma unroll
                        for (int p = 0; p < PX; ++p) acc[p][j] = __builtin_amdgcn_fdot2(xh[p][(j / OPB) * (CPG / 2) + c], w2, acc[p][j], false);
                    }
                } else {
                    const float* wj = a.w + wrow;
#pragma unroll
                    for (int c = 0; c < CPG; ++c) {
                        const float wv = wj[c];
#pragma unroll
                        for (int p = 0; p < PX; ++p) acc[p][j] = fmaf(xf[p][(j / OPB) * CPG + c], wv, acc[p][j]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int p = 0; p < PX; ++p) {
        if (!pv[p]) continue;
        float o[OCB];
#pragma unroll
        for (int j = 0; j < OCB; ++j) o[j] = acc[p][j] + (a.bias ? a.bias[o0 + j] : 0.f);
        if (res) {
            const T* r = res + int64_t(pn[p]) * a.res.sn + int64_t(py[p]) * a.res.sh + int64_t(px[p]) * a.res.sw + o0;
            float rv[OCB];
#pragma unroll
            for (int q = 0; q < OCB / V; ++q) load16(r + q * V, rv + q * V);
#pragma unroll
            for (int j = 0; j < OCB; ++j) o[j] += rv[j];
        }
#pragma unroll
        for (int j = 0; j < OCB; ++j) o[j] = epilogue<false>(a, o[j]);
        T* dst = out + int64_t(pn[p]) * a.out.sn + int64_t(py[p]) * a.out.sh + int64_t(px[p]) * a.out.sw + o0;
#pragma unroll
        for (int q = 0; q < OCB / V; ++q) store16(dst + q * V, o + q * V);
    }
}

__global__ __launch_bounds__(kGrpBlock) void conv_grouped_generic_kernel(const GroupedArgs a, const int64_t total) {
    const int64_t idx = int64_t(blockIdx.x) * kGrpBlock + threadIdx.x;
    if (idx >= total) return;
    const int C = a.out.c;
    const int o = int(idx % C);
    int64_t m = idx / C;
    const int ox = int(m % a.out.w); m /= a.out.w;
    const int oy = int(m % a.out.h);
    const int n = int(m / a.out.h);
    const int cpg = a.in.c / a.groups, opg = C / a.groups;
    const int c0 = (o / opg) * cpg;
    const float* w = a.w + int64_t(o) * a.kh * a.kw * cpg;
    const int64_t base = int64_t(n) * a.in.sn;
    float acc = 0.f;
    for (int ky = 0; ky < a.kh; ++ky) {
        const int iy = oy * a.sh - a.pt + ky;
        if (iy < 0 || iy >= a.in.h) continue;
        for (int kx = 0; kx < a.kw; ++kx) {
            const int ix = ox * a.sw - a.pl + kx;
            if (ix < 0 || ix >= a.in.w) continue;
            const int64_t px = base + int64_t(iy) * a.in.sh + int64_t(ix) * a.in.sw;
            const float* wt = w + (ky * a.kw + kx) * cpg;
            for (int c = 0; c < cpg; ++c)
                acc = fmaf(wt[c], prologue<true>(a, c0 + c, ld_any(a.in.p, a.in.f16, px + int64_t(c0 + c) * a.in.sc)), acc);
        }
    }
    float v = acc + (a.bias ? a.bias[o] : 0.f);
    if (a.res.p) v += ld_any(a.res.p, a.res.f16, int64_t(n) * a.res.sn + int64_t(oy) * a.res.sh + int64_t(ox) * a.res.sw + int64_t(o) * a.res.sc);
    v = epilogue<true>(a, v);
    const int64_t oi = int64_t(n) * a.out.sn + int64_t(oy) * a.out.sh + int64_t(ox) * a.out.sw + o;
    if (a.out.f16) reinterpret_cast<_Float16*>(a.out.p)[oi] = _Float16(v);
    else a.out.p[oi] = v;
}

template <typename T, int CFG, int PX>
hipError_t launch_fast(const GroupedArgs& a, hipStream_t stream) {
    constexpr GroupedCfg c = kGroupedCfgs[CFG];
    const int nb = a.out.c / (c.opb * c.gpb);
    const int64_t M = int64_t(a.out.n) * a.out.h * a.out.w;
    const int64_t waves = int64_t(nb) * ((M + 64 * PX - 1) / (64 * PX));
    const int64_t blocks = (waves + kGrpBlock / 64 - 1) / (kGrpBlock / 64);
    if (blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
    conv_grouped_kernel<T, c.cpg, c.opb, c.gpb, PX><<<dim3(unsigned(blocks)), dim3(kGrpBlock), 0, stream>>>(a, nb, waves, a.out.c / a.groups);
    return hipGetLastError();
}

// the instantiations GroupedTileFits admits (the others are never eligible)
template <typename T, int CFG>
hipError_t launch_px(const GroupedArgs& a, int tile, hipStream_t stream) {
    constexpr bool f16 = sizeof(T) == 2;
    if (tile == 1) return launch_fast<T, CFG, 1>(a, stream);
    if constexpr (GroupedTileFits(CFG, f16, 2)) if (tile == 2) return launch_fast<T, CFG, 2>(a, stream);
    if constexpr (GroupedTileFits(CFG, f16, 3)) if (tile == 3) return launch_fast<T, CFG, 4>(a, stream);
    return hipErrorInvalidValue;
}

template <typename T, int CFG = 0>
hipError_t launch_cfg(const GroupedArgs& a, int cfg, int tile, hipStream_t stream) {
    if constexpr (CFG < kNumGroupedCfgs) {
        if (cfg == CFG) return launch_px<T, CFG>(a, tile, stream);
        return launch_cfg<T, CFG + 1>(a, cfg, tile, stream);
    }
    return hipErrorInvalidValue;
}

}  // namespace

bool ConvGroupedEligible(const GroupedArgs& a, int tile) {
    if (tile < 0 || tile >= kNumConvGroupedTiles || !a.w || !a.in.p || !a.out.p || a.groups < 2) return false;
    if (a.in.f8 || a.out.f8 || a.res.f8 || a.in.c % a.groups || a.out.c % a.groups || a.out.sc != 1) return false;
    if (a.kh < 1 || a.kw < 1 || a.kh > 7 || a.kw > 7 || a.sh < 1 || a.sw < 1 || (a.pre_scale && !a.pre_shift)) return false;
    if (tile == 0) return true;
    if (a.act > 5 || a.pre_act > 5) return false;      // the fast kernel compiles the activations 0-5 only: a fused GELU runs on the generic kernel
    const int cfg = GroupedCfgFor(a.in.c, a.out.c, a.groups);
    const bool f16 = a.out.f16 != 0;
    if (cfg < 0 || !GroupedTileFits(cfg, f16, tile) || a.out.c % (kGroupedCfgs[cfg].opb * kGroupedCfgs[cfg].gpb)) return false;
    if (f16 && kGroupedCfgs[cfg].cpg % 2 == 0 && (!a.w16 || reinterpret_cast<uintptr_t>(a.w16) % 4)) return false;
    const int V = f16 ? 8 : 4;
    return a.in.f16 == a.out.f16 && VecViewOk(a.in, V) && VecViewOk(a.out, V) && (!a.res.p || (a.res.f16 == a.out.f16 && VecViewOk(a.res, V)));
}

hipError_t LaunchConvGrouped(const GroupedArgs& a, int tile, hipStream_t stream) {
    if (!ConvGroupedEligible(a, tile)) return hipErrorInvalidValue;
    if (int64_t(a.out.n) * a.out.h * a.out.w * a.out.c == 0) return hipSuccess;
    if (tile == 0) {
        const int64_t total = int64_t(a.out.n) * a.out.h * a.out.w * a.out.c;
        const int64_t blocks = (total + kGrpBlock - 1) / kGrpBlock;
        if (blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
        hipLaunchKernelGGL(conv_grouped_generic_kernel, dim3(unsigned(blocks)), dim3(kGrpBlock), 0, stream, a, total);
        return hipGetLastError();
    }
    const int cfg = GroupedCfgFor(a.in.c, a.out.c, a.groups);
    return a.out.f16 ? launch_cfg<_Float16>(a, cfg, tile, stream) : launch_cfg<float>(a, cfg, tile, stream);
}

}  // namespace ie
