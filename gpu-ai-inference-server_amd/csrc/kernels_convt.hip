// Transposed convolution (ONNX ConvTranspose, group 1, no dilation: U-Net / LinkNet decoders, FCN heads, generators) on gfx950.
//
//   convt_phase_kernel<T, PB>     the fast path for the non-overlapping case kh == sh, kw == sw, no pads, no output_padding.  Every output pixel
//                                 then receives exactly ONE tap, so the op is a GEMM [M = N*H*W input pixels] x [K = Cin] x [kh*kw*Cout columns]
//                                 with a depth-to-space store: tap (ky, kx) of input pixel (iy, ix) is output pixel (iy*sh + ky, ix*sw + kx).
//                                 A wave owns 32 * PB input pixels, one block of 32 output channels and one group of up to four taps.  Rows of the
//                                 MFMA tile are input pixels, columns output channels: per K-step the wave loads its pixels' A fragments once
//                                 (16 bytes per lane, straight from the NHWC rows) and issues one MFMA per tap against that tap's [Cout][Cin]
//                                 weight rows, into 4 * PB accumulator tiles.  With kh*kw <= 4 (U-Net's 2x2/s2) the activations are read once, not
//                                 once per tap; larger kernels run ceil(kh*kw / 4) tap groups (gridDim.y; a short last group repeats its last tap in the unused tiles).  By the C/D map (col = lane & 31) a
//                                 result register holds 32 consecutive channels of one output pixel: coalesced NHWC stores.
//                                 fp32: v_mfma_f32_32x32x2_f32, a float4 fragment feeds four MFMAs (K-step 8); fp16: v_mfma_f32_32x32x16_f16 on
//                                 the half mirror of the weights (K-step 16), fp32 accumulation.  Lane l (r = l & 31, h = l >> 5) holds
//                                 A[pixel r][k0 + V*h + e] and B[k0 + V*h + e][channel r] in element e of its fragment (V = 4 floats / 8 halfs):
//                                 the same k on both sides, so the K order inside a step is free.  Pixel and Cout tails load a clamped row and
//                                 are masked at the store.  No LDS, no atomics: one wave writes each output element, the sum order is fixed.
//   convt_generic_kernel          one thread per output element in gather form: tap (ky, kx) reads input row (oy + pt - ky) / sh when the division
//                                 is exact and the row is in range (columns alike), each contribution sums over Cin.  Any k, stride, pads,
//                                 output_padding, channel counts, NCHW or NHWC input, mixed element types.  Every transposed conv the planner
//                                 accepts runs on it.
//
// Epilogue of both: + bias, ReLU.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "device_util.h"
#include "kernels.h"
#include "launch_util.h"

namespace ie {
namespace {

constexpr int kConvtBlock = 256;   // 4 waves
constexpr int kConvtTapGroup = 4;  // taps per wave: 4 * PB accumulator tiles of 16 registers

template <typename T> struct Frag;
template <> struct Frag<float> { typedef f32x4 type; };
template <> struct Frag<_Float16> { typedef h8 type; };

__device__ __forceinline__ f32x16 mma(const f32x4 a, const f32x4 b, f32x16 c) {
#pragma unroll
    for (int e = 0; e < 4; ++e) c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b[e], c, 0, 0, 0);
    return c;
}
__device__ __forceinline__ f32x16 mma(const h8 a, const h8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }

// ncb channel blocks x pixel tiles of 32 * PB input pixels; wave w of the grid takes block w % ncb of tile w / ncb (consecutive waves of a
// workgroup read the same pixels); blockIdx.y = the tap group
template <typename T, int PB>
__global__ __launch_bounds__(kConvtBlock) void convt_phase_kernel(const ConvtArgs a, const int ncb, const int64_t waves) {
    typedef typename Frag<T>::type frag;
    constexpr int V = 16 / int(sizeof(T));       // elements per fragment
    constexpr int KS = 2 * V;                    // channels per K-step
    constexpr int TG = kConvtTapGroup;
    const int64_t wave = int64_t(blockIdx.x) * (kConvtBlock / 64) + __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6);
    if (wave >= waves) return;
    const int lane = int(threadIdx.x) & 63, r = lane & 31, h = lane >> 5;
    const int cb = __builtin_amdgcn_readfirstlane(int(wave % ncb));
    const int m0 = __builtin_amdgcn_readfirstlane(int(wave / ncb)) * (32 * PB);
    const int H = a.in.h, W = a.in.w, Cin = a.in.c, Cout = a.out.c;
    const int M = a.in.n * H * W;
    const int t0 = int(blockIdx.y) * TG;
    const int nt = min(TG, a.kh * a.kw - t0);

    const T* __restrict__ in = reinterpret_cast<const T*>(a.in.p);
    const T* __restrict__ wt = sizeof(T) == 2 ? static_cast<const T*>(a.w16) : reinterpret_cast<const T*>(a.w);
    T* __restrict__ out = reinterpret_cast<T*>(a.out.p);

    const T* ap[PB];
#pragma unroll
    for (int p = 0; p < PB; ++p) {
        const int m = min(m0 + p * 32 + r, M - 1);             // a pixel tail reads the last pixel again; its rows are not stored
        const int ix = m % W, iy = (m / W) % H, n = m / (W * H);
        ap[p] = in + int64_t(n) * a.in.sn + int64_t(iy) * a.in.sh + int64_t(ix) * a.in.sw + V * h;
    }
    const int o = cb * 32 + r;
    const int64_t tstride = int64_t(Cout) * Cin;               // one tap's [Cout][Cin] operand
    const T* bp = wt + (int64_t(t0) * Cout + min(o, Cout - 1)) * Cin + V * h;      // a Cout tail reads the last row again; its columns are not stored

    f32x16 acc[TG][PB];
#pragma unroll
    for (int t = 0; t < TG; ++t)
#pragma unroll
        for (int p = 0; p < PB; ++p)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[t][p][i] = 0.f;

    // a short last tap group computes its last tap again into the unused tiles (never stored): the K loop stays free of branches, so the loads of
    // step k + 1 are in flight while the MFMAs of step k issue
    const T* bt[TG];
#pragma unroll
    for (int t = 0; t < TG; ++t) bt[t] = bp + min(t, nt - 1) * tstride;
    frag A[PB], Bf[TG];
#pragma unroll
    for (int p = 0; p < PB; ++p) A[p] = *reinterpret_cast<const frag*>(ap[p]);
#pragma unroll
    for (int t = 0; t < TG; ++t) Bf[t] = *reinterpret_cast<const frag*>(bt[t]);
    for (int k = 0; k < Cin; k += KS) {
        const int kn = min(k + KS, Cin - KS);                     // (the last step loads its own operands again)
        frag An[PB], Bn[TG];
#pragma unroll
        for (int p = 0; p < PB; ++p) An[p] = *reinterpret_cast<const frag*>(ap[p] + kn);
#pragma unroll
        for (int t = 0; t < TG; ++t) Bn[t] = *reinterpret_cast<const frag*>(bt[t] + kn);
#pragma unroll
        for (int t = 0; t < TG; ++t)
#pragma unroll
            for (int p = 0; p < PB; ++p) acc[t][p] = mma(A[p], Bf[t], acc[t][p]);
#pragma unroll
        for (int p = 0; p < PB; ++p) A[p] = An[p];
#pragma unroll
        for (int t = 0; t < TG; ++t) Bf[t] = Bn[t];
    }

    // register i of a tile: row (i & 3) + 8 * (i >> 2) + 4 * h, column r
    if (o >= Cout) return;
    const float bias = a.bias ? a.bias[o] : 0.f;
#pragma unroll
    for (int p = 0; p < PB; ++p) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int m = m0 + p * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
            if (m >= M) continue;
            const int ix = m % W, iy = (m / W) % H, n = m / (W * H);
            T* dst = out + int64_t(n) * a.out.sn + int64_t(iy) * a.sh * a.out.sh + int64_t(ix) * a.sw * a.out.sw + o;
#pragma unroll
            for (int t = 0; t < TG; ++t) {
                if (t < nt) {
                    const int ky = (t0 + t) / a.kw, kx = (t0 + t) % a.kw;
                    float v = acc[t][p][i] + bias;
                    if (a.relu) v = fmaxf(v, 0.f);
                    dst[int64_t(ky) * a.out.sh + int64_t(kx) * a.out.sw] = T(v);
                }
            }
        }
    }
}

__global__ __launch_bounds__(kConvtBlock) void convt_generic_kernel(const ConvtArgs a, const int64_t total) {
    const int64_t idx = int64_t(blockIdx.x) * kConvtBlock + threadIdx.x;
    if (idx >= total) return;
    const int C = a.out.c, Cin = a.in.c;
    const int o = int(idx % C);
    int64_t m = idx / C;
    const int ox = int(m % a.out.w); m /= a.out.w;
    const int oy = int(m % a.out.h);
    const int n = int(m / a.out.h);
    const int64_t base = int64_t(n) * a.in.sn;
    float acc = 0.f;
    for (int ky = 0; ky < a.kh; ++ky) {
        const int ty = oy + a.pt - ky;
        if (ty < 0 || ty % a.sh != 0 || ty / a.sh >= a.in.h) continue;
        for (int kx = 0; kx < a.kw; ++kx) {
            const int tx = ox + a.pl - kx;
            if (tx < 0 || tx % a.sw != 0 || tx / a.sw >= a.in.w) continue;
            const int64_t px = base + int64_t(ty / a.sh) * a.in.sh + int64_t(tx / a.sw) * a.in.sw;
            const float* w = a.w + (int64_t(ky * a.kw + kx) * C + o) * Cin;
            float part = 0.f;
            for (int c = 0; c < Cin; ++c) part = fmaf(w[c], ld_any(a.in.p, a.in.f16, px + int64_t(c) * a.in.sc), part);
            acc += part;
        }
    }
    float v = acc + (a.bias ? a.bias[o] : 0.f);
    if (a.relu) v = fmaxf(v, 0.f);
    const int64_t oi = int64_t(n) * a.out.sn + int64_t(oy) * a.out.sh + int64_t(ox) * a.out.sw + o;
    if (a.out.f16) reinterpret_cast<_Float16*>(a.out.p)[oi] = _Float16(v);
    else a.out.p[oi] = v;
}

template <typename T, int PB>
hipError_t launch_phase(const ConvtArgs& a, hipStream_t stream) {
    const int ncb = (a.out.c + 31) / 32;
    const int64_t M = int64_t(a.in.n) * a.in.h * a.in.w;
    const int64_t waves = int64_t(ncb) * ((M + 32 * PB - 1) / (32 * PB));
    const int64_t blocks = (waves + kConvtBlock / 64 - 1) / (kConvtBlock / 64);
    const int groups = (a.kh * a.kw + kConvtTapGroup - 1) / kConvtTapGroup;
    if (blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
    convt_phase_kernel<T, PB><<<dim3(unsigned(blocks), unsigned(groups)), dim3(kConvtBlock), 0, stream>>>(a, ncb, waves);
    return hipGetLastError();
}

}  // namespace

bool ConvTransposedEligible(const ConvtArgs& a, int tile) {
    if (tile < 0 || tile >= kNumConvtTiles || !a.w || !a.in.p || !a.out.p) return false;
    if (a.in.f8 || a.out.f8 || a.out.sc != 1 || a.in.c < 1 || a.out.c < 1 || a.in.n != a.out.n) return false;
    if (a.kh < 1 || a.kw < 1 || a.sh < 1 || a.sw < 1 || a.pt < 0 || a.pl < 0 || a.pb < 0 || a.pr < 0 || a.oph < 0 || a.opw < 0) return false;
    if (int64_t(a.out.h) != int64_t(a.in.h - 1) * a.sh + a.kh - a.pt - a.pb + a.oph || int64_t(a.out.w) != int64_t(a.in.w - 1) * a.sw + a.kw - a.pl - a.pr + a.opw)
        return false;
    if (tile == 0) return true;
    if (a.kh != a.sh || a.kw != a.sw || a.pt || a.pl || a.pb || a.pr || a.oph || a.opw || a.kh * a.kw > 16) return false;
    const bool f16 = a.out.f16 != 0;
    const int V = f16 ? 8 : 4;
    if ((a.in.f16 != 0) != f16 || !VecViewOk(a.in, V) || a.in.c % (2 * V)) return false;      // (whole K-steps of two vectors, not only whole vectors)
    if (int64_t(a.in.n) * a.in.h * a.in.w >= (int64_t(1) << 31) - 64) return false;
    const void* w = f16 ? a.w16 : static_cast<const void*>(a.w);
    return w && Aligned16(w);
}

hipError_t LaunchConvTransposed(const ConvtArgs& a, int tile, hipStream_t stream) {
    if (!ConvTransposedEligible(a, tile)) return hipErrorInvalidValue;
    const int64_t total = int64_t(a.out.n) * a.out.h * a.out.w * a.out.c;
    if (total == 0) return hipSuccess;
    if (tile == 0) {
        const int64_t blocks = (total + kConvtBlock - 1) / kConvtBlock;
        if (blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
        hipLaunchKernelGGL(convt_generic_kernel, dim3(unsigned(blocks)), dim3(kConvtBlock), 0, stream, a, total);
        return hipGetLastError();
    }
    if (a.out.f16) return tile == 1 ? launch_phase<_Float16, 1>(a, stream) : launch_phase<_Float16, 2>(a, stream);
    return tile == 1 ? launch_phase<float, 1>(a, stream) : launch_phase<float, 2>(a, stream);
}

}  // namespace ie
