// Launchers of the hand-written gfx950 kernels (definitions in kernels.hip).
// Every launcher only enqueues work on `stream` (no allocation, no synchronisation), so a whole forward
// pass can be captured into a hipGraph (executor.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace ie {

// Strided activation operand: element (n, y, x, c) lives at  base + n*sn + y*sh + x*sw + c*sc.
// f16 != 0: the buffer holds IEEE half elements (fp16 precision mode); `p` is then only a typed alias of the address and
// all strides stay in ELEMENTS.
struct TensorArg {
    float* p = nullptr;
    int n = 0, h = 0, w = 0, c = 0;
    int64_t sn = 0, sh = 0, sw = 0, sc = 0;
    int f16 = 0;
    int f8 = 0;                        // the buffer holds OCP e4m3 bytes (fp8 precision mode); strides in ELEMENTS = bytes; never set together with f16
};

// Fused pointwise activations (plan.h ActKind): 0 none, 1 sigmoid, 2 hardsigmoid max(0, min(1, a*x + b)), 3 silu x*sigmoid(x),
// 4 hardswish x*hardsigmoid(x; a, b), 5 relu, 6 gelu 0.5*x*(1 + erf(x / sqrt 2)), 7 its tanh approximation 0.5*x*(1 + tanh(sqrt(2/pi)*(x + 0.044715*x^3))),
// 8 tanh(x) (BERT's pooler).
// fp32 math in every element type.
// ApplyActBasic: codes 0-5 only.  The channel-block kernels whose register budget decides their occupancy (kernels_grouped.hip's fast kernel) call
// it, so the erf / tanh code of the GELUs is not inlined into them; their eligibility keeps steps with a code above 5 on the generic kernels.
__host__ __device__ inline float ApplyActBasic(int kind, float a, float b, float x) {
    switch (kind) {
        case 1: return 1.f / (1.f + expf(-x));
        case 2: return fminf(fmaxf(a * x + b, 0.f), 1.f);
        case 3: return x / (1.f + expf(-x));
        case 4: return x * fminf(fmaxf(a * x + b, 0.f), 1.f);
        case 5: return fmaxf(x, 0.f);
        default: return x;
    }
}
__host__ __device__ inline float ApplyAct(int kind, float a, float b, float x) {
    switch (kind) {
        case 6: return 0.5f * x * (1.f + erff(x * 0.70710678f));
        case 7: return 0.5f * x * (1.f + tanhf(0.79788456f * (x + 0.044715f * x * x * x)));
        case 8: return tanhf(x);
        default: return ApplyActBasic(kind, a, b, x);
    }
}

struct ConvArgs {
    TensorArg in, out;                 // out is always NHWC (sc == 1)
    TensorArg res;                     // res.p != null: out = act(conv + bias + res), res has the output's shape (residual Add fused)
    const float* w = nullptr;          // [Cout][kh][kw][Cin]
    const void* w16 = nullptr;         // the same weights as halfs at the same element offset (fp16 precision mode)
    const float* wfrag = nullptr;      // fragment-major fp32 mirror of w (LaunchPermuteWeightsFrag), or null
    const float* bias = nullptr;       // [Cout] or null
    const float* pre_scale = nullptr;  // [Cin] or null: x <- x*scale + shift (then ReLU if pre_relu) before the conv
    const float* pre_shift = nullptr;
    const void* pre_scale16 = nullptr; // half copies of pre_scale / pre_shift (fp16 precision mode, packed-half prologue)
    const void* pre_shift16 = nullptr;
    int kh = 1, kw = 1, sh = 1, sw = 1, pt = 0, pl = 0;
    int pre_relu = 0, relu = 0;
    float* workspace = nullptr;        // split-K partial slabs (only when splitk > 1)
    int64_t workspace_floats = 0;      // capacity of `workspace`
    int* counters = nullptr;           // per-tile arrival counters for the in-launch combine; null = two-pass reduce kernel
    int num_counters = 0;
    // fp8 precision mode (kernels_f8.hip): e4m3 weights at the same element offsets as `w`, the per-output-channel multiplier that
    // turns the e4m3 x e4m3 dot product into real units (input scale x weight-row scale), the shortcut's scale, 1 / output scale
    const void* w8 = nullptr;
    const float* escale = nullptr;
    float res_scale = 1.f, out_qscale = 1.f;
    // fp8 mode, DUAL 1x1 (kernels_ws8.hip): a second GEMM accumulated into the same output -- the projection shortcut of a bottleneck block,
    // out = act(conv(in) + conv_b(in2)) with in2 read at pixel (oy * sh2, ox * sw2); in2.p == null: none
    TensorArg in2;
    const void* w8b = nullptr;
    const float* escale_b = nullptr;
    const float* bias_b = nullptr;
    int sh2 = 1, sw2 = 1;
    int64_t in2_bytes = 0;
    int debug = 0;                     // timing-only ablation bits (IE_DEBUG_ABLATE), 0 in production
    // dilation: tap (ky, kx) reads input pixel (oy*sh - pt + ky*dh, ox*sw - pl + kx*dw).  Only the naive kernel and the dilated instantiations
    // of the implicit GEMMs read it; it sits in the padding before in_bytes, so no other field moves and the other kernels are unchanged
    int16_t dh = 1, dw = 1;
    int64_t in_bytes = 0;              // filled by LaunchConvIgemm: byte span of the input view (buffer descriptor range)
};
static_assert(sizeof(ConvArgs) == 464 && offsetof(ConvArgs, in_bytes) == 456, "ConvArgs layout: the dilation must stay in the padding");

// The 3x3 half of a fused dense-layer step (kernels_fused.hip): bottleneck tensor in, 32 fresh channels out (the tail of the 1x1's
// input view), fragment-major 3x3 weights.
// Per-launch constants of conv_dense_fused_kernel, worked out on the host by LaunchConvDenseFused so that the kernel divides nothing:
// reciprocals (mg20_*: ceil(2^20 / d), for per-lane quotients n * d < 2^20 with a 24-bit multiply; mg32_*: floor(2^32 / d), 2^32 - 1 for
// d == 1, for wave-uniform quotients on the scalar unit with one correction step) and the slot counts of the two staging loops.
struct FusedConsts {
    unsigned mg20_c4n3 = 0, mg20_c4n = 0, mg20_w = 0, mg20_h = 0;      // columns of a window row / of an old-channel row (4 channels each), map width, map height (0: h > 512)
    unsigned hbig = 0x7fffffff;                                         // map height when it is above 512 (a tile then wraps past an image's last row at most once)
    unsigned mg32_hw = 0, mg32_w = 0, mg32_cpt3 = 0;                    // pixels per image, map width, 16-channel chunks per 3x3 tap
    int wrpp = 0, wfull = 0, wlast = 0;                                 // window: rows per slot, full slots, rows of the partial last slot
    int rpp = 0, xfull = 0, xlast = 0;                                  // old channels: the same
};

struct FusedArgs {
    TensorArg in3, out3;
    const float* wfrag3 = nullptr;
    const float* bias3 = nullptr;
    int relu3 = 0;
    FusedConsts k;                     // filled by LaunchConvDenseFused
};

struct PoolArgs {
    TensorArg in, out;                 // NHWC
    int kh = 1, kw = 1, sh = 1, sw = 1, pt = 0, pl = 0, pb = 0, pr = 0;
    int is_max = 0, count_include_pad = 0;
    const float* pre_scale = nullptr;  // per channel: x <- x*scale + shift (then ReLU if pre_relu) before pooling
    const float* pre_shift = nullptr;  // (a transition's BN -> ReLU -> 1x1 conv -> AvgPool runs as BN -> ReLU -> AvgPool -> 1x1 conv)
    int pre_relu = 0;
    float in_scale = 1.f, out_qscale = 1.f;   // e4m3 tensors: real = q * in_scale, q_out = real * out_qscale
};

struct EltArgs {
    TensorArg a, b, out;               // b.p == null: no second operand
    const float* scale = nullptr;      // per channel, or null
    const float* shift = nullptr;
    int relu = 0;
    float lo = -__builtin_huge_valf(), hi = __builtin_huge_valf();   // then min(max(v, lo), hi) (ONNX Clip); the defaults clamp nothing
    int act = 0;                       // then ApplyAct(act, act_a, act_b, v); 0 = none
    float act_a = 0.f, act_b = 0.f;
    int b_mul = 0;                     // 1: the second operand multiplies instead of adding
    int b_bcast = 0;                   // 1: b is [N, C, 1, 1], read at (n, c) for every pixel (a per-image channel gate)
    int pre_act = 0;                   // ApplyAct(pre_act, pre_act_a, pre_act_b, .) on a (after scale / shift) before b joins it: SwiGLU's Mul(SiLU(gate), up)
    float pre_act_a = 0.f, pre_act_b = 0.f;
};

// Depthwise conv (group == Cin == Cout, kernels_dw.hip): out[n, y, x, c] = clamp(act(sum_{ky,kx} w[c][ky][kx] * f(in[n, y*sh - pt + ky,
// x*sw - pl + kx, c]) + bias[c] (+ res)), lo, hi), f = the optional prologue min(act(x * pre_scale[c] + pre_shift[c]), pre_hi) on the
// in-range taps (padding taps contribute 0).  fp32 accumulation; activations float or half (TensorArg::f16), weights / vectors fp32.
struct DwArgs {
    TensorArg in, out, res;            // out NHWC (sc == 1); res.p != null: residual added before the ReLU / clamp
    const float* w = nullptr;          // [C][kh][kw] (BatchNorm folded)
    const float* bias = nullptr;       // [C] or null
    const float* pre_scale = nullptr;  // [C] or null
    const float* pre_shift = nullptr;
    int pre_relu = 0;
    float pre_hi = __builtin_huge_valf();
    int kh = 1, kw = 1, sh = 1, sw = 1, pt = 0, pl = 0;
    int relu = 0;
    float lo = -__builtin_huge_valf(), hi = __builtin_huge_valf();
    int act = 0, pre_act = 0;          // ApplyAct codes: after the clamp / after the prologue's bound (0 = none)
    float act_a = 0.f, act_b = 0.f, pre_act_a = 0.f, pre_act_b = 0.f;
};
// tile 0: generic (one channel per lane; any k <= 7, stride, padding, C, NCHW input); tiles 1-3: 16-byte channel vectors per lane (4 floats /
// 8 halfs) and 1 / 2 / 4 output pixels along W per lane, for k in {3, 5}, stride in {1, 2}, C and pitches multiples of the vector width
constexpr int kNumConvDwTiles = 4;
// Output pixels per lane the fast kernel runs for `px` requested: with a fused activation (act / pre_act) the prologue's per-element activation
// must still fit the fully unrolled filter-row loop, so the wide variants step down (k x input vectors per row x vector width <= 200)
constexpr int DwLanePixels(int px, bool f16, int k, int s, bool act) {
    return !act ? px : (px >= 4 && k * (3 * s + k) * (f16 ? 8 : 4) <= 200 ? 4 : (px >= 2 && k * (s + k) * (f16 ? 8 : 4) <= 200 ? 2 : 1));
}
bool ConvDwEligible(const DwArgs& a, int tile);
hipError_t LaunchConvDw(const DwArgs& a, int tile, hipStream_t stream);

// Grouped conv (1 < group, not depthwise; kernels_grouped.hip): the DwArgs epilogue / prologue with output channel o reading the input channels
// [(o / (Cout / groups)) * (Cin / groups), + Cin / groups).  w is [Cout][kh][kw][Cin / groups].
struct GroupedArgs : DwArgs {
    const void* w16 = nullptr;         // the same weights as halfs at the same element offsets (fp16 plans), or null
    int groups = 1;
};
// The fast kernel's per-wave channel blocks: gpb whole groups of opb output channels (opb == Cout / groups), or, with gpb == 1, a slice of opb
// output channels of one group (opb divides Cout / groups); the wave reads the cpg * gpb input channels of its groups.
struct GroupedCfg { int cpg, opb, gpb; };
inline constexpr GroupedCfg kGroupedCfgs[] = {{1, 2, 8}, {2, 2, 8}, {4, 4, 4}, {8, 8, 2}, {8, 8, 1}, {16, 16, 1}, {32, 16, 1}, {64, 16, 1}};
inline constexpr int kNumGroupedCfgs = int(sizeof(kGroupedCfgs) / sizeof(kGroupedCfgs[0]));
// tile 0: generic (one output element per thread; any group, k <= 7, stride, padding, NCHW input, mixed element types); tiles 1-3: the
// channel-block kernel with 1 / 2 / 4 output pixels per lane
constexpr int kNumConvGroupedTiles = 4;
inline constexpr int kGroupedPx[kNumConvGroupedTiles] = {0, 1, 2, 4};
// the fast config of a conv (-1: none; the generic kernel runs it)
constexpr int GroupedCfgFor(int64_t cin, int64_t cout, int64_t groups) {
    if (groups < 2 || cin % groups || cout % groups) return -1;
    const int64_t cpg = cin / groups, opg = cout / groups;
    for (int i = 0; i < kNumGroupedCfgs; ++i) {
        const GroupedCfg& c = kGroupedCfgs[i];
        if (c.cpg == cpg && (c.gpb > 1 ? opg == c.opb && groups % c.gpb == 0 : opg % c.opb == 0)) return i;
    }
    return -1;
}
// a lane's accumulators and input registers (px pixels: px * (outputs + inputs), halfs packed in pairs) stay within 128 VGPRs
constexpr bool GroupedTileFits(int cfg, bool f16, int tile) {
    if (cfg < 0 || tile < 1 || tile >= kNumConvGroupedTiles) return false;
    const GroupedCfg& c = kGroupedCfgs[cfg];
    const int in_regs = f16 && c.cpg % 2 == 0 ? c.cpg * c.gpb / 2 : c.cpg * c.gpb;
    return kGroupedPx[tile] * (c.opb * c.gpb + in_regs) <= 128;
}
bool ConvGroupedEligible(const GroupedArgs& a, int tile);
hipError_t LaunchConvGrouped(const GroupedArgs& a, int tile, hipStream_t stream);

// Transposed conv (ONNX ConvTranspose, group 1, no dilation; kernels_convt.hip): out[n, iy*sh + ky - pt, ix*sw + kx - pl, o] += sum_c in[n, iy, ix, c] *
// w[ky][kx][o][c]; output rows / columns the pads cut off are dropped, the output_padding rows / columns at the bottom / right receive the bias
// only.  Epilogue: + bias, ReLU.  fp32 accumulation; activations float or half (TensorArg::f16), bias fp32.
struct ConvtArgs {
    TensorArg in, out;                 // out NHWC (sc == 1) of extent (in.h - 1) * sh + kh - pt - pb + output_padding
    const float* w = nullptr;          // [kh][kw][Cout][Cin] (BatchNorm folded)
    const void* w16 = nullptr;         // the same weights as halfs at the same element offsets (fp16 plans), or null
    const float* bias = nullptr;       // [Cout] or null
    int kh = 1, kw = 1, sh = 1, sw = 1, pt = 0, pl = 0, pb = 0, pr = 0, oph = 0, opw = 0;
    int relu = 0;
};
// tile 0: generic (one output element per thread in gather form; any k, stride, pads, output_padding, channel counts, NCHW input, mixed element
// types); tiles 1-2: the MFMA kernel of the non-overlapping case (kh == sh, kw == sw, no pads, no output_padding, kh * kw <= 16) with 32 / 64
// input pixels per wave: NHWC operands of one element type, Cin a multiple of the K-step (8 floats / 16 halfs), 16-byte aligned input pixel rows
// and weights.  Cout and pixel tails are masked
constexpr int kNumConvtTiles = 3;
inline constexpr int kConvtPixelBlocks[kNumConvtTiles] = {0, 1, 2};      // 32-pixel MFMA row blocks per wave
bool ConvTransposedEligible(const ConvtArgs& a, int tile);
hipError_t LaunchConvTransposed(const ConvtArgs& a, int tile, hipStream_t stream);

// LayerNormalization over the channels of an NHWC view (kernels_ln.hip): out[p, c] = (in[p, c] - mean_p) * rsqrt(var_p + eps) * gamma[c] + beta[c] for
// every pixel row p, var_p the mean of the centred squares.  fp32 accumulation; activations float or half (TensorArg::f16); gamma / beta fp32.
// out may alias in.
struct LnArgs {
    TensorArg in, out;                 // the same shape; normalised over c
    const float* gamma = nullptr;      // [C]
    const float* beta = nullptr;       // [C] or null
    float eps = 1e-5f;
    // RMSNorm (Llama-class graphs): out[p, c] = in[p, c] * rsqrt(mean_c(in[p, :]^2) + eps) * gamma[c]; no mean, no centring, beta must be null.  The
    // kernels are compile-time variants of the layer norm's under their own names (rmsnorm_kernel<T, LANES>, rmsnorm_generic_kernel): the same tiles,
    // eligibility and default tile
    int rms = 0;
};
// tile 0: generic (one wave per pixel row; any C, channel stride, pitch, channel offset, mixed element types); tiles 1-4: a group of 8 / 16 / 32 / 64
// lanes per row, the row held in registers as up to kLnMaxVectors 16-byte vectors (4 floats / 8 halfs) per lane: sc == 1, C / pitch / channel offset
// multiples of the vector width, 16-byte aligned bases, C <= lanes * kLnMaxVectors * vector width (fp32: 1536 on the 64-lane tile)
constexpr int kNumLnTiles = 5;
inline constexpr int kLnLanes[kNumLnTiles] = {0, 8, 16, 32, 64};
constexpr int kLnMaxVectors = 6;
constexpr bool LnTileFits(int64_t c, bool f16, int tile) {
    const int64_t V = f16 ? 8 : 4;
    return tile >= 1 && tile < kNumLnTiles && c % V == 0 && c / V <= int64_t(kLnLanes[tile]) * kLnMaxVectors;
}
// the smallest group that holds the row in at most three vectors per lane (what the load-time search picked on 6 of the 8 spatial layer-norm shapes
// of ConvNeXt-Tiny, fp32 b32 and fp16 b128: DESIGN 3.22), else the smallest that holds it at all, else the generic kernel
constexpr int LnDefaultTile(int64_t c, bool f16) {
    for (int t = 1; t < kNumLnTiles; ++t) if (LnTileFits(c, f16, t) && c / (f16 ? 8 : 4) <= 3 * kLnLanes[t]) return t;
    for (int t = 1; t < kNumLnTiles; ++t) if (LnTileFits(c, f16, t)) return t;
    return 0;
}
bool LayerNormEligible(const LnArgs& a, int tile);
hipError_t LaunchLayerNorm(const LnArgs& a, int tile, hipStream_t stream);

// GroupNormalization of an NHWC view (kernels_gn.hip): for image n and group g = c / (C / groups), over the C / groups channels of the group and every pixel,
//   out[n, p, c] = act((in[n, p, c] - mean_ng) * rsqrt(var_ng + eps) * gamma[c] + beta[c]),  var_ng the mean of the centred squares.
// fp32 statistics in both element types; gamma / beta fp32; no atomics, every combine in a fixed order.  out may alias in.
struct GnArgs {
    TensorArg in, out;                 // the same shape
    const float* gamma = nullptr;      // [C]
    const float* beta = nullptr;       // [C] or null
    int groups = 1;
    float eps = 1e-5f;
    int act = 0; float act_a = 0.f, act_b = 0.f;   // ApplyAct on the result
    float* workspace = nullptr;        // tile 1: the (count, mean, M2) records, GnWorkspaceFloats of them
    int64_t workspace_floats = 0;
};
// tile 0: groupnorm_generic_kernel, one workgroup per (image, group), three passes over its data: any C / groups, channel stride, pitch, channel
// offset, mixed element types.  tile 1: groupnorm_stats_kernel + groupnorm_apply_kernel over (image, slab of pixels) with 16-byte channel vectors
// (V = 4 floats / 8 halfs of the OUTPUT type): C, both pitches and both channel offsets multiples of V, at most kGnMaxVectors vectors per pixel
// (a lane keeps one), and a vector inside one group or made of whole groups (C / groups a multiple or a divisor of V); the activation one of
// none / sigmoid / silu / relu.
constexpr int kNumGnTiles = 2;
constexpr int kGnBlock = 256;
constexpr int kGnMaxVectors = kGnBlock;
constexpr bool GnActOk(int act) { return act == 0 || act == 1 || act == 3 || act == 5; }
constexpr bool GnTileFits(int64_t c, int64_t groups, bool f16_out, int64_t pitch_in, int64_t off_in, int64_t pitch_out, int64_t off_out, int act, int tile) {
    const int64_t V = f16_out ? 8 : 4;
    if (tile != 1 || groups < 1 || c % groups || c % V || c / V > kGnMaxVectors || !GnActOk(act)) return false;
    const int64_t cpg = c / groups;
    return (cpg % V == 0 || V % cpg == 0) && pitch_in % V == 0 && off_in % V == 0 && pitch_out % V == 0 && off_out % V == 0;
}
// Pixels per slab: at least about 64 KiB of the image per workgroup (enough work to hide the launch), whole multiples of the pixel rows a workgroup
// covers per iteration; larger where that would make more than kGnMaxSlabs slabs per image or more than about kGnWantBlocks workgroups in all (every
// apply workgroup combines all of its image's records first: with 256 slabs of 64 KiB that combine took longer than the slab's own traffic)
constexpr int kGnMaxSlabs = 256;
constexpr int kGnWantBlocks = 2048;
constexpr int64_t GnSlabPixels(int64_t n, int64_t hw, int64_t c, bool f16) {
    const int64_t cv = c / (f16 ? 8 : 4), rows = cv >= 1 && cv <= kGnBlock ? kGnBlock / cv : 1;      // pixel rows per iteration
    int64_t px = 65536 / (c < 1 ? 1 : c * (f16 ? 2 : 4));
    int64_t want = kGnWantBlocks / (n < 1 ? 1 : n);
    want = want < 1 ? 1 : (want > kGnMaxSlabs ? kGnMaxSlabs : want);
    if (px * want < hw) px = (hw + want - 1) / want;
    px = (px + rows - 1) / rows * rows;
    return px < 1 ? 1 : px;
}
constexpr int64_t GnSlabs(int64_t n, int64_t hw, int64_t c, bool f16) { const int64_t px = GnSlabPixels(n, hw, c, f16); return (hw + px - 1) / px; }
// floats of workspace tile 1 needs: one (count, mean, M2) record per (image, slab, group)
constexpr int64_t GnWorkspaceFloats(int64_t n, int64_t hw, int64_t c, int64_t groups, bool f16) { return 3 * n * GnSlabs(n, hw, c, f16) * groups; }
// the planner's default where tile 1 fits: two launches cost more than they save while one workgroup per (image, group) still has little to read
constexpr int64_t kGnTile1MinGroupElems = 2048;
constexpr int GnDefaultTile(int64_t n, int64_t hw, int64_t c, int64_t groups) { return hw * (c / groups) >= kGnTile1MinGroupElems ? 1 : 0; }
bool GroupNormEligible(const GnArgs& a, int tile);
hipError_t LaunchGroupNorm(const GnArgs& a, int tile, hipStream_t stream);
// tile 1's launches one by one (scripts): 0 statistics, 1 apply
hipError_t LaunchGroupNormPhase(const GnArgs& a, int phase, hipStream_t stream);

// Token embedding + LayerNormalization (kernels_embed.hip; BERT-class graphs): for every token row r = (n, l) of out [N, L, D]
//   out[r, :] = LayerNorm(word[ids[r]] + type[tids[r]] + pos[l]; gamma, beta, eps)
// gamma null (a pre-LN model such as GPT-2, whose sum is read by a LayerNormalization AND by the residual Add): out[r, :] = the fp32 sum itself,
// stored in out's element type (embed_sum_kernel<T, LANES> / embed_sum_generic_kernel; the same tiles and eligibility).
// ids / tids are the dense int64 [N, L] graph inputs; a negative index counts from the end, the wrapped index is clamped into the table.  Tables,
// position rows, gamma and beta are fp32 in every precision; out is float or half (TensorArg::f16).  Statistics as LnArgs.
struct EmbedArgs {
    const int64_t* ids = nullptr;      // [N * L]
    const int64_t* tids = nullptr;     // [N * L], or null (no second table)
    const float* word = nullptr;       // [vocab][D]
    const float* type = nullptr;       // [types][D] or null
    const float* pos = nullptr;        // [L][D] or null
    const float* gamma = nullptr;      // [D], or null: no LayerNormalization behind the sum
    const float* beta = nullptr;       // [D] or null
    TensorArg out;                     // out.n = N, out.w = L, out.c = D, out.h = 1
    int vocab = 0, types = 0;
    float eps = 1e-5f;
};
// tile 0: embed_ln_generic_kernel (one wave per token row; any D, pitch, offset).  tiles 1-4: embed_ln_kernel, the lane groups of the layer-norm
// kernel (kLnLanes): D a multiple of the OUTPUT type's 16-byte vector (4 floats / 8 halfs; the fp32 table rows are then whole 16-byte vectors
// too), the row inside the register budget (at most kLnMaxVectors vectors per lane), the output pitch and offset multiples of the vector
constexpr int kNumEmbedTiles = kNumLnTiles;
constexpr bool EmbedTileFits(int64_t d, bool f16_out, int64_t pitch_out, int64_t off_out, int tile) {
    const int64_t V = f16_out ? 8 : 4;
    return LnTileFits(d, f16_out, tile) && pitch_out % V == 0 && off_out % V == 0;
}
// the planner's default: the layer-norm rule (the smallest lane group that holds the row in three vectors per lane), else the generic kernel
constexpr int EmbedDefaultTile(int64_t d, bool f16_out, int64_t pitch_out, int64_t off_out) {
    const int t = LnDefaultTile(d, f16_out);
    return t > 0 && EmbedTileFits(d, f16_out, pitch_out, off_out, t) ? t : 0;
}
bool EmbedEligible(const EmbedArgs& a, int tile);
hipError_t LaunchEmbed(const EmbedArgs& a, int tile, hipStream_t stream);

// Multi-head attention over a token view (kernels_attn.hip).  in = the qkv rows [N, L, 3 D] (in.w = L, in.c = 3 D, D = heads * head_dim): column
// s * D + h * head_dim + e of a row is element e of head h of q / k / v for s = 0 / 1 / 2.  out[n, i, h * head_dim + e] =
// sum_j softmax_j(scale * q[n, h, i, :] . k[n, h, j, :]) * v[n, h, j, e].  fp32 scores, statistics and accumulation; no score matrix in memory.
// Key mask (BERT's attention_mask): mask = the int64 [N, L] graph input (row n at mask + n * mask_sn), mask_value = c; the score of key j of image n
// gets the bias (1 - float(mask[n, j])) * c, computed in fp32 as the graph's Cast -> Sub -> Mul computes it, before the softmax.  The biased score
// is kept finite (c = finfo(float32).min would otherwise make a fully masked row exp(-inf - -inf) = NaN): such a row gives what the graph gives.
struct AttnArgs {
    TensorArg in, out;
    int heads = 0, head_dim = 0;
    float scale = 1.f;
    const int64_t* mask = nullptr;     // null: no mask
    int64_t mask_sn = 0;
    float mask_value = 0.f;
    int causal = 0;                    // query i attends to the keys j <= i only (a decoder's mask); never together with a key mask
    // Grouped-query attention (Llama-class graphs): kv_heads K / V heads (0 or heads: one per query head, as above).  With Dkv = kv_heads * head_dim a
    // token row is q (D) | k (Dkv) | v (Dkv), in.c == D + 2 Dkv, and query head h reads K / V head h / (heads / kv_heads) (HF's repeat_kv: a
    // repeat_interleave).  heads % kv_heads == 0.  Every tile
    int kv_heads = 0;
    // Rotary position embedding (null: none): fp32 tables [L][head_dim], 16-byte aligned.  q and k of token position i enter the scores as
    //   x'[e] = x[e] * cos[i][e] + s(e) * x[p(e)] * sin[i][e],  p(e) = e + hd/2, s = -1 for e < hd/2;  p(e) = e - hd/2, s = +1 otherwise
    // (x * cos + rotate_half(x) * sin with full-width tables: the two halves of a table row need not be equal).  fp32 arithmetic; a half operand is
    // rounded once, where it enters LDS (k) or the MFMA fragment (q; tile 2: k too).  Tiles 1, 2 and 3 rotate in their causal form only
    // (attention_mfma_kernel<.,.,causal,rope>), tile 2 at head_dim 128 and 256; tile 0 rotates in every form; never together with a key mask; head_dim even
    const float* rope_cos = nullptr;
    const float* rope_sin = nullptr;
};
// tile 0: attention_generic_kernel (one wave per query row; any L, head_dim, pitch, offset; float or half).  tile 1: attention_mfma_kernel<T, HD>
// (a workgroup = one image, one head, 128 queries; the head's K and V rows in LDS): head_dim 32 or 64, the channel counts, pitches and offsets
// multiples of the 16-byte vector, and both of the head's padded K and V images inside the LDS budget.  tile 2: attention_stream_kernel<T, HD>
// (a workgroup = one image, one head, 32 queries; its four waves split the head dim; K and V streamed in tiles of 32 keys, LDS independent of L):
// head_dim 128, 256 or 512, no key mask, the same vector conditions; <T, HD, CAUSAL> walks the key tiles up to the diagonal one, <T, HD, CAUSAL, ROPE>
// (head_dim 128 or 256) also rotates q and k.  tile 3: attention_chunk_kernel<T, HD, CAUSAL> (tile 1's workgroup,
// K and V staged in chunks of kAttnChunkKeys keys, LDS independent of L): head_dim 32 or 64, no key mask, the same vector conditions
constexpr int kNumAttnTiles = 4;
// IE_FORCE_TILE reaches tiles 0 and 1 of an attention step only (2 and 3 keep meaning "not forced"); tiles 2 and 3 are pinned with IE_ATTN_TILE
constexpr int kNumAttnForcedTiles = 2;
constexpr int64_t kAttnLdsBudget = 160 * 1024;
// bytes of LDS the MFMA kernel needs: K and V rows, L padded to whole 32-key tiles, every row padded by one 16-byte vector; masked: one fp32 bias
// per padded key behind them
constexpr int64_t AttnLdsBytes(int64_t L, int hd, bool f16, bool masked = false) {
    return 2 * ((L + 31) / 32 * 32) * (int64_t(hd) * (f16 ? 2 : 4) + 16) + (masked ? 4 * ((L + 31) / 32 * 32) : 0);
}
constexpr bool AttnMfmaFits(int64_t L, int hd, bool f16, int64_t c_in, int64_t pitch_in, int64_t off_in, int64_t c_out, int64_t pitch_out, int64_t off_out,
                            bool masked = false) {
    const int64_t V = f16 ? 8 : 4;
    return (hd == 32 || hd == 64) && L >= 1 && c_in % V == 0 && pitch_in % V == 0 && off_in % V == 0 && c_out % V == 0 && pitch_out % V == 0 && off_out % V == 0 &&
           AttnLdsBytes(L, hd, f16, masked) <= kAttnLdsBudget;
}
// bytes of LDS the streaming kernel needs: two V tiles of 32 keys and two sets of the four waves' partial 32 x 32 fp32 score tiles
constexpr int64_t AttnStreamLdsBytes(int hd, bool f16) { return 2 * (32 * int64_t(hd) * (f16 ? 2 : 4) + 4 * 32 * 32 * 4); }
constexpr bool AttnStreamFits(int64_t L, int hd, bool f16, int64_t c_in, int64_t pitch_in, int64_t off_in, int64_t c_out, int64_t pitch_out, int64_t off_out,
                              bool masked = false) {
    const int64_t V = f16 ? 8 : 4;
    return (hd == 128 || hd == 256 || hd == 512) && L >= 1 && !masked && c_in % V == 0 && pitch_in % V == 0 && off_in % V == 0 && c_out % V == 0 &&
           pitch_out % V == 0 && off_out % V == 0 && AttnStreamLdsBytes(hd, f16) <= kAttnLdsBudget;
}
// the planner's default: tile 1 where it fits; else tile 2 where it fits and the sequence is long enough for 32-query workgroups to beat the
// generic kernel's one wave per query row (measured: DESIGN 3.28); else the generic kernel
constexpr int64_t kAttnStreamMinTokens = 128;
constexpr int AttnDefaultTile(int64_t L, int hd, bool f16, int64_t c_in, int64_t pitch_in, int64_t off_in, int64_t c_out, int64_t pitch_out, int64_t off_out,
                              bool masked = false) {
    if (AttnMfmaFits(L, hd, f16, c_in, pitch_in, off_in, c_out, pitch_out, off_out, masked)) return 1;
    return AttnStreamFits(L, hd, f16, c_in, pitch_in, off_in, c_out, pitch_out, off_out, masked) && L >= kAttnStreamMinTokens ? 2 : 0;
}
// tile 3: keys per chunk (a multiple of the 32-key tile), and the bytes of LDS of one chunk of K and V rows, every row padded by one 16-byte vector
// (fp32 hd 64: 2 * 256 * 272 = 136 KiB: one workgroup per CU)
constexpr int kAttnChunkKeys = 256;
constexpr int64_t AttnChunkLdsBytes(int hd, bool f16) { return 2 * int64_t(kAttnChunkKeys) * (int64_t(hd) * (f16 ? 2 : 4) + 16); }
constexpr bool AttnChunkFits(int64_t L, int hd, bool f16, int64_t c_in, int64_t pitch_in, int64_t off_in, int64_t c_out, int64_t pitch_out, int64_t off_out,
                             bool masked = false) {
    const int64_t V = f16 ? 8 : 4;
    return (hd == 32 || hd == 64) && L >= 1 && !masked && c_in % V == 0 && pitch_in % V == 0 && off_in % V == 0 && c_out % V == 0 && pitch_out % V == 0 &&
           off_out % V == 0 && AttnChunkLdsBytes(hd, f16) <= kAttnLdsBudget;
}
// a causal step: tile 1 where it fits, else tile 3 where it fits, else tile 2 where it fits (a wide head) and the sequence has at least
// kAttnStreamCausalMinTokens tokens, else the generic kernel.  The constant is the smallest measured length from which tile 2 wins in both
// precisions: the shortest one measured, one key tile.  A rotary head of 512 fits no form of tile 2: the planner takes that back
// (plan.cpp EmitAttention).  A non-causal step reaches tile 3 through IE_ATTN_TILE=3 only
constexpr int64_t kAttnStreamCausalMinTokens = 32;
constexpr int AttnCausalDefaultTile(int64_t L, int hd, bool f16, int64_t c_in, int64_t pitch_in, int64_t off_in, int64_t c_out, int64_t pitch_out, int64_t off_out) {
    if (AttnMfmaFits(L, hd, f16, c_in, pitch_in, off_in, c_out, pitch_out, off_out, false)) return 1;
    if (AttnChunkFits(L, hd, f16, c_in, pitch_in, off_in, c_out, pitch_out, off_out, false)) return 3;
    return AttnStreamFits(L, hd, f16, c_in, pitch_in, off_in, c_out, pitch_out, off_out, false) && L >= kAttnStreamCausalMinTokens ? 2 : 0;
}
bool AttentionEligible(const AttnArgs& a, int tile);
hipError_t LaunchAttention(const AttnArgs& a, int tile, hipStream_t stream);

// KV cache: append and one-token decode attention (kernels_decode.hip; generation with Llama-class graphs).  The cache tensors are fp32 in every
// precision and dense [N][kv_heads][rows][head_dim]: past_k / past_v with rows = past_len (null: no past), present_k / present_v with rows =
// past_len + new_len.  in = the qkv token rows [N, new_len, (H + 2 Hkv) hd] as AttnArgs describes them (float or half).
//   kv_append          present rows < past_len = the past rows, bit for bit; row past_len + l = k of token l after the rotary embedding (AttnArgs'
//                      arithmetic: full-width fp32 tables, fp32 products) resp. v of token l, converted to fp32
//   decode attention   new_len == 1: out[n, 0, h hd + e] = sum_j softmax_j(scale q[n, h] . K[n, h / g, j] + bias[n, j]) V[n, h / g, j, e] over the
//                      past_len + 1 rows j of present, q rotated like the new k; bias = (1 - float(mask[n, j])) * mask_value as AttnArgs' key mask, kept finite
//   extend attention   new_len >= 2 (chunked prefill into a cache): out[n, i, h hd + e] the same sum for new token i over the rows j <= past_len + i of
//                      present (causal inside the chunk by chunk index, whatever the positions are), q rotated at token i's own table row
// The rotation's table row of token l of image n is the token's own id pos[n pos_sn + l] (pos = the INT64 position_ids [N, new_len]; a negative value
// counts from the end) or l without pos, clamped into [0, rope_rows - 1] on the device: a caller that skips the host check cannot make a kernel read
// outside the tables.
struct DecodeArgs {
    TensorArg in, out;
    const float* past_k = nullptr;
    const float* past_v = nullptr;
    float* present_k = nullptr;
    float* present_v = nullptr;
    int heads = 0, kv_heads = 0, head_dim = 0;
    int past_len = 0, new_len = 1;
    float scale = 1.f;
    const int64_t* mask = nullptr;     // [N][past_len + new_len] rows at mask + n * mask_sn, or null
    int64_t mask_sn = 0;
    float mask_value = 0.f;
    const float* rope_cos = nullptr;   // [rope_rows][head_dim] or null
    const float* rope_sin = nullptr;
    int64_t rope_rows = 0;
    const int64_t* pos = nullptr;      // [N][new_len] rows at pos + n * pos_sn, or null
    int64_t pos_sn = 1;
    int splits = 1;                    // tile 4: key splits per (image, K / V head)
    float* workspace = nullptr;        // tile 4, splits > 1: the split records
    int64_t workspace_floats = 0;
    // In place (a model bound to a resident cache): cache_rows > 0.  past_k == present_k and past_v == present_v are the resident cache
    // [N][kv_heads][cache_rows][head_dim]; image n holds lens[n] valid rows and the step appends its first min(news[n], new_len) tokens at the rows
    // lens[n] + i; past_len stays the graph's P (the mask has P + new_len columns, the new tokens' at P + i).  Key j is visible to new token i iff
    // (j < lens[n] and mask[n][j]) or lens[n] <= j <= lens[n] + min(i, c - 1); no kernel reads a row at or beyond lens[n] + c.  The host keeps
    // lens[n] + c <= cache_rows; the kernels write no row at or beyond cache_rows whatever the arrays hold
    int64_t cache_rows = 0;
    const int* lens = nullptr;         // [N], device
    const int* news = nullptr;         // [N], device
};
// A decode step's tiles: 0 = attention_decode_generic_kernel (one wave per (image, query head) over `present`, which a kv_append launch wrote: any
// head_dim up to kDecodeMaxHeadDim, any past_len, float or half); kAttnDecodeTile (4) = attention_decode_kernel<T, HD, G>: a workgroup = (image, K / V
// head, key split) serves the g <= G query heads of its group, loads every cached K / V element once as 16-byte lanes, stores it into `present`,
// appends the new row in the last split; splits > 1: attention_decode_combine_kernel adds the split records in a fixed order.  Tiles 1-3 take no
// decode step.  Tile 0 of an extend step (new_len >= 2) is attention_extend_generic_kernel, one wave per (image, query head, new token) behind the
// kv_append launch (its other tile: kAttnExtendTile below).  DecodeKeyTile: the keys a workgroup of tile 4 loads per iteration (4 waves x 64 lanes x 4 floats / head_dim)
constexpr int kAttnDecodeTile = 4;
constexpr int kDecodeMaxHeadDim = 512;
constexpr int kDecodeMaxGroup = 8;
constexpr int kDecodeMaxSplits = 64;
constexpr int DecodeKeyTile(int hd) { return 1024 / hd; }
// tile 4 declines a mask whose bias is small enough to keep something of a score in an fp32 sum (|c| <= 2^24, e.g. -10000): tile 0 takes the image's
// largest bias out of every score first, as attention_generic_kernel<mask> does, and a split sees only its own keys
constexpr bool DecodeFastFits(int hd, int heads, int kv_heads, bool masked, float mask_value) {
    return (hd == 32 || hd == 64 || hd == 128) && kv_heads >= 1 && heads % kv_heads == 0 && heads / kv_heads <= kDecodeMaxGroup &&
           (!masked || mask_value < -16777216.f);
}
// floats of workspace the split records of tile 4 take: (m, l, o[hd]) per (image, query head, split)
constexpr int64_t DecodeWorkspaceFloats(int64_t n, int heads, int hd, int splits) { return splits > 1 ? n * heads * splits * (hd + 2) : 0; }
// the planner's split count: enough workgroups for two per CU of a 256-CU device from N * Hkv alone, each split at least kDecodeMinSplitKeys keys
// (and one key tile), at most kDecodeMaxSplits
constexpr int64_t kDecodeMinSplitKeys = 128;
// the planner's default tile of a decode step: tile 4 from this many keys (past_len + 1) on, where it fits.  Chosen as kAttnStreamCausalMinTokens was: the
// smallest measured length at which tile 4 beats the parts in both precisions, which is the smallest there is, past_len = 1
constexpr int64_t kAttnDecodeMinKeys = 2;
constexpr int DecodeDefaultSplits(int64_t n, int kv_heads, int64_t keys, int hd) {
    const int64_t groups = n * kv_heads, want = (512 + groups - 1) / groups;
    const int64_t tiles = (keys + DecodeKeyTile(hd) - 1) / DecodeKeyTile(hd), by_keys = keys / kDecodeMinSplitKeys;
    int64_t s = want;
    if (s > by_keys) s = by_keys;
    if (s > tiles) s = tiles;
    if (s > kDecodeMaxSplits) s = kDecodeMaxSplits;
    return s < 1 ? 1 : int(s);
}
// An extend step's tiles: 0 = the generic pair above; kAttnExtendTile (5) = a kv_append launch, then attention_extend_kernel<T, HD>: a workgroup = (image,
// K / V head, block of 128 query rows, key split) over the fp32 `present`, the g Lq query rows of the group ordered (new token, head-in-group), K / V
// staged through LDS in chunks of kAttnChunkKeys keys (converted to half in fp16 mode) with the chunk's key biases beside them, MFMA as in tiles 1 and
// 3; splits > 1: attention_extend_combine_kernel adds the split records in a fixed order.  No other tile takes an extend step.  head_dim 32 or 64, a
// group of at most kDecodeMaxGroup heads, and DecodeFastFits' rule for the mask constant (a small one stays on tile 0)
constexpr int kAttnExtendTile = 5;
constexpr bool ExtendFastFits(int hd, int heads, int kv_heads, bool masked, float mask_value) {
    return (hd == 32 || hd == 64) && masked && DecodeFastFits(hd, heads, kv_heads, masked, mask_value);
}
// LDS of tile 5: tile 3's chunk of K and V rows plus one bias per key of the chunk
constexpr int64_t ExtendLdsBytes(int hd, bool f16) { return AttnChunkLdsBytes(hd, f16) + 4 * int64_t(kAttnChunkKeys); }
static_assert(ExtendLdsBytes(64, false) <= kAttnLdsBudget && ExtendLdsBytes(64, true) <= kAttnLdsBudget, "tile 5's chunk fits the LDS budget");
// floats of workspace the split records of tile 5 take: tile 4's per new token
constexpr int64_t ExtendWorkspaceFloats(int64_t n, int heads, int hd, int splits, int64_t lq) { return DecodeWorkspaceFloats(n, heads, hd, splits) * lq; }
// the planner's split count of tile 5: DecodeDefaultSplits' rule with groups = N * Hkv * row blocks (128 query rows each) and 32-key tiles, but for one
// workgroup per CU of a 256-CU device, not two: a split here costs a record per query row, and the sweeps of DESIGN 3.33 have their minima lower
constexpr int ExtendDefaultSplits(int64_t n, int kv_heads, int64_t rows, int64_t keys) {
    const int64_t groups = n * kv_heads * ((rows + 127) / 128), want = (256 + groups - 1) / groups;
    const int64_t tiles = (keys + 31) / 32, by_keys = keys / kDecodeMinSplitKeys;
    int64_t s = want;
    if (s > by_keys) s = by_keys;
    if (s > tiles) s = tiles;
    if (s > kDecodeMaxSplits) s = kDecodeMaxSplits;
    return s < 1 ? 1 : int(s);
}
// the planner's default tile of an extend step: tile 5 from this many query rows g * Lq on, where it fits: the smallest measured count at which tile 5
// beats the generic pair in both precisions
constexpr int64_t kAttnExtendMinRows = 2;
hipError_t InitKernelsDecode();          // once per process, before any capture: lets tile 5 take more than 64 KiB of LDS
bool KvAppendEligible(const DecodeArgs& a);
hipError_t LaunchKvAppend(const DecodeArgs& a, hipStream_t stream);
bool AttentionDecodeEligible(const DecodeArgs& a, int tile);
hipError_t LaunchAttentionDecode(const DecodeArgs& a, int tile, hipStream_t stream);
hipError_t InitKernelsAttn();            // once per process, before any capture: lets the MFMA kernels take more than 64 KiB of LDS

// Attention inside (shifted) windows of a channels-last map (kernels_wattn.hip; Swin).  in = the qkv map [N, H, W, 3 D], out = [N, H, W, D].  The map is
// rolled by (-sh, -sw) cyclically and cut into windows of wh x ww pixels; window (wy, wx) holds the L = wh ww tokens t = ty ww + tx at the rolled
// pixel (wy wh + ty, wx ww + tx), i.e. the map's own pixel ((wy wh + ty + sh) mod H, (wx ww + tx + sw) mod W).  Per window and head
//   out[pixel(i), h hd + e] = sum_j softmax_j(scale q_i . k_j + bias[h][i][j] + mask[window][i][j]) v[j, e]
// and every result lands on the pixel its query came from: roll, partition, reverse and roll-back are index arithmetic, never a copy.
// Tables (fp32 in every precision, packed by the planner): Lp = L rounded up to whole 32-key tiles; bias[h][j][i] and mask[window][j][i] are
// [.][Lp][Lp] with the QUERY index fastest; padded keys (j >= L) hold -inf in the bias table and 0 in the mask table, padded queries 0.
struct WinAttnArgs {
    TensorArg in, out;
    int heads = 0, head_dim = 0;
    float scale = 1.f;
    int wh = 0, ww = 0, sh = 0, sw = 0;
    const float* bias = nullptr;       // [heads][Lp][Lp]
    const float* mask = nullptr;       // [nW][Lp][Lp] or null
};
// tile 0: window_attention_generic_kernel (one wave per query row; any window, shift, head_dim, pitch, offset; float or half).  tile 1:
// window_attention_mfma_kernel<T, 32> (one wave per (image, window, head), four per workgroup; K and V of the window in LDS): head_dim 32, at most
// 64 tokens per window, channel counts, pitches and offsets multiples of the 16-byte vector
constexpr int kNumWinAttnTiles = 2;
constexpr int kWinAttnMaxTokens = 64;
constexpr int64_t WinAttnPaddedTokens(int64_t L) { return (L + 31) / 32 * 32; }
constexpr bool WinAttnMfmaFits(int64_t L, int hd, bool f16, int64_t c_in, int64_t pitch_in, int64_t off_in, int64_t c_out, int64_t pitch_out, int64_t off_out) {
    const int64_t V = f16 ? 8 : 4;
    return hd == 32 && L >= 1 && L <= kWinAttnMaxTokens && c_in % V == 0 && pitch_in % V == 0 && off_in % V == 0 && c_out % V == 0 && pitch_out % V == 0 &&
           off_out % V == 0;
}
bool WindowAttentionEligible(const WinAttnArgs& a, int tile);
hipError_t LaunchWindowAttention(const WinAttnArgs& a, int tile, hipStream_t stream);
hipError_t InitKernelsWattn();           // once per process, before any capture: the fp32 MFMA kernel takes 72 KiB of LDS

// Patch merging (kernels_wattn.hip; Swin): out[n, y, x, k C + c] = in[n, 2 y + (k & 1), 2 x + (k >> 1), c] for k = 0 ... 3 (torchvision's channel
// order x[0::2, 0::2], x[1::2, 0::2], x[0::2, 1::2], x[1::2, 1::2]); in [N, H, W, C] with even H and W, out [N, H/2, W/2, 4 C].  One thread per 16-byte
// vector where C, the pitches and the offsets allow (PatchMergeVec), else one per element.
struct PatchMergeArgs {
    TensorArg in, out;
};
constexpr bool PatchMergeVec(bool f16_in, bool f16_out, int64_t c, int64_t pitch_in, int64_t off_in, int64_t pitch_out, int64_t off_out) {
    const int64_t V = f16_out ? 8 : 4;
    return f16_in == f16_out && c % V == 0 && pitch_in % V == 0 && off_in % V == 0 && pitch_out % V == 0 && off_out % V == 0;
}
hipError_t LaunchPatchMerge(const PatchMergeArgs& a, hipStream_t stream);

// Class token and position embedding (kernels_tokens.hip): out[n, 0, :] = cls + pos[0], out[n, 1 + p, :] = in[n, p, :] + pos[1 + p]; cls [D] and
// pos [L0 + 1][D] (or null) fp32.  16-byte vectors where D, the pitches and the bases allow, else one element per thread.
struct TokenAssembleArgs {
    TensorArg in, out;                 // in.w = L0 tokens of D = in.c channels; out.w = L0 + 1
    const float* cls = nullptr;
    const float* pos = nullptr;
};
hipError_t LaunchTokenAssemble(const TokenAssembleArgs& a, hipStream_t stream);
bool TokenAssembleVectorised(const TokenAssembleArgs& a);

// Squeeze-and-excitation block (kernels_se.hip): out = in * gate[n, c], gate = act(W2^T-packed FC(act1(W1 * mean_hw(in) + b1)) + b2).
// Three phases, four launches: squeeze (fp32 partial sums per pixel chunk), fc1 (means + FC1 + act1 -> hidden [N][mid]), fc2 (FC2 + act -> gate [N][C]),
// apply.  Deterministic (fixed summation orders, no atomics).  The workspace holds chunks * N * C partials, N * mid hidden values and the N * C gate.
struct SeArgs {
    TensorArg in, out;                 // NHWC, same shape; out may be a channel slice
    const float* w1 = nullptr;         // [mid][C]
    const float* b1 = nullptr;         // [mid] or null
    const float* w2t = nullptr;        // [mid][C] (FC2's [C][mid] transposed)
    const float* b2 = nullptr;         // [C] or null
    int mid = 0;
    int act1 = 0, act = 0;             // ApplyAct codes of the inner activation and of the gate
    float act1_a = 0.f, act1_b = 0.f, act_a = 0.f, act_b = 0.f;
    int chunks = 1;                    // pixel chunks of the squeeze (SeSqueezeChunks)
    float* workspace = nullptr;
    int64_t workspace_floats = 0;
};
// Pixel chunks of the squeeze: enough (image, chunk) workgroups to fill the chip on large maps, at least 64 pixels per chunk
inline int SeSqueezeChunks(int64_t n, int64_t hw) {
    int64_t want = (1024 + n - 1) / n;
    int64_t by_px = hw / 64;
    int64_t c = want < by_px ? want : by_px;
    return int(c < 1 ? 1 : (c > 64 ? 64 : c));
}
inline int64_t SeWorkspaceFloats(int64_t n, int64_t c, int64_t mid, int chunks) { return int64_t(chunks) * n * c + n * mid + n * c + 64; }
bool SqueezeExciteEligible(const SeArgs& a);
hipError_t LaunchSqueezeExcite(const SeArgs& a, hipStream_t stream);
// the phases one by one (profiling / scripts): 0 squeeze, 1 fc1, 2 fc2, 3 apply
hipError_t LaunchSqueezeExcitePhase(const SeArgs& a, int phase, hipStream_t stream);

// vec: 1 = float4 NHWC operand staging, 0 = scalar gather staging.  tile: index into kIgemmTiles.
// splitk > 1: the K-tiles are divided over grid.y workgroups that write partial slabs to a.workspace; the slabs are
// combined inside the same launch by the last-arriving workgroup of each tile (a.counters != null) or by a second
// kernel (a.counters == null).  Both sum in slice order: deterministic, no float atomics.
bool SplitKWorkspaceOk(int64_t workspace_floats, int num_counters, int splitk, int64_t num_tiles, int tile_elems);
// Resize / Upsample (kernels_resize.hip): out(n, c, y, x) = in(n, c, f(y), g(x)) interpolated per axis, in NHWC (sc == 1, any pitch; h = w = 1
// broadcasts), out NHWC (sc == 1) or dense NCHW (sw == 1: the graph output).  fp32 or half elements, fp32 interpolation math; the source
// coordinate is computed in double from the ONNX formulas, so nearest-pixel ties break as the spec's reference does.
struct ResizeArgs {
    TensorArg in, out;
    int mode = 0;                      // plan.h ResizeMode: 0 nearest, 1 linear
    int coord = 0;                     // ResizeCoord: 0 half_pixel, 1 pytorch_half_pixel, 2 align_corners, 3 asymmetric
    int nearest = 0;                   // ResizeNearest: 0 round_prefer_floor, 1 round_prefer_ceil, 2 floor, 3 ceil
    double scale_h = 1.0, scale_w = 1.0;
};
// path 0: the generic kernel (one thread per output element); 1: 16-byte channel vectors NHWC -> NHWC; 2: NHWC -> NCHW, one thread per output
// pixel looping over the channels (stores coalesced along W).  ResizePath picks the fastest one the operands allow.
int ResizePath(const ResizeArgs& a);
hipError_t LaunchResize(const ResizeArgs& a, int path, hipStream_t stream);
hipError_t LaunchConvIgemm(const ConvArgs& a, int tile, int vec, int splitk, hipStream_t stream);
// 3x3 / stride 1 / pad 1 with an LDS-resident input window (see kernels.hip).  tile: 0..kNumConvRasterTiles-1.
constexpr int kNumConvRasterTiles = 8;
bool ConvRasterEligible(const ConvArgs& a, int tile);
int ConvRasterTileBn(int tile);
hipError_t LaunchConvRaster3x3(const ConvArgs& a, int tile, int splitk, hipStream_t stream);
hipError_t LaunchConvNaive(const ConvArgs& a, hipStream_t stream);
// fp16 precision mode (kernels_f16.hip): NHWC half activations + half weights on v_mfma_f32_32x32x16_f16, fp32 accumulate,
// fp32 scale/shift/bias; output half or float.  Same tile table as the fp32 igemm (entries with deep == 0).
// second pass of a two-pass split-K conv: out = act(sum of a.workspace slabs + bias)
hipError_t LaunchSplitKReduce(const ConvArgs& a, int splitk, hipStream_t stream);
hipError_t LaunchConvIgemmF16(const ConvArgs& a, int tile, int splitk, hipStream_t stream);
hipError_t InitKernelsF16();
// fp16 weights-stationary 1x1 conv (kernels_ws.hip): weights in LDS once per persistent workgroup, activations streamed
// from HBM straight into MFMA fragments.  tile % 6 = {output channels per workgroup, waves}; tile / 6 = 0: persistent workgroups
// with an even number of row blocks per wave, 1: one row block per wave (the hardware's workgroup dispatch balances the load),
// 2 (fp16 only, tiles 12-17): ONE persistent workgroup per CU -- fewer, longer streams: 10-15 % faster than the fuller grid on DenseNet's
// block-1 / block-2 shapes at batch 128 (scripts/probes/ws_probe.cpp -DWS_PER_CU), the search decides per shape.
constexpr int kNumConvWsTiles = 12;
constexpr int kNumConvWs16Tiles = 18;
bool ConvWsEligible(const ConvArgs& a, int tile);
hipError_t LaunchConvWs1x1F16(const ConvArgs& a, int tile, hipStream_t stream);
hipError_t InitKernelsWs();
// fp32 twin (kernels_ws32.hip): same tile table, v_mfma_f32_32x32x2_f32, float in / float out; two more tiles (12, 13) are the
// K-split variants (8 / 4 waves of a workgroup share one row block and split K, partial tiles summed through LDS); 14-19: shapes 0-5 on a grid
// of ONE persistent workgroup per CU (as the fp16 tiles 12-17)
constexpr int kNumConvWs32Tiles = kNumConvWsTiles + 2 + 6;
bool ConvWs32Eligible(const ConvArgs& a, int tile);
hipError_t LaunchConvWs1x1F32(const ConvArgs& a, int tile, hipStream_t stream);
hipError_t InitKernelsWs32();
// fp16 weights-stationary 3x3/s1/p1 conv (Cout <= 32, all weights of the layer resident in LDS, raster window per 64-channel slice)
constexpr int kNumConvWs3Tiles = 5;
bool ConvWs3Eligible(const ConvArgs& a, int tile);
hipError_t LaunchConvWs3x3F16(const ConvArgs& a, int tile, hipStream_t stream);
hipError_t InitKernelsWs3();
// "Direct split-K" conv for small output grids (kernels_direct.hip): K split over the waves of a workgroup, both operands loaded
// straight from global memory into MFMA fragments (all at once), partial tiles summed through LDS.  fp32 and fp16.
constexpr int kNumDirectBaseTiles = 6;     // tiles 0..5: both operands straight from global memory
constexpr int kNumConvDirectTiles = 15;    // tiles 6..9: "window" variants (fp32, 16x16x4 MFMA tiles): activations through LDS, fragment-major weights
                                           // tiles 10..14: activations-stationary 1x1 (fp32): 32 / 16 pixel rows in LDS, weights streamed from the mirror
hipError_t LaunchPermuteWeightsFrag(const float* src, float* dst, int Cout, int KK, int Cin, hipStream_t stream);
bool ConvDirectEligible(const ConvArgs& a, int tile);
hipError_t LaunchConvDirect(const ConvArgs& a, int tile, hipStream_t stream);
hipError_t InitKernelsDirect();
// DenseNet transition in one launch (fp32, kernels_trans.hip): conv1x1_pooled_kernel = conv1x1_as_kernel whose staging loop builds each LDS row from the 2x2 /
// stride-2 window of the pool step in front of the conv (with the pool's BN + ReLU prologue), optionally followed by a second 1x1 conv (the next
// dense block's entry conv, 128 output channels) on the tile just stored.  `a` is the conv step's argument set (a.in = the pooled view: shape
// only, never read; no prologue of its own), PooledArgs carries the pool's operands and the second conv's, the way FusedArgs carries the 3x3's.
struct PooledConsts {
    unsigned mg20_ow = 0, mg20_oh = 0;     // ceil(2^20 / d): output width / height (per-lane quotients with a 24-bit multiply)
    unsigned mg32_ohw = 0, mg32_ow = 0;    // floor(2^32 / d): output pixels per image / output width (wave-uniform quotients, one correction step)
};
struct PooledArgs {
    TensorArg pin;                     // the pool's input: NHWC channel slice at twice the conv's resolution
    const float* pool_scale = nullptr; // the pool's prologue (x * scale + shift, then ReLU if pool_relu), or null
    const float* pool_shift = nullptr;
    int pool_relu = 0;
    // chained second conv: in = the first conv's output view, prologue scale2 / shift2 (always present), 16 output channels per wave
    TensorArg out2;
    const float* wfrag2 = nullptr;
    const float* bias2 = nullptr;
    const float* scale2 = nullptr;
    const float* shift2 = nullptr;
    int pre_relu2 = 0, relu2 = 0;
    PooledConsts k;                    // filled by LaunchConvPooled
};
// tiles 0..4 = conv1x1_as_kernel's shapes {waves, 16-channel blocks per wave, 16-pixel blocks}: {8,1,2} {4,1,2} {8,2,2} {4,1,1} {2,2,1}; tiles 0 and 2
// (128 / 256 channels per workgroup) can chain; tile 5 = {1,1,2}: 16 channels per workgroup, for channel counts that are no multiple of 64; tiles 6 / 7 =
// {8,1,1} / {8,2,1}: the two chain shapes on 16-pixel blocks
constexpr int kNumConvPooledTiles = 8;
// by shapes alone (no device): K input channels, cout output channels, the chained conv's cout2
bool ConvPooledShapeOk(int tile, bool chain, int64_t k, int64_t cout, int64_t cout2);
bool ConvPooledEligible(const ConvArgs& a, const PooledArgs& p, int tile, bool chain);
hipError_t LaunchConvPooled(const ConvArgs& a, const PooledArgs& p, int tile, bool chain, hipStream_t stream);
hipError_t InitKernelsTrans();
// Stem conv (7x7 / stride 2 / pad 3, Cin = 3, Cout <= 64) straight from the dense NCHW fp32 graph input (kernels_stem.hip);
// half arithmetic + half output in fp16 mode, fp32 otherwise.
// Workgroups of `kernel` (block threads, lds dynamic LDS bytes) one CU holds, from the occupancy API (registers included), cached.
int ResidentPerCu(const void* kernel, int block, size_t lds);

bool ConvStemEligible(const ConvArgs& a);
hipError_t LaunchConvStem(const ConvArgs& a, hipStream_t stream);
// The stem AND the 3x3 / stride 2 / pad 1 max pool behind it in one launch: `a` is the stem's argument set with out = the POOLED tensor.
bool ConvStemPoolEligible(const ConvArgs& a);
hipError_t LaunchConvStemPool(const ConvArgs& a, hipStream_t stream);
hipError_t InitKernelsStem();
// Winograd F(2x2, 3x3) conv (kernels_wino.hip): fp32, 3x3 / stride 1 / pad 1, 32 output channels, even H and W; a.wfrag = the transformed
// weights U (16 x Cout x Cin floats, fragment-major) built by LaunchWinogradWeights.  tile: 0..3 = output tiles per workgroup.
constexpr int kNumConvWinoTiles = 12;       // output tiles per workgroup: 4x7, 2x14, 4x8, 2x16; 0..3 four waves, 4..7 eight waves, 8..11 eight waves with bf16x6 products (need `w16` = LaunchWinogradWeightsX6's mirror)
bool ConvWinoEligible(const ConvArgs& a, int tile);
hipError_t LaunchConvWino3x3(const ConvArgs& a, int tile, hipStream_t stream);
hipError_t LaunchWinogradWeights(const float* w, float* u, int Cout, int Cin, hipStream_t stream);
hipError_t LaunchWinogradWeightsX6(const float* w, void* dst, int Cout, int Cin, hipStream_t stream);      // 3 x 16 x Cout x Cin bf16
hipError_t InitKernelsWino();
// fp32 1x1 conv on the bf16 matrix pipe with exactly split operands (kernels_x6.hip; opt-in, IE_FP32_SPLIT=1): `w16` points at the three
// bf16 planes LaunchSplitWeightsX6 built from the conv's fp32 weights.  tile 0: 64 pixels per workgroup, 1: 32.
constexpr int kNumConvX6Tiles = 2;
bool ConvX6Eligible(const ConvArgs& a, int tile);
hipError_t LaunchConvX6(const ConvArgs& a, int tile, hipStream_t stream);
hipError_t LaunchSplitWeightsX6(const float* w, void* dst, int Cout, int K, hipStream_t stream);
hipError_t InitKernelsX6();
// Fused dense-layer step (fp32): 3x3 growth conv of layer L + 1x1 bottleneck conv of layer L+1 per 16*pb-pixel tile, one launch.
// tile: 1 / 2 = 16-pixel blocks per workgroup; 3 = 16-pixel tiles, two workgroups per CU (<= 128 VGPRs, <= 80 KB LDS);
// 4 / 5 = wave-specialised variant (3x3 and 1x1 run concurrently on different waves), 16 / 32 pixels;
// 6 = 16-pixel tiles on a two-row grid: row h recomputes the 3x3 and owns output channels [64h, 64h + 64) of the 1x1 (maps too small to fill the CUs)
constexpr int kNumConvDenseFusedTiles = 6;      // tiles 1..6; 0 = the two plain launches
bool ConvDenseFusedEligible(const ConvArgs& a, const FusedArgs& f, int tile);
hipError_t LaunchConvDenseFused(const ConvArgs& a, const FusedArgs& f, int tile, hipStream_t stream);
hipError_t InitKernelsFused();
// fp16 mode: a chain of dense layers (BN -> ReLU -> 1x1 conv K -> 128 -> BN -> ReLU -> 3x3 conv 128 -> 32) per launch, one workgroup per image, the
// bottleneck tensor kept in LDS (kernels_block.hip).  Weights come from a fragment-major mirror of the half blob (LaunchPermuteWeightsFrag16).
struct DenseBlockLayer {
    int K = 0;                         // input channels of the 1x1 (multiple of 32, >= 64): channels [in_coff, in_coff + K) of the pixel row
    int out_coff = 0;                  // where the 32 new channels go in the pixel row
    unsigned w1 = 0, w3 = 0;           // element offsets into wfrag16: fragment-major [128][K] and [32][9 * 128] half weights
    unsigned ps = 0xffffffffu, pt = 0xffffffffu;   // element offsets into w16 of the 1x1's prologue scale / shift (halfs), 0xffffffff = none
    unsigned b1 = 0xffffffffu, b3 = 0xffffffffu;   // float offsets into w32 of the two biases, 0xffffffff = none
    int flags = 0;                     // 1: ReLU in the prologue, 2: ReLU after the 1x1, 4: ReLU after the 3x3
};
constexpr int kMaxBlockLayers = 24;
struct DenseBlockArgs {
    _Float16* x = nullptr;             // block buffer, NHWC halfs
    int pitch = 0, in_coff = 0;        // halfs per pixel row; first channel the 1x1 convs read
    int n = 0, h = 0, w = 0;
    const _Float16* wfrag16 = nullptr;
    const _Float16* w16 = nullptr;
    uint64_t w16_bytes = 0;            // size of each of the two half blobs (buffer descriptors: < 2 GiB)
    const float* w32 = nullptr;
    int nlayers = 0;
    int band_rows = 0;                 // set by the launcher: 0 = a workgroup per image, else image rows per workgroup (band mode) / per step (strip mode)
    int strip_rows = 0;                // set by the launcher: > 0 = strip mode: image rows per workgroup, walked in steps of band_rows
    long long* dbg = nullptr;          // probes only: per-phase cycle sums of workgroup 0 / wave 0 (1x1 loop, weight DMA + 1x1 epilogue, 3x3, closing barrier)
    DenseBlockLayer layer[kMaxBlockLayers];
};
bool DenseBlockEligible(const DenseBlockArgs& a);
hipError_t LaunchDenseBlockF16(const DenseBlockArgs& a, hipStream_t stream);
hipError_t LaunchPermuteWeightsFrag16(const void* src, void* dst, int rows, int K, hipStream_t stream);
hipError_t InitKernelsBlock();
// fp8 precision mode (kernels_f8.hip): implicit GEMM on v_mfma_f32_32x32x16_fp8_fp8 over e4m3 NHWC activations and e4m3 weights,
// fp32 accumulate, per-channel rescale + bias + e4m3 shortcut + ReLU + re-quantisation in the epilogue.  Tiles 0..6 of kIgemmTiles.
constexpr int kNumConvF8Tiles = 7;
bool ConvF8Eligible(const ConvArgs& a, int tile);
hipError_t LaunchConvIgemmF8(const ConvArgs& a, int tile, hipStream_t stream);
hipError_t InitKernelsF8();
// fp8 weights-stationary 1x1 conv (kernels_ws8.hip): weights + epilogue constants in LDS, activations streamed from HBM into MFMA fragments;
// with a.in2 set also the projection shortcut's GEMM in the same launch.  tile: {N tiles of 32 per workgroup, waves} = {8,8} {4,8} {2,8} {4,4} {2,4}
constexpr int kNumConvWs8Tiles = 10;       // 5 tile shapes x {grid sized for two workgroups per CU, for one (tiles 5-9)}
bool ConvWs8Eligible(const ConvArgs& a, int tile);
hipError_t LaunchConvWs1x1F8(const ConvArgs& a, int tile, hipStream_t stream);
hipError_t InitKernelsWs8();
// fp8 weights-stationary 3x3/s1/p1 conv (kernels_ws8.hip): all weights of a 32-channel N tile resident in LDS, raster window per 128-channel slice
constexpr int kNumConvWs38Tiles = 8;      // 4 tile shapes x {grid sized by LDS (<= two workgroups per CU), one workgroup per CU (tiles 4-7)}
// fp8 plans: Step::tile of an IgemmF8 step (and its tune-file code) names the kernel: t < kWs8Code is tile t of conv_igemm_f8, kWs8Code + t tile t
// of the weights-stationary 1x1 kernel (a DualF8 step's tile too), kWs38Code + t tile t of the weights-stationary 3x3
constexpr int kWs8Code = 100;
constexpr int kWs38Code = 200;
bool ConvWs38Eligible(const ConvArgs& a, int tile);
hipError_t LaunchConvWs3x3F8(const ConvArgs& a, int tile, hipStream_t stream);
// w8[o, :] = e4m3(w[o, :] / wscale[o]) with wscale[o] = max|w[o, :]| / 448, one workgroup per row
hipError_t LaunchQuantizeRowsE4m3(const float* w, void* w8, float* wscale, int rows, int K, hipStream_t stream);
hipError_t LaunchScaleVector(const float* src, float* dst, float s, int n, hipStream_t stream);
hipError_t LaunchPoolF8(const PoolArgs& a, hipStream_t stream);
hipError_t LaunchGlobalAvgPoolF8(const TensorArg& in, const TensorArg& out, float in_scale, hipStream_t stream);
// calibration: *result = max(*result, max |x| over the view) (fp32 / half views; *result must start at 0)
hipError_t LaunchAbsMax(const TensorArg& t, float* result, hipStream_t stream);
hipError_t LaunchE4m3RoundTrip(const float* src, float* dst, void* codes, float scale, int64_t n, hipStream_t stream);
hipError_t LaunchConvertF32ToF16(const float* src, void* dst, int64_t n, hipStream_t stream);
// UINT8 ingest: dst[i] = float(src[i]) * scale + bias (images travel over PCIe as bytes, 4x fewer than fp32)
hipError_t LaunchConvertU8ToF32(const void* src, float* dst, int64_t n, float scale, float bias, hipStream_t stream);
hipError_t LaunchPool(const PoolArgs& a, hipStream_t stream);
// out[n, c] = mean over (y, x) of f(in[n, y, x, c]),  f = optional scale/shift/ReLU prologue
// then ApplyAct(pre_act, pre_act_a, pre_act_b, .) before the mean
hipError_t LaunchGlobalAvgPool(const TensorArg& in, const TensorArg& out, const float* pre_scale, const float* pre_shift,
                               int pre_relu, hipStream_t stream, int pre_act = 0, float pre_act_a = 0.f, float pre_act_b = 0.f);
hipError_t LaunchEltwise(const EltArgs& a, hipStream_t stream);
hipError_t LaunchCopy(const TensorArg& in, const TensorArg& out, hipStream_t stream);
// result[i] = a[i] + b[i]  (the reference's only authored kernel: cuda_utils.cu:10-15)
hipError_t LaunchVectorAdd(const float* a, const float* b, float* result, int64_t n, hipStream_t stream);

// Calibration: achievable fp32 MFMA rate of this device (register-resident loop, no memory traffic).
double MfmaPeakTflops(int nacc, int blocks_per_cu, int iters);

// One-time per-process setup (raises the dynamic-LDS limit of the igemm kernels).
hipError_t InitKernels();

}  // namespace ie
