// Graph planner: ONNX graph -> fused NHWC execution plan (host-only code, no HIP).
//
// This is the part of `Ort::Session` construction the reference relies on at model.cpp:843-847
// (parse + ORT_ENABLE_ALL graph optimisation, model.cpp:896) re-designed for MI355X:
//   * activations live in NHWC buffers (channels contiguous -> coalesced 16 B/lane HBM access)
//   * BatchNormalization is folded to per-channel scale/shift at load and fused either into the
//     producing conv's weights/bias (Conv->BN->ReLU) or into the consuming conv's operand staging
//     (DenseNet's pre-activation BN->ReLU->Conv)
//   * Concat(axis=1) is free: producers write into channel slices of one planned buffer
//   * dead activation buffers are recycled so the working set stays inside the 256 MiB Infinity Cache
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "onnx_reader.h"

namespace ie {

// An activation tensor inside a device buffer.  NHWC unless `nchw` (graph inputs/outputs as the ABI hands them).
struct View {
    int buf = -1;
    int64_t n = 0, c = 0, h = 1, w = 1;
    int64_t c_off = 0;    // first channel inside the buffer's pixel row
    int64_t pitch = 0;    // floats per pixel row of the buffer (>= c_off + c)
    bool nchw = false;    // dense NCHW (pitch/c_off unused)
    bool f16 = false;     // elements are IEEE halfs (fp16 precision mode: every buffer that is not a graph input/output)
    bool f8 = false;      // elements are OCP e4m3 bytes with one per-tensor scale (fp8 precision mode: spatial tensors between stem and global pool)
    bool i64 = false;     // elements are int64 (an INT64 graph input [N, L]: token / type ids; only an embed step reads one)
    int64_t numel() const { return n * c * h * w; }
    int esize() const { return i64 ? 8 : (f8 ? 1 : (f16 ? 2 : 4)); }
};

// Storage/compute precision of a plan.  F16: activations between the graph's fp32 inputs and outputs are stored as halfs and
// the convolutions run on the fp16 MFMA path with fp32 accumulation (BASELINE.json configs[2-3]); folded BN scale/shift,
// biases and split-K partial sums stay fp32.
// F8 (BASELINE.json configs[4]): spatial activations are stored as OCP e4m3 with a per-tensor scale calibrated at load, conv weights
// as e4m3 with a per-output-channel scale, the convolutions run on the fp8 MFMA path with fp32 accumulation; [N, C] vectors (after
// the global pool) are halfs, graph inputs / outputs stay fp32.
enum class Precision : int { F32 = 0, F16 = 1, F8 = 2 };

enum class StepKind : int { Conv = 0, Pool = 1, GlobalAvgPool = 2, Eltwise = 3, Copy = 4, SqueezeExcite = 5, Resize = 6, LayerNorm = 7, TokenAssemble = 8, Attention = 9, WindowAttention = 10, PatchMerge = 11, Embed = 12, GroupNorm = 13, KvAppend = 14 };

// Resize / Upsample (kernels_resize.hip): the interpolation mode, the ONNX coordinate_transformation_mode and nearest_mode
enum class ResizeMode : int { Nearest = 0, Linear = 1 };
enum class ResizeCoord : int { HalfPixel = 0, PytorchHalfPixel = 1, AlignCorners = 2, Asymmetric = 3 };
enum class ResizeNearest : int { RoundPreferFloor = 0, RoundPreferCeil = 1, Floor = 2, Ceil = 3 };

// Pointwise activation fused into a step (kernels.h ApplyAct): sigmoid(x), hardsigmoid(x) = max(0, min(1, a*x + b)), silu(x) = x * sigmoid(x),
// hardswish(x) = x * hardsigmoid(x; a, b) (the ONNX HardSwish op: a = 1/6, b = 1/2).  Relu only as a squeeze-excite block's inner activation.
// gelu(x) = 0.5 * x * (1 + erf(x / sqrt 2)) (the ONNX Gelu op, or the five-node Erf pattern exporters write below opset 20); GeluTanh its tanh
// approximation (Gelu with approximate = "tanh").
enum class ActKind : int { None = 0, Sigmoid = 1, HardSigmoid = 2, Silu = 3, HardSwish = 4, Relu = 5, Gelu = 6, GeluTanh = 7, Tanh = 8 };
struct Act {
    ActKind kind = ActKind::None;
    float a = 0.f, b = 0.f;
    bool operator==(const Act& o) const { return kind == o.kind && a == o.a && b == o.b; }
};

// Conv algorithm chosen at plan time.
enum class ConvAlgo : int {
    IgemmVec = 0,     // MFMA implicit GEMM, NHWC float4 operand staging (Cin % 4 == 0)
    IgemmScalar = 1,  // MFMA implicit GEMM, scalar gather staging (any Cin / NCHW input, e.g. the 7x7 stem)
    Naive = 2,        // one thread per output element (tiny or odd shapes, and on-device cross-check)
    Raster3x3 = 3,    // 3x3/s1/p1 MFMA conv with an LDS-resident input window (nine shifted GEMMs over a padded raster)
    Ws1x1 = 4,        // weights-stationary 1x1/s1 conv (fp32 and fp16), activations streamed from HBM into MFMA fragments
    Ws3x3 = 5,        // fp16 mode: weights-stationary 3x3/s1/p1 conv (Cout <= 32), raster window in LDS
    Stem = 6,         // 7x7/s2/p3 conv over the 3-channel NCHW fp32 graph input: LDS window per output tile, weights resident
    Direct = 7,       // small output grids: K split over the waves of a workgroup, operands loaded straight into MFMA fragments
    IgemmF8 = 8,      // fp8 mode: implicit GEMM over e4m3 activations / weights (v_mfma_f32_32x32x16_fp8_fp8)
    DenseFused = 9,   // fp32: 3x3 growth conv of dense layer L + 1x1 bottleneck conv of layer L+1 in one launch (Step::parts holds the two convs)
    Wino3x3 = 10,     // fp32: Winograd F(2x2, 3x3) for 3x3/s1/p1 convs with 32 output channels on even-sized images (2.25x fewer MACs)
    X6 = 11,          // fp32 1x1 conv on the bf16 matrix pipe with exactly split operands (kernels_x6.hip; opt-in IE_FP32_SPLIT=1)
    DenseBlock = 12,  // fp16: a chain of dense layers (1x1 K -> 128, 3x3 128 -> 32) in ONE launch, one workgroup per image, the bottleneck tensor
                      // kept in LDS (kernels_block.hip).  Step::parts = the 2n conv steps as the planner emitted them; tile 1 = fused, 0 = the parts
    StemPool = 14,    // the stem conv AND the 3x3/s2/p1 max pool behind it in one launch (conv_stem_kernel<POOL>, kernels_stem.hip): the conv
                      // tile is pooled in LDS, the tensor between the two ops never exists.  Step::parts = {conv, pool}; tile 1 = fused, 0 = the parts
    DualF8 = 13,      // fp8: a bottleneck block's last 1x1 conv AND the projection conv of its shortcut as two GEMMs of one launch (kernels_ws8.hip):
                      // the shortcut tensor never exists.  Step::parts = {projection conv, last conv}; this step's own fields repeat the last
                      // conv's with has_in2 cleared.  The fp16 plan built for the fp8 calibration carries the same step and runs its parts.
    Depthwise = 15,   // group == Cin == Cout conv (kernels_dw.hip): weights [C][kh][kw]; tile 0 = the generic kernel, 1-3 = 16-byte channel vectors with
                      // 1 / 2 / 4 output pixels per lane.  Epilogue clamp [lo, hi] (a fused Clip) and prologue bound pre_hi (ReLU6 in front of it)
    Grouped = 16,     // any other group > 1 (kernels_grouped.hip): weights [Cout][kh][kw][Cin / group]; tile 0 = the generic kernel, 1-3 = channel blocks
                      // with 1 / 2 / 4 output pixels per lane.  The depthwise epilogue / prologue fields
    Transposed = 17,  // ConvTranspose (kernels_convt.hip): weights [kh][kw][Cout][Cin]; tile 0 = the generic gather kernel, 1-2 = the MFMA kernel of the
                      // non-overlapping case (k == stride, no pads, no output_padding) with 32 / 64 input pixels per wave.  Epilogue: bias, ReLU
};

// The conv algorithms whose weights are not the dense [Cout][kh][kw][Cin] layout (depthwise, grouped, transposed): no dense-conv pass or weight
// mirror may take their steps
inline bool IsGroupConv(ConvAlgo a) { return a == ConvAlgo::Depthwise || a == ConvAlgo::Grouped || a == ConvAlgo::Transposed; }

struct Step {
    StepKind kind = StepKind::Conv;
    std::string name;          // ONNX node name(s) this step came from (profiling / debugging)
    View in, in2, out;         // in2: second operand of a residual Add
    bool has_in2 = false;
    // conv / pool geometry
    int kh = 1, kw = 1, sh = 1, sw = 1, pt = 0, pl = 0, pb = 0, pr = 0;
    int dh = 1, dw = 1;        // conv dilation (> 1 only on IgemmVec / IgemmScalar / Naive steps)
    int oph = 0, opw = 0;      // ConvAlgo::Transposed: the ONNX output_padding (extra output rows / columns at the bottom / right)
    bool pool_max = false;
    bool count_include_pad = false;
    // offsets (in floats) into the weight blob; -1 = absent
    int64_t w_off = -1;        // conv weights packed [Cout][kh][kw][Cin] (ConvAlgo::Transposed: [kh][kw][Cout][Cin])
    int64_t bias_off = -1;     // [Cout]
    int64_t pre_scale_off = -1, pre_shift_off = -1;   // per input channel, applied before the op (then pre_relu)
    bool pre_relu = false;
    float pre_hi = __builtin_huge_valf();     // depthwise convs: the prologue's upper bound (a ReLU6 whose ReLU runs in the producer's epilogue)
    bool relu = false;         // applied to the result
    float lo = -__builtin_huge_valf(), hi = __builtin_huge_valf();   // then min(max(v, lo), hi): a Clip (depthwise conv epilogue / eltwise step)
    Act act;                   // then this activation (depthwise conv epilogue / eltwise step); SqueezeExcite: the gate's activation
    Act pre_act;               // prologue activation after pre_relu / pre_hi (depthwise conv: in-range taps only; global pool)
    // Eltwise: in2 is a second operand multiplied (not added); in2 of [N, C, 1, 1] broadcasts over the pixels of `in`
    bool mul = false;
    // SqueezeExcite (kernels_se.hip): out = in * act(W2 * act1(W1 * mean_hw(in) + bias) + bias2); w_off = W1 [mid][C], bias_off = its bias [mid],
    // w2_off = W2 transposed [mid][C], bias2_off = [C], all fp32 in every precision; the squeeze partials and the [N, C] gate live in the workspace
    int se_mid = 0;
    Act se_act1;
    int64_t w2_off = -1, bias2_off = -1;
    int se_chunks = 0;         // pixel chunks of the squeeze (kernels.h SeSqueezeChunks)
    // Resize: in (NHWC, [N, C, 1, 1] broadcasts) -> out (NHWC, or the dense NCHW graph output); the coordinate transform divides by the given
    // per-axis scales (output / input; the ONNX `scales`, or sizes / input when the graph gives `sizes`)
    ResizeMode rs_mode = ResizeMode::Nearest;
    ResizeCoord rs_coord = ResizeCoord::HalfPixel;
    ResizeNearest rs_nearest = ResizeNearest::RoundPreferFloor;
    double rs_scale_h = 1.0, rs_scale_w = 1.0;
    // LayerNorm (kernels_ln.hip): out = (in - mean_c) * rsqrt(var_c + ln_eps) * gamma + beta per pixel row; w_off = gamma [C], bias_off = beta [C] or
    // -1, fp32 in every precision; tile = the kernel variant (kernels.h kNumLnTiles)
    float ln_eps = 1e-5f;
    // rms: an RMSNorm, out = in * rsqrt(mean_c(in^2) + ln_eps) * gamma (Llama-class graphs); bias_off = -1; the layer norm's tiles
    bool rms = false;
    // TokenAssemble (kernels_tokens.hip): in = tokens [N, 1, L0, D], out = [N, 1, L0 + 1, D]; out[n, 0, :] = cls + pos[0], out[n, 1 + p, :] = in[n, p, :] +
    // pos[1 + p]; w_off = cls [D], bias_off = pos [L0 + 1][D] or -1, fp32 in every precision
    // Attention (kernels_attn.hip): in = the qkv tokens [N, 1, L, 3 D] (column s * D + h * head_dim + e = element e of head h of q / k / v for s = 0 / 1 / 2),
    // out[n, i, h * head_dim + e] = sum_j softmax_j(attn_scale * q_i . k_j) * v[j, e]; tile 0 = the generic kernel, 1 = the MFMA kernel
    int heads = 0, head_dim = 0;
    float attn_scale = 1.f;
    // Attention with a key mask (BERT): in2 (has_in2) = the int64 mask [N, L] graph input; key j of image n gets the bias (1 - mask[n, j]) * mask_value
    bool key_mask = false;
    float mask_value = 0.f;
    // Causal attention (GPT-2): query i attends to the keys j <= i; the graph's mask constant was checked element by element at load and is not kept
    bool causal = false;
    // Grouped-query attention (Llama): kv_heads K / V heads (0 or heads: one per query head); in = q (D) | k (Dkv) | v (Dkv) with Dkv = kv_heads * head_dim,
    // query head h reads K / V head h / (heads / kv_heads).  rope: q and k are rotated at their token position inside the kernels' own loads; w_off /
    // w2_off = the cos / sin tables [L][head_dim], fp32 in every precision
    int kv_heads = 0;
    bool rope = false;
    // KV cache (kernels_decode.hip; generation with Llama-class graphs).  Cache tensors are fp32 in every precision and dense [N][kv_heads][rows][head_dim],
    // the ABI's order of a rank-4 input / output: past_k / past_v = the `past_key_values.*` graph inputs (rows = past_len), read in place;
    // present_k / present_v = the `present.*` graph outputs (rows = past_len + in.w).  A view with buf -1 is absent.
    // KvAppend: in = the qkv tokens [N, 1, L, (H + 2 Hkv) hd]; present rows < past_len are a copy of the past, row past_len + l is k of token l after the
    // rotary embedding (rope: w_off / w2_off = the cos / sin tables [rope_rows][head_dim]) resp. v of token l, converted to fp32.  The table row of
    // token l is its own id pos[n][l] where pos (an INT64 graph input [N, L]) is present, else l.  out repeats present_k.
    // Attention with past_len > 0 (a decode step, in.w = 1): the one query of every head attends to the past_len + 1 rows of present_k / present_v; q is
    // rotated at the same table row as the new k, cached keys are taken as they are; in2 = the key mask [N, past_len + 1].  parts = {the KvAppend step,
    // this step without parts}: tile 0 runs the parts (kv_append_kernel, attention_decode_generic_kernel), tile 4 is one launch that copies, appends
    // and attends (attention_decode_kernel) over `splits` key splits per (image, K / V head), plus the combine launch where splits > 1
    // Attention with past_len > 0 and in.w = Lq >= 2 (an extend step: chunked prefill into a cache): chunk_causal; new token i attends to the rows
    // j <= past_len + i of present_k / present_v (causal inside the chunk by chunk index), q rotated at its own table row; in2 = the key mask
    // [N, past_len + Lq], pos = the INT64 positions [N, Lq], one id per token (KvAppend rotates k at the same rows).  The graph's mask constant was
    // checked element by element at load and is not kept.  Tile 0 runs the parts (kv_append_kernel, attention_extend_generic_kernel), tile 5 the
    // kv_append launch and attention_extend_kernel over `splits` key splits per (image, K / V head, block of 128 query rows), plus the combine
    View past_k, past_v, present_k, present_v, pos;
    // Set by the executor on the instances of a model bound to a resident cache, never by the planner (the plan and its JSON do not know of it): the step
    // runs in place on layer kv_layer of the cache (kernels.h DecodeArgs::cache_rows)
    bool inplace = false;
    int kv_layer = -1;
    int past_len = 0;
    bool chunk_causal = false;
    int splits = 0;
    int64_t rope_rows = 0;
    // WindowAttention (kernels_wattn.hip): in = the qkv map [N, H, W, 3 D], out = [N, H, W, D]; attention inside the win_h x win_w windows of the map
    // rolled by (-shift_h, -shift_w), every result on its query's own pixel; w_off = the relative-position bias, w2_off = the shift mask (masked
    // steps only), both packed as kernels.h WinAttnArgs describes, fp32 in every precision; heads, head_dim, attn_scale, tile as for Attention
    // PatchMerge (kernels_wattn.hip): in [N, H, W, C] -> out [N, H/2, W/2, 4 C], the four pixels of every 2 x 2 block side by side
    int win_h = 0, win_w = 0, shift_h = 0, shift_w = 0;
    bool masked = false;
    // Embed (kernels_embed.hip): in = the int64 ids [N, L] of the first table, in2 (has_in2) = the ids of the second; out = tokens [N, 1, L, D] =
    // LayerNorm(word[in] + type[in2] + pos[l]; gamma, beta, ln_eps); w_off = the first table [emb_vocab][D], w2_off = the second [emb_types][D] or -1,
    // emb_pos_off = the position rows [L][D] or -1, bias_off = gamma [D], bias2_off = beta [D] or -1, fp32 in every precision; tile as for LayerNorm
    // bias_off = -1: no LayerNormalization behind the sum (a pre-LN model): out = the sum itself
    int64_t emb_vocab = 0, emb_types = 0, emb_pos_off = -1;
    // GroupNorm (kernels_gn.hip): out = act((in - mean_ng) * rsqrt(var_ng + ln_eps) * gamma + beta), the statistics over the in.c / gn_groups channels of
    // group g and every pixel of image n; w_off = gamma [C], bias_off = beta [C], fp32 in every precision; act = the fused SiLU / ReLU / Sigmoid; tile 0 =
    // the generic kernel, 1 = the statistics + apply launches, whose records live in the workspace (kernels.h GnWorkspaceFloats)
    int gn_groups = 0;
    ConvAlgo algo = ConvAlgo::Naive;
    int group = 1;             // ConvAlgo::Grouped: the ONNX group count
    int tile = 0;              // igemm tile configuration index (see igemm_tiles.h)
    int base_tile = 0;         // the tiled implicit GEMM's heuristic tile (what the executor falls back to when a specialised launcher declines)
    int splitk = 1;            // >1: K-tiles split over this many workgroups per output tile (+ reduce kernel)
    int idx = -1;              // position in Plan::steps
    int in_src = -1, in2_src = -1;   // index of the step that produced `in` / `in2` (-1: a graph input); fp8 mode looks the tensors' scales up by it
    // DenseFused: parts = {the 3x3 conv step, the 1x1 conv step} exactly as the planner emitted them; this step's own fields repeat
    // the 1x1's (in, out, weights, prologue, epilogue); tile = 16-pixel blocks per workgroup (1 or 2).  The executor launches the
    // parts one after the other when the fused launcher declines.
    std::vector<Step> parts;
    double flops = 0;          // algorithmic FLOPs (2*MACs) of this step for the planned shape
    double bytes = 0;          // algorithmic bytes: operands read once + result written once
};

struct IoDesc {
    std::string name;
    int elem_type = ONNX_FLOAT;
    std::vector<int64_t> model_dims;   // as declared in the ONNX file (-1 = symbolic)
    std::vector<int64_t> dims;         // resolved for this plan
    View view;                         // device staging view (dense NCHW order as the ABI expects)
};

// bytes per element of a Plan::buffer_f16 code
inline int BufferElemBytes(int code) { return code == 3 ? 8 : (code == 2 ? 1 : (code == 1 ? 2 : 4)); }

struct Plan {
    std::vector<IoDesc> inputs, outputs;
    Precision precision = Precision::F32;
    std::vector<int64_t> buffer_floats;   // size of each device activation buffer in ELEMENTS
    std::vector<char> buffer_f16;         // element type of each buffer: 0 = float, 1 = half, 2 = e4m3 byte, 3 = int64
    std::vector<Step> steps;
    std::vector<float> weights;           // packed blob (batch independent)
    int64_t workspace_floats = 0;         // split-K partial-sum slabs (max over steps of splitk*M*Cout)
    double total_flops = 0, total_bytes = 0;
    int64_t activation_floats() const { int64_t s = 0; for (auto b : buffer_floats) s += b; return s; }
    int64_t activation_bytes() const {
        int64_t s = 0;
        for (size_t i = 0; i < buffer_floats.size(); ++i) s += buffer_floats[i] * BufferElemBytes(buffer_f16[i]);
        return s;
    }
};

// Static (shape independent) facts, available right after parsing: what ExtractModelMetadata
// (model.cpp:910-972) and EstimateModelMemoryUsage (model.cpp:979-1035) report.
struct ModelInfo {
    std::vector<OnnxValueInfo> inputs, outputs;
    size_t memory_usage_bytes = 0;
};
ModelInfo DescribeModel(const OnnxModel& m);

// Build the plan for concrete input shapes (one entry per graph input, in graph order).
// Throws std::runtime_error with an ORT-like message on unsupported ops or shape mismatches.
// f8_fusions: apply the step fusions of the fp8 mode (DualF8) whatever the precision -- the fp8 calibration runs the graph in fp16 and needs
// the SAME step list as the fp8 plan it calibrates.
Plan BuildPlan(const OnnxModel& m, const std::vector<std::vector<int64_t>>& input_shapes, Precision precision = Precision::F32, bool f8_fusions = false);

std::string PlanToJson(const Plan& p);

}  // namespace ie
