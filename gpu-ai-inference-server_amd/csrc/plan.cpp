#include "plan.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <functional>
#include <list>
#include <map>
#include <set>
#include <sstream>
#include <stdexcept>

#include "env.h"
#include "igemm_tiles.h"
#include "kernels.h"

namespace ie {

// Dense-layer fusion applies where launches are latency-bound: up to this many output pixels (IE_FUSE_MAX_M overrides; A/B switch).
static int64_t FuseMaxPixels(const Env& env) {
    const char* e = env.get("IE_FUSE_MAX_M");
    const long long x = e ? std::atoll(e) : 0;
    const int64_t v = x > 0 ? int64_t(x) : int64_t(8192);
    return v;
}
namespace {

[[noreturn]] void fail(const std::string& msg) { throw std::runtime_error(msg); }

struct Val {
    std::string name;
    std::vector<int64_t> dims;          // resolved ONNX dims
    int64_t n = 0, c = 0, h = 1, w = 1;
    int producer = -1;                  // LNode index, -1 = graph input
    bool is_input = false, is_output = false, input_nchw = false;
    bool is_i64 = false;                // an INT64 graph input [N, L] (ids): its buffer holds int64, only an embed node reads it
    int parent = -1;                    // concat parent value
    int64_t parent_off = 0;
    int root = -1;
    int64_t abs_off = 0;
    int buf = -1;
    bool dedicated = false;             // its buffer is never recycled
    // token select (Gather(axis 1, index i) of a token value [N, L, D]): this [N, D] value is row sel_idx of every image of its parent, a view of
    // pitch sel_rows * the parent's pitch
    int64_t sel_rows = 1, sel_idx = 0;
};

enum LKind { L_CONV, L_AFFINE, L_RELU, L_ADD, L_CONCAT, L_MAXPOOL, L_AVGPOOL, L_GAP, L_ALIAS, L_COPY, L_CLIP, L_ACT, L_MUL, L_SE, L_RESIZE, L_LAYERNORM, L_ERF, L_TOKASM, L_TOKPOS, L_ATTENTION, L_WATTN, L_PATCHMERGE, L_EMBED, L_GROUPNORM, L_KVAPPEND };

constexpr float kInf = __builtin_huge_valf();

struct LNode {
    LKind kind;
    std::string name;
    std::vector<int> in;
    int out = -1;
    int kh = 1, kw = 1, sh = 1, sw = 1, pt = 0, pl = 0, pb = 0, pr = 0;
    int dil_h = 1, dil_w = 1;           // conv dilation (1 on an axis whose kernel extent is 1)
    bool count_include_pad = false;
    // L_RESIZE: mode, coordinate transform, nearest rounding, the scales (output / input) the coordinate transform divides by
    ResizeMode rs_mode = ResizeMode::Nearest;
    ResizeCoord rs_coord = ResizeCoord::HalfPixel;
    ResizeNearest rs_nearest = ResizeNearest::RoundPreferFloor;
    double rs_sh = 1.0, rs_sw = 1.0;
    std::vector<float> w, bias;         // conv: w packed [Cout][kh][kw][Cin]
    std::vector<float> s, t;            // affine; L_LAYERNORM: gamma, beta (beta may be empty)
    float eps = 1e-5f;                  // L_LAYERNORM
    bool rms = false;                   // L_LAYERNORM: an RMSNorm (no mean, no beta)
    // L_TOKASM: s = the class token [D], t = the position embedding [L][D] (empty: none); L_TOKPOS: t = the [L][D] constant an Add puts on tokens
    // L_ATTENTION: in = the qkv tokens [N, L, 3 heads head_dim]
    int heads = 0, head_dim = 0;
    double attn_scale = 1.0;
    // L_WATTN: in = the qkv map [N, 3 heads head_dim, H, W] read channels-last; w = the relative-position bias [heads][L][L], w2 = the shift mask
    // [nW][L][L] (masked only), both as the graph's constants hold them (query row, key column); EmitWindowAttention packs them for the kernels
    int win_h = 0, win_w = 0, shift_h = 0, shift_w = 0;
    bool masked = false;
    bool key_mask = false;              // L_ATTENTION: in[1] = the int64 key mask [N, L]; the bias of a masked key is mask_value
    float mask_value = 0.f;
    bool causal = false;                // L_ATTENTION: query i attends to the keys j <= i
    int kv_heads = 0;                   // L_ATTENTION: K / V heads (0: heads); in = q (D) | k (Dkv) | v (Dkv).  Rotary: w / w2 = the cos / sin tables [L][head_dim]
    // L_KVAPPEND: in[0] = the qkv tokens, out = present k (kv_v: present v) [N, Hkv, past_len + L, hd]; in[past_in] = the past input (-1: none), in[pos_in] =
    // the INT64 position input (-1: none); w / w2 = the rope tables [rope_rows][hd] (k only).  L_ATTENTION with past_len > 0 (a decode step): in[present_in]
    // and in[present_in + 1] = present k / v, in[pos_in] = the positions
    int past_len = 0, past_in = -1, pos_in = -1, present_in = -1;
    bool chunk_causal = false;          // L_ATTENTION with past_len > 0 and L >= 2 new tokens (an extend step): token i sees the keys j <= past_len + i
    bool kv_v = false;
    int64_t rope_rows = 0;
    // L_EMBED: in = the int64 ids of the first table (and of the second); w = the first table [emb_vocab][D], w2 = the second [emb_types][D] (empty:
    // none), bias = the position rows [L][D] (empty: none), s / t / eps = gamma / beta / epsilon of the LayerNormalization behind the sum
    int64_t emb_vocab = 0, emb_types = 0;
    // L_GROUPNORM: s / t = gamma / beta per channel (the inner InstanceNormalization's scale and bias folded in), eps, act = the fused activation
    int gn_groups = 0;
    bool has_pre = false, pre_relu = false, relu = false;
    std::vector<float> pre_s, pre_t;
    int res = -1;                       // conv: value added to the result before the ReLU (fused residual Add)
    bool dw = false;                    // depthwise conv (group == Cin == Cout): w packed [C][kh][kw]
    int64_t group = 1;                  // conv: the ONNX group count (> 1 and not dw: a grouped conv, w packed [Cout][kh][kw][Cin / group])
    bool transposed = false;            // ConvTranspose: w packed [kh][kw][Cout][Cin]; no dense-conv pass may take it
    int op_h = 0, op_w = 0;             // ConvTranspose: output_padding
    float lo = -kInf, hi = kInf;        // Clip bounds (L_CLIP; a depthwise conv's epilogue clamp)
    float pre_hi = kInf;                // depthwise conv: upper bound of the prologue
    Act act;                            // L_ACT; a depthwise conv's epilogue activation; L_SE: the gate's
    Act pre_act;                        // depthwise conv / global pool: prologue activation
    // L_SE: w = FC1 [mid][C], bias = its bias, w2 = FC2 transposed [mid][C], bias2 = [C]
    std::vector<float> w2, bias2;
    int se_mid = 0;
    Act se_act1;
    bool dead = false;
};

struct Lowering {
    const OnnxModel& m;
    std::vector<Val> vals;
    std::map<std::string, int> val_of;
    std::vector<LNode> nodes;
    // initializers produced at plan time by folding shape-only ops (Unsqueeze / Squeeze / Reshape / Flatten / Identity) whose
    // input is itself a constant: model-zoo exports of Caffe BN+Scale pairs route the [C] scale and bias through Unsqueeze nodes
    std::map<std::string, OnnxTensor> derived;
    // derived initializers computed from a Shape node (and the int64 arithmetic behind it): only a Resize's `sizes` may read them
    std::set<std::string> shape_derived;
    // Names that read their value channels-last: the result of Transpose(perm [0,2,3,1]) and of every op computed on such a view.  The value
    // behind the name keeps its NCHW dims, its n / c / h / w and its NHWC storage: the ONNX dims [N, H, W, C] exist only in the graph file, so
    // no pass ever sees them.  A Transpose emits no node: its output is one more name of its input's value.
    std::set<std::string> cl_names;
    bool is_cl(const std::string& name) const { return cl_names.count(name) != 0; }
    // Names that read their value as tokens [N, L, D]: the value behind the name has the dims [N, D, 1, L] (n = N, c = D, h = 1, w = L), so its NHWC
    // storage is the [N, L, D] array.  flat_names: the [N, C, H*W] Reshape of a feature map, which only the Transpose [0,2,1] to tokens may read;
    // back_names: the Transpose [0,2,1] of a token name, which only the Reshape to [N, D, h, w] may read.  Both are names of the unchanged value.
    std::set<std::string> tok_names, flat_names, back_names;
    bool is_tok(const std::string& name) const { return tok_names.count(name) != 0; }

    explicit Lowering(const OnnxModel& mm) : m(mm) {}

    int new_val(const std::string& name, const std::vector<int64_t>& dims) {
        if (val_of.count(name)) fail("ONNX graph error: value defined twice: " + name);
        Val v;
        v.name = name;
        v.dims = dims;
        if (dims.size() == 4) { v.n = dims[0]; v.c = dims[1]; v.h = dims[2]; v.w = dims[3]; }
        else if (dims.size() == 2) { v.n = dims[0]; v.c = dims[1]; }
        else if (dims.size() == 3) { v.n = dims[0]; v.c = dims[1]; v.h = dims[2]; }
        else if (dims.size() == 1) { v.n = 1; v.c = dims[0]; }
        else fail("unsupported tensor rank " + std::to_string(dims.size()) + " for value " + name);
        for (auto d : dims) if (d <= 0) fail("non-positive dimension in value " + name);
        vals.push_back(v);
        val_of[name] = int(vals.size()) - 1;
        return int(vals.size()) - 1;
    }
    // one more name for value v (a Transpose's output), read channels-last or NCHW
    void alias_name(const std::string& name, int v, bool channels_last) {
        if (val_of.count(name) || derived.count(name) || m.initializers.count(name)) fail("ONNX graph error: value defined twice: " + name);
        val_of[name] = v;
        if (channels_last) cl_names.insert(name);
    }
    int get_val(const std::string& name) const {
        auto it = val_of.find(name);
        if (it == val_of.end()) fail("ONNX graph error: undefined value: " + name);
        return it->second;
    }
    const OnnxTensor* init(const std::string& name) const {
        auto it = m.initializers.find(name);
        if (it != m.initializers.end()) return &it->second;
        auto jt = derived.find(name);
        return jt == derived.end() ? nullptr : &jt->second;
    }
    // a derived initializer under `t.name`; the name must be new to the graph
    void add_derived(OnnxTensor t) {
        if (derived.count(t.name) || m.initializers.count(t.name) || val_of.count(t.name)) fail("ONNX graph error: value defined twice: " + t.name);
        const std::string name = t.name;
        derived[name] = std::move(t);
    }
    std::vector<int> consumers(int v) const {
        std::vector<int> out;
        for (size_t i = 0; i < nodes.size(); ++i)
            if (!nodes[i].dead)
                for (int x : nodes[i].in) if (x == v) { out.push_back(int(i)); break; }
        return out;
    }

    // A constant that broadcasts along the channel axis of `x` (numpy rules): scalar, [C], [1,C], [C,1,1], [1,C,1,1].
    // legacy_axis >= 0: opset < 7 broadcasting (attributes broadcast=1, axis=k): the constant's dims align with the activation's
    // dims starting at axis k instead of at the trailing end.
    bool per_channel_const(const OnnxTensor& t, const Val& x, std::vector<float>& out, int64_t legacy_axis = -1) const {
        if (t.dtype != ONNX_FLOAT && t.dtype != ONNX_DOUBLE && t.dtype != ONNX_FLOAT16) return false;
        int64_t n = t.numel();
        if (n == 1) { out.assign(size_t(x.c), t.f[0]); return true; }
        if (n != x.c) return false;
        size_t rank = x.dims.size();
        std::vector<int64_t> d = t.dims;
        if (legacy_axis >= 0) {
            if (size_t(legacy_axis) + d.size() > rank) return false;
            d.insert(d.begin(), size_t(legacy_axis), 1);
            while (d.size() < rank) d.push_back(1);
        }
        while (d.size() < rank) d.insert(d.begin(), 1);
        if (d.size() != rank) return false;
        for (size_t k = 0; k < rank; ++k) if (d[k] != (k == 1 ? x.c : 1)) {
            // rank-1 value [C] against rank-2 x [N,C] puts C on the last axis, which IS the channel axis
            return false;
        }
        out = t.f;
        return true;
    }
};

void conv_out_hw(int64_t h, int64_t w, const LNode& n, bool ceil_mode, int64_t& oh, int64_t& ow) {
    auto f = [&](int64_t x, int k, int s, int p0, int p1) {
        int64_t num = x + p0 + p1 - k;
        if (num < 0) fail("kernel larger than padded input in node " + n.name);
        return (ceil_mode ? (num + s - 1) / s : num / s) + 1;
    };
    oh = f(h, (n.kh - 1) * n.dil_h + 1, n.sh, n.pt, n.pb);     // a dilated window spans (k - 1) * d + 1 pixels
    ow = f(w, (n.kw - 1) * n.dil_w + 1, n.sw, n.pl, n.pr);
}

void read_window_attrs(const OnnxNode& on, LNode& n, int64_t h, int64_t w, bool is_conv, const OnnxTensor* wt) {
    std::vector<int64_t> ks = on.attr_ints("kernel_shape", {});
    if (ks.empty() && is_conv && wt) ks = {wt->dims[2], wt->dims[3]};
    if (ks.size() != 2) fail("node " + on.name + ": only 2-D kernels are supported");
    n.kh = int(ks[0]); n.kw = int(ks[1]);
    auto st = on.attr_ints("strides", {1, 1});
    n.sh = int(st[0]); n.sw = int(st[1]);
    auto dl = on.attr_ints("dilations", {1, 1});
    if (dl.size() != 2 || dl[0] < 1 || dl[1] < 1) fail("node " + on.name + ": dilations must be two positive integers");
    if (!is_conv && (dl[0] != 1 || dl[1] != 1)) fail(on.op + " " + on.name + ": dilations != 1 are only supported on Conv");
    // a kernel extent of 1 reads one pixel whatever the dilation: such an axis is planned undilated
    n.dil_h = n.kh == 1 ? 1 : int(dl[0]);
    n.dil_w = n.kw == 1 ? 1 : int(dl[1]);
    auto pads = on.attr_ints("pads", {0, 0, 0, 0});
    if (pads.size() != 4) fail("node " + on.name + ": pads must have 4 entries");
    n.pt = int(pads[0]); n.pl = int(pads[1]); n.pb = int(pads[2]); n.pr = int(pads[3]);
    auto ap = on.attrs.find("auto_pad");
    if (ap != on.attrs.end() && !ap->second.s.empty() && ap->second.s != "NOTSET") {
        const std::string& mode = ap->second.s;
        if (mode == "VALID") n.pt = n.pl = n.pb = n.pr = 0;
        else if (mode == "SAME_UPPER" || mode == "SAME_LOWER") {
            auto same = [&](int64_t x, int k, int s, int& p0, int& p1) {
                int64_t o = (x + s - 1) / s;
                int64_t tot = std::max<int64_t>((o - 1) * s + k - x, 0);
                int64_t a = tot / 2, b = tot - a;
                if (mode == "SAME_UPPER") { p0 = int(a); p1 = int(b); } else { p0 = int(b); p1 = int(a); }
            };
            same(h, (n.kh - 1) * n.dil_h + 1, n.sh, n.pt, n.pb);
            same(w, (n.kw - 1) * n.dil_w + 1, n.sw, n.pl, n.pr);
        } else fail("node " + on.name + ": unsupported auto_pad " + mode);
    }
}

// A view the 16-byte channel-vector kernels can address (V = 4 floats / 8 halfs): NHWC, channel count, pitch and channel offset whole vectors, the
// step's element type.  The launchers' *Eligible functions re-check it with the pointers (launch_util.h VecViewOk)
static bool VecView(const View& v, int64_t V, bool f16) { return !v.nchw && v.c % V == 0 && v.pitch % V == 0 && v.c_off % V == 0 && v.f16 == f16; }

// Depthwise steps: the views the 16-byte channel-vector kernels need
bool DwFastViews(const Step& s) {
    const int64_t V = s.out.f16 ? 8 : 4;
    // (the fast kernel's branch-free activation knows the sigmoid family only: a fused GELU runs on the generic kernel)
    const bool gelu = int(s.act.kind) >= int(ActKind::Gelu) || int(s.pre_act.kind) >= int(ActKind::Gelu);
    return s.kh == s.kw && (s.kh == 3 || s.kh == 5) && s.sh == s.sw && (s.sh == 1 || s.sh == 2) && !gelu && VecView(s.in, V, s.out.f16) &&
           VecView(s.out, V, s.out.f16) && (!s.has_in2 || VecView(s.in2, V, s.out.f16));
}
// 4 output pixels per lane on wide rows, 2 on narrow ones (7x7 maps: 4 groups of 2 instead of 2 of 4, one wasted lane in eight), the generic kernel otherwise
int DwDefaultTile(const Step& s) { return DwFastViews(s) ? (s.out.w >= 14 ? 3 : 2) : 0; }

// Grouped steps: the views and channel blocks the fast kernel needs for `tile`
bool GroupedFastViews(const Step& s, int tile) {
    const int cfg = GroupedCfgFor(s.in.c, s.out.c, s.group);
    if (cfg < 0 || !GroupedTileFits(cfg, s.out.f16, tile) || s.out.c % (kGroupedCfgs[cfg].opb * kGroupedCfgs[cfg].gpb) || s.kh > 7 || s.kw > 7) return false;
    if (int(s.act.kind) >= int(ActKind::Gelu) || int(s.pre_act.kind) >= int(ActKind::Gelu)) return false;      // (the fast kernel compiles the activations 0-5 only)
    const int64_t V = s.out.f16 ? 8 : 4;
    return VecView(s.in, V, s.out.f16) && VecView(s.out, V, s.out.f16) && (!s.has_in2 || VecView(s.in2, V, s.out.f16));
}
// What the autotuner picked on 63 of the 64 grouped steps of ResNeXt-50 / RegNetY-400MF (fp32 b32, fp16 b128): 2 output pixels per
// lane for fp16 groups of 16 or more input channels, else 1; the generic kernel when no channel block fits
int GroupedDefaultTile(const Step& s) {
    if (s.out.f16 && s.in.c / s.group >= 16 && GroupedFastViews(s, 2)) return 2;
    return GroupedFastViews(s, 1) ? 1 : 0;
}

// Transposed steps: what the MFMA kernel of the non-overlapping case needs (kernels_convt.hip ConvTransposedEligible re-checks it with the
// pointers): k == stride with no pads and no output_padding, so every output pixel receives exactly one tap; at most 16 taps; NHWC operands of
// the plan's element type with Cin a multiple of the K-step (8 floats / 16 halfs) and 16-byte aligned input pixel rows
bool ConvtFastViews(const Step& s) {
    const int64_t KS = s.out.f16 ? 16 : 8, V = s.out.f16 ? 8 : 4;
    return s.kh == s.sh && s.kw == s.sw && !s.pt && !s.pl && !s.pb && !s.pr && !s.oph && !s.opw && s.kh * s.kw <= 16 && VecView(s.in, V, s.out.f16) &&
           s.in.c % KS == 0 && !s.out.nchw && !s.in.f8 && !s.out.f8;      // (the output only has to be NHWC: Cout tails are masked)
}
// 64 input pixels per wave reuse every weight fragment twice; 32 where that would leave the 256 CUs short of waves (one wave per
// 32-channel block, pixel block and group of four taps)
int ConvtDefaultTile(const Step& s) {
    if (!ConvtFastViews(s)) return 0;
    const int64_t M = s.in.n * s.in.h * s.in.w, waves64 = ((M + 63) / 64) * ((s.out.c + 31) / 32) * ((s.kh * s.kw + 3) / 4);
    return waves64 >= 2048 ? 2 : 1;
}

// Layer-norm steps: the views the register-resident kernel needs for `tile`; beyond VecView, no e4m3 operand
bool LnFastViews(const Step& s, int tile) {
    const int64_t V = s.out.f16 ? 8 : 4;
    return LnTileFits(s.in.c, s.out.f16, tile) && !s.in.f8 && !s.out.f8 && VecView(s.in, V, s.out.f16) && VecView(s.out, V, s.out.f16);
}

// Algorithmic FLOPs per element of a fused activation
double ActFlops(ActKind k) {
    switch (k) {
        case ActKind::Sigmoid: return 3;       // exp, add, divide
        case ActKind::HardSigmoid: return 3;   // fma, two clamps
        case ActKind::Silu: return 4;
        case ActKind::HardSwish: return 4;
        case ActKind::Relu: return 1;
        case ActKind::Gelu: return 6;          // scale, erf, add, three multiplies
        case ActKind::GeluTanh: return 10;     // cube, fma, scale, tanh, add, three multiplies
        case ActKind::Tanh: return 2;
        default: return 0;
    }
}

int choose_tile(int64_t M, int64_t N) {
    // Estimated time = rounds over the 256 CUs x tile area / tile efficiency.  Larger tiles reuse operands
    // better (higher MFMA duty); smaller ones fill the chip when M*N is small.  A lone workgroup per CU
    // cannot hide its own staging latency, so under-filled grids are charged a lower duty.
    static const double eff[kNumIgemmBaseTiles] = {1.00, 0.92, 0.78, 0.82, 0.62, 0.40, 0.84};
    int best = -1;
    double best_cost = 0;
    for (int t = 0; t < kNumIgemmBaseTiles; ++t) {
        const IgemmTile& T = kIgemmTiles[t];
        if (T.bn > 32 && N <= 32) continue;             // do not waste MFMA columns on zero padding
        if (T.bn > 64 && N <= 64) continue;
        double wgs = double((M + T.bm - 1) / T.bm) * double((N + T.bn - 1) / T.bn);
        double per_cu = wgs / 256.0;
        double rounds = std::max(1.0, 0.5 * (per_cu + std::ceil(per_cu)));
        double duty = wgs >= 512 ? 0.9 : (wgs >= 256 ? 0.75 : 0.6);
        double cost = rounds * double(T.bm) * T.bn / (eff[t] * duty);
        if (best < 0 || cost < best_cost) { best = t; best_cost = cost; }
    }
    return best;
}

double vbytes(const View& v) { return double(v.numel()) * double(v.esize()); }

const int ws_tn[14] = {4, 4, 2, 2, 1, 1, 4, 4, 2, 2, 1, 1, 1, 1};      // 12, 13: fp32 K-split variants (8 / 4 waves)

// Schedule position of a value that is never recycled (graph inputs and outputs)
constexpr int kLiveForever = 1 << 30;

// What the kernel choice of one dense conv step reads: the GEMM extents, the operand types, and the plan-time eligibility of the specialised
// kernels (the launchers re-check pointers / alignment; the executor falls back to the tiled implicit GEMM when a launcher declines)
struct ConvFacts {
    const LNode& n;
    const Step& s;                    // its views and has_in2 are final; algo / tile / splitk are what the choice fills in
    int64_t M, N, K;
    bool in16, in8, dil, vec_ok, vec16_ok, is1x1, is3x3;
    ConvFacts(const LNode& n, const Step& s);
    ConvAlgo tiled_algo() const { return (vec_ok || vec16_ok) ? ConvAlgo::IgemmVec : (K <= 2048 && !in16 ? ConvAlgo::IgemmScalar : ConvAlgo::Naive); }
    bool ws16_ok(int t) const;
    bool ws32_ok(int t) const;
    bool ws3_ok(int t3) const;
    bool direct_ok(int t) const;
    bool raster_ok() const { return vec_ok && !s.out.f16 && is3x3 && !n.has_pre; }
    bool wino_ok() const { return raster_ok() && N == 32 && s.in.c % 32 == 0 && s.in.h % 2 == 0 && s.in.w % 2 == 0 && n.res < 0 && s.out.pitch % 4 == 0 && s.out.c_off % 4 == 0; }
};

// What the passes of one BuildPlan share.  The passes run once each, in the order BuildPlan lists them; a pass may read anything an
// earlier pass left here.
struct Planner {
    const OnnxModel& m;
    const std::vector<std::vector<int64_t>>& input_shapes;
    const Env& env;                        // the planner's switches, read once per plan build
    const Precision precision;
    const bool f8_fusions;
    const bool keep_buffers;               // IE_KEEP_BUFFERS=1 (tests): no buffer is recycled, every value stays readable after the forward
    Lowering L;
    Plan plan;
    std::vector<int> out_vals;             // DensifyOutputs: the value each graph output is read from, in graph order
    std::vector<int> order;                // ComputeLiveness: the live nodes in schedule order
    std::vector<int> first_def, last_use;  // ComputeLiveness: schedule positions per root value
    std::vector<char> used;                // ComputeLiveness: root values some live node touches
    std::map<std::vector<int64_t>, int> writer;   // EmitSteps: (buffer, channel offset, channels) -> step index, for Step::in_src / in2_src

    Planner(const OnnxModel& mm, const std::vector<std::vector<int64_t>>& shapes, const Env& e, Precision p, bool f8)
        : m(mm), input_shapes(shapes), env(e), precision(p), f8_fusions(f8), keep_buffers(e.flag("IE_KEEP_BUFFERS")), L(mm) { plan.precision = p; }

    // ---- helpers ----
    bool single_consumer(int v) const { return !L.vals[v].is_output && L.consumers(v).size() == 1; }
    int ForcedTile(int limit) const;       // IE_FORCE_TILE when it is set and in [0, limit), else -1
    int64_t root_floats(int r) const { const Val& R = L.vals[r]; return R.n * R.c * R.h * R.w; }
    View view_of(int v) const;
    int64_t push_vec(const std::vector<float>& v);       // append to the weight blob (32-byte aligned), return the offset
    int src_of(const View& v) const;
    bool output_in_buffer(int buf) const;  // a graph output lives in this buffer

    // ---- ONNX graph -> logical nodes ----
    void ImportInputs();
    void ImportNode(const OnnxNode& on);
    void MarkOutputs();
    void RefuseForF8() const;
    int in_val(const OnnxNode& on, size_t k) const { return L.get_val(on.inputs[k]); }
    bool act_input(const OnnxNode& on, size_t k) const { return k < on.inputs.size() && !on.inputs[k].empty() && !L.init(on.inputs[k]); }
    bool FoldConstantNode(const OnnxNode& on);
    bool FoldShapeArithmetic(const OnnxNode& on, const LNode& n);
    bool FoldShapeOnlyOp(const OnnxNode& on, const LNode& n);
    bool ImportTranspose(const OnnxNode& on, const LNode& n);
    bool cl_out = false;                   // ImportNode: the importer computed its result on a channels-last view (the output's name is one too)
    bool tok_out = false;                  // ImportNode: the importer computed its result on a token view (the output's name is one too)
    // MatchAttention: the attention subgraphs found in the ONNX graph.  attn_head: the rank-5 Reshape of a match -> what ImportAttention needs;
    // attn_skip: the other nodes of the matches (they import nothing)
    struct AttnMatch {
        int64_t heads = 0, head_dim = 0;
        double scale = 1.0;
        std::string out, name;
        std::vector<int64_t> shape5, shape3;
        // the separate q / k / v spelling (BERT): the token value the three Linears read and their merged weights [Din, 3 D] / bias [3 D] (derived initializers)
        bool split = false;
        std::string x, w_name, b_name;
        // the key mask: the INT64 graph input behind the ext chain and its constant c
        std::string mask;
        float mask_value = 0.f;
        // GPT-2's spelling: q, k and v are the three parts of Split(axis 2) of ONE Linear's result, which is the qkv layout itself (the Split is the head)
        bool fused = false;
        // the causal mask (a Where or an additive constant on the scores), checked element by element; causal_len = its L
        bool causal = false;
        int64_t causal_len = 0;
        // Llama's spelling of the split form: Linears without a bias, kv_heads K / V heads (k and v Linears [Din, kv_heads hd]) behind repeat_kv, and the
        // rotary embedding on q and k: the cos / sin tables as the graph's constants broadcast them, [rope_rows][head_dim], and the node to name in a refusal
        bool no_bias = false;
        int64_t kv_heads = 0;
        bool rope = false;
        std::vector<float> rope_cos, rope_sin;
        int64_t rope_rows = 0;
        std::string rope_name;
        std::vector<std::vector<int64_t>> rep_expand, rep_reshape;      // repeat_kv: the Expand and Reshape shapes (k, v), checked against N and L at the import
        // the cache: past_k / past_v = the FLOAT rank-4 graph inputs a Concat(axis 2) puts in front of the step's own k / v (a decode step); present_k /
        // present_v = the graph outputs that name the Concat results (without a past: the rotated k and the transposed v of a prefill); rope_pos = the
        // INT64 graph input [N, 1] that gathers the rope tables (empty: constant positions); cat_k / cat_v = the Concat nodes (messages)
        std::string past_k, past_v, present_k, present_v, rope_pos, cat_k, cat_v;
        // an extend step: the mask is M = Where(Cast(ext, BOOL), c, C) (MatchChunkMask); chunk_c = the constant C, checked against the step's P and Lq
        // at the import; chunk_where = the Where (messages).  rope_pos_miss: the refusal of position ids that are not [N, 1], kept for a decode step
        bool chunk = false;
        const OnnxTensor* chunk_c = nullptr;
        std::string chunk_where, rope_pos_miss;
    };
    // M = Where(Cast(ext, to BOOL), c <= -1e30, C) with ext a key-mask chain and C a float constant [1, 1, Lq, P + Lq]: the 4-D mask of an extend step,
    // matched once per name and shared by all layers.  Its Where and Cast import nothing, and only attention Adds may read M
    struct ChunkMask { bool ok = false; std::string ext; const OnnxTensor* c = nullptr; float fill = 0.f; std::vector<const OnnxNode*> nodes; int uses = 0; };
    std::map<std::string, ChunkMask> chunk_masks;
    const ChunkMask* MatchChunkMask(const std::string& name, const std::string& prefix);
    std::map<std::vector<float>, int64_t> rope_blob;      // EmitKvAppend: the rope tables already in the weight blob (every layer of a model gathers the same ones)
    std::set<const OnnxNode*> rope_const_nodes;      // the Unsqueeze / Slice / Gather nodes that cut the rope tables out of constants: evaluated at load, import nothing
    // MatchCausalWhere / MatchCausalAdd: the two spellings of a causal mask on the scores (false / a refusal by name: not one)
    void MatchCausalWhere(const OnnxNode& wh, const std::string& prefix, AttnMatch& am, std::vector<const OnnxNode*>& taken);
    bool MatchCausalAdd(const OnnxTensor& mk, AttnMatch& am) const;
    // MatchConv1D: HF's Conv1D on tokens, Reshape [-1, D] -> Gemm -> Reshape [N, L, Dout].  conv1d_view: the two Reshapes (false: the first, true: the
    // second), which rename their input's token value; conv1d_gemm: the Gemms, which then read a token view like a MatMul does
    std::map<const OnnxNode*, bool> conv1d_view;
    std::set<const OnnxNode*> conv1d_gemm;
    void MatchConv1D();
    bool ImportConv1DView(const OnnxNode& on, bool second);
    // MatchGeluTanh: gelu_new spelled out, 0.5 x (1 + Tanh(c (x + 0.044715 x^3))).  gelu_head: its last Mul -> x; gelu_skip: its other nodes
    std::map<const OnnxNode*, std::string> gelu_head;
    std::set<const OnnxNode*> gelu_skip;
    void MatchGeluTanh();
    bool FoldConstTranspose(const OnnxNode& on);
    std::set<int> tok_outputs;                 // MarkOutputs: the graph outputs that are token values [N, L, D] (row-major in their NHWC buffer)
    // the ext chain of a key mask, matched once per name and shared by all layers: Unsqueeze(s) -> Cast FLOAT -> Sub(1, .) -> Mul(., c)
    struct KeyMask { bool ok = false; std::string input; float c = 0.f; std::vector<const OnnxNode*> nodes; int uses = 0; };
    std::map<std::string, KeyMask> key_masks;
    const KeyMask& MatchKeyMask(const std::string& name);
    std::set<const OnnxNode*> mask_nodes;          // the nodes of the matched ext chains (they import nothing; they may read an INT64 graph input)
    std::list<OnnxNode> synth_nodes;               // nodes the planner writes itself (the merged qkv Linear of a split attention)
    struct SplitCore;
    bool MatchSplitAttention(const OnnxNode& sm, const OnnxNode* pv, const std::string& scores, const std::string& prefix, AttnMatch& am, const OnnxNode*& head,
                             std::vector<const OnnxNode*>& taken);
    std::map<const OnnxNode*, AttnMatch> attn_head;
    std::set<const OnnxNode*> attn_skip;
    void MatchAttention();
    void ImportAttention(const OnnxNode& on, const AttnMatch& am);
    // What the matchers on the ONNX nodes share: producer and reader count of every name, the constants (initializers and Constant nodes)
    struct GraphIndex {
        const OnnxModel* m = nullptr;
        std::map<std::string, const OnnxNode*> prod;
        std::map<std::string, int> readers;
        std::map<std::string, OnnxTensor> consts;
        const OnnxTensor* cst(const std::string& name) const {
            const auto it = m->initializers.find(name);
            if (it != m->initializers.end()) return &it->second;
            const auto jt = consts.find(name);
            return jt == consts.end() ? nullptr : &jt->second;
        }
        const OnnxNode* producer(const std::string& name) const { const auto it = prod.find(name); return it == prod.end() ? nullptr : it->second; }
        int nreaders(const std::string& name) const { const auto it = readers.find(name); return it == readers.end() ? 0 : it->second; }
        std::vector<const OnnxNode*> readers_of(const std::string& name) const {
            std::vector<const OnnxNode*> out;
            for (const OnnxNode& on : m->nodes) for (const std::string& i : on.inputs) if (i == name) { out.push_back(&on); break; }
            return out;
        }
        const OnnxNode* only_reader(const std::string& name) const {
            if (nreaders(name) != 1) return nullptr;
            const auto r = readers_of(name);
            return r.size() == 1 ? r[0] : nullptr;
        }
        bool act_matmul(const OnnxNode* p) const { return p && p->op == "MatMul" && p->inputs.size() == 2 && !cst(p->inputs[0]) && !cst(p->inputs[1]); }
        // the name above a chain of Mul / Div by constants (nothing checked, nothing taken)
        std::string peel_quiet(std::string cur) const {
            for (;;) {
                const OnnxNode* p = producer(cur);
                if (!p || (p->op != "Mul" && p->op != "Div") || p->inputs.size() != 2) return cur;
                const OnnxTensor *c0 = cst(p->inputs[0]), *c1 = cst(p->inputs[1]);
                if ((c0 != nullptr) == (c1 != nullptr) || (p->op == "Div" && !c1)) return cur;
                cur = p->inputs[c0 ? 1 : 0];
            }
        }
    };
    GraphIndex gi;
    void IndexGraph();
    // the part of an attention between the [., L, 3, H, hd] Reshape and the [., L, D] Reshape, matched from its Softmax and the name of its scores
    struct AttnCore { const OnnxNode *rs = nullptr, *orr = nullptr; std::vector<const OnnxNode*> taken; double scale = 1.0; std::vector<int64_t> shape5, shape3; };
    AttnCore MatchAttentionCore(const OnnxNode& sm, const OnnxNode* pv, const std::string& scores, const std::string& miss_prefix);
    // MatchWindowAttention: the shifted-window attention regions of a Swin export.  wattn_head: the rank-5 Reshape of a region -> what
    // ImportWindowAttention needs; view_alias: the last node of a partition / of a reverse -> the name whose channels-last value its output renames;
    // wattn_skip: the other nodes of the regions (they import nothing); wattn_softmax: the Softmax nodes MatchAttention must leave alone
    struct WinMatch {
        int64_t heads = 0, head_dim = 0, wh = 0, ww = 0, nh = 0, nw = 0, sh = 0, sw = 0;
        bool masked = false;
        double scale = 1.0;
        std::vector<float> bias, mask;
        std::string out, name;
    };
    std::map<const OnnxNode*, WinMatch> wattn_head;
    std::map<const OnnxNode*, std::string> view_alias;
    std::set<const OnnxNode*> wattn_skip, wattn_softmax;
    void MatchWindowAttention();
    void ImportWindowAttention(const OnnxNode& on, const WinMatch& wm);
    // MatchPatchMerge: the eight strided Slices and the Concat(axis -1) of a Swin patch merging.  merge_head: the Concat -> the sliced name
    std::map<const OnnxNode*, std::string> merge_head;
    void MatchPatchMerge();
    void ImportPatchMerge(const OnnxNode& on, const std::string& src);
    // MatchEmbed: the token-embedding sums of a BERT-class export.  embed_head: the LayerNormalization behind a sum -> what ImportEmbed needs;
    // embed_skip: the Gathers, Adds and position-id nodes of the sums (they import nothing)
    // (sum_only: the head is the sum's last Add, not a LayerNormalization: a pre-LN model, whose sum has other readers)
    struct EmbedMatch { std::vector<std::string> ids; std::vector<const OnnxTensor*> tables; std::vector<float> pos; std::string names; bool sum_only = false; };
    std::map<const OnnxNode*, EmbedMatch> embed_head;
    std::set<const OnnxNode*> embed_skip;
    void MatchEmbed();
    void ImportEmbed(const OnnxNode& on, const EmbedMatch& em);
    void EmitEmbed(const LNode& n, Step& s);
    // MatchGroupNorm: the spellings of a group norm.  gn_head: the last node of a match -> what ImportGroupNorm needs; gn_skip: its other nodes
    struct GnMatch {
        char form = 'a';                       // 'a' Reshape -> InstanceNormalization -> Reshape [-> Mul] [-> Add], 'b' GroupNormalization, 'c' InstanceNormalization on the map
        std::string x, out, name, in_name;     // in_name: the InstanceNormalization / GroupNormalization node (messages)
        int64_t groups = 0;                    // form c: the channel count, known at the import
        float eps = 1e-5f;
        std::vector<int64_t> shape1, back;     // form a: the two Reshape targets; back empty: Shape(x)
        const OnnxTensor *scale = nullptr, *bias = nullptr, *gamma = nullptr, *beta = nullptr;
        std::string gamma_name, beta_name;
    };
    std::map<const OnnxNode*, GnMatch> gn_head;
    std::set<const OnnxNode*> gn_skip;
    void MatchGroupNorm();
    void ImportGroupNorm(const OnnxNode& on, const GnMatch& gm);
    void FuseGroupNormActivations();
    void EmitGroupNorm(const LNode& n, Step& s);
    // MatchRmsNorm: an RMSNorm spelled out (Pow | Mul(x, x) -> ReduceMean -> Add eps -> Sqrt -> Div(1, .) | Reciprocal -> Mul x -> Mul weight, Casts to
    // FLOAT anywhere).  rms_head: its last Mul -> the RMSNormalization node (in synth_nodes) that imports in its place; rms_skip: its other nodes
    std::map<const OnnxNode*, const OnnxNode*> rms_head;
    std::set<const OnnxNode*> rms_skip;
    void MatchRmsNorm();
    bool FoldExpand(const OnnxNode& on, const LNode& n);
    bool ImportTokenView(const OnnxNode& on, LNode& n);
    void ImportTokenConcat(const OnnxNode& on, LNode& n, std::vector<int64_t>& odims);
    void push_node(LNode&& n, const std::string& out_name, const std::vector<int64_t>& odims, bool tok);
    void ImportLayerNorm(const OnnxNode& on, LNode& n, std::vector<int64_t>& odims);
    void ImportConv(const OnnxNode& on, LNode& n, std::vector<int64_t>& odims);
    void ImportConvTranspose(const OnnxNode& on, LNode& n, std::vector<int64_t>& odims);
    void ImportGemm(const OnnxNode& on, LNode& n, std::vector<int64_t>& odims);
    void ImportBatchNorm(const OnnxNode& on, LNode& n, std::vector<int64_t>& odims);
    void ImportArithmetic(const OnnxNode& on, LNode& n, std::vector<int64_t>& odims);
    void ImportActivation(const OnnxNode& on, LNode& n, std::vector<int64_t>& odims);
    void ImportConcat(const OnnxNode& on, LNode& n, std::vector<int64_t>& odims);
    void ImportPool(const OnnxNode& on, LNode& n, std::vector<int64_t>& odims);
    void ImportReshape(const OnnxNode& on, LNode& n, std::vector<int64_t>& odims);
    void ImportResize(const OnnxNode& on, LNode& n, std::vector<int64_t>& odims);

    // ---- graph-level fusions ----
    void FuseTokenAssemble();
    void FuseActivationPatterns();
    void FuseGatedActivations();
    void FuseSqueezeExcite();
    void MergeAffineChains();
    void FuseConvEpilogues();
    void FuseRelu6IntoDepthwise();
    void FuseActivationPrologues();
    void SwapConvAndAvgPool();
    void FusePrologues();
    void FuseTrailingRelu();

    // ---- where every value lives ----
    void StageNchwInputs();
    void DensifyOutputs();
    void PlaceConcatsAndAliases();
    void ComputeLiveness();
    void KeepDenseFusionInputsLive();
    void AssignBuffers();
    void alloc_buf(int r, std::multimap<int64_t, int>& free_pool);
    void MarkBufferTypes();

    // ---- logical nodes -> steps ----
    void EmitSteps();
    void EmitConcatCopies(const LNode& n);
    void EmitConv(const LNode& n, Step& s);
    void EmitGroupConv(const LNode& n, Step& s);
    void EmitTransposedConv(const LNode& n, Step& s);
    void ChooseBaseAlgo(const ConvFacts& f, Step& s) const;
    void ForceTileF8(const ConvFacts& f, Step& s) const;
    void ApplyForcedAlgo(const ConvFacts& f, Step& s) const;
    void ApplyForcedTileAndSplitK(const ConvFacts& f, Step& s);
    void EmitPool(const LNode& n, Step& s) const;
    void EmitSqueezeExcite(const LNode& n, Step& s);
    void EmitEltwise(const LNode& n, Step& s);
    void EmitResize(const LNode& n, Step& s) const;
    void EmitLayerNorm(const LNode& n, Step& s);
    void EmitTokenAssemble(const LNode& n, Step& s);
    void EmitAttention(const LNode& n, Step& s);
    void EmitKvAppend(const LNode& n, Step& s);
    void EmitWindowAttention(const LNode& n, Step& s);
    void EmitPatchMerge(const LNode& n, Step& s) const;

    // ---- step-level fusions, I/O descriptors ----
    void FuseDenseLayers();
    bool DenseLayerAt(size_t i) const;
    void FuseDenseBlocks();
    void FuseStemPool();
    void FuseDualF8();
    void DescribeIo();
};


}  // namespace

ModelInfo DescribeModel(const OnnxModel& m) {
    ModelInfo info;
    info.inputs = m.inputs;
    info.outputs = m.outputs;
    // EstimateModelMemoryUsage (model.cpp:979-1035): sum of I/O tensor bytes over positive dims + 10 MiB.
    auto elem = [](int t) -> size_t {
        switch (t) {
            case ONNX_FLOAT: case ONNX_INT32: return 4;
            case ONNX_INT64: return 8;
            case ONNX_UINT8: case ONNX_INT8: case ONNX_BOOL: return 1;
            case ONNX_FLOAT16: return 2;
            default: return 4;
        }
    };
    size_t total = 0;
    for (auto* list : {&m.inputs, &m.outputs})
        for (auto& vi : *list) {
            size_t n = 1;
            for (auto d : vi.dims) if (d > 0) n *= size_t(d);
            total += n * elem(vi.elem_type);
        }
    info.memory_usage_bytes = total + size_t(10) * 1024 * 1024;
    return info;
}

// ---- graph inputs ---------------------------------------------------------------------------
void Planner::ImportInputs() {
    if (input_shapes.size() != m.inputs.size())
        fail("Expected " + std::to_string(m.inputs.size()) + " inputs, got " + std::to_string(input_shapes.size()));
    for (size_t i = 0; i < m.inputs.size(); ++i) {
        const auto& vi = m.inputs[i];
        const auto& got = input_shapes[i];
        // INT64 [N, L]: token / type ids.  What may read one is MatchEmbed's business; every other non-float input is refused as before
        const bool i64 = vi.elem_type == ONNX_INT64 && vi.dims.size() == 2;
        if (vi.elem_type != ONNX_FLOAT && !i64) fail("Unsupported data type for input: " + vi.name);
        if (!vi.dims.empty()) {
            if (got.size() != vi.dims.size())
                fail("Invalid rank for input: " + vi.name + " Got: " + std::to_string(got.size()) +
                     " Expected: " + std::to_string(vi.dims.size()));
            for (size_t k = 0; k < got.size(); ++k)
                if (vi.dims[k] > 0 && vi.dims[k] != got[k])
                    fail("Got invalid dimensions for input: " + vi.name + " for the following indices index: " +
                         std::to_string(k) + " Got: " + std::to_string(got[k]) + " Expected: " + std::to_string(vi.dims[k]));
        }
        int v = L.new_val(vi.name, got);
        L.vals[v].is_input = true;
        L.vals[v].input_nchw = (L.vals[v].h * L.vals[v].w > 1);
        L.vals[v].is_i64 = i64;
    }
}

// a constant becomes an initializer under its output name (exporters write Clip bounds this way)
bool Planner::FoldConstantNode(const OnnxNode& on) {
    if (on.op != "Constant") return false;
    if (on.outputs.size() != 1 || on.attrs.size() != 1) fail("Constant " + on.name + ": expected one output and one value attribute");
    const OnnxAttr& at = on.attrs.begin()->second;
    OnnxTensor t;
    if (at.name == "value" && at.has_t) t = at.t;
    else if (at.name == "value_float") { t.dtype = ONNX_FLOAT; t.f = {at.f}; }
    else if (at.name == "value_floats") { t.dtype = ONNX_FLOAT; t.f = at.floats; t.dims = {int64_t(at.floats.size())}; }
    else if (at.name == "value_int") { t.dtype = ONNX_INT64; t.i = {at.i}; }
    else if (at.name == "value_ints") { t.dtype = ONNX_INT64; t.i = at.ints; t.dims = {int64_t(at.ints.size())}; }
    else fail("Constant " + on.name + ": the form '" + at.name + "' is not supported");
    t.name = on.outputs[0];
    L.add_derived(std::move(t));
    return true;
}

// Shape arithmetic: every shape is known at plan time, so Shape -> Gather / Slice -> Unsqueeze -> Concat (-> Cast), the way torch exports the
// `sizes` of an F.interpolate, folds into derived int64 initializers.  Only a Resize's `sizes` may read the result.  true: the node is done
bool Planner::FoldShapeArithmetic(const OnnxNode& on, const LNode& n) {
    const std::string& op = on.op;
    const bool folding = op == "Shape" || op == "Gather" || op == "Slice" || op == "Cast" || op == "Concat" || op == "Unsqueeze" || op == "Squeeze" ||
                         op == "Reshape" || op == "Flatten" || op == "Identity";
    bool from_shape = op == "Shape";
    for (size_t k = 0; k < on.inputs.size(); ++k) {
        if (!L.shape_derived.count(on.inputs[k])) continue;
        const bool sizes_in = (op == "Resize" && k == 3) || (op == "Expand" && k == 1);      // (an Expand of a constant folds: FoldExpand)
        if (!folding && !sizes_in)
            fail(op + " " + n.name + ": reads the shape arithmetic of a Shape node; shapes are only supported as the sizes of a Resize");
        from_shape = true;
    }
    if (from_shape && folding && op != "Shape" && !L.init(on.inputs[0]))
        fail(op + " " + n.name + ": reads the shape arithmetic of a Shape node; shapes are only supported as the sizes of a Resize");
    if (from_shape && folding) {
        OnnxTensor t;
        t.dtype = ONNX_INT64;
        auto const_in = [&](size_t k) -> const OnnxTensor& {
            const OnnxTensor* c = k < on.inputs.size() && !on.inputs[k].empty() ? L.init(on.inputs[k]) : nullptr;
            if (!c) fail(op + " " + n.name + ": shape arithmetic needs constant operands");
            return *c;
        };
        auto ints_of = [&](const OnnxTensor& c) {
            if (!c.i.empty() || c.numel() == 0) return c.i;
            std::vector<int64_t> v;
            for (float f : c.f) v.push_back(int64_t(f));
            return v;
        };
        if (op == "Shape") {
            const Val& X = L.vals[in_val(on, 0)];
            int64_t r = int64_t(X.dims.size());
            int64_t b = on.attr_i("start", 0), e = on.attr_i("end", r);
            if (b < 0) b += r;
            if (e < 0) e += r;
            b = std::clamp<int64_t>(b, 0, r);
            e = std::clamp<int64_t>(e, b, r);
            t.i.assign(X.dims.begin() + b, X.dims.begin() + e);
            t.dims = {e - b};
        } else if (op == "Gather") {
            const std::vector<int64_t> d = ints_of(const_in(0));
            const OnnxTensor& ix = const_in(1);
            if (const_in(0).dims.size() != 1 || on.attr_i("axis", 0) != 0) fail("Gather " + n.name + ": shape arithmetic only gathers from a 1-D shape");
            for (int64_t v : ints_of(ix)) {
                if (v < 0) v += int64_t(d.size());
                if (v < 0 || v >= int64_t(d.size())) fail("Gather " + n.name + ": index out of range");
                t.i.push_back(d[size_t(v)]);
            }
            t.dims = ix.dims;
        } else if (op == "Slice") {
            const std::vector<int64_t> d = ints_of(const_in(0));
            const int64_t r = int64_t(d.size());
            std::vector<int64_t> st = on.attr_ints("starts", {}), en = on.attr_ints("ends", {}), ax = on.attr_ints("axes", {0}), stp = {1};
            if (on.inputs.size() > 1) {              // opset >= 10: starts, ends, axes, steps are inputs
                st = ints_of(const_in(1));
                en = ints_of(const_in(2));
                if (on.inputs.size() > 3 && !on.inputs[3].empty()) ax = ints_of(const_in(3));
                if (on.inputs.size() > 4 && !on.inputs[4].empty()) stp = ints_of(const_in(4));
            }
            if (st.size() != 1 || en.size() != 1 || ax.size() != 1 || (ax[0] != 0 && ax[0] != -1) || stp.size() != 1 || stp[0] != 1)
                fail("Slice " + n.name + ": shape arithmetic only slices a 1-D shape with step 1");
            int64_t b = st[0] < 0 ? st[0] + r : st[0], e = en[0] < 0 ? en[0] + r : en[0];
            b = std::clamp<int64_t>(b, 0, r);
            e = std::clamp<int64_t>(e, b, r);
            t.i.assign(d.begin() + b, d.begin() + e);
            t.dims = {e - b};
        } else if (op == "Concat") {
            for (size_t k = 0; k < on.inputs.size(); ++k) {
                const OnnxTensor& c = const_in(k);
                if (c.dims.size() > 1) fail("Concat " + n.name + ": shape arithmetic only concatenates 1-D tensors (" + on.inputs[k] + " has rank " + std::to_string(c.dims.size()) + ")");
                const std::vector<int64_t> v = ints_of(c);
                t.i.insert(t.i.end(), v.begin(), v.end());
            }
            t.dims = {int64_t(t.i.size())};
        } else if (op == "Cast") {
            const OnnxTensor& c = const_in(0);
            const int64_t to = on.attr_i("to", ONNX_INT64);
            t = c;
            if (to == ONNX_INT64 || to == ONNX_INT32) { t.i = ints_of(c); t.f.clear(); t.dtype = int(to); }
            else if (to == ONNX_FLOAT || to == ONNX_DOUBLE) { t.f.clear(); for (int64_t v : ints_of(c)) t.f.push_back(float(v)); t.i.clear(); t.dtype = int(to); }
            else fail("Cast " + n.name + ": shape arithmetic only casts to integer or floating-point types");
        } else {
            t.dtype = -1;                            // Unsqueeze / Squeeze / Reshape / Flatten / Identity: the constant folding below
        }
        L.shape_derived.insert(on.outputs[0]);
        if (t.dtype != -1) {
            t.name = on.outputs[0];
            L.add_derived(std::move(t));
            return true;
        }
    }
    return false;
}

// shape-only ops on constants fold into a derived initializer (nothing is emitted).  true: the node is done
bool Planner::FoldShapeOnlyOp(const OnnxNode& on, const LNode& n) {
    const std::string& op = on.op;
    if (!((op == "Unsqueeze" || op == "Squeeze" || op == "Reshape" || op == "Flatten" || op == "Identity") && L.init(on.inputs[0]))) return false;
    OnnxTensor t = *L.init(on.inputs[0]);
    auto axes_of = [&]() {
        std::vector<int64_t> ax = on.attr_ints("axes", {});
        if (ax.empty() && on.inputs.size() > 1 && !on.inputs[1].empty()) {       // opset >= 13: axes is an input
            const OnnxTensor* at = L.init(on.inputs[1]);
            if (!at) fail(op + " " + n.name + ": axes must be an initializer");
            ax = at->i;
        }
        return ax;
    };
    if (op == "Unsqueeze") {
        std::vector<int64_t> ax = axes_of();
        if (ax.empty()) fail("Unsqueeze " + n.name + ": axes are required");
        const int64_t orank = int64_t(t.dims.size() + ax.size());
        for (auto& a : ax) { if (a < 0) a += orank; if (a < 0 || a >= orank) fail("Unsqueeze " + n.name + ": axis out of range"); }
        std::sort(ax.begin(), ax.end());
        std::vector<int64_t> nd;
        size_t src = 0;
        for (int64_t k = 0; k < orank; ++k) {
            if (std::binary_search(ax.begin(), ax.end(), k)) nd.push_back(1);
            else nd.push_back(t.dims.at(src++));
        }
        t.dims = nd;
    } else if (op == "Squeeze") {
        std::vector<int64_t> ax = axes_of();
        const int64_t rank = int64_t(t.dims.size());
        for (auto& a : ax) if (a < 0) a += rank;
        std::vector<int64_t> nd;
        for (int64_t k = 0; k < rank; ++k) {
            const bool listed = std::find(ax.begin(), ax.end(), k) != ax.end();
            if (listed && t.dims[size_t(k)] != 1) fail("Squeeze " + n.name + ": cannot squeeze a dimension of size != 1");
            if (ax.empty() ? t.dims[size_t(k)] != 1 : !listed) nd.push_back(t.dims[size_t(k)]);
        }
        t.dims = nd;
    } else if (op == "Reshape") {
        const OnnxTensor* shp = on.inputs.size() > 1 ? L.init(on.inputs[1]) : nullptr;
        std::vector<int64_t> d = shp ? shp->i : on.attr_ints("shape", {});
        if (d.empty() && t.numel() != 1) fail("Reshape " + n.name + ": shape must be an initializer");
        int64_t known = 1, neg = -1;
        for (size_t k = 0; k < d.size(); ++k) {
            if (d[k] == 0 && k < t.dims.size()) d[k] = t.dims[k];
            if (d[k] == -1) neg = int64_t(k); else known *= d[k];
        }
        if (neg >= 0 && known > 0) d[size_t(neg)] = t.numel() / known;
        int64_t tot = 1; for (auto v : d) tot *= v;
        if (tot != t.numel()) fail("Reshape " + n.name + ": element count mismatch");
        t.dims = d;
    } else if (op == "Flatten") {
        int64_t ax = on.attr_i("axis", 1);
        if (ax < 0) ax += int64_t(t.dims.size());
        int64_t a = 1, b = 1;
        for (size_t k = 0; k < t.dims.size(); ++k) (int64_t(k) < ax ? a : b) *= t.dims[k];
        t.dims = {a, b};
    }
    t.name = on.outputs[0];
    L.add_derived(std::move(t));
    return true;
}

void Planner::ImportConv(const OnnxNode& on, LNode& n, std::vector<int64_t>& odims) {
    if (!act_input(on, 0)) fail("Conv " + n.name + ": constant input is not supported");
    const OnnxTensor* w = L.init(on.inputs.at(1));
    if (!w || w->dims.size() != 4) fail("Conv " + n.name + ": weights must be a 4-D initializer");
    int x = in_val(on, 0);
    const Val& X = L.vals[x];
    if (X.dims.size() != 4) fail("Conv " + n.name + ": input must be 4-D");
    int64_t co = w->dims[0], ci = w->dims[1];
    const int64_t group = on.attr_i("group", 1);
    if (group < 1) fail("Conv " + n.name + ": group = " + std::to_string(group) + " must be positive");
    if (group != 1) {
        // depthwise: one filter per channel; the weights [C, 1, kh, kw] pack as [C][kh][kw] (= [Cout][kh][kw][Cin] with Cin = 1).
        // Any other group: output channel o reads input channels (o / (Cout / group)) * Cin / group ..., weights [Cout, Cin / group, kh, kw]
        if (X.c % group != 0)
            fail("Conv " + n.name + ": group = " + std::to_string(group) + " does not divide the input channels " + std::to_string(X.c));
        if (co % group != 0)
            fail("Conv " + n.name + ": group = " + std::to_string(group) + " does not divide the output channels " + std::to_string(co));
        if (ci != X.c / group)
            fail("Conv " + n.name + ": weight channels " + std::to_string(ci) + " != input channels / group = " + std::to_string(X.c / group));
        n.dw = group == X.c && co == group;
        // Grouped convolutions are opt-in: without IE_GROUPED_CONV=1 the planner keeps refusing them as it always has, so a model that
        // loads (or is refused) today is planned exactly as before
        if (!n.dw && !env.flag("IE_GROUPED_CONV"))
            fail("Conv " + n.name + ": group = " + std::to_string(group) + " is not supported (only depthwise grouped convolutions, with group == input "
                 "channels == output channels, are; set IE_GROUPED_CONV=1 to run the others on the grouped-convolution kernels)");
        n.group = group;
    } else if (ci != X.c) {
        fail("Conv " + n.name + ": input channels " + std::to_string(X.c) + " != weight channels " + std::to_string(ci));
    }
    n.kind = L_CONV;
    read_window_attrs(on, n, X.h, X.w, true, w);
    if (n.kh != w->dims[2] || n.kw != w->dims[3]) fail("Conv " + n.name + ": kernel_shape does not match weights");
    n.w.resize(size_t(co * ci * n.kh * n.kw));
    for (int64_t o = 0; o < co; ++o)
        for (int64_t c = 0; c < ci; ++c)
            for (int ky = 0; ky < n.kh; ++ky)
                for (int kx = 0; kx < n.kw; ++kx)
                    n.w[size_t(((o * n.kh + ky) * n.kw + kx) * ci + c)] =
                        w->f[size_t(((o * ci + c) * n.kh + ky) * n.kw + kx)];
    if (on.inputs.size() > 2 && !on.inputs[2].empty()) {
        const OnnxTensor* b = L.init(on.inputs[2]);
        if (!b || b->numel() != co) fail("Conv " + n.name + ": bias must be a [Cout] initializer");
        n.bias = b->f;
    }
    if (n.dil_h > 1 || n.dil_w > 1) {
        if (group != 1)
            fail("Conv " + n.name + ": dilated " + std::string(n.dw ? "depthwise" : "grouped") + " convolutions are not supported (dilations " +
                 std::to_string(n.dil_h) + "x" + std::to_string(n.dil_w) + ", group = " + std::to_string(group) + ")");
        // Centre-tap collapse (exact): stride 1, odd k, pads d * (k / 2) and d >= the image extent on every dilated axis.  The nearest
        // off-centre tap is d pixels from the output pixel, so it lands in the padding for EVERY output pixel: the conv is the 1x1 conv of
        // its centre weights (DeepLabV3's rate-36 ASPP branch at 28x28).  It then takes every 1x1 path, and its FLOPs are the 1x1's.
        auto centre_only = [](int k, int d, int s, int p0, int p1, int64_t len) {
            return k == 1 ? (p0 == 0 && p1 == 0) : (s == 1 && k % 2 == 1 && p0 == d * (k / 2) && p1 == p0 && d >= len);
        };
        if (centre_only(n.kh, n.dil_h, n.sh, n.pt, n.pb, X.h) && centre_only(n.kw, n.dil_w, n.sw, n.pl, n.pr, X.w)) {
            std::vector<float> wc(size_t(co * ci));
            for (int64_t o = 0; o < co; ++o)
                for (int64_t c = 0; c < ci; ++c) wc[size_t(o * ci + c)] = n.w[size_t(((o * n.kh + n.kh / 2) * n.kw + n.kw / 2) * ci + c)];
            n.w = std::move(wc);
            n.kh = n.kw = 1;
            n.pt = n.pl = n.pb = n.pr = 0;
            n.dil_h = n.dil_w = 1;
        }
    }
    int64_t oh, ow;
    conv_out_hw(X.h, X.w, n, false, oh, ow);
    n.in = {x};
    odims = {X.n, co, oh, ow};
}

// ConvTranspose: out[n, o, iy * sh + ky - pt, ix * sw + kx - pl] += x[n, c, iy, ix] * W[c, o, ky, kx].  The weights [Cin, Cout, kh, kw] pack as
// [kh][kw][Cout][Cin]: each tap is one [Cout][Cin] GEMM operand.
void Planner::ImportConvTranspose(const OnnxNode& on, LNode& n, std::vector<int64_t>& odims) {
    if (!act_input(on, 0)) fail("ConvTranspose " + n.name + ": constant input is not supported");
    const OnnxTensor* w = L.init(on.inputs.at(1));
    if (!w || w->dims.size() != 4) fail("ConvTranspose " + n.name + ": weights must be a 4-D initializer");
    int x = in_val(on, 0);
    const Val& X = L.vals[x];
    if (X.dims.size() != 4) fail("ConvTranspose " + n.name + ": input must be 4-D");
    const int64_t group = on.attr_i("group", 1);
    if (group != 1) fail("ConvTranspose " + n.name + ": group = " + std::to_string(group) + " is not supported (only group = 1 is)");
    const int64_t ci = w->dims[0], co = w->dims[1];
    if (ci != X.c) fail("ConvTranspose " + n.name + ": input channels " + std::to_string(X.c) + " != weight channels " + std::to_string(ci));
    std::vector<int64_t> ks = on.attr_ints("kernel_shape", {w->dims[2], w->dims[3]});
    if (ks.size() != 2) fail("node " + on.name + ": only 2-D kernels are supported");
    if (ks[0] != w->dims[2] || ks[1] != w->dims[3]) fail("ConvTranspose " + n.name + ": kernel_shape does not match weights");
    auto st = on.attr_ints("strides", {1, 1});
    auto dl = on.attr_ints("dilations", {1, 1});
    auto pads = on.attr_ints("pads", {0, 0, 0, 0});
    auto op = on.attr_ints("output_padding", {0, 0});
    if (st.size() != 2 || st[0] < 1 || st[1] < 1) fail("ConvTranspose " + n.name + ": strides must be two positive integers");
    if (dl.size() != 2 || dl[0] < 1 || dl[1] < 1) fail("node " + on.name + ": dilations must be two positive integers");
    if (dl[0] != 1 || dl[1] != 1)
        fail("ConvTranspose " + n.name + ": dilated transposed convolutions are not supported (dilations " + std::to_string(dl[0]) + "x" + std::to_string(dl[1]) + ")");
    if (pads.size() != 4 || pads[0] < 0 || pads[1] < 0 || pads[2] < 0 || pads[3] < 0) fail("node " + on.name + ": pads must have 4 non-negative entries");
    auto ap = on.attrs.find("auto_pad");
    if (ap != on.attrs.end() && !ap->second.s.empty() && ap->second.s != "NOTSET") {
        if (ap->second.s == "VALID") pads = {0, 0, 0, 0};
        else fail("ConvTranspose " + n.name + ": auto_pad " + ap->second.s + " is not supported (NOTSET and VALID are)");
    }
    if (on.attrs.count("output_shape")) fail("ConvTranspose " + n.name + ": the output_shape attribute is not supported (give pads and output_padding)");
    if (op.size() != 2 || op[0] < 0 || op[1] < 0) fail("ConvTranspose " + n.name + ": output_padding must be two non-negative integers");
    if (op[0] >= st[0] || op[1] >= st[1])
        fail("ConvTranspose " + n.name + ": output_padding " + std::to_string(op[0]) + "x" + std::to_string(op[1]) + " must be smaller than the strides " +
             std::to_string(st[0]) + "x" + std::to_string(st[1]));
    n.kind = L_CONV;
    n.transposed = true;
    n.kh = int(ks[0]); n.kw = int(ks[1]);
    n.sh = int(st[0]); n.sw = int(st[1]);
    n.pt = int(pads[0]); n.pl = int(pads[1]); n.pb = int(pads[2]); n.pr = int(pads[3]);
    n.op_h = int(op[0]); n.op_w = int(op[1]);
    const int64_t oh = (X.h - 1) * n.sh + n.kh - n.pt - n.pb + n.op_h, ow = (X.w - 1) * n.sw + n.kw - n.pl - n.pr + n.op_w;
    if (oh < 1 || ow < 1) fail("ConvTranspose " + n.name + ": the output would be empty (" + std::to_string(oh) + "x" + std::to_string(ow) + ")");
    n.w.resize(size_t(co * ci * n.kh * n.kw));
    for (int64_t c = 0; c < ci; ++c)
        for (int64_t o = 0; o < co; ++o)
            for (int ky = 0; ky < n.kh; ++ky)
                for (int kx = 0; kx < n.kw; ++kx)
                    n.w[size_t(((int64_t(ky) * n.kw + kx) * co + o) * ci + c)] = w->f[size_t(((c * co + o) * n.kh + ky) * n.kw + kx)];
    if (on.inputs.size() > 2 && !on.inputs[2].empty()) {
        const OnnxTensor* b = L.init(on.inputs[2]);
        if (!b || b->numel() != co) fail("ConvTranspose " + n.name + ": bias must be a [Cout] initializer");
        n.bias = b->f;
    }
    n.in = {x};
    odims = {X.n, co, oh, ow};
}

void Planner::ImportGemm(const OnnxNode& on, LNode& n, std::vector<int64_t>& odims) {
    const std::string& op = on.op;
    if (!act_input(on, 0)) fail(op + " " + n.name + ": constant first operand is not supported");
    // (a product of two activations exists only inside the attention pattern, which MatchAttention took)
    if (op == "MatMul" && act_input(on, 1)) fail("Unsupported ONNX operator: MatMul (node " + n.name + ")");
    const OnnxTensor* b = L.init(on.inputs.at(1));
    if (!b || b->dims.size() != 2) fail(op + " " + n.name + ": second operand must be a 2-D initializer");
    int x = in_val(on, 0);
    const Val& X = L.vals[x];
    // a channels-last view [N, H, W, K] times [K, N']: the 1x1 conv of its pixels (ConvNeXt's Linear layers), the result channels-last again
    // (a token view [N, L, K] likewise: the 1x1 conv of its L token rows)
    const bool tok = L.is_tok(on.inputs[0]);
    const bool cl = L.is_cl(on.inputs[0]) || tok;
    if (!cl && X.h * X.w != 1) fail(op + " " + n.name + ": input must be [N, K]");
    bool transB = op == "Gemm" && on.attr_i("transB", 0) != 0;
    if (op == "Gemm" && on.attr_i("transA", 0) != 0) fail("Gemm " + n.name + ": transA is not supported");
    float alpha = op == "Gemm" ? on.attr_f("alpha", 1.f) : 1.f;
    float beta = op == "Gemm" ? on.attr_f("beta", 1.f) : 1.f;
    int64_t K = transB ? b->dims[1] : b->dims[0], N = transB ? b->dims[0] : b->dims[1];
    if (K != X.c) fail(op + " " + n.name + ": inner dimensions do not match");
    // (a vocabulary head: the conv kernels' eligibility keeps 32-bit kernels off spans of 2^31 bytes and more, and no kernel is checked beyond them)
    if (tok && X.n * X.w * N * 4 >= (int64_t(1) << 31))
        fail(op + " " + n.name + ": the result [" + std::to_string(X.n) + ", " + std::to_string(X.w) + ", " + std::to_string(N) + "] holds 2^31 bytes or more in fp32; no conv kernel runs on such a span (use a smaller batch)");
    n.kind = L_CONV;
    n.w.resize(size_t(N * K));
    for (int64_t o = 0; o < N; ++o)
        for (int64_t k = 0; k < K; ++k)
            n.w[size_t(o * K + k)] = alpha * (transB ? b->f[size_t(o * K + k)] : b->f[size_t(k * N + o)]);
    if (op == "Gemm" && on.inputs.size() > 2 && !on.inputs[2].empty()) {
        const OnnxTensor* c = L.init(on.inputs[2]);
        if (!c) fail("Gemm " + n.name + ": C must be an initializer");
        if (c->numel() == N) n.bias = c->f;
        else if (c->numel() == 1) n.bias.assign(size_t(N), c->f[0]);
        else fail("Gemm " + n.name + ": C must broadcast over rows");
        for (auto& v : n.bias) v *= beta;
    }
    n.in = {x};
    odims = {X.n, N};
    if (X.dims.size() == 1) odims = {N};
    if (cl) { odims = {X.n, N, X.h, X.w}; cl_out = !tok; tok_out = tok; }
}

void Planner::ImportBatchNorm(const OnnxNode& on, LNode& n, std::vector<int64_t>& odims) {
    int x = in_val(on, 0);
    const Val& X = L.vals[x];
    const OnnxTensor *g = L.init(on.inputs.at(1)), *be = L.init(on.inputs.at(2)), *mu = L.init(on.inputs.at(3)),
                     *var = L.init(on.inputs.at(4));
    if (!g || !be || !mu || !var) fail("BatchNormalization " + n.name + ": parameters must be initializers");
    if (g->numel() != X.c || be->numel() != X.c || mu->numel() != X.c || var->numel() != X.c)
        fail("BatchNormalization " + n.name + ": parameter size != channels");
    double eps = on.attr_f("epsilon", 1e-5f);
    n.kind = L_AFFINE;
    n.s.resize(size_t(X.c)); n.t.resize(size_t(X.c));
    for (int64_t c = 0; c < X.c; ++c) {
        double s = double(g->f[c]) / std::sqrt(double(var->f[c]) + eps);
        n.s[c] = float(s);
        n.t[c] = float(double(be->f[c]) - double(mu->f[c]) * s);
    }
    n.in = {x};
    odims = X.dims;
}

// Add / Mul / Div: of two activations (L_ADD, L_MUL), or of an activation and a per-channel constant (L_AFFINE)
void Planner::ImportArithmetic(const OnnxNode& on, LNode& n, std::vector<int64_t>& odims) {
    const std::string& op = on.op;
    bool a0 = act_input(on, 0), a1 = act_input(on, 1);
    if (op == "Div" && (a1 || !a0)) fail("Div " + n.name + ": only the division of an activation by a constant is supported");
    if (a0 && a1 && L.is_cl(on.inputs[0]) != L.is_cl(on.inputs[1]))
        fail(op + " " + n.name + ": the operands mix a channels-last view and an NCHW value");
    cl_out = (a0 && L.is_cl(on.inputs[0])) || (a1 && L.is_cl(on.inputs[1]));
    tok_out = (a0 && L.is_tok(on.inputs[0])) || (a1 && L.is_tok(on.inputs[1]));
    if (a0 && a1 && L.is_tok(on.inputs[0]) != L.is_tok(on.inputs[1]))
        fail(op + " " + n.name + ": the operands mix a token view and another value");
    if (a0 && a1 && op == "Mul") {
        // same shapes, or [N,C,H,W] x [N,C,1,1] in either order (a squeeze-excite gate); in[0] = the full tensor
        int a = in_val(on, 0), b = in_val(on, 1);
        const Val &A = L.vals[a], &Bv = L.vals[b];
        const bool bcast_b = A.dims.size() == 4 && Bv.dims.size() == 4 && A.n == Bv.n && A.c == Bv.c && Bv.h == 1 && Bv.w == 1;
        const bool bcast_a = A.dims.size() == 4 && Bv.dims.size() == 4 && A.n == Bv.n && A.c == Bv.c && A.h == 1 && A.w == 1;
        if (A.dims != Bv.dims) {
            if (bcast_a && !bcast_b) std::swap(a, b);
            else if (!bcast_b) fail("Mul " + n.name + ": only same-shape activations or [N,C,H,W] x [N,C,1,1] broadcasting are supported between two activations");
        }
        n.kind = L_MUL;
        n.in = {a, b};
        odims = L.vals[a].dims;
    } else if (a0 && a1) {
        int a = in_val(on, 0), b = in_val(on, 1);
        if (L.vals[a].dims != L.vals[b].dims) fail("Add " + n.name + ": broadcasting between activations is not supported");
        n.kind = L_ADD;
        n.in = {a, b};
        odims = L.vals[a].dims;
    } else if (a0 || a1) {
        int x = in_val(on, a0 ? 0 : 1);
        const OnnxTensor* c = L.init(on.inputs[a0 ? 1 : 0]);
        std::vector<float> pc;
        // rank-1 constant against a rank-2 activation aligns with the last (= channel) axis
        const Val& X = L.vals[x];
        // opset < 7 (Caffe2-era exports): Add/Mul carry broadcast=1 and an axis that places the constant's dims inside the
        // activation's (axis=1 with a [C] constant = per channel); without an axis the constant aligns with the trailing dims
        int64_t legacy_axis = -1;
        if (m.opset > 0 && m.opset < 7 && on.attr_i("broadcast", 0) != 0 && on.attrs.count("axis")) {
            legacy_axis = on.attr_i("axis", 0);
            if (legacy_axis < 0) legacy_axis += int64_t(X.dims.size());
        }
        if (m.opset > 0 && m.opset < 7 && on.attr_i("broadcast", 0) == 0 && c->dims != X.dims && c->numel() != 1)
            fail(op + " " + n.name + ": operand shapes differ and the opset-" + std::to_string(m.opset) + " broadcast attribute is not set");
        if (tok_out && op == "Add" && X.w > 1 && c->numel() == X.w * X.c && (c->dtype == ONNX_FLOAT || c->dtype == ONNX_DOUBLE || c->dtype == ONNX_FLOAT16) &&
            (c->dims == std::vector<int64_t>{1, X.w, X.c} || c->dims == std::vector<int64_t>{X.w, X.c})) {
            // a position embedding: FuseTokenAssemble folds it into the class-token concat in front of it, or refuses it
            n.kind = L_TOKPOS;
            n.t = c->f;
            n.in = {x};
            odims = X.dims;
            return;
        }
        bool ok = !cl_out && !tok_out && L.per_channel_const(*c, X, pc, legacy_axis);
        if (tok_out) {
            const bool flt = c->dtype == ONNX_FLOAT || c->dtype == ONNX_DOUBLE || c->dtype == ONNX_FLOAT16;
            if (flt && c->numel() == 1) { pc.assign(size_t(X.c), c->f[0]); ok = true; }
            else if (flt && c->numel() == X.c && c->dims.size() <= 3 && !c->dims.empty() && c->dims.back() == X.c) { pc = c->f; ok = true; }
            if (!ok) fail(op + " " + n.name + ": constant operand must broadcast along the last axis of the token view " + on.inputs[a0 ? 0 : 1] +
                          " (or be the [1, L, D] position embedding added directly behind the class-token Concat)");
        }
        if (cl_out) {
            // against the ONNX dims [N, H, W, C] numpy broadcasting puts the channels last: a scalar, [C], [1, C] ... [1, 1, 1, C]
            const bool flt = c->dtype == ONNX_FLOAT || c->dtype == ONNX_DOUBLE || c->dtype == ONNX_FLOAT16;
            if (flt && c->numel() == 1) { pc.assign(size_t(X.c), c->f[0]); ok = true; }
            else if (flt && c->numel() == X.c && c->dims.size() <= 4 && !c->dims.empty() && c->dims.back() == X.c) { pc = c->f; ok = true; }
            if (!ok) fail(op + " " + n.name + ": constant operand must broadcast along the last axis of the channels-last view " + on.inputs[a0 ? 0 : 1]);
        }
        if (!ok && X.dims.size() == 2 && c->dims.size() == 1 && c->numel() == X.c) { pc = c->f; ok = true; }
        if (!ok && X.dims.size() == 2 && c->dims.size() == 2 && c->dims[0] == 1 && c->dims[1] == X.c) { pc = c->f; ok = true; }
        if (!ok) fail(op + " " + n.name + ": constant operand must broadcast per channel");
        n.kind = L_AFFINE;
        if (op == "Add") { n.s.assign(size_t(X.c), 1.f); n.t = pc; }
        else if (op == "Div") {
            // x / c = x * (1 / c): an affine step like a Mul (hardswish exports that end in "/ 6")
            for (float& v : pc) {
                if (v == 0.f) fail("Div " + n.name + ": division by zero");
                v = 1.f / v;
            }
            n.s = pc;
            n.t.assign(size_t(X.c), 0.f);
        }
        else { n.s = pc; n.t.assign(size_t(X.c), 0.f); }
        n.in = {x};
        odims = X.dims;
    } else fail(op + " " + n.name + ": constant folding of two initializers is not supported");
}

// Clip, Sigmoid / HardSigmoid / HardSwish / Gelu, Relu, Erf
void Planner::ImportActivation(const OnnxNode& on, LNode& n, std::vector<int64_t>& odims) {
    const std::string& op = on.op;
    if (op == "Clip") {
        // opset < 11: min / max attributes; opset >= 11: optional scalar inputs 2 and 3 (absent or "" = unbounded)
        n.kind = L_CLIP;
        n.in = {in_val(on, 0)};
        odims = L.vals[n.in[0]].dims;
        if (on.attrs.count("min")) n.lo = on.attr_f("min", -kInf);
        if (on.attrs.count("max")) n.hi = on.attr_f("max", kInf);
        for (size_t k = 1; k < 3 && k < on.inputs.size(); ++k) {
            if (on.inputs[k].empty()) continue;
            const OnnxTensor* b = L.init(on.inputs[k]);
            if (!b) fail("Clip " + n.name + ": the " + (k == 1 ? "min" : "max") + " bound must be a constant (initializer or Constant node)");
            if (b->numel() != 1 || (b->dtype != ONNX_FLOAT && b->dtype != ONNX_DOUBLE && b->dtype != ONNX_FLOAT16))
                fail("Clip " + n.name + ": the " + (k == 1 ? "min" : "max") + " bound must be a floating-point scalar");
            (k == 1 ? n.lo : n.hi) = b->f[0];
        }
    } else if (op == "Relu") {
        n.kind = L_RELU;
        n.in = {in_val(on, 0)};
        odims = L.vals[n.in[0]].dims;
    } else if (op == "Erf") {
        // only as the middle of the five-node GELU pattern (FuseActivationPatterns); alone it is refused there
        if (!act_input(on, 0)) fail(op + " " + n.name + ": constant input is not supported");
        n.kind = L_ERF;
        n.in = {in_val(on, 0)};
        odims = L.vals[n.in[0]].dims;
        cl_out = L.is_cl(on.inputs[0]);
        tok_out = L.is_tok(on.inputs[0]);
    } else {
        n.kind = L_ACT;
        if (op == "Gelu") {
            const auto ap = on.attrs.find("approximate");
            const std::string mode = ap == on.attrs.end() || ap->second.s.empty() ? "none" : ap->second.s;
            if (mode != "none" && mode != "tanh") fail("Gelu " + n.name + ": approximate '" + mode + "' is not supported (none and tanh are)");
            n.act.kind = mode == "tanh" ? ActKind::GeluTanh : ActKind::Gelu;
            cl_out = L.is_cl(on.inputs[0]);
            tok_out = L.is_tok(on.inputs[0]);
        }
        else if (op == "Tanh") n.act.kind = ActKind::Tanh;
        else if (op == "Sigmoid") { n.act.kind = ActKind::Sigmoid; tok_out = L.is_tok(on.inputs[0]); }      // (on tokens: the SiLU of a gated MLP)
        else if (op == "HardSigmoid") { n.act.kind = ActKind::HardSigmoid; n.act.a = on.attr_f("alpha", 0.2f); n.act.b = on.attr_f("beta", 0.5f); }
        else { n.act.kind = ActKind::HardSwish; n.act.a = 1.f / 6.f; n.act.b = 0.5f; }
        if (!act_input(on, 0)) fail(op + " " + n.name + ": constant input is not supported");
        n.in = {in_val(on, 0)};
        odims = L.vals[n.in[0]].dims;
    }
}

void Planner::ImportConcat(const OnnxNode& on, LNode& n, std::vector<int64_t>& odims) {
    for (const std::string& name : on.inputs)
        if (L.is_tok(name)) { ImportTokenConcat(on, n, odims); return; }
    int64_t axis = on.attr_i("axis", 1);
    n.kind = L_CONCAT;
    for (size_t k = 0; k < on.inputs.size(); ++k) {
        if (!act_input(on, k)) fail("Concat " + n.name + ": constant inputs are not supported");
        n.in.push_back(in_val(on, k));
    }
    const Val& X0 = L.vals[n.in[0]];
    if (axis < 0) axis += int64_t(X0.dims.size());
    if (axis != 1) fail("Concat " + n.name + ": only axis=1 (channels) is supported");
    odims = X0.dims;
    int64_t ctot = 0;
    for (int v : n.in) {
        const Val& X = L.vals[v];
        if (X.dims.size() != X0.dims.size()) fail("Concat " + n.name + ": rank mismatch");
        for (size_t k = 0; k < X.dims.size(); ++k)
            if (k != 1 && X.dims[k] != X0.dims[k]) fail("Concat " + n.name + ": shape mismatch");
        ctot += X.c;
    }
    odims[1] = ctot;
}

// MaxPool / AveragePool / GlobalAveragePool
void Planner::ImportPool(const OnnxNode& on, LNode& n, std::vector<int64_t>& odims) {
    const std::string& op = on.op;
    if (op == "GlobalAveragePool") {
        int x = in_val(on, 0);
        const Val& X = L.vals[x];
        if (X.dims.size() != 4) fail("GlobalAveragePool " + n.name + ": input must be 4-D");
        n.kind = L_GAP;
        n.in = {x};
        odims = {X.n, X.c, 1, 1};
        return;
    }
    int x = in_val(on, 0);
    const Val& X = L.vals[x];
    if (X.dims.size() != 4) fail(op + " " + n.name + ": input must be 4-D");
    if (on.outputs.size() > 1 && !on.outputs[1].empty()) fail("MaxPool " + n.name + ": Indices output is not supported");
    n.kind = op == "MaxPool" ? L_MAXPOOL : L_AVGPOOL;
    read_window_attrs(on, n, X.h, X.w, false, nullptr);
    n.count_include_pad = on.attr_i("count_include_pad", 0) != 0;
    int64_t oh, ow;
    conv_out_hw(X.h, X.w, n, on.attr_i("ceil_mode", 0) != 0, oh, ow);
    n.in = {x};
    odims = {X.n, X.c, oh, ow};
}

// The ops that only rename storage: Unsqueeze, Flatten, Reshape, Squeeze, Identity, Dropout
void Planner::ImportReshape(const OnnxNode& on, LNode& n, std::vector<int64_t>& odims) {
    const std::string& op = on.op;
    if (op == "Unsqueeze") {
        // [N,C] -> [N,C,1,1]: storage is unchanged when only trailing unit axes are added
        int x = in_val(on, 0);
        const Val& X = L.vals[x];
        std::vector<int64_t> ax = on.attr_ints("axes", {});
        if (ax.empty() && on.inputs.size() > 1) { const OnnxTensor* at = L.init(on.inputs[1]); if (at) ax = at->i; }
        const int64_t orank = int64_t(X.dims.size() + ax.size());
        for (auto& a : ax) if (a < 0) a += orank;
        std::sort(ax.begin(), ax.end());
        if (ax.empty() || X.h * X.w != 1 || X.dims.size() < 2 || ax[0] < int64_t(X.dims.size()) || orank > 4)
            fail("Unsqueeze " + n.name + ": only trailing unit axes on [N,C] tensors are supported");
        n.kind = L_ALIAS;
        n.in = {x};
        odims = X.dims;
        while (int64_t(odims.size()) < orank) odims.push_back(1);
        return;
    }
    int x = in_val(on, 0);
    const Val& X = L.vals[x];
    n.kind = L_ALIAS;
    n.in = {x};
    if (op == "Identity" || op == "Dropout") odims = X.dims;
    else {
        // Storage is NHWC: a reshape is a pure alias only when H*W == 1 on both sides.
        if (X.h * X.w != 1) fail(op + " " + n.name + ": only supported on [N,C,1,1] / [N,C] tensors");
        if (op == "Flatten") {
            if (on.attr_i("axis", 1) != 1) fail("Flatten " + n.name + ": only axis=1 is supported");
            odims = {X.n, X.c};
        } else if (op == "Squeeze") odims = {X.n, X.c};
        else {
            const OnnxTensor* shp = on.inputs.size() > 1 ? L.init(on.inputs[1]) : nullptr;
            if (!shp) fail("Reshape " + n.name + ": shape must be an initializer");
            std::vector<int64_t> d = shp->i;
            int64_t known = 1, neg = -1;
            for (size_t k = 0; k < d.size(); ++k) {
                if (d[k] == 0 && k < X.dims.size()) d[k] = X.dims[k];
                if (d[k] == -1) neg = int64_t(k); else known *= d[k];
            }
            if (neg >= 0) d[size_t(neg)] = X.n * X.c / known;
            int64_t tot = 1; for (auto v : d) tot *= v;
            if (tot != X.n * X.c || d.empty() || d[0] != X.n) fail("Reshape " + n.name + ": must keep the batch axis");
            for (size_t k = 2; k < d.size(); ++k) if (d[k] != 1) fail("Reshape " + n.name + ": unsupported target shape");
            odims = d;
        }
    }
}

// Resize-10 / 11 / 13 / 18 / 19 and Upsample-7 / 9 over 4-D tensors, scaling H and W only.  Resize-10 and Upsample have no
// coordinate_transformation_mode: they are `asymmetric` (with floor rounding for nearest, what the opset-10 definitions compute)
void Planner::ImportResize(const OnnxNode& on, LNode& n, std::vector<int64_t>& odims) {
    const std::string& op = on.op;
    if (!act_input(on, 0)) fail(op + " " + n.name + ": constant input is not supported");
    const int x = in_val(on, 0);
    const Val& X = L.vals[x];
    if (X.dims.size() != 4) fail(op + " " + n.name + ": only 4-D inputs are supported");
    const bool legacy = op == "Upsample" || m.opset < 11;
    std::string mode = "nearest";
    if (on.attrs.count("mode")) mode = on.attrs.at("mode").s;
    if (mode == "nearest") n.rs_mode = ResizeMode::Nearest;
    else if (mode == "linear" || mode == "bilinear") n.rs_mode = ResizeMode::Linear;
    else fail(op + " " + n.name + ": mode '" + mode + "' is not supported (nearest and linear are)");
    std::string coord = legacy ? "asymmetric" : "half_pixel";
    if (!legacy && on.attrs.count("coordinate_transformation_mode")) coord = on.attrs.at("coordinate_transformation_mode").s;
    if (coord == "half_pixel") n.rs_coord = ResizeCoord::HalfPixel;
    else if (coord == "pytorch_half_pixel") n.rs_coord = ResizeCoord::PytorchHalfPixel;
    else if (coord == "align_corners") n.rs_coord = ResizeCoord::AlignCorners;
    else if (coord == "asymmetric") n.rs_coord = ResizeCoord::Asymmetric;
    else fail(op + " " + n.name + ": coordinate_transformation_mode '" + coord + "' is not supported");
    std::string nearest = legacy ? "floor" : "round_prefer_floor";
    if (!legacy && on.attrs.count("nearest_mode")) nearest = on.attrs.at("nearest_mode").s;
    if (nearest == "round_prefer_floor") n.rs_nearest = ResizeNearest::RoundPreferFloor;
    else if (nearest == "round_prefer_ceil") n.rs_nearest = ResizeNearest::RoundPreferCeil;
    else if (nearest == "floor") n.rs_nearest = ResizeNearest::Floor;
    else if (nearest == "ceil") n.rs_nearest = ResizeNearest::Ceil;
    else fail(op + " " + n.name + ": nearest_mode '" + nearest + "' is not supported");
    if (on.attr_i("antialias", 0) != 0) fail(op + " " + n.name + ": antialias = 1 is not supported");
    if (on.attrs.count("keep_aspect_ratio_policy") && on.attrs.at("keep_aspect_ratio_policy").s != "stretch")
        fail(op + " " + n.name + ": keep_aspect_ratio_policy '" + on.attrs.at("keep_aspect_ratio_policy").s + "' is not supported (stretch is)");
    const bool has_axes = on.attrs.count("axes") != 0;
    std::vector<int64_t> axes = on.attr_ints("axes", {0, 1, 2, 3});
    for (auto& a : axes) {
        if (a < 0) a += 4;
        if (a < 0 || a > 3 || (has_axes && a < 2)) fail(op + " " + n.name + ": axes must be a subset of {2, 3}");
    }
    // the scales / sizes operand: Upsample-7 an attribute, Upsample-9 / Resize-10 input 1, Resize-11+ input 2 (scales) or 3 (sizes)
    auto operand = [&](size_t k) -> const OnnxTensor* {
        if (k >= on.inputs.size() || on.inputs[k].empty()) return nullptr;
        const OnnxTensor* t = L.init(on.inputs[k]);
        if (!t) fail(op + " " + n.name + ": " + (k == 3 ? "sizes" : "scales") + " must be a constant (initializer or Constant node)");
        return t->numel() == 0 ? nullptr : t;
    };
    std::vector<double> scales;
    std::vector<int64_t> sizes;
    if (op == "Upsample" && on.attrs.count("scales")) for (float f : on.attrs.at("scales").floats) scales.push_back(f);
    else if (legacy) { if (const OnnxTensor* t = operand(1)) for (float f : t->f) scales.push_back(f); }
    else {
        if (const OnnxTensor* t = operand(2)) for (float f : t->f) scales.push_back(f);
        if (const OnnxTensor* t = operand(3)) sizes = t->i;
        if (!scales.empty() && !sizes.empty()) fail(op + " " + n.name + ": only one of scales and sizes may be given");
    }
    if (scales.empty() && sizes.empty()) fail(op + " " + n.name + ": scales or sizes must be given");
    const size_t cnt = scales.empty() ? sizes.size() : scales.size();
    if (cnt != axes.size()) fail(op + " " + n.name + ": " + (scales.empty() ? "sizes" : "scales") + " must have one entry per axis");
    double sc[4] = {1, 1, 1, 1};
    int64_t out[4] = {X.dims[0], X.dims[1], X.dims[2], X.dims[3]};
    for (size_t k = 0; k < axes.size(); ++k) {
        const int a = int(axes[k]);
        if (scales.empty()) {
            if (sizes[k] <= 0) fail(op + " " + n.name + ": sizes must be positive");
            out[a] = sizes[k];
            sc[a] = double(sizes[k]) / double(X.dims[size_t(a)]);
        } else {
            if (!(scales[k] > 0)) fail(op + " " + n.name + ": scales must be positive");
            sc[a] = scales[k];
            out[a] = int64_t(std::floor(double(X.dims[size_t(a)]) * scales[k]));
            if (out[a] <= 0) fail(op + " " + n.name + ": the output would be empty");
        }
    }
    if (out[0] != X.dims[0] || out[1] != X.dims[1])
        fail(op + " " + n.name + ": only the spatial axes (2 and 3) may be resized; N and C must keep their size");
    n.kind = L_RESIZE;
    n.rs_sh = sc[2];
    n.rs_sw = sc[3];
    n.in = {x};
    odims = {out[0], out[1], out[2], out[3]};
}

// LayerNormalization-17 over the channel axis: the last axis of a channels-last view or of an [N, C] value.  (axis = 1 of an NCHW value would
// normalise over C*H*W: refused.)
void Planner::ImportLayerNorm(const OnnxNode& on, LNode& n, std::vector<int64_t>& odims) {
    const bool rms = on.op == "RMSNormalization";      // (opset 23, or the node MatchRmsNorm wrote for the spelled-out pattern)
    const std::string who = on.op + " " + n.name;
    if (!act_input(on, 0)) fail(who + ": constant input is not supported");
    const int x = in_val(on, 0);
    const Val& X = L.vals[x];
    const bool tok = L.is_tok(on.inputs[0]);
    const bool cl = L.is_cl(on.inputs[0]) || tok;
    const int64_t rank = tok ? 3 : int64_t(X.dims.size()), axis_attr = on.attr_i("axis", -1);
    const int64_t axis = axis_attr < 0 ? axis_attr + rank : axis_attr;
    if (!(cl ? axis == rank - 1 : (rank == 2 && axis == 1)))
        fail(who + ": axis = " + std::to_string(axis_attr) + " on " + (tok ? std::string("a token view") : cl ? std::string("a channels-last view") : "an NCHW value of rank " + std::to_string(rank)) +
             " is not supported (only the channel axis alone is normalised: the last axis of a channels-last view or of an [N, C] value)");
    if (on.attr_i("stash_type", 1) != 1) fail(who + ": stash_type = " + std::to_string(on.attr_i("stash_type", 1)) + " is not supported (1 is)");
    for (size_t k = 1; k < on.outputs.size(); ++k)
        if (!on.outputs[k].empty()) fail(who + ": the Mean / InvStdDev outputs are not supported");
    const OnnxTensor* g = on.inputs.size() > 1 ? L.init(on.inputs[1]) : nullptr;
    if (!g || g->dims.size() != 1 || g->numel() != X.c) fail(who + ": scale must be a [C] initializer");
    n.s = g->f;
    if (rms && on.inputs.size() > 2) fail(who + ": expected the inputs X and scale");
    n.rms = rms;
    if (on.inputs.size() > 2 && !on.inputs[2].empty()) {
        const OnnxTensor* b = L.init(on.inputs[2]);
        if (!b || b->dims.size() != 1 || b->numel() != X.c) fail(who + ": B must be a [C] initializer");
        n.t = b->f;
    }
    n.kind = L_LAYERNORM;
    n.eps = on.attr_f("epsilon", 1e-5f);
    n.in = {x};
    odims = X.dims;
    cl_out = cl && !tok;
    tok_out = tok;
}

// Transpose is a view of the NHWC storage, never a kernel: perm [0,2,3,1] of a 4-D value reads it channels-last, perm [0,3,1,2] of such a view
// reads it as NCHW again.  The output becomes one more name of the input's value (no node, no step).  true: the node is done
// Transpose(perm [1,0]) of a 2-D floating-point constant: a derived initializer (a tied vocabulary head reads the embedding table this way)
bool Planner::FoldConstTranspose(const OnnxNode& on) {
    if (on.op != "Transpose" || on.inputs.size() != 1) return false;
    const OnnxTensor* t = L.init(on.inputs[0]);
    const std::vector<int64_t> perm = on.attr_ints("perm", {1, 0});
    if (!t || t->dims.size() != 2 || t->f.empty() || perm != std::vector<int64_t>{1, 0}) return false;
    OnnxTensor o;
    o.dtype = t->dtype;
    o.name = on.outputs[0];
    const int64_t R = t->dims[0], C = t->dims[1];
    o.dims = {C, R};
    o.f.resize(t->f.size());
    for (int64_t r = 0; r < R; ++r)
        for (int64_t c = 0; c < C; ++c) o.f[size_t(c * R + r)] = t->f[size_t(r * C + c)];
    L.add_derived(std::move(o));
    return true;
}

// The two Reshapes of a matched Conv1D (MatchConv1D) rename their input's token value: [N, L, D] -> [N L, D] in front of the Gemm, [N L, Dout] ->
// [N, L, Dout] behind it.  false: the input is no token view or the shape is another one, and the node imports (or is refused) as before
bool Planner::ImportConv1DView(const OnnxNode& on, bool second) {
    if (!L.is_tok(on.inputs[0])) return false;
    const int v = in_val(on, 0);
    const Val& X = L.vals[v];
    const OnnxTensor* shp = on.inputs.size() > 1 ? L.init(on.inputs[1]) : nullptr;
    if (!shp) return false;
    std::vector<int64_t> d = shp->i;
    const std::vector<int64_t> idims = second ? std::vector<int64_t>{X.n * X.w, X.c} : std::vector<int64_t>{X.n, X.w, X.c};
    int64_t known = 1, neg = -1;
    for (size_t k = 0; k < d.size(); ++k) {
        if (d[k] == 0 && k < idims.size()) d[k] = idims[k];
        if (d[k] == -1) neg = int64_t(k); else known *= d[k];
    }
    if (neg >= 0 && known > 0) d[size_t(neg)] = X.n * X.w * X.c / known;
    if (d != (second ? std::vector<int64_t>{X.n, X.w, X.c} : std::vector<int64_t>{X.n * X.w, X.c})) return false;
    L.alias_name(on.outputs[0], v, false);
    L.tok_names.insert(on.outputs[0]);
    return true;
}

bool Planner::ImportTranspose(const OnnxNode& on, const LNode& n) {
    if (on.op != "Transpose") return false;
    if (!act_input(on, 0)) fail("Transpose " + n.name + ": constant input is not supported");
    const std::vector<int64_t> perm = on.attr_ints("perm", {});
    std::string ps = "[";
    for (size_t k = 0; k < perm.size(); ++k) ps += (k ? "," : "") + std::to_string(perm[k]);
    ps += "]";
    const int v = in_val(on, 0);
    // tokens: [N, C, H*W] (a flat name) -> [N, H*W, C] is the NHWC storage itself; the way back [N, L, D] -> [N, D, L] waits for its Reshape
    if (L.flat_names.count(on.inputs[0]) || L.is_tok(on.inputs[0]) || L.back_names.count(on.inputs[0])) {
        const bool flat = L.flat_names.count(on.inputs[0]) != 0, back = L.back_names.count(on.inputs[0]) != 0;
        if (perm != std::vector<int64_t>{0, 2, 1})
            fail("Transpose " + n.name + ": perm " + ps + " on " + (flat ? "the [N, C, H*W] reshape of a feature map" : back ? "the [N, D, L] transpose of a token view" : "a token view") + " is not supported (only [0,2,1] is)");
        const Val X = L.vals[v];
        // [N, L, D] -> [N, D, L] -> [N, L, D]: two transposes back to back cancel (torch writes group_norm(h.transpose(1, 2)).transpose(1, 2) unfolded)
        if (back) { L.alias_name(on.outputs[0], v, false); L.tok_names.insert(on.outputs[0]); }
        else if (!flat) { L.alias_name(on.outputs[0], v, false); L.back_names.insert(on.outputs[0]); }
        else if (X.h == 1) { L.alias_name(on.outputs[0], v, false); L.tok_names.insert(on.outputs[0]); }
        else {
            LNode a;
            a.kind = L_ALIAS;
            a.name = n.name;
            a.in = {v};
            push_node(std::move(a), on.outputs[0], {X.n, X.c, 1, X.h * X.w}, true);
        }
        return true;
    }
    const bool cl = L.is_cl(on.inputs[0]);
    const bool to_cl = perm == std::vector<int64_t>{0, 2, 3, 1}, from_cl = perm == std::vector<int64_t>{0, 3, 1, 2};
    if (L.vals[v].dims.size() != 4 || !((to_cl && !cl) || (from_cl && cl)))
        fail("Transpose " + n.name + ": perm " + ps + " on " + (cl ? "a channels-last view" : "an NCHW value of rank " + std::to_string(L.vals[v].dims.size())) +
             " is not supported (only [0,2,3,1] on a 4-D NCHW value and [0,3,1,2] on its channels-last view are)");
    L.alias_name(on.outputs[0], v, to_cl);
    return true;
}

// ---- one ONNX node -> one logical node with shape inference (or a derived initializer) ----
void Planner::ImportNode(const OnnxNode& on) {
    if (FoldConstantNode(on)) return;
    if (on.outputs.empty() || on.inputs.empty()) fail("node " + on.name + " (" + on.op + ") has no inputs/outputs");
    LNode n;
    n.name = on.name.empty() ? on.outputs[0] : on.name;
    const std::string& op = on.op;
    // the nodes of a matched window-attention region or patch merging: ranks 5 and 6 and the Slices never become values
    if (const auto va = view_alias.find(&on); va != view_alias.end()) {
        if (!L.is_cl(va->second)) fail(op + " " + n.name + ": the window region reads " + va->second + ", which is not a channels-last view [N, H, W, C]");
        L.alias_name(on.outputs[0], L.get_val(va->second), true);
        return;
    }
    if (wattn_skip.count(&on)) return;
    if (const auto wm = wattn_head.find(&on); wm != wattn_head.end()) { ImportWindowAttention(on, wm->second); return; }
    if (const auto mh = merge_head.find(&on); mh != merge_head.end()) { ImportPatchMerge(on, mh->second); return; }
    // a matched group norm: its last node imports the whole of it (ImportGroupNorm checks what its input may be: a flat name is one of them)
    if (gn_skip.count(&on)) return;
    if (const auto gh = gn_head.find(&on); gh != gn_head.end()) { ImportGroupNorm(on, gh->second); return; }
    // an RMSNorm spelled out: its last Mul imports the whole of it as the RMSNormalization node it is
    if (rms_skip.count(&on)) return;
    if (const auto rh = rms_head.find(&on); rh != rms_head.end()) { ImportNode(*rh->second); return; }
    // gelu_new spelled out: its last Mul imports the whole of it as the Gelu(approximate = "tanh") node it is
    if (gelu_skip.count(&on)) return;
    if (const auto gh = gelu_head.find(&on); gh != gelu_head.end()) {
        OnnxNode g;
        g.op = "Gelu";
        g.name = n.name;
        g.inputs = {gh->second};
        g.outputs = {on.outputs[0]};
        OnnxAttr ap;
        ap.name = "approximate";
        ap.s = "tanh";
        g.attrs["approximate"] = ap;
        synth_nodes.push_back(std::move(g));
        ImportNode(synth_nodes.back());
        return;
    }
    // a channels-last view may feed only the ops that read it as one: anything else (a Shape and the other folded ops included, hence before
    // the folds) would take its n / c / h / w for the ONNX dims
    static const std::set<std::string> cl_ops = {"LayerNormalization", "RMSNormalization", "MatMul", "Add", "Mul", "Div", "Erf", "Gelu", "Transpose"};
    for (const std::string& name : on.inputs)
        if (L.is_cl(name) && !cl_ops.count(op))
            fail(op + " " + n.name + ": input " + name + " is a channels-last view (a Transpose with perm [0,2,3,1]); only LayerNormalization, MatMul, Add, Mul, Div, Erf, "
                 "Gelu and Transpose may read one");
    // token views likewise, and the two half-way names of their creation and of the way back
    static const std::set<std::string> tok_ops = {"LayerNormalization", "RMSNormalization", "MatMul", "Add", "Mul", "Div", "Erf", "Gelu", "Transpose", "Concat", "Gather", "Reshape"};
    for (const std::string& name : on.inputs) {
        // (a Conv1D's Gemm reads its token view like a MatMul; the Split of a GPT-2 attention is its head; a Pow is no operator of the planner at all, whatever it reads;
        // a Sigmoid on tokens is the SiLU of a Llama MLP's gate)
        if (L.is_tok(name) && !tok_ops.count(op) && !(op == "Gemm" && conv1d_gemm.count(&on)) && !attn_head.count(&on) && op != "Pow" && op != "Sigmoid")
            fail(op + " " + n.name + ": input " + name + " is a token view [N, L, D]; only LayerNormalization, MatMul, Add, Mul, Div, Erf, Gelu, Transpose, Concat, "
                 "Gather and the Reshape of the attention pattern may read one");
        if (L.flat_names.count(name) && op != "Transpose")
            fail(op + " " + n.name + ": input " + name + " is the [N, C, H*W] reshape of a feature map; only a Transpose with perm [0,2,1] (to tokens [N, L, D]) may read it");
        if (L.back_names.count(name) && op != "Reshape" && op != "Transpose")
            fail(op + " " + n.name + ": input " + name + " is the [N, D, L] transpose of a token view; only a Reshape to [N, D, h, w] with h * w = L may read it");
    }
    if (embed_skip.count(&on)) return;                     // inside a matched embedding sum: the LayerNormalization behind it imports the whole of it
    if (const auto eh = embed_head.find(&on); eh != embed_head.end()) { ImportEmbed(on, eh->second); return; }
    if (attn_skip.count(&on)) return;                      // inside a matched attention subgraph: its head node imports the whole of it
    if (const auto am = attn_head.find(&on); am != attn_head.end()) { ImportAttention(on, am->second); return; }
    if (const auto cv = conv1d_view.find(&on); cv != conv1d_view.end() && ImportConv1DView(on, cv->second)) return;
    if (FoldShapeArithmetic(on, n) || FoldShapeOnlyOp(on, n) || FoldExpand(on, n) || FoldConstTranspose(on) || ImportTranspose(on, n) || ImportTokenView(on, n)) return;
    std::vector<int64_t> odims;
    cl_out = tok_out = false;
    if (op == "Conv") ImportConv(on, n, odims);
    else if (op == "ConvTranspose") ImportConvTranspose(on, n, odims);
    else if (op == "MatMul" || op == "Gemm") ImportGemm(on, n, odims);
    else if (op == "BatchNormalization") ImportBatchNorm(on, n, odims);
    else if (op == "LayerNormalization" || op == "RMSNormalization") ImportLayerNorm(on, n, odims);
    else if (op == "Clip" || op == "Sigmoid" || op == "HardSigmoid" || op == "HardSwish" || op == "Relu" || op == "Erf" || op == "Gelu" || op == "Tanh") ImportActivation(on, n, odims);
    else if (op == "Add" || op == "Mul" || op == "Div") ImportArithmetic(on, n, odims);
    else if (op == "Concat") ImportConcat(on, n, odims);
    else if (op == "MaxPool" || op == "AveragePool" || op == "GlobalAveragePool") ImportPool(on, n, odims);
    else if (op == "Unsqueeze" || op == "Flatten" || op == "Reshape" || op == "Identity" || op == "Dropout" || op == "Squeeze") ImportReshape(on, n, odims);
    else if (op == "Resize" || op == "Upsample") ImportResize(on, n, odims);
    else fail("Unsupported ONNX operator: " + op + " (node " + n.name + ")");
    n.out = L.new_val(on.outputs[0], odims);
    if (cl_out) L.cl_names.insert(on.outputs[0]);
    if (tok_out) L.tok_names.insert(on.outputs[0]);
    L.vals[n.out].producer = int(L.nodes.size());
    L.nodes.push_back(std::move(n));
}

void Planner::push_node(LNode&& n, const std::string& out_name, const std::vector<int64_t>& odims, bool tok) {
    n.out = L.new_val(out_name, odims);
    if (tok) L.tok_names.insert(out_name);
    L.vals[n.out].producer = int(L.nodes.size());
    L.nodes.push_back(std::move(n));
}

// Expand of a constant to a constant shape (the class token [1, 1, D] to [N, 1, D]): a derived initializer.  true: the node is done
bool Planner::FoldExpand(const OnnxNode& on, const LNode& n) {
    if (on.op != "Expand" || on.inputs.size() < 2 || !L.init(on.inputs[0]) || !L.init(on.inputs[1])) return false;
    OnnxTensor t = *L.init(on.inputs[0]);
    const std::vector<int64_t> shp = L.init(on.inputs[1])->i;
    if (t.f.empty() || shp.empty()) fail("Expand " + n.name + ": only a floating-point constant and an integer shape are supported");
    std::vector<int64_t> id = t.dims, od = shp;
    while (id.size() < od.size()) id.insert(id.begin(), 1);
    while (od.size() < id.size()) od.insert(od.begin(), 1);
    int64_t total = 1;
    for (size_t k = 0; k < od.size(); ++k) {
        if (od[k] == 1) od[k] = id[k];
        if (id[k] != 1 && id[k] != od[k]) fail("Expand " + n.name + ": the shape does not broadcast");
        if (od[k] <= 0) fail("Expand " + n.name + ": non-positive dimension");
        total *= od[k];
    }
    if (total > (int64_t(1) << 26)) fail("Expand " + n.name + ": the result is too large to fold");
    std::vector<float> f(static_cast<size_t>(total));
    for (int64_t o = 0; o < total; ++o) {
        int64_t rem = o, src = 0, stride = 1;
        for (size_t k = od.size(); k-- > 0;) {
            const int64_t ix = rem % od[k];
            rem /= od[k];
            if (id[k] != 1) { src += ix * stride; }
            stride *= id[k];
        }
        f[size_t(o)] = t.f[size_t(src)];
    }
    t.f = std::move(f);
    t.dims = od;
    t.name = on.outputs[0];
    L.add_derived(std::move(t));
    return true;
}

// The token constructs that emit no node of their own kind.  true: the node is done
//   Reshape [N, C, H, W] -> [N, C, H*W]: a flat name (one more name of the value; its Transpose [0,2,1] makes the tokens)
//   Reshape of a back name (the Transpose [0,2,1] of tokens [N, L, D]) to [N, D, h, w], h * w = L: a plain NCHW value on the same storage
//   Gather(axis 1, scalar index i) of tokens: the [N, D] view of row i of every image (pitch L * pitch, offset i * pitch): no step
bool Planner::ImportTokenView(const OnnxNode& on, LNode& n) {
    const std::string& op = on.op;
    if (op == "Reshape" && act_input(on, 0)) {
        const int v = in_val(on, 0);
        const Val X = L.vals[v];
        const bool back = L.back_names.count(on.inputs[0]) != 0, tok = L.is_tok(on.inputs[0]);
        if (!back && !tok && !(X.dims.size() == 4 && X.h * X.w != 1 && !L.is_cl(on.inputs[0]))) return false;
        const OnnxTensor* shp = on.inputs.size() > 1 ? L.init(on.inputs[1]) : nullptr;
        if (!shp && !back && !tok) return false;
        if (!shp) fail("Reshape " + n.name + ": shape must be an initializer");
        std::vector<int64_t> d = shp->i;
        // the ONNX dims of the input: [N, L, D] of a token name, [N, D, L] of a back name, else the value's own
        const std::vector<int64_t> idims = tok ? std::vector<int64_t>{X.n, X.w, X.c} : back ? std::vector<int64_t>{X.n, X.c, X.w} : X.dims;
        int64_t known = 1, neg = -1, total = 1;
        for (int64_t x : idims) total *= x;
        for (size_t k = 0; k < d.size(); ++k) {
            if (d[k] == 0 && k < idims.size()) d[k] = idims[k];
            if (d[k] == -1) neg = int64_t(k); else known *= d[k];
        }
        if (neg >= 0 && known > 0) d[size_t(neg)] = total / known;
        if (tok) {
            // only as the head of the attention pattern, which MatchAttention took: a left-over one is an unsupported operator
            if (d.size() == 5) fail("Unsupported ONNX operator: Reshape (node " + n.name + ")");
            fail("Reshape " + n.name + ": input " + on.inputs[0] + " is a token view [N, L, D]; only the [N, L, 3, H, hd] Reshape of the attention pattern may reshape one");
        }
        if (back) {
            if (d.size() != 4 || d[0] != X.n || d[1] != X.c || d[2] * d[3] != X.w || d[2] <= 0)
                fail("Reshape " + n.name + ": the [N, D, L] transpose of a token view only reshapes to [N, D, h, w] with h * w = L");
            if (d[2] == 1) { L.alias_name(on.outputs[0], v, false); return true; }
            n.kind = L_ALIAS;
            n.in = {v};
            push_node(std::move(n), on.outputs[0], d, false);
            return true;
        }
        if (d.size() != 3 || d[0] != X.n || d[1] != X.c || d[2] != X.h * X.w) return false;       // (ImportReshape refuses it as before)
        L.alias_name(on.outputs[0], v, false);
        L.flat_names.insert(on.outputs[0]);
        return true;
    }
    if (op == "Gather" && L.is_tok(on.inputs[0])) {
        const int v = in_val(on, 0);
        const Val X = L.vals[v];
        const OnnxTensor* ix = on.inputs.size() > 1 ? L.init(on.inputs[1]) : nullptr;
        int64_t axis = on.attr_i("axis", 0);
        if (axis < 0) axis += 3;
        if (axis != 1 || !ix || !ix->dims.empty() || ix->i.size() != 1)
            fail("Gather " + n.name + ": only Gather(axis = 1, scalar constant index) selects a token of the token view " + on.inputs[0]);
        int64_t i = ix->i[0];
        if (i < 0) i += X.w;
        if (i < 0 || i >= X.w) fail("Gather " + n.name + ": index out of range");
        const int o = L.new_val(on.outputs[0], {X.n, X.c});
        L.vals[o].parent = v;
        L.vals[o].parent_off = 0;
        L.vals[o].sel_rows = X.w;
        L.vals[o].sel_idx = i;
        return true;
    }
    return false;
}

// Concat(axis 1) of a class-token constant [1 | N, 1, D] and a token value [N, L0, D]: the token-assemble node.  Every other token-axis concat is refused
void Planner::ImportTokenConcat(const OnnxNode& on, LNode& n, std::vector<int64_t>& odims) {
    int64_t axis = on.attr_i("axis", 1);
    if (axis < 0) axis += 3;
    if (axis != 1) fail("Concat " + n.name + ": only axis = 1 (the token axis) is supported on token views");
    if (on.inputs.size() != 2)
        fail("Concat " + n.name + ": a token-axis concat takes exactly two operands, a class-token constant and the tokens (it has " + std::to_string(on.inputs.size()) + ")");
    if (act_input(on, 0) && act_input(on, 1))
        fail("Concat " + n.name + ": concatenating two activations along the token axis is not supported (only a class-token constant in front of the tokens)");
    if (!L.is_tok(on.inputs[1]))
        fail("Concat " + n.name + ": a constant behind the tokens is not supported (only a class-token constant in front of the tokens)");
    const OnnxTensor* c = L.init(on.inputs[0]);
    const int x = in_val(on, 1);
    const Val& X = L.vals[x];
    if (!c || c->f.empty() || c->dims.size() != 3 || (c->dims[0] != 1 && c->dims[0] != X.n) || c->dims[1] != 1 || c->dims[2] != X.c)
        fail("Concat " + n.name + ": the class token must be a floating-point constant of shape [1 | N, 1, D]");
    for (int64_t r = 1; r < c->dims[0]; ++r)
        for (int64_t k = 0; k < X.c; ++k)
            if (c->f[size_t(r * X.c + k)] != c->f[size_t(k)]) fail("Concat " + n.name + ": the class token must be the same for every image");
    n.kind = L_TOKASM;
    n.s.assign(c->f.begin(), c->f.begin() + X.c);
    n.in = {x};
    odims = {X.n, X.c, 1, X.w + 1};
    tok_out = true;
}

// ---- attention: the unfused multi-head attention subgraph of a ViT export as ONE node ------------------------------------------------
// Matched on the ONNX nodes, before the import (its inner values have ranks 4 and 5, which no Val holds), around every Softmax that sits between
// two MatMuls of activations:
//   R = Reshape(qkv, [N, L, 3, H, hd]) -> T = Transpose(R, [2,0,3,1,4]) -> q, k, v = Gather(T, axis 0, index 0 / 1 / 2) | Squeeze(Split(T, axis 0)[i], [0])
//   S = MatMul(q [* c], Transpose(k, [0,1,3,2]) [* c]) [* c | / c] -> P = Softmax(S, axis -1) -> MatMul(P, v) -> Transpose [0,2,1,3] -> Reshape [N, L, D]
// with scalar constants c in either operand order, every intermediate read by the next node only.  A near miss is refused naming what did not
// match; nothing is approximated.  A Softmax elsewhere is left to the import, which refuses it as an unsupported operator.
void Planner::IndexGraph() {
    if (gi.m) return;
    gi.m = &m;
    for (const OnnxNode& on : m.nodes) {
        for (const std::string& o : on.outputs) if (!o.empty()) gi.prod[o] = &on;
        for (const std::string& i : on.inputs) if (!i.empty()) ++gi.readers[i];
        if (on.op == "Constant" && on.outputs.size() == 1 && on.attrs.size() == 1) {
            const OnnxAttr& at = on.attrs.begin()->second;
            OnnxTensor t;
            if (at.name == "value" && at.has_t) t = at.t;
            else if (at.name == "value_float") { t.dtype = ONNX_FLOAT; t.f = {at.f}; }
            else if (at.name == "value_int") { t.dtype = ONNX_INT64; t.i = {at.i}; }
            else continue;
            gi.consts[on.outputs[0]] = t;
        }
    }
    for (const auto& vo : m.outputs) ++gi.readers[vo.name];
}

void Planner::MatchAttention() {
    IndexGraph();
    for (const OnnxNode& sm : m.nodes) {
        if (sm.op != "Softmax" || sm.inputs.size() != 1 || sm.outputs.size() != 1 || wattn_softmax.count(&sm)) continue;
        const std::string nm = sm.name.empty() ? sm.outputs[0] : sm.name;
        const std::string prefix = "Softmax " + nm + ": the attention pattern around it does not match: ";
        // is this an attention at all?  scores from a MatMul of two activations (through scalings, or behind a mask Add), probabilities into a MatMul
        const OnnxNode* pv = nullptr;
        for (const OnnxNode& on : m.nodes)
            if (on.op == "MatMul" && on.inputs.size() == 2 && on.inputs[0] == sm.outputs[0] && !gi.cst(on.inputs[1])) pv = &on;
        if (!pv) continue;
        AttnMatch am;
        std::vector<const OnnxNode*> causal_nodes;
        // a causal mask as Where(cond, scores, c), directly in front of the Softmax or of the key-mask Add (GPT-2 writes the Where first)
        auto causal_where = [&](const std::string& name) -> const OnnxNode* {
            const OnnxNode* p = gi.producer(name);
            return p && p->op == "Where" && p->inputs.size() == 3 && gi.act_matmul(gi.producer(gi.peel_quiet(p->inputs[1]))) ? p : nullptr;
        };
        // the scaled product of two activations, also behind a causal Where
        auto is_scores = [&](const std::string& name) {
            const std::string cur = gi.peel_quiet(name);
            return gi.act_matmul(gi.producer(cur)) || causal_where(cur) != nullptr;
        };
        const std::string both = "a causal mask together with a key mask (attention_mask) on the scores is not supported";
        std::string sm_in = sm.inputs[0];          // the name the scores reach the Softmax (or the causal Where in front of it) under
        if (const OnnxNode* wh = causal_where(sm_in)) {
            MatchCausalWhere(*wh, prefix, am, causal_nodes);
            sm_in = wh->inputs[1];
        }
        const OnnxNode* top = gi.producer(gi.peel_quiet(sm_in));
        std::string scores = sm_in;
        const OnnxNode* mask_add = nullptr;
        if (top && top->op == "Add" && top->inputs.size() == 2 && (is_scores(top->inputs[0]) || is_scores(top->inputs[1]))) {
            const int si = is_scores(top->inputs[0]) ? 0 : 1;
            const std::string tname = top->name.empty() ? top->outputs[0] : top->name;
            const OnnxTensor* mk = gi.cst(top->inputs[size_t(1 - si)]);
            if (top->outputs[0] == sm_in && !am.causal && mk && MatchCausalAdd(*mk, am)) {
                // the causal mask as an additive constant: 0 on and below the diagonal, one value <= -1e30 above it
                causal_nodes.push_back(top);
            } else if (const ChunkMask* cm = top->outputs[0] == sm_in ? MatchChunkMask(top->inputs[size_t(1 - si)], prefix + "Add " + tname + ": ") : nullptr) {
                // the 4-D mask of an extend step: the key mask and the chunk's causal constant in one value; P and Lq are known at the import
                if (am.causal) fail(prefix + both + " (Add " + tname + ")");
                am.mask = key_masks.at(cm->ext).input;
                am.mask_value = cm->fill;
                am.chunk = true;
                am.chunk_c = cm->c;
                am.chunk_where = top->inputs[size_t(1 - si)];
                ++chunk_masks[top->inputs[size_t(1 - si)]].uses;
                mask_add = top;
            } else {
                // only the key mask of an INT64 graph input [N, L], broadcast as [N, 1, 1, L], directly in front of the Softmax
                const KeyMask* km = top->outputs[0] == sm_in ? &MatchKeyMask(top->inputs[size_t(1 - si)]) : nullptr;
                if (km && km->ok && am.causal) fail(prefix + both + " (Add " + tname + ")");
                if (!km || !km->ok) fail(prefix + "an additive mask (Add " + tname + ") on the scores is not supported");
                am.mask = km->input;
                am.mask_value = km->c;
                ++key_masks[top->inputs[size_t(1 - si)]].uses;
                mask_add = top;
            }
            scores = top->inputs[size_t(si)];
            // one mask only: whatever masks the scores below this Add makes two
            if (causal_where(gi.peel_quiet(scores))) fail(prefix + both + " (Where " + causal_where(gi.peel_quiet(scores))->outputs[0] + " below Add " + tname + ")");
            top = gi.producer(gi.peel_quiet(scores));
            if (top && top->op == "Add" && top->inputs.size() == 2 && (is_scores(top->inputs[0]) || is_scores(top->inputs[1]))) {
                bool two = am.causal;
                AttnMatch probe;
                for (const std::string& o : top->inputs) if (const OnnxTensor* c2 = gi.cst(o); c2 && MatchCausalAdd(*c2, probe)) two = true;
                if (two) fail(prefix + both + " (Add " + (top->name.empty() ? top->outputs[0] : top->name) + " below Add " + tname + ")");
            }
        }
        if (!gi.act_matmul(top)) continue;
        for (const OnnxNode* p : causal_nodes) {
            if (p->op != "Slice" && gi.nreaders(p->outputs[0]) != 1) fail(prefix + "the masked scores " + p->outputs[0] + " have " + std::to_string(gi.nreaders(p->outputs[0])) + " readers, not 1");
            attn_skip.insert(p);
        }
        if (mask_add && gi.nreaders(mask_add->outputs[0]) != 1) fail(prefix + "the scores " + mask_add->outputs[0] + " have " + std::to_string(gi.nreaders(mask_add->outputs[0])) + " readers, not 1");
        if (mask_add) attn_skip.insert(mask_add);
        {
            const OnnxNode* head = nullptr;
            std::vector<const OnnxNode*> taken;
            if (MatchSplitAttention(sm, pv, scores, prefix, am, head, taken)) {
                am.name += "+" + nm;
                attn_head[head] = am;
                for (const OnnxNode* p : taken) if (p != head) attn_skip.insert(p);
                continue;
            }
        }
        const AttnCore c = MatchAttentionCore(sm, pv, scores, prefix);
        am.heads = c.shape5[3];
        am.head_dim = c.shape5[4];
        am.scale = c.scale;
        am.out = c.orr->outputs[0];
        am.shape5 = c.shape5;
        am.shape3 = c.shape3;
        am.name = (c.rs->name.empty() ? c.rs->outputs[0] : c.rs->name) + "+" + nm + "+" + (c.orr->name.empty() ? c.orr->outputs[0] : c.orr->name);
        attn_head[c.rs] = am;
        for (const OnnxNode* p : c.taken) attn_skip.insert(p);
        attn_skip.insert(c.orr);
    }
    // the nodes that cut the rope tables out of constants were evaluated at load: they import nothing, and only rotary products may read them
    for (const OnnxNode* p : rope_const_nodes) {
        for (const OnnxNode* r : gi.readers_of(p->outputs[0]))
            if (!attn_skip.count(r) && !rope_const_nodes.count(r))
                fail(p->op + " " + (p->name.empty() ? p->outputs[0] : p->name) + ": the rope table " + p->outputs[0] + " is read by " + r->op + " " + (r->name.empty() ? r->outputs[0] : r->name) +
                     "; only the products of a rotary embedding may read it");
    }
    for (const OnnxNode* p : rope_const_nodes) attn_skip.insert(p);
    // a chunk mask M is the matched attentions' alone; its Where and Cast import nothing (its ext chain: below, the Cast being the chain's one reader)
    for (const auto& kv : chunk_masks)
        if (kv.second.ok && kv.second.uses > 0) {
            if (gi.nreaders(kv.first) != kv.second.uses)
                fail("Where " + kv.first + ": the chunk mask has " + std::to_string(gi.nreaders(kv.first)) + " readers, " + std::to_string(kv.second.uses) + " of them attention scores; only those may read it");
            for (const OnnxNode* p : kv.second.nodes) { attn_skip.insert(p); mask_nodes.insert(p); }
            key_masks[kv.second.ext].uses = 1;
        }
    // an ext chain is the matched attentions' alone
    for (const auto& kv : key_masks)
        if (kv.second.ok && kv.second.uses > 0) {
            if (gi.nreaders(kv.first) != kv.second.uses)
                fail("Mul " + kv.first + ": the key mask has " + std::to_string(gi.nreaders(kv.first)) + " readers, " + std::to_string(kv.second.uses) + " of them attention scores; only those may read it");
            for (const OnnxNode* p : kv.second.nodes) { attn_skip.insert(p); mask_nodes.insert(p); }
        }
}

// ext = Mul(Sub(1.0, Cast(Unsqueeze(Unsqueeze(mask, [1]), [2]) | Unsqueeze(mask, [1, 2]), FLOAT)), c), mask an INT64 graph input [N, L]: ok, else not a key mask
const Planner::KeyMask& Planner::MatchKeyMask(const std::string& name) {
    if (const auto it = key_masks.find(name); it != key_masks.end()) return it->second;
    KeyMask& km = key_masks[name];
    auto scalar = [&](const std::string& n, float& v) {
        const OnnxTensor* t = gi.cst(n);
        if (!t || t->numel() != 1 || t->f.size() != 1) return false;
        v = t->f[0];
        return true;
    };
    const OnnxNode* mul = gi.producer(name);
    if (!mul || mul->op != "Mul" || mul->inputs.size() != 2) return km;
    float c = 0.f, one = 0.f;
    const int ci = scalar(mul->inputs[0], c) ? 0 : (scalar(mul->inputs[1], c) ? 1 : -1);
    if (ci < 0) return km;
    const OnnxNode* sb = gi.producer(mul->inputs[size_t(1 - ci)]);
    if (!sb || sb->op != "Sub" || sb->inputs.size() != 2 || !scalar(sb->inputs[0], one) || one != 1.f || gi.nreaders(sb->outputs[0]) != 1) return km;
    const OnnxNode* cast = gi.producer(sb->inputs[1]);
    if (!cast || cast->op != "Cast" || cast->attr_i("to", 0) != ONNX_FLOAT || gi.nreaders(cast->outputs[0]) != 1) return km;
    std::vector<int64_t> axes;
    std::vector<const OnnxNode*> nodes = {mul, sb, cast};
    std::string cur = cast->inputs[0];
    for (int k = 0; k < 2; ++k) {
        const OnnxNode* u = gi.producer(cur);
        if (!u) break;
        if (u->op != "Unsqueeze" || gi.nreaders(cur) != 1) return km;
        std::vector<int64_t> ax = u->attr_ints("axes", {});
        if (ax.empty() && u->inputs.size() > 1) if (const OnnxTensor* t = gi.cst(u->inputs[1])) ax = t->i;
        axes.insert(axes.begin(), ax.begin(), ax.end());
        nodes.push_back(u);
        cur = u->inputs[0];
    }
    // [N, L] -> [N, 1, 1, L]: axes [1] then [2], or [1, 2] at once
    if (axes != std::vector<int64_t>{1, 2}) return km;
    bool is_input = false;
    for (const auto& vi : m.inputs) if (vi.name == cur && vi.elem_type == ONNX_INT64 && vi.dims.size() == 2) is_input = true;
    if (!is_input) return km;
    km.ok = true;
    km.input = cur;
    km.c = c;
    km.nodes = nodes;
    return km;
}

// M = Where(Cast(ext, to BOOL), c, C): ext a key-mask chain (non-zero on a masked key), c a scalar constant <= -1e30, C a float constant of rank 4.
// nullptr: `name` is no such value (the caller's own refusal follows).  Add(ext, C), which sums two finfo.min to -inf, and a near miss of the Where
// form are refused by name.  C's elements are checked at the import (ImportAttention), where the step's P and Lq are known
const Planner::ChunkMask* Planner::MatchChunkMask(const std::string& name, const std::string& prefix) {
    if (const auto it = chunk_masks.find(name); it != chunk_masks.end()) return it->second.ok ? &it->second : nullptr;
    const OnnxNode* wh = gi.producer(name);
    auto rank4 = [&](const std::string& n) { const OnnxTensor* t = gi.cst(n); return t && !t->f.empty() && t->dims.size() == 4 ? t : nullptr; };
    const std::string form = "; supported: Where(Cast(ext, to BOOL), finfo.min, C) with C [1, 1, Lq, P + Lq], as AttentionMaskConverter.to_4d lowers it with a past";
    if (wh && wh->op == "Add" && wh->inputs.size() == 2)
        for (int k = 0; k < 2; ++k)
            if (rank4(wh->inputs[size_t(k)]) && gi.producer(wh->inputs[size_t(1 - k)]) && MatchKeyMask(wh->inputs[size_t(1 - k)]).ok)
                fail(prefix + "the mask " + name + " is Add(ext, C) of a key mask and a constant: a masked key of the chunk's future would be finfo.min + finfo.min = -inf" + form);
    if (!wh || wh->op != "Where" || wh->inputs.size() != 3) return nullptr;
    const OnnxNode* cast = gi.producer(wh->inputs[0]);
    if (!cast || cast->op != "Cast" || cast->inputs.size() != 1 || !gi.producer(cast->inputs[0]) || !MatchKeyMask(cast->inputs[0]).ok) return nullptr;
    const KeyMask& km = MatchKeyMask(cast->inputs[0]);
    const std::string who = prefix + "the chunk mask Where " + (wh->name.empty() ? wh->outputs[0] : wh->name) + ": ";
    if (cast->attr_i("to", 0) != ONNX_BOOL) fail(who + "its condition is not Cast(ext, to BOOL)" + form);
    if (km.c == 0.f) fail(who + "the key mask's constant is 0: Cast(ext, to BOOL) is false on every key" + form);
    if (gi.nreaders(cast->outputs[0]) != 1 || gi.nreaders(cast->inputs[0]) != 1) fail(who + "its condition or the key mask " + cast->inputs[0] + " has a second reader" + form);
    const OnnxTensor* c = gi.cst(wh->inputs[1]);
    if (!c || c->numel() != 1 || c->f.size() != 1) fail(who + "the value " + wh->inputs[1] + " of a masked key is not a scalar floating-point constant" + form);
    if (!(c->f[0] <= -1e30f)) fail(who + "the value " + std::to_string(c->f[0]) + " of a masked key is above -1e30: a masked key of the chunk's future would keep a probability" + form);
    const OnnxTensor* C = rank4(wh->inputs[2]);
    if (!C) fail(who + "its third operand " + wh->inputs[2] + " is not a floating-point constant of rank 4" + form);
    ChunkMask& cm = chunk_masks[name];
    cm.ok = true;
    cm.ext = cast->inputs[0];
    cm.c = C;
    cm.fill = c->f[0];
    cm.nodes = {wh, cast};
    return &cm;
}

// Where(cond, scores, c) on the scores: cond a BOOL constant [1, 1, L, L], or one or two Slices with constant indices of a [1, 1, P, P] one (GPT-2's
// `bias` buffer), exactly j <= i after slicing; c a scalar constant <= -1e30.  At such a value exp(c - max) is exactly 0 in fp32 and in float64 for
// every score an fp32 graph can produce: leaving the masked keys out approximates nothing.  Anything else is refused naming the Where and the rule
void Planner::MatchCausalWhere(const OnnxNode& wh, const std::string& prefix, AttnMatch& am, std::vector<const OnnxNode*>& taken) {
    const std::string nm = wh.name.empty() ? wh.outputs[0] : wh.name;
    auto miss = [&](const std::string& what) { fail(prefix + "Where " + nm + ": " + what); };
    std::vector<const OnnxNode*> slices;
    std::string cur = wh.inputs[0];
    for (const OnnxNode* p = gi.producer(cur); p && p->op == "Slice" && !p->inputs.empty() && slices.size() < 2; p = gi.producer(cur)) {
        slices.push_back(p);
        cur = p->inputs[0];
    }
    const OnnxTensor* base = gi.cst(cur);
    if (!base || base->dtype != ONNX_BOOL || base->dims.size() != 4 || base->dims[0] != 1 || base->dims[1] != 1 || base->dims[2] != base->dims[3])
        miss("its condition " + wh.inputs[0] + " is not a BOOL constant [1, 1, L, L], nor one or two constant Slices of a [1, 1, P, P] one");
    std::vector<int64_t> dims = base->dims, v = base->i;
    for (size_t k = slices.size(); k-- > 0;) {
        const OnnxNode* sl = slices[k];
        const std::string snm = sl->name.empty() ? sl->outputs[0] : sl->name;
        auto ints = [&](size_t i, std::vector<int64_t>& out) {
            if (i >= sl->inputs.size() || sl->inputs[i].empty()) return false;
            const OnnxTensor* t = gi.cst(sl->inputs[i]);
            if (!t || t->i.empty()) miss("the indices of Slice " + snm + " in front of its condition are not constants");
            out = t->i;
            return true;
        };
        std::vector<int64_t> st, en, ax, stp;
        if (!ints(1, st) || !ints(2, en) || st.size() != en.size()) miss("the indices of Slice " + snm + " in front of its condition are not constants");
        if (!ints(3, ax)) for (size_t a = 0; a < st.size(); ++a) ax.push_back(int64_t(a));
        if (!ints(4, stp)) stp.assign(st.size(), 1);
        if (ax.size() != st.size() || stp.size() != st.size()) miss("Slice " + snm + ": starts, ends, axes and steps differ in length");
        for (size_t a = 0; a < ax.size(); ++a) {
            const int64_t axis = ax[a] < 0 ? ax[a] + 4 : ax[a];
            if (axis < 0 || axis > 3 || stp[a] != 1) miss("Slice " + snm + ": only step 1 along the axes of the [1, 1, P, P] condition is supported");
            const int64_t P = dims[size_t(axis)];
            const int64_t b = std::clamp<int64_t>(st[a] < 0 ? st[a] + P : st[a], 0, P), e = std::clamp<int64_t>(en[a] < 0 ? en[a] + P : en[a], b, P);
            int64_t outer = 1, inner = 1;
            for (int64_t d = 0; d < axis; ++d) outer *= dims[size_t(d)];
            for (int64_t d = axis + 1; d < 4; ++d) inner *= dims[size_t(d)];
            std::vector<int64_t> w;
            w.reserve(size_t(outer * (e - b) * inner));
            for (int64_t o = 0; o < outer; ++o) w.insert(w.end(), v.begin() + (o * P + b) * inner, v.begin() + (o * P + e) * inner);
            v = std::move(w);
            dims[size_t(axis)] = e - b;
        }
        taken.push_back(sl);
    }
    if (dims[0] != 1 || dims[1] != 1 || dims[2] != dims[3] || dims[2] < 1) miss("its condition is [" + std::to_string(dims[0]) + ", " + std::to_string(dims[1]) + ", " + std::to_string(dims[2]) + ", " + std::to_string(dims[3]) + "] after slicing, not [1, 1, L, L]");
    const int64_t Lq = dims[2];
    for (int64_t i = 0; i < Lq; ++i)
        for (int64_t j = 0; j < Lq; ++j)
            if ((v[size_t(i * Lq + j)] != 0) != (j <= i))
                miss("its condition is not the causal mask j <= i: element [" + std::to_string(i) + ", " + std::to_string(j) + "] is " + (v[size_t(i * Lq + j)] ? "true" : "false"));
    const OnnxTensor* c = gi.cst(wh.inputs[2]);
    if (!c || c->numel() != 1 || c->f.size() != 1) miss("the value " + wh.inputs[2] + " of the masked scores is not a scalar floating-point constant");
    if (!(c->f[0] <= -1e30f)) miss("the value " + std::to_string(c->f[0]) + " of the masked scores is above -1e30: the masked keys keep a probability, and the kernels leave them out");
    am.causal = true;
    am.causal_len = Lq;
    taken.push_back(&wh);
}

// Add(scores, M): M a floating-point constant [1, 1, L, L], 0 where j <= i and ONE value, -inf or <= -1e30, above the diagonal (HF's additive masks
// hold finfo.min): s + M is M there for every score an fp32 graph can produce, the masked keys' probabilities are exactly 0.  false: not such a mask
bool Planner::MatchCausalAdd(const OnnxTensor& mk, AttnMatch& am) const {
    if (mk.f.empty() || mk.dims.size() != 4 || mk.dims[0] != 1 || mk.dims[1] != 1 || mk.dims[2] != mk.dims[3] || mk.dims[2] < 1) return false;
    const int64_t Lq = mk.dims[2];
    const float fill = Lq > 1 ? mk.f[1] : 0.f;
    if (Lq > 1 && !(fill <= -1e30f)) return false;
    for (int64_t i = 0; i < Lq; ++i)
        for (int64_t j = 0; j < Lq; ++j)
            if (mk.f[size_t(i * Lq + j)] != (j <= i ? 0.f : fill)) return false;
    am.causal = true;
    am.causal_len = Lq;
    return true;
}

// HF's Conv1D on a token value: Reshape(t, [-1, D] | [N L, D]) -> Gemm(., W [D, Dout], b; alpha = beta = 1, no transposes) -> Reshape(., [N, L, Dout]).
// Matched on the structure and the reader counts; the shapes are checked at the import, where t's are known (ImportConv1DView).  The Gemm is then the
// 1x1 conv a MatMul + Add on the token value gives, and the two Reshapes cost nothing.  Any other Reshape of a token value keeps its refusal
void Planner::MatchConv1D() {
    bool any = false;
    for (const OnnxNode& on : m.nodes) any = any || on.op == "Gemm";
    if (!any) return;
    IndexGraph();
    for (const OnnxNode& g : m.nodes) {
        if (g.op != "Gemm" || g.inputs.size() < 2 || g.outputs.size() != 1 || gi.cst(g.inputs[0]) || !gi.cst(g.inputs[1])) continue;
        if (g.attr_i("transA", 0) != 0 || g.attr_i("transB", 0) != 0 || g.attr_f("alpha", 1.f) != 1.f || g.attr_f("beta", 1.f) != 1.f) continue;
        const OnnxNode* r1 = gi.producer(g.inputs[0]);
        const OnnxNode* r2 = gi.only_reader(g.outputs[0]);
        auto shape_rank = [&](const OnnxNode* r) -> size_t {
            const OnnxTensor* t = r && r->op == "Reshape" && r->inputs.size() == 2 ? gi.cst(r->inputs[1]) : nullptr;
            return t ? t->i.size() : 0;
        };
        if (shape_rank(r1) != 2 || shape_rank(r2) != 3 || r2->inputs[0] != g.outputs[0] || gi.nreaders(r1->outputs[0]) != 1 || gi.cst(r1->inputs[0])) continue;
        conv1d_view[r1] = false;
        conv1d_view[r2] = true;
        conv1d_gemm.insert(&g);
    }
}

// gelu_new as torch spells it: 0.5 * x * (1 + Tanh(sqrt(2 / pi) * (x + 0.044715 * Pow(x, 3)))), every operand order, Mul(x, Mul(x, x)) in place of the
// Pow, the constants to 1e-6 relative (as the Erf pattern's).  It is the activation Gelu(approximate = "tanh") names.  Every intermediate is read once;
// a near miss is no match and its nodes import (or are refused: a left-over Pow is an unsupported operator) one by one
void Planner::MatchGeluTanh() {
    bool any = false;
    for (const OnnxNode& on : m.nodes) any = any || on.op == "Tanh";
    if (!any) return;
    IndexGraph();
    auto near = [&](const std::string& name, double want) {
        const OnnxTensor* t = gi.cst(name);
        if (!t || t->numel() != 1) return false;
        const double v = t->f.size() == 1 ? double(t->f[0]) : (t->i.size() == 1 ? double(t->i[0]) : want + 1.0);
        return std::fabs(v - want) <= 1e-6 * std::fabs(want);
    };
    // Mul / Add of a constant near c and something else: the something else's name (empty: not that)
    auto with_const = [&](const OnnxNode* p, const char* op, double c) -> std::string {
        if (!p || p->op != op || p->inputs.size() != 2 || gi.nreaders(p->outputs[0]) != 1) return "";
        if (near(p->inputs[0], c) && !gi.cst(p->inputs[1])) return p->inputs[1];
        if (near(p->inputs[1], c) && !gi.cst(p->inputs[0])) return p->inputs[0];
        return "";
    };
    for (const OnnxNode& th : m.nodes) {
        if (th.op != "Tanh" || th.inputs.size() != 1 || gi.nreaders(th.outputs[0]) != 1) continue;
        std::vector<const OnnxNode*> taken = {&th};
        const OnnxNode* m1 = gi.producer(th.inputs[0]);                    // c1 * (x + c2 x^3)
        const std::string inner = with_const(m1, "Mul", 0.7978845608028654);
        const OnnxNode* ad = inner.empty() ? nullptr : gi.producer(inner);
        if (!ad || ad->op != "Add" || ad->inputs.size() != 2 || gi.nreaders(ad->outputs[0]) != 1) continue;
        taken.insert(taken.end(), {m1, ad});
        std::string x;
        bool ok = false;
        for (int side = 0; side < 2 && !ok; ++side) {
            x = ad->inputs[size_t(side)];
            const OnnxNode* m2 = gi.producer(ad->inputs[size_t(1 - side)]);  // c2 * x^3
            const std::string cube = with_const(m2, "Mul", 0.044715);
            const OnnxNode* cb = cube.empty() ? nullptr : gi.producer(cube);
            if (!cb || cb->inputs.size() != 2 || gi.nreaders(cb->outputs[0]) != 1 || gi.cst(x)) continue;
            if (cb->op == "Pow" && cb->inputs[0] == x && near(cb->inputs[1], 3.0)) { taken.insert(taken.end(), {m2, cb}); ok = true; }
            else if (cb->op == "Mul") {
                for (int s2 = 0; s2 < 2 && !ok; ++s2) {
                    const OnnxNode* sq = gi.producer(cb->inputs[size_t(1 - s2)]);
                    if (cb->inputs[size_t(s2)] == x && sq && sq->op == "Mul" && sq->inputs.size() == 2 && sq->inputs[0] == x && sq->inputs[1] == x && gi.nreaders(sq->outputs[0]) == 1) {
                        taken.insert(taken.end(), {m2, cb, sq});
                        ok = true;
                    }
                }
            }
        }
        if (!ok) continue;
        // behind the Tanh: 1 + tanh, then the product with x and 0.5 in any association
        const OnnxNode* a1 = gi.only_reader(th.outputs[0]);
        if (with_const(a1, "Add", 1.0) != th.outputs[0]) continue;
        taken.push_back(a1);
        const OnnxNode* p1 = gi.only_reader(a1->outputs[0]);
        if (!p1 || p1->op != "Mul" || p1->inputs.size() != 2) continue;
        const std::string o1 = p1->inputs[p1->inputs[0] == a1->outputs[0] ? 1 : 0];
        const OnnxNode* head = nullptr;
        if (const OnnxNode* hx = gi.producer(o1); with_const(hx, "Mul", 0.5) == x) { taken.push_back(hx); head = p1; }      // (0.5 x) (1 + t)
        else {
            const OnnxNode* p2 = gi.only_reader(p1->outputs[0]);
            if (!p2 || p2->op != "Mul" || p2->inputs.size() != 2) continue;
            const std::string o2 = p2->inputs[p2->inputs[0] == p1->outputs[0] ? 1 : 0];
            if ((o1 == x && near(o2, 0.5)) || (near(o1, 0.5) && o2 == x)) { taken.push_back(p1); head = p2; }               // ((1 + t) x) 0.5, ((1 + t) 0.5) x
        }
        if (!head) continue;
        for (const OnnxNode* p : taken) gelu_skip.insert(p);
        gelu_head[head] = x;
    }
}

// The separate q / k / v spelling (BERT's eager attention):
//   q, k, v = Transpose(Reshape(MatMul(x, W*) + b*, [N, L, H, hd]), [0,2,1,3]);  kT = Transpose(k, [0,1,3,2]) (or the single Transpose [0,2,3,1] of the Reshape)
//   MatMul(q, kT) [* c | / c] -> [+ mask] -> Softmax -> MatMul(., v) -> Transpose [0,2,1,3] -> Reshape [N, L, D]
// The three Linears read the same token value and are read by their Reshape alone: they become ONE Linear x -> [N, L, 3 D] (weights and bias
// concatenated, column s D + h hd + e), and the attention node reads today's qkv layout.  false: q is not Transpose [0,2,1,3] (the other spelling)
// Llama's eager attention is the same spelling with three additions, each matched here and refused by name on a near miss:
//   * the Linears have no bias (a MatMul alone): the merged Linear then has none either
//   * k and v come from narrower Linears [Din, Hkv hd] (Reshape [N, L, Hkv, hd]) and pass repeat_kv, Unsqueeze(axis 2) -> Expand([N, Hkv, g, L, hd]) ->
//     Reshape([N, H, L, hd]) with constant shapes (g = 1: a no-op), behind their Transpose: the merged Linear is [Din, D + 2 Dkv], the step has kv_heads
//   * q and k pass the rotary embedding between their Transpose [0,2,1,3] and the score MatMul, Add(Mul(t, cos), Mul(Concat(Neg(Slice(t, hd/2:)),
//     Slice(t, :hd/2), axis -1), sin)), either operand order; cos / sin are float constants that broadcast as [1, 1, L, hd]: initializers, or Unsqueeze /
//     Slice / Gather-by-constant of a [P, hd] table, evaluated here.  q and k must use the same tables, element for element; the tables ride in the
//     weight blob and the kernels rotate inside their own loads (no step, no pass over the qkv buffer)
bool Planner::MatchSplitAttention(const OnnxNode& sm, const OnnxNode* pv, const std::string& scores, const std::string& prefix, AttnMatch& am, const OnnxNode*& head,
                                  std::vector<const OnnxNode*>& taken) {
    auto miss = [&](const std::string& what) { fail(prefix + what); };
    auto nm_of = [](const OnnxNode* p) { return p->name.empty() ? p->outputs[0] : p->name; };
    auto perm_is = [](const OnnxNode* p, std::vector<int64_t> want) { return p && p->op == "Transpose" && p->attr_ints("perm", {}) == want; };
    auto graph_input = [&](const std::string& name) -> const OnnxValueInfo* {
        for (const auto& vi : m.inputs) if (vi.name == name) return &vi;
        return nullptr;
    };
    auto graph_output = [&](const std::string& name) { for (const auto& vo : m.outputs) if (vo.name == name) return true; return false; };
    double scale = 1.0;
    auto peel = [&](std::string cur) -> std::string {
        for (;;) {
            const OnnxNode* p = gi.producer(cur);
            if (!p || (p->op != "Mul" && p->op != "Div") || p->inputs.size() != 2) return cur;
            const OnnxTensor *c0 = gi.cst(p->inputs[0]), *c1 = gi.cst(p->inputs[1]);
            if ((c0 != nullptr) == (c1 != nullptr) || (p->op == "Div" && !c1)) return cur;
            const OnnxTensor* c = c0 ? c0 : c1;
            if (c->numel() != 1 || c->f.size() != 1) miss("the scale constant of " + p->op + " " + nm_of(p) + " is not a scalar");
            if (p->op == "Div" && c->f[0] == 0.f) miss("division by zero in " + nm_of(p));
            scale = p->op == "Div" ? scale / double(c->f[0]) : scale * double(c->f[0]);
            taken.push_back(p);
            cur = p->inputs[c0 ? 1 : 0];
        }
    };
    // ---- Llama's additions between Transpose(., [0,2,1,3]) and the two MatMuls ----
    auto ints_of = [&](const OnnxNode* p, const char* attr, size_t input) {
        std::vector<int64_t> v = p->attr_ints(attr, {});
        if (v.empty() && p->inputs.size() > input && !p->inputs[input].empty()) if (const OnnxTensor* t = gi.cst(p->inputs[input])) v = t->i;
        return v;
    };
    auto one_reader = [&](const OnnxNode* p) {
        if (gi.nreaders(p->outputs[0]) != 1) miss("the intermediate " + p->outputs[0] + " (" + p->op + " " + nm_of(p) + ") has " + std::to_string(gi.nreaders(p->outputs[0])) + " readers, not 1");
    };
    // a rope table as the graph's constants give it: an initializer / Constant, or Unsqueeze / Slice (step 1) / Gather(axis 0, constant indices) of one
    std::string gather_pos;                        // const_eval: the INT64 graph input that gathers the table being evaluated (empty: constant positions)
    std::string pos_miss;                          // const_eval: the refusal of position ids wider than [N, 1], for the import (AttnMatch::rope_pos_miss)
    std::function<bool(const std::string&, OnnxTensor&, std::vector<const OnnxNode*>&)> const_eval = [&](const std::string& name, OnnxTensor& out, std::vector<const OnnxNode*>& nodes) -> bool {
        if (const OnnxTensor* t = gi.cst(name)) { out = *t; return !t->f.empty(); }
        const OnnxNode* p = gi.producer(name);
        if (!p || p->inputs.empty()) return false;
        OnnxTensor in;
        if (p->op != "Unsqueeze" && p->op != "Slice" && p->op != "Gather") return false;
        if (!const_eval(p->inputs[0], in, nodes)) return false;
        nodes.push_back(p);
        const int64_t rank = int64_t(in.dims.size());
        // run-time positions (a decode step): Gather(table [max_pos, hd], position_ids [N, 1], axis 0) -> Unsqueeze(axes [1]) broadcasts as [N, 1, 1, hd].
        // The whole table is the constant; the kernels index it with the input's values
        if (p->op == "Gather" && p->inputs.size() == 2 && !gi.cst(p->inputs[1])) {
            const std::string who = "Gather " + nm_of(p) + ": the position ids " + p->inputs[1] + " of the rope table ";
            bool ok = false;
            int64_t width = 0;
            for (size_t i = 0; i < m.inputs.size(); ++i)
                if (m.inputs[i].name == p->inputs[1]) { ok = m.inputs[i].elem_type == ONNX_INT64 && input_shapes[i].size() == 2; width = ok ? input_shapes[i][1] : 0; }
            const std::string not_n1 = who + "are neither a constant nor an INT64 graph input [N, 1] (supported: constant positions, or position_ids [N, 1] of a decode step)";
            if (!ok) miss(not_n1);
            if (width != 1) pos_miss = prefix + not_n1;      // (an extend step takes [N, Lq]: the import, which knows Lq, decides)
            if (p->attr_i("axis", 0) != 0 || rank != 2 || !gather_pos.empty()) miss(who + "must gather a [max_pos, hd] table once, along axis 0");
            gather_pos = p->inputs[1];
            out = in;
            return true;
        }
        if (p->op == "Unsqueeze" && !gather_pos.empty()) {
            if (ints_of(p, "axes", 1) != std::vector<int64_t>{1}) miss("Unsqueeze " + nm_of(p) + ": a rope table gathered by " + gather_pos + " [N, 1] must be unsqueezed at axes [1] (it then broadcasts as [N, 1, 1, hd])");
            out = in;
            return true;
        }
        if (!gather_pos.empty()) return false;
        if (p->op == "Unsqueeze") {
            std::vector<int64_t> ax = ints_of(p, "axes", 1);
            if (ax.empty()) return false;
            const int64_t orank = rank + int64_t(ax.size());
            for (int64_t& a : ax) if (a < 0) a += orank;
            std::sort(ax.begin(), ax.end());
            out = in;
            for (int64_t a : ax) { if (a < 0 || a > int64_t(out.dims.size())) return false; out.dims.insert(out.dims.begin() + a, 1); }
            return true;
        }
        // Slice and Gather along one leading-row axis of the table: the rows [r0, r1) or the rows idx[...] of `in` seen as [rows][inner]
        int64_t axis = 0;
        std::vector<int64_t> pick;
        if (p->op == "Gather") {
            const OnnxTensor* ix = p->inputs.size() == 2 ? gi.cst(p->inputs[1]) : nullptr;
            axis = p->attr_i("axis", 0);
            if (!ix || ix->i.empty() || ix->dims.size() != 1) return false;
            pick = ix->i;
        } else {
            const std::vector<int64_t> st = ints_of(p, "starts", 1), en = ints_of(p, "ends", 2), ax = ints_of(p, "axes", 3), sp = ints_of(p, "steps", 4);
            if (st.size() != 1 || en.size() != 1 || ax.size() > 1 || sp.size() > 1 || (!sp.empty() && sp[0] != 1)) return false;
            axis = ax.empty() ? 0 : ax[0];
            if (axis < 0) axis += rank;
            if (axis < 0 || axis >= rank) return false;
            const int64_t n = in.dims[size_t(axis)];
            int64_t a = st[0] < 0 ? st[0] + n : st[0], b = en[0] < 0 ? en[0] + n : en[0];
            a = std::min(std::max(a, int64_t(0)), n);
            b = std::min(std::max(b, int64_t(0)), n);
            for (int64_t r = a; r < b; ++r) pick.push_back(r);
        }
        if (axis < 0) axis += rank;
        if (axis < 0 || axis >= rank) return false;
        int64_t outer = 1, inner = 1;
        for (int64_t k = 0; k < axis; ++k) outer *= in.dims[size_t(k)];
        for (int64_t k = axis + 1; k < rank; ++k) inner *= in.dims[size_t(k)];
        const int64_t n = in.dims[size_t(axis)];
        out = OnnxTensor();
        out.dtype = in.dtype;
        out.dims = in.dims;
        out.dims[size_t(axis)] = int64_t(pick.size());
        for (int64_t o = 0; o < outer; ++o)
            for (int64_t r : pick) {
                if (r < 0) r += n;
                if (r < 0 || r >= n) return false;
                out.f.insert(out.f.end(), in.f.begin() + (o * n + r) * inner, in.f.begin() + (o * n + r + 1) * inner);
            }
        return true;
    };
    struct Rope { bool on = false; std::vector<float> cos, sin; int64_t rows = 0, hd = 0; std::string name, pos; int tables = 0; };
    // name = Add(Mul(t, cos), Mul(Concat(Neg(Slice(t, hd/2:)), Slice(t, :hd/2), axis -1), sin)), either operand order: -> t (name itself: no rotation here)
    auto unrope = [&](const std::string& name, const char* which, Rope& r) -> std::string {
        const OnnxNode* ad = gi.producer(name);
        if (!ad || ad->op != "Add" || ad->inputs.size() != 2) return name;
        const OnnxNode *m0 = gi.producer(ad->inputs[0]), *m1 = gi.producer(ad->inputs[1]);
        if (!m0 || !m1 || m0->op != "Mul" || m1->op != "Mul" || m0->inputs.size() != 2 || m1->inputs.size() != 2) return name;
        const std::string who = std::string("the rotary embedding of ") + which + " (Add " + nm_of(ad) + "): ";
        r.name = nm_of(ad);
        // the Mul whose activation operand is a Concat is the rotate_half branch
        auto act_side = [&](const OnnxNode* mu, OnnxTensor& table) -> std::string {
            for (int k = 0; k < 2; ++k) {
                std::vector<const OnnxNode*> nodes;
                OnnxTensor t;
                gather_pos.clear();
                if (const_eval(mu->inputs[size_t(k)], t, nodes)) {
                    const std::string gp = gather_pos;
                    if (r.tables++ > 0 && r.pos != gp) miss(who + "its cos and sin tables are not gathered by the same position ids");
                    r.pos = gp;
                    if (!gp.empty()) for (const OnnxNode* p : nodes) mask_nodes.insert(p);      // (they may read the INT64 graph input)
                    OnnxTensor dummy;
                    std::vector<const OnnxNode*> n2;
                    if (const_eval(mu->inputs[size_t(1 - k)], dummy, n2)) miss(who + "both operands of Mul " + nm_of(mu) + " are constants");
                    table = std::move(t);
                    for (const OnnxNode* p : nodes) rope_const_nodes.insert(p);
                    return mu->inputs[size_t(1 - k)];
                }
            }
            miss(who + "Mul " + nm_of(mu) + " has no constant operand: cos and sin must be float constants (initializers, or Unsqueeze / Slice / Gather by constants of a table)");
            return "";
        };
        OnnxTensor t0, t1;
        const std::string a0 = act_side(m0, t0), a1 = act_side(m1, t1);
        const OnnxNode *c0 = gi.producer(a0), *c1 = gi.producer(a1);
        const bool rot0 = c0 && c0->op == "Concat", rot1 = c1 && c1->op == "Concat";
        if (rot0 == rot1) miss(who + "exactly one of its two products must read rotate_half, Concat(Neg(Slice(t, hd/2:)), Slice(t, :hd/2), axis -1)");
        const OnnxNode* cat = rot0 ? c0 : c1;
        const std::string t = rot0 ? a1 : a0;
        OnnxTensor& cos = rot0 ? t1 : t0;
        OnnxTensor& sin = rot0 ? t0 : t1;
        // the tables broadcast as [1, 1, L, hd]
        auto table2 = [&](OnnxTensor& tb, const char* what) {
            std::vector<int64_t> d = tb.dims;
            while (d.size() > 2 && d[0] == 1) d.erase(d.begin());
            if (d.size() != 2 || tb.dims.size() > 4 || int64_t(tb.f.size()) != d[0] * d[1]) miss(who + "the " + what + " table does not broadcast as [1, 1, L, hd]");
            tb.dims = d;
        };
        table2(cos, "cos");
        table2(sin, "sin");
        if (cos.dims != sin.dims) miss(who + "the cos and sin tables differ in shape");
        const int64_t hd = cos.dims[1];
        if (hd < 2 || hd % 2) miss(who + "the head size " + std::to_string(hd) + " of the tables is not even");
        // rotate_half
        const int64_t cax = cat->attr_i("axis", 0);
        if (cat->inputs.size() != 2 || (cax != -1 && cax != 3)) miss(who + "Concat " + nm_of(cat) + " is not a Concat of two parts along the last axis");
        const OnnxNode *ng = gi.producer(cat->inputs[0]), *lo = gi.producer(cat->inputs[1]);
        if (!ng || ng->op != "Neg")
            miss(who + "Concat " + nm_of(cat) + " is not rotate_half: its first part must be Neg(Slice(t, hd/2:)) and its second Slice(t, :hd/2); the order (x1, -x2) is another function");
        const OnnxNode* hi = gi.producer(ng->inputs[0]);
        auto half_slice = [&](const OnnxNode* sl, bool upper) {
            if (!sl || sl->op != "Slice" || sl->inputs.empty() || sl->inputs[0] != t) return false;
            const std::vector<int64_t> st = ints_of(sl, "starts", 1), en = ints_of(sl, "ends", 2), ax = ints_of(sl, "axes", 3), sp = ints_of(sl, "steps", 4);
            if (st.size() != 1 || en.size() != 1 || ax.size() != 1 || (ax[0] != -1 && ax[0] != 3) || (!sp.empty() && (sp.size() != 1 || sp[0] != 1))) return false;
            return upper ? st[0] == hd / 2 && en[0] >= hd : st[0] == 0 && en[0] == hd / 2;
        };
        if (!half_slice(hi, true) || !half_slice(lo, false))
            miss(who + "Concat " + nm_of(cat) + " is not rotate_half of " + t + ": its parts must be Neg(Slice(t, " + std::to_string(hd / 2) + ":)) and Slice(t, :" + std::to_string(hd / 2) + ") along the last axis");
        for (const OnnxNode* p : {m0, m1, cat, ng, hi, lo}) one_reader(p);
        if (gi.nreaders(t) != 3) miss(who + "the rotated value " + t + " has " + std::to_string(gi.nreaders(t)) + " readers, not 3 (its product with cos and the two Slices of rotate_half)");
        taken.insert(taken.end(), {ad, m0, m1, cat, ng, hi, lo});
        r.on = true;
        r.cos = cos.f;
        r.sin = sin.f;
        r.rows = cos.dims[0];
        r.hd = hd;
        return t;
    };
    // name = Reshape(Expand(Unsqueeze(t, axis 2), [N, Hkv, g, L, hd]), [N, H, L, hd]) with constant shapes: -> t (name itself: no repeat_kv here)
    auto unrepeat = [&](const std::string& name, const char* which, int64_t& g) -> std::string {
        const OnnxNode* rs = gi.producer(name);
        const OnnxNode* ex = rs && rs->op == "Reshape" && !rs->inputs.empty() ? gi.producer(rs->inputs[0]) : nullptr;
        if (!ex || ex->op != "Expand") return name;
        const std::string who = std::string("repeat_kv of ") + which + " (Expand " + nm_of(ex) + "): ";
        const OnnxNode* us = gi.producer(ex->inputs[0]);
        if (!us || us->op != "Unsqueeze" || ints_of(us, "axes", 1) != std::vector<int64_t>{2}) miss(who + "its input is not Unsqueeze(., axes [2])");
        const OnnxTensor *e5 = ex->inputs.size() == 2 ? gi.cst(ex->inputs[1]) : nullptr, *r4 = rs->inputs.size() == 2 ? gi.cst(rs->inputs[1]) : nullptr;
        if (!e5 || e5->i.size() != 5 || !r4 || r4->i.size() != 4) miss(who + "the shapes of the Expand [N, Hkv, g, L, hd] and of the Reshape [N, H, L, hd] behind it must be constants");
        g = e5->i[2];
        if (g < 1) miss(who + "the group size " + std::to_string(g) + " is not positive");
        if (graph_output(rs->outputs[0]))
            miss(who + "the graph output " + rs->outputs[0] + " is the value behind repeat_kv; a present output is the value in front of it, [N, Hkv, rows, hd]");
        for (const OnnxNode* p : {us, ex, rs}) one_reader(p);
        taken.insert(taken.end(), {us, ex, rs});
        am.rep_expand.push_back(e5->i);
        am.rep_reshape.push_back(r4->i);
        return us->inputs[0];
    };
    // name = Concat(past, t, axis 2) with past a FLOAT rank-4 graph input, the cache of a decode step: -> t (name itself: no cache here)
    auto uncat = [&](const std::string& name, const char* which, std::string& past, std::string& present, std::string& cat_name) -> std::string {
        const OnnxNode* cat = gi.producer(name);
        if (!cat || cat->op != "Concat" || cat->inputs.size() != 2) return name;
        const OnnxValueInfo *i0 = graph_input(cat->inputs[0]), *i1 = graph_input(cat->inputs[1]);
        if (!i0 && !i1) return name;
        const std::string who = std::string("the cache of ") + which + " (Concat " + nm_of(cat) + "): ";
        const std::string form = std::string("; supported: Concat(past, ") + which + ", axis 2) with past a FLOAT graph input [N, Hkv, P, hd] read by this Concat alone";
        if (!i0) miss(who + "its operands are in the order (" + which + ", past)" + form);
        if (i1) miss(who + "both operands are graph inputs" + form);
        const int64_t ax = cat->attr_i("axis", 0);
        if (ax != 2 && ax != -2) miss(who + "axis = " + std::to_string(ax) + form);
        if (i0->elem_type != ONNX_FLOAT || i0->dims.size() != 4) miss(who + "the past input " + i0->name + " is not a FLOAT tensor of rank 4" + form);
        if (gi.nreaders(i0->name) != 1) miss(who + "the past input " + i0->name + " has " + std::to_string(gi.nreaders(i0->name)) + " readers, not 1" + form);
        if (!graph_output(cat->outputs[0]) || gi.nreaders(cat->outputs[0]) != 2)
            miss(who + "its result " + cat->outputs[0] + " must be a graph output (present.*) and be read by this attention alone besides; it has " + std::to_string(gi.nreaders(cat->outputs[0])) + " readers");
        taken.push_back(cat);
        past = i0->name;
        present = cat->outputs[0];
        cat_name = nm_of(cat);
        return cat->inputs[1];
    };
    const OnnxNode* qk = gi.producer(peel(scores));
    {
        // the other spelling (q a Gather / Squeeze slice of one transposed qkv tensor): nothing here is an Add of two products or a Transpose [0,2,1,3]
        const OnnxNode* q0 = gi.producer(gi.peel_quiet(qk->inputs[0]));
        const bool rope_add = q0 && q0->op == "Add" && q0->inputs.size() == 2 && gi.producer(q0->inputs[0]) && gi.producer(q0->inputs[0])->op == "Mul" &&
                              gi.producer(q0->inputs[1]) && gi.producer(q0->inputs[1])->op == "Mul";
        if (!perm_is(q0, {0, 2, 1, 3}) && !rope_add) { taken.clear(); return false; }
    }
    Rope rq, rk;
    const OnnxNode* qt = gi.producer(unrope(peel(qk->inputs[0]), "q", rq));
    if (!perm_is(qt, {0, 2, 1, 3})) miss(std::string("q is not ") + (rq.on ? "the rotary embedding of " : "") + "Transpose(Reshape(Linear(x), [N, L, H, hd]), [0,2,1,3])");
    const OnnxNode* kt = gi.producer(peel(qk->inputs[1]));
    const OnnxNode* k_rs = nullptr;
    int64_t gk = 0, gv = 0;                        // repeat_kv's group size on k and on v (0: no repeat_kv)
    if (perm_is(kt, {0, 2, 3, 1})) k_rs = gi.producer(kt->inputs[0]);
    else if (perm_is(kt, {0, 1, 3, 2})) {
        const std::string k_cat = unrepeat(kt->inputs[0], "k", gk);
        const std::string k_new = uncat(k_cat, "k", am.past_k, am.present_k, am.cat_k);
        // a prefill with a cache: the rotated k (without rope: its Transpose) is also the graph output present.*.key
        if (am.past_k.empty() && graph_output(k_new)) am.present_k = k_new;
        const OnnxNode* k2 = gi.producer(unrope(k_new, "k", rk));
        if (!perm_is(k2, {0, 2, 1, 3})) miss("the second operand of MatMul " + nm_of(qk) + " is neither Transpose(Transpose(k, [0,2,1,3]), [0,1,3,2]) nor Transpose(k, [0,2,3,1])");
        taken.push_back(k2);
        k_rs = gi.producer(k2->inputs[0]);
    } else miss("the second operand of MatMul " + nm_of(qk) + " is neither Transpose(Transpose(k, [0,2,1,3]), [0,1,3,2]) nor Transpose(k, [0,2,3,1])");
    const std::string v_new = uncat(unrepeat(pv->inputs[1], "v", gv), "v", am.past_v, am.present_v, am.cat_v);
    if (am.past_v.empty() && graph_output(v_new)) am.present_v = v_new;
    const OnnxNode* vt = gi.producer(v_new);
    if (!perm_is(vt, {0, 2, 1, 3})) miss("the second operand of MatMul " + nm_of(pv) + " is not Transpose(v, perm [0,2,1,3])");
    if (am.past_k.empty() != am.past_v.empty())
        miss(std::string("only ") + (am.past_k.empty() ? "v" : "k") + " has a cache (Concat " + (am.past_k.empty() ? am.cat_v : am.cat_k) + "); k and v must both be Concat(past, ., axis 2)");
    if (am.present_k.empty() != am.present_v.empty())
        miss(std::string("only ") + (am.present_k.empty() ? am.present_v : am.present_k) + " is a graph output; present key and present value come as a pair");
    if (rq.on && rq.pos != rk.pos)
        miss("the positions of k (Add " + rk.name + ": " + (rk.pos.empty() ? "constant" : rk.pos) + ") are not the positions of q (Add " + rq.name + ": " + (rq.pos.empty() ? "constant" : rq.pos) + ")");
    if (!pos_miss.empty() && am.past_k.empty()) fail(pos_miss);
    if (rq.on && !rq.pos.empty() && am.past_k.empty())
        miss("the rope tables (Add " + rq.name + ") are gathered by the graph input " + rq.pos + " without a cache; run-time positions are supported in a decode step (Concat(past, k, axis 2)) only");
    if (rq.on != rk.on) miss(std::string("only ") + (rq.on ? "q" : "k") + " passes a rotary embedding (Add " + (rq.on ? rq.name : rk.name) + "); q and k must both be rotated");
    if (rq.on) {
        if (rq.rows != rk.rows || rq.hd != rk.hd || rq.cos != rk.cos) miss("the cos table of q (Add " + rq.name + ") is not the cos table of k (Add " + rk.name + "), element for element");
        if (rq.sin != rk.sin) miss("the sin table of q (Add " + rq.name + ") is not the sin table of k (Add " + rk.name + "), element for element");
    }
    if (gk != gv) miss("repeat_kv repeats k " + std::to_string(gk) + " times and v " + std::to_string(gv) + " times");
    const OnnxNode* rs[3] = {gi.producer(qt->inputs[0]), k_rs, gi.producer(vt->inputs[0])};
    static const char* const which[3] = {"q", "k", "v"};
    const OnnxNode *mm[3], *add[3];
    const OnnxTensor *W[3], *B[3];
    std::vector<int64_t> shape4;
    // GPT-2: q, k, v = the three parts of Split(axis 2, [D, D, D]) of one c_attn Linear (the exporter omits `split` when the parts are equal): the
    // Split's input is the qkv layout itself, and the Split is the head
    const OnnxNode* sp = rs[0] && !rs[0]->inputs.empty() ? gi.producer(rs[0]->inputs[0]) : nullptr;
    const bool fused = sp && sp->op == "Split" && sp->outputs.size() == 3 && rs[1] && rs[2] && rs[0]->op == "Reshape" && rs[1]->op == "Reshape" && rs[2]->op == "Reshape";
    if (fused) {
        for (int s = 0; s < 3; ++s) {
            const OnnxTensor* s4 = rs[s]->inputs.size() == 2 ? gi.cst(rs[s]->inputs[1]) : nullptr;
            if (!s4 || s4->i.size() != 4 || s4->i[2] <= 0 || s4->i[3] <= 0) miss(std::string(which[s]) + " is not Reshape(part " + std::to_string(s) + " of the Split, [N, L, H, hd]) with a constant shape");
            if (s == 0) shape4 = s4->i;
            else if (s4->i[2] != shape4[2] || s4->i[3] != shape4[3]) miss("the q / k / v Reshapes differ in heads or head size");
            if (rs[s]->inputs[0] != sp->outputs[size_t(s)]) miss(std::string(which[s]) + " is not part " + std::to_string(s) + " of Split " + nm_of(sp) + " (q, k, v must be its outputs 0, 1, 2)");
            for (const OnnxNode* p : {rs[s]})
                if (gi.nreaders(p->outputs[0]) != 1 || gi.nreaders(p->inputs[0]) != 1) miss("the " + std::string(which[s]) + " part of Split " + nm_of(sp) + " or its Reshape has a second reader (only its own attention may read it)");
            taken.push_back(rs[s]);
        }
        const int64_t D = shape4[2] * shape4[3], ax = sp->attr_i("axis", 0);
        if (ax != 2 && ax != -1) miss("Split " + nm_of(sp) + " has axis = " + std::to_string(ax) + ", not 2 (the channel axis of [N, L, 3 D])");
        std::vector<int64_t> parts = sp->attr_ints("split", {});
        if (parts.empty() && sp->inputs.size() > 1 && !sp->inputs[1].empty()) {
            const OnnxTensor* pt = gi.cst(sp->inputs[1]);
            if (!pt) miss("the split sizes of Split " + nm_of(sp) + " are not constant");
            parts = pt->i;
        }
        if (!parts.empty() && parts != std::vector<int64_t>{D, D, D}) miss("Split " + nm_of(sp) + " does not cut [H * hd, H * hd, H * hd] = three parts of " + std::to_string(D));
    }
    int64_t kvh = 0;                               // K / V heads of the split form (k's and v's Reshape)
    for (int s = 0; s < 3 && !fused; ++s) {
        const OnnxTensor* s4 = rs[s] && rs[s]->op == "Reshape" && rs[s]->inputs.size() == 2 ? gi.cst(rs[s]->inputs[1]) : nullptr;
        if (!s4 || s4->i.size() != 4 || s4->i[2] <= 0 || s4->i[3] <= 0) miss(std::string(which[s]) + " is not Reshape(Linear(x), [N, L, H, hd]) with a constant shape");
        if (s == 0) shape4 = s4->i;
        else if (s4->i[3] != shape4[3] || (s == 2 && s4->i[2] != kvh)) miss("the q / k / v Reshapes differ in heads or head size");
        if (s == 1) kvh = s4->i[2];
        // grouped K / V heads: fewer heads on k and v, whole groups of query heads per K / V head, repeat_kv by exactly that group
        if (s == 1 && kvh != shape4[2]) {
            if (kvh > shape4[2] || shape4[2] % kvh)
                miss("heads % kv_heads != 0: q has " + std::to_string(shape4[2]) + " heads (Reshape " + nm_of(rs[0]) + "), k has " + std::to_string(kvh) + " (Reshape " + nm_of(rs[1]) +
                     "); a K / V head serves a whole group of query heads");
            if (gk != shape4[2] / kvh) miss("k and v have " + std::to_string(kvh) + " heads for q's " + std::to_string(shape4[2]) + ", but repeat_kv repeats them " + std::to_string(gk) + " times, not " + std::to_string(shape4[2] / kvh));
        }
        if (s == 1 && kvh == shape4[2] && gk > 1) miss("repeat_kv repeats k and v " + std::to_string(gk) + " times although they have q's " + std::to_string(kvh) + " heads");
        const int64_t Ds = s4->i[2] * s4->i[3];    // this Linear's columns: H hd for q, Hkv hd for k and v
        // the Linear: MatMul + Add, or the MatMul alone (Llama's projections have no bias)
        const OnnxNode* top = gi.producer(rs[s]->inputs[0]);
        add[s] = top && top->op == "Add" && top->inputs.size() == 2 ? top : nullptr;
        B[s] = nullptr;
        if (add[s]) {
            const int bi = gi.cst(add[s]->inputs[0]) ? 0 : 1;
            B[s] = gi.cst(add[s]->inputs[size_t(bi)]);
            mm[s] = gi.producer(add[s]->inputs[size_t(1 - bi)]);
            if (!B[s] || B[s]->f.empty()) miss(std::string(which[s]) + " is not the Reshape of a Linear (MatMul(x, W [Din, D]) + b [D])");
        } else mm[s] = top;
        if (!mm[s] || mm[s]->op != "MatMul") miss(std::string(which[s]) + " is not the Reshape of a Linear (MatMul + Add, or a MatMul alone)");
        W[s] = mm[s]->inputs.size() == 2 ? gi.cst(mm[s]->inputs[1]) : nullptr;
        if (!W[s] || gi.cst(mm[s]->inputs[0]) || W[s]->f.empty() || W[s]->dims.size() != 2)
            miss(std::string(which[s]) + " is not the Reshape of a Linear (MatMul(x, W [Din, D]) + b [D])");
        if (mm[s]->inputs[0] != mm[0]->inputs[0])
            miss("the " + std::string(which[s]) + " Linear " + nm_of(mm[s]) + " reads " + mm[s]->inputs[0] + ", the q Linear " + mm[0]->inputs[0] + " (q, k and v must come from the same tokens)");
        if (W[s]->dims[0] != W[0]->dims[0] || W[s]->dims[1] != Ds || (B[s] && B[s]->numel() != Ds))
            miss("the " + std::string(which[s]) + " Linear " + nm_of(mm[s]) + " is not [Din, H * hd = " + std::to_string(Ds) + "] with a bias [" + std::to_string(Ds) + "] like the q Linear");
        for (const OnnxNode* p : {mm[s], add[s], rs[s]})
            if (p && gi.nreaders(p->outputs[0]) != 1) miss("the " + std::string(which[s]) + " Linear's " + p->op + " " + nm_of(p) + " has " + std::to_string(gi.nreaders(p->outputs[0])) + " readers, not 1 (only its own attention may read it)");
        taken.push_back(mm[s]);
        if (add[s]) taken.push_back(add[s]);
        taken.push_back(rs[s]);
    }
    if (fused && !am.past_k.empty())
        miss("a cache (Concat " + am.cat_k + ") behind the Split of one qkv Linear (GPT-2's spelling) is not supported; the separate q / k / v Linears of a Llama-class graph are");
    if (fused && !am.present_k.empty()) miss("the graph output " + am.present_k + " behind the Split of one qkv Linear (GPT-2's spelling) is not supported");
    if (fused && (rq.on || gk > 0)) miss("a rotary embedding or repeat_kv behind the Split of one qkv Linear is not supported (the separate q / k / v Linears are)");
    if (rq.on && rq.hd != shape4[3]) miss("the rope tables (Add " + rq.name + ") are " + std::to_string(rq.hd) + " wide, the heads " + std::to_string(shape4[3]));
    const int64_t axis = sm.attr_i("axis", -1);
    if (axis != -1 && axis != 3) miss("Softmax axis = " + std::to_string(axis) + " (only the last axis, -1 or 3, is an attention)");
    const OnnxNode* ot = gi.only_reader(pv->outputs[0]);
    if (!perm_is(ot, {0, 2, 1, 3})) miss("the result of MatMul " + nm_of(pv) + " is not read by Transpose(perm [0,2,1,3]) alone");
    const OnnxNode* orr = gi.only_reader(ot->outputs[0]);
    const OnnxTensor* s3 = orr && orr->op == "Reshape" && orr->inputs.size() == 2 ? gi.cst(orr->inputs[1]) : nullptr;
    if (!s3 || s3->i.size() != 3) miss("the transposed result is not read by Reshape(., [N, L, D]) alone");
    // (a rotated value has three readers, its product with cos and the two Slices of rotate_half: the rotary match counted them)
    const bool prefill_present = am.past_k.empty() && !am.present_k.empty();      // (a present output of a prefill is one more reader of k's and v's value)
    for (const OnnxNode* p : {qk, qt, kt, vt, pv, ot, &sm})
        if (gi.nreaders(p->outputs[0]) != (rq.on && p == qt ? 3 : 1) + (prefill_present && p == vt ? 1 : 0)) miss("the intermediate " + p->outputs[0] + " has " + std::to_string(gi.nreaders(p->outputs[0])) + " readers, not 1");
    for (const OnnxNode* p : taken)
        if ((p->op == "Mul" || p->op == "Div" || p->op == "Transpose") && gi.nreaders(p->outputs[0]) != (rk.on && perm_is(p, {0, 2, 1, 3}) ? 3 : 1) + (prefill_present && p->outputs[0] == am.present_k ? 1 : 0)) miss("the intermediate " + p->outputs[0] + " has " + std::to_string(gi.nreaders(p->outputs[0])) + " readers, not 1");
    taken.insert(taken.end(), {qk, qt, kt, vt, pv, ot, orr, &sm});
    if (fused) {
        head = sp;
        am.fused = true;
        am.name = nm_of(sp);
        am.heads = shape4[2];
        am.head_dim = shape4[3];
        am.scale = scale;
        am.out = orr->outputs[0];
        am.shape3 = s3->i;
        return true;
    }
    // the merged Linear: columns q (D) | k (Dkv) | v (Dkv), head h at h hd inside its part; without a bias where none of the three has one
    const int64_t Din = W[0]->dims[0], D = W[0]->dims[1], Dkv = W[1]->dims[1], Dall = D + 2 * Dkv;
    const int64_t off[3] = {0, D, D + Dkv};
    OnnxTensor w, b;
    w.dtype = b.dtype = ONNX_FLOAT;
    w.dims = {Din, Dall};
    b.dims = {Dall};
    w.f.resize(size_t(Din * Dall));
    for (int64_t k = 0; k < Din; ++k)
        for (int s = 0; s < 3; ++s) {
            const int64_t Ds = W[s]->dims[1];
            std::copy(W[s]->f.begin() + k * Ds, W[s]->f.begin() + (k + 1) * Ds, w.f.begin() + k * Dall + off[s]);
        }
    am.no_bias = !B[0] && !B[1] && !B[2];
    for (int s = 0; s < 3 && !am.no_bias; ++s) {
        if (B[s]) b.f.insert(b.f.end(), B[s]->f.begin(), B[s]->f.end());
        else b.f.insert(b.f.end(), size_t(W[s]->dims[1]), 0.f);      // (a mixed form: some of the three Linears have a bias)
    }
    am.kv_heads = kvh;
    if (rq.on) {
        am.rope = true;
        am.rope_cos = rq.cos;
        am.rope_sin = rq.sin;
        am.rope_rows = rq.rows;
        am.rope_name = rq.name;
        am.rope_pos = rq.pos;
        am.rope_pos_miss = pos_miss;
    }
    // the head: the first of the three MatMuls in graph order (x is defined there)
    for (const OnnxNode& on : m.nodes) if (&on == mm[0] || &on == mm[1] || &on == mm[2]) { head = &on; break; }
    am.split = true;
    am.x = mm[0]->inputs[0];
    am.name = nm_of(mm[0]) + "+" + nm_of(mm[1]) + "+" + nm_of(mm[2]);
    am.w_name = w.name = am.name + "/qkv_w";
    am.b_name = b.name = am.name + "/qkv_b";
    L.add_derived(std::move(w));
    if (!am.no_bias) L.add_derived(std::move(b));
    am.heads = shape4[2];
    am.head_dim = shape4[3];
    am.scale = scale;
    am.out = orr->outputs[0];
    am.shape3 = s3->i;
    return true;
}

// `scores`: the name the scaled q k^T product reaches the Softmax (or, in a window attention, the bias Add) under
Planner::AttnCore Planner::MatchAttentionCore(const OnnxNode& sm, const OnnxNode* pv, const std::string& scores, const std::string& miss_prefix) {
    const auto& readers = gi.readers;
    auto cst = [&](const std::string& name) { return gi.cst(name); };
    auto producer = [&](const std::string& name) { return gi.producer(name); };
    auto perm_is = [](const OnnxNode* p, std::vector<int64_t> want) { return p && p->op == "Transpose" && p->attr_ints("perm", {}) == want; };
    auto nreaders = [&](const std::string& name) { const auto it = readers.find(name); return it == readers.end() ? 0 : it->second; };
    {
        auto miss = [&](const std::string& what) { fail(miss_prefix + what); };
        std::vector<const OnnxNode*> taken;
        double scale = 1.0;
        // a chain of Mul / Div by scalar constants above `cur`; each link read once
        auto peel = [&](std::string cur) -> std::string {
            for (;;) {
                const OnnxNode* p = producer(cur);
                if (!p || (p->op != "Mul" && p->op != "Div") || p->inputs.size() != 2) return cur;
                const OnnxTensor *c0 = cst(p->inputs[0]), *c1 = cst(p->inputs[1]);
                if ((c0 != nullptr) == (c1 != nullptr) || (p->op == "Div" && !c1)) return cur;
                const OnnxTensor* c = c0 ? c0 : c1;
                if (c->numel() != 1 || c->f.size() != 1) miss("the scale constant of " + p->op + " " + (p->name.empty() ? p->outputs[0] : p->name) + " is not a scalar");
                if (p->op == "Div" && c->f[0] == 0.f) miss("division by zero in " + p->name);
                scale = p->op == "Div" ? scale / double(c->f[0]) : scale * double(c->f[0]);
                taken.push_back(p);
                cur = p->inputs[c0 ? 1 : 0];
            }
        };
        const int64_t axis = sm.attr_i("axis", -1);
        if (axis != -1 && axis != 3) miss("Softmax axis = " + std::to_string(axis) + " (only the last axis, -1 or 3, is an attention)");
        const OnnxNode* qk = producer(peel(scores));
        const std::string q = peel(qk->inputs[0]);
        const std::string kt_name = peel(qk->inputs[1]);
        const OnnxNode* kt = producer(kt_name);
        if (!perm_is(kt, {0, 1, 3, 2})) miss("the second operand of MatMul " + qk->name + " is not Transpose(k, perm [0,1,3,2])");
        const std::string k = peel(kt->inputs[0]);
        const std::string v = pv->inputs[1];
        // q, k, v = slices 0, 1, 2 of one transposed qkv tensor
        const OnnxNode* split = nullptr;
        std::string T;
        auto slice_of = [&](const std::string& name, int64_t want) {
            const OnnxNode* g = producer(name);
            std::string src;
            int64_t idx = -1;
            if (g && g->op == "Gather" && g->inputs.size() == 2 && g->attr_i("axis", 0) == 0) {
                const OnnxTensor* ix = cst(g->inputs[1]);
                if (ix && ix->dims.empty() && ix->i.size() == 1) { idx = ix->i[0]; src = g->inputs[0]; }
            } else if (g && g->op == "Squeeze" && !g->inputs.empty()) {
                std::vector<int64_t> ax = g->attr_ints("axes", {});
                if (ax.empty() && g->inputs.size() > 1) if (const OnnxTensor* at = cst(g->inputs[1])) ax = at->i;
                const OnnxNode* sp = producer(g->inputs[0]);
                if (ax == std::vector<int64_t>{0} && sp && sp->op == "Split" && sp->outputs.size() == 3 && sp->attr_i("axis", 0) == 0 && !sp->inputs.empty()) {
                    for (int64_t o = 0; o < 3; ++o) if (sp->outputs[size_t(o)] == g->inputs[0]) idx = o;
                    src = sp->inputs[0];
                    if (split && split != sp) idx = -1;
                    split = sp;
                    if (nreaders(g->inputs[0]) != 1) miss("the Split output " + g->inputs[0] + " has a second reader");
                }
            }
            if (idx != want || src.empty() || (!T.empty() && src != T))
                miss(name + " is not slice " + std::to_string(want) + " of the transposed qkv tensor (q, k, v must be Gather(axis 0, index 0 / 1 / 2) or Split(axis 0) + "
                     "Squeeze slices of one Transpose [2,0,3,1,4])");
            T = src;
            taken.push_back(g);
        };
        slice_of(q, 0);
        slice_of(k, 1);
        slice_of(v, 2);
        if (split) taken.push_back(split);
        const OnnxNode* tr = producer(T);
        if (!perm_is(tr, {2, 0, 3, 1, 4})) miss("q, k and v are not slices of Transpose(perm [2,0,3,1,4])");
        const OnnxNode* rs = producer(tr->inputs[0]);
        const OnnxTensor* s5 = rs && rs->op == "Reshape" && rs->inputs.size() == 2 ? cst(rs->inputs[1]) : nullptr;
        if (!s5 || s5->i.size() != 5 || s5->i[2] != 3 || s5->i[3] <= 0 || s5->i[4] <= 0)
            miss("the qkv tensor is not Reshape(x, [N, L, 3, H, hd]) with a constant shape");
        // behind the second MatMul: Transpose [0,2,1,3] -> Reshape [N, L, D]
        const OnnxNode* ot = gi.only_reader(pv->outputs[0]);
        if (!perm_is(ot, {0, 2, 1, 3})) miss("the result of MatMul " + pv->name + " is not read by Transpose(perm [0,2,1,3]) alone");
        const OnnxNode* orr = gi.only_reader(ot->outputs[0]);
        const OnnxTensor* s3 = orr && orr->op == "Reshape" && orr->inputs.size() == 2 ? cst(orr->inputs[1]) : nullptr;
        if (!s3 || s3->i.size() != 3) miss("the transposed result is not read by Reshape(., [N, L, D]) alone");
        // every intermediate has one reader (the transposed qkv tensor: its three Gathers or its Split)
        taken.insert(taken.end(), {qk, kt, pv, ot, tr, &sm});
        for (const OnnxNode* p : taken)
            for (const std::string& o : p->outputs) {
                const int want = (p == tr && !split) ? 3 : 1;
                if (nreaders(o) != want) miss((p == qk || o == sm.inputs[0] ? "the scores " : "the intermediate ") + o + " has " + std::to_string(nreaders(o)) + " readers, not " + std::to_string(want));
            }
        if (nreaders(rs->outputs[0]) != 1) miss("the intermediate " + rs->outputs[0] + " has a second reader");
        AttnCore c;
        c.rs = rs;
        c.orr = orr;
        c.taken = std::move(taken);
        c.scale = scale;
        c.shape5 = s5->i;
        c.shape3 = s3->i;
        return c;
    }
}

void Planner::ImportAttention(const OnnxNode& on, const AttnMatch& am) {
    auto miss = [&](const std::string& what) { fail("attention " + am.name + ": " + what); };
    std::string qkv = on.inputs[0];
    if (am.split) {
        // the merged Linear as two nodes of the planner's own, imported like any Linear on tokens (a 1x1 conv; the bias folds into it)
        if (!L.is_tok(am.x)) miss("the input " + am.x + " of its q / k / v Linears is not a token view [N, L, D]");
        OnnxNode mm, add;
        mm.op = "MatMul";
        mm.name = am.name + "/qkv";
        mm.inputs = {am.x, am.w_name};
        mm.outputs = {am.name + "/qkv_mm"};
        add.op = "Add";
        add.name = am.name + "/qkv_bias";
        add.inputs = {mm.outputs[0], am.b_name};
        add.outputs = {am.name + "/qkv_out"};
        qkv = am.no_bias ? mm.outputs[0] : add.outputs[0];
        synth_nodes.push_back(std::move(mm));
        ImportNode(synth_nodes.back());
        if (!am.no_bias) {
            synth_nodes.push_back(std::move(add));
            ImportNode(synth_nodes.back());
        }
    }
    if (!L.is_tok(qkv)) miss("its qkv input " + qkv + " is not a token view [N, L, 3 D]");
    const int x = L.get_val(qkv);
    const Val X = L.vals[x];
    const int64_t D = am.heads * am.head_dim, Hkv = am.kv_heads > 0 ? am.kv_heads : am.heads;
    if (X.c != D + 2 * Hkv * am.head_dim)
        miss("the qkv rows have " + std::to_string(X.c) + " columns, not " + (Hkv == am.heads ? "3 * H * hd = " : "(H + 2 Hkv) * hd = ") + std::to_string(D + 2 * Hkv * am.head_dim));
    // the cache of a decode step: the past inputs [N, Hkv, P, hd] of this step, one new token
    const bool decode = !am.past_k.empty();
    int64_t P = 0;
    if (decode) {
        const Val &PK = L.vals[L.get_val(am.past_k)], &PV = L.vals[L.get_val(am.past_v)];
        auto dims_of = [](const Val& v) { return "[" + std::to_string(v.n) + ", " + std::to_string(v.c) + ", " + std::to_string(v.h) + ", " + std::to_string(v.w) + "]"; };
        if (PK.h != PV.h) miss("the K and V pasts differ in their rows P: " + am.past_k + " is " + dims_of(PK) + ", " + am.past_v + " is " + dims_of(PV));
        for (const Val* v : {&PK, &PV})
            if (v->n != X.n || v->c != Hkv || v->w != am.head_dim)
                miss("the past input " + v->name + " is " + dims_of(*v) + ", not [N, Hkv, P, hd] = [" + std::to_string(X.n) + ", " + std::to_string(Hkv) + ", P, " + std::to_string(am.head_dim) + "] of this step");
        P = PK.h;
        if (X.w != 1 && !am.chunk)
            miss("a past (Concat " + am.cat_k + ") with Lq = " + std::to_string(X.w) + " new tokens (chunked prefill into a cache) needs the chunk's causal mask, Add(scores, Where(Cast(ext, to BOOL), "
                 "finfo.min, C)), on the scores; it has " + (am.causal ? "a causal mask of the new tokens alone" : am.mask.empty() ? "no mask: the new tokens would see each other's future" : "a key mask alone: the new tokens would see each other's future") +
                 "; only a decode step, one new token, Lq = 1, goes without it");
        if (am.causal) miss("a causal mask together with a past (Concat " + am.cat_k + ") is not supported; one query attends to every cached key the key mask admits");
    }
    if (am.chunk) {
        // the constant C of the chunk mask against this step's P and Lq, element by element: 0 on the P cached columns and on and below the chunk's diagonal, <= -1e30 above it
        const std::string who = "the chunk mask Where " + am.chunk_where + ": ";
        if (!decode)
            miss(who + "a key mask and a causal constant in one value without a past (no Concat(past, k, axis 2)) is not supported; it is the mask of an extend step over a cache");
        const std::vector<int64_t>& d = am.chunk_c->dims;
        if (d[0] != 1 || d[1] != 1 || d[2] != X.w || d[3] != P + X.w)
            miss(who + "its constant is [" + std::to_string(d[0]) + ", " + std::to_string(d[1]) + ", " + std::to_string(d[2]) + ", " + std::to_string(d[3]) + "], not [1, 1, Lq, P + Lq] = [1, 1, " + std::to_string(X.w) + ", " +
                 std::to_string(P + X.w) + "] of this step (P = " + std::to_string(P) + " cached rows, Lq = " + std::to_string(X.w) + " new tokens)");
        for (int64_t i = 0; i < X.w; ++i)
            for (int64_t j = 0; j < P + X.w; ++j) {
                const float v = am.chunk_c->f[size_t(i * (P + X.w) + j)];
                const bool visible = j <= P + i;
                if (visible ? v != 0.f : !(v <= -1e30f))
                    miss(who + "its constant is not the chunk's causal mask (0 where j <= P + i, <= -1e30 above): element [" + std::to_string(i) + ", " + std::to_string(j) + "] is " + std::to_string(v) + " at P = " + std::to_string(P));
            }
    }
    const int64_t Lk = X.w + P;                    // keys of a query
    // repeat_kv's constant shapes: Expand to [N, Hkv, g, L, hd] (a 1 keeps the dim), Reshape to [N, H, L, hd]
    for (size_t k = 0; k < am.rep_expand.size(); ++k) {
        const std::vector<int64_t>&e = am.rep_expand[k], &r = am.rep_reshape[k];
        const int64_t want5[5] = {X.n, Hkv, e[2], Lk, am.head_dim}, want4[4] = {X.n, am.heads, Lk, am.head_dim};
        bool ok = e[2] * Hkv == am.heads;
        for (int d = 0; d < 5; ++d) ok = ok && (e[size_t(d)] == want5[d] || (d != 2 && e[size_t(d)] == 1));
        int neg = 0;
        for (int d = 0; d < 4; ++d) { neg += r[size_t(d)] == -1; ok = ok && (r[size_t(d)] == want4[d] || r[size_t(d)] == -1 || (d == 0 && r[0] == 0)); }
        if (!ok || neg > 1) miss("repeat_kv does not expand to [N, Hkv, g, L, hd] = [" + std::to_string(X.n) + ", " + std::to_string(Hkv) + ", " + std::to_string(am.heads / Hkv) + ", " + std::to_string(Lk) + ", " +
                                 std::to_string(am.head_dim) + "] and reshape to [N, H, L, hd]");
    }
    if (!am.split && !am.fused && ((am.shape5[0] != 0 && am.shape5[0] != X.n) || (am.shape5[1] != -1 && am.shape5[1] != 0 && am.shape5[1] != X.w))) miss("the Reshape to [N, L, 3, H, hd] does not keep N and L");
    if ((am.shape3[0] != 0 && am.shape3[0] != X.n) || (am.shape3[1] != -1 && am.shape3[1] != 0 && am.shape3[1] != X.w) || (am.shape3[2] != -1 && am.shape3[2] != D))
        miss("the last Reshape is not to [N, L, H * hd]");
    if (am.shape3[1] == -1 && am.shape3[2] == -1) miss("the last Reshape is not to [N, L, H * hd]");
    // the cache outputs: one kv_append node each for K and V, in front of the attention node (EmitSteps makes one step of the pair)
    int pres[2] = {-1, -1}, pos_val = -1;
    if (am.rope && !am.rope_pos.empty()) pos_val = L.get_val(am.rope_pos);
    if (pos_val >= 0 && L.vals[pos_val].c != X.w) {
        if (X.w == 1) fail(am.rope_pos_miss);      // (a decode step: the refusal of the match, word for word)
        miss("the position ids " + am.rope_pos + " of the rope table are [" + std::to_string(L.vals[pos_val].n) + ", " + std::to_string(L.vals[pos_val].c) + "]; a step with a past and Lq = " + std::to_string(X.w) +
             " new tokens takes an INT64 graph input [N, Lq] = [" + std::to_string(X.n) + ", " + std::to_string(X.w) + "], every token's own table row");
    }
    if (!am.present_k.empty()) {
        for (int which = 0; which < 2; ++which) {
            LNode a;
            a.kind = L_KVAPPEND;
            a.name = am.name + (which ? "/kv_append_v" : "/kv_append_k");
            a.in = {x};
            a.heads = int(am.heads);
            a.head_dim = int(am.head_dim);
            a.kv_heads = int(Hkv);
            a.kv_v = which == 1;
            a.past_len = int(P);
            if (decode) { a.past_in = int(a.in.size()); a.in.push_back(L.get_val(which ? am.past_v : am.past_k)); }
            if (which == 0 && am.rope) {
                a.w = am.rope_cos;
                a.w2 = am.rope_sin;
                a.rope_rows = am.rope_rows;
                if (pos_val >= 0) { a.pos_in = int(a.in.size()); a.in.push_back(pos_val); }
            }
            push_node(std::move(a), which ? am.present_v : am.present_k, {X.n, Hkv, Lk, am.head_dim}, false);
            pres[which] = L.get_val(which ? am.present_v : am.present_k);
        }
    }
    LNode n;
    n.kind = L_ATTENTION;
    n.name = am.name;
    n.in = {x};
    n.heads = int(am.heads);
    n.head_dim = int(am.head_dim);
    n.attn_scale = am.scale;
    if (!am.mask.empty()) {
        const int mv = L.get_val(am.mask);
        if (decode && X.w > 1 && (L.vals[mv].n != X.n || L.vals[mv].c != Lk))
            miss("the key mask " + am.mask + " is [" + std::to_string(L.vals[mv].n) + ", " + std::to_string(L.vals[mv].c) + "]; its width must be P + Lq = " + std::to_string(Lk) + " (the " + std::to_string(P) +
                 " cached rows and the " + std::to_string(X.w) + " new keys) for [N = " + std::to_string(X.n) + "] images");
        if (decode && (L.vals[mv].n != X.n || L.vals[mv].c != Lk))
            miss("the key mask " + am.mask + " is [" + std::to_string(L.vals[mv].n) + ", " + std::to_string(L.vals[mv].c) + "]; its width must be P + 1 = " + std::to_string(Lk) + " (the " + std::to_string(P) +
                 " cached rows and the new key) for [N = " + std::to_string(X.n) + "] images");
        if (!decode && (L.vals[mv].n != X.n || L.vals[mv].c != X.w))
            miss("the key mask " + am.mask + " is [" + std::to_string(L.vals[mv].n) + ", " + std::to_string(L.vals[mv].c) + "], the tokens [" + std::to_string(X.n) + ", " + std::to_string(X.w) + ", .]");
        n.in.push_back(mv);
        n.key_mask = true;
        n.mask_value = am.mask_value;
    }
    n.kv_heads = int(Hkv);
    if (am.rope) {
        if (!am.mask.empty() && !decode) miss("a rotary embedding (Add " + am.rope_name + ") together with a key mask (attention_mask) is not supported");
        if (am.rope_pos.empty() && am.rope_rows != X.w)      // (run-time positions: the whole [max_pos, hd] table, any number of rows)
            miss("the rope tables (Add " + am.rope_name + ") have " + std::to_string(am.rope_rows) + " rows after slicing, the sequence has " + std::to_string(X.w) + " tokens (table rows != L)");
        n.w = am.rope_cos;
        n.w2 = am.rope_sin;
        n.rope_rows = am.rope_rows;
    }
    if (decode) {
        n.past_len = int(P);
        n.chunk_causal = X.w > 1;
        n.present_in = int(n.in.size());
        n.in.push_back(pres[0]);
        n.in.push_back(pres[1]);
        if (pos_val >= 0) { n.pos_in = int(n.in.size()); n.in.push_back(pos_val); }
    }
    if (am.causal) {
        if (am.causal_len != X.w) miss("its causal mask is [1, 1, " + std::to_string(am.causal_len) + ", " + std::to_string(am.causal_len) + "], the sequence has " + std::to_string(X.w) + " tokens");
        n.causal = true;
    }
    push_node(std::move(n), am.out, {X.n, D, 1, X.w}, true);
}

// ---- window attention: the shifted-window attention of a Swin export as ONE node on the unpermuted map -------------------------------
// Matched on the ONNX nodes, before the import and before MatchAttention, around every Softmax whose scores pass an Add of a constant and whose
// qkv tensor comes from a rank-6 window partition:
//   src [N,H,W,C] -> [Pad, all pads 0] -> [roll: per dim Concat(Slice(starts [s], ends [max]), Slice(starts [0], ends [s]))]
//   -> Reshape [N, H/wh, wh, W/ww, ww, C] -> Transpose [0,1,3,2,4,5] -> Reshape [N nW, L, C] -> [MatMul W -> Add b]                (the partition)
//   -> the attention of MatchAttentionCore with Add bias [1 | -, heads, L, L] behind the scaled scores and, in shifted blocks,
//      Reshape [N, nW, heads, L, L] -> Add mask [1 | -, nW, 1, L, L] -> Reshape [N nW, heads, L, L] in front of the Softmax
//   -> [MatMul Wp -> Add bp] -> Reshape [N, H/wh, W/ww, wh, ww, C] -> Transpose [0,1,3,2,4,5] -> Reshape [N, H, W, C]             (the reverse)
//   -> [roll back: the same with starts [-s] / ends [-s]] -> [Slice(starts [0,0], ends [H,W], axes [1,2]) of the padding]
// A Linear acts per token and commutes with the permutation of tokens, so the Linears stay ordinary nodes on the channels-last map: the last
// partition node renames src, the last reverse node renames the projection's result, and the attention node between them does the index arithmetic.
// A Softmax whose qkv tensor does not come from a rank-6 partition is left to MatchAttention (which refuses an additive mask by name).
void Planner::MatchWindowAttention() {
    IndexGraph();
    auto nm_of = [](const OnnxNode* p) { return p->name.empty() ? p->outputs[0] : p->name; };
    auto perm_is = [](const OnnxNode* p, std::vector<int64_t> want) { return p && p->op == "Transpose" && p->attr_ints("perm", {}) == want; };
    auto shape_of = [&](const OnnxNode* p, size_t rank) -> const OnnxTensor* {
        const OnnxTensor* t = p && p->op == "Reshape" && p->inputs.size() == 2 ? gi.cst(p->inputs[1]) : nullptr;
        return t && t->i.size() == rank ? t : nullptr;
    };
    // an Add / MatMul with exactly one constant operand: the index of the activation operand, else -1
    auto act_side = [&](const OnnxNode* p) { return !p || p->inputs.size() != 2 || (gi.cst(p->inputs[0]) != nullptr) == (gi.cst(p->inputs[1]) != nullptr) ? -1 : (gi.cst(p->inputs[0]) ? 1 : 0); };
    // a float constant, through Unsqueeze nodes of constants (the constant folds of the import reduce exactly these)
    std::function<bool(const std::string&, OnnxTensor&)> resolve = [&](const std::string& name, OnnxTensor& out) -> bool {
        if (const OnnxTensor* t = gi.cst(name)) { out = *t; return true; }
        const OnnxNode* p = gi.producer(name);
        if (!p || p->op != "Unsqueeze" || p->inputs.empty() || !resolve(p->inputs[0], out)) return false;
        std::vector<int64_t> ax = p->attr_ints("axes", {});
        if (ax.empty() && p->inputs.size() > 1) if (const OnnxTensor* at = gi.cst(p->inputs[1])) ax = at->i;
        if (ax.empty()) return false;
        const int64_t rank = int64_t(out.dims.size() + ax.size());
        for (auto& a : ax) if (a < 0) a += rank;
        std::sort(ax.begin(), ax.end());
        for (int64_t a : ax) { if (a < 0 || a > int64_t(out.dims.size())) return false; out.dims.insert(out.dims.begin() + a, 1); }
        return true;
    };
    for (const OnnxNode& sm : m.nodes) {
        if (sm.op != "Softmax" || sm.inputs.size() != 1 || sm.outputs.size() != 1) continue;
        const std::string nm = nm_of(&sm);
        const std::string prefix = "Softmax " + nm + ": the window-attention pattern around it does not match: ";
        auto miss = [&](const std::string& what) { fail(prefix + what); };
        // ---- is this a window attention at all?  (quietly: everything else is MatchAttention's) ----
        const OnnxNode* pv = nullptr;
        for (const OnnxNode& on : m.nodes)
            if (on.op == "MatMul" && on.inputs.size() == 2 && on.inputs[0] == sm.outputs[0] && !gi.cst(on.inputs[1])) pv = &on;
        if (!pv) continue;
        const OnnxNode *m4 = nullptr, *madd = nullptr, *m5 = nullptr;
        const OnnxNode* badd = gi.producer(sm.inputs[0]);
        if (badd && badd->op == "Reshape") {
            m4 = badd;
            madd = gi.producer(m4->inputs[0]);
            if (!madd || madd->op != "Add" || madd->inputs.size() != 2) continue;
            for (int k = 0; k < 2 && !m5; ++k)
                if (const OnnxNode* p = gi.producer(madd->inputs[size_t(k)]); p && p->op == "Reshape") m5 = p;
            if (!m5) continue;
            badd = gi.producer(m5->inputs[0]);
        }
        if (!badd || badd->op != "Add" || badd->inputs.size() != 2) continue;
        int bs = -1;
        for (int k = 0; k < 2; ++k) if (gi.act_matmul(gi.producer(gi.peel_quiet(badd->inputs[size_t(k)])))) bs = k;
        if (bs < 0) continue;
        const OnnxNode* rs = nullptr;
        {
            const OnnxNode* qk = gi.producer(gi.peel_quiet(badd->inputs[size_t(bs)]));
            const OnnxNode* g = gi.producer(gi.peel_quiet(qk->inputs[0]));
            if (g && g->op == "Squeeze" && !g->inputs.empty()) g = gi.producer(g->inputs[0]);
            const OnnxNode* tr = g && !g->inputs.empty() ? gi.producer(g->inputs[0]) : nullptr;
            rs = tr && tr->op == "Transpose" && !tr->inputs.empty() ? gi.producer(tr->inputs[0]) : nullptr;
        }
        if (!rs || rs->op != "Reshape" || rs->inputs.empty()) continue;
        const OnnxNode *qadd = nullptr, *qmm = nullptr;
        std::string part_out = rs->inputs[0];
        if (const OnnxNode* p = gi.producer(part_out); p && p->op == "Add" && act_side(p) >= 0)
            if (const OnnxNode* q = gi.producer(p->inputs[size_t(act_side(p))]); q && q->op == "MatMul" && act_side(q) == 0) { qadd = p; qmm = q; part_out = q->inputs[0]; }
        const OnnxNode* p3 = gi.producer(part_out);
        const OnnxNode* pt = p3 && p3->op == "Reshape" && !p3->inputs.empty() ? gi.producer(p3->inputs[0]) : nullptr;
        if (!pt || pt->op != "Transpose" || pt->attr_ints("perm", {}).size() != 6) continue;
        wattn_softmax.insert(&sm);

        // ---- the attention between the two Reshapes, the bias and the mask ----
        if (sm.attr_i("axis", -1) != -1 && sm.attr_i("axis", -1) != 3) miss("Softmax axis = " + std::to_string(sm.attr_i("axis", -1)) + " (only the last axis, -1 or 3, is an attention)");
        const AttnCore c = MatchAttentionCore(sm, pv, badd->inputs[size_t(bs)], prefix);
        if (c.rs != rs) miss("q, k and v do not come from one Reshape [N nW, L, 3, heads, hd]");
        std::set<const OnnxNode*> skip(c.taken.begin(), c.taken.end());
        skip.insert(c.orr);
        skip.insert(badd);
        auto one_reader = [&](const OnnxNode* p) {
            for (const std::string& o : p->outputs)
                if (gi.nreaders(o) != 1) miss("the intermediate " + o + " (" + p->op + " " + nm_of(p) + ") has " + std::to_string(gi.nreaders(o)) + " readers, not 1");
        };
        one_reader(badd);
        const OnnxTensor* s6 = shape_of(gi.producer(pt->inputs[0]), 6);
        const OnnxNode* p6 = gi.producer(pt->inputs[0]);
        if (!s6) miss("Transpose " + nm_of(pt) + " does not read Reshape(x, [N, H/wh, wh, W/ww, ww, C]) with a constant shape");
        if (!perm_is(pt, {0, 1, 3, 2, 4, 5})) miss("the partition Transpose " + nm_of(pt) + " does not have perm [0,1,3,2,4,5]");
        WinMatch wm;
        wm.nh = s6->i[1]; wm.wh = s6->i[2]; wm.nw = s6->i[3]; wm.ww = s6->i[4];
        if (wm.nh < 1 || wm.wh < 1 || wm.nw < 1 || wm.ww < 1) miss("the partition Reshape " + nm_of(p6) + " must give the window grid and the window as positive constants");
        const int64_t L = wm.wh * wm.ww, nW = wm.nh * wm.nw;
        wm.heads = c.shape5[3];
        wm.head_dim = c.shape5[4];
        wm.scale = c.scale;
        const OnnxTensor* s3p = shape_of(p3, 3);
        if (!s3p || s3p->i[1] != L) miss("Reshape " + nm_of(p3) + " is not to [N nW, L, C] with L = wh ww = " + std::to_string(L));
        if (c.shape5[1] != L && c.shape5[1] != 0 && c.shape5[1] != -1) miss("Reshape " + nm_of(rs) + " is not to [N nW, L, 3, heads, hd] with L = " + std::to_string(L));
        if (c.shape3[1] != L && c.shape3[1] != 0 && c.shape3[1] != -1) miss("Reshape " + nm_of(c.orr) + " is not to [N nW, L, D] with L = " + std::to_string(L));
        for (const OnnxNode* p : {p6, pt, p3}) { one_reader(p); skip.insert(p); }
        if (qmm) { one_reader(qmm); one_reader(qadd); }
        // the bias: a constant [1 | -, heads, L, L]
        {
            const OnnxTensor* b = gi.cst(badd->inputs[size_t(1 - bs)]);
            if (!b || b->f.empty()) miss("Add " + nm_of(badd) + ": the relative-position bias must be a floating-point constant");
            std::vector<int64_t> d = b->dims;
            if (d.size() == 4 && d[0] == 1) d.erase(d.begin());
            if (d.size() != 3 || d[0] != wm.heads || d[1] != L || d[2] != L)
                miss("Add " + nm_of(badd) + ": the relative-position bias must have the shape [1, heads, L, L] = [1, " + std::to_string(wm.heads) + ", " + std::to_string(L) + ", " + std::to_string(L) + "]");
            wm.bias = b->f;
        }
        if (m4) {
            const OnnxTensor *s5m = shape_of(m5, 5), *s4m = shape_of(m4, 4);
            if (!s5m || s5m->i[1] != nW || s5m->i[2] != wm.heads || s5m->i[3] != L || s5m->i[4] != L)
                miss("Reshape " + nm_of(m5) + " in front of the mask is not to [N, nW, heads, L, L] with nW = " + std::to_string(nW));
            if (!s4m || s4m->i[1] != wm.heads || s4m->i[2] != L || s4m->i[3] != L) miss("Reshape " + nm_of(m4) + " behind the mask is not to [N nW, heads, L, L]");
            const int ms = gi.producer(madd->inputs[0]) == m5 ? 1 : 0;
            OnnxTensor mk;
            if (!resolve(madd->inputs[size_t(ms)], mk) || mk.f.empty())
                miss("Add " + nm_of(madd) + ": the shift mask does not reduce to a floating-point constant");
            std::vector<int64_t> d = mk.dims;
            while (d.size() > 4 && d[0] == 1) d.erase(d.begin());
            if (d.size() != 4 || d[2] != L || d[3] != L) miss("Add " + nm_of(madd) + ": the shift mask must have the shape [1, nW, 1, L, L] with L = " + std::to_string(L));
            if (d[1] != 1) miss("Add " + nm_of(madd) + ": the shift mask must broadcast along the head axis ([1, nW, 1, L, L]), not hold " + std::to_string(d[1]) + " heads");
            if (d[0] != nW) miss("Add " + nm_of(madd) + ": the shift mask holds " + std::to_string(d[0]) + " windows, the partition " + std::to_string(nW));
            wm.mask = mk.f;
            wm.masked = true;
            for (const OnnxNode* p : {m5, madd, m4}) { one_reader(p); skip.insert(p); }
        }

        // ---- a roll: Concat(axis d) of Slice(x, [s], [max], [d]) and Slice(x, [0], [s], [d]); false: `name` is not made by a Concat of two Slices ----
        struct Roll { std::string src; int64_t axis = 0, shift = 0; const OnnxNode *cat = nullptr, *a = nullptr, *b = nullptr; };
        auto parse_roll = [&](const std::string& name, Roll& r) -> bool {
            const OnnxNode* cat = gi.producer(name);
            if (!cat || cat->op != "Concat" || cat->inputs.size() != 2) return false;
            const OnnxNode *a = gi.producer(cat->inputs[0]), *b = gi.producer(cat->inputs[1]);
            if (!a || !b || a->op != "Slice" || b->op != "Slice") return false;
            auto bad = [&](const std::string& what) { miss("Concat " + nm_of(cat) + " is not a roll of the map: " + what); };
            auto one = [&](const OnnxNode* sl, size_t k, int64_t& v) {
                const OnnxTensor* t = sl->inputs.size() > k ? gi.cst(sl->inputs[k]) : nullptr;
                if (!t || t->i.size() != 1) bad("Slice " + nm_of(sl) + " must have one constant start, end and axis");
                v = t->i[0];
            };
            int64_t as, ae, aa, bs_, be, ba;
            one(a, 1, as); one(a, 2, ae); one(a, 3, aa); one(b, 1, bs_); one(b, 2, be); one(b, 3, ba);
            for (const OnnxNode* sl : {a, b})
                if (sl->inputs.size() > 4 && !sl->inputs[4].empty()) { int64_t st; one(sl, 4, st); if (st != 1) bad("Slice " + nm_of(sl) + " has a step"); }
            int64_t ax = cat->attr_i("axis", 0);
            if (ax < 0) ax += 4;
            if (aa < 0) aa += 4;
            if (ba < 0) ba += 4;
            if (a->inputs[0] != b->inputs[0]) bad("its two Slices read different values");
            if (aa != ax || ba != ax) bad("the Slices' axes " + std::to_string(aa) + ", " + std::to_string(ba) + " differ from the Concat's axis " + std::to_string(ax));
            if (ax != 1 && ax != 2) bad("only the axes 1 (H) and 2 (W) of the [N, H, W, C] map roll, not axis " + std::to_string(ax));
            if (bs_ != 0 || be != as || as == 0 || ae < (int64_t(1) << 31) - 1) bad("its Slices must be [s:] and [:s] of one axis");
            if (gi.nreaders(cat->inputs[0]) != 1 || gi.nreaders(cat->inputs[1]) != 1) bad("a Slice result has a second reader");
            r.src = a->inputs[0]; r.axis = ax; r.shift = as; r.cat = cat; r.a = a; r.b = b;
            return true;
        };
        // ---- above the partition: the roll, the zero Pad ----
        int64_t fsh[3] = {0, 0, 0};
        std::string cur = p6->inputs[0];
        bool padded = false;
        {
            Roll r;
            int need = 1;
            for (int k = 0; k < 2 && parse_roll(cur, r); ++k) {
                if (gi.nreaders(cur) != need) miss("the intermediate " + cur + " has " + std::to_string(gi.nreaders(cur)) + " readers, not " + std::to_string(need));
                if (fsh[r.axis] != 0) miss("Concat " + nm_of(r.cat) + " rolls axis " + std::to_string(r.axis) + " a second time");
                if (r.shift < 0) miss("Concat " + nm_of(r.cat) + " rolls the map forward (by " + std::to_string(-r.shift) + ") in front of the partition; torchvision rolls by -shift there");
                fsh[r.axis] = r.shift;
                for (const OnnxNode* p : {r.cat, r.a, r.b}) skip.insert(p);
                cur = r.src;
                need = 2;
            }
            if (const OnnxNode* pd = gi.producer(cur); pd && pd->op == "Pad") {
                if (gi.nreaders(cur) != need) miss("the intermediate " + cur + " has " + std::to_string(gi.nreaders(cur)) + " readers, not " + std::to_string(need));
                const OnnxTensor* pads = pd->inputs.size() > 1 ? gi.cst(pd->inputs[1]) : nullptr;
                bool zero = pads && !pads->i.empty();
                if (pads) for (int64_t v : pads->i) zero = zero && v == 0;
                if (!zero) miss("Pad " + nm_of(pd) + ": a non-zero window padding is not supported (the map extents must be multiples of the window, all pads 0)");
                skip.insert(pd);
                padded = true;
                cur = pd->inputs[0];
            }
        }
        const std::string src = cur;
        wm.sh = fsh[1];
        wm.sw = fsh[2];
        if (wm.sh >= wm.wh || wm.sw >= wm.ww)
            miss("the shift " + std::to_string(wm.sh) + " x " + std::to_string(wm.sw) + " is not smaller than the window " + std::to_string(wm.wh) + " x " + std::to_string(wm.ww));
        const bool rolled = wm.sh != 0 || wm.sw != 0;
        if (rolled && !wm.masked) miss("the map is rolled (by " + std::to_string(wm.sh) + " x " + std::to_string(wm.sw) + ") but no shift mask is added to the scores");
        if (!rolled && wm.masked) miss("a shift mask (Add " + nm_of(madd) + ") is added to the scores but the map is not rolled");

        // ---- behind the attention: [the projection Linear], the reverse, the roll back, the crop of the padding ----
        std::string tail = c.orr->outputs[0];
        auto reader_or_miss = [&](const std::string& name, const char* what) -> const OnnxNode* {
            const OnnxNode* r = gi.only_reader(name);
            if (!r) miss("the intermediate " + name + " has " + std::to_string(gi.nreaders(name)) + " readers, not 1 (" + what + ")");
            return r;
        };
        const OnnxNode* r6 = reader_or_miss(tail, "the attention's result");
        if (r6->op == "MatMul" && act_side(r6) == 0) {
            const OnnxNode* pa = reader_or_miss(r6->outputs[0], "the projection MatMul");
            tail = r6->outputs[0];
            if (pa->op == "Add" && act_side(pa) >= 0) { tail = pa->outputs[0]; pa = reader_or_miss(tail, "the projection's bias Add"); }
            r6 = pa;
        }
        const OnnxTensor* s6r = shape_of(r6, 6);
        if (!s6r) miss("the result " + tail + " is not read by the reverse Reshape [N, H/wh, W/ww, wh, ww, C]");
        if (s6r->i[1] != wm.nh || s6r->i[2] != wm.nw || s6r->i[3] != wm.wh || s6r->i[4] != wm.ww)
            miss("Reshape " + nm_of(r6) + ": the reverse has the window grid " + std::to_string(s6r->i[1]) + " x " + std::to_string(s6r->i[2]) + " and the window " +
                 std::to_string(s6r->i[3]) + " x " + std::to_string(s6r->i[4]) + ", the partition " + std::to_string(wm.nh) + " x " + std::to_string(wm.nw) + " and " +
                 std::to_string(wm.wh) + " x " + std::to_string(wm.ww));
        const OnnxNode* rt = reader_or_miss(r6->outputs[0], "the reverse Reshape");
        if (!perm_is(rt, {0, 1, 3, 2, 4, 5})) miss("the reverse " + rt->op + " " + nm_of(rt) + " is not Transpose(perm [0,1,3,2,4,5]), the partition's");
        const OnnxNode* r4 = reader_or_miss(rt->outputs[0], "the reverse Transpose");
        const OnnxTensor* s4r = shape_of(r4, 4);
        if (!s4r || s4r->i[1] != wm.nh * wm.wh || s4r->i[2] != wm.nw * wm.ww) miss("the reverse does not end in Reshape [N, H, W, C] with H x W = " + std::to_string(wm.nh * wm.wh) + " x " + std::to_string(wm.nw * wm.ww));
        const OnnxNode* last = r4;
        int64_t bsh[3] = {0, 0, 0};
        for (int k = 0; k < 2; ++k) {
            const auto rd = gi.readers_of(last->outputs[0]);
            if (rd.size() != 2 || rd[0]->op != "Slice" || rd[1]->op != "Slice" || gi.nreaders(last->outputs[0]) != 2) break;
            const OnnxNode* cat = gi.only_reader(rd[0]->outputs[0]);
            Roll r;
            if (!cat || !parse_roll(cat->outputs[0], r) || r.src != last->outputs[0]) break;
            if (bsh[r.axis] != 0) miss("Concat " + nm_of(r.cat) + " rolls axis " + std::to_string(r.axis) + " back a second time");
            bsh[r.axis] = r.shift;
            for (const OnnxNode* p : {r.a, r.b, last}) skip.insert(p);
            last = r.cat;
        }
        for (int ax = 1; ax <= 2; ++ax)
            if (bsh[ax] != -fsh[ax])
                miss("the roll back does not undo the roll: axis " + std::to_string(ax) + " is rolled by " + std::to_string(-fsh[ax]) + " in front of the partition and by " +
                     std::to_string(-bsh[ax]) + " behind the reverse");
        if (padded) {
            const OnnxNode* cr = reader_or_miss(last->outputs[0], "the reversed map");
            const OnnxTensor *st = cr->op == "Slice" && cr->inputs.size() >= 4 ? gi.cst(cr->inputs[1]) : nullptr, *en = st ? gi.cst(cr->inputs[2]) : nullptr,
                             *ax = st ? gi.cst(cr->inputs[3]) : nullptr;
            if (!st || !en || !ax || st->i != std::vector<int64_t>{0, 0} || ax->i != std::vector<int64_t>{1, 2} || en->i.size() != 2 || en->i[0] < wm.nh * wm.wh ||
                en->i[1] < wm.nw * wm.ww || (cr->inputs.size() > 4 && !cr->inputs[4].empty()))
                miss("the padded map is not cropped by Slice(starts [0,0], ends [H,W], axes [1,2])");
            skip.insert(last);
            last = cr;
        }
        for (const OnnxNode* p : {r6, rt}) skip.insert(p);
        if (last != r4) skip.insert(r4);
        skip.erase(last);
        skip.erase(p3);
        wm.out = c.orr->outputs[0];
        wm.name = nm_of(rs) + "+" + nm + "+" + nm_of(c.orr);
        view_alias[p3] = src;
        view_alias[last] = r6->inputs[0];
        wattn_head[rs] = wm;
        skip.erase(rs);
        for (const OnnxNode* p : skip) wattn_skip.insert(p);
    }
}

void Planner::ImportWindowAttention(const OnnxNode& on, const WinMatch& wm) {
    auto miss = [&](const std::string& what) { fail("window attention " + wm.name + ": " + what); };
    if (!L.is_cl(on.inputs[0])) miss("its qkv input " + on.inputs[0] + " is not a channels-last view [N, H, W, 3 D]");
    const int x = in_val(on, 0);
    const Val X = L.vals[x];
    const int64_t D = wm.heads * wm.head_dim;
    if (X.c != 3 * D) miss("the qkv rows have " + std::to_string(X.c) + " columns, not 3 * heads * hd = " + std::to_string(3 * D));
    if (X.h % wm.wh || X.w % wm.ww)
        miss("the map " + std::to_string(X.h) + " x " + std::to_string(X.w) + " is no multiple of the window " + std::to_string(wm.wh) + " x " + std::to_string(wm.ww) +
             " (torchvision pads such a map; a non-zero window padding is not supported)");
    if (X.h != wm.nh * wm.wh || X.w != wm.nw * wm.ww)
        miss("the partition Reshape cuts a " + std::to_string(wm.nh * wm.wh) + " x " + std::to_string(wm.nw * wm.ww) + " map, the value is " + std::to_string(X.h) + " x " + std::to_string(X.w));
    LNode n;
    n.kind = L_WATTN;
    n.name = wm.name;
    n.in = {x};
    n.heads = int(wm.heads);
    n.head_dim = int(wm.head_dim);
    n.attn_scale = wm.scale;
    n.win_h = int(wm.wh); n.win_w = int(wm.ww); n.shift_h = int(wm.sh); n.shift_w = int(wm.sw);
    n.masked = wm.masked;
    n.w = wm.bias;
    n.w2 = wm.mask;
    push_node(std::move(n), wm.out, {X.n, D, X.h, X.w}, false);
    L.cl_names.insert(wm.out);
}

// ---- patch merging: Concat(axis -1) of x[:, a::2, b::2, :] for (a, b) = (0,0), (1,0), (0,1), (1,1), each two strided Slices ----------
void Planner::MatchPatchMerge() {
    IndexGraph();
    auto nm_of = [](const OnnxNode* p) { return p->name.empty() ? p->outputs[0] : p->name; };
    // Slice(x, starts [s], ends [>= 2^31 - 1], axes [axis], steps [2])
    auto strided = [&](const OnnxNode* sl, int64_t axis, int64_t& start) {
        if (!sl || sl->op != "Slice" || sl->inputs.size() != 5) return false;
        const OnnxTensor *st = gi.cst(sl->inputs[1]), *en = gi.cst(sl->inputs[2]), *ax = gi.cst(sl->inputs[3]), *sp = gi.cst(sl->inputs[4]);
        if (!st || !en || !ax || !sp || st->i.size() != 1 || en->i.size() != 1 || ax->i.size() != 1 || sp->i.size() != 1) return false;
        const int64_t a = ax->i[0] < 0 ? ax->i[0] + 4 : ax->i[0];
        if (a != axis || sp->i[0] != 2 || en->i[0] < (int64_t(1) << 31) - 1) return false;
        start = st->i[0];
        return true;
    };
    for (const OnnxNode& cat : m.nodes) {
        if (cat.op != "Concat" || cat.inputs.size() != 4) continue;
        const int64_t axis = cat.attr_i("axis", 1);
        if (axis != -1 && axis != 3) continue;
        std::string src;
        std::vector<const OnnxNode*> slices;
        bool all = true, any = false;
        int64_t ab[4][2];
        for (size_t k = 0; k < 4; ++k) {
            const OnnxNode* w = gi.producer(cat.inputs[k]);
            const OnnxNode* h = w && w->op == "Slice" && !w->inputs.empty() ? gi.producer(w->inputs[0]) : nullptr;
            const bool ok = strided(w, 2, ab[k][1]) && strided(h, 1, ab[k][0]) && (src.empty() || src == h->inputs[0]);
            all = all && ok;
            any = any || ok;
            if (!ok) continue;
            src = h->inputs[0];
            slices.push_back(w);
            slices.push_back(h);
        }
        if (!any) continue;
        const std::string nm = nm_of(&cat);
        if (!all) fail("Concat " + nm + ": a patch merging concatenates four x[:, a::2, b::2, :] slices (each Slice(axes [1], steps [2]) -> Slice(axes [2], steps [2])) of ONE map");
        static const int64_t want[4][2] = {{0, 0}, {1, 0}, {0, 1}, {1, 1}};
        for (size_t k = 0; k < 4; ++k)
            if (ab[k][0] != want[k][0] || ab[k][1] != want[k][1])
                fail("Concat " + nm + ": the slices of a patch merging must start at (0,0), (1,0), (0,1), (1,1) in this order (torchvision's x0, x1, x2, x3); operand " +
                     std::to_string(k) + " starts at (" + std::to_string(ab[k][0]) + "," + std::to_string(ab[k][1]) + ")");
        for (const OnnxNode* p : slices)
            if (gi.nreaders(p->outputs[0]) != 1) fail("Concat " + nm + ": the slice " + p->outputs[0] + " of the patch merging has a second reader");
        merge_head[&cat] = src;
        for (const OnnxNode* p : slices) wattn_skip.insert(p);
    }
}

void Planner::ImportPatchMerge(const OnnxNode& on, const std::string& src) {
    const std::string nm = on.name.empty() ? on.outputs[0] : on.name;
    if (!L.is_cl(src)) fail("Concat " + nm + ": the patch merging reads " + src + ", which is not a channels-last view [N, H, W, C]");
    const int x = L.get_val(src);
    const Val X = L.vals[x];
    if (X.h % 2 || X.w % 2)
        fail("Concat " + nm + ": patch merging of an odd map (" + std::to_string(X.h) + " x " + std::to_string(X.w) + ") is not supported (torchvision pads it: a non-zero padding)");
    LNode n;
    n.kind = L_PATCHMERGE;
    n.name = nm;
    n.in = {x};
    push_node(std::move(n), on.outputs[0], {X.n, 4 * X.c, X.h / 2, X.w / 2}, false);
    L.cl_names.insert(on.outputs[0]);
}

// ---- token assemble: the position-embedding Add directly behind the class-token concat, as its sole reader, folds into it ----
// ---- token embeddings: table Gathers by INT64 graph inputs, their sum and the LayerNormalization behind it as ONE node ----------------------
// Matched on the ONNX nodes, before the import (no Val ever holds an integer activation or a [N, L, D] sum of gathers):
//   e = Gather(word [V, D], ids, axis 0) [+ Gather(type [T, D], type_ids, axis 0)] [+ pos]  ->  LayerNormalization(e, axis -1)
// ids / type_ids INT64 graph inputs [N, L]; pos a floating-point constant [1, L, D] / [L, D], or Gather(table [P, D], position ids) with the ids a
// constant or a Slice of one (how exporters write BERT's position embedding); the Adds in any order, every partial sum read by the next node only.
// A near miss is refused naming what did not match.  Graphs without an INT64 [N, L] input are not looked at.
void Planner::MatchEmbed() {
    std::vector<std::string> id_inputs;
    for (const auto& vi : m.inputs) if (vi.elem_type == ONNX_INT64 && vi.dims.size() == 2) id_inputs.push_back(vi.name);
    if (id_inputs.empty()) return;
    IndexGraph();
    auto input_index = [&](const std::string& name) {
        for (size_t k = 0; k < id_inputs.size(); ++k) if (id_inputs[k] == name) return int(k);
        return -1;
    };
    auto float_const = [&](const std::string& name) -> const OnnxTensor* {
        const OnnxTensor* t = gi.cst(name);
        return t && !t->f.empty() && (t->dtype == ONNX_FLOAT || t->dtype == ONNX_DOUBLE || t->dtype == ONNX_FLOAT16) ? t : nullptr;
    };
    // Gather(floating-point constant, an activation): an embedding lookup, which must be the supported one
    auto table_gather = [&](const OnnxNode& g) {
        if (g.op != "Gather" || g.inputs.size() != 2 || !float_const(g.inputs[0]) || gi.cst(g.inputs[1])) return false;
        if (const OnnxNode* sl = gi.producer(g.inputs[1]); sl && sl->op == "Slice" && !sl->inputs.empty() && gi.cst(sl->inputs[0])) return false;      // constant position ids
        const std::string nm = g.name.empty() ? g.outputs[0] : g.name;
        if (input_index(g.inputs[1]) < 0)
            fail("Gather " + nm + ": the indices " + g.inputs[1] + " of an embedding table are not an INT64 graph input [N, L] (only a graph input may index a table)");
        const OnnxTensor* t = float_const(g.inputs[0]);
        if (t->dims.size() != 2)
            fail("Gather " + nm + ": the embedding table " + g.inputs[0] + " must be a 2-D floating-point initializer [V, D] (it has rank " + std::to_string(t->dims.size()) + ")");
        if (g.attr_i("axis", 0) != 0) fail("Gather " + nm + ": an embedding table is gathered along axis 0 (axis = " + std::to_string(g.attr_i("axis", 0)) + ")");
        return true;
    };
    auto ints_const = [&](const std::string& name, std::vector<int64_t>& out) {
        const OnnxTensor* t = name.empty() ? nullptr : gi.cst(name);
        if (!t || t->i.empty()) return false;
        out = t->i;
        return true;
    };
    for (const OnnxNode& g : m.nodes) {
        if (embed_skip.count(&g) || attn_skip.count(&g) || !table_gather(g)) continue;      // (attn_skip: a rope table gathered by position_ids)
        const std::string gname = g.name.empty() ? g.outputs[0] : g.name;
        // down to the LayerNormalization: Adds only, every value read once
        std::string cur = g.outputs[0];
        const OnnxNode* ln = nullptr;
        // A sum that is not read by one LayerNormalization alone (a pre-LN model: GPT-2's is read by ln_1 and by the residual Add) becomes an embed step
        // without the norm, headed by its last Add, where it is one table Gather plus position rows; any other such sum keeps `refusal`
        std::string refusal;
        for (;;) {
            const OnnxNode* r = gi.only_reader(cur);
            if (!r) refusal = "Gather " + gname + ": " + cur + " has " + std::to_string(gi.nreaders(cur)) + " readers; the sum of the embedding gathers is read by its LayerNormalization alone, every partial sum by the next Add alone";
            else if (r->op == "Add") { cur = r->outputs[0]; continue; }
            else if (r->op == "LayerNormalization" && r->inputs[0] == cur) { ln = r; break; }
            else refusal = r->op + " " + (r->name.empty() ? r->outputs[0] : r->name) + ": reads the embedding sum " + cur + "; only Adds and then a LayerNormalization may (the embedding and its LayerNormalization run as one step)";
            // (a Llama-class model has no position rows: the Gather itself is the value its first RMSNorm and the residual Add read, and heads the step)
            const OnnxNode* last = gi.producer(cur);
            if (cur == g.outputs[0] && !r) last = &g;      // (several readers: a sole reader that is neither an Add nor a LayerNormalization keeps its refusal)
            else if (cur == g.outputs[0] || !last || last->op != "Add") fail(refusal);
            ln = last;
            break;
        }
        if (embed_head.count(ln)) continue;
        const std::string lname = ln->name.empty() ? ln->outputs[0] : ln->name;
        EmbedMatch em;
        em.sum_only = !refusal.empty();
        const std::string who = (ln == &g ? "Gather " : em.sum_only ? "Add " : "LayerNormalization ") + lname;
        std::vector<const OnnxNode*> gathers, taken;
        int pos_count = 0;
        int64_t Lq = 0;
        for (size_t i = 0; i < m.inputs.size(); ++i) if (m.inputs[i].name == g.inputs[1]) Lq = input_shapes[i].size() == 2 ? input_shapes[i][1] : 0;
        auto add_pos = [&](const std::vector<float>& f, const std::vector<int64_t>& dims, const std::string& what) {
            const bool ok = (dims.size() == 3 && dims[0] == 1 && dims[1] == Lq) || (dims.size() == 2 && dims[0] == Lq);
            if (!ok || f.empty()) fail(who + ": " + what + " of the embedding sum must be a floating-point constant [1, L, D] or [L, D] with L = " + std::to_string(Lq));
            if (++pos_count > 1) fail(who + ": the embedding sum has more than one constant operand (" + what + ")");
            em.pos = f;
        };
        std::function<void(const std::string&)> walk = [&](const std::string& name) {
            const OnnxNode* p = gi.producer(name);
            if (p && p->op == "Add" && p->inputs.size() == 2 && !(gi.cst(p->inputs[0]) && gi.cst(p->inputs[1]))) {
                if (gi.nreaders(name) != 1 && !(em.sum_only && p == ln))
                    fail("Add " + (p->name.empty() ? name : p->name) + ": the embedding sum " + name + " has a second reader in front of its LayerNormalization");
                taken.push_back(p);
                walk(p->inputs[0]);
                walk(p->inputs[1]);
                return;
            }
            if (const OnnxTensor* c = gi.cst(name)) {
                if (!float_const(name)) fail(who + ": the constant " + name + " of the embedding sum is not floating-point");
                add_pos(c->f, c->dims, "the constant " + name);
                return;
            }
            if (p && table_gather(*p)) {
                if (gi.nreaders(name) != 1 && p != ln) fail("Gather " + (p->name.empty() ? name : p->name) + ": " + name + " has " + std::to_string(gi.nreaders(name)) + " readers; an embedding gather is read by its sum alone");
                gathers.push_back(p);
                return;
            }
            // the position embedding as exporters write it: Gather(table [P, D], position ids), the ids a constant or a Slice (step 1, last axis) of one
            if (p && p->op == "Gather" && p->inputs.size() == 2 && float_const(p->inputs[0]) && p->attr_i("axis", 0) == 0 && gi.nreaders(name) == 1) {
                const OnnxTensor* tab = float_const(p->inputs[0]);
                std::vector<int64_t> ix;
                const OnnxNode* sl = gi.producer(p->inputs[1]);
                bool ok = tab->dims.size() == 2 && ints_const(p->inputs[1], ix);
                if (!ok && tab->dims.size() == 2 && sl && sl->op == "Slice" && sl->inputs.size() >= 3 && gi.nreaders(p->inputs[1]) == 1) {
                    std::vector<int64_t> src, st, en, ax = {0}, stp = {1};
                    const OnnxTensor* srct = gi.cst(sl->inputs[0]);
                    ok = srct && ints_const(sl->inputs[0], src) && ints_const(sl->inputs[1], st) && ints_const(sl->inputs[2], en) && st.size() == 1 && en.size() == 1;
                    if (ok && sl->inputs.size() > 3 && !sl->inputs[3].empty()) ok = ints_const(sl->inputs[3], ax) && ax.size() == 1;
                    if (ok && sl->inputs.size() > 4 && !sl->inputs[4].empty()) ok = ints_const(sl->inputs[4], stp) && stp.size() == 1;
                    if (ok) {
                        const int64_t rank = int64_t(srct->dims.size()), P = int64_t(src.size());
                        const int64_t axis = ax[0] < 0 ? ax[0] + rank : ax[0];
                        ok = rank >= 1 && rank <= 2 && axis == rank - 1 && srct->dims[size_t(rank - 1)] == P && stp[0] == 1;
                        if (ok) {
                            const int64_t b = std::clamp<int64_t>(st[0] < 0 ? st[0] + P : st[0], 0, P), e = std::clamp<int64_t>(en[0] < 0 ? en[0] + P : en[0], b, P);
                            ix.assign(src.begin() + b, src.begin() + e);
                            taken.push_back(sl);
                        }
                    }
                }
                if (ok && int64_t(ix.size()) == Lq) {
                    const int64_t P = tab->dims[0], D = tab->dims[1];
                    std::vector<float> f(size_t(Lq * D));
                    for (int64_t l = 0; l < Lq; ++l) {
                        const int64_t r = ix[size_t(l)] < 0 ? ix[size_t(l)] + P : ix[size_t(l)];
                        if (r < 0 || r >= P) fail("Gather " + (p->name.empty() ? name : p->name) + ": position id " + std::to_string(ix[size_t(l)]) + " is outside the table of " + std::to_string(P) + " rows");
                        std::copy(tab->f.begin() + r * D, tab->f.begin() + (r + 1) * D, f.begin() + l * D);
                    }
                    taken.push_back(p);
                    add_pos(f, {Lq, D}, "the position Gather " + (p->name.empty() ? name : p->name));
                    return;
                }
            }
            fail(who + ": the operand " + name + " of the embedding sum is neither the Gather of a table [V, D] by an INT64 graph input nor a constant [1, L, D] "
                 "(nor the Gather of a table by constant position ids)");
        };
        walk(em.sum_only ? ln->outputs[0] : ln->inputs[0]);
        if (em.sum_only && (gathers.size() != 1 || pos_count != (ln == &g ? 0 : 1))) fail(refusal);
        if (gathers.empty() || gathers.size() > 2)
            fail(who + ": the embedding sum has " + std::to_string(gathers.size()) + " table Gathers by graph inputs (one or two are supported)");
        std::sort(gathers.begin(), gathers.end(), [&](const OnnxNode* a, const OnnxNode* b) { return input_index(a->inputs[1]) < input_index(b->inputs[1]); });
        if (gathers.size() == 2 && gathers[0]->inputs[1] == gathers[1]->inputs[1])
            fail(who + ": both table Gathers of the embedding sum read " + gathers[0]->inputs[1] + " (two different INT64 graph inputs are expected)");
        for (const OnnxNode* t : gathers) {
            const OnnxTensor* tab = float_const(t->inputs[0]);
            if (tab->dims[1] != float_const(gathers[0]->inputs[0])->dims[1] || (pos_count && int64_t(em.pos.size()) != Lq * tab->dims[1]))
                fail(who + ": the tables and the position rows of the embedding sum differ in width");
            em.ids.push_back(t->inputs[1]);
            em.tables.push_back(tab);
            em.names += (em.names.empty() ? "" : "+") + (t->name.empty() ? t->outputs[0] : t->name);
            if (t != ln) embed_skip.insert(t);
        }
        for (const OnnxNode* t : taken) if (t != ln) embed_skip.insert(t);
        embed_head[ln] = std::move(em);
    }
    // whatever else reads an id input is refused by name
    for (const std::string& in : id_inputs) {
        for (const auto& vo : m.outputs) if (vo.name == in) fail("graph output " + in + " is an INT64 graph input; only the Gather of an embedding table may read one");
        for (const OnnxNode* r : gi.readers_of(in))
            if (mask_nodes.count(r)) continue;             // the key mask of the attentions (MatchAttention took its chain)
            else if ((!embed_skip.count(r) && !embed_head.count(r)) || r->op != "Gather")
                fail(r->op + " " + (r->name.empty() ? r->outputs[0] : r->name) + ": reads the INT64 graph input " + in + "; only the Gather (axis 0) of a floating-point embedding table [V, D] may read one");
    }
}

void Planner::ImportEmbed(const OnnxNode& on, const EmbedMatch& em) {
    LNode n;
    n.kind = L_EMBED;
    n.name = on.name.empty() ? on.outputs[0] : on.name;
    for (const std::string& id : em.ids) n.in.push_back(L.get_val(id));
    const Val& I = L.vals[n.in[0]];
    for (int v : n.in)
        if (L.vals[v].dims != I.dims) fail("LayerNormalization " + n.name + ": the id inputs of the embedding sum differ in shape");
    const int64_t N = I.n, Lq = I.c, D = em.tables[0]->dims[1];
    if (em.sum_only) {
        // `on` is the sum's last Add: no norm behind it, the step writes the sum (gamma absent)
        n.w = em.tables[0]->f;
        n.emb_vocab = em.tables[0]->dims[0];
        n.bias = em.pos;
        if (n.emb_vocab < 1 || n.emb_vocab >= (int64_t(1) << 31) || D < 1 || D >= (int64_t(1) << 31)) fail("Add " + n.name + ": embedding table sizes out of range");
        n.name = on.op == "Gather" ? em.names : em.names + "+" + n.name;      // (a Gather that heads its own step is its only node)
        push_node(std::move(n), on.outputs[0], {N, D, 1, Lq}, true);
        return;
    }
    const int64_t axis = on.attr_i("axis", -1);
    if (axis != -1 && axis != 2) fail("LayerNormalization " + n.name + ": axis = " + std::to_string(axis) + " on a token view is not supported (only the channel axis alone is normalised: the last axis of a channels-last view or of an [N, C] value)");
    if (on.attr_i("stash_type", 1) != 1) fail("LayerNormalization " + n.name + ": stash_type = " + std::to_string(on.attr_i("stash_type", 1)) + " is not supported (1 is)");
    for (size_t k = 1; k < on.outputs.size(); ++k)
        if (!on.outputs[k].empty()) fail("LayerNormalization " + n.name + ": the Mean / InvStdDev outputs are not supported");
    const OnnxTensor* g = on.inputs.size() > 1 ? L.init(on.inputs[1]) : nullptr;
    if (!g || g->dims.size() != 1 || g->numel() != D) fail("LayerNormalization " + n.name + ": scale must be a [C] initializer");
    n.s = g->f;
    if (on.inputs.size() > 2 && !on.inputs[2].empty()) {
        const OnnxTensor* b = L.init(on.inputs[2]);
        if (!b || b->dims.size() != 1 || b->numel() != D) fail("LayerNormalization " + n.name + ": B must be a [C] initializer");
        n.t = b->f;
    }
    n.eps = on.attr_f("epsilon", 1e-5f);
    n.w = em.tables[0]->f;
    n.emb_vocab = em.tables[0]->dims[0];
    if (em.tables.size() > 1) { n.w2 = em.tables[1]->f; n.emb_types = em.tables[1]->dims[0]; }
    n.bias = em.pos;
    if (n.emb_vocab < 1 || n.emb_vocab >= (int64_t(1) << 31) || n.emb_types >= (int64_t(1) << 31) || D < 1 || D >= (int64_t(1) << 31))
        fail("LayerNormalization " + n.name + ": embedding table sizes out of range");
    n.name = em.names + "+" + n.name;
    push_node(std::move(n), on.outputs[0], {N, D, 1, Lq}, true);
}

// ---- group norm: every spelling of a GroupNorm as ONE node ---------------------------------------------------------------------------------
// Matched on the ONNX nodes, before the import (the [N, G, -1] value in the middle is no feature map):
//   a) Reshape(x, [0, G, -1]) -> InstanceNormalization(scale [G], B [G]) -> Reshape(constant | Shape(x)) [-> Mul(gamma)] [-> Add(beta)]   (torch below opset 18)
//   b) GroupNormalization(x, scale, bias; num_groups, epsilon)       scale / bias [G] below opset 21, [C] from it on
//   c) InstanceNormalization directly on a map: G = C
// The matcher takes the structure and the reader counts; ImportGroupNorm, which knows x's shape, checks the shapes.  A near miss is refused naming
// the node and what did not match.
void Planner::MatchGroupNorm() {
    bool any = false;
    for (const OnnxNode& on : m.nodes) any = any || on.op == "InstanceNormalization" || on.op == "GroupNormalization";
    if (!any) return;
    IndexGraph();
    auto nm = [](const OnnxNode& o) { return o.name.empty() ? o.outputs[0] : o.name; };
    // the constant operand of a two-operand node with exactly one; act = the index of the other
    auto const_operand = [&](const OnnxNode& o, int& act) -> const OnnxTensor* {
        if (o.inputs.size() != 2) return nullptr;
        const OnnxTensor *c0 = gi.cst(o.inputs[0]), *c1 = gi.cst(o.inputs[1]);
        if ((c0 != nullptr) == (c1 != nullptr)) return nullptr;
        act = c0 ? 1 : 0;
        return c0 ? c0 : c1;
    };
    for (const OnnxNode& on : m.nodes) {
        if (on.op != "InstanceNormalization" && on.op != "GroupNormalization") continue;
        GnMatch gm;
        gm.name = gm.in_name = nm(on);
        const std::string who = on.op + " " + gm.in_name;
        if (on.inputs.size() != 3 || on.outputs.size() != 1) fail(who + ": expected the inputs x, scale, bias and one output");
        gm.scale = gi.cst(on.inputs[1]);
        gm.bias = gi.cst(on.inputs[2]);
        if (!gm.scale || !gm.bias || gm.scale->f.empty() || gm.bias->f.empty()) fail(who + ": scale and bias must be floating-point constants");
        gm.eps = on.attr_f("epsilon", 1e-5f);
        gm.x = on.inputs[0];
        gm.out = on.outputs[0];
        if (on.op == "GroupNormalization") {
            gm.form = 'b';
            gm.groups = on.attr_i("num_groups", 0);
            if (gm.groups < 1) fail(who + ": num_groups must be positive");
            if (on.attr_i("stash_type", 1) != 1) fail(who + ": stash_type = " + std::to_string(on.attr_i("stash_type", 1)) + " is not supported (1 is)");
            gn_head[&on] = gm;
            continue;
        }
        const OnnxNode* r1 = gi.producer(on.inputs[0]);
        const OnnxTensor* shp1 = r1 && r1->op == "Reshape" && r1->inputs.size() == 2 ? gi.cst(r1->inputs[1]) : nullptr;
        if (!shp1 || shp1->i.size() != 3) {          // directly on a map
            gm.form = 'c';
            gn_head[&on] = gm;
            continue;
        }
        const std::string prefix = who + ": the group-norm pattern around it does not match: ";
        auto one_reader = [&](const std::string& name) {
            if (gi.nreaders(name) != 1) fail(prefix + "the intermediate value " + name + " has " + std::to_string(gi.nreaders(name)) + " readers, not 1");
        };
        gm.form = 'a';
        gm.shape1 = shp1->i;
        gm.groups = gm.shape1[1];
        gm.x = r1->inputs[0];
        one_reader(r1->outputs[0]);
        one_reader(on.outputs[0]);
        const OnnxNode* r2 = gi.only_reader(on.outputs[0]);
        if (!r2 || r2->op != "Reshape" || r2->inputs.size() != 2 || r2->inputs[0] != on.outputs[0])
            fail(prefix + "a Reshape back to the input's shape must read " + on.outputs[0]);
        std::vector<const OnnxNode*> taken = {r1, &on, r2};
        if (const OnnxTensor* b = gi.cst(r2->inputs[1])) {
            gm.back = b->i;
            if (gm.back.empty()) fail(prefix + "the shape of Reshape " + nm(*r2) + " must be an integer constant or Shape(" + gm.x + ")");
        } else {
            const OnnxNode* sh = gi.producer(r2->inputs[1]);
            if (!sh || sh->op != "Shape" || sh->inputs.size() != 1 || sh->inputs[0] != gm.x || sh->attrs.count("start") || sh->attrs.count("end"))
                fail(prefix + "the shape of Reshape " + nm(*r2) + " must be an integer constant or Shape(" + gm.x + ")");
            one_reader(sh->outputs[0]);
            taken.push_back(sh);
        }
        // Mul(gamma) and Add(beta) behind it, either operand order; a missing one is gamma 1 / beta 0
        const OnnxNode* last = r2;
        auto affine = [&](const char* op, const OnnxTensor*& c, std::string& cname) {
            const std::string& o = last->outputs[0];
            const OnnxNode* hit = nullptr;
            int act = 0;
            for (const OnnxNode* r : gi.readers_of(o))
                if (r->op == op && const_operand(*r, act) && r->inputs[size_t(act)] == o) hit = r;
            if (!hit) return;
            one_reader(o);
            c = const_operand(*hit, act);
            cname = hit->inputs[size_t(1 - act)];
            taken.push_back(hit);
            last = hit;
        };
        affine("Mul", gm.gamma, gm.gamma_name);
        affine("Add", gm.beta, gm.beta_name);
        gm.out = last->outputs[0];
        gm.name.clear();
        for (const OnnxNode* p : taken) if (p->op != "Shape") gm.name += (gm.name.empty() ? "" : "+") + nm(*p);
        for (const OnnxNode* p : taken) if (p != last) gn_skip.insert(p);
        gn_head[last] = gm;
    }
}

// ---- RMSNorm as exporters write it below opset 23 (HF's LlamaRMSNorm) ---------------------------------------------------------------------------
//   v = ReduceMean(Pow(x, 2) | Mul(x, x), axes [-1], keepdims 1);  y = Mul(weight [D], Mul(x, Reciprocal(Sqrt(Add(v, eps))) | Div(1, Sqrt(Add(v, eps)))))
// either operand order on every Mul / Add, the axes as an attribute or as an input, Cast(to = FLOAT) nodes anywhere in between (hidden_states.to(float32)
// exports as one; the values here are floats already, so they are names).  The match starts at a ReduceMean of a square; from there a node that is not
// the pattern's is refused by name.  A ReduceMean of anything else stays what it was, an unsupported operator.  The last Mul imports the whole as an
// RMSNormalization node over the ReduceMean's axis (ImportLayerNorm checks that it is the channel axis of x's view and that weight is [D])
void Planner::MatchRmsNorm() {
    bool any = false;
    for (const OnnxNode& on : m.nodes) any = any || on.op == "ReduceMean";
    if (!any) return;
    IndexGraph();
    auto nm = [](const OnnxNode& o) { return o.name.empty() ? o.outputs[0] : o.name; };
    auto float_cast = [](const OnnxNode* p) { return p && p->op == "Cast" && p->inputs.size() == 1 && p->attr_i("to", 0) == ONNX_FLOAT; };
    auto scalar = [&](const std::string& name, double& v) {
        const OnnxTensor* t = gi.cst(name);
        if (!t || t->numel() != 1 || (t->f.size() != 1 && t->i.size() != 1)) return false;
        v = t->f.size() == 1 ? double(t->f[0]) : double(t->i[0]);
        return true;
    };
    for (const OnnxNode& rm : m.nodes) {
        if (rm.op != "ReduceMean" || rm.inputs.empty() || rm.outputs.size() != 1) continue;
        std::vector<const OnnxNode*> taken;
        // the name above a chain of Casts to FLOAT
        auto up = [&](std::string name) {
            for (const OnnxNode* p = gi.producer(name); float_cast(p); p = gi.producer(name)) { taken.push_back(p); name = p->inputs[0]; }
            return name;
        };
        const OnnxNode* sq = gi.producer(up(rm.inputs[0]));
        if (!sq || sq->inputs.size() != 2) continue;
        double e = 0.0;
        std::string x;
        if (sq->op == "Pow" && scalar(sq->inputs[1], e) && e == 2.0) x = up(sq->inputs[0]);
        else if (sq->op == "Mul" && up(sq->inputs[0]) == up(sq->inputs[1])) x = up(sq->inputs[0]);
        else continue;
        if (gi.cst(x)) continue;
        taken.insert(taken.end(), {sq, &rm});
        const std::string prefix = "ReduceMean " + nm(rm) + ": the RMSNorm pattern around it does not match: ";
        // the sole reader of a name, below a chain of Casts to FLOAT
        auto down = [&](std::string name) -> const OnnxNode* {
            for (;;) {
                const OnnxNode* r = gi.only_reader(name);
                if (!r) fail(prefix + "the intermediate value " + name + " has " + std::to_string(gi.nreaders(name)) + " readers, not 1");
                if (!float_cast(r)) return r;
                taken.push_back(r);
                name = r->outputs[0];
            }
        };
        // r reads `from` (below Casts) as one of its two operands: the index of the other one
        auto other = [&](const OnnxNode* r, const std::string& from) {
            if (r->inputs.size() != 2) return -1;
            for (int k = 0; k < 2; ++k) if (up(r->inputs[size_t(k)]) == from) return 1 - k;
            return -1;
        };
        std::vector<int64_t> axes = rm.attr_ints("axes", {});
        if (rm.inputs.size() > 1 && !rm.inputs[1].empty()) {
            const OnnxTensor* t = gi.cst(rm.inputs[1]);
            if (!t || t->i.empty()) fail(prefix + "the axes must be an integer constant");
            axes = t->i;
        }
        if (axes.size() != 1) fail(prefix + "the mean is taken over " + std::to_string(axes.size()) + " axes, not over the last one alone");
        if (rm.attr_i("keepdims", 1) != 1) fail(prefix + "keepdims must be 1");
        const OnnxNode* ad = down(rm.outputs[0]);
        int k = ad->op == "Add" ? other(ad, rm.outputs[0]) : -1;
        double eps = 0.0;
        if (k < 0 || !scalar(ad->inputs[size_t(k)], eps) || !(eps >= 0.0)) fail(prefix + ad->op + " " + nm(*ad) + " reads the mean; an Add of the scalar constant eps must");
        taken.push_back(ad);
        const OnnxNode* sr = down(ad->outputs[0]);
        if (sr->op != "Sqrt") fail(prefix + sr->op + " " + nm(*sr) + " reads the sum with eps; a Sqrt must");
        taken.push_back(sr);
        const OnnxNode* rc = down(sr->outputs[0]);
        double one = 0.0;
        const bool recip = (rc->op == "Reciprocal" && rc->inputs.size() == 1) ||
                           (rc->op == "Div" && rc->inputs.size() == 2 && up(rc->inputs[1]) == sr->outputs[0] && scalar(rc->inputs[0], one) && one == 1.0);
        if (!recip) fail(prefix + rc->op + " " + nm(*rc) + " reads the root; a Reciprocal or Div(1, root) must");
        taken.push_back(rc);
        const OnnxNode* mx = down(rc->outputs[0]);
        k = mx->op == "Mul" ? other(mx, rc->outputs[0]) : -1;
        if (k < 0 || up(mx->inputs[size_t(k)]) != x) fail(prefix + mx->op + " " + nm(*mx) + " reads the reciprocal root; a Mul with " + x + ", the value that was squared, must");
        taken.push_back(mx);
        const OnnxNode* mw = down(mx->outputs[0]);
        k = mw->op == "Mul" ? other(mw, mx->outputs[0]) : -1;
        const OnnxTensor* w = k >= 0 ? gi.cst(mw->inputs[size_t(k)]) : nullptr;
        if (!w || w->f.empty() || w->dims.size() != 1) fail(prefix + mw->op + " " + nm(*mw) + " reads the normalised value; a Mul with the weight, a floating-point constant [D], must");
        // every taken node but the last Mul is read inside the pattern only (a Cast of x may feed the square and the product: both are taken)
        std::set<const OnnxNode*> inside(taken.begin(), taken.end());
        inside.insert(mw);
        for (const OnnxNode* p : taken)
            for (const OnnxNode* r : gi.readers_of(p->outputs[0]))
                if (!inside.count(r)) fail(prefix + "the intermediate value " + p->outputs[0] + " has a reader outside the pattern (" + r->op + " " + nm(*r) + ")");
        for (const auto& vo : m.outputs)
            for (const OnnxNode* p : taken) if (p->outputs[0] == vo.name) fail(prefix + "the intermediate value " + vo.name + " is a graph output");
        OnnxNode g;
        g.op = "RMSNormalization";
        for (const OnnxNode& on : m.nodes)      // (graph order)
            if (inside.count(&on) && on.op != "Cast") g.name += (g.name.empty() ? "" : "+") + nm(on);
        g.inputs = {x, mw->inputs[size_t(k)]};
        g.outputs = {mw->outputs[0]};
        OnnxAttr ax, ep;
        ax.name = "axis"; ax.i = axes[0];
        ep.name = "epsilon"; ep.f = float(eps);
        g.attrs["axis"] = ax;
        g.attrs["epsilon"] = ep;
        synth_nodes.push_back(std::move(g));
        for (const OnnxNode* p : taken) rms_skip.insert(p);
        rms_head[mw] = &synth_nodes.back();
    }
}

void Planner::ImportGroupNorm(const OnnxNode& on, const GnMatch& gm) {
    const std::string who = std::string(gm.form == 'b' ? "GroupNormalization " : "InstanceNormalization ") + gm.in_name;
    auto dstr = [](const std::vector<int64_t>& d) {
        std::string s = "[";
        for (size_t k = 0; k < d.size(); ++k) s += (k ? "," : "") + std::to_string(d[k]);
        return s + "]";
    };
    if (L.init(gm.x)) fail(who + ": constant input is not supported");
    if (L.is_tok(gm.x)) fail(who + ": input " + gm.x + " is a token view [N, L, D]; a group norm reads an NCHW feature map or its [N, C, H*W] reshape");
    if (L.is_cl(gm.x)) fail(who + ": input " + gm.x + " is a channels-last view (a Transpose with perm [0,2,3,1]); a group norm reads an NCHW feature map or its [N, C, H*W] reshape");
    const int v = L.get_val(gm.x);
    const Val X = L.vals[v];
    if (X.is_i64) fail(who + ": input " + gm.x + " is not a floating-point value");
    const bool flat = L.flat_names.count(gm.x) != 0, back = L.back_names.count(gm.x) != 0;
    const std::vector<int64_t> xd = flat ? std::vector<int64_t>{X.n, X.c, X.h * X.w} : back ? std::vector<int64_t>{X.n, X.c, X.w} : X.dims;
    if (xd.size() != 3 && xd.size() != 4) fail(who + ": an input of rank " + std::to_string(xd.size()) + " is not supported (ranks 3 and 4 are)");
    const int64_t C = X.c, G = gm.form == 'c' ? C : gm.groups;
    if (G < 1 || C % G) fail(who + ": C = " + std::to_string(C) + " is not divisible by num_groups = " + std::to_string(G));
    int64_t total = 1;
    for (int64_t d : xd) total *= d;
    const int64_t per = gm.form == 'b' && m.opset >= 21 ? C : (gm.form == 'c' ? C : G);
    if (gm.scale->numel() != per || gm.bias->numel() != per || gm.scale->dims.size() != 1 || gm.bias->dims.size() != 1)
        fail(who + ": scale " + dstr(gm.scale->dims) + " and bias " + dstr(gm.bias->dims) + " must both be [" + std::to_string(per) + "]");
    if (gm.form == 'a') {
        const std::vector<int64_t>& s1 = gm.shape1;
        if (!((s1[0] == 0 || s1[0] == xd[0]) && (s1[2] == -1 || s1[2] == total / (xd[0] * G))))
            fail(who + ": the Reshape in front of it goes to " + dstr(s1) + ", not to [0, " + std::to_string(G) + ", -1]");
        if (!gm.back.empty()) {
            std::vector<int64_t> d = gm.back;
            int64_t known = 1, neg = -1;
            for (size_t k = 0; k < d.size(); ++k) {
                if (d[k] == 0 && k < 3) d[k] = k == 0 ? xd[0] : (k == 1 ? G : total / (xd[0] * G));      // (0 copies the dim of the Reshape's own input [N, G, .])
                if (d[k] == -1) neg = int64_t(k); else known *= d[k];
            }
            if (neg >= 0 && known > 0 && total % known == 0) d[size_t(neg)] = total / known;
            if (d != xd) fail(who + ": the Reshape behind it restores " + dstr(gm.back) + ", not the input's shape " + dstr(xd));
        }
        const std::vector<int64_t> want = xd.size() == 4 ? std::vector<int64_t>{C, 1, 1} : std::vector<int64_t>{C, 1};
        auto per_channel = [&](const OnnxTensor* t, const std::string& name, const char* what) {
            if (t && (t->f.empty() || t->dims != want)) fail(who + ": " + what + " " + name + " has the shape " + dstr(t->dims) + ", not " + dstr(want));
        };
        per_channel(gm.gamma, gm.gamma_name, "gamma");
        per_channel(gm.beta, gm.beta_name, "beta");
    }
    LNode n;
    n.kind = L_GROUPNORM;
    n.name = gm.name;
    n.gn_groups = int(G);
    n.eps = gm.eps;
    n.s.resize(size_t(C));
    n.t.resize(size_t(C));
    const int64_t cpg = C / G;
    for (int64_t c = 0; c < C; ++c) {
        const size_t k = size_t(per == C ? c : c / cpg);
        const float s = gm.scale->f[k], b = gm.bias->f[k];
        const float g = gm.gamma ? gm.gamma->f[size_t(c)] : 1.f, be = gm.beta ? gm.beta->f[size_t(c)] : 0.f;
        // (xn * s + b) * g + be: exact where the inner scale and bias are 1 and 0
        n.s[size_t(c)] = s * g;
        n.t[size_t(c)] = b * g + be;
    }
    n.in = {v};
    (void)on;
    push_node(std::move(n), gm.out, X.dims, false);
    if (flat) L.flat_names.insert(gm.out);
    if (back) L.back_names.insert(gm.out);
}

// ---- a SiLU, ReLU or Sigmoid behind a group norm, as its sole reader, runs in the norm's apply phase ----
void Planner::FuseGroupNormActivations() {
    for (size_t i = 0; i < L.nodes.size(); ++i) {
        LNode& gn = L.nodes[i];
        if (gn.dead || gn.kind != L_GROUPNORM || gn.act.kind != ActKind::None || !single_consumer(gn.out)) continue;
        LNode& b = L.nodes[size_t(L.consumers(gn.out)[0])];
        if (b.in.size() != 1) continue;
        if (b.kind == L_RELU) gn.act = Act{ActKind::Relu, 0.f, 0.f};
        else if (b.kind == L_ACT && (b.act.kind == ActKind::Silu || b.act.kind == ActKind::Sigmoid)) gn.act = b.act;
        else continue;
        gn.name += "+" + b.name;
        gn.out = b.out;
        L.vals[gn.out].producer = int(i);
        b.dead = true;
    }
}

void Planner::FuseTokenAssemble() {
    for (size_t i = 0; i < L.nodes.size(); ++i) {
        LNode& a = L.nodes[i];
        if (a.dead || a.kind != L_TOKPOS) continue;
        const int p = L.vals[a.in[0]].producer;
        if (p < 0 || L.nodes[size_t(p)].dead || L.nodes[size_t(p)].kind != L_TOKASM || !L.nodes[size_t(p)].t.empty() || !single_consumer(a.in[0]))
            fail("Add " + a.name + ": a [1, L, D] constant is only added to tokens directly behind the class-token Concat, as its sole reader");
        LNode& c = L.nodes[size_t(p)];
        c.t = a.t;
        c.name += "+" + a.name;
        c.out = a.out;
        L.vals[c.out].producer = p;
        a.dead = true;
    }
}

void Planner::MarkOutputs() {
    for (const auto& vo : m.outputs) {
        int v = L.get_val(vo.name);
        // A token value [N, L, D] is an output as it is where a decoder needs one: its NHWC buffer [N, 1, L, D] is that tensor row-major.  Two kinds
        // are taken: the result of a Linear (the vocabulary head: a conv step writes the dense fp32 buffer itself in every precision, as a classifier's
        // last Gemm does), and a value the graph also reads further (last_hidden_state under the head: copied, like every output that is read further).
        // A token value that no Linear made and nothing else reads keeps the refusal (another producer would have to write fp32 out of an fp16
        // plan: an attention step then leaves its MFMA tiles, which want one element type on both sides), and so do the half-way names of the token views
        auto linear_result = [&](int x) {
            const int p = L.vals[x].producer;
            if (p < 0) return false;
            const LNode& n = L.nodes[size_t(p)];
            if (n.kind == L_CONV) return true;
            // (the bias Add of a Linear, which FuseConvEpilogues folds into the conv in front of it)
            const int q = n.kind == L_AFFINE && single_consumer(n.in[0]) ? L.vals[n.in[0]].producer : -1;
            return q >= 0 && L.nodes[size_t(q)].kind == L_CONV;
        };
        const bool half_way = L.flat_names.count(vo.name) || L.back_names.count(vo.name);
        if (L.is_tok(vo.name) && !half_way && (linear_result(v) || !L.consumers(v).empty())) tok_outputs.insert(v);
        else if (L.is_tok(vo.name) || half_way)
            fail("graph output " + vo.name + " is a token view; outputs are NCHW: transpose it back with perm [0,2,1] and reshape it to [N, D, h, w]");
        if (L.is_cl(vo.name)) fail("graph output " + vo.name + " is a channels-last view (a Transpose with perm [0,2,3,1]); outputs are NCHW: transpose it back with perm [0,3,1,2]");
        L.vals[v].is_output = true;
    }
}

// fp8 mode has no kernels for these: a load error, never another kernel reading the bytes
void Planner::RefuseForF8() const {
    for (const LNode& n : L.nodes) {
        if (n.transposed) fail("ConvTranspose is not supported in fp8 mode (node " + n.name + ")");
        if (n.dw) fail("depthwise convolution is not supported in fp8 mode (Conv " + n.name + ")");
        if (n.kind == L_CONV && n.group != 1) fail("grouped convolution is not supported in fp8 mode (Conv " + n.name + ")");
        if (n.kind == L_CONV && (n.dil_h > 1 || n.dil_w > 1)) fail("dilated convolution is not supported in fp8 mode (Conv " + n.name + ")");
        if (n.kind == L_RESIZE) fail("Resize is not supported in fp8 mode (node " + n.name + ")");
        if (n.kind == L_LAYERNORM && n.rms) fail("RMSNormalization is not supported in fp8 mode (node " + n.name + ")");
        if (n.kind == L_LAYERNORM || n.kind == L_EMBED) fail("LayerNormalization is not supported in fp8 mode (node " + n.name + ")");
        if (n.kind == L_GROUPNORM) fail("GroupNormalization is not supported in fp8 mode (node " + n.name + ")");
    }
    for (const LNode& n : L.nodes)
        if (n.kind == L_ATTENTION || n.kind == L_TOKASM || n.kind == L_TOKPOS) fail("attention and token views are not supported in fp8 mode (node " + n.name + ")");
    for (const LNode& n : L.nodes)
        if (n.kind == L_WATTN || n.kind == L_PATCHMERGE) fail("window attention and patch merging are not supported in fp8 mode (node " + n.name + ")");
    for (const LNode& n : L.nodes)
        if (n.kind == L_ACT || n.kind == L_MUL || n.kind == L_ERF)
            fail("activation and squeeze-excite nodes (Sigmoid, HardSigmoid, HardSwish, Mul of two activations) are not supported in fp8 mode (node " + n.name + ")");
}

// ---- activation patterns: Mul(x, Sigmoid(x)) = SiLU, Mul(x, HardSigmoid(x; a, b)) = hardswish(a, b) (opset < 14 exports), either order ----
void Planner::FuseActivationPatterns() {
    for (size_t i = 0; i < L.nodes.size(); ++i) {
        LNode& mu = L.nodes[i];
        if (mu.dead || mu.kind != L_MUL || L.vals[mu.in[0]].dims != L.vals[mu.in[1]].dims) continue;
        for (int k = 0; k < 2; ++k) {
            const int g = L.vals[mu.in[k]].producer, x = mu.in[1 - k];
            if (g < 0 || L.nodes[g].dead || L.nodes[g].kind != L_ACT || L.nodes[g].in[0] != x || !single_consumer(mu.in[k])) continue;
            LNode& sg = L.nodes[g];
            if (sg.act.kind == ActKind::Sigmoid) mu.act.kind = ActKind::Silu;
            else if (sg.act.kind == ActKind::HardSigmoid) { mu.act = sg.act; mu.act.kind = ActKind::HardSwish; }
            else continue;
            mu.kind = L_ACT;
            mu.in = {x};
            mu.name = sg.name + "+" + mu.name;
            sg.dead = true;
            break;
        }
    }
    // GELU as exporters write it below opset 20: Div(x, sqrt 2) | Mul(x, 1 / sqrt 2) -> Erf -> Add 1 -> Mul x (either order) -> Mul 0.5, every
    // intermediate read by the next node only.  The constants must be the GELU's to 1e-6 relative: a near miss is not approximated, its Erf is
    // refused like any Erf outside the pattern.
    auto uniform_affine = [&](const LNode& a, double sv, double tv) {
        if (a.dead || a.kind != L_AFFINE || a.relu) return false;
        for (float v : a.s) if (std::fabs(double(v) - sv) > 1e-6 * std::fabs(sv)) return false;
        for (float v : a.t) if (std::fabs(double(v) - tv) > 1e-6 * std::fabs(tv)) return false;
        return true;
    };
    auto only_reader = [&](int v) -> LNode* { return single_consumer(v) ? &L.nodes[size_t(L.consumers(v)[0])] : nullptr; };
    for (size_t i = 0; i < L.nodes.size(); ++i) {
        LNode& e = L.nodes[i];
        if (e.dead || e.kind != L_ERF) continue;
        const int p = L.vals[e.in[0]].producer;
        LNode* dv = p >= 0 && single_consumer(e.in[0]) ? &L.nodes[size_t(p)] : nullptr;
        LNode* a1 = only_reader(e.out);
        LNode* mu = a1 ? only_reader(a1->out) : nullptr;
        LNode* hf = mu ? only_reader(mu->out) : nullptr;
        if (!dv || !hf || !uniform_affine(*dv, 0.70710678118654752, 0.0) || !uniform_affine(*a1, 1.0, 1.0) || !uniform_affine(*hf, 0.5, 0.0)) continue;
        const int x = dv->in[0];
        if (mu->dead || mu->kind != L_MUL || L.vals[mu->in[0]].dims != L.vals[mu->in[1]].dims || !((mu->in[0] == x && mu->in[1] == a1->out) || (mu->in[1] == x && mu->in[0] == a1->out)))
            continue;
        hf->kind = L_ACT;
        hf->act = Act{ActKind::Gelu, 0.f, 0.f};
        hf->in = {x};
        hf->s.clear();
        hf->t.clear();
        hf->name = dv->name + "+" + e.name + "+" + a1->name + "+" + mu->name + "+" + hf->name;
        dv->dead = e.dead = a1->dead = mu->dead = true;
    }
    for (const LNode& e : L.nodes)
        if (!e.dead && e.kind == L_ERF) fail("Unsupported ONNX operator: Erf (node " + e.name + ")");
}

// ---- gated units (SwiGLU, GeGLU): Mul(act(a), b) of two activations of one shape, act a SiLU or a GELU read by the Mul alone, either operand order:
//      ONE eltwise step, out = act(a) * b (EltArgs::pre_act).  Runs behind FuseActivationPatterns, so every SiLU / GELU spelling is an L_ACT here ----
void Planner::FuseGatedActivations() {
    for (size_t i = 0; i < L.nodes.size(); ++i) {
        LNode& mu = L.nodes[i];
        if (mu.dead || mu.kind != L_MUL || mu.pre_act.kind != ActKind::None || mu.in[0] == mu.in[1] || L.vals[mu.in[0]].dims != L.vals[mu.in[1]].dims) continue;
        for (int k = 0; k < 2; ++k) {
            const int g = L.vals[mu.in[k]].producer;
            if (g < 0 || L.nodes[g].dead || L.nodes[g].kind != L_ACT || !single_consumer(mu.in[k])) continue;
            LNode& ac = L.nodes[g];
            if (ac.act.kind != ActKind::Silu && ac.act.kind != ActKind::Gelu && ac.act.kind != ActKind::GeluTanh) continue;
            mu.pre_act = ac.act;
            mu.in = {ac.in[0], mu.in[1 - k]};
            mu.name = ac.name + "+" + mu.name;
            ac.dead = true;
            break;
        }
    }
}

// ---- squeeze-excite: GlobalAveragePool -> Conv1x1 -> ReLU | act -> Conv1x1 -> act -> Mul(x, gate) as ONE node, where x is read by the pool
//      and the Mul only (IE_NO_SE_FUSE=1: the separate steps) ----
void Planner::FuseSqueezeExcite() {
    auto prod = [&](int v, LKind k) -> LNode* {
        const int p = L.vals[v].producer;
        if (p < 0 || L.nodes[p].dead || L.nodes[p].kind != k || !single_consumer(v)) return nullptr;
        return &L.nodes[p];
    };
    auto fc_ok = [&](const LNode* c, int64_t cin, int64_t cout) {
        return c && c->group == 1 && !c->transposed && c->kh == 1 && c->kw == 1 && c->sh == 1 && c->sw == 1 && !c->pt && !c->pl && !c->pb && !c->pr && c->res < 0 &&
               L.vals[c->in[0]].dims.size() == 4 && L.vals[c->in[0]].c == cin && L.vals[c->out].c == cout && int64_t(c->w.size()) == cin * cout;
    };
    for (size_t i = 0; i < L.nodes.size(); ++i) {
        LNode& mu = L.nodes[i];
        if (mu.dead || mu.kind != L_MUL) continue;
        const int x = mu.in[0];
        const Val& X = L.vals[x];
        if (X.dims.size() != 4 || L.vals[mu.in[1]].h * L.vals[mu.in[1]].w != 1 || X.h * X.w == 1 || X.is_output || X.is_input) continue;
        LNode* gate = prod(mu.in[1], L_ACT);
        LNode* c2 = gate ? prod(gate->in[0], L_CONV) : nullptr;
        if (!c2) continue;
        const int hv = c2->in[0];
        const int64_t mid = L.vals[hv].c;
        LNode* a1 = prod(hv, L_RELU);
        if (!a1) a1 = prod(hv, L_ACT);
        LNode* c1 = a1 ? prod(a1->in[0], L_CONV) : nullptr;
        LNode* gp = c1 ? prod(c1->in[0], L_GAP) : nullptr;
        if (!gp || gp->in[0] != x || !fc_ok(c1, X.c, mid) || !fc_ok(c2, mid, X.c)) continue;
        const std::vector<int> readers = L.consumers(x);
        if (readers.size() != 2) continue;
        LNode se;
        se.kind = L_SE;
        se.name = gp->name + " ... " + mu.name;
        se.in = {x};
        se.out = mu.out;
        se.w = c1->w;
        se.bias = c1->bias;
        se.w2.resize(c2->w.size());
        for (int64_t o = 0; o < X.c; ++o)
            for (int64_t j = 0; j < mid; ++j) se.w2[size_t(j * X.c + o)] = c2->w[size_t(o * mid + j)];
        se.bias2 = c2->bias;
        se.se_mid = int(mid);
        if (a1->kind == L_RELU) se.se_act1.kind = ActKind::Relu;
        else se.se_act1 = a1->act;
        se.act = gate->act;
        gp->dead = c1->dead = a1->dead = c2->dead = gate->dead = true;
        mu = std::move(se);
    }
}

// ---- fusion 1: merge Affine->Affine chains (BN followed by Caffe-style Scale Mul/Add) ----------
void Planner::MergeAffineChains() {
    for (size_t i = 0; i < L.nodes.size(); ++i) {
        LNode& a = L.nodes[i];
        if (a.dead || a.kind != L_AFFINE) continue;
        while (single_consumer(a.out)) {
            int ci = L.consumers(a.out)[0];
            LNode& b = L.nodes[ci];
            if (b.kind != L_AFFINE) break;
            for (size_t c = 0; c < a.s.size(); ++c) {
                a.t[c] = b.s[c] * a.t[c] + b.t[c];
                a.s[c] = b.s[c] * a.s[c];
            }
            a.name += "+" + b.name;
            a.out = b.out;
            L.vals[a.out].producer = int(i);
            b.dead = true;
        }
    }
}

// ---- fusion 2: conv epilogues (Conv -> Affine -> Relu) -----------------------------------------
void Planner::FuseConvEpilogues() {
    for (size_t i = 0; i < L.nodes.size(); ++i) {
        LNode& cv = L.nodes[i];
        if (cv.dead || cv.kind != L_CONV) continue;
        int64_t cout = L.vals[cv.out].c;
        size_t kper = cv.w.size() / size_t(cout);
        bool clamped = false;
        while (single_consumer(cv.out) && !cv.relu && !clamped && cv.act.kind == ActKind::None) {
            int ci = L.consumers(cv.out)[0];
            LNode& b = L.nodes[ci];
            if (b.kind == L_ACT) {
                // only the depthwise and grouped kernels have an activation epilogue (an activation behind another conv: fusion 2d below, or an
                // eltwise step)
                if (cv.group == 1) break;              // (a transposed conv has group 1: it keeps the eltwise step)
                cv.act = b.act;
            } else if (b.kind == L_CLIP) {
                // only the depthwise and grouped kernels have a clamp epilogue (a Clip behind another conv: see the ReLU6 pass below, or an
                // eltwise step)
                if (cv.group == 1) break;
                cv.lo = b.lo;
                cv.hi = b.hi;
                clamped = true;
            } else if (b.kind == L_AFFINE) {
                // Once a residual has been absorbed the epilogue computes conv + bias + res: scaling weights and bias would leave
                // the shortcut unscaled (pre-activation / ResNet-v2 blocks: Conv -> Add -> BN -> ReLU).  The BN then becomes the
                // consumer's prologue (fusion 3) or a standalone eltwise step (fusion 4).
                if (cv.res >= 0) break;
                if (cv.bias.empty()) cv.bias.assign(size_t(cout), 0.f);
                if (cv.transposed) {               // w is [kh][kw][Cout][Cin]: row (tap, o) scales by s[o]
                    const size_t cin = size_t(L.vals[cv.in[0]].c);
                    for (size_t row = 0; row < cv.w.size() / cin; ++row)
                        for (size_t c = 0; c < cin; ++c) cv.w[row * cin + c] *= b.s[row % size_t(cout)];
                    for (int64_t o = 0; o < cout; ++o) cv.bias[o] = cv.bias[o] * b.s[o] + b.t[o];
                } else {
                    for (int64_t o = 0; o < cout; ++o) {
                        for (size_t k = 0; k < kper; ++k) cv.w[size_t(o) * kper + k] *= b.s[o];
                        cv.bias[o] = cv.bias[o] * b.s[o] + b.t[o];
                    }
                }
            } else if (b.kind == L_RELU) cv.relu = true;
            else if (b.kind == L_ADD && cv.res < 0 && !cv.transposed) {
                // residual shortcut: fold the Add into this conv's epilogue when the other operand already exists at this point of
                // the schedule (its producer runs earlier); otherwise the other branch's conv picks the Add up when its turn comes
                const int other = b.in[0] == cv.out ? b.in[1] : b.in[0];
                const int op = L.vals[other].producer;
                if (other == cv.out || !(L.vals[other].is_input ? false : op >= 0 && op < int(i))) break;
                cv.res = other;
                cv.in.push_back(other);
            } else break;
            cv.name += "+" + b.name;
            cv.out = b.out;
            L.vals[cv.out].producer = int(i);
            b.dead = true;
        }
    }
}

// ---- fusion 2b: ReLU6 between a conv and a depthwise conv (MobileNetV2's expand 1x1 -> Clip(0, 6) -> depthwise 3x3) ---------------
// A Clip with lo == 0 on a conv's output whose only reader is a depthwise conv without a prologue: the producing conv's epilogue applies
// the ReLU, the upper bound rides into the depthwise conv's prologue (min(max(x, 0), hi) on every in-range tap).  No dense-conv kernel
// needs a clamp epilogue.
void Planner::FuseRelu6IntoDepthwise() {
    for (size_t i = 0; i < L.nodes.size(); ++i) {
        LNode& c = L.nodes[i];
        if (c.dead || c.kind != L_CLIP || c.lo != 0.f) continue;
        const int x = c.in[0];
        const int p = L.vals[x].producer;
        if (p < 0 || L.nodes[p].dead || L.nodes[p].kind != L_CONV || L.nodes[p].dw || L.nodes[p].transposed || !single_consumer(x) || !single_consumer(c.out)) continue;
        LNode& d = L.nodes[L.consumers(c.out)[0]];
        if (d.kind != L_CONV || !d.dw || d.has_pre || d.in[0] != c.out || d.res == c.out) continue;
        LNode& cv = L.nodes[p];
        cv.relu = true;
        cv.name += "+" + c.name;
        cv.out = c.out;
        L.vals[cv.out].producer = p;
        d.has_pre = true;
        d.pre_relu = true;
        d.pre_hi = c.hi;
        d.pre_s.assign(size_t(L.vals[c.out].c), 1.f);
        d.pre_t.assign(size_t(L.vals[c.out].c), 0.f);
        c.dead = true;
    }
}

// ---- fusion 2d: an activation between a conv and a depthwise conv (expand 1x1 -> BN -> act -> depthwise) goes into the depthwise conv's
//      prologue (the producer runs linear: no dense-conv kernel needs an activation epilogue); one in front of a global pool (head 1x1 ->
//      act -> GlobalAveragePool) into the pool's prologue.  Any other activation becomes an eltwise step. -------------------------------
void Planner::FuseActivationPrologues() {
    for (size_t i = 0; i < L.nodes.size(); ++i) {
        LNode& a = L.nodes[i];
        if (a.dead || a.kind != L_ACT || !single_consumer(a.out)) continue;
        const int x = a.in[0];
        LNode& d = L.nodes[L.consumers(a.out)[0]];
        const int p = L.vals[x].producer;
        if (d.kind == L_CONV && d.dw && !d.has_pre && d.in[0] == a.out && d.res != a.out && p >= 0 && !L.nodes[p].dead && L.nodes[p].kind == L_CONV &&
            !L.nodes[p].dw && !L.nodes[p].transposed && single_consumer(x)) {
            LNode& cv = L.nodes[p];
            cv.name += "+" + a.name;
            cv.out = a.out;
            L.vals[cv.out].producer = p;
            d.has_pre = true;
            d.pre_act = a.act;
            d.pre_s.assign(size_t(L.vals[a.out].c), 1.f);
            d.pre_t.assign(size_t(L.vals[a.out].c), 0.f);
            a.dead = true;
        } else if (d.kind == L_GAP && d.in[0] == a.out && d.pre_act.kind == ActKind::None && !d.has_pre) {
            d.pre_act = a.act;
            d.name = a.name + "+" + d.name;
            d.in[0] = x;
            a.dead = true;
        }
    }
}

// ---- fusion 2c: Conv1x1 -> AveragePool  ==>  AveragePool -> Conv1x1 ---------------------------------
// Both are linear and a 1x1/stride-1 conv acts per pixel, so they commute (the conv's bias too: the mean of a constant is the
// constant).  DenseNet's transitions (BN -> ReLU -> Conv1x1 -> AvgPool2x2) then run their conv on a quarter of the pixels:
// 4x fewer FLOPs for those layers (8 % of the network), and the BN+ReLU prologue rides on the pool.  Only when the pool window
// tiles the image exactly (no padding, no partial windows), so every output averages the same number of inputs.
void Planner::SwapConvAndAvgPool() {
    for (size_t i = 0; i < L.nodes.size(); ++i) {
        if (L.nodes[i].dead || L.nodes[i].kind != L_CONV) continue;
        const LNode& cv0 = L.nodes[i];
        if (cv0.transposed || cv0.kh != 1 || cv0.kw != 1 || cv0.sh != 1 || cv0.sw != 1 || cv0.pt || cv0.pl || cv0.pb || cv0.pr || cv0.relu || cv0.res >= 0) continue;
        if (!single_consumer(cv0.out)) continue;
        const int pj = L.consumers(cv0.out)[0];
        const LNode& pl0 = L.nodes[pj];
        const Val& X = L.vals[cv0.in[0]];
        if (pl0.kind != L_AVGPOOL || pl0.pt || pl0.pl || pl0.pb || pl0.pr || pl0.kh != pl0.sh || pl0.kw != pl0.sw || X.h % pl0.kh || X.w % pl0.kw ||
            X.is_input)
            continue;
        // new value: the pooled conv input [N, Cin, H/k, W/k]
        const int x = cv0.in[0], conv_out = cv0.out, pool_out = pl0.out;
        const int pooled = L.new_val(L.vals[x].name + "/pooled@" + pl0.name, {X.n, X.c, X.h / pl0.kh, X.w / pl0.kw});
        LNode conv = L.nodes[i], pool = L.nodes[size_t(pj)];
        pool.in = {x};
        pool.out = pooled;
        pool.name = pl0.name + "(before " + cv0.name + ")";
        conv.in[0] = pooled;
        conv.out = pool_out;                        // same dims as before: [N, Cout, H/k, W/k]
        (void)conv_out;                             // the full-resolution conv output no longer exists
        // the pool takes the conv's slot in the schedule, the conv the pool's (everything in between is independent of both)
        L.nodes[i] = pool;
        L.nodes[size_t(pj)] = conv;
        L.vals[pooled].producer = int(i);
        L.vals[pool_out].producer = pj;
        L.vals[conv_out].producer = -1;
    }
}

// ---- fusion 3: prologues (Affine -> Relu -> {Conv, GlobalAveragePool, swapped AveragePool}) ---------
void Planner::FusePrologues() {
    for (size_t i = 0; i < L.nodes.size(); ++i) {
        LNode& cv = L.nodes[i];
        if (cv.dead || (cv.kind != L_CONV && cv.kind != L_GAP && cv.kind != L_AVGPOOL) || cv.transposed) continue;
        int x = cv.in[0];
        bool took_relu = false;
        int p = L.vals[x].producer;
        if (p >= 0 && !L.nodes[p].dead && L.nodes[p].kind == L_RELU && single_consumer(x)) {
            cv.pre_relu = true;
            cv.has_pre = true;
            cv.name = L.nodes[p].name + "+" + cv.name;
            L.nodes[p].dead = true;
            x = L.nodes[p].in[0];
            took_relu = true;
        }
        p = L.vals[x].producer;
        if (p >= 0 && !L.nodes[p].dead && L.nodes[p].kind == L_AFFINE && !L.vals[x].is_output) {
            // live consumers of x: none if its Relu was just absorbed, else exactly this node
            std::vector<int> cons = L.consumers(x);
            bool ok = took_relu ? cons.empty() : (cons.size() == 1 && cons[0] == int(i));
            if (ok) {
                cv.pre_s = L.nodes[p].s;
                cv.pre_t = L.nodes[p].t;
                cv.has_pre = true;
                cv.name = L.nodes[p].name + "+" + cv.name;
                L.nodes[p].dead = true;
                x = L.nodes[p].in[0];
            }
        }
        if (cv.has_pre && cv.pre_s.empty()) {
            cv.pre_s.assign(size_t(L.vals[x].c), 1.f);
            cv.pre_t.assign(size_t(L.vals[x].c), 0.f);
        }
        cv.in[0] = x;
    }
}

// ---- fusion 4: Add -> Relu, Affine -> Relu -----------------------------------------------------
void Planner::FuseTrailingRelu() {
    for (size_t i = 0; i < L.nodes.size(); ++i) {
        LNode& a = L.nodes[i];
        if (a.dead || (a.kind != L_ADD && a.kind != L_AFFINE)) continue;
        if (single_consumer(a.out)) {
            LNode& b = L.nodes[L.consumers(a.out)[0]];
            if (b.kind == L_RELU) {
                a.relu = true;
                a.name += "+" + b.name;
                a.out = b.out;
                L.vals[a.out].producer = int(i);
                b.dead = true;
            }
        }
    }
}

// ---- graph inputs in NCHW: only convs can read them strided; otherwise stage an NHWC copy ------
void Planner::StageNchwInputs() {
    std::vector<LNode> pre;
    for (size_t v = 0; v < L.vals.size(); ++v) {
        if (!L.vals[v].is_input || !L.vals[v].input_nchw) continue;
        bool all_conv = true;
        for (int ci : L.consumers(int(v)))
            if (L.nodes[ci].kind != L_CONV || L.nodes[ci].transposed || L.nodes[ci].in[0] != int(v) || L.nodes[ci].res == int(v)) all_conv = false;
        if (all_conv && !L.vals[v].is_output) continue;
        // the cache of a decode step is read in place, in the ABI's own order [N][Hkv][P][hd]: no staging copy
        bool all_kv = !L.consumers(int(v)).empty() && !L.vals[v].is_output;
        for (int ci : L.consumers(int(v))) if (L.nodes[ci].kind != L_KVAPPEND || L.nodes[ci].in[0] == int(v)) all_kv = false;
        if (all_kv) continue;
        LNode cp;
        cp.kind = L_COPY;
        cp.name = "nchw_to_nhwc(" + L.vals[v].name + ")";
        cp.in = {int(v)};
        cp.out = L.new_val(L.vals[v].name + "/nhwc", L.vals[v].dims);
        for (auto& nd : L.nodes) if (!nd.dead) for (int& x : nd.in) if (x == int(v)) x = cp.out;
        pre.push_back(cp);
    }
    if (!pre.empty()) {
        size_t shift = pre.size();
        L.nodes.insert(L.nodes.begin(), pre.begin(), pre.end());
        for (auto& val : L.vals) if (val.producer >= 0) val.producer += int(shift);
        for (size_t k = 0; k < shift; ++k) L.vals[L.nodes[k].out].producer = int(k);
    }
}

// ---- graph outputs must end up dense (NCHW order) in their own buffer --------------------------
void Planner::DensifyOutputs() {
    for (const auto& vo : m.outputs) {
        int v = L.get_val(vo.name);
        // Always materialise through a copy when the tensor is spatial (NHWC->NCHW) or is a graph input;
        // [N,C,1,1] / [N,C] tensors are already in ABI order and only need their own dense buffer.
        const bool tok = tok_outputs.count(v) != 0;
        bool spatial = L.vals[v].h * L.vals[v].w > 1 && !tok;      // (a token output stays [N, L, D] rows: no NCHW transposition)
        bool consumed = !L.consumers(v).empty();
        // a Resize whose result is read by nothing else writes the dense NCHW fp32 output itself (a segmentation head's last step)
        const int pr = L.vals[v].producer;
        if (spatial && !consumed && !L.vals[v].is_input && pr >= 0 && L.nodes[size_t(pr)].kind == L_RESIZE && !L.nodes[size_t(pr)].dead &&
            std::find(out_vals.begin(), out_vals.end(), v) == out_vals.end()) {
            L.vals[v].input_nchw = true;           // reused flag: dense NCHW layout
            out_vals.push_back(v);
            continue;
        }
        // a kv_append node writes the dense fp32 [N][Hkv][rows][hd] output itself; a decode step's attention reads it there
        if (!L.vals[v].is_input && pr >= 0 && L.nodes[size_t(pr)].kind == L_KVAPPEND && std::find(out_vals.begin(), out_vals.end(), v) == out_vals.end()) {
            L.vals[v].input_nchw = true;           // reused flag: dense NCHW layout
            out_vals.push_back(v);
            continue;
        }
        if (spatial || L.vals[v].is_input || consumed || L.vals[v].sel_rows > 1 ||
            (tok && (std::find(out_vals.begin(), out_vals.end(), v) != out_vals.end() || L.vals[v].producer < 0 || L.nodes[size_t(L.vals[v].producer)].kind == L_ALIAS))) {
            LNode cp;
            cp.kind = L_COPY;
            cp.name = "to_output(" + L.vals[v].name + ")";
            cp.in = {v};
            cp.out = L.new_val(L.vals[v].name + "/out", L.vals[v].dims);
            L.vals[cp.out].is_output = true;
            L.vals[cp.out].input_nchw = spatial;   // reused flag: dense NCHW layout
            if (tok) tok_outputs.insert(cp.out);
            L.vals[v].is_output = false;
            L.vals[cp.out].producer = int(L.nodes.size());
            L.nodes.push_back(cp);
            out_vals.push_back(cp.out);
        } else out_vals.push_back(v);
    }
}

// ---- concat / alias placement ---------------------------------------------------------------
void Planner::PlaceConcatsAndAliases() {
    for (int i = int(L.nodes.size()) - 1; i >= 0; --i) {
        LNode& n = L.nodes[i];
        if (n.dead) continue;
        if (n.kind == L_ALIAS) {
            Val& src = L.vals[n.in[0]];
            // the alias output shares storage with its input: make the *input* a child of the output
            if (src.parent < 0 && !src.is_input && !src.is_output) { src.parent = n.out; src.parent_off = 0; }
            else {  // cannot alias: degrade to a copy
                // (the copy kernel walks both sides by the output's rows and columns: a token view of another height is not a copy it can do)
                if (src.h != L.vals[n.out].h || src.w != L.vals[n.out].w)
                    fail("token view " + n.name + ": its input " + src.name + " already lives in another value's buffer (a second view of it, or a Concat); reshaping it "
                         "between a feature map and tokens would need a copy, which is not supported");
                n.kind = L_COPY;
            }
        } else if (n.kind == L_CONCAT) {
            int64_t off = 0;
            for (size_t k = 0; k < n.in.size(); ++k) {
                Val& src = L.vals[n.in[k]];
                bool dup = false;
                for (size_t j = 0; j < k; ++j) if (n.in[j] == n.in[k]) dup = true;
                if (src.parent < 0 && !src.is_input && !src.is_output && !dup) { src.parent = n.out; src.parent_off = off; }
                off += src.c;
            }
        }
    }
    // roots, absolute offsets
    for (size_t v = 0; v < L.vals.size(); ++v) {
        int r = int(v);
        int64_t off = 0;
        while (L.vals[r].parent >= 0) { off += L.vals[r].parent_off; r = L.vals[r].parent; }
        L.vals[v].root = r;
        L.vals[v].abs_off = off;
    }
}

// ---- liveness over live nodes ----
void Planner::ComputeLiveness() {
    for (size_t i = 0; i < L.nodes.size(); ++i) if (!L.nodes[i].dead) order.push_back(int(i));
    first_def.assign(L.vals.size(), kLiveForever);
    last_use.assign(L.vals.size(), -1);
    used.assign(L.vals.size(), 0);
    for (size_t v = 0; v < L.vals.size(); ++v)
        if (L.vals[v].is_input) { first_def[L.vals[v].root] = -1; used[L.vals[v].root] = 1; }
    for (size_t pos = 0; pos < order.size(); ++pos) {
        const LNode& n = L.nodes[order[pos]];
        int r = L.vals[n.out].root;
        used[r] = 1;
        first_def[r] = std::min(first_def[r], int(pos));
        last_use[r] = std::max(last_use[r], int(pos));
        for (int x : n.in) { int rx = L.vals[x].root; last_use[rx] = std::max(last_use[rx], int(pos)); used[rx] = 1; }
    }
}

// Dense fusion (FuseDenseLayers): when a 3x3 conv and the 1x1 conv behind it will run as ONE launch, the 3x3's
// input (the bottleneck tensor, read as halo by neighbouring tiles) must outlive the launch that also writes the next
// bottleneck: keep it live one position longer so the two never share a buffer.
void Planner::KeepDenseFusionInputsLive() {
    for (size_t pos = 0; pos + 1 < order.size(); ++pos) {
        const LNode& a3 = L.nodes[order[pos]];
        size_t nxt = pos + 1;                      // Concat / alias nodes emit nothing: the launch behind the 3x3 is the next real node
        while (nxt < order.size() && (L.nodes[order[nxt]].kind == L_CONCAT || L.nodes[order[nxt]].kind == L_ALIAS)) ++nxt;
        if (nxt >= order.size()) break;
        const LNode& b1 = L.nodes[order[nxt]];
        if (a3.kind != L_CONV || b1.kind != L_CONV || a3.kh != 3 || a3.kw != 3 || b1.kh != 1 || b1.kw != 1 || a3.has_pre || a3.group != 1 || b1.group != 1 ||
            a3.dil_h != 1 || a3.dil_w != 1 || a3.transposed || b1.transposed)
            continue;
        if (L.vals[a3.out].c != 32 || L.vals[b1.out].c != 128 || L.vals[b1.in[0]].root != L.vals[a3.out].root) continue;
        if (L.vals[a3.out].n * L.vals[a3.out].h * L.vals[a3.out].w > FuseMaxPixels(env)) continue;
        const int rb = L.vals[a3.in[0]].root;
        last_use[rb] = std::max(last_use[rb], int(nxt));
    }
}

void Planner::alloc_buf(int r, std::multimap<int64_t, int>& free_pool) {
    int64_t need = root_floats(r);
    // fp8 mode types buffers by tensor shape ([N, C] vectors are halfs, spatial tensors e4m3): vectors get their own buffers so
    // a recycled buffer never changes element type
    bool dedicated = last_use[r] == kLiveForever || (precision == Precision::F8 && L.vals[r].h * L.vals[r].w == 1);
    L.vals[r].dedicated = dedicated;
    if (!dedicated && !keep_buffers) {
        auto it = free_pool.lower_bound(need);
        // accept a recycled buffer up to 2x the needed size; otherwise grow a new one
        if (it != free_pool.end() && it->first <= 2 * need) {
            int b = it->second;
            free_pool.erase(it);
            L.vals[r].buf = b;
            return;
        }
    }
    plan.buffer_floats.push_back(need);
    L.vals[r].buf = int(plan.buffer_floats.size()) - 1;
}

// ---- buffer recycling: graph inputs and outputs keep their buffers, every other root value takes a free buffer of a fitting size ----
void Planner::AssignBuffers() {
    for (int v : out_vals) last_use[L.vals[v].root] = kLiveForever;
    for (size_t v = 0; v < L.vals.size(); ++v) if (L.vals[v].is_input) last_use[L.vals[v].root] = kLiveForever;  // staging buffers stay dedicated
    std::multimap<int64_t, int> free_pool;   // size -> buffer id
    for (size_t v = 0; v < L.vals.size(); ++v)
        if (used[v] && L.vals[v].root == int(v) && first_def[v] == -1) alloc_buf(int(v), free_pool);
    for (size_t pos = 0; pos < order.size(); ++pos) {
        // a group norm whose whole-buffer input dies here writes in place (its kernels read every element before they write it): the output takes over
        // the input's buffer, which therefore does not return to the pool at this position
        // (an RMSNorm likewise: a lane group / wave reads all of its row before it writes any of it, and element for element in and out are one address)
        int handed = -1;
        if (const LNode& gn = L.nodes[size_t(order[pos])]; gn.kind == L_GROUPNORM || (gn.kind == L_LAYERNORM && gn.rms)) {
            const int ri = L.vals[gn.in[0]].root, ro = L.vals[gn.out].root;
            const Val& I = L.vals[gn.in[0]];
            if (ro == gn.out && first_def[ro] == int(pos) && last_use[ro] != kLiveForever && last_use[ri] == int(pos) && L.vals[ri].buf >= 0 && !L.vals[ri].dedicated &&
                I.abs_off == 0 && I.c == L.vals[ri].c && I.sel_rows == 1 && root_floats(ri) == root_floats(ro) && precision != Precision::F8) {
                L.vals[ro].buf = L.vals[ri].buf;
                L.vals[ro].dedicated = false;
                handed = ri;
            }
        }
        for (size_t v = 0; v < L.vals.size(); ++v)
            if (used[v] && L.vals[v].root == int(v) && first_def[v] == int(pos) && !(handed >= 0 && int(v) == L.vals[L.nodes[size_t(order[pos])].out].root)) alloc_buf(int(v), free_pool);
        for (size_t v = 0; v < L.vals.size(); ++v)
            if (!keep_buffers && used[v] && L.vals[v].root == int(v) && last_use[v] == int(pos) && L.vals[v].buf >= 0 && !L.vals[v].dedicated && int(v) != handed)
                free_pool.insert({plan.buffer_floats[size_t(L.vals[v].buf)], L.vals[v].buf});
    }
}

// fp16 mode: every buffer except the graph's own inputs/outputs (dedicated, never recycled) holds halfs
void Planner::MarkBufferTypes() {
    plan.buffer_f16.assign(plan.buffer_floats.size(), precision == Precision::F16 ? 1 : (precision == Precision::F8 ? 2 : 0));
    if (precision == Precision::F8)
        for (size_t v = 0; v < L.vals.size(); ++v)
            if (used[v] && L.vals[v].root == int(v) && L.vals[v].buf >= 0 && L.vals[v].h * L.vals[v].w == 1) plan.buffer_f16[size_t(L.vals[v].buf)] = 1;
    for (size_t v = 0; v < L.vals.size(); ++v)
        if (L.vals[v].is_input && L.vals[L.vals[v].root].buf >= 0) plan.buffer_f16[size_t(L.vals[L.vals[v].root].buf)] = L.vals[v].is_i64 ? 3 : 0;
    for (int v : out_vals)
        if (L.vals[L.vals[v].root].buf >= 0) plan.buffer_f16[size_t(L.vals[L.vals[v].root].buf)] = 0;
}

View Planner::view_of(int v) const {
    const Val& X = L.vals[v];
    const Val& R = L.vals[X.root];
    View w;
    w.buf = R.buf;
    w.f16 = R.buf >= 0 && plan.buffer_f16[size_t(R.buf)] == 1;
    w.f8 = R.buf >= 0 && plan.buffer_f16[size_t(R.buf)] == 2;
    w.i64 = R.buf >= 0 && plan.buffer_f16[size_t(R.buf)] == 3;
    w.n = X.n; w.c = X.c; w.h = X.h; w.w = X.w;
    w.c_off = X.abs_off + X.sel_idx * R.c;
    w.pitch = R.c * X.sel_rows;
    w.nchw = (X.is_input || X.is_output) && X.input_nchw;
    if (w.buf < 0) fail("internal planner error: value " + X.name + " has no buffer");
    return w;
}

bool Planner::output_in_buffer(int buf) const {
    for (int v : out_vals) if (view_of(v).buf == buf) return true;
    return false;
}

ConvFacts::ConvFacts(const LNode& nn, const Step& ss) : n(nn), s(ss) {
    // a dilated conv may only take the kernels that honour the dilation (launch.cpp ConvFamily::dilation): the implicit GEMMs' base tiles and the
    // naive kernel.  Every specialised kernel's eligibility is false for it, and the forcing switches cannot move it elsewhere
    dil = s.dh > 1 || s.dw > 1;
    M = s.out.n * s.out.h * s.out.w; N = s.out.c; K = int64_t(n.kh) * n.kw * s.in.c;
    in16 = s.in.f16;
    in8 = s.in.f8;
    vec_ok = !in16 && !in8 && !s.in.nchw && s.in.c % 4 == 0 && s.in.pitch % 4 == 0 && s.in.c_off % 4 == 0 && n.kh * n.kw <= 32 &&
             s.in.n * s.in.h * s.in.w * s.in.pitch * 4 < (int64_t(1) << 31) && int64_t(n.w.size()) * 4 < (int64_t(1) << 31);
    // fp16 MFMA path: 16-byte chunks of 8 halfs, so channel counts / slice offsets must be multiples of 8
    vec16_ok = in16 && !s.in.nchw && s.in.c % 8 == 0 && s.in.pitch % 8 == 0 && s.in.c_off % 8 == 0 && n.kh * n.kw <= 32 &&
               s.in.n * s.in.h * s.in.w * s.in.pitch * 2 < (int64_t(1) << 31) && int64_t(n.w.size()) * 2 < (int64_t(1) << 31) &&
               s.out.n * s.out.h * s.out.w * s.out.pitch < (int64_t(1) << 31);
    is1x1 = n.kh == 1 && n.kw == 1 && n.sh == 1 && n.sw == 1 && n.pt == 0 && n.pl == 0 && n.pb == 0 && n.pr == 0;
    is3x3 = !dil && n.kh == 3 && n.kw == 3 && n.sh == 1 && n.sw == 1 && n.pt == 1 && n.pl == 1 && n.pb == 1 && n.pr == 1;
}

bool ConvFacts::ws16_ok(int t) const {
    if (t < 0 || t >= 18) return false;          // (12-17: the one-workgroup-per-CU grids of shapes 0-5)
    const int tn = ws_tn[t % 6];
    return vec16_ok && is1x1 && s.in.c % 32 == 0 &&
           (32 * tn * (s.in.c + 8) + 2 * s.in.c) * 2 + 128 * tn <= 160 * 1024 && !(tn > 1 && N <= 32 * (tn / 2)) &&
           (s.out.f16 ? (N % 8 == 0 && s.out.pitch % 8 == 0 && s.out.c_off % 8 == 0) : (N % 4 == 0 && s.out.pitch % 4 == 0 && s.out.c_off % 4 == 0));
}

bool ConvFacts::ws32_ok(int t) const {
    if (t >= 14 && t < 20) t -= 14;              // 14-19: shapes 0-5 on a grid of one workgroup per CU: same operand conditions
    return t >= 0 && t < 14 && vec_ok && !s.out.f16 && is1x1 && s.in.c % 16 == 0 &&
           (t < 12 ? (32 * ws_tn[t] * (s.in.c + 4) + 2 * s.in.c + 32 * ws_tn[t]) * 4 <= 160 * 1024
                   : (s.in.c / 16 >= (t == 12 ? 8 : 4) &&
                      (32 * (s.in.c + 4) + 2 * s.in.c + 32 + (t == 12 ? 4 : 2) * 32 * 36) * 4 <= 160 * 1024)) &&
           !(ws_tn[t] > 1 && N <= 32 * (ws_tn[t] / 2)) && N % 4 == 0 && s.out.pitch % 4 == 0 && s.out.c_off % 4 == 0;
}

bool ConvFacts::ws3_ok(int t3) const {
    static const int ws3_cfg[5][3] = {{4, 2, 12}, {4, 1, 8}, {8, 1, 6}, {2, 1, 12}, {12, 1, 6}};   // waves, row blocks per wave, prefetch depth (kWs3Tiles, kernels_ws.hip)
    if (t3 < 0 || t3 >= 5) return false;
    const int64_t pr3 = 32 * ws3_cfg[t3][1] * ws3_cfg[t3][0] + 2 * (s.in.w + 1) + 2;
    return vec16_ok && s.out.f16 && is3x3 && !n.has_pre && N % 8 == 0 && s.out.pitch % 8 == 0 && s.out.c_off % 8 == 0 &&
           pr3 <= ws3_cfg[t3][2] * (64 * ws3_cfg[t3][0] / 8) && (9 * ((s.in.c + 63) / 64) * 32 + pr3) * 144 + 128 <= 160 * 1024;
}

bool ConvFacts::direct_ok(int t) const {
    static const int dcfg[6][3] = {{1, 8, 8}, {1, 16, 4}, {1, 9, 8}, {1, 4, 8}, {1, 12, 6}, {2, 8, 4}};   // tn, waves, max chunks
    static const int wcfg[4][3] = {{1, 8, 9}, {2, 8, 9}, {1, 4, 18}, {2, 4, 18}};                      // window variants: tn, waves, max chunks
    if (t < 0 || t >= 15 || dil) return false;
    if (t >= 10) {     // activations-stationary 1x1 (fp32): the workgroup's 32 / 16 pixel rows in LDS, weights streamed from the mirror
        static const int acfg[5] = {128, 64, 256, 64, 64};                                        // output channels per workgroup
        return vec_ok && !in16 && !s.out.f16 && !s.has_in2 && is1x1 && s.in.c % 16 == 0 && N % acfg[t - 10] == 0 && s.out.pitch % 4 == 0 &&
               s.out.c_off % 4 == 0 && M <= (int64_t(1) << 22) && 32 * (s.in.c + 4) * 4 <= 160 * 1024;
    }
    if (t >= 6) {      // fp32, output grid == input grid, activations through an LDS window, fragment-major weights
        const int* wc = wcfg[t - 6];
        const int64_t total = s.in.c % 16 == 0 ? int64_t(n.kh) * n.kw * (s.in.c / 16) : 0;
        const int64_t win = (16 + (n.kh - 1) * s.in.w + (n.kw - 1)) * (s.in.c + 4) * 4, part = int64_t(wc[1]) * 16 * (16 * wc[0] + 4) * 4;
        return vec_ok && !in16 && !s.out.f16 && !s.has_in2 && s.in.c % 16 == 0 && N % (16 * wc[0]) == 0 && n.sh == 1 && n.sw == 1 &&
               s.out.h == s.in.h && s.out.w == s.in.w && n.pt < n.kh && n.pl < n.kw && s.out.pitch % 2 == 0 && s.out.c_off % 2 == 0 &&
               total >= wc[1] && total <= wc[1] * wc[2] && M <= 65536 && n.kh * n.kw <= 49 && std::max(win, part) <= 160 * 1024;
    }
    const int cw = in16 ? 32 : 16, al = in16 ? 8 : 4;
    const int64_t total = s.in.c % cw == 0 ? int64_t(n.kh) * n.kw * (s.in.c / cw) : 0;
    return (vec_ok || vec16_ok) && s.in.c % cw == 0 && s.in.pitch % al == 0 && s.in.c_off % al == 0 && N % 2 == 0 && s.out.pitch % 2 == 0 &&
           s.out.c_off % 2 == 0 && total >= dcfg[t][1] && total <= dcfg[t][1] * dcfg[t][2] && !(dcfg[t][0] > 1 && N <= 32) && M <= 65536 &&
           n.kh * n.kw <= 49;
}

int Planner::ForcedTile(int limit) const {
    const char* ft = env.get("IE_FORCE_TILE");
    const int t = ft ? std::atoi(ft) : -1;
    return t >= 0 && t < limit ? t : -1;
}

int64_t Planner::push_vec(const std::vector<float>& v) {
    while (plan.weights.size() % 8) plan.weights.push_back(0.f);   // 32 B in the fp32 blob, 16 B in its half mirror
    int64_t off = int64_t(plan.weights.size());
    plan.weights.insert(plan.weights.end(), v.begin(), v.end());
    return off;
}

int Planner::src_of(const View& v) const {
    auto it = writer.find({int64_t(v.buf), v.c_off, v.c});
    return it == writer.end() ? -1 : it->second;
}

// members that could not be placed in the parent buffer are copied into their slice
void Planner::EmitConcatCopies(const LNode& n) {
    int64_t off = 0;
    for (size_t k = 0; k < n.in.size(); ++k) {
        const Val& src = L.vals[n.in[k]];
        bool placed = src.root == L.vals[n.out].root && src.abs_off == L.vals[n.out].abs_off + off;
        if (!placed) {
            Step c;
            c.kind = StepKind::Copy;
            c.name = n.name + "/copy" + std::to_string(k);
            c.in = view_of(n.in[k]);
            c.out = view_of(n.out);
            c.out.c = src.c;
            c.out.c_off += off;
            c.bytes = vbytes(c.in) + vbytes(c.out);
            if (c.in.f8 || c.out.f8) fail("fp8 precision: concat copy " + c.name + " of an fp8 tensor is not supported");
            c.idx = int(plan.steps.size());
            c.in_src = src_of(c.in);
            writer[{int64_t(c.out.buf), c.out.c_off, c.out.c}] = c.idx;
            plan.steps.push_back(c);
        }
        off += src.c;
    }
}

// depthwise and grouped convs: their own kernels whatever IE_FORCE_ALGO says; IE_FORCE_TILE indexes the depthwise / grouped variants
// (kernels.h kNumConvDwTiles, kNumConvGroupedTiles)
void Planner::EmitGroupConv(const LNode& n, Step& s) {
    s.algo = n.dw ? ConvAlgo::Depthwise : ConvAlgo::Grouped;
    if (!n.dw) s.group = int(n.group);
    s.lo = n.lo;
    s.hi = n.hi;
    s.act = n.act;
    s.pre_act = n.pre_act;
    if (n.dw) s.flops = 2.0 * double(s.out.n) * double(s.out.c) * double(s.out.h) * double(s.out.w) * n.kh * n.kw;
    else s.flops = 2.0 * double(s.out.n) * double(s.out.h) * double(s.out.w) * double(s.out.c) * n.kh * n.kw * double(s.in.c / n.group);
    s.bytes = vbytes(s.in) + vbytes(s.out) + (!n.dw && s.in.f16 ? 2.0 : 4.0) * double(n.w.size()) + (n.res >= 0 ? vbytes(s.in2) : 0.0);
    s.tile = n.dw ? DwDefaultTile(s) : GroupedDefaultTile(s);
    const int t = ForcedTile(n.dw ? kNumConvDwTiles : kNumConvGroupedTiles);
    if (t >= 0 && (t == 0 || (n.dw ? DwFastViews(s) : GroupedFastViews(s, t)))) s.tile = t;
    s.base_tile = 0;
}

// transposed convs: their own kernels whatever IE_FORCE_ALGO says; IE_FORCE_TILE picks a variant where eligible (kernels.h kNumConvtTiles)
void Planner::EmitTransposedConv(const LNode& n, Step& s) {
    s.algo = ConvAlgo::Transposed;
    s.oph = n.op_h;
    s.opw = n.op_w;
    if (s.in.f8 || s.out.f8) fail("ConvTranspose is not supported in fp8 mode (node " + n.name + ")");
    if (s.out.nchw) fail("internal planner error: transposed conv " + n.name + " writes an NCHW view");
    s.flops = 2.0 * double(s.in.n) * double(s.in.h) * double(s.in.w) * double(s.in.c) * double(s.out.c) * n.kh * n.kw;
    s.bytes = vbytes(s.in) + vbytes(s.out) + (s.in.f16 ? 2.0 : 4.0) * double(n.w.size());
    s.tile = ConvtDefaultTile(s);
    const int t = ForcedTile(kNumConvtTiles);
    if (t >= 0 && (t == 0 || ConvtFastViews(s))) s.tile = t;
    s.base_tile = 0;
}

// ---- the base algorithm: naive for toy problems, the implicit GEMMs, the stem kernel, the fp8 GEMM; the heuristic tile ----
void Planner::ChooseBaseAlgo(const ConvFacts& f, Step& s) const {
    const LNode& n = f.n;
    // one-thread-per-output only for toy problems (test_model's 3->5->2 MLP): at batch 1 DenseNet's block-4 convs have
    // M*N = 1568 outputs but K = 1152 - the naive kernel took 141 us there, the MFMA kernels 13 us
    if (f.M * f.N * f.K <= 32768 || (f.M * f.N < 2048 && f.K <= 4096 && !(f.vec_ok || f.vec16_ok))) s.algo = ConvAlgo::Naive;
    else if (f.vec_ok || f.vec16_ok) s.algo = ConvAlgo::IgemmVec;
    else if (f.K <= 2048 && !f.in16) s.algo = ConvAlgo::IgemmScalar;
    else s.algo = ConvAlgo::Naive;
    // the stem of an image classifier (7x7 / stride 2 / pad 3 over the 3-channel NCHW graph input) has its own kernel
    const bool stem_ok = !f.dil && s.in.nchw && !f.in16 && s.in.c == 3 && n.kh == 7 && n.kw == 7 && n.sh == 2 && n.sw == 2 && n.pt == 3 &&
                         n.pl == 3 && n.pb == 3 && n.pr == 3 && !n.has_pre && f.N <= 64 && f.N % 8 == 0 && s.out.pitch % 8 == 0 &&
                         s.out.c_off % 8 == 0 && s.in.numel() * 4 < (int64_t(1) << 31) &&
                         s.out.n * s.out.h * s.out.w * s.out.pitch * 4 < (int64_t(1) << 31);
    if (stem_ok && f.M * f.N >= 2048 && !(s.out.f8 && (f.N % 16 || s.out.pitch % 16 || s.out.c_off % 16))) s.algo = ConvAlgo::Stem;
    if (f.in8 || s.out.f8) {
        // fp8 mode: e4m3 tensors are only understood by the fp8 kernels; anything they cannot run is a load error, never a
        // silent reinterpretation of the bytes by another kernel
        if (s.out.f8 && !f.in8) {
            if (s.algo != ConvAlgo::Stem)
                fail("fp8 precision: conv " + n.name + " reads a non-fp8 tensor and writes an fp8 one; only the 7x7/s2 stem over the fp32 graph input does that");
        } else {
            if (n.has_pre) fail("fp8 precision: conv " + n.name + " has an activation prologue (pre-activation graphs are not supported in fp8 mode)");
            if (!s.out.f8) fail("fp8 precision: conv " + n.name + " reads an fp8 tensor and writes a non-fp8 one");
            if (s.in.nchw || s.in.c % 16 || s.in.pitch % 16 || s.in.c_off % 16 || f.N % 16 || s.out.pitch % 16 || s.out.c_off % 16 || n.kh * n.kw > 32)
                fail("fp8 precision: conv " + n.name + " needs channel counts and slice offsets that are multiples of 16");
            if (n.res >= 0 && !s.in2.f8) fail("fp8 precision: the shortcut of conv " + n.name + " is not an fp8 tensor");
            s.algo = ConvAlgo::IgemmF8;
        }
    }
    s.tile = choose_tile(f.M, f.N);
    s.splitk = 1;
    s.base_tile = s.tile;
}

// fp8 steps: IE_FORCE_TILE names a tile of the tiled kernel or one of the weights-stationary kernels
void Planner::ForceTileF8(const ConvFacts& f, Step& s) const {
    const int t = ForcedTile(INT_MAX);
    if (t >= 0 && t < kNumIgemmBaseTiles && !(kIgemmTiles[t].bn > 32 && f.N <= 32)) s.tile = t;
    // kWs8Code + t: the weights-stationary 1x1 kernel's tiles, kWs38Code + t: the 3x3's (kernels_ws8.hip); a launcher that
    // declines the operands hands the step back to the tiled kernel (executor)
    if (t >= kWs8Code && t < kWs8Code + kNumConvWs8Tiles && f.n.kh == 1 && f.n.kw == 1) s.tile = t;      // (strided 1x1 convs too: the kernel's STR form)
    if (t >= kWs38Code && t < kWs38Code + kNumConvWs38Tiles && f.is3x3) s.tile = t;
}

namespace {
// ---- default choice without the autotuner (IE_AUTOTUNE=0, or before Prepare() has timed anything): the kernels
//      the exhaustive search picks for DenseNet / ResNet shapes ----
void PickDefaultKernel(const ConvFacts& f, Step& s) {
    int pick = -1;
    if (f.M <= 2048) {                                                       // tiny grids: split K over the waves
        if (f.is3x3 && f.direct_ok(6)) pick = 6;                             // 16-pixel window tiles: 4x the workgroups
        else if (f.is1x1 && f.direct_ok(13)) pick = 13;                      // 16-pixel activations-stationary tiles
        for (int t : {1, 0, 4, 3}) if (pick < 0 && f.direct_ok(t)) pick = t;
        if (pick >= 0) { s.algo = ConvAlgo::Direct; s.tile = pick; }
    } else if (f.in16) {
        if (f.is1x1) { for (int t : {0, 2, 4}) if (pick < 0 && f.ws16_ok(t)) pick = t; if (pick >= 0) { s.algo = ConvAlgo::Ws1x1; s.tile = pick; } }
        else if (f.is3x3) { for (int t : {2, 1, 0}) if (pick < 0 && f.ws3_ok(t)) pick = t; if (pick >= 0) { s.algo = ConvAlgo::Ws3x3; s.tile = pick; } }
    } else {
        if (f.is1x1 && f.direct_ok(10)) { s.algo = ConvAlgo::Direct; s.tile = 10; }      // activations-stationary 1x1: 128-channel multiples whose 32 pixel rows fit in LDS
        else if (f.is1x1 && f.M >= 20000) { for (int t : {0, 2, 4}) if (pick < 0 && f.ws32_ok(t)) pick = t; if (pick >= 0) { s.algo = ConvAlgo::Ws1x1; s.tile = pick; } }
        else if (f.wino_ok() && f.M >= 20000) { s.algo = ConvAlgo::Wino3x3; s.tile = 5; }     // Winograd F(2x2,3x3), 2x14 tiles, eight waves (falls back to the tiled kernel without the U mirror)
        else if (f.raster_ok() && f.M >= 20000 && f.N <= 64) { s.algo = ConvAlgo::Raster3x3; s.tile = f.N <= 32 ? 0 : 4; }
        else if (f.is3x3 && f.M <= 8192) { if (f.direct_ok(4)) { s.algo = ConvAlgo::Direct; s.tile = 4; } }
    }
}
}  // namespace

// Test / tuning override (read at plan time): IE_FORCE_ALGO=naive|scalar|igemm|raster|ws|direct|x6|wino; ws, direct, x6, wino and raster read
// IE_FORCE_TILE as an index into their own tile tables
void Planner::ApplyForcedAlgo(const ConvFacts& f, Step& s) const {
    const LNode& n = f.n;
    const char* fa = env.get("IE_FORCE_ALGO");
    if (fa && f.dil && std::string(fa) != "naive" && std::string(fa) != "scalar" && std::string(fa) != "igemm") fa = nullptr;
    if (fa) {
        const std::string word = fa;
        if (word == "naive") s.algo = ConvAlgo::Naive;
        else if (word == "scalar" && f.K <= 2048 && !f.in16) s.algo = ConvAlgo::IgemmScalar;
        else if (word == "igemm" && s.algo == ConvAlgo::Stem) s.algo = f.K <= 2048 ? ConvAlgo::IgemmScalar : ConvAlgo::Naive;
        else if (word == "igemm" && s.algo == ConvAlgo::Naive) s.algo = f.tiled_algo();
        else if (word == "ws") {
            const int t = std::max(0, ForcedTile(f.in16 ? kNumConvWs16Tiles : kNumConvWs32Tiles));
            if (f.ws16_ok(t) || f.ws32_ok(t)) { s.algo = ConvAlgo::Ws1x1; s.tile = t; }
            else if (f.ws3_ok(t % kNumConvWs3Tiles)) { s.algo = ConvAlgo::Ws3x3; s.tile = t % kNumConvWs3Tiles; }
            else if (s.algo == ConvAlgo::Naive && f.vec16_ok) s.algo = ConvAlgo::IgemmVec;
        }
        else if (word == "direct") {
            const int t = std::max(0, ForcedTile(kNumConvDirectTiles));
            if (f.direct_ok(t)) { s.algo = ConvAlgo::Direct; s.tile = t; }
            else if (s.algo == ConvAlgo::Naive && (f.vec_ok || f.vec16_ok)) s.algo = ConvAlgo::IgemmVec;
        }
        else if (word == "x6") {
            const bool x6_ok = f.vec_ok && !s.out.f16 && f.is1x1 && n.sh == 1 && n.sw == 1 && s.in.c % 32 == 0 && f.N % 128 == 0 && n.res < 0;
            if (x6_ok) {
                s.algo = ConvAlgo::X6;
                s.tile = std::max(0, ForcedTile(kNumConvX6Tiles));
            }
        }
        else if (word == "wino") {
            if (f.wino_ok()) {
                s.algo = ConvAlgo::Wino3x3;
                s.tile = std::max(0, ForcedTile(kNumConvWinoTiles));
            } else if (s.algo == ConvAlgo::Naive) s.algo = f.tiled_algo();
        }
        else if (word == "raster") {
            if (f.raster_ok()) {
                s.algo = ConvAlgo::Raster3x3;
                s.tile = std::max(0, ForcedTile(kNumConvRasterTiles));
            } else if (s.algo == ConvAlgo::Naive) s.algo = f.tiled_algo();
        }
    }
}

// IE_FORCE_TILE on the tiled implicit GEMMs, then split-K: the heuristic, or IE_FORCE_SPLITK
void Planner::ApplyForcedTileAndSplitK(const ConvFacts& f, Step& s) {
    const LNode& n = f.n;
    const int heuristic_tile = s.base_tile;
    // the specialised kernels read IE_FORCE_TILE through their own tables (ApplyForcedAlgo) or not at all
    const bool own_tiles = s.algo == ConvAlgo::Raster3x3 || s.algo == ConvAlgo::Ws1x1 || s.algo == ConvAlgo::Ws3x3 || s.algo == ConvAlgo::Stem || s.algo == ConvAlgo::Direct || s.algo == ConvAlgo::Wino3x3 || s.algo == ConvAlgo::X6;
    const int t = own_tiles ? -1 : ForcedTile(kNumIgemmTiles);
    if (t >= 0 && (t < kNumIgemmBaseTiles || (s.algo == ConvAlgo::IgemmVec && !f.dil)) && !(f.in16 && kIgemmTiles[t].deep)) s.tile = t;
    if (s.algo != ConvAlgo::IgemmVec && s.algo != ConvAlgo::Raster3x3 && s.algo != ConvAlgo::Ws1x1 && s.algo != ConvAlgo::Ws3x3 && s.algo != ConvAlgo::Direct && s.algo != ConvAlgo::Wino3x3 && s.algo != ConvAlgo::X6 && s.tile >= kNumIgemmBaseTiles)
        s.tile = heuristic_tile;       // K-group tiles exist for the vector path only
    if (s.algo == ConvAlgo::Raster3x3) {
        if (const char* fs = env.get("IE_FORCE_SPLITK")) {
            int v = std::atoi(fs);
            if (v >= 1 && v <= 64) s.splitk = v;
        }
        if (s.splitk > 1) plan.workspace_floats = std::max<int64_t>(plan.workspace_floats, int64_t(s.splitk) * f.M * f.N);
    } else if (s.algo == ConvAlgo::Ws1x1 || s.algo == ConvAlgo::Ws3x3 || s.algo == ConvAlgo::Stem || s.algo == ConvAlgo::Direct || s.algo == ConvAlgo::Wino3x3 || s.algo == ConvAlgo::X6) {
        s.splitk = 1;
    } else if (s.algo != ConvAlgo::Naive) {
        // split-K when the output grid cannot fill the chip: aim for >= ~768 workgroups, keep >= 2 K-tiles
        // per split.  (Deterministic two-pass reduction, see kernels.hip.)
        const IgemmTile& T = kIgemmTiles[s.tile];
        const int64_t bk = f.in16 ? 2 * kIgemmBK : kIgemmBK;       // K-tile depth in elements (128 B per LDS row either way)
        const int64_t wgs = ((f.M + T.bm - 1) / T.bm) * ((f.N + T.bn - 1) / T.bn);
        const int64_t cblocks = (s.in.c + bk - 1) / bk;
        const int64_t KT = s.algo == ConvAlgo::IgemmVec ? int64_t(n.kh) * n.kw * cblocks : (f.K + kIgemmBK - 1) / kIgemmBK;
        if (wgs < 384 && KT >= 4) {
            int64_t want = (768 + wgs - 1) / wgs;
            s.splitk = int(std::max<int64_t>(1, std::min<int64_t>({want, KT / 2, 32})));
        }
        if (const char* fs = env.get("IE_FORCE_SPLITK")) {
            int v = std::atoi(fs);
            if (v >= 1 && v <= 64) s.splitk = v;
        }
        if (s.splitk > 1) plan.workspace_floats = std::max<int64_t>(plan.workspace_floats, int64_t(s.splitk) * f.M * f.N);
    }
}

void Planner::EmitConv(const LNode& n, Step& s) {
    s.kind = StepKind::Conv;
    s.kh = n.kh; s.kw = n.kw; s.sh = n.sh; s.sw = n.sw; s.pt = n.pt; s.pl = n.pl; s.pb = n.pb; s.pr = n.pr;
    s.dh = n.dil_h; s.dw = n.dil_w;
    s.w_off = push_vec(n.w);
    if (!n.bias.empty()) s.bias_off = push_vec(n.bias);
    if (n.res >= 0) { s.in2 = view_of(n.res); s.has_in2 = true; }
    if (n.transposed) { EmitTransposedConv(n, s); return; }
    if (n.dw || n.group != 1) { EmitGroupConv(n, s); return; }
    const ConvFacts f(n, s);
    s.flops = 2.0 * double(f.M) * double(f.N) * double(f.K);
    s.bytes = vbytes(s.in) + vbytes(s.out) + (f.in8 ? 1.0 : (f.in16 ? 2.0 : 4.0)) * double(n.w.size()) + (n.res >= 0 ? vbytes(s.in2) : 0.0);
    ChooseBaseAlgo(f, s);
    if (s.algo == ConvAlgo::IgemmF8) { ForceTileF8(f, s); return; }
    if (!env.get("IE_FORCE_ALGO") && !env.get("IE_FORCE_TILE") && s.algo == ConvAlgo::IgemmVec) PickDefaultKernel(f, s);
    ApplyForcedAlgo(f, s);
    ApplyForcedTileAndSplitK(f, s);
}

void Planner::EmitPool(const LNode& n, Step& s) const {
    if (n.kind == L_GAP) {
        if (s.in.f8 && (n.has_pre || s.out.f8)) fail("fp8 precision: global pool " + n.name + " with a prologue is not supported");
        s.kind = StepKind::GlobalAvgPool;
        s.pre_act = n.pre_act;
        s.bytes = vbytes(s.in) + vbytes(s.out);
        s.flops = double(s.in.numel()) * (1.0 + ActFlops(n.pre_act.kind));
        return;
    }
    if ((s.in.f8 || s.out.f8) && (!s.in.f8 || !s.out.f8 || n.has_pre || s.in.c % 16 || s.in.pitch % 16 || s.in.c_off % 16 || s.out.pitch % 16 || s.out.c_off % 16))
        fail("fp8 precision: pool " + n.name + " needs fp8 operands without a prologue and channel counts that are multiples of 16");
    s.kind = StepKind::Pool;
    s.pool_max = n.kind == L_MAXPOOL;
    s.count_include_pad = n.count_include_pad;
    s.kh = n.kh; s.kw = n.kw; s.sh = n.sh; s.sw = n.sw; s.pt = n.pt; s.pl = n.pl; s.pb = n.pb; s.pr = n.pr;
    s.bytes = vbytes(s.in) + vbytes(s.out);
    s.flops = double(s.out.numel()) * n.kh * n.kw;
}

void Planner::EmitSqueezeExcite(const LNode& n, Step& s) {
    s.kind = StepKind::SqueezeExcite;
    s.w_off = push_vec(n.w);
    if (!n.bias.empty()) s.bias_off = push_vec(n.bias);
    s.w2_off = push_vec(n.w2);
    if (!n.bias2.empty()) s.bias2_off = push_vec(n.bias2);
    s.se_mid = n.se_mid;
    s.se_act1 = n.se_act1;
    s.act = n.act;
    s.se_chunks = SeSqueezeChunks(s.in.n, s.in.h * s.in.w);
    plan.workspace_floats = std::max<int64_t>(plan.workspace_floats, SeWorkspaceFloats(s.in.n, s.in.c, n.se_mid, s.se_chunks));
    // squeeze (one add per element), the two FCs (2 x MACs, activations), the gate multiply; the input is read twice
    const double nc = double(s.in.n) * double(s.in.c), nm = double(s.in.n) * n.se_mid;
    s.flops = double(s.in.numel()) + 4.0 * nc * n.se_mid + nm * ActFlops(n.se_act1.kind) + nc * ActFlops(n.act.kind) + double(s.out.numel());
    s.bytes = 2.0 * vbytes(s.in) + vbytes(s.out) + 4.0 * double(n.w.size() + n.w2.size() + n.bias.size() + n.bias2.size());
}

// the stand-alone pointwise steps: activation, gate multiply, scale/shift, Clip, Relu, Add
void Planner::EmitEltwise(const LNode& n, Step& s) {
    s.kind = StepKind::Eltwise;
    switch (n.kind) {
        case L_ACT:
            s.act = n.act;
            s.bytes = vbytes(s.in) + vbytes(s.out);
            s.flops = double(s.in.numel()) * ActFlops(n.act.kind);
            break;
        case L_MUL:
            s.in2 = view_of(n.in[1]);
            s.has_in2 = true;
            s.mul = true;
            s.pre_act = n.pre_act;             // (a gated unit: act(in) * in2)
            s.bytes = vbytes(s.in) + vbytes(s.in2) + vbytes(s.out);
            s.flops = double(s.out.numel()) * (1.0 + (n.pre_act.kind != ActKind::None ? ActFlops(n.pre_act.kind) : 0.0));
            break;
        case L_AFFINE:
            if (s.in.f8 || s.out.f8) fail("fp8 precision: stand-alone scale/shift " + n.name + " on an fp8 tensor is not supported");
            s.pre_scale_off = push_vec(n.s);
            s.pre_shift_off = push_vec(n.t);
            s.bytes = vbytes(s.in) + vbytes(s.out);
            s.flops = 2.0 * double(s.in.numel());
            break;
        case L_CLIP:
            if (s.in.f8 || s.out.f8) fail("fp8 precision: stand-alone Clip " + n.name + " on an fp8 tensor is not supported");
            s.lo = n.lo;
            s.hi = n.hi;
            s.bytes = vbytes(s.in) + vbytes(s.out);
            s.flops = 2.0 * double(s.in.numel());
            break;
        case L_RELU:
            if (s.in.f8 || s.out.f8) fail("fp8 precision: stand-alone Relu " + n.name + " on an fp8 tensor is not supported");
            s.relu = true;
            s.bytes = vbytes(s.in) + vbytes(s.out);
            break;
        default:      // L_ADD
            if (s.in.f8 || s.out.f8) fail("fp8 precision: stand-alone Add " + n.name + " on fp8 tensors is not supported (only shortcuts folded into a conv)");
            s.in2 = view_of(n.in[1]);
            s.has_in2 = true;
            s.bytes = vbytes(s.in) + vbytes(s.in2) + vbytes(s.out);
            s.flops = double(s.in.numel());
            break;
    }
}

void Planner::EmitResize(const LNode& n, Step& s) const {
    s.kind = StepKind::Resize;
    s.rs_mode = n.rs_mode;
    s.rs_coord = n.rs_coord;
    s.rs_nearest = n.rs_nearest;
    s.rs_scale_h = n.rs_sh;
    s.rs_scale_w = n.rs_sw;
    s.bytes = vbytes(s.in) + vbytes(s.out);
    s.flops = n.rs_mode == ResizeMode::Linear ? 6.0 * double(s.out.numel()) : 0.0;    // two lerps per axis pair: 3 FMA-equivalents
}

// layer norm: gamma at w_off, beta at bias_off (fp32 in every precision); the tile is the smallest lane group that holds the row in three 16-byte
// vectors per lane (kernels.h LnDefaultTile), IE_FORCE_TILE picks among the eligible ones (an ineligible one: the generic kernel)
void Planner::EmitLayerNorm(const LNode& n, Step& s) {
    if (s.in.f8 || s.out.f8) fail(std::string(n.rms ? "RMSNormalization" : "LayerNormalization") + " is not supported in fp8 mode (node " + n.name + ")");
    s.kind = StepKind::LayerNorm;
    s.w_off = push_vec(n.s);
    if (!n.t.empty()) s.bias_off = push_vec(n.t);
    s.ln_eps = n.eps;
    s.rms = n.rms;
    const int def = LnDefaultTile(s.in.c, s.out.f16);
    s.tile = def > 0 && LnFastViews(s, def) ? def : 0;
    const int t = ForcedTile(kNumLnTiles);
    if (t >= 0) s.tile = t == 0 || LnFastViews(s, t) ? t : 0;
    s.flops = (n.rms ? 4.0 : 8.0) * double(s.in.numel());
    s.bytes = vbytes(s.in) + vbytes(s.out);
}

// Group-norm steps: the views tile 1 needs.  Not VecView: the vector terms are GnTileFits's (the input's channel count stands for both), and neither
// e4m3 nor int64 operands
static bool GnFastViews(const Step& s, int tile) {
    return !s.in.nchw && !s.out.nchw && !s.in.f8 && !s.out.f8 && !s.in.i64 && !s.out.i64 && s.in.f16 == s.out.f16 &&
           GnTileFits(s.in.c, s.gn_groups, s.out.f16, s.in.pitch, s.in.c_off, s.out.pitch, s.out.c_off, int(s.act.kind), tile);
}

// group norm: gamma at w_off, beta at bias_off (fp32 in every precision).  Tile 1 (statistics + apply) where kernels.h GnTileFits admits the views and the
// group is large enough to pay for a second launch (GnDefaultTile), else the generic kernel; IE_FORCE_TILE as for layer norm, IE_GN_TILE the same for
// the group norms alone.  Tile 1's records live in the workspace
void Planner::EmitGroupNorm(const LNode& n, Step& s) {
    if (s.in.f8 || s.out.f8) fail("GroupNormalization is not supported in fp8 mode (node " + n.name + ")");
    s.kind = StepKind::GroupNorm;
    s.w_off = push_vec(n.s);
    s.bias_off = push_vec(n.t);
    s.ln_eps = n.eps;
    s.gn_groups = n.gn_groups;
    s.act = n.act;
    const int64_t hw = s.in.h * s.in.w;
    s.tile = GnFastViews(s, 1) ? GnDefaultTile(s.in.n, hw, s.in.c, s.gn_groups) : 0;
    int t = ForcedTile(kNumGnTiles);
    if (const char* e = env.get("IE_GN_TILE"); e && t < 0 && std::atoi(e) >= 0 && std::atoi(e) < kNumGnTiles) t = std::atoi(e);      // (the group norms alone)
    if (t >= 0) s.tile = t == 0 || GnFastViews(s, t) ? t : 0;
    if (s.tile == 1) plan.workspace_floats = std::max<int64_t>(plan.workspace_floats, GnWorkspaceFloats(s.in.n, hw, s.in.c, s.gn_groups, s.out.f16));
    s.flops = 8.0 * double(s.in.numel());
    // tile 1 reads the input twice (statistics, apply), the generic kernel three times (sum, centred squares, apply)
    s.bytes = (s.tile == 1 ? 2.0 : 3.0) * vbytes(s.in) + vbytes(s.out);
}

// embed: the tables, the position rows, gamma and beta fp32 in the blob (in that order); the tile as for layer norm, by kernels.h EmbedTileFits
void Planner::EmitEmbed(const LNode& n, Step& s) {
    if (s.out.f8) fail("LayerNormalization is not supported in fp8 mode (node " + n.name + ")");
    s.kind = StepKind::Embed;
    if (n.in.size() > 1) { s.in2 = view_of(n.in[1]); s.has_in2 = true; }
    if (!s.in.i64 || (s.has_in2 && !s.in2.i64) || s.out.nchw) fail("internal planner error: embed views of node " + n.name);
    s.emb_vocab = n.emb_vocab;
    s.emb_types = n.emb_types;
    s.w_off = push_vec(n.w);
    if (!n.w2.empty()) s.w2_off = push_vec(n.w2);
    if (!n.bias.empty()) s.emb_pos_off = push_vec(n.bias);
    if (!n.s.empty()) s.bias_off = push_vec(n.s);      // (empty: the sum without a LayerNormalization)
    if (!n.t.empty()) s.bias2_off = push_vec(n.t);
    s.ln_eps = n.eps;
    s.tile = EmbedDefaultTile(s.out.c, s.out.f16, s.out.pitch, s.out.c_off);
    const int t = ForcedTile(kNumEmbedTiles);
    if (t >= 0) s.tile = t == 0 || EmbedTileFits(s.out.c, s.out.f16, s.out.pitch, s.out.c_off, t) ? t : 0;
    const double rows = double(s.out.n) * double(s.out.w), D = double(s.out.c);
    s.flops = (n.s.empty() ? 2.0 : 8.0) * rows * D;
    // per token row: one fp32 row of every table and of the position rows, the ids, the result once
    s.bytes = rows * (4.0 * D * double(1 + (s.has_in2 ? 1 : 0) + (s.emb_pos_off >= 0 ? 1 : 0)) + 8.0 * double(s.has_in2 ? 2 : 1)) + vbytes(s.out);
}

// token assemble: the class token at w_off, the position embedding at bias_off (fp32 in every precision)
void Planner::EmitTokenAssemble(const LNode& n, Step& s) {
    if (s.in.f8 || s.out.f8) fail("attention and token views are not supported in fp8 mode (node " + n.name + ")");
    s.kind = StepKind::TokenAssemble;
    s.w_off = push_vec(n.s);
    if (!n.t.empty()) s.bias_off = push_vec(n.t);
    s.flops = n.t.empty() ? 0.0 : double(s.out.numel());
    s.bytes = vbytes(s.in) + vbytes(s.out);
}

// attention: kernels.h AttnDefaultTile (tile 1, the MFMA kernel, where AttnMfmaFits says so; tile 2, the streaming kernel, on a wide head with
// at least kAttnStreamMinTokens tokens; else the generic kernel).  A causal step: AttnCausalDefaultTile (tile 1, else tile 3, the chunk kernel, else
// tile 2's causal form on a wide head with at least kAttnStreamCausalMinTokens tokens, else the generic kernel).  IE_FORCE_TILE as for layer norm but over tiles 0 and 1 only; IE_ATTN_TILE pins the attention steps alone, tiles 2 and 3
// included (an ineligible value is the generic kernel); a non-causal step reaches tile 3 this way only
// kv_append (kernels_decode.hip): the K half of a pair; EmitSteps adds the V half.  The rope tables go into the blob once per model (rope_blob): every
// layer gathers the same ones
void Planner::EmitKvAppend(const LNode& n, Step& s) {
    if (s.in.f8) fail("attention and token views are not supported in fp8 mode (node " + n.name + ")");
    s.kind = StepKind::KvAppend;
    s.heads = n.heads;
    s.head_dim = n.head_dim;
    s.kv_heads = n.kv_heads;
    s.past_len = n.past_len;
    s.present_k = s.out;
    if (!s.out.nchw || s.out.f16) fail("internal planner error: the present output of node " + n.name + " is not a dense fp32 graph output");
    if (n.past_in >= 0) s.past_k = view_of(n.in[size_t(n.past_in)]);
    if (!n.w.empty()) {
        auto table = [&](const std::vector<float>& t) {
            const auto it = rope_blob.find(t);
            return it != rope_blob.end() ? it->second : (rope_blob[t] = push_vec(t));
        };
        s.rope = true;
        s.w_off = table(n.w);
        s.w2_off = table(n.w2);
        s.rope_rows = n.rope_rows;
        if (n.pos_in >= 0) {
            s.pos = view_of(n.in[size_t(n.pos_in)]);
            if (!s.pos.i64) fail("internal planner error: the positions of node " + n.name + " are not an int64 view");
        }
    }
    s.bytes = vbytes(s.present_k) + (n.past_in >= 0 ? vbytes(s.past_k) : 0.0) + double(s.in.n) * double(s.in.w) * 2.0 * double(n.kv_heads) * double(n.head_dim) * double(s.in.esize());
}

void Planner::EmitAttention(const LNode& n, Step& s) {
    if (s.in.f8 || s.out.f8) fail("attention and token views are not supported in fp8 mode (node " + n.name + ")");
    s.kind = StepKind::Attention;
    s.heads = n.heads;
    s.head_dim = n.head_dim;
    s.attn_scale = float(n.attn_scale);
    if (n.past_len > 0) {
        // a decode step: one query per head over the past_len + 1 rows of `present`.  Tile 4 where kernels.h DecodeFastFits says so, else the parts;
        // IE_ATTN_TILE = 0 | 4 pins it (an ineligible 4 is the parts), IE_ATTN_SPLITS the key splits of tile 4.  No other tile takes a past
        s.past_len = n.past_len;
        s.kv_heads = n.kv_heads > 0 ? n.kv_heads : n.heads;
        s.present_k = view_of(n.in[size_t(n.present_in)]);
        s.present_v = view_of(n.in[size_t(n.present_in) + 1]);
        if (n.key_mask) {
            s.in2 = view_of(n.in[1]);
            s.has_in2 = true;
            s.key_mask = true;
            s.mask_value = n.mask_value;
            if (!s.in2.i64) fail("internal planner error: the key mask of node " + n.name + " is not an int64 view");
        }
        s.rope = !n.w.empty();
        if (n.chunk_causal) {
            // an extend step: in.w = Lq >= 2 new tokens, token i over the past_len + i + 1 rows of `present` it may see.  Tile 5 where kernels.h
            // ExtendFastFits says so and there are at least kAttnExtendMinRows query rows per K / V head, else the parts; IE_ATTN_TILE = 0 | 5 pins it (an
            // ineligible 5 is the parts), IE_ATTN_SPLITS the key splits of tile 5 (at most one 32-key tile per split).  No other tile takes it
            s.chunk_causal = true;
            const int64_t rows = int64_t(s.heads / s.kv_heads) * s.in.w, keys = int64_t(n.past_len) + s.in.w;
            const bool fits = !s.in.nchw && !s.out.nchw && s.in.f16 == s.out.f16 && ExtendFastFits(s.head_dim, s.heads, s.kv_heads, n.key_mask, n.mask_value);
            s.tile = fits && rows >= kAttnExtendMinRows ? kAttnExtendTile : 0;
            if (const char* e = env.get("IE_ATTN_TILE"); e && (std::atoi(e) == 0 || std::atoi(e) == kAttnExtendTile)) s.tile = std::atoi(e) == kAttnExtendTile && fits ? kAttnExtendTile : 0;
            if (ForcedTile(kNumAttnForcedTiles) >= 0) s.tile = 0;
            if (s.tile == kAttnExtendTile) {
                s.splits = ExtendDefaultSplits(s.in.n, s.kv_heads, rows, keys);
                if (const int f = env.integer("IE_ATTN_SPLITS", 0); f >= 1) s.splits = int(std::min<int64_t>(std::min(f, kDecodeMaxSplits), (keys + 31) / 32));
                plan.workspace_floats = std::max<int64_t>(plan.workspace_floats, ExtendWorkspaceFloats(s.in.n, s.heads, s.head_dim, s.splits, s.in.w));
            }
            s.flops = 2.0 * double(s.in.n) * double(s.heads) * double(s.in.w) * double(2 * n.past_len + s.in.w + 1) * double(s.head_dim);      // (the visible keys: the work needed)
            s.bytes = vbytes(s.in) + vbytes(s.out) + vbytes(s.in2);
            return;
        }
        const int64_t keys = int64_t(n.past_len) + 1;
        const bool fits = !s.in.nchw && !s.out.nchw && DecodeFastFits(s.head_dim, s.heads, s.kv_heads, n.key_mask, n.mask_value);
        s.tile = fits && keys >= kAttnDecodeMinKeys ? kAttnDecodeTile : 0;
        if (const char* e = env.get("IE_ATTN_TILE"); e && (std::atoi(e) == 0 || std::atoi(e) == kAttnDecodeTile)) s.tile = std::atoi(e) == kAttnDecodeTile && fits ? kAttnDecodeTile : 0;
        if (ForcedTile(kNumAttnForcedTiles) >= 0) s.tile = 0;      // (IE_FORCE_TILE pins generic kernels everywhere: a decode step's are its parts)
        if (s.tile == kAttnDecodeTile) {
            s.splits =DecodeDefaultSplits(s.in.n, s.kv_heads, keys, s.head_dim);
            if (const int f = env.integer("IE_ATTN_SPLITS", 0); f >= 1) s.splits = int(std::min<int64_t>(std::min(f, kDecodeMaxSplits), (keys + DecodeKeyTile(s.head_dim) - 1) / DecodeKeyTile(s.head_dim)));
            plan.workspace_floats = std::max<int64_t>(plan.workspace_floats, DecodeWorkspaceFloats(s.in.n, s.heads, s.head_dim, s.splits));
        }
        s.flops = 4.0 * double(s.in.n) * double(s.heads) * double(keys) * double(s.head_dim);
        s.bytes = vbytes(s.in) + vbytes(s.out) + (n.key_mask ? vbytes(s.in2) : 0.0);      // (the cache traffic is counted on the kv_append part)
        return;
    }
    if (n.key_mask) {
        s.in2 = view_of(n.in[1]);
        s.has_in2 = true;
        s.key_mask = true;
        s.mask_value = n.mask_value;
        if (!s.in2.i64) fail("internal planner error: the key mask of node " + n.name + " is not an int64 view");
    }
    s.causal = n.causal;
    s.kv_heads = n.kv_heads > 0 ? n.kv_heads : n.heads;
    const bool rope = !n.w.empty();
    if (rope) {                                        // the cos / sin tables [L][hd], fp32 in every precision (push_vec aligns them to 32 bytes)
        s.rope = true;
        s.w_off = push_vec(n.w);
        s.w2_off = push_vec(n.w2);
    }
    // a rotary step runs on tiles 1 / 3 (head dims 32 / 64) and tile 2 (head dims 128 / 256) in their causal form only; non-causal rope, a rotary head
    // of 512 and every other head dim: the generic kernel.  Grouped K / V heads are a run-time property of every tile
    const bool views = !s.in.nchw && !s.out.nchw && s.in.f16 == s.out.f16 && !(rope && !n.causal);
    auto fits = [&](int tile) {
        if (tile == 0) return true;
        if (tile == 2 && rope && s.head_dim != 128 && s.head_dim != 256) return false;      // (tile 2 has no rotary form at hd 512)
        if (tile == 3) return views && AttnChunkFits(s.in.w, s.head_dim, s.out.f16, s.in.c, s.in.pitch, s.in.c_off, s.out.c, s.out.pitch, s.out.c_off, n.key_mask);
        return views && (tile == 1 ? AttnMfmaFits(s.in.w, s.head_dim, s.out.f16, s.in.c, s.in.pitch, s.in.c_off, s.out.c, s.out.pitch, s.out.c_off, n.key_mask)
                                   : AttnStreamFits(s.in.w, s.head_dim, s.out.f16, s.in.c, s.in.pitch, s.in.c_off, s.out.c, s.out.pitch, s.out.c_off, n.key_mask));
    };
    s.tile = views ? AttnDefaultTile(s.in.w, s.head_dim, s.out.f16, s.in.c, s.in.pitch, s.in.c_off, s.out.c, s.out.pitch, s.out.c_off, n.key_mask) : 0;
    if (n.causal) s.tile = views ? AttnCausalDefaultTile(s.in.w, s.head_dim, s.out.f16, s.in.c, s.in.pitch, s.in.c_off, s.out.c, s.out.pitch, s.out.c_off) : 0;
    if (s.tile == 2 && !fits(2)) s.tile = 0;
    int t = ForcedTile(kNumAttnForcedTiles);
    if (const char* e = env.get("IE_ATTN_TILE"); e && t < 0 && std::atoi(e) >= 0 && std::atoi(e) < kNumAttnTiles) t = std::atoi(e);      // (the attention steps alone)
    if (t >= 0) s.tile = fits(t) ? t : 0;
    s.flops = 4.0 * double(s.in.n) * double(s.heads) * double(s.in.w) * double(s.in.w) * double(s.head_dim);
    if (n.causal) s.flops = 2.0 * double(s.in.n) * double(s.heads) * double(s.in.w) * double(s.in.w + 1) * double(s.head_dim);      // the lower triangle: the work needed
    s.bytes = vbytes(s.in) + vbytes(s.out) + (n.key_mask ? vbytes(s.in2) : 0.0) + (rope ? 8.0 * double(s.in.w) * double(s.head_dim) : 0.0);
}

// window attention: the bias and the mask packed for the kernels (kernels.h WinAttnArgs: [.][Lp][Lp], the query index fastest, -inf in the bias
// rows of the padded keys), fp32 in every precision; tile 1 (the MFMA kernel) where kernels.h WinAttnMfmaFits says so; IE_FORCE_TILE as for attention
void Planner::EmitWindowAttention(const LNode& n, Step& s) {
    if (s.in.f8 || s.out.f8) fail("window attention and patch merging are not supported in fp8 mode (node " + n.name + ")");
    s.kind = StepKind::WindowAttention;
    s.heads = n.heads;
    s.head_dim = n.head_dim;
    s.attn_scale = float(n.attn_scale);
    s.win_h = n.win_h; s.win_w = n.win_w; s.shift_h = n.shift_h; s.shift_w = n.shift_w;
    s.masked = n.masked;
    const int64_t Lw = int64_t(n.win_h) * n.win_w, Lp = WinAttnPaddedTokens(Lw), nW = (s.in.h / n.win_h) * (s.in.w / n.win_w);
    auto pack = [&](const std::vector<float>& t, int64_t count, float pad_key) {
        std::vector<float> p(size_t(count * Lp * Lp), 0.f);
        for (int64_t b = 0; b < count; ++b)
            for (int64_t j = 0; j < Lp; ++j)
                for (int64_t i = 0; i < Lp; ++i)
                    p[size_t((b * Lp + j) * Lp + i)] = j >= Lw ? pad_key : (i >= Lw ? 0.f : t[size_t((b * Lw + i) * Lw + j)]);
        return p;
    };
    if (int64_t(n.w.size()) != n.heads * Lw * Lw || (n.masked && int64_t(n.w2.size()) != nW * Lw * Lw)) fail("internal planner error: window-attention tables of node " + n.name);
    s.w_off = push_vec(pack(n.w, n.heads, -kInf));
    if (n.masked) s.w2_off = push_vec(pack(n.w2, nW, 0.f));
    const bool fits = !s.in.nchw && !s.out.nchw && s.in.f16 == s.out.f16 &&
                      WinAttnMfmaFits(Lw, s.head_dim, s.out.f16, s.in.c, s.in.pitch, s.in.c_off, s.out.c, s.out.pitch, s.out.c_off);
    s.tile = fits ? 1 : 0;
    const int t = ForcedTile(kNumWinAttnTiles);
    if (t >= 0) s.tile = t == 0 || fits ? t : 0;
    s.flops = 4.0 * double(s.in.n) * double(nW) * double(s.heads) * double(Lw) * double(Lw) * double(s.head_dim);
    s.bytes = vbytes(s.in) + vbytes(s.out) + 4.0 * double(Lp * Lp) * double(n.heads + (n.masked ? nW : 0));
}

void Planner::EmitPatchMerge(const LNode& n, Step& s) const {
    if (s.in.f8 || s.out.f8) fail("window attention and patch merging are not supported in fp8 mode (node " + n.name + ")");
    s.kind = StepKind::PatchMerge;
    s.bytes = vbytes(s.in) + vbytes(s.out);
}

// ---- emit steps --------------------------------------------------------------------------------
void Planner::EmitSteps() {
    for (int idx : order) {
        const LNode& n = L.nodes[idx];
        if (n.kind == L_ALIAS) continue;
        if (n.kind == L_CONCAT) { EmitConcatCopies(n); continue; }
        if (n.kind == L_KVAPPEND && n.kv_v) {          // the V half of a kv_append pair: one step with the K half in front of it
            if (plan.steps.empty() || plan.steps.back().kind != StepKind::KvAppend || plan.steps.back().present_v.buf >= 0) fail("internal planner error: kv_append pair of node " + n.name);
            Step& k = plan.steps.back();
            k.name += "+" + n.name;
            k.present_v = view_of(n.out);
            if (n.past_in >= 0) k.past_v = view_of(n.in[size_t(n.past_in)]);
            const double b = vbytes(k.present_v) + (n.past_in >= 0 ? vbytes(k.past_v) : 0.0);
            k.bytes += b;
            plan.total_bytes += b;
            writer[{int64_t(k.present_v.buf), k.present_v.c_off, k.present_v.c}] = int(plan.steps.size()) - 1;
            continue;
        }
        Step s;
        s.name = n.name;
        s.in = view_of(n.in[0]);
        s.out = view_of(n.out);
        s.relu = n.relu;
        if (n.has_pre) {
            s.pre_scale_off = push_vec(n.pre_s);
            s.pre_shift_off = push_vec(n.pre_t);
            s.pre_relu = n.pre_relu;
            s.pre_hi = n.pre_hi;
        }
        switch (n.kind) {
            case L_CONV: EmitConv(n, s); break;
            case L_MAXPOOL: case L_AVGPOOL: case L_GAP: EmitPool(n, s); break;
            case L_SE: EmitSqueezeExcite(n, s); break;
            case L_ACT: case L_MUL: case L_AFFINE: case L_CLIP: case L_RELU: case L_ADD: EmitEltwise(n, s); break;
            case L_RESIZE: EmitResize(n, s); break;
            case L_LAYERNORM: EmitLayerNorm(n, s); break;
            case L_TOKASM: EmitTokenAssemble(n, s); break;
            case L_ATTENTION: EmitAttention(n, s); break;
            case L_KVAPPEND: EmitKvAppend(n, s); break;
            case L_WATTN: EmitWindowAttention(n, s); break;
            case L_PATCHMERGE: EmitPatchMerge(n, s); break;
            case L_EMBED: EmitEmbed(n, s); break;
            case L_GROUPNORM: EmitGroupNorm(n, s); break;
            case L_COPY:
                if (s.in.f8 || s.out.f8) fail("fp8 precision: layout copy " + n.name + " of an fp8 tensor is not supported");
                s.kind = StepKind::Copy;
                s.bytes = vbytes(s.in) + vbytes(s.out);
                break;
            default: fail("internal planner error: unexpected node kind");
        }
        if (s.kind != StepKind::Conv && s.kind != StepKind::Copy && s.in.nchw)
            fail("internal planner error: NCHW view reached a non-conv step");
        if (s.kind == StepKind::Attention && s.past_len > 0) {
            // a decode step: the kv_append step in front of it becomes its first part, the attention over `present` its second (tile 0 = the parts)
            Step kv = std::move(plan.steps.back());
            plan.steps.pop_back();
            s.past_k = kv.past_k; s.past_v = kv.past_v;
            s.w_off = kv.w_off; s.w2_off = kv.w2_off; s.rope_rows = kv.rope_rows; s.pos = kv.pos;
            s.name = kv.name + "+" + s.name;
            Step at = s;
            at.name = n.name;
            at.tile = 0;
            at.splits = 0;
            s.parts = {std::move(kv), std::move(at)};
            writer[{int64_t(s.present_k.buf), s.present_k.c_off, s.present_k.c}] = int(plan.steps.size());
            writer[{int64_t(s.present_v.buf), s.present_v.c_off, s.present_v.c}] = int(plan.steps.size());
        }
        s.idx = int(plan.steps.size());
        s.in_src = src_of(s.in);
        if (s.has_in2) s.in2_src = src_of(s.in2);
        writer[{int64_t(s.out.buf), s.out.c_off, s.out.c}] = int(plan.steps.size());
        plan.total_flops += s.flops;
        plan.total_bytes += s.bytes;
        plan.steps.push_back(std::move(s));
    }
    while (plan.weights.size() % 8) plan.weights.push_back(0.f);
}

namespace {

// `steps` replaces the plan's step list: a step of algorithm `fused` stands for all of its parts.  idx, in_src / in2_src follow the new
// positions (a fused step is the producer of every output of its parts)
void ReplaceSteps(Plan& plan, std::vector<Step> steps, ConvAlgo fused) {
    if (steps.size() == plan.steps.size()) return;
    std::vector<int> remap(plan.steps.size(), -1);
    for (size_t k = 0; k < steps.size(); ++k) {
        if (steps[k].algo == fused) for (const Step& q : steps[k].parts) remap[size_t(q.idx)] = int(k);
        else remap[size_t(steps[k].idx)] = int(k);
    }
    for (size_t k = 0; k < steps.size(); ++k) {
        Step& st = steps[k];
        st.idx = int(k);
        if (st.in_src >= 0) st.in_src = remap[size_t(st.in_src)];
        if (st.in2_src >= 0) st.in2_src = remap[size_t(st.in2_src)];
    }
    plan.steps = std::move(steps);
}

}  // namespace

// ---- dense fusion (fp32, small output grids): 3x3 growth conv of layer L + the 1x1 bottleneck conv of layer L+1 ------------------
// Pattern: step i = plain 3x3/s1/p1 conv (no prologue, 32 output channels) writing a channel slice of a concat buffer; step i+1 =
// 1x1 conv with 128 output channels whose input view is that buffer's channels [c_off, slice end): its last 32 input channels are
// exactly what step i produces, for the same pixels (kernels_fused.hip).  Only where launches are latency-bound (M <= 8192).
void Planner::FuseDenseLayers() {
    std::vector<Step> fusedsteps;
    for (size_t i = 0; i < plan.steps.size(); ++i) {
        const Step& s3 = plan.steps[i];
        bool fuse = false;
        if (i + 1 < plan.steps.size()) {
            const Step& s1 = plan.steps[i + 1];
            const int64_t M = s3.out.n * s3.out.h * s3.out.w;
            fuse = s3.kind == StepKind::Conv && s1.kind == StepKind::Conv && !IsGroupConv(s3.algo) && !IsGroupConv(s1.algo) && s3.dh == 1 && s3.dw == 1 && s3.kh == 3 && s3.kw == 3 && s3.sh == 1 && s3.sw == 1 && s3.pt == 1 && s3.pl == 1 &&
                   s3.pb == 1 && s3.pr == 1 && s3.pre_scale_off < 0 && !s3.has_in2 && s3.out.c == 32 && s3.in.c % 16 == 0 && 9 * (s3.in.c / 16) <= 72 &&
                   9 * (s3.in.c / 16) >= 8 && s1.kh == 1 && s1.kw == 1 && s1.sh == 1 && s1.sw == 1 && s1.pt == 0 && s1.pl == 0 && s1.pb == 0 && s1.pr == 0 &&
                   !s1.has_in2 && s1.out.c == 128 && s1.in.buf == s3.out.buf && s1.in.pitch == s3.out.pitch && !s1.in.nchw && !s3.in.nchw &&
                   s1.in.c_off + s1.in.c == s3.out.c_off + s3.out.c && s1.in.c >= 48 && s1.in.c % 16 == 0 && s1.in.n == s3.out.n && s1.in.h == s3.out.h &&
                   s1.in.w == s3.out.w && s1.out.buf != s3.in.buf && M <= FuseMaxPixels(env) && s3.algo != ConvAlgo::Naive && s1.algo != ConvAlgo::Naive &&
                   s3.in.pitch % 4 == 0 && s3.in.c_off % 4 == 0 && s1.in.pitch % 4 == 0 && s1.in.c_off % 4 == 0 && s1.out.pitch % 4 == 0 && s1.out.c_off % 4 == 0;
            if (fuse) {
                int pb = M <= 2048 ? 1 : 2;
                int ftile = 0;
                if (const char* e = env.get("IE_FUSE_PB")) { const int v = std::atoi(e); if (v == 1 || v == 2) pb = v; if (v == 3) { pb = 1; ftile = 3; } if (v == 4 || v == 5) { pb = v - 3; ftile = v; } if (v == 6) { pb = 1; ftile = 6; } }
                const int64_t px = 16 * pb;
                const int64_t win = (px + 2 * s3.in.w + 2) * (s3.in.c + 8) * 4, part = 4 * px * 36 * 4;
                const int64_t c4n = (s1.in.c - 32) / 4, rpp = c4n > 0 && c4n <= 512 ? 512 / c4n : 0;
                if (std::max(px * (s1.in.c + 8) * 4, win) + part > 160 * 1024 || rpp == 0 || (px + rpp - 1) / rpp > (pb == 1 ? 8 : 16) ||
                    (px + 2 * s3.in.w + 2) * (s3.in.c / 4) > 8 * 512)
                    fuse = false;
                if (fuse) {
                    Step f = s1;
                    f.algo = ConvAlgo::DenseFused;
                    f.tile = ftile ? ftile : pb;
                    f.splitk = 1;
                    f.name = s3.name + " | " + s1.name;
                    f.flops = s3.flops + s1.flops;
                    f.bytes = s3.bytes + s1.bytes;
                    f.parts = {s3, s1};
                    fusedsteps.push_back(std::move(f));
                    ++i;
                }
            }
        }
        if (!fuse) fusedsteps.push_back(s3);
    }
    ReplaceSteps(plan, std::move(fusedsteps), ConvAlgo::DenseFused);
}

// One dense layer of a dense-block chain at steps i (the 1x1 conv) and i + 1 (the 3x3 conv): see FuseDenseBlocks
bool Planner::DenseLayerAt(size_t i) const {
    auto same_view = [](const View& a, const View& b) {
        return a.buf == b.buf && a.n == b.n && a.c == b.c && a.h == b.h && a.w == b.w && a.c_off == b.c_off && a.pitch == b.pitch && a.nchw == b.nchw && a.f16 == b.f16;
    };
    if (i + 1 >= plan.steps.size()) return false;
    const Step& s1 = plan.steps[i];
    const Step& s3 = plan.steps[i + 1];
    if (s1.kind != StepKind::Conv || s3.kind != StepKind::Conv || !s1.parts.empty() || !s3.parts.empty()) return false;
    if (IsGroupConv(s1.algo) || IsGroupConv(s3.algo)) return false;
    if (s1.kh != 1 || s1.kw != 1 || s1.sh != 1 || s1.sw != 1 || s1.pt || s1.pl || s1.pb || s1.pr || s1.has_in2 || s1.out.c != 128) return false;
    if (s3.kh != 3 || s3.kw != 3 || s3.sh != 1 || s3.sw != 1 || s3.pt != 1 || s3.pl != 1 || s3.pb != 1 || s3.pr != 1 || s3.has_in2 || s3.out.c != 32) return false;
    if (s3.dh != 1 || s3.dw != 1) return false;
    if (s3.pre_scale_off >= 0 || s1.w_off < 0 || s3.w_off < 0) return false;
    if (!s1.in.f16 || !s1.out.f16 || !s3.out.f16 || s1.in.nchw || s1.out.nchw || s3.out.nchw) return false;
    if (!same_view(s3.in, s1.out) || s3.out.buf != s1.in.buf || s3.out.pitch != s1.in.pitch || s1.out.buf == s1.in.buf) return false;
    if (s3.out.n != s1.in.n || s3.out.h != s1.in.h || s3.out.w != s1.in.w) return false;
    if (s1.in.c < 64 || s1.in.c % 32 || s1.in.pitch % 8 || s1.in.c_off % 8 || s3.out.c_off % 8) return false;
    if (s3.out.c_off < s1.in.c_off + s1.in.c && s3.out.c_off + 32 > s1.in.c_off) return false;
    if ((s1.pre_scale_off >= 0) != (s1.pre_shift_off >= 0)) return false;
    // up to 7 raster tiles: a workgroup per image (chains of layers); larger maps: bands of rows, one layer per launch, while at least one
    // row + halo fits the 8 staged tiles
    // Band mode measured no faster than the two streaming kernels at batch 128 (28x28: 39-58 vs 42-54 us per layer; 56x56: 160-218 vs 93-123 us:
    // the per-band fixed cost -- 72 KB of 3x3 weights into LDS, raster reset, epilogue -- is paid 5 ... 28 times per image), so such steps are
    // only formed on request (IE_DENSE_BAND=1: tests, experiments).
    const int64_t ntiles = (s1.in.h * (s1.in.w + 1) + 31) / 32;
    if (ntiles > 7 && (!env.flag("IE_DENSE_BAND") || (s1.in.w + 1 > 64 && 256 / (s1.in.w + 1) < 3))) return false;
    // T must have no other reader: the fused kernel never writes it to memory
    for (size_t j = i + 2; j < plan.steps.size(); ++j) {
        const Step& q = plan.steps[j];
        if (q.in.buf == s1.out.buf || (q.has_in2 && q.in2.buf == s1.out.buf)) return false;
        if (q.out.buf == s1.out.buf) break;                // the buffer was recycled for another tensor: T was dead by then (liveness pass)
    }
    return !output_in_buffer(s1.out.buf);
}

// ---- dense-block chains (fp16, small maps): consecutive dense layers of one concat buffer as ONE step ---------------------------------------
// Pattern per layer: step i = 1x1/s1 conv with 128 output channels reading channels [c_off, c_off + K) of a concat buffer into a bottleneck
// tensor T, step i+1 = plain 3x3/s1/p1 conv (no prologue, no residual) from T to 32 channels of the SAME concat buffer outside what the
// layer reads, T read by nothing else.  A layer touches only its own image, so a workgroup per image walks the whole chain with T in LDS
// (kernels_block.hip): DenseNet-121 blocks 3-4 at batch 128 go from 80 launches to 2.  Maps of at most 8 x 32 raster positions (14x14, 7x7).
void Planner::FuseDenseBlocks() {
    std::vector<Step> blocksteps;
    for (size_t i = 0; i < plan.steps.size();) {
        size_t n = 0;
        while (n < 24 && DenseLayerAt(i + 2 * n)) {
            if (n > 0) {
                if ((plan.steps[i].in.h * (plan.steps[i].in.w + 1) + 31) / 32 > 7) break;       // band mode: one layer per launch
                const Step& f1 = plan.steps[i], &c1 = plan.steps[i + 2 * n], &p3 = plan.steps[i + 2 * n - 1];
                if (c1.in.buf != f1.in.buf || c1.in.pitch != f1.in.pitch || c1.in.c_off != f1.in.c_off || c1.in.n != f1.in.n || c1.in.h != f1.in.h || c1.in.w != f1.in.w)
                    break;
                // a layer's first 192 input channels are requested while the previous layer's 3x3 still runs: they must not be its output
                if (p3.out.c_off < c1.in.c_off + 192 && p3.out.c_off + 32 > c1.in.c_off) break;
            }
            ++n;
        }
        if (n == 0) { blocksteps.push_back(plan.steps[i]); ++i; continue; }
        Step f = plan.steps[i];
        f.algo = ConvAlgo::DenseBlock;
        f.tile = 1;
        f.splitk = 1;
        f.flops = 0;
        f.bytes = 0;
        f.parts.clear();
        for (size_t q = 0; q < 2 * n; ++q) {
            const Step& ps = plan.steps[i + q];
            f.parts.push_back(ps);
            f.flops += ps.flops;
            f.bytes += ps.bytes;       // SURVEY §8d's per-conv accounting (the bottleneck tensor's write + read is in it although it stays on-chip here)
        }
        f.name = plan.steps[i].name + " ... " + plan.steps[i + 2 * n - 1].name;
        f.out = plan.steps[i + 2 * n - 1].out;             // what the step leaves in memory last (every part's slice is produced by this step)
        blocksteps.push_back(std::move(f));
        i += 2 * n;
    }
    ReplaceSteps(plan, std::move(blocksteps), ConvAlgo::DenseBlock);
}

// ---- stem + max pool: the 7x7/s2 stem conv and the 3x3/s2/p1 max pool behind it -> ONE step -------------------------------------
// Pattern: step i = the stem conv (algo Stem, ReLU'd), step i + 1 = a max pool 3x3 / stride 2 / pad 1 without a prologue that
// reads exactly step i's output, which nothing else reads.  conv_stem_kernel<POOL> (kernels_stem.hip) pools the conv tile in LDS: the tensor
// between the two ops (the largest of DenseNet / ResNet) is never written.  parts = {conv, pool}; tile 1 = fused, 0 = the two launches.
void Planner::FuseStemPool() {
    for (size_t i = 0; i + 1 < plan.steps.size(); ++i) {
        const Step& c = plan.steps[i];
        const Step& pl = plan.steps[i + 1];
        if (c.kind != StepKind::Conv || c.algo != ConvAlgo::Stem || !c.relu || c.has_in2 || !c.parts.empty() || c.out.nchw || c.out.c > 64 || c.out.c % 8) continue;
        if (pl.kind != StepKind::Pool || !pl.pool_max || pl.kh != 3 || pl.kw != 3 || pl.sh != 2 || pl.sw != 2 || pl.pt != 1 || pl.pl != 1 || pl.pb > 1 || pl.pr > 1) continue;
        if (pl.pre_scale_off >= 0 || pl.pre_relu || pl.has_in2 || pl.in_src != int(i)) continue;
        if (pl.in.buf != c.out.buf || pl.in.c_off != c.out.c_off || pl.in.c != c.out.c || pl.in.pitch != c.out.pitch || pl.in.h != c.out.h || pl.in.w != c.out.w) continue;
        if (pl.out.f16 != c.out.f16 || pl.out.f8 != c.out.f8 || pl.out.nchw || pl.out.buf == c.out.buf || pl.out.buf == c.in.buf) continue;
        if (pl.out.h != (c.out.h + 2 - 3) / 2 + 1 || pl.out.w != (c.out.w + 2 - 3) / 2 + 1) continue;
        if (pl.out.pitch % 8 || pl.out.c_off % 8 || (pl.out.f8 && (pl.out.pitch % 16 || pl.out.c_off % 16))) continue;
        // the conv's output must have no other reader: walk the launches behind the pool in execution order (a fused step = its parts) until the
        // buffer is written again -- recycled for another tensor, so the stem's tensor was dead by then (liveness pass)
        bool ok = true, recycled = false;
        auto visit = [&](const Step& u) {
            if (recycled || !ok) return;
            if (u.in.buf == c.out.buf || (u.has_in2 && u.in2.buf == c.out.buf)) ok = false;
            else if (u.out.buf == c.out.buf) recycled = true;
        };
        for (size_t q = i + 2; q < plan.steps.size() && ok && !recycled; ++q) {
            const Step& t = plan.steps[q];
            if (t.parts.empty()) visit(t);
            else for (const Step& tp : t.parts) visit(tp);
        }
        if (!ok || output_in_buffer(c.out.buf)) continue;
        Step f = c;
        f.algo = ConvAlgo::StemPool;
        f.tile = 1;
        f.out = pl.out;
        f.name = c.name + " + " + pl.name;
        f.flops = c.flops + pl.flops;
        f.bytes = double(c.in.numel()) * c.in.esize() + double(pl.out.numel()) * pl.out.esize() + double(c.out.c) * c.kh * c.kw * c.in.c * 4;
        f.parts = {c, pl};
        std::vector<Step> ns;
        ns.reserve(plan.steps.size() - 1);
        for (size_t q = 0; q < plan.steps.size(); ++q) {
            if (q == i + 1) continue;
            ns.push_back(q == i ? f : plan.steps[q]);
        }
        auto remap = [&](int src) { return src < 0 ? src : (size_t(src) > i ? src - 1 : src); };     // i + 1 -> i, everything behind moves up
        for (size_t q = 0; q < ns.size(); ++q) {
            Step& st = ns[q];
            st.idx = int(q);
            st.in_src = remap(st.in_src);
            st.in2_src = remap(st.in2_src);
            for (Step& part : st.parts) { part.in_src = remap(part.in_src); part.in2_src = remap(part.in2_src); }
        }
        // run as two launches, the parts share the fused step's slot: one tensor scale (a max pool keeps its operand's), same producer index
        ns[i].parts[0].idx = int(i);
        ns[i].parts[1].idx = int(i);
        ns[i].parts[1].in_src = int(i);
        plan.steps = std::move(ns);
        break;                                // one stem per graph
    }
}

// ---- projection shortcuts (fp8): conv3 + residual where the residual is a 1x1 projection conv -> ONE step of two GEMMs ------------------------
// Pattern: step j = 1x1/s1 conv C with a fused residual whose producer is step i < j = a plain 1x1 conv P (any stride, no prologue, no
// residual, no ReLU) read by nothing else.  out = relu(C(a) + P(x)) then runs as two accumulator sets of one launch (kernels_ws8.hip) and
// P's output -- the largest tensor of the block -- is never written.  P moves down to C's position (everything between them is independent
// of P's output: its only reader is C).
void Planner::FuseDualF8() {
    for (size_t j = 0; j < plan.steps.size(); ++j) {
        Step& c = plan.steps[j];
        if (c.kind != StepKind::Conv || IsGroupConv(c.algo) || !c.has_in2 || !c.parts.empty() || c.kh != 1 || c.kw != 1 || c.sh != 1 || c.sw != 1 || c.pt || c.pl || c.pb || c.pr) continue;
        if (c.pre_scale_off >= 0 || c.in.nchw || c.out.nchw || c.in.c % 32 || c.out.c % 32 || c.in2_src < 0 || size_t(c.in2_src) >= j) continue;
        const size_t i = size_t(c.in2_src);
        const Step& pr = plan.steps[i];
        if (pr.kind != StepKind::Conv || IsGroupConv(pr.algo) || !pr.parts.empty() || pr.has_in2 || pr.relu || pr.pre_scale_off >= 0 || pr.kh != 1 || pr.kw != 1 || pr.pt || pr.pl || pr.pb || pr.pr) continue;
        if (pr.in.nchw || pr.in.c % 32 || pr.out.buf != c.in2.buf || pr.out.c_off != c.in2.c_off || pr.out.c != c.in2.c || pr.out.pitch != c.in2.pitch) continue;
        if (pr.out.n != c.out.n || pr.out.h != c.out.h || pr.out.w != c.out.w || pr.out.c != c.out.c) continue;
        if (precision == Precision::F8 && (!pr.in.f8 || !c.in.f8 || !c.out.f8)) continue;
        if (pr.in.buf == c.out.buf || pr.out.buf == c.out.buf) continue;
        // P's output must have no other reader, and P's INPUT must still hold its value at C's position (not recycled in between)
        bool ok = true;
        for (size_t q = i + 1; q < plan.steps.size() && ok; ++q) {
            const Step& t = plan.steps[q];
            if (q != j && (t.in.buf == pr.out.buf || (t.has_in2 && t.in2.buf == pr.out.buf))) ok = false;
            if (q > j && t.out.buf == pr.out.buf) break;
        }
        for (size_t q = i + 1; q < j && ok; ++q)
            if (plan.steps[q].out.buf == pr.in.buf) ok = false;
        if (!ok || output_in_buffer(pr.out.buf)) continue;
        Step f = c;
        f.algo = ConvAlgo::DualF8;
        f.tile = 1;
        f.splitk = 1;
        f.has_in2 = false;
        f.in2 = View();
        f.in2_src = -1;
        f.name = pr.name + " (+) " + c.name;
        f.flops = pr.flops + c.flops;
        f.bytes = pr.bytes + c.bytes;
        f.parts = {pr, c};
        // steps i+1 .. j-1 move up by one, the fused step takes position j - 1 ... simpler: erase i, replace j (indices above i shift by -1)
        std::vector<Step> ns;
        ns.reserve(plan.steps.size() - 1);
        for (size_t q = 0; q < plan.steps.size(); ++q) {
            if (q == i) continue;
            ns.push_back(q == j ? f : plan.steps[q]);
        }
        auto remap = [&](int src) { return src < 0 ? src : (size_t(src) == i ? int(j) - 1 : (size_t(src) > i ? src - 1 : src)); };
        for (size_t q = 0; q < ns.size(); ++q) {
            Step& st = ns[q];
            st.idx = int(q);
            st.in_src = remap(st.in_src);
            st.in2_src = remap(st.in2_src);
            for (Step& part : st.parts) { part.in_src = remap(part.in_src); part.in2_src = remap(part.in2_src); }
        }
        // inside the fused step: the last conv's shortcut comes from the projection part (no plan step of its own any more)
        ns[j - 1].parts[1].in2_src = -1;
        plan.steps = std::move(ns);
        --j;
    }
}

// ---- I/O descriptors ---------------------------------------------------------------------------
void Planner::DescribeIo() {
    for (size_t i = 0; i < m.inputs.size(); ++i) {
        IoDesc d;
        d.name = m.inputs[i].name;
        d.elem_type = m.inputs[i].elem_type;
        d.model_dims = m.inputs[i].dims;
        d.dims = input_shapes[i];
        int v = L.get_val(d.name);
        if (!used[size_t(L.vals[v].root)]) {   // input never consumed: still give it a staging buffer
            plan.buffer_floats.push_back(root_floats(v));
            plan.buffer_f16.push_back(L.vals[v].is_i64 ? 3 : 0);
            L.vals[v].buf = int(plan.buffer_floats.size()) - 1;
        }
        d.view = view_of(v);
        plan.inputs.push_back(d);
    }
    for (size_t i = 0; i < m.outputs.size(); ++i) {
        IoDesc d;
        d.name = m.outputs[i].name;
        d.elem_type = m.outputs[i].elem_type;
        d.model_dims = m.outputs[i].dims;
        d.dims = L.vals[out_vals[i]].dims;
        d.view = view_of(out_vals[i]);
        const bool tok = tok_outputs.count(out_vals[i]) != 0;      // [N, L, D]: the rows of the NHWC buffer [N, 1, L, D], dense when the pitch is D
        if (tok) d.dims = {d.view.n, d.view.w, d.view.c};
        if (!d.view.nchw && (d.view.c_off != 0 || d.view.pitch != d.view.c || (tok ? d.view.h != 1 : d.view.h * d.view.w != 1)))
            fail("internal planner error: output " + d.name + " is not dense");
        plan.outputs.push_back(d);
    }
}

// The passes in the order they run.  Their order, the order in which they append to the weight blob and the order of their checks are
// behaviour: the blob layout and which error a bad graph reports first follow from them (tests/test_plan_digests.py pins both).
Plan BuildPlan(const OnnxModel& m, const std::vector<std::vector<int64_t>>& input_shapes, Precision precision, bool f8_fusions) {
    const Env env = Env::Read();          // the planner's switches, read once per plan build (load / prepare time)
    Planner P(m, input_shapes, env, precision, f8_fusions);
    const bool f8 = precision == Precision::F8 || f8_fusions;
    const bool forced = env.get("IE_FORCE_ALGO") || env.get("IE_FORCE_TILE");

    // ---- ONNX graph -> logical nodes with shape inference ----
    P.ImportInputs();
    P.MatchWindowAttention();                                    // the shifted-window attention regions of a Swin export: Linears stay, the rest is one node
    P.MatchPatchMerge();                                         // eight strided Slices and a Concat: one node
    P.MatchAttention();                                          // the unfused attention subgraphs, found on the ONNX nodes: each imports as one node
    P.MatchEmbed();                                              // table Gathers by INT64 graph inputs, their sum and the LayerNormalization behind it: one node
    P.MatchGroupNorm();                                          // the spellings of a group norm: one node
    P.MatchRmsNorm();                                            // an RMSNorm spelled out with Pow, ReduceMean and Sqrt: the RMSNormalization node
    P.MatchConv1D();                                             // HF's Conv1D on tokens (Reshape -> Gemm -> Reshape): a Linear, the Reshapes are names
    P.MatchGeluTanh();                                           // gelu_new spelled out with Pow and Tanh: the Gelu(approximate = "tanh") node
    for (const OnnxNode& on : m.nodes) P.ImportNode(on);
    P.MarkOutputs();
    if (f8) P.RefuseForF8();

    // ---- graph-level fusions ----
    P.FuseTokenAssemble();                                       // class-token Concat -> Add pos_embedding as one node
    P.FuseActivationPatterns();                                  // Mul(x, Sigmoid(x)) -> SiLU, Mul(x, HardSigmoid(x)) -> hardswish
    P.FuseGroupNormActivations();                                // GroupNorm -> SiLU / ReLU / Sigmoid as one node
    P.FuseGatedActivations();                                    // Mul(SiLU | GELU(a), b) -> one gated eltwise node (SwiGLU)
    if (!env.get("IE_NO_SE_FUSE")) P.FuseSqueezeExcite();        // pool -> 1x1 -> act -> 1x1 -> act -> Mul as one node
    P.MergeAffineChains();                                       // fusion 1: Affine -> Affine
    P.FuseConvEpilogues();                                       // fusion 2: Conv -> Affine / ReLU / Add / Clip / activation
    P.FuseRelu6IntoDepthwise();                                  // fusion 2b
    P.FuseActivationPrologues();                                 // fusion 2d
    if (!env.get("IE_NO_POOL_SWAP")) P.SwapConvAndAvgPool();     // fusion 2c: Conv1x1 -> AveragePool => AveragePool -> Conv1x1
    P.FusePrologues();                                           // fusion 3: Affine -> Relu -> {Conv, GlobalAveragePool, swapped AveragePool}
    P.FuseTrailingRelu();                                        // fusion 4: Add -> Relu, Affine -> Relu

    // ---- where every value lives ----
    P.StageNchwInputs();
    P.DensifyOutputs();
    P.PlaceConcatsAndAliases();
    P.ComputeLiveness();
    if (precision == Precision::F32 && !env.get("IE_NO_DENSE_FUSE")) P.KeepDenseFusionInputsLive();
    P.AssignBuffers();
    P.MarkBufferTypes();

    // ---- one step per live node, the kernel choice of every conv ----
    P.EmitSteps();

    // ---- step-level fusions, I/O descriptors ----
    if (precision == Precision::F32 && !env.get("IE_NO_DENSE_FUSE") && !forced) P.FuseDenseLayers();
    if (precision == Precision::F16 && !env.get("IE_NO_DENSE_BLOCK") && !forced) P.FuseDenseBlocks();
    if (!env.get("IE_NO_STEM_POOL")) P.FuseStemPool();
    if (f8 && !env.get("IE_NO_DUAL_F8")) P.FuseDualF8();
    P.DescribeIo();
    return std::move(P.plan);
}

static void json_view(std::ostringstream& o, const View& v) {
    o << "{\"buf\":" << v.buf << ",\"n\":" << v.n << ",\"c\":" << v.c << ",\"h\":" << v.h << ",\"w\":" << v.w
      << ",\"c_off\":" << v.c_off << ",\"pitch\":" << v.pitch << ",\"nchw\":" << (v.nchw ? "true" : "false")
      << ",\"f16\":" << (v.f16 ? "true" : "false") << ",\"f8\":" << (v.f8 ? "true" : "false");
    if (v.i64) o << ",\"i64\":true";      // (int64 id inputs only: other plans are unchanged)
    o << "}";
}
static void json_act(std::ostringstream& o, const char* key, const Act& a) {
    static const char* names[] = {"none", "sigmoid", "hardsigmoid", "silu", "hardswish", "relu", "gelu", "gelu_tanh", "tanh"};
    o << ",\"" << key << "\":[\"" << names[int(a.kind)] << "\"," << a.a << "," << a.b << "]";
}
static std::string json_escape(const std::string& s) {
    std::string o;
    for (char c : s) { if (c == '"' || c == '\\') o += '\\'; if (uint8_t(c) >= 0x20) o += c; }
    return o;
}

std::string PlanToJson(const Plan& p) {
    static const char* kinds[] = {"conv", "pool", "gap", "eltwise", "copy", "squeeze_excite", "resize", "layer_norm", "token_assemble", "attention", "window_attention", "patch_merge", "embed", "group_norm", "kv_append"};
    static const char* rs_modes[] = {"nearest", "linear"};
    static const char* rs_coords[] = {"half_pixel", "pytorch_half_pixel", "align_corners", "asymmetric"};
    static const char* rs_nearest[] = {"round_prefer_floor", "round_prefer_ceil", "floor", "ceil"};
    static const char* algos[] = {"igemm_vec", "igemm_scalar", "naive", "raster3x3", "ws1x1", "ws3x3", "stem", "direct", "igemm_f8", "dense_fused", "wino3x3", "conv1x1_x6", "dense_block", "dual_f8", "stem_pool", "depthwise", "grouped", "transposed"};
    std::ostringstream o;
    o.precision(17);
    o << "{\"inputs\":[";
    for (size_t i = 0; i < p.inputs.size(); ++i) {
        o << (i ? "," : "") << "{\"name\":\"" << json_escape(p.inputs[i].name) << "\",\"dims\":[";
        for (size_t k = 0; k < p.inputs[i].dims.size(); ++k) o << (k ? "," : "") << p.inputs[i].dims[k];
        o << "],\"view\":"; json_view(o, p.inputs[i].view); o << "}";
    }
    o << "],\"outputs\":[";
    for (size_t i = 0; i < p.outputs.size(); ++i) {
        o << (i ? "," : "") << "{\"name\":\"" << json_escape(p.outputs[i].name) << "\",\"dims\":[";
        for (size_t k = 0; k < p.outputs[i].dims.size(); ++k) o << (k ? "," : "") << p.outputs[i].dims[k];
        o << "],\"view\":"; json_view(o, p.outputs[i].view); o << "}";
    }
    o << "],\"buffers\":[";
    for (size_t i = 0; i < p.buffer_floats.size(); ++i) o << (i ? "," : "") << p.buffer_floats[i];
    o << "],\"precision\":\"" << (p.precision == Precision::F16 ? "fp16" : (p.precision == Precision::F8 ? "fp8" : "fp32")) << "\",\"activation_bytes\":" << p.activation_bytes()
      << ",\"workspace_floats\":" << p.workspace_floats << ",\"weight_floats\":" << p.weights.size() << ",\"total_flops\":" << p.total_flops
      << ",\"total_bytes\":" << p.total_bytes << ",\"steps\":[";
    for (size_t i = 0; i < p.steps.size(); ++i) {
        const Step& s = p.steps[i];
        o << (i ? "," : "") << "{\"kind\":\"" << kinds[int(s.kind)] << "\",\"name\":\"" << json_escape(s.name) << "\",\"in\":";
        json_view(o, s.in);
        if (s.has_in2) { o << ",\"in2\":"; json_view(o, s.in2); }
        if (s.kind == StepKind::Conv) o << ",\"residual\":" << (s.has_in2 ? "true" : "false");
        o << ",\"out\":"; json_view(o, s.out);
        o << ",\"k\":[" << s.kh << "," << s.kw << "],\"stride\":[" << s.sh << "," << s.sw << "],\"pads\":[" << s.pt << ","
          << s.pl << "," << s.pb << "," << s.pr << "]";
        if (s.dh != 1 || s.dw != 1) o << ",\"dilations\":[" << s.dh << "," << s.dw << "]";     // (dilated convs only: other plans are unchanged)
        o << ",\"pre\":" << (s.pre_scale_off >= 0 ? "true" : "false") << ",\"pre_relu\":" << (s.pre_relu ? "true" : "false")
          << ",\"relu\":" << (s.relu ? "true" : "false") << ",\"bias\":" << (s.bias_off >= 0 ? "true" : "false");
        // (only on the steps that have them: the plans of graphs without a Clip are unchanged)
        if (s.pre_hi < kInf) o << ",\"pre_clip\":" << s.pre_hi;
        if (s.lo > -kInf || s.hi < kInf) {
            o << ",\"clip\":[";
            if (s.lo > -kInf) o << s.lo; else o << "null";
            o << ",";
            if (s.hi < kInf) o << s.hi; else o << "null";
            o << "]";
        }
        // (only where set: the plans of graphs without these activations are unchanged)
        if (s.act.kind != ActKind::None || s.kind == StepKind::GroupNorm) json_act(o, "act", s.act);
        if (s.pre_act.kind != ActKind::None) json_act(o, "pre_act", s.pre_act);
        if (s.mul) o << ",\"mul\":true";
        if (s.kind == StepKind::SqueezeExcite) {
            o << ",\"se\":{\"mid\":" << s.se_mid << ",\"chunks\":" << s.se_chunks << ",\"w2_off\":" << s.w2_off << ",\"bias2_off\":" << s.bias2_off;
            json_act(o, "act1", s.se_act1);
            o << "}";
        }
        if (s.kind == StepKind::Conv) o << ",\"algo\":\"" << algos[int(s.algo)] << "\",\"tile\":" << s.tile << ",\"splitk\":" << s.splitk;
        if (s.kind == StepKind::Conv && s.algo == ConvAlgo::Grouped) o << ",\"group\":" << s.group;      // (grouped steps only)
        if (s.kind == StepKind::Conv && s.algo == ConvAlgo::Transposed) o << ",\"output_padding\":[" << s.oph << "," << s.opw << "]";      // (transposed steps only)
        if (s.kind == StepKind::Pool) o << ",\"max\":" << (s.pool_max ? "true" : "false");
        if (s.kind == StepKind::Resize)
            o << ",\"resize\":{\"mode\":\"" << rs_modes[int(s.rs_mode)] << "\",\"coord\":\"" << rs_coords[int(s.rs_coord)] << "\",\"nearest\":\""
              << rs_nearest[int(s.rs_nearest)] << "\",\"scales\":[" << s.rs_scale_h << "," << s.rs_scale_w << "]}";
        if (s.kind == StepKind::LayerNorm) o << ",\"eps\":" << s.ln_eps << ",\"tile\":" << s.tile;      // (layer-norm steps only)
        if (s.kind == StepKind::LayerNorm && s.rms) o << ",\"rms\":true";      // (RMSNorm steps only)
        if (s.kind == StepKind::Attention)
            o << ",\"heads\":" << s.heads << ",\"head_dim\":" << s.head_dim << ",\"scale\":" << s.attn_scale << ",\"tile\":" << s.tile;      // (attention steps only)
        if (s.kind == StepKind::Attention && s.key_mask) o << ",\"key_mask\":true,\"mask_value\":" << s.mask_value;      // (masked attention steps only)
        if (s.kind == StepKind::Attention && s.causal) o << ",\"causal\":true";      // (causal attention steps only)
        if (s.kind == StepKind::Attention && s.kv_heads > 0 && s.kv_heads != s.heads) o << ",\"kv_heads\":" << s.kv_heads;      // (grouped-query steps only)
        if (s.kind == StepKind::Attention && s.rope) o << ",\"rope\":true,\"w2_off\":" << s.w2_off;      // (rotary steps only)
        if (s.kind == StepKind::KvAppend || (s.kind == StepKind::Attention && s.past_len > 0)) {      // (the steps of a graph with a cache only: each field where set)
            if (s.kind == StepKind::KvAppend) {
                o << ",\"heads\":" << s.heads << ",\"head_dim\":" << s.head_dim << ",\"kv_heads\":" << s.kv_heads;
                if (s.rope) o << ",\"rope\":true,\"w2_off\":" << s.w2_off;
            }
            if (s.past_len > 0) o << ",\"past_len\":" << s.past_len;
            if (s.past_len > 0 && s.in.w > 1) o << ",\"new_len\":" << s.in.w;      // (the steps of an extend graph only)
            if (s.chunk_causal) o << ",\"chunk_causal\":true";
            if (s.rope) o << ",\"rope_rows\":" << s.rope_rows;
            if (s.splits > 0) o << ",\"splits\":" << s.splits;
            const std::pair<const char*, const View*> views[] = {{"past_k", &s.past_k}, {"past_v", &s.past_v}, {"present_k", &s.present_k}, {"present_v", &s.present_v}, {"positions", &s.pos}};
            for (const auto& kv : views)
                if (kv.second->buf >= 0) { o << ",\"" << kv.first << "\":"; json_view(o, *kv.second); }
        }
        if (s.kind == StepKind::WindowAttention)      // (window-attention steps only)
            o << ",\"heads\":" << s.heads << ",\"head_dim\":" << s.head_dim << ",\"scale\":" << s.attn_scale << ",\"window\":[" << s.win_h << "," << s.win_w << "],\"shift\":["
              << s.shift_h << "," << s.shift_w << "],\"masked\":" << (s.masked ? "true" : "false") << ",\"tile\":" << s.tile;
        if (s.kind == StepKind::GroupNorm) o << ",\"groups\":" << s.gn_groups << ",\"eps\":" << s.ln_eps << ",\"tile\":" << s.tile;      // (group-norm steps only)
        if (s.kind == StepKind::Embed) {      // (embed steps only)
            o << ",\"tables\":" << (s.w2_off >= 0 ? 2 : 1) << ",\"vocab\":[" << s.emb_vocab;
            if (s.w2_off >= 0) o << "," << s.emb_types;
            o << "],\"ln\":" << (s.bias_off >= 0 ? "true" : "false") << ",\"eps\":" << s.ln_eps << ",\"tile\":" << s.tile << ",\"w2_off\":" << s.w2_off << ",\"pos_off\":" << s.emb_pos_off
              << ",\"bias2_off\":" << s.bias2_off;
        }
        if (!s.parts.empty()) {
            Plan sub;
            sub.steps = s.parts;
            const std::string js = PlanToJson(sub);
            const size_t b = js.find("\"steps\":[");
            o << ",\"parts\":" << js.substr(b + 8, js.size() - (b + 8) - 1);
        }
        o << ",\"idx\":" << s.idx << ",\"in_src\":" << s.in_src << ",\"in2_src\":" << s.in2_src << ",\"w_off\":" << s.w_off << ",\"bias_off\":" << s.bias_off
          << ",\"pre_scale_off\":" << s.pre_scale_off << ",\"pre_shift_off\":" << s.pre_shift_off << ",\"count_include_pad\":" << (s.count_include_pad ? "true" : "false");
        o << ",\"flops\":" << s.flops << ",\"bytes\":" << s.bytes << "}";
    }
    o << "]}";
    return o.str();
}

}  // namespace ie
