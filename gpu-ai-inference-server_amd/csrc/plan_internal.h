// What the planner's translation units share: the lowered graph (Val, LNode, Lowering), the facts a conv step's kernel choice reads (ConvFacts) and the
// Planner itself, the state and the passes of one BuildPlan.  plan.cpp holds the import, the fusions, the buffer assignment and the step emission;
// plan_match.cpp holds the pattern matchers on the raw ONNX nodes (IndexGraph, GraphIndex, every Match*).  Nothing outside the planner includes this.
#pragma once

#include <algorithm>
#include <cstdint>
#include <list>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "env.h"
#include "plan.h"

namespace ie {
namespace plan_internal {

[[noreturn]] inline void fail(const std::string& msg) { throw std::runtime_error(msg); }

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

// the name an ONNX node goes by in a message: its own, or its first output's where the exporter gave it none
inline std::string node_name(const OnnxNode& n) { return n.name.empty() ? n.outputs[0] : n.name; }
inline std::string node_name(const OnnxNode* p) { return node_name(*p); }
inline bool is_transpose(const OnnxNode* p, const std::vector<int64_t>& perm) { return p && p->op == "Transpose" && p->attr_ints("perm", {}) == perm; }

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
    // MatchScoreMasks: the masks between the q k^T product and the Softmax -> the name of the scores above them, the nodes of a causal mask (its Where
    // and Slices, or its Add) and the Add of a key or chunk mask
    struct ScoreMasks { std::string scores; std::vector<const OnnxNode*> causal_nodes; const OnnxNode* mask_add = nullptr; };
    ScoreMasks MatchScoreMasks(const OnnxNode& sm, const std::string& prefix, AttnMatch& am);
    const OnnxNode* CausalWhereOf(const std::string& name) const;
    bool IsScores(const std::string& name) const;
    // what both attention forms end in: Softmax over the last axis; MatMul(P, v) -> Transpose ot [0,2,1,3] -> Reshape orr to s3 = [N, L, D]
    struct AttnTail { const OnnxNode *ot = nullptr, *orr = nullptr; const OnnxTensor* s3 = nullptr; };
    void RequireSoftmaxOverKeys(const OnnxNode& sm, const std::string& miss_prefix) const;
    AttnTail MatchAttentionTail(const OnnxNode* pv, const std::string& miss_prefix) const;
    std::map<const OnnxNode*, AttnMatch> attn_head;
    std::set<const OnnxNode*> attn_skip;
    void MatchAttention();
    void ImportAttention(const OnnxNode& on, const AttnMatch& am);
    // What the matchers on the ONNX nodes share (built once, by IndexGraph): the producer and the reader count of every name, the constants
    // (initializers and Constant nodes), the graph's inputs and outputs by name, and the small questions every matcher asks of a node
    struct GraphIndex {
        const OnnxModel* m = nullptr;
        std::map<std::string, const OnnxNode*> prod;
        std::map<std::string, int> readers;
        std::map<std::string, OnnxTensor> consts;
        std::map<std::string, const OnnxValueInfo*> inputs;
        std::set<std::string> outputs;
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
        const OnnxValueInfo* graph_input(const std::string& name) const { const auto it = inputs.find(name); return it == inputs.end() ? nullptr : it->second; }
        bool is_graph_output(const std::string& name) const { return outputs.count(name) != 0; }
        bool act_matmul(const OnnxNode* p) const { return p && p->op == "MatMul" && p->inputs.size() == 2 && !cst(p->inputs[0]) && !cst(p->inputs[1]); }
        // the integers of `attr`, else of the constant input `input` (opsets moved axes, starts, ... from the one to the other); empty: neither
        std::vector<int64_t> ints(const OnnxNode* p, const char* attr, size_t input) const {
            std::vector<int64_t> v = p->attr_ints(attr, {});
            if (v.empty() && p->inputs.size() > input && !p->inputs[input].empty()) if (const OnnxTensor* t = cst(p->inputs[input])) v = t->i;
            return v;
        }
        // dims with the axes of the Unsqueeze p inserted; false: its axes are no constants, or out of range
        bool unsqueeze(const OnnxNode* p, std::vector<int64_t>& dims) const {
            std::vector<int64_t> ax = ints(p, "axes", 1);
            if (ax.empty()) return false;
            const int64_t rank = int64_t(dims.size() + ax.size());
            for (int64_t& a : ax) if (a < 0) a += rank;
            std::sort(ax.begin(), ax.end());
            for (int64_t a : ax) { if (a < 0 || a > int64_t(dims.size())) return false; dims.insert(dims.begin() + a, 1); }
            return true;
        }
        // the constant shape of a Reshape, where it has `rank` entries; else nullptr
        const OnnxTensor* reshape_shape(const OnnxNode* p, size_t rank) const {
            const OnnxTensor* t = p && p->op == "Reshape" && p->inputs.size() == 2 ? cst(p->inputs[1]) : nullptr;
            return t && t->i.size() == rank ? t : nullptr;
        }
        // every output of p is read once, or the load is refused under miss_prefix
        void require_one_reader(const OnnxNode* p, const std::string& miss_prefix) const;
        // What peel_scales collects on its way up: the product of the constants, the links (appended to *taken), and the prefix of its refusals
        struct Scales { double scale = 1.0; std::vector<const OnnxNode*>* taken = nullptr; std::string miss_prefix; };
        // the name above a chain of Mul / Div by constants.  Without `acc` nothing is checked and nothing taken; with it every constant must be a scalar
        // (a Div's not zero), or the load is refused
        std::string peel_scales(std::string cur, Scales* acc = nullptr) const;
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

}  // namespace plan_internal
}  // namespace ie
