#include "plan.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <functional>
#include <sstream>

#include "igemm_tiles.h"
#include "kernels.h"
#include "plan_internal.h"

namespace ie {
using namespace plan_internal;

// Dense-layer fusion applies where launches are latency-bound: up to this many output pixels (IE_FUSE_MAX_M overrides; A/B switch).
static int64_t FuseMaxPixels(const Env& env) {
    const char* e = env.get("IE_FUSE_MAX_M");
    const long long x = e ? std::atoll(e) : 0;
    const int64_t v = x > 0 ? int64_t(x) : int64_t(8192);
    return v;
}
namespace {

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
    n.name = node_name(on);
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

void Planner::ImportPatchMerge(const OnnxNode& on, const std::string& src) {
    const std::string nm = node_name(on);
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
void Planner::ImportEmbed(const OnnxNode& on, const EmbedMatch& em) {
    LNode n;
    n.kind = L_EMBED;
    n.name = node_name(on);
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
    P.IndexGraph();                                              // what the matchers below ask of the ONNX graph: producers, readers, constants
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
