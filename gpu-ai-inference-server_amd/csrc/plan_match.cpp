// The pattern matchers of the planner: recognition of exporter spellings on the raw ONNX nodes, before the import.  Every matcher is built from the
// vocabulary of GraphIndex (plan_internal.h), takes the nodes of a match out of the import (a head that imports the whole, the rest skipped), and
// refuses a near miss naming what did not match; nothing is approximated.
#include <cmath>
#include <functional>

#include "plan_internal.h"

namespace ie {
using namespace plan_internal;

// ---- attention: the unfused multi-head attention subgraph of a ViT export as ONE node ------------------------------------------------
// Matched on the ONNX nodes, before the import (its inner values have ranks 4 and 5, which no Val holds), around every Softmax that sits between
// two MatMuls of activations:
//   R = Reshape(qkv, [N, L, 3, H, hd]) -> T = Transpose(R, [2,0,3,1,4]) -> q, k, v = Gather(T, axis 0, index 0 / 1 / 2) | Squeeze(Split(T, axis 0)[i], [0])
//   S = MatMul(q [* c], Transpose(k, [0,1,3,2]) [* c]) [* c | / c] -> P = Softmax(S, axis -1) -> MatMul(P, v) -> Transpose [0,2,1,3] -> Reshape [N, L, D]
// with scalar constants c in either operand order, every intermediate read by the next node only.  A near miss is refused naming what did not
// match; nothing is approximated.  A Softmax elsewhere is left to the import, which refuses it as an unsupported operator.
void Planner::IndexGraph() {
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
    for (const auto& vo : m.outputs) { ++gi.readers[vo.name]; gi.outputs.insert(vo.name); }
    for (const auto& vi : m.inputs) gi.inputs.emplace(vi.name, &vi);
}

void Planner::GraphIndex::require_one_reader(const OnnxNode* p, const std::string& miss_prefix) const {
    for (const std::string& o : p->outputs)
        if (nreaders(o) != 1) fail(miss_prefix + "the intermediate " + o + " (" + p->op + " " + node_name(p) + ") has " + std::to_string(nreaders(o)) + " readers, not 1");
}

std::string Planner::GraphIndex::peel_scales(std::string cur, Scales* acc) const {
    for (;;) {
        const OnnxNode* p = producer(cur);
        if (!p || (p->op != "Mul" && p->op != "Div") || p->inputs.size() != 2) return cur;
        const OnnxTensor *c0 = cst(p->inputs[0]), *c1 = cst(p->inputs[1]);
        if ((c0 != nullptr) == (c1 != nullptr) || (p->op == "Div" && !c1)) return cur;
        if (acc) {
            const OnnxTensor* c = c0 ? c0 : c1;
            if (c->numel() != 1 || c->f.size() != 1) fail(acc->miss_prefix + "the scale constant of " + p->op + " " + node_name(p) + " is not a scalar");
            if (p->op == "Div" && c->f[0] == 0.f) fail(acc->miss_prefix + "division by zero in " + node_name(p));
            acc->scale = p->op == "Div" ? acc->scale / double(c->f[0]) : acc->scale * double(c->f[0]);
            acc->taken->push_back(p);
        }
        cur = p->inputs[c0 ? 1 : 0];
    }
}

// The separate q / k / v spelling (BERT's eager attention):
//   q, k, v = Transpose(Reshape(MatMul(x, W*) + b*, [N, L, H, hd]), [0,2,1,3]);  kT = Transpose(k, [0,1,3,2]) (or the single Transpose [0,2,3,1] of the Reshape)
//   MatMul(q, kT) [* c | / c] -> [+ mask] -> Softmax -> MatMul(., v) -> Transpose [0,2,1,3] -> Reshape [N, L, D]
// GPT-2 writes q, k and v as the three parts of a Split of ONE Linear (MatchFusedSplit); BERT and Llama write three Linears (MatchLinears), which
// become one (MergeLinears).  Llama's eager attention adds three things between Transpose(., [0,2,1,3]) and the two MatMuls, each matched by its own
// member and refused by name on a near miss: the rotary embedding on q and k (UnRope), repeat_kv on k and v (UnRepeatKv) and the cache Concat on k and
// v (UnCache).  One object matches one Softmax; what it finds goes to `am`, `head` and `taken`.
namespace {

struct SplitAttention {
    Planner& P;
    const Planner::GraphIndex& gi;
    const std::string prefix;              // of every refusal: "Softmax <name>: the attention pattern around it does not match: "
    Planner::AttnMatch& am;
    std::vector<const OnnxNode*> taken;    // the nodes of the match (they import nothing, but for the head)
    Planner::GraphIndex::Scales scales;    // the product of the scalar constants on q, k and the scores, and their Mul / Div nodes (into taken)
    const OnnxNode* head = nullptr;        // the node that imports the attention: the Split, or the first of the three MatMuls in graph order
    std::string gather_pos;                // EvalRopeTable: the INT64 graph input that gathers the table being evaluated (empty: constant positions)
    std::string pos_miss;                  // EvalRopeTable: the refusal of position ids wider than [N, 1], for the import (AttnMatch::rope_pos_miss)
    // q's, k's and v's Reshape [N, L, H, hd], and behind a Reshape its Linear: the MatMul, the bias Add (or none), their constants
    const OnnxNode *rs[3] = {}, *mm[3] = {}, *add[3] = {};
    const OnnxTensor *W[3] = {}, *B[3] = {};
    std::vector<int64_t> shape4;           // q's Reshape target
    int64_t kvh = 0;                       // K / V heads of the split form (k's and v's Reshape)
    struct Rope { bool on = false; std::vector<float> cos, sin; int64_t rows = 0, hd = 0; std::string name, pos; int tables = 0; };
    static constexpr const char* kWhich[3] = {"q", "k", "v"};

    SplitAttention(Planner& p, const std::string& miss_prefix, Planner::AttnMatch& a) : P(p), gi(p.gi), prefix(miss_prefix), am(a) {
        scales.taken = &taken;
        scales.miss_prefix = prefix;
    }
    [[noreturn]] void miss(const std::string& what) const { fail(prefix + what); }
    std::string peel(const std::string& name) { return gi.peel_scales(name, &scales); }

    // A rope table as the graph's constants give it: an initializer / Constant, or Unsqueeze / Slice (step 1) / Gather(axis 0, constant indices) of one,
    // evaluated here.  nodes: the Unsqueeze / Slice / Gather nodes on the way.  false: `name` is no such constant
    bool EvalRopeTable(const std::string& name, OnnxTensor& out, std::vector<const OnnxNode*>& nodes) {
        if (const OnnxTensor* t = gi.cst(name)) { out = *t; return !t->f.empty(); }
        const OnnxNode* p = gi.producer(name);
        if (!p || p->inputs.empty()) return false;
        OnnxTensor in;
        if (p->op != "Unsqueeze" && p->op != "Slice" && p->op != "Gather") return false;
        if (!EvalRopeTable(p->inputs[0], in, nodes)) return false;
        nodes.push_back(p);
        const int64_t rank = int64_t(in.dims.size());
        // run-time positions (a decode step): Gather(table [max_pos, hd], position_ids [N, 1], axis 0) -> Unsqueeze(axes [1]) broadcasts as [N, 1, 1, hd].
        // The whole table is the constant; the kernels index it with the input's values
        if (p->op == "Gather" && p->inputs.size() == 2 && !gi.cst(p->inputs[1])) {
            const std::string who = "Gather " + node_name(p) + ": the position ids " + p->inputs[1] + " of the rope table ";
            const OnnxValueInfo* vi = gi.graph_input(p->inputs[1]);
            const std::vector<int64_t>* shape = vi ? &P.input_shapes[size_t(vi - P.m.inputs.data())] : nullptr;
            const bool ok = vi && vi->elem_type == ONNX_INT64 && shape->size() == 2;
            const int64_t width = ok ? (*shape)[1] : 0;
            const std::string not_n1 = who + "are neither a constant nor an INT64 graph input [N, 1] (supported: constant positions, or position_ids [N, 1] of a decode step)";
            if (!ok) miss(not_n1);
            if (width != 1) pos_miss = prefix + not_n1;      // (an extend step takes [N, Lq]: the import, which knows Lq, decides)
            if (p->attr_i("axis", 0) != 0 || rank != 2 || !gather_pos.empty()) miss(who + "must gather a [max_pos, hd] table once, along axis 0");
            gather_pos = p->inputs[1];
            out = in;
            return true;
        }
        if (p->op == "Unsqueeze" && !gather_pos.empty()) {
            if (gi.ints(p, "axes", 1) != std::vector<int64_t>{1}) miss("Unsqueeze " + node_name(p) + ": a rope table gathered by " + gather_pos + " [N, 1] must be unsqueezed at axes [1] (it then broadcasts as [N, 1, 1, hd])");
            out = in;
            return true;
        }
        if (!gather_pos.empty()) return false;
        if (p->op == "Unsqueeze") { out = in; return gi.unsqueeze(p, out.dims); }
        // Slice and Gather along one leading-row axis of the table: the rows [r0, r1) or the rows idx[...] of `in` seen as [rows][inner]
        int64_t axis = 0;
        std::vector<int64_t> pick, st, en;
        if (p->op == "Gather") {
            const OnnxTensor* ix = p->inputs.size() == 2 ? gi.cst(p->inputs[1]) : nullptr;
            axis = p->attr_i("axis", 0);
            if (!ix || ix->i.empty() || ix->dims.size() != 1) return false;
            pick = ix->i;
        } else {
            const std::vector<int64_t> ax = gi.ints(p, "axes", 3), sp = gi.ints(p, "steps", 4);
            st = gi.ints(p, "starts", 1);
            en = gi.ints(p, "ends", 2);
            if (st.size() != 1 || en.size() != 1 || ax.size() > 1 || sp.size() > 1 || (!sp.empty() && sp[0] != 1)) return false;
            axis = ax.empty() ? 0 : ax[0];
        }
        if (axis < 0) axis += rank;
        if (axis < 0 || axis >= rank) return false;
        const int64_t n = in.dims[size_t(axis)];
        if (p->op == "Slice") {
            const int64_t a = std::clamp<int64_t>(st[0] < 0 ? st[0] + n : st[0], 0, n), b = std::clamp<int64_t>(en[0] < 0 ? en[0] + n : en[0], 0, n);
            for (int64_t r = a; r < b; ++r) pick.push_back(r);
        }
        int64_t outer = 1, inner = 1;
        for (int64_t k = 0; k < axis; ++k) outer *= in.dims[size_t(k)];
        for (int64_t k = axis + 1; k < rank; ++k) inner *= in.dims[size_t(k)];
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
    }

    // One product of a rotary embedding, Mul(activation, table) in either order: -> the activation operand, `table` = the constant one evaluated
    std::string RopeTableOperand(const OnnxNode* mu, const std::string& who, Rope& r, OnnxTensor& table) {
        for (int k = 0; k < 2; ++k) {
            std::vector<const OnnxNode*> nodes;
            OnnxTensor t;
            gather_pos.clear();
            if (EvalRopeTable(mu->inputs[size_t(k)], t, nodes)) {
                const std::string gp = gather_pos;
                if (r.tables++ > 0 && r.pos != gp) miss(who + "its cos and sin tables are not gathered by the same position ids");
                r.pos = gp;
                if (!gp.empty()) for (const OnnxNode* p : nodes) P.mask_nodes.insert(p);      // (they may read the INT64 graph input)
                OnnxTensor dummy;
                std::vector<const OnnxNode*> n2;
                if (EvalRopeTable(mu->inputs[size_t(1 - k)], dummy, n2)) miss(who + "both operands of Mul " + node_name(mu) + " are constants");
                table = std::move(t);
                for (const OnnxNode* p : nodes) P.rope_const_nodes.insert(p);
                return mu->inputs[size_t(1 - k)];
            }
        }
        miss(who + "Mul " + node_name(mu) + " has no constant operand: cos and sin must be float constants (initializers, or Unsqueeze / Slice / Gather by constants of a table)");
    }

    // the tables broadcast as [1, 1, L, hd]: tb becomes [L, hd]
    void AsRopeTable2D(OnnxTensor& tb, const char* what, const std::string& who) const {
        std::vector<int64_t> d = tb.dims;
        while (d.size() > 2 && d[0] == 1) d.erase(d.begin());
        if (d.size() != 2 || tb.dims.size() > 4 || int64_t(tb.f.size()) != d[0] * d[1]) miss(who + "the " + what + " table does not broadcast as [1, 1, L, hd]");
        tb.dims = d;
    }

    // sl = Slice(t, hd/2:) (upper) or Slice(t, :hd/2) along the last axis
    bool IsHalfSlice(const OnnxNode* sl, const std::string& t, int64_t hd, bool upper) const {
        if (!sl || sl->op != "Slice" || sl->inputs.empty() || sl->inputs[0] != t) return false;
        const std::vector<int64_t> st = gi.ints(sl, "starts", 1), en = gi.ints(sl, "ends", 2), ax = gi.ints(sl, "axes", 3), sp = gi.ints(sl, "steps", 4);
        if (st.size() != 1 || en.size() != 1 || ax.size() != 1 || (ax[0] != -1 && ax[0] != 3) || (!sp.empty() && (sp.size() != 1 || sp[0] != 1))) return false;
        return upper ? st[0] == hd / 2 && en[0] >= hd : st[0] == 0 && en[0] == hd / 2;
    }

    // q and k pass the rotary embedding between their Transpose [0,2,1,3] and the score MatMul:
    //   name = Add(Mul(t, cos), Mul(Concat(Neg(Slice(t, hd/2:)), Slice(t, :hd/2), axis -1), sin)), either operand order: -> t (name itself: no rotation here)
    // cos / sin are float constants that broadcast as [1, 1, L, hd] (EvalRopeTable).  q and k must use the same tables, element for element (Match); the
    // tables ride in the weight blob and the kernels rotate inside their own loads (no step, no pass over the qkv buffer)
    std::string UnRope(const std::string& name, const char* which, Rope& r) {
        const OnnxNode* ad = gi.producer(name);
        if (!ad || ad->op != "Add" || ad->inputs.size() != 2) return name;
        const OnnxNode *m0 = gi.producer(ad->inputs[0]), *m1 = gi.producer(ad->inputs[1]);
        if (!m0 || !m1 || m0->op != "Mul" || m1->op != "Mul" || m0->inputs.size() != 2 || m1->inputs.size() != 2) return name;
        const std::string who = std::string("the rotary embedding of ") + which + " (Add " + node_name(ad) + "): ";
        r.name = node_name(ad);
        // the Mul whose activation operand is a Concat is the rotate_half branch
        OnnxTensor t0, t1;
        const std::string a0 = RopeTableOperand(m0, who, r, t0), a1 = RopeTableOperand(m1, who, r, t1);
        const OnnxNode *c0 = gi.producer(a0), *c1 = gi.producer(a1);
        const bool rot0 = c0 && c0->op == "Concat", rot1 = c1 && c1->op == "Concat";
        if (rot0 == rot1) miss(who + "exactly one of its two products must read rotate_half, Concat(Neg(Slice(t, hd/2:)), Slice(t, :hd/2), axis -1)");
        const OnnxNode* cat = rot0 ? c0 : c1;
        const std::string t = rot0 ? a1 : a0;
        OnnxTensor& cos = rot0 ? t1 : t0;
        OnnxTensor& sin = rot0 ? t0 : t1;
        AsRopeTable2D(cos, "cos", who);
        AsRopeTable2D(sin, "sin", who);
        if (cos.dims != sin.dims) miss(who + "the cos and sin tables differ in shape");
        const int64_t hd = cos.dims[1];
        if (hd < 2 || hd % 2) miss(who + "the head size " + std::to_string(hd) + " of the tables is not even");
        // rotate_half
        const int64_t cax = cat->attr_i("axis", 0);
        if (cat->inputs.size() != 2 || (cax != -1 && cax != 3)) miss(who + "Concat " + node_name(cat) + " is not a Concat of two parts along the last axis");
        const OnnxNode *ng = gi.producer(cat->inputs[0]), *lo = gi.producer(cat->inputs[1]);
        if (!ng || ng->op != "Neg")
            miss(who + "Concat " + node_name(cat) + " is not rotate_half: its first part must be Neg(Slice(t, hd/2:)) and its second Slice(t, :hd/2); the order (x1, -x2) is another function");
        const OnnxNode* hi = gi.producer(ng->inputs[0]);
        if (!IsHalfSlice(hi, t, hd, true) || !IsHalfSlice(lo, t, hd, false))
            miss(who + "Concat " + node_name(cat) + " is not rotate_half of " + t + ": its parts must be Neg(Slice(t, " + std::to_string(hd / 2) + ":)) and Slice(t, :" + std::to_string(hd / 2) + ") along the last axis");
        for (const OnnxNode* p : {m0, m1, cat, ng, hi, lo}) gi.require_one_reader(p, prefix);
        if (gi.nreaders(t) != 3) miss(who + "the rotated value " + t + " has " + std::to_string(gi.nreaders(t)) + " readers, not 3 (its product with cos and the two Slices of rotate_half)");
        taken.insert(taken.end(), {ad, m0, m1, cat, ng, hi, lo});
        r.on = true;
        r.cos = cos.f;
        r.sin = sin.f;
        r.rows = cos.dims[0];
        r.hd = hd;
        return t;
    }

    // k and v come from narrower Linears [Din, Hkv hd] (Reshape [N, L, Hkv, hd]) and pass repeat_kv behind their Transpose:
    //   name = Reshape(Expand(Unsqueeze(t, axis 2), [N, Hkv, g, L, hd]), [N, H, L, hd]) with constant shapes (g = 1: a no-op): -> t (name itself: no repeat_kv here)
    // The merged Linear is then [Din, D + 2 Dkv], and the step has kv_heads
    std::string UnRepeatKv(const std::string& name, const char* which, int64_t& g) {
        const OnnxNode* r4 = gi.producer(name);
        const OnnxNode* ex = r4 && r4->op == "Reshape" && !r4->inputs.empty() ? gi.producer(r4->inputs[0]) : nullptr;
        if (!ex || ex->op != "Expand") return name;
        const std::string who = std::string("repeat_kv of ") + which + " (Expand " + node_name(ex) + "): ";
        const OnnxNode* us = gi.producer(ex->inputs[0]);
        if (!us || us->op != "Unsqueeze" || gi.ints(us, "axes", 1) != std::vector<int64_t>{2}) miss(who + "its input is not Unsqueeze(., axes [2])");
        const OnnxTensor *e5 = ex->inputs.size() == 2 ? gi.cst(ex->inputs[1]) : nullptr, *s4 = r4->inputs.size() == 2 ? gi.cst(r4->inputs[1]) : nullptr;
        if (!e5 || e5->i.size() != 5 || !s4 || s4->i.size() != 4) miss(who + "the shapes of the Expand [N, Hkv, g, L, hd] and of the Reshape [N, H, L, hd] behind it must be constants");
        g = e5->i[2];
        if (g < 1) miss(who + "the group size " + std::to_string(g) + " is not positive");
        if (gi.is_graph_output(r4->outputs[0]))
            miss(who + "the graph output " + r4->outputs[0] + " is the value behind repeat_kv; a present output is the value in front of it, [N, Hkv, rows, hd]");
        for (const OnnxNode* p : {us, ex, r4}) gi.require_one_reader(p, prefix);
        taken.insert(taken.end(), {us, ex, r4});
        am.rep_expand.push_back(e5->i);
        am.rep_reshape.push_back(s4->i);
        return us->inputs[0];
    }

    // name = Concat(past, t, axis 2) with past a FLOAT rank-4 graph input, the cache of a decode step: -> t (name itself: no cache here)
    std::string UnCache(const std::string& name, const char* which, std::string& past, std::string& present, std::string& cat_name) {
        const OnnxNode* cat = gi.producer(name);
        if (!cat || cat->op != "Concat" || cat->inputs.size() != 2) return name;
        const OnnxValueInfo *i0 = gi.graph_input(cat->inputs[0]), *i1 = gi.graph_input(cat->inputs[1]);
        if (!i0 && !i1) return name;
        const std::string who = std::string("the cache of ") + which + " (Concat " + node_name(cat) + "): ";
        const std::string form = std::string("; supported: Concat(past, ") + which + ", axis 2) with past a FLOAT graph input [N, Hkv, P, hd] read by this Concat alone";
        if (!i0) miss(who + "its operands are in the order (" + which + ", past)" + form);
        if (i1) miss(who + "both operands are graph inputs" + form);
        const int64_t ax = cat->attr_i("axis", 0);
        if (ax != 2 && ax != -2) miss(who + "axis = " + std::to_string(ax) + form);
        if (i0->elem_type != ONNX_FLOAT || i0->dims.size() != 4) miss(who + "the past input " + i0->name + " is not a FLOAT tensor of rank 4" + form);
        if (gi.nreaders(i0->name) != 1) miss(who + "the past input " + i0->name + " has " + std::to_string(gi.nreaders(i0->name)) + " readers, not 1" + form);
        if (!gi.is_graph_output(cat->outputs[0]) || gi.nreaders(cat->outputs[0]) != 2)
            miss(who + "its result " + cat->outputs[0] + " must be a graph output (present.*) and be read by this attention alone besides; it has " + std::to_string(gi.nreaders(cat->outputs[0])) + " readers");
        taken.push_back(cat);
        past = i0->name;
        present = cat->outputs[0];
        cat_name = node_name(cat);
        return cat->inputs[1];
    }

    // GPT-2: q, k, v = the three parts of Split(axis 2, [D, D, D]) of one c_attn Linear (the exporter omits `split` when the parts are equal): the
    // Split's input is the qkv layout itself, and the Split is the head
    void MatchFusedSplit(const OnnxNode* sp) {
        for (int s = 0; s < 3; ++s) {
            const OnnxTensor* s4 = gi.reshape_shape(rs[s], 4);
            if (!s4 || s4->i[2] <= 0 || s4->i[3] <= 0) miss(std::string(kWhich[s]) + " is not Reshape(part " + std::to_string(s) + " of the Split, [N, L, H, hd]) with a constant shape");
            if (s == 0) shape4 = s4->i;
            else if (s4->i[2] != shape4[2] || s4->i[3] != shape4[3]) miss("the q / k / v Reshapes differ in heads or head size");
            if (rs[s]->inputs[0] != sp->outputs[size_t(s)]) miss(std::string(kWhich[s]) + " is not part " + std::to_string(s) + " of Split " + node_name(sp) + " (q, k, v must be its outputs 0, 1, 2)");
            if (gi.nreaders(rs[s]->outputs[0]) != 1 || gi.nreaders(rs[s]->inputs[0]) != 1)
                miss("the " + std::string(kWhich[s]) + " part of Split " + node_name(sp) + " or its Reshape has a second reader (only its own attention may read it)");
            taken.push_back(rs[s]);
        }
        const int64_t D = shape4[2] * shape4[3], ax = sp->attr_i("axis", 0);
        if (ax != 2 && ax != -1) miss("Split " + node_name(sp) + " has axis = " + std::to_string(ax) + ", not 2 (the channel axis of [N, L, 3 D])");
        std::vector<int64_t> parts = sp->attr_ints("split", {});
        if (parts.empty() && sp->inputs.size() > 1 && !sp->inputs[1].empty()) {
            const OnnxTensor* pt = gi.cst(sp->inputs[1]);
            if (!pt) miss("the split sizes of Split " + node_name(sp) + " are not constant");
            parts = pt->i;
        }
        if (!parts.empty() && parts != std::vector<int64_t>{D, D, D}) miss("Split " + node_name(sp) + " does not cut [H * hd, H * hd, H * hd] = three parts of " + std::to_string(D));
    }

    // The three Linears read the same token value and are read by their Reshape alone.  A Linear is MatMul + Add, or the MatMul alone (Llama's projections
    // have no bias).  k and v may have fewer heads than q (grouped K / V heads): whole groups of query heads per K / V head, repeat_kv (gk) by exactly that group
    void MatchLinears(int64_t gk) {
        for (int s = 0; s < 3; ++s) {
            const char* const which = kWhich[s];
            const OnnxTensor* s4 = gi.reshape_shape(rs[s], 4);
            if (!s4 || s4->i[2] <= 0 || s4->i[3] <= 0) miss(std::string(which) + " is not Reshape(Linear(x), [N, L, H, hd]) with a constant shape");
            if (s == 0) shape4 = s4->i;
            else if (s4->i[3] != shape4[3] || (s == 2 && s4->i[2] != kvh)) miss("the q / k / v Reshapes differ in heads or head size");
            if (s == 1) kvh = s4->i[2];
            if (s == 1 && kvh != shape4[2]) {
                if (kvh > shape4[2] || shape4[2] % kvh)
                    miss("heads % kv_heads != 0: q has " + std::to_string(shape4[2]) + " heads (Reshape " + node_name(rs[0]) + "), k has " + std::to_string(kvh) + " (Reshape " + node_name(rs[1]) +
                         "); a K / V head serves a whole group of query heads");
                if (gk != shape4[2] / kvh) miss("k and v have " + std::to_string(kvh) + " heads for q's " + std::to_string(shape4[2]) + ", but repeat_kv repeats them " + std::to_string(gk) + " times, not " + std::to_string(shape4[2] / kvh));
            }
            if (s == 1 && kvh == shape4[2] && gk > 1) miss("repeat_kv repeats k and v " + std::to_string(gk) + " times although they have q's " + std::to_string(kvh) + " heads");
            const int64_t Ds = s4->i[2] * s4->i[3];    // this Linear's columns: H hd for q, Hkv hd for k and v
            const OnnxNode* top = gi.producer(rs[s]->inputs[0]);
            add[s] = top && top->op == "Add" && top->inputs.size() == 2 ? top : nullptr;
            B[s] = nullptr;
            if (add[s]) {
                const int bi = gi.cst(add[s]->inputs[0]) ? 0 : 1;
                B[s] = gi.cst(add[s]->inputs[size_t(bi)]);
                mm[s] = gi.producer(add[s]->inputs[size_t(1 - bi)]);
                if (!B[s] || B[s]->f.empty()) miss(std::string(which) + " is not the Reshape of a Linear (MatMul(x, W [Din, D]) + b [D])");
            } else mm[s] = top;
            if (!mm[s] || mm[s]->op != "MatMul") miss(std::string(which) + " is not the Reshape of a Linear (MatMul + Add, or a MatMul alone)");
            W[s] = mm[s]->inputs.size() == 2 ? gi.cst(mm[s]->inputs[1]) : nullptr;
            if (!W[s] || gi.cst(mm[s]->inputs[0]) || W[s]->f.empty() || W[s]->dims.size() != 2)
                miss(std::string(which) + " is not the Reshape of a Linear (MatMul(x, W [Din, D]) + b [D])");
            if (mm[s]->inputs[0] != mm[0]->inputs[0])
                miss("the " + std::string(which) + " Linear " + node_name(mm[s]) + " reads " + mm[s]->inputs[0] + ", the q Linear " + mm[0]->inputs[0] + " (q, k and v must come from the same tokens)");
            if (W[s]->dims[0] != W[0]->dims[0] || W[s]->dims[1] != Ds || (B[s] && B[s]->numel() != Ds))
                miss("the " + std::string(which) + " Linear " + node_name(mm[s]) + " is not [Din, H * hd = " + std::to_string(Ds) + "] with a bias [" + std::to_string(Ds) + "] like the q Linear");
            for (const OnnxNode* p : {mm[s], add[s], rs[s]})
                if (p && gi.nreaders(p->outputs[0]) != 1) miss("the " + std::string(which) + " Linear's " + p->op + " " + node_name(p) + " has " + std::to_string(gi.nreaders(p->outputs[0])) + " readers, not 1 (only its own attention may read it)");
            taken.push_back(mm[s]);
            if (add[s]) taken.push_back(add[s]);
            taken.push_back(rs[s]);
        }
    }

    // The three Linears become ONE Linear x -> [N, L, D + 2 Dkv]: columns q (D) | k (Dkv) | v (Dkv), head h at h hd inside its part (weights and bias
    // concatenated, derived initializers), without a bias where none of the three has one.  The attention node then reads today's qkv layout.  The head is
    // the first of the three MatMuls in graph order (x is defined there)
    void MergeLinears() {
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
        for (const OnnxNode& on : P.m.nodes) if (&on == mm[0] || &on == mm[1] || &on == mm[2]) { head = &on; break; }
        am.split = true;
        am.x = mm[0]->inputs[0];
        am.name = node_name(mm[0]) + "+" + node_name(mm[1]) + "+" + node_name(mm[2]);
        am.w_name = w.name = am.name + "/qkv_w";
        am.b_name = b.name = am.name + "/qkv_b";
        P.L.add_derived(std::move(w));
        if (!am.no_bias) P.L.add_derived(std::move(b));
    }

    // false: q is neither Transpose [0,2,1,3] nor a rotary embedding (the other spelling, MatchAttentionCore's: q a Gather / Squeeze slice of one
    // transposed qkv tensor, where nothing is an Add of two products or a Transpose [0,2,1,3])
    bool Match(const OnnxNode& sm, const OnnxNode* pv, const std::string& scores) {
        const OnnxNode* qk = gi.producer(peel(scores));
        const OnnxNode* q0 = gi.producer(gi.peel_scales(qk->inputs[0]));
        const bool rope_add = q0 && q0->op == "Add" && q0->inputs.size() == 2 && gi.producer(q0->inputs[0]) && gi.producer(q0->inputs[0])->op == "Mul" &&
                              gi.producer(q0->inputs[1]) && gi.producer(q0->inputs[1])->op == "Mul";
        if (!is_transpose(q0, {0, 2, 1, 3}) && !rope_add) return false;
        // q: [rope of] Transpose(Reshape(.)); k: [Transposed] [repeat_kv of] [cache Concat of] [rope of] Transpose(Reshape(.)); v: the same without a rope
        Rope rq, rk;
        const OnnxNode* qt = gi.producer(UnRope(peel(qk->inputs[0]), "q", rq));
        if (!is_transpose(qt, {0, 2, 1, 3})) miss(std::string("q is not ") + (rq.on ? "the rotary embedding of " : "") + "Transpose(Reshape(Linear(x), [N, L, H, hd]), [0,2,1,3])");
        const OnnxNode* kt = gi.producer(peel(qk->inputs[1]));
        const OnnxNode* k_rs = nullptr;
        int64_t gk = 0, gv = 0;                        // repeat_kv's group size on k and on v (0: no repeat_kv)
        if (is_transpose(kt, {0, 2, 3, 1})) k_rs = gi.producer(kt->inputs[0]);
        else if (is_transpose(kt, {0, 1, 3, 2})) {
            const std::string k_cat = UnRepeatKv(kt->inputs[0], "k", gk);
            const std::string k_new = UnCache(k_cat, "k", am.past_k, am.present_k, am.cat_k);
            // a prefill with a cache: the rotated k (without rope: its Transpose) is also the graph output present.*.key
            if (am.past_k.empty() && gi.is_graph_output(k_new)) am.present_k = k_new;
            const OnnxNode* k2 = gi.producer(UnRope(k_new, "k", rk));
            if (!is_transpose(k2, {0, 2, 1, 3})) miss("the second operand of MatMul " + node_name(qk) + " is neither Transpose(Transpose(k, [0,2,1,3]), [0,1,3,2]) nor Transpose(k, [0,2,3,1])");
            taken.push_back(k2);
            k_rs = gi.producer(k2->inputs[0]);
        } else miss("the second operand of MatMul " + node_name(qk) + " is neither Transpose(Transpose(k, [0,2,1,3]), [0,1,3,2]) nor Transpose(k, [0,2,3,1])");
        const std::string v_new = UnCache(UnRepeatKv(pv->inputs[1], "v", gv), "v", am.past_v, am.present_v, am.cat_v);
        if (am.past_v.empty() && gi.is_graph_output(v_new)) am.present_v = v_new;
        const OnnxNode* vt = gi.producer(v_new);
        if (!is_transpose(vt, {0, 2, 1, 3})) miss("the second operand of MatMul " + node_name(pv) + " is not Transpose(v, perm [0,2,1,3])");
        // what q's, k's and v's chains found agrees
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
        // the Reshapes and what is in front of them: one Split, or three Linears
        rs[0] = gi.producer(qt->inputs[0]);
        rs[1] = k_rs;
        rs[2] = gi.producer(vt->inputs[0]);
        const OnnxNode* sp = rs[0] && !rs[0]->inputs.empty() ? gi.producer(rs[0]->inputs[0]) : nullptr;
        const bool fused = sp && sp->op == "Split" && sp->outputs.size() == 3 && rs[1] && rs[2] && rs[0]->op == "Reshape" && rs[1]->op == "Reshape" && rs[2]->op == "Reshape";
        if (fused) MatchFusedSplit(sp);
        else MatchLinears(gk);
        if (fused && !am.past_k.empty())
            miss("a cache (Concat " + am.cat_k + ") behind the Split of one qkv Linear (GPT-2's spelling) is not supported; the separate q / k / v Linears of a Llama-class graph are");
        if (fused && !am.present_k.empty()) miss("the graph output " + am.present_k + " behind the Split of one qkv Linear (GPT-2's spelling) is not supported");
        if (fused && (rq.on || gk > 0)) miss("a rotary embedding or repeat_kv behind the Split of one qkv Linear is not supported (the separate q / k / v Linears are)");
        if (rq.on && rq.hd != shape4[3]) miss("the rope tables (Add " + rq.name + ") are " + std::to_string(rq.hd) + " wide, the heads " + std::to_string(shape4[3]));
        // the Softmax and what is behind it; every intermediate read by the next node only
        P.RequireSoftmaxOverKeys(sm, prefix);
        const Planner::AttnTail tail = P.MatchAttentionTail(pv, prefix);
        // (a rotated value has three readers, its product with cos and the two Slices of rotate_half: the rotary match counted them)
        const bool prefill_present = am.past_k.empty() && !am.present_k.empty();      // (a present output of a prefill is one more reader of k's and v's value)
        for (const OnnxNode* p : {qk, qt, kt, vt, pv, tail.ot, &sm})
            if (gi.nreaders(p->outputs[0]) != (rq.on && p == qt ? 3 : 1) + (prefill_present && p == vt ? 1 : 0)) miss("the intermediate " + p->outputs[0] + " has " + std::to_string(gi.nreaders(p->outputs[0])) + " readers, not 1");
        for (const OnnxNode* p : taken)
            if ((p->op == "Mul" || p->op == "Div" || p->op == "Transpose") && gi.nreaders(p->outputs[0]) != (rk.on && is_transpose(p, {0, 2, 1, 3}) ? 3 : 1) + (prefill_present && p->outputs[0] == am.present_k ? 1 : 0)) miss("the intermediate " + p->outputs[0] + " has " + std::to_string(gi.nreaders(p->outputs[0])) + " readers, not 1");
        taken.insert(taken.end(), {qk, qt, kt, vt, pv, tail.ot, tail.orr, &sm});
        if (fused) {
            head = sp;
            am.fused = true;
            am.name = node_name(sp);
        } else {
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
            MergeLinears();
        }
        am.heads = shape4[2];
        am.head_dim = shape4[3];
        am.scale = scales.scale;
        am.out = tail.orr->outputs[0];
        am.shape3 = tail.s3->i;
        return true;
    }
};

}  // namespace

// The Softmax of an attention normalises over the keys, the last axis of the scores [N, H, L, L]
void Planner::RequireSoftmaxOverKeys(const OnnxNode& sm, const std::string& miss_prefix) const {
    const int64_t axis = sm.attr_i("axis", -1);
    if (axis != -1 && axis != 3) fail(miss_prefix + "Softmax axis = " + std::to_string(axis) + " (only the last axis, -1 or 3, is an attention)");
}

// behind the second MatMul: Transpose [0,2,1,3] -> Reshape [N, L, D], each the sole reader of what it reads
Planner::AttnTail Planner::MatchAttentionTail(const OnnxNode* pv, const std::string& miss_prefix) const {
    AttnTail t;
    t.ot = gi.only_reader(pv->outputs[0]);
    if (!is_transpose(t.ot, {0, 2, 1, 3})) fail(miss_prefix + "the result of MatMul " + node_name(pv) + " is not read by Transpose(perm [0,2,1,3]) alone");
    t.orr = gi.only_reader(t.ot->outputs[0]);
    t.s3 = gi.reshape_shape(t.orr, 3);
    if (!t.s3) fail(miss_prefix + "the transposed result is not read by Reshape(., [N, L, D]) alone");
    return t;
}

// The other spelling: q, k, v = slices 0, 1, 2 of one transposed qkv tensor (the comment above IndexGraph).
// `scores`: the name the scaled q k^T product reaches the Softmax (or, in a window attention, the bias Add) under
Planner::AttnCore Planner::MatchAttentionCore(const OnnxNode& sm, const OnnxNode* pv, const std::string& scores, const std::string& miss_prefix) {
    auto miss = [&](const std::string& what) { fail(miss_prefix + what); };
    AttnCore c;
    std::vector<const OnnxNode*>& taken = c.taken;
    // the chains of Mul / Div by scalar constants on the scores, on q and on k; each link read once
    GraphIndex::Scales scales;
    scales.taken = &taken;
    scales.miss_prefix = miss_prefix;
    RequireSoftmaxOverKeys(sm, miss_prefix);
    const OnnxNode* qk = gi.producer(gi.peel_scales(scores, &scales));
    const std::string q = gi.peel_scales(qk->inputs[0], &scales);
    const OnnxNode* kt = gi.producer(gi.peel_scales(qk->inputs[1], &scales));
    if (!is_transpose(kt, {0, 1, 3, 2})) miss("the second operand of MatMul " + qk->name + " is not Transpose(k, perm [0,1,3,2])");
    const std::string k = gi.peel_scales(kt->inputs[0], &scales);
    const std::string v = pv->inputs[1];
    // q, k, v = slices 0, 1, 2 of one transposed qkv tensor
    const OnnxNode* split = nullptr;
    std::string T;
    auto slice_of = [&](const std::string& name, int64_t want) {
        const OnnxNode* g = gi.producer(name);
        std::string src;
        int64_t idx = -1;
        if (g && g->op == "Gather" && g->inputs.size() == 2 && g->attr_i("axis", 0) == 0) {
            const OnnxTensor* ix = gi.cst(g->inputs[1]);
            if (ix && ix->dims.empty() && ix->i.size() == 1) { idx = ix->i[0]; src = g->inputs[0]; }
        } else if (g && g->op == "Squeeze" && !g->inputs.empty()) {
            const OnnxNode* sp = gi.producer(g->inputs[0]);
            if (gi.ints(g, "axes", 1) == std::vector<int64_t>{0} && sp && sp->op == "Split" && sp->outputs.size() == 3 && sp->attr_i("axis", 0) == 0 && !sp->inputs.empty()) {
                for (int64_t o = 0; o < 3; ++o) if (sp->outputs[size_t(o)] == g->inputs[0]) idx = o;
                src = sp->inputs[0];
                if (split && split != sp) idx = -1;
                split = sp;
                if (gi.nreaders(g->inputs[0]) != 1) miss("the Split output " + g->inputs[0] + " has a second reader");
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
    const OnnxNode* tr = gi.producer(T);
    if (!is_transpose(tr, {2, 0, 3, 1, 4})) miss("q, k and v are not slices of Transpose(perm [2,0,3,1,4])");
    const OnnxNode* rs = gi.producer(tr->inputs[0]);
    const OnnxTensor* s5 = gi.reshape_shape(rs, 5);
    if (!s5 || s5->i[2] != 3 || s5->i[3] <= 0 || s5->i[4] <= 0)
        miss("the qkv tensor is not Reshape(x, [N, L, 3, H, hd]) with a constant shape");
    const AttnTail tail = MatchAttentionTail(pv, miss_prefix);
    // every intermediate has one reader (the transposed qkv tensor: its three Gathers or its Split)
    taken.insert(taken.end(), {qk, kt, pv, tail.ot, tr, &sm});
    for (const OnnxNode* p : taken)
        for (const std::string& o : p->outputs) {
            const int want = (p == tr && !split) ? 3 : 1;
            if (gi.nreaders(o) != want) miss((p == qk || o == sm.inputs[0] ? "the scores " : "the intermediate ") + o + " has " + std::to_string(gi.nreaders(o)) + " readers, not " + std::to_string(want));
        }
    if (gi.nreaders(rs->outputs[0]) != 1) miss("the intermediate " + rs->outputs[0] + " has a second reader");
    c.rs = rs;
    c.orr = tail.orr;
    c.scale = scales.scale;
    c.shape5 = s5->i;
    c.shape3 = tail.s3->i;
    return c;
}

// a causal mask as Where(cond, scores, c), directly in front of the Softmax or of the key-mask Add (GPT-2 writes the Where first)
const OnnxNode* Planner::CausalWhereOf(const std::string& name) const {
    const OnnxNode* p = gi.producer(name);
    return p && p->op == "Where" && p->inputs.size() == 3 && gi.act_matmul(gi.producer(gi.peel_scales(p->inputs[1]))) ? p : nullptr;
}

// the scaled product of two activations, also behind a causal Where
bool Planner::IsScores(const std::string& name) const {
    const std::string cur = gi.peel_scales(name);
    return gi.act_matmul(gi.producer(cur)) || CausalWhereOf(cur) != nullptr;
}

// The masks between the q k^T product and the Softmax sm: a causal Where, a causal additive constant, the chunk mask of an extend step, or the key mask
// of an INT64 graph input; one mask only (a second one is refused by name).  What the mask says goes to am; -> the name of the scores above the masks,
// and the mask nodes
Planner::ScoreMasks Planner::MatchScoreMasks(const OnnxNode& sm, const std::string& prefix, AttnMatch& am) {
    ScoreMasks r;
    const std::string both = "a causal mask together with a key mask (attention_mask) on the scores is not supported";
    std::string sm_in = sm.inputs[0];          // the name the scores reach the Softmax (or the causal Where in front of it) under
    if (const OnnxNode* wh = CausalWhereOf(sm_in)) {
        MatchCausalWhere(*wh, prefix, am, r.causal_nodes);
        sm_in = wh->inputs[1];
    }
    const OnnxNode* top = gi.producer(gi.peel_scales(sm_in));
    r.scores = sm_in;
    if (!top || top->op != "Add" || top->inputs.size() != 2 || (!IsScores(top->inputs[0]) && !IsScores(top->inputs[1]))) return r;
    const int si = IsScores(top->inputs[0]) ? 0 : 1;
    const std::string tname = node_name(top);
    const std::string& mask = top->inputs[size_t(1 - si)];
    const OnnxTensor* mk = gi.cst(mask);
    if (top->outputs[0] == sm_in && !am.causal && mk && MatchCausalAdd(*mk, am)) {
        // the causal mask as an additive constant: 0 on and below the diagonal, one value <= -1e30 above it
        r.causal_nodes.push_back(top);
    } else if (const ChunkMask* cm = top->outputs[0] == sm_in ? MatchChunkMask(mask, prefix + "Add " + tname + ": ") : nullptr) {
        // the 4-D mask of an extend step: the key mask and the chunk's causal constant in one value; P and Lq are known at the import
        if (am.causal) fail(prefix + both + " (Add " + tname + ")");
        am.mask = key_masks.at(cm->ext).input;
        am.mask_value = cm->fill;
        am.chunk = true;
        am.chunk_c = cm->c;
        am.chunk_where = mask;
        ++chunk_masks[mask].uses;
        r.mask_add = top;
    } else {
        // only the key mask of an INT64 graph input [N, L], broadcast as [N, 1, 1, L], directly in front of the Softmax
        const KeyMask* km = top->outputs[0] == sm_in ? &MatchKeyMask(mask) : nullptr;
        if (km && km->ok && am.causal) fail(prefix + both + " (Add " + tname + ")");
        if (!km || !km->ok) fail(prefix + "an additive mask (Add " + tname + ") on the scores is not supported");
        am.mask = km->input;
        am.mask_value = km->c;
        ++key_masks[mask].uses;
        r.mask_add = top;
    }
    r.scores = top->inputs[size_t(si)];
    // one mask only: whatever masks the scores below this Add makes two
    if (const OnnxNode* wh = CausalWhereOf(gi.peel_scales(r.scores))) fail(prefix + both + " (Where " + wh->outputs[0] + " below Add " + tname + ")");
    const OnnxNode* below = gi.producer(gi.peel_scales(r.scores));
    if (below && below->op == "Add" && below->inputs.size() == 2 && (IsScores(below->inputs[0]) || IsScores(below->inputs[1]))) {
        bool two = am.causal;
        AttnMatch probe;
        for (const std::string& o : below->inputs) if (const OnnxTensor* c2 = gi.cst(o); c2 && MatchCausalAdd(*c2, probe)) two = true;
        if (two) fail(prefix + both + " (Add " + node_name(below) + " below Add " + tname + ")");
    }
    return r;
}

void Planner::MatchAttention() {
    for (const OnnxNode& sm : m.nodes) {
        if (sm.op != "Softmax" || sm.inputs.size() != 1 || sm.outputs.size() != 1 || wattn_softmax.count(&sm)) continue;
        const std::string nm = node_name(sm);
        const std::string prefix = "Softmax " + nm + ": the attention pattern around it does not match: ";
        // is this an attention at all?  scores from a MatMul of two activations (through scalings, or behind a mask Add), probabilities into a MatMul
        const OnnxNode* pv = nullptr;
        for (const OnnxNode& on : m.nodes)
            if (on.op == "MatMul" && on.inputs.size() == 2 && on.inputs[0] == sm.outputs[0] && !gi.cst(on.inputs[1])) pv = &on;
        if (!pv) continue;
        AttnMatch am;
        const ScoreMasks masks = MatchScoreMasks(sm, prefix, am);
        if (!gi.act_matmul(gi.producer(gi.peel_scales(masks.scores)))) continue;
        for (const OnnxNode* p : masks.causal_nodes) {
            if (p->op != "Slice" && gi.nreaders(p->outputs[0]) != 1) fail(prefix + "the masked scores " + p->outputs[0] + " have " + std::to_string(gi.nreaders(p->outputs[0])) + " readers, not 1");
            attn_skip.insert(p);
        }
        if (masks.mask_add && gi.nreaders(masks.mask_add->outputs[0]) != 1)
            fail(prefix + "the scores " + masks.mask_add->outputs[0] + " have " + std::to_string(gi.nreaders(masks.mask_add->outputs[0])) + " readers, not 1");
        if (masks.mask_add) attn_skip.insert(masks.mask_add);
        SplitAttention split(*this, prefix, am);
        if (split.Match(sm, pv, masks.scores)) {
            am.name += "+" + nm;
            attn_head[split.head] = am;
            for (const OnnxNode* p : split.taken) if (p != split.head) attn_skip.insert(p);
            continue;
        }
        const AttnCore c = MatchAttentionCore(sm, pv, masks.scores, prefix);
        am.heads = c.shape5[3];
        am.head_dim = c.shape5[4];
        am.scale = c.scale;
        am.out = c.orr->outputs[0];
        am.shape5 = c.shape5;
        am.shape3 = c.shape3;
        am.name = node_name(c.rs) + "+" + nm + "+" + node_name(c.orr);
        attn_head[c.rs] = am;
        for (const OnnxNode* p : c.taken) attn_skip.insert(p);
        attn_skip.insert(c.orr);
    }
    // the nodes that cut the rope tables out of constants were evaluated at load: they import nothing, and only rotary products may read them
    for (const OnnxNode* p : rope_const_nodes) {
        for (const OnnxNode* r : gi.readers_of(p->outputs[0]))
            if (!attn_skip.count(r) && !rope_const_nodes.count(r))
                fail(p->op + " " + node_name(p) + ": the rope table " + p->outputs[0] + " is read by " + r->op + " " + node_name(r) +
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
        const std::vector<int64_t> ax = gi.ints(u, "axes", 1);
        axes.insert(axes.begin(), ax.begin(), ax.end());
        nodes.push_back(u);
        cur = u->inputs[0];
    }
    // [N, L] -> [N, 1, 1, L]: axes [1] then [2], or [1, 2] at once
    if (axes != std::vector<int64_t>{1, 2}) return km;
    const OnnxValueInfo* vi = gi.graph_input(cur);
    if (!vi || vi->elem_type != ONNX_INT64 || vi->dims.size() != 2) return km;
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
    const std::string who = prefix + "the chunk mask Where " + node_name(wh) + ": ";
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
    const std::string nm = node_name(wh);
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
        const std::string snm = node_name(sl);
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
    for (const OnnxNode& g : m.nodes) {
        if (g.op != "Gemm" || g.inputs.size() < 2 || g.outputs.size() != 1 || gi.cst(g.inputs[0]) || !gi.cst(g.inputs[1])) continue;
        if (g.attr_i("transA", 0) != 0 || g.attr_i("transB", 0) != 0 || g.attr_f("alpha", 1.f) != 1.f || g.attr_f("beta", 1.f) != 1.f) continue;
        const OnnxNode* r1 = gi.producer(g.inputs[0]);
        const OnnxNode* r2 = gi.only_reader(g.outputs[0]);
        if (!gi.reshape_shape(r1, 2) || !gi.reshape_shape(r2, 3) || r2->inputs[0] != g.outputs[0] || gi.nreaders(r1->outputs[0]) != 1 || gi.cst(r1->inputs[0])) continue;
        conv1d_view[r1] = false;
        conv1d_view[r2] = true;
        conv1d_gemm.insert(&g);
    }
}

// gelu_new as torch spells it: 0.5 * x * (1 + Tanh(sqrt(2 / pi) * (x + 0.044715 * Pow(x, 3)))), every operand order, Mul(x, Mul(x, x)) in place of the
// Pow, the constants to 1e-6 relative (as the Erf pattern's).  It is the activation Gelu(approximate = "tanh") names.  Every intermediate is read once;
// a near miss is no match and its nodes import (or are refused: a left-over Pow is an unsupported operator) one by one
void Planner::MatchGeluTanh() {
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
    // an Add / MatMul with exactly one constant operand: the index of the activation operand, else -1
    auto act_side = [&](const OnnxNode* p) { return !p || p->inputs.size() != 2 || (gi.cst(p->inputs[0]) != nullptr) == (gi.cst(p->inputs[1]) != nullptr) ? -1 : (gi.cst(p->inputs[0]) ? 1 : 0); };
    // a float constant, through Unsqueeze nodes of constants (the constant folds of the import reduce exactly these)
    std::function<bool(const std::string&, OnnxTensor&)> resolve = [&](const std::string& name, OnnxTensor& out) -> bool {
        if (const OnnxTensor* t = gi.cst(name)) { out = *t; return true; }
        const OnnxNode* p = gi.producer(name);
        return p && p->op == "Unsqueeze" && !p->inputs.empty() && resolve(p->inputs[0], out) && gi.unsqueeze(p, out.dims);
    };
    for (const OnnxNode& sm : m.nodes) {
        if (sm.op != "Softmax" || sm.inputs.size() != 1 || sm.outputs.size() != 1) continue;
        const std::string nm = node_name(&sm);
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
        for (int k = 0; k < 2; ++k) if (gi.act_matmul(gi.producer(gi.peel_scales(badd->inputs[size_t(k)])))) bs = k;
        if (bs < 0) continue;
        const OnnxNode* rs = nullptr;
        {
            const OnnxNode* qk = gi.producer(gi.peel_scales(badd->inputs[size_t(bs)]));
            const OnnxNode* g = gi.producer(gi.peel_scales(qk->inputs[0]));
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
        RequireSoftmaxOverKeys(sm, prefix);
        const AttnCore c = MatchAttentionCore(sm, pv, badd->inputs[size_t(bs)], prefix);
        if (c.rs != rs) miss("q, k and v do not come from one Reshape [N nW, L, 3, heads, hd]");
        std::set<const OnnxNode*> skip(c.taken.begin(), c.taken.end());
        skip.insert(c.orr);
        skip.insert(badd);
        gi.require_one_reader(badd, prefix);
        const OnnxTensor* s6 = gi.reshape_shape(gi.producer(pt->inputs[0]), 6);
        const OnnxNode* p6 = gi.producer(pt->inputs[0]);
        if (!s6) miss("Transpose " + node_name(pt) + " does not read Reshape(x, [N, H/wh, wh, W/ww, ww, C]) with a constant shape");
        if (!is_transpose(pt, {0, 1, 3, 2, 4, 5})) miss("the partition Transpose " + node_name(pt) + " does not have perm [0,1,3,2,4,5]");
        WinMatch wm;
        wm.nh = s6->i[1]; wm.wh = s6->i[2]; wm.nw = s6->i[3]; wm.ww = s6->i[4];
        if (wm.nh < 1 || wm.wh < 1 || wm.nw < 1 || wm.ww < 1) miss("the partition Reshape " + node_name(p6) + " must give the window grid and the window as positive constants");
        const int64_t L = wm.wh * wm.ww, nW = wm.nh * wm.nw;
        wm.heads = c.shape5[3];
        wm.head_dim = c.shape5[4];
        wm.scale = c.scale;
        const OnnxTensor* s3p = gi.reshape_shape(p3, 3);
        if (!s3p || s3p->i[1] != L) miss("Reshape " + node_name(p3) + " is not to [N nW, L, C] with L = wh ww = " + std::to_string(L));
        if (c.shape5[1] != L && c.shape5[1] != 0 && c.shape5[1] != -1) miss("Reshape " + node_name(rs) + " is not to [N nW, L, 3, heads, hd] with L = " + std::to_string(L));
        if (c.shape3[1] != L && c.shape3[1] != 0 && c.shape3[1] != -1) miss("Reshape " + node_name(c.orr) + " is not to [N nW, L, D] with L = " + std::to_string(L));
        for (const OnnxNode* p : {p6, pt, p3}) { gi.require_one_reader(p, prefix); skip.insert(p); }
        if (qmm) { gi.require_one_reader(qmm, prefix); gi.require_one_reader(qadd, prefix); }
        // the bias: a constant [1 | -, heads, L, L]
        {
            const OnnxTensor* b = gi.cst(badd->inputs[size_t(1 - bs)]);
            if (!b || b->f.empty()) miss("Add " + node_name(badd) + ": the relative-position bias must be a floating-point constant");
            std::vector<int64_t> d = b->dims;
            if (d.size() == 4 && d[0] == 1) d.erase(d.begin());
            if (d.size() != 3 || d[0] != wm.heads || d[1] != L || d[2] != L)
                miss("Add " + node_name(badd) + ": the relative-position bias must have the shape [1, heads, L, L] = [1, " + std::to_string(wm.heads) + ", " + std::to_string(L) + ", " + std::to_string(L) + "]");
            wm.bias = b->f;
        }
        if (m4) {
            const OnnxTensor *s5m = gi.reshape_shape(m5, 5), *s4m = gi.reshape_shape(m4, 4);
            if (!s5m || s5m->i[1] != nW || s5m->i[2] != wm.heads || s5m->i[3] != L || s5m->i[4] != L)
                miss("Reshape " + node_name(m5) + " in front of the mask is not to [N, nW, heads, L, L] with nW = " + std::to_string(nW));
            if (!s4m || s4m->i[1] != wm.heads || s4m->i[2] != L || s4m->i[3] != L) miss("Reshape " + node_name(m4) + " behind the mask is not to [N nW, heads, L, L]");
            const int ms = gi.producer(madd->inputs[0]) == m5 ? 1 : 0;
            OnnxTensor mk;
            if (!resolve(madd->inputs[size_t(ms)], mk) || mk.f.empty())
                miss("Add " + node_name(madd) + ": the shift mask does not reduce to a floating-point constant");
            std::vector<int64_t> d = mk.dims;
            while (d.size() > 4 && d[0] == 1) d.erase(d.begin());
            if (d.size() != 4 || d[2] != L || d[3] != L) miss("Add " + node_name(madd) + ": the shift mask must have the shape [1, nW, 1, L, L] with L = " + std::to_string(L));
            if (d[1] != 1) miss("Add " + node_name(madd) + ": the shift mask must broadcast along the head axis ([1, nW, 1, L, L]), not hold " + std::to_string(d[1]) + " heads");
            if (d[0] != nW) miss("Add " + node_name(madd) + ": the shift mask holds " + std::to_string(d[0]) + " windows, the partition " + std::to_string(nW));
            wm.mask = mk.f;
            wm.masked = true;
            for (const OnnxNode* p : {m5, madd, m4}) { gi.require_one_reader(p, prefix); skip.insert(p); }
        }

        // ---- a roll: Concat(axis d) of Slice(x, [s], [max], [d]) and Slice(x, [0], [s], [d]); false: `name` is not made by a Concat of two Slices ----
        struct Roll { std::string src; int64_t axis = 0, shift = 0; const OnnxNode *cat = nullptr, *a = nullptr, *b = nullptr; };
        auto parse_roll = [&](const std::string& name, Roll& r) -> bool {
            const OnnxNode* cat = gi.producer(name);
            if (!cat || cat->op != "Concat" || cat->inputs.size() != 2) return false;
            const OnnxNode *a = gi.producer(cat->inputs[0]), *b = gi.producer(cat->inputs[1]);
            if (!a || !b || a->op != "Slice" || b->op != "Slice") return false;
            auto bad = [&](const std::string& what) { miss("Concat " + node_name(cat) + " is not a roll of the map: " + what); };
            auto one = [&](const OnnxNode* sl, size_t k, int64_t& v) {
                const OnnxTensor* t = sl->inputs.size() > k ? gi.cst(sl->inputs[k]) : nullptr;
                if (!t || t->i.size() != 1) bad("Slice " + node_name(sl) + " must have one constant start, end and axis");
                v = t->i[0];
            };
            int64_t as, ae, aa, bs_, be, ba;
            one(a, 1, as); one(a, 2, ae); one(a, 3, aa); one(b, 1, bs_); one(b, 2, be); one(b, 3, ba);
            for (const OnnxNode* sl : {a, b})
                if (sl->inputs.size() > 4 && !sl->inputs[4].empty()) { int64_t st; one(sl, 4, st); if (st != 1) bad("Slice " + node_name(sl) + " has a step"); }
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
                if (fsh[r.axis] != 0) miss("Concat " + node_name(r.cat) + " rolls axis " + std::to_string(r.axis) + " a second time");
                if (r.shift < 0) miss("Concat " + node_name(r.cat) + " rolls the map forward (by " + std::to_string(-r.shift) + ") in front of the partition; torchvision rolls by -shift there");
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
                if (!zero) miss("Pad " + node_name(pd) + ": a non-zero window padding is not supported (the map extents must be multiples of the window, all pads 0)");
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
        if (!rolled && wm.masked) miss("a shift mask (Add " + node_name(madd) + ") is added to the scores but the map is not rolled");

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
        const OnnxTensor* s6r = gi.reshape_shape(r6, 6);
        if (!s6r) miss("the result " + tail + " is not read by the reverse Reshape [N, H/wh, W/ww, wh, ww, C]");
        if (s6r->i[1] != wm.nh || s6r->i[2] != wm.nw || s6r->i[3] != wm.wh || s6r->i[4] != wm.ww)
            miss("Reshape " + node_name(r6) + ": the reverse has the window grid " + std::to_string(s6r->i[1]) + " x " + std::to_string(s6r->i[2]) + " and the window " +
                 std::to_string(s6r->i[3]) + " x " + std::to_string(s6r->i[4]) + ", the partition " + std::to_string(wm.nh) + " x " + std::to_string(wm.nw) + " and " +
                 std::to_string(wm.wh) + " x " + std::to_string(wm.ww));
        const OnnxNode* rt = reader_or_miss(r6->outputs[0], "the reverse Reshape");
        if (!is_transpose(rt, {0, 1, 3, 2, 4, 5})) miss("the reverse " + rt->op + " " + node_name(rt) + " is not Transpose(perm [0,1,3,2,4,5]), the partition's");
        const OnnxNode* r4 = reader_or_miss(rt->outputs[0], "the reverse Transpose");
        const OnnxTensor* s4r = gi.reshape_shape(r4, 4);
        if (!s4r || s4r->i[1] != wm.nh * wm.wh || s4r->i[2] != wm.nw * wm.ww) miss("the reverse does not end in Reshape [N, H, W, C] with H x W = " + std::to_string(wm.nh * wm.wh) + " x " + std::to_string(wm.nw * wm.ww));
        const OnnxNode* last = r4;
        int64_t bsh[3] = {0, 0, 0};
        for (int k = 0; k < 2; ++k) {
            const auto rd = gi.readers_of(last->outputs[0]);
            if (rd.size() != 2 || rd[0]->op != "Slice" || rd[1]->op != "Slice" || gi.nreaders(last->outputs[0]) != 2) break;
            const OnnxNode* cat = gi.only_reader(rd[0]->outputs[0]);
            Roll r;
            if (!cat || !parse_roll(cat->outputs[0], r) || r.src != last->outputs[0]) break;
            if (bsh[r.axis] != 0) miss("Concat " + node_name(r.cat) + " rolls axis " + std::to_string(r.axis) + " back a second time");
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
        wm.name = node_name(rs) + "+" + nm + "+" + node_name(c.orr);
        view_alias[p3] = src;
        view_alias[last] = r6->inputs[0];
        wattn_head[rs] = wm;
        skip.erase(rs);
        for (const OnnxNode* p : skip) wattn_skip.insert(p);
    }
}

// ---- patch merging: Concat(axis -1) of x[:, a::2, b::2, :] for (a, b) = (0,0), (1,0), (0,1), (1,1), each two strided Slices ----------
void Planner::MatchPatchMerge() {
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
        const std::string nm = node_name(&cat);
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
        const std::string nm = node_name(g);
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
        const std::string gname = node_name(g);
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
            else refusal = r->op + " " + node_name(r) + ": reads the embedding sum " + cur + "; only Adds and then a LayerNormalization may (the embedding and its LayerNormalization run as one step)";
            // (a Llama-class model has no position rows: the Gather itself is the value its first RMSNorm and the residual Add read, and heads the step)
            const OnnxNode* last = gi.producer(cur);
            if (cur == g.outputs[0] && !r) last = &g;      // (several readers: a sole reader that is neither an Add nor a LayerNormalization keeps its refusal)
            else if (cur == g.outputs[0] || !last || last->op != "Add") fail(refusal);
            ln = last;
            break;
        }
        if (embed_head.count(ln)) continue;
        const std::string lname = node_name(ln);
        EmbedMatch em;
        em.sum_only = !refusal.empty();
        const std::string who = (ln == &g ? "Gather " : em.sum_only ? "Add " : "LayerNormalization ") + lname;
        std::vector<const OnnxNode*> gathers, taken;
        int pos_count = 0;
        int64_t Lq = 0;
        if (const OnnxValueInfo* vi = gi.graph_input(g.inputs[1])) { const auto& shape = input_shapes[size_t(vi - m.inputs.data())]; Lq = shape.size() == 2 ? shape[1] : 0; }
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
                    fail("Add " + node_name(p) + ": the embedding sum " + name + " has a second reader in front of its LayerNormalization");
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
                if (gi.nreaders(name) != 1 && p != ln) fail("Gather " + node_name(p) + ": " + name + " has " + std::to_string(gi.nreaders(name)) + " readers; an embedding gather is read by its sum alone");
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
                        if (r < 0 || r >= P) fail("Gather " + node_name(p) + ": position id " + std::to_string(ix[size_t(l)]) + " is outside the table of " + std::to_string(P) + " rows");
                        std::copy(tab->f.begin() + r * D, tab->f.begin() + (r + 1) * D, f.begin() + l * D);
                    }
                    taken.push_back(p);
                    add_pos(f, {Lq, D}, "the position Gather " + node_name(p));
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
            em.names += (em.names.empty() ? "" : "+") + node_name(t);
            if (t != ln) embed_skip.insert(t);
        }
        for (const OnnxNode* t : taken) if (t != ln) embed_skip.insert(t);
        embed_head[ln] = std::move(em);
    }
    // whatever else reads an id input is refused by name
    for (const std::string& in : id_inputs) {
        if (gi.is_graph_output(in)) fail("graph output " + in + " is an INT64 graph input; only the Gather of an embedding table may read one");
        for (const OnnxNode* r : gi.readers_of(in))
            if (mask_nodes.count(r)) continue;             // the key mask of the attentions (MatchAttention took its chain)
            else if ((!embed_skip.count(r) && !embed_head.count(r)) || r->op != "Gather")
                fail(r->op + " " + node_name(r) + ": reads the INT64 graph input " + in + "; only the Gather (axis 0) of a floating-point embedding table [V, D] may read one");
    }
}

// ---- group norm: every spelling of a GroupNorm as ONE node ---------------------------------------------------------------------------------
// Matched on the ONNX nodes, before the import (the [N, G, -1] value in the middle is no feature map):
//   a) Reshape(x, [0, G, -1]) -> InstanceNormalization(scale [G], B [G]) -> Reshape(constant | Shape(x)) [-> Mul(gamma)] [-> Add(beta)]   (torch below opset 18)
//   b) GroupNormalization(x, scale, bias; num_groups, epsilon)       scale / bias [G] below opset 21, [C] from it on
//   c) InstanceNormalization directly on a map: G = C
// The matcher takes the structure and the reader counts; ImportGroupNorm, which knows x's shape, checks the shapes.  A near miss is refused naming
// the node and what did not match.
void Planner::MatchGroupNorm() {
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
        gm.name = gm.in_name = node_name(on);
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
        const OnnxTensor* shp1 = gi.reshape_shape(r1, 3);
        if (!shp1) {          // directly on a map
            gm.form = 'c';
            gn_head[&on] = gm;
            continue;
        }
        const std::string prefix = who + ": the group-norm pattern around it does not match: ";
        // (this pattern's wording names the value alone, not its node: kept as its tests pin it)
        auto read_once = [&](const std::string& name) {
            if (gi.nreaders(name) != 1) fail(prefix + "the intermediate value " + name + " has " + std::to_string(gi.nreaders(name)) + " readers, not 1");
        };
        gm.form = 'a';
        gm.shape1 = shp1->i;
        gm.groups = gm.shape1[1];
        gm.x = r1->inputs[0];
        read_once(r1->outputs[0]);
        read_once(on.outputs[0]);
        const OnnxNode* r2 = gi.only_reader(on.outputs[0]);
        if (!r2 || r2->op != "Reshape" || r2->inputs.size() != 2 || r2->inputs[0] != on.outputs[0])
            fail(prefix + "a Reshape back to the input's shape must read " + on.outputs[0]);
        std::vector<const OnnxNode*> taken = {r1, &on, r2};
        if (const OnnxTensor* b = gi.cst(r2->inputs[1])) {
            gm.back = b->i;
            if (gm.back.empty()) fail(prefix + "the shape of Reshape " + node_name(*r2) + " must be an integer constant or Shape(" + gm.x + ")");
        } else {
            const OnnxNode* sh = gi.producer(r2->inputs[1]);
            if (!sh || sh->op != "Shape" || sh->inputs.size() != 1 || sh->inputs[0] != gm.x || sh->attrs.count("start") || sh->attrs.count("end"))
                fail(prefix + "the shape of Reshape " + node_name(*r2) + " must be an integer constant or Shape(" + gm.x + ")");
            read_once(sh->outputs[0]);
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
            read_once(o);
            c = const_operand(*hit, act);
            cname = hit->inputs[size_t(1 - act)];
            taken.push_back(hit);
            last = hit;
        };
        affine("Mul", gm.gamma, gm.gamma_name);
        affine("Add", gm.beta, gm.beta_name);
        gm.out = last->outputs[0];
        gm.name.clear();
        for (const OnnxNode* p : taken) if (p->op != "Shape") gm.name += (gm.name.empty() ? "" : "+") + node_name(*p);
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
        const std::string prefix = "ReduceMean " + node_name(rm) + ": the RMSNorm pattern around it does not match: ";
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
        if (k < 0 || !scalar(ad->inputs[size_t(k)], eps) || !(eps >= 0.0)) fail(prefix + ad->op + " " + node_name(*ad) + " reads the mean; an Add of the scalar constant eps must");
        taken.push_back(ad);
        const OnnxNode* sr = down(ad->outputs[0]);
        if (sr->op != "Sqrt") fail(prefix + sr->op + " " + node_name(*sr) + " reads the sum with eps; a Sqrt must");
        taken.push_back(sr);
        const OnnxNode* rc = down(sr->outputs[0]);
        double one = 0.0;
        const bool recip = (rc->op == "Reciprocal" && rc->inputs.size() == 1) ||
                           (rc->op == "Div" && rc->inputs.size() == 2 && up(rc->inputs[1]) == sr->outputs[0] && scalar(rc->inputs[0], one) && one == 1.0);
        if (!recip) fail(prefix + rc->op + " " + node_name(*rc) + " reads the root; a Reciprocal or Div(1, root) must");
        taken.push_back(rc);
        const OnnxNode* mx = down(rc->outputs[0]);
        k = mx->op == "Mul" ? other(mx, rc->outputs[0]) : -1;
        if (k < 0 || up(mx->inputs[size_t(k)]) != x) fail(prefix + mx->op + " " + node_name(*mx) + " reads the reciprocal root; a Mul with " + x + ", the value that was squared, must");
        taken.push_back(mx);
        const OnnxNode* mw = down(mx->outputs[0]);
        k = mw->op == "Mul" ? other(mw, mx->outputs[0]) : -1;
        const OnnxTensor* w = k >= 0 ? gi.cst(mw->inputs[size_t(k)]) : nullptr;
        if (!w || w->f.empty() || w->dims.size() != 1) fail(prefix + mw->op + " " + node_name(*mw) + " reads the normalised value; a Mul with the weight, a floating-point constant [D], must");
        // every taken node but the last Mul is read inside the pattern only (a Cast of x may feed the square and the product: both are taken)
        std::set<const OnnxNode*> inside(taken.begin(), taken.end());
        inside.insert(mw);
        for (const OnnxNode* p : taken)
            for (const OnnxNode* r : gi.readers_of(p->outputs[0]))
                if (!inside.count(r)) fail(prefix + "the intermediate value " + p->outputs[0] + " has a reader outside the pattern (" + r->op + " " + node_name(*r) + ")");
        for (const auto& vo : m.outputs)
            for (const OnnxNode* p : taken) if (p->outputs[0] == vo.name) fail(prefix + "the intermediate value " + vo.name + " is a graph output");
        OnnxNode g;
        g.op = "RMSNormalization";
        for (const OnnxNode& on : m.nodes)      // (graph order)
            if (inside.count(&on) && on.op != "Cast") g.name += (g.name.empty() ? "" : "+") + node_name(on);
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

}  // namespace ie
