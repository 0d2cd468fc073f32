"""CPU: ViT through the ONNX reader and the planner (EngineDescribeModel): the token views (Reshape / Transpose / Gather are never a step), the
class-token concat and the position embedding as one token_assemble step, the unfused attention subgraph as one attention step in every spelling,
the Linear layers as 1x1 convs with bias and shortcut folded, the attention tiles, the refusals, and plan digests.
tests/golden/plan_digests_vit.json pins the plans and weight blobs of ViT-Tiny/16 and of the narrow test net.

    python tests/test_vit_plan.py            # rewrites tests/golden/plan_digests_vit.json from the built library
"""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    from _pkg import load_package
    load_package()

import vit_graphs as G  # noqa: E402
import ref64  # noqa: E402
import test_plan_digests as D  # noqa: E402
from engine_run import describe  # noqa: E402
from gpu_ai_inference_server_amd import binding as B  # noqa: E402
from gpu_ai_inference_server_amd.modelgen import models  # noqa: E402
from gpu_ai_inference_server_amd.modelgen import onnx_pb as pb  # noqa: E402
from refusals import refused  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "plan_digests_vit.json")
PRECS = ("fp32", "fp16")
BATCH, DIM, HEADS, MLP, DEPTH, L = 2, 64, 2, 128, 2, 17


def _same_view(a, b):
    return all(a[k] == b[k] for k in ("buf", "n", "c", "h", "w", "c_off", "pitch", "f16"))


# ---- the narrow net in every spelling ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("scale", G.SCALES)
@pytest.mark.parametrize("unbind", G.UNBINDS)
def test_narrow_vit_plan(tmp_path, monkeypatch, unbind, scale, prec):
    path = models.write_repo(str(tmp_path), "vit", G.narrow(BATCH, unbind=unbind, scale=scale))
    p = describe(path, BATCH, monkeypatch, prec)
    steps = p["steps"]
    f16 = prec == "fp16"
    layer = ["layer_norm", "conv", "attention", "conv", "layer_norm", "conv", "eltwise", "conv"]
    assert [s["kind"] for s in steps] == ["conv", "token_assemble"] + layer * DEPTH + ["layer_norm", "conv"], [(s["kind"], s["name"]) for s in steps]
    assert [s["name"] for s in steps if s["kind"] == "copy"] == []          # the patch conv reads the NCHW input itself; no view costs a copy
    patch, asm = steps[0], steps[1]
    assert patch["k"] == [8, 8] and patch["stride"] == [8, 8] and patch["bias"] and patch["in"]["nchw"]
    # the tokens are the conv's NHWC output under another shape: [N, D, 4, 4] -> n, c, h, w = N, D, 1, 16 in the same buffer
    assert (asm["in"]["buf"], asm["in"]["c"], asm["in"]["h"], asm["in"]["w"]) == (patch["out"]["buf"], DIM, 1, L - 1)
    assert (asm["out"]["n"], asm["out"]["c"], asm["out"]["h"], asm["out"]["w"]) == (BATCH, DIM, 1, L)
    assert asm["w_off"] >= 0 and asm["bias_off"] >= 0 and asm["name"].count("+") == 1               # the class token and the position embedding
    for li in range(DEPTH):
        ln1, qkv, at, proj, ln2, fc1, gelu, fc2 = steps[2 + 8 * li: 10 + 8 * li]
        assert ln1["name"] == f"l{li}_ln1" and ln2["name"] == f"l{li}_ln2" and ln1["eps"] == float(np.float32(1e-6))
        assert (qkv["in"]["c"], qkv["out"]["c"], qkv["out"]["w"], qkv["k"]) == (DIM, 3 * DIM, L, [1, 1]) and qkv["bias"] and not qkv["residual"]
        assert (at["heads"], at["head_dim"]) == (HEADS, DIM // HEADS)
        assert abs(at["scale"] / (DIM // HEADS) ** -0.5 - 1) < 1e-6
        assert _same_view(at["in"], qkv["out"]) and _same_view(at["out"], proj["in"])
        assert (at["out"]["n"], at["out"]["c"], at["out"]["h"], at["out"]["w"]) == (BATCH, DIM, 1, L)
        esz = 2 if f16 else 4
        assert at["flops"] == 4 * BATCH * HEADS * L * L * (DIM // HEADS) and at["bytes"] == esz * BATCH * L * (3 * DIM + DIM)
        assert at["tile"] == 1 and at["in"]["f16"] == at["out"]["f16"] == f16
        assert proj["residual"] and proj["bias"] and fc2["residual"] and fc2["bias"] and not fc1["residual"]
        assert (fc1["out"]["c"], fc2["in"]["c"], fc2["out"]["c"]) == (MLP, MLP, DIM) and gelu["act"] == ["gelu", 0, 0]
        assert _same_view(proj["in2"], ln1["in"]) and _same_view(fc2["in2"], proj["out"])
    head_ln, fc = steps[-2], steps[-1]
    assert head_ln["name"] == "head_ln" and head_ln["out"]["w"] == L
    # the class-token select is a view of the layer norm's output: row 0 of every image, L rows apart
    assert (fc["in"]["buf"], fc["in"]["n"], fc["in"]["c"], fc["in"]["h"], fc["in"]["w"]) == (head_ln["out"]["buf"], BATCH, DIM, 1, 1)
    assert (fc["in"]["pitch"], fc["in"]["c_off"]) == (L * head_ln["out"]["pitch"], head_ln["out"]["c_off"])
    assert p["outputs"][0]["dims"] == [BATCH, 10]


def test_spellings_give_the_same_plan(tmp_path, monkeypatch):
    plans = {}
    for unbind in G.UNBINDS:
        for scale in G.SCALES:
            path = models.write_repo(str(tmp_path), f"v_{unbind}_{scale}", G.narrow(BATCH, unbind=unbind, scale=scale))
            steps = describe(path, BATCH, monkeypatch, "fp32")["steps"]
            plans[unbind, scale] = [(s["kind"], s.get("algo"), s.get("tile"), s["in"], s["out"], s.get("residual"), s.get("heads"), s["w_off"]) for s in steps]
    first = plans["gather", "q"]
    assert all(v == first for v in plans.values())


def test_symbolic_batch_folds_the_expand_shape(tmp_path, monkeypatch):
    """batch "N": the Expand's shape is Shape(input) -> Gather 0 -> Unsqueeze -> Concat; the plan is that of the constant shape"""
    a = describe(models.write_repo(str(tmp_path), "sym", G.narrow("N")), 3, monkeypatch, "fp32")
    b = describe(models.write_repo(str(tmp_path), "con", G.narrow(3)), 3, monkeypatch, "fp32")
    assert [(s["kind"], s["in"], s["out"]) for s in a["steps"]] == [(s["kind"], s["in"], s["out"]) for s in b["steps"]]
    assert np.array_equal(B.PlanWeights(os.path.join(str(tmp_path), "sym", "1"), 3), B.PlanWeights(os.path.join(str(tmp_path), "con", "1"), 3))


def test_assemble_constants_are_in_the_blob(tmp_path, monkeypatch):
    from oracle import onnx_oracle as O
    mb = G.narrow(BATCH)
    path = models.write_repo(str(tmp_path), "vit", mb)
    asm = describe(path, BATCH, monkeypatch, "fp16")["steps"][1]
    blob = B.PlanWeights(path, BATCH)
    inits = O.load_model(mb).inits
    np.testing.assert_array_equal(blob[asm["w_off"]:asm["w_off"] + DIM], inits["class_token"].reshape(DIM))
    np.testing.assert_array_equal(blob[asm["bias_off"]:asm["bias_off"] + L * DIM], inits["pos_embedding"].reshape(L * DIM))
    assert np.abs(inits["pos_embedding"]).max() > 0.5 and np.abs(inits["class_token"]).max() > 0.5          # O(1): a dropped one is visible


# ---- attention tiles ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_attention_tiles(tmp_path, monkeypatch, prec):
    """default tile and IE_FORCE_TILE: hd 32 / 64 take the MFMA kernel, hd 20 the generic one whatever is forced, and L just past the LDS budget too"""
    f16 = prec == "fp16"
    lmax = G.max_mfma_tokens(64, f16)
    assert lmax == (288 if not f16 else 544)
    for l, heads, hd in ((5, 1, 32), (33, 3, 64), (7, 2, 20), (lmax, 1, 64), (lmax + 1, 1, 64)):
        path = models.write_repo(str(tmp_path), f"a{l}_{hd}", G.attn_graph(2, l, heads, hd))
        got = {}
        for forced in (None, "0", "1", "2"):
            steps = describe(path, 2, monkeypatch, prec, **({} if forced is None else {"IE_FORCE_TILE": forced}))["steps"]
            assert [s["kind"] for s in steps] == ["copy", "attention", "copy"]             # the NCHW graph input and output; nothing for the views
            got[forced] = steps[1]["tile"]
        ok = G.attn_mfma_ok(l, hd, heads * hd, f16)
        assert ok == (hd != 20 and l <= lmax)
        assert got == {None: int(ok), "0": 0, "1": int(ok), "2": int(ok)}, (l, hd, got)


# ---- the way back ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_tokens_back_to_a_feature_map(tmp_path, monkeypatch, prec):
    path = models.write_repo(str(tmp_path), "back", G.way_back_graph(2))
    steps = describe(path, 2, monkeypatch, prec)["steps"]
    assert [s["kind"] for s in steps] == ["conv", "layer_norm", "conv", "copy"] and steps[3]["name"] == "to_output(y)"       # (the NCHW graph output)
    ln, c3 = steps[1], steps[2]
    assert (ln["in"]["h"], ln["in"]["w"], ln["in"]["c"]) == (1, 16, 8) and ln["in"]["buf"] == steps[0]["out"]["buf"]
    assert (c3["in"]["buf"], c3["in"]["h"], c3["in"]["w"], c3["in"]["c"], c3["k"]) == (ln["out"]["buf"], 4, 4, 8, [3, 3])


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def _refused(tmp_path, monkeypatch, name, build, ishape, match, prec="fp32"):
    gb = models.GraphBuilder("r", 3)
    y = build(gb)
    if y != "y":
        gb.nodes.append(pb.node("Identity", [y], ["y"], "out"))
    path = models.write_repo(str(tmp_path), name, gb.finish([("x", ishape)], [("y", [1])], opset=17))
    refused(path, ishape[0], monkeypatch, prec=prec, match=match)


def _tok(gb, c=8):
    return models.vit_tokens(gb, "x", c)


def _back(gb, t, c, l):
    """tokens t [N, l, c] -> the graph output y [N, c, 1, l]"""
    return gb.simple("Reshape", [gb.transpose(t, (0, 2, 1)), _i64(gb, "back_shape", [0, c, 1, l])], out="y")


def _i64(gb, name, v):
    return gb.init(name, np.array(v, np.int64))


def _scalar(gb, name, v):
    gb.nodes.append(pb.node("Constant", [], [name], name, [pb.attr_int("value_int", v)]))
    return name


def test_token_view_refusals(tmp_path, monkeypatch):
    x4 = [2, 8, 2, 3]                                   # tokens [2, 6, 8]
    r = lambda *a: _refused(tmp_path, monkeypatch, *a)  # noqa: E731
    r("flat_conv", lambda gb: gb.relu(gb.simple("Reshape", ["x", _i64(gb, "s", [0, 8, -1])])), x4,
      r"Relu relu_\d+: input reshape_\d+_out is the \[N, C, H\*W\] reshape of a feature map; only a Transpose with perm \[0,2,1\] \(to tokens \[N, L, D\]\) may read it")
    r("flat_perm", lambda gb: gb.transpose(gb.simple("Reshape", ["x", _i64(gb, "s", [0, 8, -1])]), (1, 0, 2)), x4,
      r"Transpose transpose_\d+: perm \[1,0,2\] on the \[N, C, H\*W\] reshape of a feature map is not supported \(only \[0,2,1\] is\)")
    r("tok_perm", lambda gb: gb.transpose(_tok(gb), (2, 0, 1)), x4, r"Transpose transpose_\d+: perm \[2,0,1\] on a token view is not supported \(only \[0,2,1\] is\)")
    r("tok_relu", lambda gb: gb.relu(_tok(gb)), x4,
      r"Relu relu_\d+: input transpose_\d+_out is a token view \[N, L, D\]; only LayerNormalization, MatMul, Add, Mul, Div, Erf, Gelu, Transpose, Concat, Gather and "
      r"the Reshape of the attention pattern may read one")
    r("tok_conv", lambda gb: gb.conv(_tok(gb), 8, 4, 1, name="c"), x4, r"Conv c: input transpose_\d+_out is a token view")
    r("tok_shape", lambda gb: gb.simple("Shape", [_tok(gb)]), x4, r"Shape shape_\d+: input transpose_\d+_out is a token view")
    r("tok_softmax", lambda gb: gb.simple("Softmax", [_tok(gb)], [pb.attr_int("axis", -1)]), x4, r"Softmax softmax_\d+: input transpose_\d+_out is a token view")
    r("tok_reshape", lambda gb: gb.simple("Reshape", [_tok(gb), _i64(gb, "s", [0, -1])]), x4,
      r"Reshape reshape_\d+: input transpose_\d+_out is a token view \[N, L, D\]; only the \[N, L, 3, H, hd\] Reshape of the attention pattern may reshape one")
    r("tok_reshape5", lambda gb: gb.simple("Reshape", [_tok(gb), _i64(gb, "s", [0, -1, 1, 2, 4])]), x4, r"Unsupported ONNX operator: Reshape \(node reshape_\d+\)")
    r("back_relu", lambda gb: gb.relu(gb.transpose(_tok(gb), (0, 2, 1))), x4,
      r"Relu relu_\d+: input transpose_\d+_out is the \[N, D, L\] transpose of a token view; only a Reshape to \[N, D, h, w\] with h \* w = L may read it")
    r("back_shape", lambda gb: gb.simple("Reshape", [gb.transpose(_tok(gb), (0, 2, 1)), _i64(gb, "s", [0, 4, 3, 4])]), x4,
      r"Reshape reshape_\d+: the \[N, D, L\] transpose of a token view only reshapes to \[N, D, h, w\] with h \* w = L")
    r("ln_axis", lambda gb: gb.layernorm(_tok(gb), 8, axis=1, name="ln"), x4, r"LayerNormalization ln: axis = 1 on a token view is not supported")
    r("bcast", lambda gb: gb.simple("Mul", [_tok(gb), gb.init("s", np.ones((6, 1), np.float32))]), x4,
      r"Mul mul_\d+: constant operand must broadcast along the last axis of the token view transpose_\d+_out")
    r("mixed", lambda gb: gb.simple("Add", [_tok(gb), gb.conv("x", 8, 8, 1, name="c")]), x4, r"Add add_\d+: the operands mix a token view and another value")
    r("matmul_k", lambda gb: gb.simple("MatMul", [_tok(gb), gb.init("w", np.ones((6, 4), np.float32))]), x4, r"MatMul matmul_\d+: inner dimensions do not match")
    # token-axis concats
    cls = lambda gb: gb.init("cls", np.ones((1, 1, 8), np.float32))  # noqa: E731
    r("cat_two", lambda gb: gb.concat([_tok(gb), _tok(gb)]), x4,
      r"Concat concat_\d+: concatenating two activations along the token axis is not supported \(only a class-token constant in front of the tokens\)")
    r("cat_behind", lambda gb: gb.concat([_tok(gb), cls(gb)]), x4,
      r"Concat concat_\d+: a constant behind the tokens is not supported \(only a class-token constant in front of the tokens\)")
    r("cat_three", lambda gb: gb.concat([cls(gb), _tok(gb), _tok(gb)]), x4,
      r"Concat concat_\d+: a token-axis concat takes exactly two operands, a class-token constant and the tokens \(it has 3\)")
    r("cat_axis", lambda gb: gb.concat([cls(gb), _tok(gb)], axis=2), x4, r"Concat concat_\d+: only axis = 1 \(the token axis\) is supported on token views")
    r("cat_shape", lambda gb: gb.concat([gb.init("cls", np.ones((1, 2, 8), np.float32)), _tok(gb)]), x4,
      r"Concat concat_\d+: the class token must be a floating-point constant of shape \[1 \| N, 1, D\]")
    # a position embedding anywhere but directly behind the concat
    pos = lambda gb, l: gb.init("pos", np.ones((1, l, 8), np.float32))  # noqa: E731
    r("pos_alone", lambda gb: _back(gb, gb.simple("Add", [_tok(gb), pos(gb, 6)]), 8, 6), x4,
      r"Add add_\d+: a \[1, L, D\] constant is only added to tokens directly behind the class-token Concat, as its sole reader")

    def pos_shared(gb):
        c = gb.concat([cls(gb), _tok(gb)])
        return _back(gb, gb.simple("Add", [gb.simple("Add", [c, pos(gb, 7)]), c]), 8, 7)
    r("pos_shared", pos_shared, x4, r"Add add_\d+: a \[1, L, D\] constant is only added to tokens directly behind the class-token Concat, as its sole reader")
    # token select
    r("gather_axis", lambda gb: gb.simple("Gather", [_tok(gb), _scalar(gb, "i0", 0)], [pb.attr_int("axis", 2)]), x4,
      r"Gather gather_\d+: only Gather\(axis = 1, scalar constant index\) selects a token of the token view transpose_\d+_out")
    r("gather_vec", lambda gb: gb.simple("Gather", [_tok(gb), _i64(gb, "ix", [0])], [pb.attr_int("axis", 1)]), x4, r"Gather gather_\d+: only Gather\(axis = 1, scalar constant index\)")
    r("gather_range", lambda gb: gb.simple("Gather", [_tok(gb), _scalar(gb, "i9", 9)], [pb.attr_int("axis", 1)]), x4, r"Gather gather_\d+: index out of range")
    r("expand_act", lambda gb: gb.simple("Expand", [gb.conv("x", 8, 8, 1, name="c"), _i64(gb, "s", [2, 8, 2, 3])]), x4, r"Unsupported ONNX operator: Expand \(node expand_\d+\)")


def test_second_token_view_of_one_map_is_refused(tmp_path, monkeypatch):
    """H > 1: the token value is an alias of the map's buffer; a second one would need a reshaping copy, which no kernel does"""
    def build(gb):
        a = gb.conv("x", 8, 8, 1, name="a")
        t = gb.simple("Add", [gb.layernorm(models.vit_tokens(gb, a, 8), 8, name="ln1"), gb.layernorm(models.vit_tokens(gb, a, 8), 8, name="ln2")])
        return _back(gb, t, 8, 6)
    _refused(tmp_path, monkeypatch, "twoviews", build, [2, 8, 2, 3],
             r"token view transpose_\d+: its input a_out already lives in another value's buffer \(a second view of it, or a Concat\); reshaping it between a feature map "
             r"and tokens would need a copy, which is not supported")


def test_token_graph_output_is_refused(tmp_path, monkeypatch):
    gb = models.GraphBuilder("r", 3)
    y = gb.layernorm(_tok(gb), 8, name="ln")
    path = models.write_repo(str(tmp_path), "tokout", gb.finish([("x", [2, 8, 2, 3])], [(y, [2, 6, 8])], opset=17))
    refused(path, 2, monkeypatch, match=r"graph output ln_out is a token view")


def _attn_variant(tmp_path, monkeypatch, name, mutate, match, heads=2, hd=4, l=6):
    """the attention test graph with one node changed by mutate(nodes as (op, inputs, outputs, name, attrs) builder access)"""
    d = heads * hd
    gb = models.GraphBuilder("attn", 5)
    t = models.vit_tokens(gb, "x", 3 * d)
    mutate(gb, t, d, heads)
    path = models.write_repo(str(tmp_path), name, gb.finish([("x", [2, 3 * d, 1, l])], [("y", [2, d, 1, l])], opset=17))
    refused(path, 2, monkeypatch, match=match)


def _attention_by_hand(gb, t, d, heads, *, softmax_axis=-1, scale_shape=(), mask=False, second_reader=False, k_index=1, perm5=(2, 0, 3, 1, 4), out_perm=(0, 2, 1, 3)):
    hd = d // heads
    y = gb.transpose(gb.simple("Reshape", [t, _i64(gb, "s5", [0, -1, 3, heads, hd])]), perm5)
    q, k, v = [gb.simple("Gather", [y, _scalar(gb, f"i{n}_{i}", i)], [pb.attr_int("axis", 0)]) for n, i in enumerate((0, k_index, 2))]
    q = gb.simple("Mul", [q, gb.init("scale", np.full(scale_shape, hd ** -0.5, np.float32))])
    s = gb.simple("MatMul", [q, gb.transpose(k, (0, 1, 3, 2))])
    if mask:
        s = gb.simple("Add", [s, gb.init("mask", np.zeros((1, 1, 6, 6), np.float32))])
    if second_reader:
        gb.simple("Mul", [s, gb.init("two", np.array(2.0, np.float32))])          # (a dangling second reader of the scores)
    p = gb.simple("Softmax", [s], [pb.attr_int("axis", softmax_axis)])
    o = gb.simple("MatMul", [p, v])
    o = gb.simple("Reshape", [gb.transpose(o, out_perm), _i64(gb, "s3", [0, -1, d])])
    gb.simple("Reshape", [gb.transpose(o, (0, 2, 1)), _i64(gb, "sb", [0, d, 1, 6])], out="y")


def test_attention_near_misses_are_refused(tmp_path, monkeypatch):
    pre = r"Softmax softmax_\d+: the attention pattern around it does not match: "
    v = lambda name, match, **kw: _attn_variant(tmp_path, monkeypatch, name, lambda gb, t, d, h: _attention_by_hand(gb, t, d, h, **kw), match)  # noqa: E731
    v("axis2", pre + r"Softmax axis = 2 \(only the last axis, -1 or 3, is an attention\)", softmax_axis=2)
    v("vecscale", pre + r"the scale constant of Mul mul_\d+ is not a scalar", scale_shape=(4,))
    v("mask", pre + r"an additive mask \(Add add_\d+\) on the scores is not supported", mask=True)
    v("reader", pre + r"the scores matmul_\d+_out has 2 readers, not 1", second_reader=True)
    v("kslice", pre + r"gather_\d+_out is not slice 1 of the transposed qkv tensor", k_index=0)
    v("perm5", pre + r"q, k and v are not slices of Transpose\(perm \[2,0,3,1,4\]\)", perm5=(2, 0, 1, 3, 4))
    v("operm", pre + r"the result of MatMul matmul_\d+ is not read by Transpose\(perm \[0,2,1,3\]\) alone", out_perm=(0, 1, 2, 3))
    # the pattern is fine but the qkv rows are not 3 * H * hd wide
    def narrow_rows(gb, t, d, heads):
        _attention_by_hand(gb, gb.simple("MatMul", [t, gb.init("w", np.ones((3 * d, 3 * d + 8), np.float32))]), d, heads)
    _attn_variant(tmp_path, monkeypatch, "width", narrow_rows, r"attention reshape_\d+\+softmax_\d+\+reshape_\d+: the qkv rows have 32 columns, not 3 \* H \* hd = 24")


def test_left_over_pieces_are_unsupported_operators(tmp_path, monkeypatch):
    r = lambda *a: _refused(tmp_path, monkeypatch, *a)  # noqa: E731
    x4 = [2, 8, 2, 3]
    # a Softmax that is no attention; a MatMul of two activations; a Split
    r("softmax", lambda gb: gb.simple("Softmax", [gb.conv("x", 8, 8, 1, name="c")], [pb.attr_int("axis", 1)]), x4, r"Unsupported ONNX operator: Softmax \(node softmax_\d+\)")
    r("matmul", lambda gb: gb.simple("MatMul", [gb.gap("x"), gb.gap("x")]), x4, r"Unsupported ONNX operator: MatMul \(node matmul_\d+\)")

    def split(gb):
        gb.nodes.append(pb.node("Split", ["x", _i64(gb, "sp", [4, 4])], ["a", "b"], "sp0", [pb.attr_int("axis", 1)]))
        return "a"
    r("split", split, x4, r"Unsupported ONNX operator: Split \(node sp0\)")


def test_fp8_is_refused(tmp_path, monkeypatch):
    path = models.write_repo(str(tmp_path), "vit", G.narrow(BATCH))
    refused(path, BATCH, monkeypatch, prec="fp8", match=r"^LayerNormalization is not supported in fp8 mode \(node l0_ln1\)$")
    # without a LayerNormalization, the attention itself is refused
    p8 = models.write_repo(str(tmp_path), "a8", G.attn_graph(2, 6, 2, 16))
    refused(p8, 2, monkeypatch, prec="fp8", match=r"^attention and token views are not supported in fp8 mode \(node ")


# ---- the reference ------------------------------------------------------------------------------------------------------------------------
def test_reference_walk_is_the_attention_definition():
    """the float64 walk of the unfused graph equals the closed form, in every spelling (the constants are float32: 1e-7)"""
    x = np.random.RandomState(0).randn(2, 3 * 24, 1, 7)
    want = ref64.attention(x[:, :, 0, :].transpose(0, 2, 1), 3, 8 ** -0.5).transpose(0, 2, 1)[:, :, None, :]
    for unbind in G.UNBINDS:
        for scale in G.SCALES:
            for swap in (False, True):
                y = ref64.run_f64(G.attn_graph(2, 7, 3, 8, unbind=unbind, scale=scale, swap=swap), {"x": x})["y"]
                assert y.shape == want.shape and ref64.rel_err(y, want) < 1e-6, (unbind, scale, swap)
    import torch
    import torch.nn.functional as F
    t = torch.from_numpy(x[:, :, 0, :].transpose(0, 2, 1).reshape(2, 7, 3, 3, 8)).permute(2, 0, 3, 1, 4)
    sd = F.scaled_dot_product_attention(t[0], t[1], t[2]).permute(0, 2, 1, 3).reshape(2, 7, 24).numpy()
    assert ref64.rel_err(sd.transpose(0, 2, 1)[:, :, None, :], want) < 1e-12


def test_dropped_class_token_or_position_embedding_would_be_seen():
    """both constants are O(1): the float64 logits of the narrow net move by far more than either GPU bound (3e-3) when one is zeroed"""
    from oracle import onnx_oracle as O
    mb = G.narrow(2)
    x = models.synthetic_input((2, 3, 32, 32), stream="vit")
    ref = ref64.run_f64(mb, {"input": x})["logits"]
    inits = O.load_model(mb).inits
    for name in ("pos_embedding", "class_token"):
        y = ref64.run_f64(mb, {"input": x, name: np.zeros_like(inits[name])})["logits"]           # (a feed overrides the initializer)
        assert ref64.rel_err(y, ref) > 0.05, name


# ---- digests ------------------------------------------------------------------------------------------------------------------------------
def _entries():
    """(key, model, batch, switches): ViT-Tiny/16 in every precision at batch 1 and 32 and with IE_FORCE_TILE 0 / 1, the narrow net in both spellings"""
    out = [(f"vit_tiny_16/{prec}/b{b}", "tiny", b, {"IE_PRECISION": prec}) for prec in ("fp32", "fp16", "fp8") for b in (1, 32)]
    out += [(f"vit_tiny_16/{prec}/b32/IE_FORCE_TILE={t}", "tiny", 32, {"IE_PRECISION": prec, "IE_FORCE_TILE": str(t)}) for prec in PRECS for t in (0, 1)]
    out += [(f"narrow_{unbind}_{scale}/{prec}/b2", f"narrow_{unbind}_{scale}", 2, {"IE_PRECISION": prec})
            for unbind, scale in (("gather", "q"), ("split", "sdpa")) for prec in PRECS]
    return out


def _digests(root):
    paths = {"tiny": models.write_repo(root, "vit_tiny_16", models.vit_tiny_16("N"))}
    for unbind, scale in (("gather", "q"), ("split", "sdpa")):
        paths[f"narrow_{unbind}_{scale}"] = models.write_repo(root, f"narrow_{unbind}_{scale}", G.narrow("N", unbind=unbind, scale=scale))
    return {key: D.digest(paths[model], batch, sw) for key, model, batch, sw in _entries()}


def test_vit_plan_digests(tmp_path, engine_lib):
    want = D.load_golden(GOLDEN)
    got = _digests(str(tmp_path))
    assert sorted(got) == sorted(want)
    bad = {k: (want[k], v) for k, v in got.items() if want[k] != v}
    assert not bad, "%d of %d entries differ from %s (golden, now): %s" % (len(bad), len(got), os.path.basename(GOLDEN), json.dumps(bad, indent=1)[:4000])
    assert sum("error" in v for v in got.values()) == 2               # the two fp8 entries: refusals


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as root:
        D.save_golden(_digests(root), sys.argv[1] if len(sys.argv) > 1 else GOLDEN)
    print(GOLDEN)
