"""CPU: GPT-2 through the ONNX reader and the planner (EngineDescribeModel): the embedding sum without a LayerNormalization, HF's Conv1D, the causal
attention behind a Split, gelu_new spelled out, the tied head and the token outputs; every spelling gives one plan and one weight blob; the causal
default tiles at their limits; the refusals by node and rule; and the plans of BERT and ViT graphs as the parent commit printed them."""
import hashlib
import itertools
import json
import os

import numpy as np
import pytest

import bert_graphs as BG
import gpt2_graphs as GG
import ref64
import test_plan_digests as TPD
import vit_graphs as G
from engine_run import describe
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models
from gpu_ai_inference_server_amd.modelgen import onnx_pb as pb
from refusals import refused

N, L, V, D, H = 2, 40, 61, 128, 2


def _plan(tmp_path, monkeypatch, mb, name="g", batch=N, prec="fp32", **env):
    return describe(models.write_repo(str(tmp_path), name, mb), batch, monkeypatch, prec, **env)


def _refused(tmp_path, monkeypatch, mb, *matches, batch=N):
    """the load is refused, and the text holds every one of `matches` (the node and the rule)"""
    refused(mb, batch, monkeypatch, *matches)


@pytest.mark.parametrize("prec", ("fp32", "fp16"))
def test_gpt2_tiny_plan(tmp_path, monkeypatch, prec, engine_lib):
    p = _plan(tmp_path, monkeypatch, models.gpt2_tiny(N, last_hidden_state=True), prec=prec)
    layer = ["layer_norm", "conv", "attention", "conv", "layer_norm", "conv", "eltwise", "conv"]
    assert [s["kind"] for s in p["steps"]] == ["embed"] + 2 * layer + ["layer_norm", "conv", "copy"]
    st = p["steps"]
    assert st[0]["ln"] is False and st[0]["tables"] == 1 and st[0]["vocab"] == [V] and st[0]["pos_off"] >= 0 and st[0]["bias_off"] == -1
    for at in (st[3], st[11]):
        assert at["causal"] is True and (at["heads"], at["head_dim"], at["tile"]) == (H, D // H, 1) and "key_mask" not in at
        assert at["scale"] == pytest.approx(1.0 / np.sqrt(D // H), rel=1e-6)
    for proj in (st[4], st[8], st[12], st[16]):
        assert proj["residual"] is True                       # the projections carry the residual Adds
    for g in (st[7], st[15]):
        assert g["act"][0] == "gelu_tanh"                     # ActKind 7, what Gelu(approximate = "tanh") gives
    assert [o["dims"] for o in p["outputs"]] == [[N, L, V], [N, L, D]]
    for o in p["outputs"]:                                    # row-major [N, L, C]: an fp32 NHWC buffer of its own with pitch C
        v = o["view"]
        assert (v["nchw"], v["f16"], v["h"], v["c_off"]) == (False, False, 1, 0) and v["pitch"] == v["c"]
    # the logits come straight from the head conv; last_hidden_state is read further, so it is copied like any other output that is
    assert st[-2]["out"]["buf"] == p["outputs"][0]["view"]["buf"] and st[-1]["name"] == "to_output(last_hidden_state)"
    only = _plan(tmp_path, monkeypatch, models.gpt2_tiny(N), name="only", prec=prec)
    assert [s["kind"] for s in only["steps"]][-2:] == ["layer_norm", "conv"] and "copy" not in [s["kind"] for s in only["steps"]]


def _canon(plan):
    """the plan without the node names of its steps (the spellings differ in them and in nothing else)"""
    p = json.loads(json.dumps(plan))
    for s in p["steps"]:
        s.pop("name")
    return json.dumps(p, sort_keys=True)


def test_every_spelling_gives_the_same_plan_and_blob(tmp_path, monkeypatch, engine_lib):
    base = dict(mask="where_slice", scale="div", ktrans="two", linear="conv1d", gelu="pow", lm_head="transpose", split_attr=True, pos="gather")
    variants = [base] + [dict(base, **{k: v}) for k, v in (("mask", "where_const"), ("mask", "add"), ("scale", "mul"), ("ktrans", "one"), ("linear", "matmul"),
                                                           ("gelu", "mulmul"), ("gelu", "op"), ("lm_head", "init"), ("split_attr", False), ("pos", "const"))]
    variants.append(dict(mask="add", scale="mul", ktrans="one", linear="matmul", gelu="mulmul", lm_head="init", split_attr=False, pos="const"))
    seen = set()
    for i, kw in enumerate(variants):
        path = models.write_repo(str(tmp_path), "v%d" % i, models.gpt2_tiny(N, last_hidden_state=True, **kw))
        plan = describe(path, N, monkeypatch)
        seen.add((_canon(plan), hashlib.sha256(B.PlanWeights(path, N).tobytes()).hexdigest()))
        assert len(seen) == 1, kw


@pytest.mark.parametrize("l, prec, causal, env, tile", [
    (288, "fp32", True, {}, 1), (289, "fp32", True, {}, 3), (544, "fp16", True, {}, 1), (545, "fp16", True, {}, 3),
    (320, "fp32", False, {}, 0), (320, "fp32", False, {"IE_ATTN_TILE": "3"}, 3), (320, "fp32", True, {"IE_ATTN_TILE": "2"}, 0),
    (320, "fp32", True, {"IE_FORCE_TILE": "3"}, 3)])
def test_default_tiles_at_the_limits(tmp_path, monkeypatch, l, prec, causal, env, tile, engine_lib):
    """hd 64: tile 1 up to the LDS budget (288 keys in fp32, 544 in fp16), tile 3 beyond; a non-causal step stays on tile 0 unless IE_ATTN_TILE=3 pins it;
    tile 2 is never a causal step's; IE_FORCE_TILE reaches tiles 0 and 1 only (3 is "not forced": the default stays)"""
    assert G.max_mfma_tokens(64, False) == 288 and G.max_mfma_tokens(64, True) == 544
    (at,) = [s for s in _plan(tmp_path, monkeypatch, GG.causal_attn_graph(1, l, 1, 64, mask="where_const" if causal else None), batch=1, prec=prec, **env)["steps"]
             if s["kind"] == "attention"]
    assert at["tile"] == tile and at.get("causal", False) is causal
    if causal and not env:
        assert tile == GG.causal_default_tile(l, 64, 64, prec == "fp16")
    flops = 2.0 * l * (l + 1) * 64 if causal else 4.0 * l * l * 64
    assert at["flops"] == flops


def test_hd48_takes_the_generic_kernel(tmp_path, monkeypatch, engine_lib):
    (at,) = [s for s in _plan(tmp_path, monkeypatch, GG.causal_attn_graph(1, 40, 2, 48), batch=1)["steps"] if s["kind"] == "attention"]
    assert at["tile"] == 0 and at["causal"] is True and GG.causal_default_tile(40, 48, 96, False) == 0


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def _attn_with(l, build_mask, heads=2, hd=32, n=N):
    """causal_attn_graph with the masking of the scores written by build_mask(gb, scores) -> masked scores"""
    d = heads * hd
    gb = models.GraphBuilder("cattn", 5)
    t = models.vit_tokens(gb, "x", 3 * d)
    real = gb.simple

    def simple(op, xs, attrs=(), out=None):          # the Softmax's input goes through build_mask
        if op == "Softmax":
            xs = [build_mask(gb, xs[0])]
        return real(op, xs, attrs, out)
    gb.simple = simple
    y = models.gpt2_attention(gb, t, l, d, heads, "a", mask=None)
    gb.simple = real
    gb.simple("Reshape", [gb.transpose(y, (0, 2, 1)), gb.init("back_shape", np.array([0, d, 1, l], np.int64))], out="y")
    return gb.finish([("x", [n, 3 * d, 1, l])] + ([("attention_mask", [n, l], pb.INT64)] if build_mask.__name__ == "with_key_mask" else []), [("y", [n, d, 1, l])], opset=17)


def _where(cond, c=models.FLOAT32_MIN):
    def build(gb, s):
        return gb.simple("Where", [gb.init("cond", cond.reshape(1, 1, *cond.shape[-2:])), s, gb.init("fill", np.array(c, np.float32))], out="masked")
    return build


def test_mask_refusals(tmp_path, monkeypatch, engine_lib):
    l = 6
    tril = np.tril(np.ones((l, l), np.bool_))
    one_wrong = tril.copy()
    one_wrong[2, 4] = True
    _refused(tmp_path, monkeypatch, _attn_with(l, _where(one_wrong)), "Where where_", ": its condition is not the causal mask j <= i: element [2, 4] is true")
    _refused(tmp_path, monkeypatch, _attn_with(l, _where(np.tril(np.ones((l, l), np.bool_), -1))), "Where where_", ": its condition is not the causal mask j <= i: element [0, 0] is false")
    _refused(tmp_path, monkeypatch, _attn_with(l, _where(tril, -10000.0)), "Where where_", ": the value -10000.000000 of the masked scores is above -1e30")
    _refused(tmp_path, monkeypatch, _attn_with(l + 1, _where(tril)), "its causal mask is [1, 1, 6, 6], the sequence has 7 tokens")

    def add_const(m):
        def build(gb, s):
            return gb.simple("Add", [s, gb.init("M", m.astype(np.float32))], out="masked")
        return build
    good = np.triu(np.full((l, l), models.FLOAT32_MIN, np.float32), 1).reshape(1, 1, l, l)
    assert [s for s in _plan(tmp_path, monkeypatch, _attn_with(l, add_const(good)), name="ok")["steps"] if s["kind"] == "attention"][0]["causal"] is True
    refusal = ") on the scores is not supported"
    _refused(tmp_path, monkeypatch, _attn_with(l, add_const(np.where(good < 0, np.float32(-10000.0), 0))), "an additive mask (Add add_", refusal)           # the masked keys keep a probability
    _refused(tmp_path, monkeypatch, _attn_with(l, add_const(np.broadcast_to(good, (N, 1, l, l)))), "an additive mask (Add add_", refusal)                    # [N, 1, L, L]
    _refused(tmp_path, monkeypatch, _attn_with(l, add_const(np.broadcast_to(good, (1, 2, l, l)))), "an additive mask (Add add_", refusal)                    # per head
    band = good.copy()
    band[0, 0, 4, 0] = models.FLOAT32_MIN
    _refused(tmp_path, monkeypatch, _attn_with(l, add_const(band)), "an additive mask (Add add_", refusal)                                                   # not triangular

    def not_constant(gb, s):
        return gb.simple("Add", [s, gb.simple("Mul", [s, gb.init("zero", np.array(0.0, np.float32))])], out="masked")
    _refused(tmp_path, monkeypatch, _attn_with(l, not_constant), "an additive mask (Add add_", refusal)

    def with_key_mask(gb, s):
        s = gb.simple("Where", [gb.init("cond", tril.reshape(1, 1, l, l)), s, gb.init("fill", np.array(models.FLOAT32_MIN, np.float32))], out="masked")
        return gb.simple("Add", [s, models.bert_extended_mask(gb)], out="both")
    _refused(tmp_path, monkeypatch, _attn_with(l, with_key_mask), "a causal mask together with a key mask (attention_mask) on the scores is not supported (Where masked below Add add_")


def test_leftover_pow_and_token_reshape_are_refused(tmp_path, monkeypatch, engine_lib):
    def graph(build):
        gb = models.GraphBuilder("bad", 3)
        t = build(gb, models.vit_tokens(gb, "x", 8))
        gb.simple("Reshape", [gb.transpose(t, (0, 2, 1)), gb.init("back_shape", np.array([0, 8, 1, 6], np.int64))], out="y")
        return gb.finish([("x", [2, 8, 1, 6])], [("y", [2, 8, 1, 6])], opset=17)
    # a cube that is not gelu_new's (the constant 0.05 is not 0.044715): nothing matches and the Pow is what it was, an unsupported operator
    def near_miss(gb, t):
        c = lambda name, v: gb.init(name, np.array(v, np.float32))  # noqa: E731
        inner = gb.simple("Add", [t, gb.simple("Mul", [gb.simple("Pow", [t, c("three", 3.0)]), c("c2", 0.05)])])
        th = gb.simple("Tanh", [gb.simple("Mul", [inner, c("c1", np.sqrt(2.0 / np.pi))])])
        return gb.simple("Mul", [gb.simple("Mul", [t, c("half", 0.5)]), gb.simple("Add", [th, c("one", 1.0)])])
    _refused(tmp_path, monkeypatch, graph(near_miss), "Unsupported ONNX operator: Pow (node pow_", batch=2)
    # a Reshape of a token value outside the Conv1D form: [-1, 8] without a Gemm behind it, and a Conv1D whose second Reshape regroups the rows
    flat = lambda gb, t: gb.layernorm(gb.simple("Reshape", [t, gb.init("flat", np.array([-1, 8], np.int64))]), 8, name="ln")  # noqa: E731
    _refused(tmp_path, monkeypatch, graph(flat), "is a token view [N, L, D]; only the [N, L, 3, H, hd] Reshape of the attention pattern may reshape one", batch=2)

    def regroup(gb, t):
        f = gb.simple("Reshape", [t, gb.init("flat", np.array([-1, 8], np.int64))])
        g = gb.simple("Gemm", [f, gb.init("w", np.eye(8, dtype=np.float32)), gb.init("b", np.zeros(8, np.float32))])
        return gb.simple("Reshape", [g, gb.init("back", np.array([3, 4, 8], np.int64))])
    _refused(tmp_path, monkeypatch, graph(regroup), "is a token view [N, L, D]; only the [N, L, 3, H, hd] Reshape of the attention pattern may reshape one", batch=2)


def test_other_output_views_keep_their_refusals(tmp_path, monkeypatch, engine_lib):
    gb = models.GraphBuilder("r", 3)
    flat = gb.simple("Reshape", [gb.conv("x", 8, 8, 1, name="c"), gb.init("flat_shape", np.array([0, 8, -1], np.int64))], out="flat")
    _refused(tmp_path, monkeypatch, gb.finish([("x", [2, 8, 2, 3])], [(flat, [2, 8, 6])], opset=17),
             "graph output flat is a token view; outputs are NCHW: transpose it back with perm [0,2,1] and reshape it to [N, D, h, w]")
    gb = models.GraphBuilder("r", 3)
    cl = gb.transpose(gb.conv("x", 8, 8, 1, name="c"), (0, 2, 3, 1))
    _refused(tmp_path, monkeypatch, gb.finish([("x", [2, 8, 2, 3])], [(cl, [2, 2, 3, 8])], opset=17),
             "is a channels-last view (a Transpose with perm [0,2,3,1]); outputs are NCHW: transpose it back with perm [0,3,1,2]")


def test_which_token_values_may_be_outputs(tmp_path, monkeypatch, engine_lib):
    """a Linear's result (with or without a bias) and a value that is read further are token outputs; a token value that no Linear made and nothing
    else reads keeps the refusal tests/test_vit_plan.py and tests/test_bert_plan.py pin, with its old text"""
    def graph(build):
        gb = models.GraphBuilder("tok", 3)
        outs = build(gb, models.vit_tokens(gb, "x", 8))
        return gb.finish([("x", [2, 8, 2, 3])], [(o, [2, 6, c]) for o, c in outs], opset=17)
    p = _plan(tmp_path, monkeypatch, graph(lambda gb, t: [(gb.linear(gb.layernorm(t, 8, name="ln"), 8, 12, name="head"), 12)]), name="lin")
    assert [s["kind"] for s in p["steps"]][-1] == "conv" and p["steps"][-1]["bias"] is True and p["steps"][-1]["out"] == p["outputs"][0]["view"]
    assert p["outputs"][0]["dims"] == [2, 6, 12] and p["outputs"][0]["view"]["nchw"] is False

    def both(gb, t):
        h = gb.layernorm(t, 8, name="ln")
        return [(gb.simple("MatMul", [h, gb.init("w", np.ones((8, 12), np.float32))]), 12), (h, 8)]
    p = _plan(tmp_path, monkeypatch, graph(both), name="both")
    assert [o["dims"] for o in p["outputs"]] == [[2, 6, 12], [2, 6, 8]] and p["steps"][-1]["name"] == "to_output(ln_out)"
    text = " is a token view; outputs are NCHW: transpose it back with perm [0,2,1] and reshape it to [N, D, h, w]"
    _refused(tmp_path, monkeypatch, graph(lambda gb, t: [(gb.layernorm(t, 8, name="ln"), 8)]), "graph output ln_out" + text)
    _refused(tmp_path, monkeypatch, graph(lambda gb, t: [(gb.gelu(gb.linear(t, 8, 8, name="fc"), "op"), 8)]), "graph output gelu_", text)
    _refused(tmp_path, monkeypatch, models.gpt2_tiny(N, logits=False), "graph output last_hidden_state" + text)


def test_embedding_sums_that_stay_refused(tmp_path, monkeypatch, engine_lib):
    """the norm-less embed step is one table Gather plus position rows; the sums test_bert_plan.py refuses stay refused with their texts"""
    def two_tables(gb):
        t = lambda name, rows: gb.init(name, np.random.RandomState(len(name)).randn(rows, D).astype(np.float32))  # noqa: E731
        s = gb.simple("Add", [gb.simple("Gather", [t("a", V), "input_ids"], [pb.attr_int("axis", 0)]), gb.simple("Gather", [t("b", 2), "token_type_ids"], [pb.attr_int("axis", 0)])])
        return gb.simple("Add", [gb.layernorm(s, D, name="ln"), s], out="y")
    gb = models.GraphBuilder("bad", 3)
    two_tables(gb)
    mb = gb.finish([("input_ids", [N, L], pb.INT64), ("token_type_ids", [N, L], pb.INT64)], [("y", [N, L, D])], opset=17)
    _refused(tmp_path, monkeypatch, mb, "readers; the sum of the embedding gathers is read by its LayerNormalization alone")


def test_embed_sum_graph_plan_and_fp8(tmp_path, monkeypatch, engine_lib):
    for pos in ("gather", "const"):
        p = _plan(tmp_path, monkeypatch, GG.embed_sum_graph(N, L, V, D, pos=pos), name="e" + pos)
        assert [s["kind"] for s in p["steps"]] == ["embed", "layer_norm", "eltwise", "copy", "copy"] and p["steps"][0]["ln"] is False
        assert [o["dims"] for o in p["outputs"]] == [[N, L, D], [N, D, 1, L]]
    path = models.write_repo(str(tmp_path), "f8", models.gpt2_tiny(N))
    refused(path, N, monkeypatch, prec="fp8", match="is not supported in fp8 mode")


def test_float64_walk_agrees_across_spellings(engine_lib):
    """the spellings are one function: the float64 walks of two far-apart spellings agree to rounding"""
    ids = GG.gpt2_ids(N, L, V)
    a = ref64.run_f64(models.gpt2_tiny(N), {"input_ids": ids})["logits"]
    b = ref64.run_f64(models.gpt2_tiny(N, mask="add", scale="mul", ktrans="one", linear="matmul", gelu="mulmul", lm_head="init", split_attr=False, pos="const"), {"input_ids": ids})["logits"]
    assert a.shape == (N, L, V) and ref64.rel_err(a, b) < 1e-12
    # causality of the reference itself: a later token does not move an earlier row
    ids2 = ids.copy()
    ids2[:, 20:] = (ids2[:, 20:] + 1) % V
    c = ref64.run_f64(models.gpt2_tiny(N), {"input_ids": ids2})["logits"]
    assert np.array_equal(a[:, :20], c[:, :20]) and not np.array_equal(a[:, 20:], c[:, 20:])


def test_fp16_format_cost_of_the_narrow_model(engine_lib):
    """what the half format alone costs the narrow GPT-2 of tests/test_gpt2_gpu.py (every stored value rounded to half, arithmetic in double) stays
    under half of the fp16 bound, for both sequence lengths the GPU test runs"""
    from engine_run import RTOL
    for seq in (40, GG.KC + 8):
        mb = GG.narrow_gpt2(N, seq=seq, max_pos=seq + 8)
        ids = GG.gpt2_ids(N, seq, V)
        ref = ref64.run_f64(mb, {"input_ids": ids})
        with np.errstate(over="ignore"):          # (the mask's fill value, finfo(float32).min, is -inf as a half: still a mask)
            half = ref64.run_f64(mb, {"input_ids": ids}, round_half=True)
        for k in ("logits", "last_hidden_state"):
            err = ref64.rel_err(half[k], ref[k])
            print(f"narrow GPT-2 seq {seq} {k}: half storage alone costs {err:.3e} of max|ref| (bound {RTOL['fp16']:.0e})")
            assert err < 0.5 * RTOL["fp16"], (seq, k, err)


def test_bert_and_vit_plans_are_the_parents(tmp_path, monkeypatch, engine_lib):
    """tests/golden/gpt2_parent_plans.json: the plan and blob digests (test_plan_digests.digest's form) the parent commit gave for BERT, ViT and two
    bare attention graphs at the tile-1 limit; and the pinned matrix itself still holds for a model of each family it covers"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gpt2_parent_plans.json")) as f:
        parent = json.load(f)
    cases = {"narrow_bert": (lambda: BG.narrow_bert(3), 3), "narrow_vit": (lambda: G.narrow(2), 2), "bert_tiny": (lambda: models.bert_tiny(4), 4),
             "vit_attn_288": (lambda: G.attn_graph(1, 288, 1, 64), 1), "vit_attn_320": (lambda: G.attn_graph(1, 320, 1, 64), 1)}
    assert sorted(parent) == sorted(f"{n}/{p}" for n, p in itertools.product(cases, ("fp32", "fp16")))
    for name, (mk, b) in cases.items():
        path = models.write_repo(str(tmp_path), name, mk())
        for prec in ("fp32", "fp16"):
            d = TPD.digest(path, b, {"IE_PRECISION": prec})
            assert " ".join(d[k] for k in ("plan", "weights") if k in d) == parent[f"{name}/{prec}"], (name, prec)
    golden = TPD.load_golden()
    for name in ("gemm_mlp", "mini_resnet_block"):
        got = TPD.model_digests(name, str(tmp_path))
        assert got and all(golden[k] == v for k, v in got.items())
