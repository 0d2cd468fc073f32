"""CPU: Llama through the ONNX reader and the planner (EngineDescribeModel): the embedding Gather without a sum, RMSNorm spelled out, the q / k / v
Linears without a bias merged to one of D + 2 Dkv columns, the rotary embedding and repeat_kv inside the attention step, the gated unit as one eltwise
step, the token outputs; every spelling gives one plan and one weight blob; the refusals by node and rule; the default tiles at their limits; the plans
of GPT-2, BERT, ViT and a ConvNeXt block as the parent commit printed them; and what the half format alone costs the narrow model of the GPU test."""
import hashlib
import itertools
import json
import os

import numpy as np
import pytest

import gpt2_graphs as GG
import llama_graphs as LG
import ref64
import test_plan_digests as TPD
import vit_graphs as G
from engine_run import describe, RTOL
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models
from refusals import refused

N, L, V, D, H, HKV, MLP = 2, 40, 61, 128, 4, 2, 256


def _plan(tmp_path, monkeypatch, mb, name="g", batch=N, prec="fp32", **env):
    return describe(models.write_repo(str(tmp_path), name, mb), batch, monkeypatch, prec, **env)


def _refused(tmp_path, monkeypatch, mb, *matches, batch=N, prec="fp32"):
    """the load is refused, and the text holds every one of `matches` (the node and the rule)"""
    refused(mb, batch, monkeypatch, *matches, prec=prec)


@pytest.mark.parametrize("prec", ("fp32", "fp16"))
def test_llama_tiny_plan(tmp_path, monkeypatch, prec, engine_lib):
    p = _plan(tmp_path, monkeypatch, models.llama_tiny(N, last_hidden_state=True), prec=prec)
    layer = ["layer_norm", "conv", "attention", "conv", "layer_norm", "conv", "conv", "eltwise", "conv"]
    assert [s["kind"] for s in p["steps"]] == ["embed"] + 2 * layer + ["layer_norm", "conv", "copy"]
    st = p["steps"]
    assert st[0]["ln"] is False and st[0]["tables"] == 1 and st[0]["vocab"] == [V] and st[0]["pos_off"] == -1 and st[0]["bias_off"] == -1
    hd = D // H
    for b in (1, 10):
        n1, qkv, at, o, n2, gate, up, glu, down = st[b:b + 9]
        for nm in (n1, n2):
            assert nm["rms"] is True and nm["bias_off"] == -1 and nm["bias"] is False
        assert qkv["out"]["c"] == D + 2 * HKV * hd and qkv["bias"] is False and qkv["residual"] is False
        assert at["causal"] is True and at["rope"] is True and at["kv_heads"] == HKV and (at["heads"], at["head_dim"], at["tile"]) == (H, hd, 1) and "key_mask" not in at
        assert at["w_off"] >= 0 and at["w2_off"] > at["w_off"] and at["scale"] == pytest.approx(1.0 / np.sqrt(hd), rel=1e-6)
        assert o["residual"] is True and down["residual"] is True and gate["residual"] is False and up["residual"] is False
        assert gate["out"]["c"] == up["out"]["c"] == MLP and gate["in"] == up["in"]
        assert glu["mul"] is True and glu["pre_act"][0] == "silu" and "act" not in glu
    assert st[19]["rms"] is True
    assert [o["dims"] for o in p["outputs"]] == [[N, L, V], [N, L, D]]
    assert st[-2]["out"]["buf"] == p["outputs"][0]["view"]["buf"] and st[-1]["name"] == "to_output(last_hidden_state)"
    # no stand-alone SiLU, Mul, Add, Slice, Concat or Expand step: the eltwise steps are the two gated units
    assert sum(s["kind"] == "eltwise" for s in st) == 2


def _canon(plan):
    """the plan without the node names of its steps (the spellings differ in them and in nothing else)"""
    p = json.loads(json.dumps(plan))
    for s in p["steps"]:
        s.pop("name")
    return json.dumps(p, sort_keys=True)


def test_every_spelling_gives_the_same_plan_and_blob(tmp_path, monkeypatch, engine_lib):
    base = dict(norm="pow", cast=False, swap=False, rope="init", repeat="auto", scale="mul", mask="add")
    variants = [base] + [dict(base, **{k: v}) for k, v in (("norm", "mul"), ("norm", "reciprocal"), ("norm", "mul_reciprocal"), ("norm", "op"), ("cast", True), ("swap", True),
                                                           ("rope", "unsqueeze"), ("rope", "slice"), ("rope", "gather"), ("scale", "div"), ("mask", "where_const"))]
    variants.append(dict(norm="mul_reciprocal", cast=True, swap=True, rope="slice", repeat="auto", scale="div", mask="where_const"))
    seen = set()
    for i, kw in enumerate(variants):
        path = models.write_repo(str(tmp_path), "v%d" % i, models.llama_tiny(N, last_hidden_state=True, **kw))
        plan = describe(path, N, monkeypatch)
        seen.add((_canon(plan), hashlib.sha256(B.PlanWeights(path, N).tobytes()).hexdigest()))
        assert len(seen) == 1, kw
    # a g = 1 Expand (repeat_kv of a model with as many K / V heads as heads) present or absent
    seen = set()
    for i, rep in enumerate(("always", "never")):
        path = models.write_repo(str(tmp_path), "r%d" % i, models.llama_tiny(N, kv_heads=H, repeat=rep))
        plan = describe(path, N, monkeypatch)
        assert "kv_heads" not in [s for s in plan["steps"] if s["kind"] == "attention"][0]
        seen.add((_canon(plan), hashlib.sha256(B.PlanWeights(path, N).tobytes()).hexdigest()))
    assert len(seen) == 1


def test_rms_norm_spellings_alone(tmp_path, monkeypatch, engine_lib):
    seen = set()
    for i, (form, kw) in enumerate([("pow", {}), ("mul", {}), ("reciprocal", {}), ("mul_reciprocal", dict(cast=True, swap=True)), ("pow", dict(cast=True)), ("pow", dict(axes_input=False)),
                                    ("pow", dict(swap=True)), ("op", {})]):
        path = models.write_repo(str(tmp_path), "n%d" % i, LG.rms_graph(N, 5, 64, form=form, **kw))
        plan = describe(path, N, monkeypatch)
        (st,) = [s for s in plan["steps"] if s["kind"] == "layer_norm"]
        assert st["rms"] is True and st["eps"] == pytest.approx(1e-5, rel=1e-6)
        seen.add((_canon(plan), hashlib.sha256(B.PlanWeights(path, N).tobytes()).hexdigest()))
        assert len(seen) == 1, (form, kw)
    (st,) = [s for s in _plan(tmp_path, monkeypatch, LG.rms_cl_graph(N, 8, 3, 5), name="cl")["steps"] if s["kind"] == "layer_norm"]
    assert st["rms"] is True and (st["in"]["h"], st["in"]["w"], st["in"]["c"]) == (3, 5, 8)


def test_gated_unit_spellings(tmp_path, monkeypatch, engine_lib):
    for act, kind in (("silu", "silu"), ("erf", "gelu"), ("op", "gelu"), ("op_tanh", "gelu_tanh")):
        for swap in (False, True):
            steps = _plan(tmp_path, monkeypatch, LG.swiglu_graph(N, 5, 64, 96, act=act, swap=swap), name="glu")["steps"]
            assert [s["kind"] for s in steps] == ["conv", "conv", "eltwise", "conv", "copy"]
            gate, up, glu = steps[:3]
            assert glu["mul"] is True and glu["pre_act"][0] == kind and "act" not in glu and glu["in"]["buf"] == gate["out"]["buf"] and glu["in2"]["buf"] == up["out"]["buf"]
            assert gate["name"].startswith("matmul") and gate["w_off"] < up["w_off"]      # (the activation is on the gate Linear's result, whichever operand order)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals(tmp_path, monkeypatch, engine_lib):
    l, hd = 6, 8
    other = (LG.random_tables(l, hd, seed=4)[0], models.rope_tables(l, hd)[1])
    r = lambda mb, *m, **kw: _refused(tmp_path, monkeypatch, mb, *m, **kw)  # noqa: E731
    r(LG.gqa_attn_graph(N, l, 4, 2, hd, rope_k_tables=other), "the cos table of q (Add add_", "is not the cos table of k (Add add_", "element for element")
    r(LG.gqa_attn_graph(N, l, 4, 2, hd, tables=tuple(t[: l - 1] for t in models.rope_tables(l, hd)), rope="unsqueeze"), "the rope tables (Add add_", "have 5 rows after slicing, the sequence has 6 tokens")
    r(LG.gqa_attn_graph(N, l, 4, 3, hd, repeat="never"), "heads % kv_heads != 0: q has 4 heads (Reshape reshape_", "k has 3 (Reshape reshape_")
    r(LG.gqa_attn_graph(N, l, 4, 2, hd, rope_order="x1_first"), "the rotary embedding of q (Add add_", "is not rotate_half", "the order (x1, -x2) is another function")
    r(LG.gqa_attn_graph(N, l, 4, 2, hd, repeat="never"), "k and v have 2 heads for q's 4, but repeat_kv repeats them 0 times, not 2")
    r(LG.rms_graph(N, 5, 64, axis=1), "RMSNormalization pow_", "axis = 1 on a token view is not supported (only the channel axis alone is normalised")
    r(models.llama_tiny(N), "is not supported in fp8 mode", prec="fp8")
    r(LG.rms_graph(N, 5, 64), "RMSNormalization is not supported in fp8 mode (node pow_", prec="fp8")


def test_rope_with_a_key_mask_and_a_second_reader_are_refused(tmp_path, monkeypatch, engine_lib):
    from gpu_ai_inference_server_amd.modelgen import onnx_pb as pb
    l, hd, heads, kvh = 6, 8, 4, 2
    d, c = heads * hd, (heads + 2 * kvh) * hd

    def graph(edit, extra_inputs=(), extra_outputs=()):
        gb = models.GraphBuilder("gqa", 5)
        t = models.vit_tokens(gb, "x", c)
        real = gb.simple

        def simple(op, xs, attrs=(), out=None):
            return edit(gb, real, op, xs, attrs, out)
        gb.simple = simple
        cs = models.rope_constants(gb, l, hd, "rotary", form="init")
        y = models.llama_attention(gb, t, l, d, heads, kvh, "a", batch=N, rope=cs, mask=None, hd=hd,
                                   linear=lambda y, name, cout: real("MatMul", [y, gb.init(name + "_w", np.ones((c, cout), np.float32))]))
        gb.simple = real
        gb.simple("Reshape", [gb.transpose(y, (0, 2, 1)), gb.init("back_shape", np.array([0, d, 1, l], np.int64))], out="y")
        return gb.finish([("x", [N, c, 1, l])] + list(extra_inputs), [("y", [N, d, 1, l])] + list(extra_outputs), opset=17)

    def key_mask(gb, real, op, xs, attrs, out):
        if op == "Softmax":
            xs = [real("Add", [xs[0], models.bert_extended_mask(gb)])]
        return real(op, xs, attrs, out)
    _refused(tmp_path, monkeypatch, graph(key_mask, [("attention_mask", [N, l], pb.INT64)]), "a rotary embedding (Add add_", "together with a key mask (attention_mask) is not supported")

    state = {}

    def second_reader(gb, real, op, xs, attrs, out):      # one more reader (a dangling Relu) of the first rotate_half's Neg
        y = real(op, xs, attrs, out)
        if op == "Neg" and "done" not in state:
            state["done"] = True
            real("Relu", [y])
        return y
    _refused(tmp_path, monkeypatch, graph(second_reader), "the intermediate neg_", "has 2 readers, not 1")


@pytest.mark.parametrize("l, prec, kvh, env, tile", [
    (288, "fp32", 2, {}, 1), (289, "fp32", 2, {}, 3), (544, "fp16", 1, {}, 1), (545, "fp16", 1, {}, 3), (320, "fp32", 4, {"IE_ATTN_TILE": "2"}, 0),
    (320, "fp32", 2, {"IE_FORCE_TILE": "0"}, 0), (64, "fp32", 2, {"IE_ATTN_TILE": "3"}, 3)])
def test_default_tiles_at_the_limits(tmp_path, monkeypatch, l, prec, kvh, env, tile, engine_lib):
    """hd 64 with the grouped row width: tile 1 up to the LDS budget (288 keys in fp32, 544 in fp16), tile 3 beyond; tile 2 is never a rotary step's"""
    assert G.max_mfma_tokens(64, False) == 288 and G.max_mfma_tokens(64, True) == 544
    (at,) = [s for s in _plan(tmp_path, monkeypatch, LG.gqa_attn_graph(1, l, 4, kvh, 64), batch=1, prec=prec, **env)["steps"] if s["kind"] == "attention"]
    assert at["tile"] == tile and at["rope"] is True and at["causal"] is True
    if not env:
        assert tile == LG.rope_default_tile(l, 64, 4, kvh, prec == "fp16")
    assert at["flops"] == 2.0 * 4 * l * (l + 1) * 64


def test_hd48_and_non_causal_rope_take_the_generic_kernel(tmp_path, monkeypatch, engine_lib):
    (at,) = [s for s in _plan(tmp_path, monkeypatch, LG.gqa_attn_graph(1, 40, 4, 2, 48), batch=1)["steps"] if s["kind"] == "attention"]
    assert at["tile"] == 0 and at["rope"] is True and LG.rope_default_tile(40, 48, 4, 2, False) == 0
    for env in ({}, {"IE_FORCE_TILE": "1"}, {"IE_ATTN_TILE": "3"}):
        (at,) = [s for s in _plan(tmp_path, monkeypatch, LG.gqa_attn_graph(1, 40, 4, 2, 64, causal=False), batch=1, name="nc", **env)["steps"] if s["kind"] == "attention"]
        assert at["tile"] == 0 and at["rope"] is True and "causal" not in at


def test_float64_walk_agrees_across_spellings(engine_lib):
    ids = GG.gpt2_ids(N, L, V)
    a = ref64.run_f64(models.llama_tiny(N), {"input_ids": ids})["logits"]
    # (not scale="div": sqrt(32) and 1 / sqrt(32) are rounded to float32 each, so the two products differ by 1e-8 of the scores, which is no rounding of the walk)
    b = ref64.run_f64(models.llama_tiny(N, norm="op", cast=True, swap=True, rope="gather", mask="where_const"), {"input_ids": ids})["logits"]
    assert a.shape == (N, L, V) and ref64.rel_err(a, b) < 1e-12
    # causality of the reference itself, and the rotation: a later token does not move an earlier row; without the rope the logits are others
    ids2 = ids.copy()
    ids2[:, 20:] = (ids2[:, 20:] + 1) % V
    c = ref64.run_f64(models.llama_tiny(N), {"input_ids": ids2})["logits"]
    assert np.array_equal(a[:, :20], c[:, :20]) and not np.array_equal(a[:, 20:], c[:, 20:])
    # repeat_kv is a repeat_interleave: head h reads K / V head h // group (numpy, on the attention subgraph's own reference)
    l, hd, kvh = 7, 8, 2
    x = LG.gqa_input(1, l, H, kvh, hd)
    y = ref64.run_f64(LG.gqa_attn_graph(1, l, H, kvh, hd, rope=None), {"x": x})["y"][0, :, 0, :].T.reshape(l, H, hd)
    rows = x[0, :, 0, :].T.astype(np.float64)
    q, k, v = rows[:, : H * hd].reshape(l, H, hd), rows[:, H * hd:(H + kvh) * hd].reshape(l, kvh, hd), rows[:, (H + kvh) * hd:].reshape(l, kvh, hd)
    for h in range(H):
        s = q[:, h] @ k[:, h // (H // kvh)].T * float(np.float32(1.0 / np.sqrt(hd))) + np.triu(np.full((l, l), -np.inf), 1)
        pr = np.exp(s - s.max(axis=1, keepdims=True))
        np.testing.assert_allclose(y[:, h], (pr / pr.sum(axis=1, keepdims=True)) @ v[:, h // (H // kvh)], rtol=0, atol=1e-12)


def test_fp16_format_cost_of_the_narrow_model(engine_lib):
    """what the half format alone costs the narrow Llama of tests/test_llama_gpu.py (every stored value rounded to half, arithmetic in double) stays
    under half of the fp16 bound, for both sequence lengths the GPU test runs.  The walk that rounds runs the model with its norms as the RMSNormalization
    operator, the same function (test_float64_walk_agrees_across_spellings): a norm's result is a stored value, the square, the mean and the root inside
    the spelled-out form are not (the kernel keeps them in fp32 registers), and rounding those to half too would charge the format for stores no plan makes"""
    for seq in (40, LG.KC + 8):
        mb = LG.narrow_llama(N, seq=seq, max_pos=seq + 8, norm="op")
        ids = GG.gpt2_ids(N, seq, V)
        ref = ref64.run_f64(LG.narrow_llama(N, seq=seq, max_pos=seq + 8), {"input_ids": ids})
        with np.errstate(over="ignore"):          # (the mask's fill value, finfo(float32).min, is -inf as a half: still a mask)
            half = ref64.run_f64(mb, {"input_ids": ids}, round_half=True)
        for k in ("logits", "last_hidden_state"):
            err = ref64.rel_err(half[k], ref[k])
            print(f"narrow Llama seq {seq} {k}: half storage alone costs {err:.3e} of max|ref| (bound {RTOL['fp16']:.0e})")
            assert err < 0.5 * RTOL["fp16"], (seq, k, err)


def test_parent_plans_are_unchanged(tmp_path, monkeypatch, engine_lib):
    """tests/golden/llama_parent_plans.json: the plan and blob digests (test_plan_digests.digest's form) a build of the parent commit gave for GPT-2, BERT,
    ViT and a ConvNeXt block: graphs with none of the new patterns plan exactly as they did"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "llama_parent_plans.json")) as f:
        parent = json.load(f)
    cases = {"gpt2_tiny": (lambda: models.gpt2_tiny(2), 2), "bert_tiny": (lambda: models.bert_tiny(4), 4), "vit_tiny_16": (lambda: models.vit_tiny_16(2), 2),
             "convnext_block": (lambda: models.convnext_block(2, 96, 14), 2)}
    assert sorted(parent) == sorted(f"{n}/{p}" for n, p in itertools.product(cases, ("fp32", "fp16")))
    for name, (mk, b) in cases.items():
        path = models.write_repo(str(tmp_path), name, mk())
        for prec in ("fp32", "fp16"):
            d = TPD.digest(path, b, {"IE_PRECISION": prec})
            assert " ".join(d[k] for k in ("plan", "weights") if k in d) == parent[f"{name}/{prec}"], (name, prec)
