"""CPU: integer graph inputs and the token embedding through the ONNX reader and the planner (EngineDescribeModel), and the BERT graph writer.

* the embedding sum (one or two table Gathers by INT64 graph inputs, position rows as a constant or as Gather + Slice, either Add order) and the
  LayerNormalization behind it are ONE embed step in every spelling, the same plan modulo names; the tables sit in the weight blob as the graph holds them
* INT64 inputs in DescribeModel: element type 7, 8-byte buffers, the memory estimate
* every near miss is refused by name, and the refusals older tests pin still fire
* modelgen.models.bert: the float64 walk of the graph (tests/ref64.py) agrees with an independent torch restatement of the model to 1e-10, and the
  type table, the position rows and the mask each move the narrow net's logits by more than 5 %
* whole encoders: bert_base is 1 embed + 12 x 8 steps + head without a copy; the three q / k / v Linears are ONE qkv conv whose blob is the concatenation
  of the graph's matrices; every spelling (Unsqueeze forms, k-transpose forms, Div / Mul scale, Add operand order, position forms) is the same plan; near
  misses of the q / k / v Linears are refused by name, every other additive mask with the text the ViT tests pin
"""
import numpy as np
import pytest

import bert_graphs as G
import ref64
from engine_run import describe_model, RTOL
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models
from gpu_ai_inference_server_amd.modelgen import onnx_pb as pb
from oracle import onnx_oracle as O
from refusals import refused

PRECS = ("fp32", "fp16")
N, L, V, D = 2, 5, 37, 8


def _refused(tmp_path, monkeypatch, mb, text, prec="fp32", batch=N):
    refused(mb, batch, monkeypatch, text, prec=prec)


def _nameless(step):
    return {k: v for k, v in step.items() if k != "name"}


# ---- the embed step ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_embed_plan(tmp_path, monkeypatch, prec):
    path = models.write_repo(str(tmp_path), "embed", G.embed_graph(N, L, V, D))
    d = describe_model(path, N, monkeypatch, prec)
    steps = d["plan"]["steps"]
    assert [s["kind"] for s in steps] == ["embed", "copy"]
    em = steps[0]
    f16 = prec == "fp16"
    for key in ("in", "in2"):
        assert em[key]["i64"] and (em[key]["n"], em[key]["c"], em[key]["h"], em[key]["w"], em[key]["pitch"]) == (N, L, 1, 1, L) and not em[key]["f16"]
    assert em["in"]["buf"] != em["in2"]["buf"]
    assert (em["out"]["n"], em["out"]["c"], em["out"]["h"], em["out"]["w"], em["out"]["f16"]) == (N, D, 1, L, f16) and "i64" not in em["out"]
    assert em["tables"] == 2 and em["vocab"] == [V, 2] and em["ln"] is True and em["eps"] == float(np.float32(1e-12))
    assert em["tile"] == G.embed_default_tile(D, f16) == 1
    assert em["flops"] == 8 * N * L * D
    assert em["bytes"] == N * L * (3 * 4 * D + 2 * 8) + N * L * D * (2 if f16 else 4)          # three fp32 rows and two ids read, the row written once
    # the tables, the position rows, gamma and beta: fp32 in the blob in both precisions, as the graph holds them
    m = O.load_model(G.embed_graph(N, L, V, D))
    w = B.PlanWeights(path, N)
    blob = lambda off, name: np.testing.assert_array_equal(w[off:off + m.inits[name].size], np.asarray(m.inits[name], np.float32).ravel())  # noqa: E731
    blob(em["w_off"], "word_embeddings")
    blob(em["w2_off"], "token_type_embeddings")
    blob(em["pos_off"], "position_rows")
    blob(em["bias_off"], "emb_ln_scale")
    blob(em["bias2_off"], "emb_ln_B")


@pytest.mark.parametrize("prec", PRECS)
def test_every_spelling_is_the_same_plan(tmp_path, monkeypatch, prec):
    """Add order, and the position rows as a constant or as Gather(table, Slice(position_ids)): the same steps and the same blob, modulo names"""
    plans, blobs = [], []
    for i, kw in enumerate([dict(), dict(order="wpt"), dict(order="ptw"), dict(pos="gather"), dict(pos="gather", order="ptw")]):
        path = models.write_repo(str(tmp_path), f"e{i}", G.embed_graph(N, L, V, D, **kw))
        plans.append([_nameless(s) for s in describe_model(path, N, monkeypatch, prec)["plan"]["steps"]])
        blobs.append(B.PlanWeights(path, N))
    for p, w in zip(plans[1:], blobs[1:]):
        assert p == plans[0]
        np.testing.assert_array_equal(w, blobs[0])


def test_embed_without_type_table_or_positions(tmp_path, monkeypatch):
    path = models.write_repo(str(tmp_path), "embed", G.embed_graph(N, L, V, D, types=0, pos=None))
    em = describe_model(path, N, monkeypatch)["plan"]["steps"][0]
    assert em["kind"] == "embed" and "in2" not in em and em["tables"] == 1 and em["vocab"] == [V] and em["w2_off"] == -1 and em["pos_off"] == -1
    assert em["bytes"] == N * L * (4 * D + 8) + N * L * D * 4


@pytest.mark.parametrize("d,f16,forced,tile", [(8, False, 4, 4), (8, False, 0, 0), (20, True, 1, 0), (20, False, 2, 2), (7, False, 1, 0), (3080, False, 4, 0), (768, True, 2, 2), (768, False, 2, 0)])
def test_forced_embed_tiles(tmp_path, monkeypatch, d, f16, forced, tile):
    """IE_FORCE_TILE picks the lane group where kernels.h EmbedTileFits allows it, else the generic kernel"""
    path = models.write_repo(str(tmp_path), "embed", G.embed_graph(1, 3, 5, d))
    em = describe_model(path, 1, monkeypatch, "fp16" if f16 else "fp32", IE_FORCE_TILE=str(forced))["plan"]["steps"][0]
    assert em["tile"] == tile == (forced if forced == 0 or G.embed_tile_fits(d, f16, forced) else 0)


def test_int64_inputs_in_describe_model(tmp_path, monkeypatch):
    path = models.write_repo(str(tmp_path), "embed", G.embed_graph("N", L, V, D))
    d = describe_model(path, 3, monkeypatch)
    assert d["inputs"] == [{"name": "input_ids", "elem_type": 7, "dims": [-1, L]}, {"name": "token_type_ids", "elem_type": 7, "dims": [-1, L]}]
    assert d["outputs"][0]["elem_type"] == 1
    # the reference's estimate: the I/O tensors over their positive dims (8-byte ids) + 10 MiB
    assert d["memory_usage_bytes"] == 2 * L * 8 + D * L * 4 + 10 * 1024 * 1024
    p = d["plan"]
    assert [i["view"].get("i64", False) for i in p["inputs"]] == [True, True] and [i["dims"] for i in p["inputs"]] == [[3, L], [3, L]]
    ids, tt, tok, out = p["buffers"]
    assert (ids, tt, tok, out) == (3 * L, 3 * L, 3 * L * D, 3 * L * D)
    assert p["activation_bytes"] == 2 * 3 * L * 8 + 2 * 3 * L * D * 4


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def _custom(build, ins=(("input_ids", [N, L], pb.INT64), ("token_type_ids", [N, L], pb.INT64)), out=("y", [N, D, 1, L])):
    gb = models.GraphBuilder("bad", 3)
    t = build(gb)
    if t is not None:
        gb.simple("Reshape", [gb.transpose(t, (0, 2, 1)), gb.init("back_shape", np.array([0, D, 1, L], np.int64))], out="y")
    return gb.finish(list(ins), [out], opset=17)


def _table(gb, name, rows=V, d=D):
    return gb.init(name, np.random.RandomState(len(name)).randn(rows, d).astype(np.float32))


def _gather(gb, table, ids):
    return gb.simple("Gather", [table, ids], [pb.attr_int("axis", 0)])


def test_three_gathers_are_refused(tmp_path, monkeypatch):
    ins = [(n, [N, L], pb.INT64) for n in ("input_ids", "token_type_ids", "third_ids")]
    mb = _custom(lambda gb: gb.layernorm(gb.simple("Add", [gb.simple("Add", [_gather(gb, _table(gb, "a"), "input_ids"), _gather(gb, _table(gb, "b"), "token_type_ids")]),
                                                          _gather(gb, _table(gb, "c"), "third_ids")]), D, name="ln"), ins)
    _refused(tmp_path, monkeypatch, mb, "LayerNormalization ln: the embedding sum has 3 table Gathers by graph inputs (one or two are supported)")


def test_gather_by_a_non_input_is_refused(tmp_path, monkeypatch):
    def build(gb):
        x = gb.layernorm(_gather(gb, _table(gb, "a"), "input_ids"), D, name="ln")
        return gb.layernorm(_gather(gb, _table(gb, "b", rows=D), x), D, name="ln2")
    _refused(tmp_path, monkeypatch, _custom(build), "of an embedding table are not an INT64 graph input [N, L] (only a graph input may index a table)")


def test_table_must_be_2d(tmp_path, monkeypatch):
    def build(gb):
        t3 = gb.init("t3", np.zeros((V, 1, D), np.float32))
        return gb.layernorm(_gather(gb, t3, "input_ids"), D, name="ln")
    _refused(tmp_path, monkeypatch, _custom(build, ins=[("input_ids", [N, L], pb.INT64)]), "the embedding table t3 must be a 2-D floating-point initializer [V, D] (it has rank 3)")


def test_second_reader_of_the_sum_is_refused(tmp_path, monkeypatch):
    def build(gb):
        s = gb.simple("Add", [_gather(gb, _table(gb, "a"), "input_ids"), _gather(gb, _table(gb, "b", rows=2), "token_type_ids")])
        y = gb.layernorm(s, D, name="ln")
        return gb.simple("Add", [y, s])
    _refused(tmp_path, monkeypatch, _custom(build), "readers; the sum of the embedding gathers is read by its LayerNormalization alone")


def test_sum_without_layernorm_is_refused(tmp_path, monkeypatch):
    mb = _custom(lambda gb: gb.gelu(_gather(gb, _table(gb, "a"), "input_ids"), "op"), ins=[("input_ids", [N, L], pb.INT64)])
    _refused(tmp_path, monkeypatch, mb, "reads the embedding sum")


def test_other_readers_of_an_id_input_are_refused(tmp_path, monkeypatch):
    def build(gb):
        gb.simple("Cast", ["token_type_ids"], [pb.attr_int("to", pb.FLOAT)])
        return gb.layernorm(_gather(gb, _table(gb, "a"), "input_ids"), D, name="ln")
    _refused(tmp_path, monkeypatch, _custom(build), "reads the INT64 graph input token_type_ids; only the Gather (axis 0) of a floating-point embedding table [V, D] may read one")


def test_other_integer_inputs_keep_their_refusal(tmp_path, monkeypatch):
    build = lambda gb: gb.layernorm(_gather(gb, _table(gb, "a"), "input_ids"), D, name="ln")  # noqa: E731
    _refused(tmp_path, monkeypatch, _custom(build, ins=[("input_ids", [N, L], pb.INT32)]), "Unsupported data type for input: input_ids")
    _refused(tmp_path, monkeypatch, _custom(build, ins=[("input_ids", [N, L, 1], pb.INT64)]), "Unsupported data type for input: input_ids")


def test_token_output_is_still_refused(tmp_path, monkeypatch):
    gb = models.GraphBuilder("bad", 3)
    gb.nodes.append(pb.node("LayerNormalization", [_gather(gb, _table(gb, "a"), "input_ids"), gb.init("g", np.ones(D, np.float32))], ["y"], "ln", [pb.attr_int("axis", -1)]))
    mb = gb.finish([("input_ids", [N, L], pb.INT64)], [("y", [N, L, D])], opset=17)
    _refused(tmp_path, monkeypatch, mb, "graph output y is a token view")


def test_fp8_is_refused_by_the_first_layernorm(tmp_path, monkeypatch):
    _refused(tmp_path, monkeypatch, G.embed_graph(N, L, V, D), "LayerNormalization is not supported in fp8 mode", prec="fp8")


# ---- the whole encoder -------------------------------------------------------------------------------------------------------------------------
# (the engine runs a GELU behind a Linear as an eltwise step of its own, as in the ViT and ConvNeXt plans: a layer is eight steps, "fc1 + GELU" two of them)
LAYER = ["conv", "attention", "conv", "layer_norm", "conv", "eltwise", "conv", "layer_norm"]


def _check_encoder(steps, depth, dim, heads, mlp, n, seq, f16, c):
    assert [s["kind"] for s in steps] == ["embed"] + LAYER * depth + ["conv", "eltwise", "conv"], [(s["kind"], s["name"]) for s in steps]
    masks = set()
    for li in range(depth):
        qkv, at, proj, ln1, fc1, gelu, fc2, ln2 = steps[1 + 8 * li: 9 + 8 * li]
        assert (qkv["in"]["c"], qkv["out"]["c"], qkv["out"]["w"], qkv["k"]) == (dim, 3 * dim, seq, [1, 1]) and qkv["bias"] and not qkv["residual"]
        assert (at["heads"], at["head_dim"], at["key_mask"], at["mask_value"]) == (heads, dim // heads, True, c) and abs(at["scale"] * (dim // heads) ** 0.5 - 1) < 1e-6
        assert at["in"]["buf"] == qkv["out"]["buf"] and at["out"]["buf"] == proj["in"]["buf"] and at["in2"]["i64"] and (at["in2"]["n"], at["in2"]["c"]) == (n, seq)
        assert at["tile"] == 1 and at["in"]["f16"] == at["out"]["f16"] == f16
        assert at["bytes"] == (2 if f16 else 4) * n * seq * 4 * dim + 8 * n * seq
        masks.add(at["in2"]["buf"])
        assert proj["residual"] and proj["bias"] and fc2["residual"] and fc2["bias"] and not fc1["residual"] and gelu["act"] == ["gelu", 0, 0]
        assert (fc1["out"]["c"], fc2["in"]["c"], fc2["out"]["c"]) == (mlp, mlp, dim)
        assert ln1.get("name", f"l{li}_ln1") == f"l{li}_ln1" and ln2.get("name", f"l{li}_ln2") == f"l{li}_ln2"
    assert len(masks) == 1                              # one mask buffer, matched once, shared by all layers
    pooler, tanh, cls = steps[-3:]
    assert (pooler["in"]["w"], pooler["in"]["h"], pooler["in"]["c"], pooler["in"]["pitch"]) == (1, 1, dim, seq * dim)       # the class token: a view of row 0, no step
    assert tanh["act"] == ["tanh", 0, 0] and cls["out"]["c"] == 2


@pytest.mark.parametrize("prec", PRECS)
def test_bert_base_plan(tmp_path, monkeypatch, prec):
    """1 embed + 12 x (qkv conv, attention with key_mask, proj conv + residual, LN, fc1, GELU, fc2 + residual, LN) + head; no copy step (logits is the last conv's output)"""
    path = models.write_repo(str(tmp_path), "bert", models.bert_base(2, vocab=1000))          # (the plan does not depend on the vocabulary; 30522 rows are 94 MB)
    steps = describe_model(path, 2, monkeypatch, prec)["plan"]["steps"]
    assert "copy" not in [s["kind"] for s in steps]
    _check_encoder(steps, 12, 768, 12, 3072, 2, 128, prec == "fp16", float(np.finfo(np.float32).min))
    assert steps[0]["tile"] == (3 if prec == "fp16" else 4) and steps[0]["vocab"] == [1000, 2]


VARIANTS = [dict(unsqueeze="one"), dict(ktrans="one"), dict(scale="mul"), dict(mask_swap=True), dict(pos="gather"), dict(order="ptw")]


@pytest.mark.parametrize("prec", PRECS)
def test_every_encoder_spelling_is_the_same_plan(tmp_path, monkeypatch, prec):
    def plan(i, **kw):
        path = models.write_repo(str(tmp_path), f"b{i}", NARROW(**kw))
        return [_nameless(s) for s in describe_model(path, 3, monkeypatch, prec)["plan"]["steps"]], B.PlanWeights(path, 3)
    base, blob = plan(0)
    _check_encoder(base[:-1], 2, 64, 2, 128, 3, 40, prec == "fp16", float(np.finfo(np.float32).min))
    assert base[-1]["kind"] == "copy"                   # pooler_output is read by the classifier too: it is copied to its own output buffer
    for i, kw in enumerate(VARIANTS):
        p, w = plan(i + 1, **kw)
        if kw == dict(scale="mul"):                     # 1 / sqrt(hd) rounded to fp32 is not the reciprocal of sqrt(hd) rounded to fp32: the last bit of the scale may differ
            for a, b in zip(p, base):
                if a["kind"] == "attention":
                    assert abs(a["scale"] / b["scale"] - 1) < 1e-6
                    a["scale"] = b["scale"]
        assert p == base, kw
        np.testing.assert_array_equal(w, blob)
    p, _ = plan(9, mask_value=-10000.0)
    assert [s["mask_value"] for s in p if s["kind"] == "attention"] == [-10000.0, -10000.0]


def test_merged_qkv_weights_are_the_concatenation(tmp_path, monkeypatch):
    mb = NARROW()
    path = models.write_repo(str(tmp_path), "bert", mb)
    steps = describe_model(path, 3, monkeypatch)["plan"]["steps"]
    m = O.load_model(mb)
    w = B.PlanWeights(path, 3)
    for li in range(2):
        qkv = steps[1 + 8 * li]
        cat = np.concatenate([np.asarray(m.inits[f"l{li}_attn_{s}_w"], np.float32) for s in ("query", "key", "value")], axis=1)       # [Din, 3 D]: column s D + h hd + e
        np.testing.assert_array_equal(w[qkv["w_off"]:qkv["w_off"] + cat.size].reshape(3 * 64, 64), cat.T)                         # the conv's weights are [Cout][Cin]
        bias = np.concatenate([np.asarray(m.inits[f"l{li}_attn_{s}_b"], np.float32) for s in ("query", "key", "value")])
        np.testing.assert_array_equal(w[qkv["bias_off"]:qkv["bias_off"] + 3 * 64], bias)


def _attn_only(**kw):
    """tokens from a float input -> bert attention -> y, for the near misses"""
    def build(linear=None, ext=None, mask_input=True, tail=None):
        gb = models.GraphBuilder("bad", 3)
        t = models.vit_tokens(gb, "x", 64)
        e = ext(gb) if ext else models.bert_extended_mask(gb)
        y = models.bert_attention(gb, t, e, 64, 2, "a", linear=(lambda y_, name: linear(gb, t, y_, name)) if linear else None)
        if tail:
            y = tail(gb, y)
        gb.simple("Reshape", [gb.transpose(y, (0, 2, 1)), gb.init("back_shape", np.array([0, 64, 1, 9], np.int64))], out="y")
        ins = [("x", [2, 64, 1, 9])] + ([("attention_mask", [2, 9], pb.INT64)] if mask_input else [])
        return gb.finish(ins, [("y", [2, 64, 1, 9])], opset=17)
    return build(**kw)


def test_attention_near_misses_are_refused(tmp_path, monkeypatch):
    # a q / k / v Linear with another reader
    extra = {}

    def second_reader(gb, t, y, name):
        out = gb.linear(y, 64, 64, name=name)
        if name.endswith("key"):
            extra["k"] = out
        return out
    mb = _attn_only(linear=second_reader, tail=lambda gb, y: gb.simple("Add", [y, extra["k"]]))
    _refused(tmp_path, monkeypatch, mb, "readers, not 1 (only its own attention may read it)")
    # different inputs
    def other_input(gb, t, y, name):
        return gb.linear(gb.layernorm(y, 64, name="side_ln") if name.endswith("value") else y, 64, 64, name=name)
    _refused(tmp_path, monkeypatch, _attn_only(linear=other_input), "(q, k and v must come from the same tokens)")
    # mismatched shapes: v from a wider Linear input
    def wide(gb, t, y, name):
        return gb.linear(gb.linear(y, 64, 96, name="widen"), 96, 64, name=name) if name.endswith("value") else gb.linear(y, 64, 64, name=name)
    _refused(tmp_path, monkeypatch, _attn_only(linear=wide), "(q, k and v must come from the same tokens)")


@pytest.mark.parametrize("shape", [(1, 1, 1, 9), (2, 1, 9, 9), (1, 2, 1, 9)], ids=str)
def test_other_masks_keep_the_old_refusal(tmp_path, monkeypatch, shape):
    """a constant mask, [N, 1, L, L] and a per-head mask: `an additive mask`, as the ViT tests pin it"""
    ext = lambda gb: gb.init("const_mask", np.zeros(shape, np.float32))  # noqa: E731
    _refused(tmp_path, monkeypatch, _attn_only(ext=ext, mask_input=False), "an additive mask (Add ")


def test_a_float_activation_as_mask_keeps_the_old_refusal(tmp_path, monkeypatch):
    def ext(gb):
        return gb.simple("Mul", [gb.simple("Sub", [gb.init("one", np.array(1.0, np.float32)), "fmask"]), gb.init("c", np.array(-10000.0, np.float32))])
    gb = models.GraphBuilder("bad", 3)
    t = models.vit_tokens(gb, "x", 64)
    y = models.bert_attention(gb, t, ext(gb), 64, 2, "a")
    gb.simple("Reshape", [gb.transpose(y, (0, 2, 1)), gb.init("back_shape", np.array([0, 64, 1, 9], np.int64))], out="y")
    mb = gb.finish([("x", [2, 64, 1, 9]), ("fmask", [2, 1, 1, 9])], [("y", [2, 64, 1, 9])], opset=17)
    _refused(tmp_path, monkeypatch, mb, "an additive mask (Add ")


def test_left_over_chain_ops_stay_unsupported(tmp_path, monkeypatch):
    for op, attrs in (("Cast", [pb.attr_int("to", pb.FLOAT)]), ("Tanh", None)):
        gb = models.GraphBuilder("bad", 3)
        y = gb.simple(op, [gb.conv("x", 3, 8, 1, name="c")], attrs or [])
        gb.conv(y, 8, 8, 1, name="c2", out="y")
        mb = gb.finish([("x", [2, 3, 4, 4])], [("y", [2, 8, 4, 4])], opset=17)
        path = models.write_repo(str(tmp_path), "left" + op, mb)
        if op == "Tanh":
            steps = describe_model(path, 2, monkeypatch)["plan"]["steps"]
            assert any(s.get("act", [None])[0] == "tanh" for s in steps)
        else:
            refused(path, 2, monkeypatch, match="Unsupported ONNX operator: Cast")


# ---- the graph writer ------------------------------------------------------------------------------------------------------------------------
def NARROW(**kw):
    return models.bert(3, **dict(dict(seq=40, vocab=50, dim=64, depth=2, heads=2, mlp=128, max_pos=64, pooler_output=True), **kw))


def torch_bert(mb, feeds, c):
    """the same model restated with torch (float64, CPU): nn.Embedding, F.layer_norm, softmax, the graph's own weights"""
    import torch
    import torch.nn.functional as F
    m = O.load_model(mb)
    W = {k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in m.inits.items() if np.asarray(v).dtype.kind == "f"}
    ids, tt, mask = (torch.from_numpy(feeds[k]) for k in ("input_ids", "token_type_ids", "attention_mask"))
    dim, heads, eps = W["word_embeddings"].shape[1], 2, 1e-12
    emb = lambda name: torch.nn.Embedding.from_pretrained(W[name], freeze=True)  # noqa: E731
    ln = lambda x, name: F.layer_norm(x, (dim,), W[name + "_scale"], W[name + "_B"], float(np.float32(eps)))  # noqa: E731
    lin = lambda x, name: x @ W[name + "_w"] + W[name + "_b"]  # noqa: E731
    x = ln(emb("word_embeddings")(ids) + emb("token_type_embeddings")(tt) + W["position_rows"], "emb_ln")
    ext = (1.0 - mask[:, None, None, :].to(torch.float64)) * c
    n, l = ids.shape
    li = 0
    while f"l{li}_attn_query_w" in W:
        t = f"l{li}"
        heads_of = lambda y: y.view(n, l, heads, dim // heads).permute(0, 2, 1, 3)  # noqa: E731
        q, k, v = (heads_of(lin(x, f"{t}_attn_{s}")) for s in ("query", "key", "value"))
        p = torch.softmax(q @ k.transpose(-1, -2) / np.sqrt(np.float32(dim // heads)).astype(np.float64) + ext, -1)
        y = (p @ v).permute(0, 2, 1, 3).reshape(n, l, dim)
        x = ln(lin(y, t + "_out") + x, t + "_ln1")
        y = lin(x, t + "_fc1")
        y = 0.5 * y * (1.0 + torch.erf(y / np.float64(np.float32(np.sqrt(2.0)))))
        x = ln(lin(y, t + "_fc2") + x, t + "_ln2")
        li += 1
    pooled = torch.tanh(x[:, 0] @ W["pooler_w"].T + W["pooler_b"])
    return {"logits": (pooled @ W["classifier_w"].T + W["classifier_b"]).numpy(), "pooler_output": pooled.numpy()}


@pytest.mark.parametrize("mask_value", ["min", -10000.0])
def test_walk_agrees_with_torch(mask_value):
    mb = NARROW(mask_value=mask_value)
    ref = ref64.run_f64(mb, G.narrow_feeds())
    c = float(np.finfo(np.float32).min) if mask_value == "min" else -10000.0
    other = torch_bert(mb, G.narrow_feeds(), c)
    for k in ("logits", "pooler_output"):
        assert np.isfinite(ref[k]).all()
        assert ref64.rel_err(other[k], ref[k]) < 1e-10, k


def test_every_spelling_walks_to_the_same_logits():
    ref = ref64.run_f64(NARROW(), G.narrow_feeds())["logits"]
    for kw in (dict(unsqueeze="one"), dict(ktrans="one"), dict(scale="mul"), dict(mask_swap=True), dict(pos="gather"), dict(order="ptw")):
        assert ref64.rel_err(ref64.run_f64(NARROW(**kw), G.narrow_feeds())["logits"], ref) < 1e-6, kw


def test_type_table_positions_and_mask_matter():
    """zeroing the type table, the position rows or the mask each move the narrow net's float64 logits by more than 5 %"""
    mb = NARROW()
    ref = ref64.run_f64(mb, G.narrow_feeds())["logits"]
    m = O.load_model(mb)

    def without(name):
        z = np.zeros_like(np.asarray(m.inits[name]))
        return mb.replace(pb.tensor(name, np.asarray(m.inits[name])), pb.tensor(name, z))

    for name in ("token_type_embeddings", "position_rows"):
        changed = without(name)
        assert changed != mb
        moved = ref64.rel_err(ref64.run_f64(changed, G.narrow_feeds())["logits"], ref)
        print(f"without {name}: logits move by {moved:.3f} of max|ref|")
        assert moved > 0.05, (name, moved)
    feeds = dict(G.narrow_feeds(), attention_mask=np.ones((3, 40), np.int64))
    moved = ref64.rel_err(ref64.run_f64(mb, feeds)["logits"][1:], ref[1:])          # (image 0 has no padding)
    print(f"without the mask: logits move by {moved:.3f} of max|ref|")
    assert moved > 0.05, moved


# ---- what the GPU tests' data is claimed to show, checked here on the CPU ------------------------------------------------------------------------
def test_embed_tiles_are_as_the_shapes_claim():
    assert [G.embed_default_tile(d, False) for d in (8, 20, 7, 768, 3080)] == [1, 1, 0, 4, 0]
    assert [G.embed_default_tile(d, True) for d in (8, 20, 7, 768, 3080)] == [1, 0, 0, 3, 0]
    assert 768 // 4 == 3 * 64                                # three fp32 vectors per lane on the 64-lane group


def test_the_offset_tables_need_the_centred_variance():
    """a LayerNormalization of the test's own mean-100 rows with var = E[x^2] - mean^2 in fp32 misses the fp32 bound the GPU test holds the kernel to"""
    n, l, v, d = 2, 4, 11, 768
    mb, ref = G.embed_graph_and_reference(n, l, v, d, "offset", 2, "const")
    m = O.load_model(mb)
    ids, tt = G.make_ids(n, l, v)
    f32 = lambda name: np.asarray(m.inits[name], np.float32)  # noqa: E731
    x = f32("word_embeddings")[ids] + f32("token_type_embeddings")[tt] + f32("position_rows")
    mean = x.mean(-1, keepdims=True, dtype=np.float32)
    var = (x * x).mean(-1, keepdims=True, dtype=np.float32) - mean * mean
    y = (x - mean) / np.sqrt(np.maximum(var, np.float32(0)) + np.float32(1e-12)) * f32("emb_ln_scale") + f32("emb_ln_B")
    err = ref64.rel_err(y.transpose(0, 2, 1).reshape(n, d, 1, l), ref)
    print(f"naive fp32 variance on the offset tables: max err / max|ref| {err:.3e}")
    assert err > RTOL["fp32"]


@pytest.mark.parametrize("kind", G.MASKED_KINDS)
@pytest.mark.parametrize("c", G.MASK_VALUES, ids=str)
def test_a_dropped_mask_is_far_outside_the_bound(kind, c):
    """float64: ignoring the mask moves every partly masked image by more than 30 x the fp16 bound"""
    n, l, h, hd = 2, 33, 3, 64
    _, idx = G.mask_requests(n, l)
    for r in idx:
        ref, bare = G.masked_reference(n, l, h, hd, kind, c, tuple(r)), G.masked_reference(n, l, h, hd, kind, c, tuple(r), masked=False)
        for i, row in enumerate(r):
            hidden = G.mask_rows(l)[row]
            if hidden.all() or not hidden.any():
                continue
            moved = float(np.abs(bare[i] - ref[i]).max() / np.abs(ref).max())
            assert moved > 30 * RTOL["fp16"], (kind, c, row, moved)


def test_fully_masked_rows_are_what_the_graph_gives():
    """float64: with c = min a fully masked image is the uniform average of V; with c = -10000 the unmasked softmax"""
    n, l, h, hd = 2, 33, 3, 64
    _, idx = G.mask_requests(n, l)
    (r,) = [r for r in idx if 6 in r]
    i = list(r).index(6)
    x = G.masked_input(n, l, h, hd, "randn", tuple(r)).astype(np.float64)[i, :, 0, :].T.reshape(l, 3, h, hd)
    uniform = x[:, 2].mean(0).reshape(h * hd)
    y = G.masked_reference(n, l, h, hd, "randn", "min", tuple(r))[i, :, 0, :]
    assert np.abs(y - uniform[:, None]).max() < 1e-12
    y = G.masked_reference(n, l, h, hd, "randn", -10000.0, tuple(r))[i]
    bare = G.masked_reference(n, l, h, hd, "randn", -10000.0, tuple(r), masked=False)[i]
    assert np.abs(y - bare).max() < 1e-9
