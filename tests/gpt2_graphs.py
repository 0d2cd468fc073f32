"""Test graphs shared by the GPT-2 plan and GPU tests, what the tests know about the causal attention tiles (Python mirrors of kernels.h), and the
operators a GPT-2 graph needs from the float64 walk: importing this module registers Where and Pow in ref64.OPS (and lets Split cut equal parts when
the exporter left its sizes out)."""
from __future__ import annotations

import functools

import numpy as np

import bert_graphs as BG
import ref64
import vit_graphs as G
from engine_run import tensor, with_env
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models
from gpu_ai_inference_server_amd.modelgen import onnx_pb as pb


def _split(i, a, m, _sized=ref64.OPS["Split"]):
    if "split" in a or len(i) > 1:
        return _sized(i, a, m)
    return list(np.split(i[0], 3, axis=a.get("axis", 0)))        # (the test graphs' only Split without sizes has three outputs)


ref64.OPS["Where"] = lambda i, a, m: np.where(i[0] != 0, i[1], i[2])
ref64.OPS["Pow"] = lambda i, a, m: np.power(i[0], i[1])
ref64.OPS["Split"] = _split

KC = 256                               # kernels.h kAttnChunkKeys
LDS_BUDGET = G.LDS_BUDGET
MASKS = ("where_slice", "where_const", "add")


def attn_chunk_lds_bytes(hd: int, f16: bool) -> int:
    """kernels.h AttnChunkLdsBytes: one chunk of K and V rows, every row padded by one 16-byte vector"""
    return 2 * KC * (hd * (2 if f16 else 4) + 16)


def attn_chunk_ok(l: int, hd: int, d: int, f16: bool, masked: bool = False) -> bool:
    """kernels.h AttnChunkFits for the views of the test graphs (pitch = channels, offset 0)"""
    return hd in (32, 64) and l >= 1 and not masked and d % (8 if f16 else 4) == 0 and attn_chunk_lds_bytes(hd, f16) <= LDS_BUDGET


def causal_default_tile(l: int, hd: int, d: int, f16: bool) -> int:
    """kernels.h AttnCausalDefaultTile: tile 1 where it fits, else tile 3 where it fits, else the generic kernel"""
    if G.attn_mfma_ok(l, hd, d, f16):
        return 1
    return 3 if attn_chunk_ok(l, hd, d, f16) else 0


def attn_label(tile: int, f16: bool, hd: int, causal: bool) -> str:
    t = "f16" if f16 else "f32"
    if tile == 0:
        return "attention_generic_kernel<causal>" if causal else "attention_generic_kernel"
    stem = "attention_chunk_kernel" if tile == 3 else "attention_mfma_kernel"
    return "%s<%s,%d%s>" % (stem, t, hd, ",causal" if causal else "")


def embed_sum_label(tile: int, f16: bool) -> str:
    return "embed_sum_generic_kernel" if tile == 0 else "embed_sum_kernel<%s,%d>" % ("f16" if f16 else "f32", BG.LN_LANES[tile])


def causal_attn_graph(n: int, l: int, heads: int, hd: int, *, mask: str | None = "where_const", linear: bool = False, **kw) -> bytes:
    """x [n, 3 D, 1, l] -> tokens -> GPT-2's attention (Split, causal mask; mask None: the same graph without it) -> Transpose [0,2,1] -> Reshape
    [n, D, 1, l] -> y: the kernel sees the raw input as q | k | v.  linear: x [n, D, 1, l] and a real Linear D -> 3 D writes the qkv rows"""
    d = heads * hd
    gb = models.GraphBuilder("cattn", 5)
    t = models.vit_tokens(gb, "x", d if linear else 3 * d)
    if linear:
        t = gb.linear(t, d, 3 * d, name="c_attn")
    y = models.gpt2_attention(gb, t, l, d, heads, "a", mask=mask, max_pos=l + 3, **kw)
    gb.simple("Reshape", [gb.transpose(y, (0, 2, 1)), gb.init("back_shape", np.array([0, d, 1, l], np.int64))], out="y")
    return gb.finish([("x", [n, d if linear else 3 * d, 1, l])], [("y", [n, d, 1, l])], opset=17)


def causal_attn_graph_one_token(rows: np.ndarray, n: int, heads: int, hd: int, *, mask: str | None = "where_const") -> bytes:
    """L = 1, which no feature map reshapes to (a [N, C, 1, 1] value is no token view): input_ids [n, 1] pick qkv rows out of `rows` [R, 3 D] (the embed
    step without a norm writes them as they are: the position row is zero) -> GPT-2's attention -> [n, 1, D], a token output under its own node's name"""
    d = heads * hd
    gb = models.GraphBuilder("cattn1", 5)
    w = gb.simple("Gather", [gb.init("rows", np.ascontiguousarray(rows, np.float32)), "input_ids"], [pb.attr_int("axis", 0)])
    t = gb.simple("Add", [w, gb.init("no_position", np.zeros((1, 1, 3 * d), np.float32))])
    y = models.gpt2_attention(gb, t, 1, d, heads, "a", mask=mask, max_pos=4)
    y = gb.simple("MatMul", [y, gb.init("identity", np.eye(d, dtype=np.float32))])      # (exact; a Linear's result may be a token output, and an fp16 plan's attention writes halfs, as inside a model)
    return gb.finish([("input_ids", [n, 1], pb.INT64)], [(y, [n, 1, d])], opset=17)      # (ModelInfer pairs outputs by position, whatever their names)


@functools.lru_cache(maxsize=None)
def causal_reference(n, l, h, hd, kind, causal=True):
    """the float64 walk of causal_attn_graph on vit_graphs.make_input, computed once per input; read-only"""
    ref = ref64.run_f64(causal_attn_graph(n, l, h, hd, mask="where_const" if causal else None), {"x": G.make_input(n, l, h, hd, kind)})["y"]
    ref.setflags(write=False)
    return ref


def embed_sum_graph(n: int | str, l: int, vocab: int, d: int, *, pos: str = "gather", seed: int = 11) -> bytes:
    """input_ids [n, l] INT64 -> s = Gather(wte, ids) + positions, read by a LayerNormalization AND by the residual Add behind it (GPT-2's two readers).
    outputs: s itself ("sum", a token tensor [n, l, d]: it is read further, so it may be one) and LayerNormalization(s) + s, back as NCHW ("y" [n, d, 1, l])"""
    gb = models.GraphBuilder("esum", seed)
    table = lambda name, rows: gb.init(name, models.rng.gaussish(seed, name, rows * d).reshape(rows, d).astype(np.float32))  # noqa: E731
    w = gb.simple("Gather", [table("wte", vocab), "input_ids"], [pb.attr_int("axis", 0)])
    if pos == "gather":
        i64 = lambda name, v: gb.init(name, np.array(v, np.int64))  # noqa: E731
        pid = gb.simple("Slice", [gb.init("position_ids", np.arange(l + 3, dtype=np.int64).reshape(1, l + 3)), i64("ps", [0]), i64("pe", [l]), i64("pa", [1]), i64("pt", [1])])
        p = gb.simple("Gather", [table("wpe", l + 3), pid], [pb.attr_int("axis", 0)])
    else:
        p = gb.init("position_rows", models.rng.gaussish(seed, "wpe", l * d).reshape(1, l, d).astype(np.float32))
    s = gb.simple("Add", [w, p], out="sum")
    y = gb.simple("Add", [gb.layernorm(s, d, eps=1e-5, name="ln_1"), s])
    gb.simple("Reshape", [gb.transpose(y, (0, 2, 1)), gb.init("back_shape", np.array([0, d, 1, l], np.int64))], out="y")
    return gb.finish([("input_ids", [n, l], pb.INT64)], [("sum", [n, l, d]), ("y", [n, d, 1, l])], opset=17)


def narrow_gpt2(batch=2, **kw) -> bytes:
    """depth 2, dim 128, 2 heads of 64, seq 40, vocab 61; logits and last_hidden_state"""
    return models.gpt2(batch, **dict(dict(seq=40, vocab=61, dim=128, depth=2, heads=2, mlp=256, max_pos=64, last_hidden_state=True), **kw))


def gpt2_ids(n: int, l: int, vocab: int) -> np.ndarray:
    ids = np.random.RandomState(100 * l + vocab).randint(0, vocab, size=(n, l)).astype(np.int64)
    ids.ravel()[:3] = [0, vocab - 1, 0]
    return ids


def run_outputs(path, name, env, feeds, outs):
    """A model of its own under IE_AUTOTUNE=0 plus env, one request for several outputs at once.  outs: {output name: shape} ->
    ({name: array}, {name: the shape ModelInfer wrote back}, the launched kernels in plan order)"""
    def go():
        m = B.CreateModel(path, name)
        try:
            r = m.Infer([tensor(k, v) for k, v in feeds.items()], [B.OutputConfig(k, Shape=list(s), DataType="FLOAT32") for k, s in outs.items()])
            ys = {t.Name: t.Data.reshape(outs[t.Name]).copy() for t in r}
            shapes = {t.Name: list(t.Shape.Dims) for t in r}
            return ys, shapes, [p["kernel"] for p in B.Profile(m, 1)]
        finally:
            m.Destroy()
    return with_env(dict(IE_AUTOTUNE="0", **env), go)

