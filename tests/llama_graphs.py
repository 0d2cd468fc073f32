"""Test graphs shared by the Llama-class plan and GPU tests (RMSNorm, gated units), the kernel labels the tests expect, and the operators such a
graph needs from the float64 walk: importing this module registers ReduceMean, Sqrt, Reciprocal, Neg and RMSNormalization in ref64.OPS (Pow comes
with gpt2_graphs)."""
from __future__ import annotations

import numpy as np

import convnext_graphs as CG
import gpt2_graphs  # noqa: F401  (registers Pow)
import ref64
from gpu_ai_inference_server_amd.modelgen import models


def _reduce_mean(i, a, m):
    axes = [int(v) for v in (i[1] if len(i) > 1 and i[1] is not None else a.get("axes", range(i[0].ndim)))]
    return i[0].mean(axis=tuple(axes), keepdims=bool(a.get("keepdims", 1)))


def rms_norm(x, weight, axis: int = -1, eps: float = 1e-5) -> np.ndarray:
    """the ONNX RMSNormalization definition in float64: x / sqrt(mean(x^2 over the axes from `axis`) + eps) * weight"""
    x = np.asarray(x, np.float64)
    axes = tuple(range(axis % x.ndim, x.ndim))
    return x / np.sqrt((x * x).mean(axis=axes, keepdims=True) + eps) * np.asarray(weight, np.float64)


ref64.OPS["ReduceMean"] = _reduce_mean
ref64.OPS["Sqrt"] = lambda i, a, m: np.sqrt(i[0])
ref64.OPS["Reciprocal"] = lambda i, a, m: 1.0 / i[0]
ref64.OPS["Neg"] = lambda i, a, m: -i[0]
ref64.OPS["RMSNormalization"] = lambda i, a, m: rms_norm(i[0], i[1], a.get("axis", -1), float(np.float32(a.get("epsilon", 1e-5))))

RMS_FORMS = ("pow", "mul", "reciprocal", "mul_reciprocal", "op")


def rms_label(tile: int, f16: bool) -> str:
    """launch.cpp kernel_label of an RMSNorm step"""
    return "rmsnorm_generic_kernel" if tile == 0 else "rmsnorm_kernel<%s,%d>" % ("f16" if f16 else "f32", CG.LANES[tile])


def rms_graph(n: int, l: int, d: int, *, eps: float = 1e-5, form: str = "pow", tail: str | None = None, **kw) -> bytes:
    """x [n, d, 1, l] -> tokens [n, l, d] -> RMSNorm -> back to [n, d, 1, l] -> y.
    tail "add": y = RMSNorm(x) + x, so the norm is NOT the last reader of its input; None: it is, and its output may take its input's buffer"""
    gb = models.GraphBuilder("rms", 9)
    t = models.vit_tokens(gb, "x", d)
    y = gb.rmsnorm(t, d, eps=eps, form=form, name="rms", **kw)
    if tail == "add":
        y = gb.simple("Add", [y, t])
    gb.simple("Reshape", [gb.transpose(y, (0, 2, 1)), gb.init("back_shape", np.array([0, d, 1, l], np.int64))], out="y")
    return gb.finish([("x", [n, d, 1, l])], [("y", [n, d, 1, l])], opset=23 if form == "op" else 18)


def rms_cl_graph(n: int, c: int, h: int, w: int, **kw) -> bytes:
    """x [n, c, h, w] -> Transpose(0,2,3,1) -> RMSNorm -> Transpose(0,3,1,2) -> y: the norm on a channels-last view"""
    gb = models.GraphBuilder("rmscl", 9)
    y = gb.rmsnorm(gb.transpose("x", (0, 2, 3, 1)), c, name="rms", **kw)
    gb.nodes.append(models.pb.node("Transpose", [y], ["y"], "back", [models.pb.attr_ints("perm", [0, 3, 1, 2])]))
    return gb.finish([("x", [n, c, h, w])], [("y", [n, c, h, w])], opset=18)


def swiglu_graph(n: int, l: int, d: int, mlp: int, *, act: str = "silu", swap: bool = False) -> bytes:
    """x [n, d, 1, l] -> tokens -> down(act(gate(x)) * up(x)) (three Linears without a bias) -> back -> y: Llama's MLP"""
    gb = models.GraphBuilder("glu", 13)
    t = models.vit_tokens(gb, "x", d)
    h = gb.swiglu(gb.linear(t, d, mlp, name="gate", bias=False), gb.linear(t, d, mlp, name="up", bias=False), act=act, swap=swap)
    y = gb.linear(h, mlp, d, name="down", bias=False)
    gb.simple("Reshape", [gb.transpose(y, (0, 2, 1)), gb.init("back_shape", np.array([0, d, 1, l], np.int64))], out="y")
    return gb.finish([("x", [n, d, 1, l])], [("y", [n, d, 1, l])], opset=20 if act.startswith("op") else 17)


# ---- grouped-query attention with rotary positions -------------------------------------------------------------------------------------------------
KC = gpt2_graphs.KC                      # kernels.h kAttnChunkKeys
VG = gpt2_graphs.G                       # vit_graphs: LDS_BUDGET, attn_lds_bytes, make_input


def attn_mfma_ok(l: int, hd: int, c_in: int, c_out: int, f16: bool) -> bool:
    """kernels.h AttnMfmaFits with the grouped row width c_in = D + 2 Dkv (pitch = channels, offset 0)"""
    v = 8 if f16 else 4
    return hd in (32, 64) and l >= 1 and c_in % v == 0 and c_out % v == 0 and VG.attn_lds_bytes(l, hd, f16) <= VG.LDS_BUDGET


def attn_chunk_ok(l: int, hd: int, c_in: int, c_out: int, f16: bool) -> bool:
    """kernels.h AttnChunkFits likewise"""
    v = 8 if f16 else 4
    return hd in (32, 64) and l >= 1 and c_in % v == 0 and c_out % v == 0 and gpt2_graphs.attn_chunk_lds_bytes(hd, f16) <= VG.LDS_BUDGET


def rope_default_tile(l: int, hd: int, heads: int, kv_heads: int, f16: bool, causal: bool = True) -> int:
    """plan.cpp EmitAttention for a rotary step: AttnCausalDefaultTile on the grouped width; non-causal rope and other head dims: the generic kernel"""
    c_in, c_out = (heads + 2 * kv_heads) * hd, heads * hd
    if not causal:
        return 0
    if attn_mfma_ok(l, hd, c_in, c_out, f16):
        return 1
    return 3 if attn_chunk_ok(l, hd, c_in, c_out, f16) else 0


def attn_label(tile: int, f16: bool, hd: int, causal: bool, rope: bool) -> str:
    t = "f16" if f16 else "f32"
    if tile == 0:
        return "attention_generic_kernel<causal>" if causal else "attention_generic_kernel"
    stem = "attention_chunk_kernel" if tile == 3 else "attention_mfma_kernel"
    return "%s<%s,%d%s>" % (stem, t, hd, ",causal,rope" if rope else ",causal" if causal else "")


def random_tables(l: int, hd: int, seed: int = 3):
    """cos / sin tables of independent values in both halves of every row (no rope has them: a kernel that reads half a row shows)"""
    r = np.random.RandomState(seed)
    return r.uniform(-1.0, 1.0, (l, hd)).astype(np.float32), r.uniform(-1.0, 1.0, (l, hd)).astype(np.float32)


def gqa_attn_graph(n: int, l: int, heads: int, kv_heads: int, hd: int, *, rope: str | None = "init", tables=None, causal: bool = True, repeat: str = "auto",
                   rope_k_tables=None, **kw) -> bytes:
    """x [n, (H + 2 Hkv) hd, 1, l] -> tokens -> Llama's attention whose q / k / v "Linears" are identity matrices cut from the input's columns, so the
    kernel sees the raw input as q | k | v (exact: a product with 0 / 1) -> Transpose [0,2,1] -> Reshape [n, D, 1, l] -> y.  rope: rope_constants' form
    (None: no rotation); tables: (cos, sin) [l, hd] given; rope_k_tables: other tables for k (a refusal)"""
    d, dkv = heads * hd, kv_heads * hd
    c = d + 2 * dkv
    gb = models.GraphBuilder("gqa", 5)
    t = models.vit_tokens(gb, "x", c)
    off = {"q_proj": 0, "k_proj": d, "v_proj": d + dkv}

    def pick(y, name, cout):
        w = np.zeros((c, cout), np.float32)
        o = off[name.rsplit("_", 2)[-2] + "_proj"]
        w[o:o + cout] = np.eye(cout, dtype=np.float32)
        return gb.simple("MatMul", [y, gb.init(name + "_w", w)])
    cs = models.rope_constants(gb, l, hd, "rotary", form=rope, max_pos=l + 3, tables=tables) if rope else None
    ck = models.rope_constants(gb, l, hd, "rotary_k", form=rope, max_pos=l + 3, tables=rope_k_tables) if rope and rope_k_tables is not None else None
    y = models.llama_attention(gb, t, l, d, heads, kv_heads, "a", batch=n, rope=cs, rope_k=ck, repeat=repeat, mask="add" if causal else None, linear=pick, hd=hd, **kw)
    gb.simple("Reshape", [gb.transpose(y, (0, 2, 1)), gb.init("back_shape", np.array([0, d, 1, l], np.int64))], out="y")
    return gb.finish([("x", [n, c, 1, l])], [("y", [n, d, 1, l])], opset=17)


def gqa_input(n: int, l: int, heads: int, kv_heads: int, hd: int, seed: int = 0) -> np.ndarray:
    """N(0, 1) q | k | v rows; every K and V head is another draw, so a wrong head mapping shows"""
    return np.random.RandomState(1000 * l + 10 * heads + kv_heads + seed).randn(n, (heads + 2 * kv_heads) * hd, 1, l).astype(np.float32)


def narrow_llama(batch=2, **kw) -> bytes:
    """depth 2, dim 128, 2 heads of 64 over 1 K / V head, mlp 256, vocab 61; logits and last_hidden_state"""
    return models.llama(batch, **dict(dict(seq=40, vocab=61, dim=128, depth=2, heads=2, kv_heads=1, mlp=256, max_pos=64, last_hidden_state=True), **kw))


def gqa_attn_graph_one_token(rows: np.ndarray, n: int, heads: int, kv_heads: int, hd: int, *, tables=None) -> bytes:
    """L = 1, which no feature map reshapes to: input_ids [n, 1] pick q | k | v rows out of `rows` [R, (H + 2 Hkv) hd] (the embed step without a norm writes
    them as they are) -> gqa_attn_graph's attention with rope -> [n, 1, D], a token output under its own node's name (an identity Linear makes it one)"""
    d, dkv = heads * hd, kv_heads * hd
    c = d + 2 * dkv
    gb = models.GraphBuilder("gqa1", 5)
    t = gb.simple("Gather", [gb.init("rows", np.ascontiguousarray(rows, np.float32)), "input_ids"], [models.pb.attr_int("axis", 0)])
    off = {"q": 0, "k": d, "v": d + dkv}

    def pick(y, name, cout):
        w = np.zeros((c, cout), np.float32)
        o = off[name.rsplit("_", 2)[-2]]
        w[o:o + cout] = np.eye(cout, dtype=np.float32)
        return gb.simple("MatMul", [y, gb.init(name + "_w", w)])
    cs = models.rope_constants(gb, 1, hd, "rotary", form="unsqueeze", tables=tables)
    y = models.llama_attention(gb, t, 1, d, heads, kv_heads, "a", batch=n, rope=cs, linear=pick, hd=hd)
    y = gb.simple("MatMul", [y, gb.init("identity", np.eye(d, dtype=np.float32))])
    return gb.finish([("input_ids", [n, 1], models.pb.INT64)], [(y, [n, 1, d])], opset=17)
