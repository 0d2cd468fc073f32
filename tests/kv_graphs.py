"""Test graphs of the KV cache (tests/test_kv_cache_plan.py, tests/test_kv_cache_gpu.py): the attention subgraph alone as a decode step and as a prefill
with `present` outputs, the narrow Llama of both tests, and mirrors of the planner's kernel choice and labels.  Importing llama_graphs registers what
ref64 needs beyond its own table (Neg and the RMSNorm operators; Concat, Gather, Unsqueeze, Cast and Expand are there already)."""
from __future__ import annotations

import numpy as np

import llama_graphs as LG  # noqa: F401  (registers the operators of a Llama graph in ref64.OPS)
from gpu_ai_inference_server_amd.modelgen import models

DECODE_TILE = 4                     # kernels.h kAttnDecodeTile
MAX_GROUP = 8                       # kernels.h kDecodeMaxGroup
MAX_SPLITS = 64                     # kernels.h kDecodeMaxSplits
MIN_SPLIT_KEYS = 128                # kernels.h kDecodeMinSplitKeys
MASK_SHIFT_MAX = 16777216.0         # kernels.h DecodeFastFits: a mask constant at or above -2^24 stays on tile 0


def key_tile(hd: int) -> int:
    """kernels.h DecodeKeyTile: the keys a workgroup of tile 4 loads per iteration"""
    return 1024 // hd


def fast_fits(hd: int, heads: int, kv_heads: int, masked: bool = False, mask_value: float = models.FLOAT32_MIN) -> bool:
    """kernels.h DecodeFastFits"""
    return hd in (32, 64, 128) and heads % kv_heads == 0 and heads // kv_heads <= MAX_GROUP and (not masked or mask_value < -MASK_SHIFT_MAX)


def default_splits(n: int, kv_heads: int, keys: int, hd: int) -> int:
    """kernels.h DecodeDefaultSplits"""
    groups = n * kv_heads
    tiles = -(-keys // key_tile(hd))
    return max(1, min(-(-512 // groups), keys // MIN_SPLIT_KEYS, tiles, MAX_SPLITS))


def decode_label(tile: int, f16: bool, hd: int, splits: int = 1) -> str:
    """launch.cpp kernel_label of a decode attention step"""
    t = "f16" if f16 else "f32"
    if tile == DECODE_TILE:
        return "attention_decode_kernel<%s,%d>" % (t, hd) + (" + attention_decode_combine_kernel" if splits > 1 else "")
    return "kv_append_kernel + attention_decode_generic_kernel<%s>" % t


def _picker(gb, c: int, offsets: dict):
    """llama_attention's `linear=` hook: the q / k / v "Linears" are identity matrices cut from the columns of the input rows (exact: products with 0 / 1)"""
    def pick(y, name, cout):
        w = np.zeros((c, cout), np.float32)
        o = offsets[name.rsplit("_", 2)[-2]]
        w[o:o + cout] = np.eye(cout, dtype=np.float32)
        return gb.simple("MatMul", [y, gb.init(name + "_w", w)])
    return pick


def decode_attn_graph(rows: np.ndarray, n: int, heads: int, kv_heads: int, hd: int, past: int, *, rope: str | None = "input", tables=None, max_pos: int = 64,
                      mask: bool = True, mask_value="min", lq: int = 1, past_k_dims=None, past_v_rows: int | None = None, extra_reader: bool = False, pos_dims=None,
                      k_positions: bool = False, mask_width: int | None = None, **kw) -> bytes:
    """One decode step of the attention alone.  input_ids [n, 1] pick q | k | v rows out of `rows` [R, (H + 2 Hkv) hd] (an embed step without a norm writes
    them as they are, as llama_graphs.gqa_attn_graph_one_token does: no feature map reshapes to one token), past_key_values.0.key / .value
    [n, Hkv, past, hd] are the cache.  rope "input": tables [max_pos, hd] gathered by position_ids [n, 1]; "const": the one row tables[past] as an
    Unsqueeze of an initializer; None: no rotation.  mask: attention_mask [n, past + 1] through BERT's chain.  Outputs: `out` [n, 1, D] (an identity
    Linear behind the attention makes it a token output of a Linear), present.0.key, present.0.value [n, Hkv, past + 1, hd].
    The rest are near misses the planner refuses: lq > 1 new tokens; past_k_dims / past_v_rows: other declared dims of the cache inputs; extra_reader: a
    second reader of the K cache; pos_dims: other dims of position_ids; k_positions: k rotated by another input's positions; mask_width: another mask
    width; and llama_attention's concat_order / present_after_repeat."""
    d, dkv = heads * hd, kv_heads * hd
    c = d + 2 * dkv
    gb = models.GraphBuilder("kvdec", 5)
    t = gb.simple("Gather", [gb.init("rows", np.ascontiguousarray(rows, np.float32)), "input_ids"], [models.pb.attr_int("axis", 0)])
    ext = models.bert_extended_mask(gb, mask_value=mask_value, unsqueeze="one") if mask else None
    ck = None
    if rope == "input":
        cs = models.rope_gathered(gb, hd, "rotary", max_pos=max_pos, tables=tables)
        ck = models.rope_gathered(gb, hd, "rotary_k", max_pos=max_pos, tables=tables, positions="position_ids_k") if k_positions else None
    elif rope == "const":
        full = tables if tables is not None else models.rope_tables(max_pos, hd)
        cs = models.rope_constants(gb, 1, hd, "rotary", form="unsqueeze", tables=(full[0][past:past + 1], full[1][past:past + 1]))
    else:
        cs = None
    if extra_reader:
        gb.simple("Identity", ["past_key_values.0.key"], out="leak")
    y = models.llama_attention(gb, t, lq, d, heads, kv_heads, "a", batch=n, rope=cs, rope_k=ck, mask=None, linear=_picker(gb, c, {"q": 0, "k": d, "v": d + dkv}), hd=hd,
                               past=("past_key_values.0.key", "past_key_values.0.value"), past_len=past, present=("present.0.key", "present.0.value"), key_mask=ext, **kw)
    gb.simple("MatMul", [y, gb.init("identity", np.eye(d, dtype=np.float32))], out="out")
    ins = [("input_ids", [n, lq], models.pb.INT64)] + ([("attention_mask", [n, mask_width or past + lq], models.pb.INT64)] if mask else []) + \
          ([("position_ids", pos_dims or [n, 1], models.pb.INT64)] if rope == "input" else []) + ([("position_ids_k", [n, 1], models.pb.INT64)] if ck else []) + \
          [("past_key_values.0.key", past_k_dims or [n, kv_heads, past, hd]), ("past_key_values.0.value", [n, kv_heads, past_v_rows or past, hd])]
    outs = [("out", [n, lq, d]), ("present.0.key", [n, kv_heads, past + lq, hd]), ("present.0.value", [n, kv_heads, past + lq, hd])] + \
           ([("leak", [n, kv_heads, past, hd])] if extra_reader else [])
    return gb.finish(ins, outs, opset=17)


def gpt2_decode_attn_graph(n: int, heads: int, hd: int, past: int) -> bytes:
    """GPT-2's merged-qkv spelling with a cache (a refusal: the follow-up): Split(axis 2) of one c_attn row into q, k, v, Concat(past, k / v, axis 2), no mask"""
    d = heads * hd
    gb = models.GraphBuilder("kvgpt2", 5)
    rows = np.random.RandomState(1).randn(7, 3 * d).astype(np.float32)
    t = gb.simple("Gather", [gb.init("rows", rows), "input_ids"], [models.pb.attr_int("axis", 0)])
    qkv = gb.simple("MatMul", [t, gb.init("c_attn_w", np.eye(3 * d, dtype=np.float32))])
    parts = [gb._uid("part") for _ in range(3)]
    gb.nodes.append(models.pb.node("Split", [qkv, gb.init("split", np.array([d, d, d], np.int64))], parts, "split_qkv", [models.pb.attr_int("axis", 2)]))
    shp = gb.init("shape4", np.array([0, -1, heads, hd], np.int64))
    q, k, v = (gb.transpose(gb.simple("Reshape", [p, shp]), (0, 2, 1, 3)) for p in parts)
    k = gb.simple("Concat", ["past_key_values.0.key", k], [models.pb.attr_int("axis", 2)], out="present.0.key")
    v = gb.simple("Concat", ["past_key_values.0.value", v], [models.pb.attr_int("axis", 2)], out="present.0.value")
    s = gb.simple("Div", [gb.simple("MatMul", [q, gb.transpose(k, (0, 1, 3, 2))]), gb.init("sqrt_hd", np.array(np.sqrt(float(hd)), np.float32))])
    y = gb.transpose(gb.simple("MatMul", [gb.simple("Softmax", [s], [models.pb.attr_int("axis", -1)]), v]), (0, 2, 1, 3))
    y = gb.simple("Reshape", [y, gb.init("shape3", np.array([0, -1, d], np.int64))])
    gb.simple("MatMul", [y, gb.init("identity", np.eye(d, dtype=np.float32))], out="out")
    cache = [n, heads, past, hd]
    return gb.finish([("input_ids", [n, 1], models.pb.INT64), ("past_key_values.0.key", cache), ("past_key_values.0.value", cache)],
                     [("out", [n, 1, d]), ("present.0.key", [n, heads, past + 1, hd]), ("present.0.value", [n, heads, past + 1, hd])], opset=17)


def decode_feeds(n: int, heads: int, kv_heads: int, hd: int, past: int, *, rows: int = 7, valid=None, positions=None, mask: bool = True, rope: str | None = "input",
                 seed: int = 0):
    """(rows, feeds) of decode_attn_graph: N(0, 1) rows and cache (every K / V head another draw, so a wrong head mapping shows); valid[i] = the valid
    cache rows of image i (default: all), the new key always valid; positions[i] = image i's position"""
    r = np.random.RandomState(100 * past + 10 * heads + kv_heads + seed)
    table = r.randn(rows, (heads + 2 * kv_heads) * hd).astype(np.float32)
    feeds = {"input_ids": r.randint(0, rows, (n, 1)).astype(np.int64)}
    if mask:
        m = np.ones((n, past + 1), np.int64)
        for i, v in enumerate(valid if valid is not None else [past] * n):
            m[i, v:past] = 0
        feeds["attention_mask"] = m
    if rope == "input":
        feeds["position_ids"] = np.asarray(positions if positions is not None else [past] * n, np.int64).reshape(n, 1)
    feeds["past_key_values.0.key"] = r.randn(n, kv_heads, past, hd).astype(np.float32)
    feeds["past_key_values.0.value"] = r.randn(n, kv_heads, past, hd).astype(np.float32)
    return table, feeds


def prefill_attn_graph(n: int, l: int, heads: int, kv_heads: int, hd: int, *, rope: str | None = "init", tables=None, present: bool = True, **kw) -> bytes:
    """llama_graphs.gqa_attn_graph (causal) with the outputs present.0.key / present.0.value [n, Hkv, l, hd] beside y; present False: the same graph
    without them"""
    d, dkv = heads * hd, kv_heads * hd
    c = d + 2 * dkv
    gb = models.GraphBuilder("gqa", 5)
    t = models.vit_tokens(gb, "x", c)
    cs = models.rope_constants(gb, l, hd, "rotary", form=rope, max_pos=l + 3, tables=tables) if rope else None
    y = models.llama_attention(gb, t, l, d, heads, kv_heads, "a", batch=n, rope=cs, mask="add", linear=_picker(gb, c, {"q": 0, "k": d, "v": d + dkv}), hd=hd,
                               present=("present.0.key", "present.0.value") if present else None, **kw)
    gb.simple("Reshape", [gb.transpose(y, (0, 2, 1)), gb.init("back_shape", np.array([0, d, 1, l], np.int64))], out="y")
    outs = [("y", [n, d, 1, l])] + ([("present.0.key", [n, kv_heads, l, hd]), ("present.0.value", [n, kv_heads, l, hd])] if present else [])
    return gb.finish([("x", [n, c, 1, l])], outs, opset=17)


# ---- the narrow Llama of both tests: depth 2, dim 128, 4 heads of 32 over 2 K / V heads, vocab 61, N = 2 --------------------------------------------------
NARROW = dict(vocab=61, dim=128, depth=2, heads=4, kv_heads=2, mlp=256, max_pos=64)
NARROW_N, NARROW_P = 2, 12


def narrow(batch: int = NARROW_N, **kw) -> bytes:
    return models.llama(batch, **dict(NARROW, **kw))


def present_names(depth: int = NARROW["depth"]):
    return [f"present.{i}.{w}" for i in range(depth) for w in ("key", "value")]


def cache_from(present: dict, lengths, capacity: int = NARROW_P, left: bool = False, dtype=np.float32) -> dict:
    """past_key_values.* feeds of capacity `capacity` from a prefill's present.* [N, Hkv, L, hd]: image i keeps its first lengths[i] rows, right-padded
    (valid rows first) or left-padded (valid rows last); the padding is NaN-free garbage a correct mask never lets through"""
    out = {}
    for name, p in present.items():
        n, hkv, _, hd = p.shape
        c = (np.random.RandomState(len(name)).randn(n, hkv, capacity, hd) * 3.0).astype(dtype)
        for i, ln in enumerate(lengths):
            if left:
                c[i, :, capacity - ln:] = p[i, :, :ln]
            else:
                c[i, :, :ln] = p[i, :, :ln]
        out[name.replace("present", "past_key_values")] = c
    return out


def cache_mask(lengths, capacity: int = NARROW_P, left: bool = False) -> np.ndarray:
    """attention_mask [N, capacity + 1] of cache_from's layout: the valid rows and the new key (the last column)"""
    m = np.zeros((len(lengths), capacity + 1), np.int64)
    m[:, capacity] = 1
    for i, ln in enumerate(lengths):
        if left:
            m[i, capacity - ln:capacity] = 1
        else:
            m[i, :ln] = 1
    return m
