"""Test graphs of an extend step (tests/test_extend_plan.py, tests/test_extend_gpu.py): an attention step with a past of P rows and Lq >= 2 new tokens
(chunked prefill into a cache).  The attention subgraph alone like kv_graphs.decode_attn_graph, but with the chunk mask M = Where(Cast(ext, to BOOL),
finfo.min, C) and position_ids [N, Lq]; its feeds; mirrors of the planner's kernel choice and labels.  Importing gpt2_graphs registers Where in
ref64.OPS, llama_graphs what a Llama graph needs."""
from __future__ import annotations

import numpy as np

import gpt2_graphs as GG  # noqa: F401  (registers Where in ref64.OPS)
import kv_graphs as KG
import llama_graphs as LG  # noqa: F401
from gpu_ai_inference_server_amd.modelgen import models

EXTEND_TILE = 5                     # kernels.h kAttnExtendTile
MIN_ROWS = 2                        # kernels.h kAttnExtendMinRows: tile 5 is the default from this many query rows g * Lq on


def fast_fits(hd: int, heads: int, kv_heads: int, mask_value: float = models.FLOAT32_MIN) -> bool:
    """kernels.h ExtendFastFits (an extend step always has its mask)"""
    return hd in (32, 64) and KG.fast_fits(hd, heads, kv_heads, True, mask_value)


def default_splits(n: int, kv_heads: int, rows: int, keys: int) -> int:
    """kernels.h ExtendDefaultSplits: rows = g * Lq query rows per K / V head, keys = P + Lq"""
    groups = n * kv_heads * -(-rows // 128)
    return max(1, min(-(-256 // groups), keys // KG.MIN_SPLIT_KEYS, -(-keys // 32), KG.MAX_SPLITS))


def extend_label(tile: int, f16: bool, hd: int, splits: int = 1) -> str:
    """launch.cpp kernel_label of an extend step"""
    t = "f16" if f16 else "f32"
    if tile == EXTEND_TILE:
        return "kv_append_kernel + attention_extend_kernel<%s,%d>" % (t, hd) + (" + attention_extend_combine_kernel" if splits > 1 else "")
    return "kv_append_kernel + attention_extend_generic_kernel<%s>" % t


def extend_attn_graph(rows: np.ndarray, n: int, heads: int, kv_heads: int, hd: int, past: int, lq: int, *, rope: str | None = "input", tables=None, max_pos: int = 64,
                      mask: str | None = "where", fill: float = models.FLOAT32_MIN, mask_value="min", c_past: int | None = None, c_edit=None, mask_width: int | None = None,
                      pos_dims=None, with_past: bool = True) -> bytes:
    """One extend step of the attention alone.  input_ids [n, lq] pick q | k | v rows out of `rows` [R, (H + 2 Hkv) hd], past_key_values.0.key / .value
    [n, Hkv, past, hd] are the cache, attention_mask [n, past + lq] and position_ids [n, lq] the other inputs.  Outputs: `out` [n, lq, D],
    present.0.key / .value [n, Hkv, past + lq, hd].  mask "where": the chunk mask of models.chunk_causal_mask on the scores.
    The rest are near misses the planner refuses: mask "add" (Add(ext, C)), "key" (the key mask alone) and None; fill: another value of a masked key;
    c_past: C built for another number of cached rows (a wrong width); c_edit (i, j, value): one element of C overwritten (a wrong triangle);
    mask_width / pos_dims: other dims of attention_mask / position_ids; with_past False: the same mask on a plain prefill (no cache inputs)"""
    d, dkv = heads * hd, kv_heads * hd
    c = d + 2 * dkv
    gb = models.GraphBuilder("kvext", 5)
    t = gb.simple("Gather", [gb.init("rows", np.ascontiguousarray(rows, np.float32)), "input_ids"], [models.pb.attr_int("axis", 0)])
    p_eff = past if with_past else 0
    key_mask = None
    if mask is not None:
        ext = models.bert_extended_mask(gb, mask_value=mask_value, unsqueeze="one")
        key_mask = ext if mask == "key" else models.chunk_causal_mask(gb, ext, lq, p_eff if c_past is None else c_past, "chunk", form=mask, fill=fill, edit=c_edit)
    cs = models.rope_gathered(gb, hd, "rotary", max_pos=max_pos, tables=tables) if rope == "input" else None
    kv = dict(past=("past_key_values.0.key", "past_key_values.0.value"), past_len=past, present=("present.0.key", "present.0.value")) if with_past else {}
    y = models.llama_attention(gb, t, lq, d, heads, kv_heads, "a", batch=n, rope=cs, mask=None, linear=KG._picker(gb, c, {"q": 0, "k": d, "v": d + dkv}), hd=hd, key_mask=key_mask, **kv)
    gb.simple("MatMul", [y, gb.init("identity", np.eye(d, dtype=np.float32))], out="out")
    ins = [("input_ids", [n, lq], models.pb.INT64)] + ([("attention_mask", [n, mask_width or p_eff + lq], models.pb.INT64)] if mask is not None else []) + \
          ([("position_ids", pos_dims or [n, lq], models.pb.INT64)] if cs else [])
    outs = [("out", [n, lq, d])]
    if with_past:
        ins += [("past_key_values.0.key", [n, kv_heads, past, hd]), ("past_key_values.0.value", [n, kv_heads, past, hd])]
        outs += [("present.0.key", [n, kv_heads, past + lq, hd]), ("present.0.value", [n, kv_heads, past + lq, hd])]
    return gb.finish(ins, outs, opset=17)


def chunk_mask(valid, chunk_valid, past: int, lq: int, left: bool = False) -> np.ndarray:
    """attention_mask [N, past + lq]: image i has valid[i] valid cache rows (the first ones, or with `left` the last ones) and its first chunk_valid[i]
    new tokens (a ragged chunk is padded on the right, the padded tokens' own columns 0)"""
    m = np.zeros((len(valid), past + lq), np.int64)
    for i, (v, cv) in enumerate(zip(valid, chunk_valid)):
        if left:
            m[i, past - v:past] = 1
        else:
            m[i, :v] = 1
        m[i, past:past + cv] = 1
    return m


def extend_feeds(n: int, heads: int, kv_heads: int, hd: int, past: int, lq: int, *, rows: int = 7, valid=None, chunk_valid=None, positions=None, left: bool = False,
                 rope: str | None = "input", max_pos: int = 64, seed: int = 0):
    """(rows, feeds) of extend_attn_graph: N(0, 1) rows and cache (every K / V head and cache row another draw).  positions [n, lq]; the default differs per
    image and runs BACKWARDS inside the chunk (token l of image i sits at table row valid[i] + lq - 1 - l), so a kernel that adds l to one position fails"""
    r = np.random.RandomState(1000 * lq + 100 * past + 10 * heads + kv_heads + seed)
    table = r.randn(rows, (heads + 2 * kv_heads) * hd).astype(np.float32)
    valid = [past if v is None else min(v, past) for v in (valid if valid is not None else [None] * n)]
    chunk_valid = list(chunk_valid) if chunk_valid is not None else [lq] * n
    feeds = {"input_ids": r.randint(0, rows, (n, lq)).astype(np.int64), "attention_mask": chunk_mask(valid, chunk_valid, past, lq, left)}
    if rope == "input":
        if positions is None:
            positions = [[(v + lq - 1 - l) % max_pos for l in range(lq)] for v in valid]
        feeds["position_ids"] = np.asarray(positions, np.int64).reshape(n, lq)
    feeds["past_key_values.0.key"] = r.randn(n, kv_heads, past, hd).astype(np.float32)
    feeds["past_key_values.0.value"] = r.randn(n, kv_heads, past, hd).astype(np.float32)
    return table, feeds


def own_key_valid(feeds, past: int) -> np.ndarray:
    """[N, Lq] bool: the new tokens whose own key is valid (the rows of `out` a client reads; the rest are finite and otherwise unspecified)"""
    return feeds["attention_mask"][:, past:] != 0
