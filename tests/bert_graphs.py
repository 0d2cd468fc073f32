"""Test graphs shared by the BERT plan and GPU tests, and what the tests know about the embed kernel's tiles."""
from __future__ import annotations

import functools

import numpy as np

import ref64
from gpu_ai_inference_server_amd.modelgen import models
from gpu_ai_inference_server_amd.modelgen import onnx_pb as pb

LN_LANES = (0, 8, 16, 32, 64)          # kernels.h kLnLanes: the embed kernel's lane groups are the layer-norm kernel's
LN_MAX_VECTORS = 6


def embed_tile_fits(d: int, f16: bool, tile: int) -> bool:
    """kernels.h EmbedTileFits for the views of the test graphs (pitch = D, offset 0)"""
    v = 8 if f16 else 4
    return 1 <= tile < len(LN_LANES) and d % v == 0 and d // v <= LN_LANES[tile] * LN_MAX_VECTORS


def embed_default_tile(d: int, f16: bool) -> int:
    """kernels.h EmbedDefaultTile: the smallest lane group that holds the row in three vectors per lane, else the smallest that holds it, else 0"""
    v = 8 if f16 else 4
    for t in range(1, len(LN_LANES)):
        if embed_tile_fits(d, f16, t) and d // v <= 3 * LN_LANES[t]:
            return t
    for t in range(1, len(LN_LANES)):
        if embed_tile_fits(d, f16, t):
            return t
    return 0


def embed_label(tile: int, f16: bool) -> str:
    return "embed_ln_generic_kernel" if tile == 0 else "embed_ln_kernel<%s,%d>" % ("f16" if f16 else "f32", LN_LANES[tile])


def embed_graph(n: int | str, l: int, vocab: int, d: int, *, types: int = 2, pos: str | None = "const", order: str = "wtp", table_mean: float = 0.0,
                max_pos: int | None = None, seed: int = 11) -> bytes:
    """input_ids (, token_type_ids) [n, l] INT64 -> the embedding sum -> LayerNormalization -> Transpose [0,2,1] -> Reshape [n, d, 1, l] -> y: every
    token row of the embed step reaches the output"""
    gb = models.GraphBuilder("embed", seed)
    t = models.bert_embeddings(gb, l, vocab, d, types=types, max_pos=max_pos or l + 3, pos=pos, order=order, table_mean=table_mean, eps=1e-12)
    gb.simple("Reshape", [gb.transpose(t, (0, 2, 1)), gb.init("back_shape", np.array([0, d, 1, l], np.int64))], out="y")
    ins = [("input_ids", [n, l], pb.INT64)] + ([("token_type_ids", [n, l], pb.INT64)] if types else [])
    return gb.finish(ins, [("y", [n, d, 1, l])], opset=17)


# ---- the key-masked attention ----------------------------------------------------------------------------------------------------------------
LDS_BUDGET = 160 * 1024


def masked_attn_lds_bytes(l: int, hd: int, f16: bool) -> int:
    """kernels.h AttnLdsBytes with the mask: K and V rows (L padded to 32-key tiles, every row padded by 16 bytes) and one fp32 bias per padded key"""
    lp = (l + 31) // 32 * 32
    return 2 * lp * (hd * (2 if f16 else 4) + 16) + 4 * lp


def masked_attn_mfma_ok(l: int, hd: int, d: int, f16: bool) -> bool:
    v = 8 if f16 else 4
    return hd in (32, 64) and d % v == 0 and masked_attn_lds_bytes(l, hd, f16) <= LDS_BUDGET


def max_masked_mfma_tokens(hd: int, f16: bool) -> int:
    l = 32
    while masked_attn_lds_bytes(l + 32, hd, f16) <= LDS_BUDGET:
        l += 32
    return l


def masked_attn_label(tile: int, f16: bool, hd: int) -> str:
    return "attention_generic_kernel<mask>" if tile == 0 else "attention_mfma_kernel<%s,%d,mask>" % ("f16" if f16 else "f32", hd)


def masked_attn_graph(n: int, l: int, heads: int, hd: int, *, mask_value="min", **kw) -> bytes:
    """x [n, 3 D, 1, l] (q | k | v) -> tokens -> BERT's attention with the key mask of attention_mask [n, l] -> Transpose [0,2,1] -> Reshape [n, D, 1, l] -> y.
    The q / k / v Linears SELECT their third of the row (0 / 1 weights, zero bias: exact in fp32 and fp16), so the kernel sees the raw input as q | k | v
    and the planner's merge of the three Linears is part of what runs."""
    d = heads * hd
    gb = models.GraphBuilder("mattn", 5)
    t = models.vit_tokens(gb, "x", 3 * d)

    def select(y, name):
        s = ("query", "key", "value").index(name.rsplit("_", 1)[1])
        w = np.zeros((3 * d, d), np.float32)
        w[s * d + np.arange(d), np.arange(d)] = 1.0
        mm = gb.simple("MatMul", [y, gb.init(name + "_w", w)])
        return gb.simple("Add", [mm, gb.init(name + "_b", np.zeros(d, np.float32))])

    ext = models.bert_extended_mask(gb, mask_value=mask_value, unsqueeze=kw.pop("unsqueeze", "two"))
    y = models.bert_attention(gb, t, ext, d, heads, "a", linear=select, **kw)
    gb.simple("Reshape", [gb.transpose(y, (0, 2, 1)), gb.init("back_shape", np.array([0, d, 1, l], np.int64))], out="y")
    return gb.finish([("x", [n, 3 * d, 1, l]), ("attention_mask", [n, l], pb.INT64)], [("y", [n, d, 1, l])], opset=17)


def narrow_bert(batch=3, **kw) -> bytes:
    """dim 64, 2 heads of 32, 2 layers, seq 40, vocab 50; logits and pooler_output"""
    return models.bert(batch, **dict(dict(seq=40, vocab=50, dim=64, depth=2, heads=2, mlp=128, max_pos=64, pooler_output=True), **kw))


@functools.lru_cache(maxsize=None)
def narrow_feeds():
    """three rows of ids / mask / types for narrow_bert (lengths 40 / 17 / 1); shared, read-only by convention"""
    st = np.random.RandomState(7)
    ids = st.randint(0, 50, size=(3, 40)).astype(np.int64)
    tt = (st.rand(3, 40) < 0.5).astype(np.int64)
    mask = np.zeros((3, 40), np.int64)
    for n, ln in enumerate((40, 17, 1)):
        mask[n, :ln] = 1
    return {"input_ids": ids, "attention_mask": mask, "token_type_ids": tt}


# ---- data of the embed and key-masked attention tests, with their float64 references (computed once, read-only) ----------------------------------
TABLE_MEANS = {"randn": 0.0, "offset": 100.0}
MASKED_KINDS = ("randn", "peaked")
MASK_VALUES = ("min", -10000.0)


def make_ids(n, l, v, types=2):
    """ids with 0, V - 1, -1, -V and a repeat; type ids that use both rows"""
    st = np.random.RandomState(100 * l + v)
    ids = st.randint(0, v, size=(n, l)).astype(np.int64)
    special = [0, v - 1, -1, -v, v - 1]
    ids.ravel()[:min(len(special), ids.size)] = special[:ids.size]
    tt = (np.arange(n * l).reshape(n, l) % max(types, 1)).astype(np.int64)
    return ids, tt


def embed_feeds(ids, tt, types):
    return {"input_ids": ids, **({"token_type_ids": tt} if types else {})}


@functools.lru_cache(maxsize=None)
def embed_graph_and_reference(n, l, v, d, kind, types, pos):
    mb = embed_graph(n, l, v, d, types=types, pos=pos, table_mean=TABLE_MEANS[kind])
    ids, tt = make_ids(n, l, v, types)
    ref = ref64.run_f64(mb, embed_feeds(ids, tt, types))["y"]
    ref.setflags(write=False)
    return mb, ref


def mask_rows(l):
    """the eight mask rows of the test, [8, l]"""
    rows = []
    for ln in (1, 31, 32, 33, l):
        r = np.zeros(l, np.int64)
        r[:min(ln, l)] = 1
        rows.append(r)
    hole = np.ones(l, np.int64)
    hole[l // 3: max(l // 3 + 1, 2 * l // 3)] = 0
    return np.stack(rows + [hole, np.zeros(l, np.int64), np.ones(l, np.int64)])


def mask_requests(n, l):
    """the mask rows dealt over mask_requests of n images: [mask_requests, n, l], and per request the index of each image's mask row"""
    rows = mask_rows(l)
    idx = np.arange(8).reshape(8 // n, n)
    return rows[idx], idx


@functools.lru_cache(maxsize=None)
def masked_input(n, l, h, hd, kind, row):
    """x [n, 3 D, 1, l] for the images whose mask rows are `row` (a tuple): hidden keys are multiples of the all-ones vector"""
    st = np.random.RandomState(1000 * l + 10 * hd + h + len(kind))
    half = lambda a: a.astype(np.float16).astype(np.float32)  # noqa: E731
    v = half(st.randn(n, h, l, hd))
    if kind == "randn":
        q, k, big = half(st.randn(n, h, l, hd) + 0.5), half(st.randn(n, h, l, hd)), 2.0
    else:
        k = st.randint(-2, 3, size=(n, h, l, hd)).astype(np.float32)
        q, big = 16.0 * k + 16.0, 4.0
    rows = mask_rows(l)
    for i, r in enumerate(row):
        if rows[r].any():                              # (a fully masked image keeps its keys: nothing is hidden from anything)
            k[i][:, rows[r] == 0, :] = big
    x = np.stack([q, k, v], 0).transpose(1, 0, 2, 4, 3).reshape(n, 3 * h * hd, 1, l)
    x = np.ascontiguousarray(x, np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def masked_reference(n, l, h, hd, kind, c, row, masked=True):
    m = mask_rows(l)[list(row)] if masked else np.ones((n, l), np.int64)
    ref = ref64.run_f64(masked_attn_graph(n, l, h, hd, mask_value=c), {"x": masked_input(n, l, h, hd, kind, row), "attention_mask": m})["y"]
    ref.setflags(write=False)
    return ref
