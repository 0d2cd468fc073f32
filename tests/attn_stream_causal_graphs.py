"""What the tests know about the causal, rotary and grouped forms of attention tile 2 (attention_stream_kernel<T, HD, CAUSAL, ROPE>): the Profile label,
Python mirrors of kernels.h AttnCausalDefaultTile / kAttnStreamCausalMinTokens and of plan.cpp EmitAttention's choice, a float64 restatement of the
rotary grouped-query attention with one way of breaking the rotary wave slicing, the narrow Llama with heads of 128, and the graphs whose plans must be
the parent commit's."""
from __future__ import annotations

import numpy as np

import attn_wide_graphs as W
import llama_graphs as LG
import vit_graphs as G
from gpu_ai_inference_server_amd.modelgen import models

CAUSAL_MIN_TOKENS = 32                   # kernels.h kAttnStreamCausalMinTokens: a causal step's default is tile 2 from this many tokens on
ROPE_HEAD_DIMS = (128, 256)              # tile 2 rotates these; a rotary head of 512 keeps the generic kernel


def attn_label(tile: int, f16: bool, hd: int, causal: bool, rope: bool) -> str:
    """launch.cpp kernel_label of an attention step"""
    if tile != 2:
        return LG.attn_label(tile, f16, hd, causal, rope)
    return "attention_stream_kernel<%s,%d%s>" % ("f16" if f16 else "f32", hd, ",causal,rope" if rope else ",causal" if causal else "")


def stream_ok(l: int, hd: int, heads: int, kv_heads: int, f16: bool, causal: bool, rope: bool) -> bool:
    """plan.cpp EmitAttention fits(2) for the views of the test graphs (pitch = channels, offset 0)"""
    v = 8 if f16 else 4
    c_in, c_out = (heads + 2 * kv_heads) * hd, heads * hd
    if rope and (not causal or hd not in ROPE_HEAD_DIMS):
        return False
    return hd in W.WIDE_HEAD_DIMS and l >= 1 and c_in % v == 0 and c_out % v == 0


def default_tile(l: int, hd: int, heads: int, kv_heads: int, f16: bool, causal: bool = True, rope: bool = False) -> int:
    """plan.cpp EmitAttention without a pin: a causal step takes tile 1, else tile 3, else tile 2 from CAUSAL_MIN_TOKENS on; a non-causal one
    AttnDefaultTile (tile 2 from attn_wide_graphs.MIN_TOKENS on); non-causal rope is the generic kernel"""
    c_in, c_out = (heads + 2 * kv_heads) * hd, heads * hd
    if rope and not causal:
        return 0
    if LG.attn_mfma_ok(l, hd, c_in, c_out, f16):
        return 1
    if causal and LG.attn_chunk_ok(l, hd, c_in, c_out, f16):
        return 3
    return 2 if stream_ok(l, hd, heads, kv_heads, f16, causal, rope) and l >= (CAUSAL_MIN_TOKENS if causal else W.MIN_TOKENS) else 0


def rope_pair_elements(hd: int, wave: int) -> np.ndarray:
    """the head-dim elements wave `wave` of a rotary workgroup supplies to QK^T: the half-slices [w SL/2, (w + 1) SL/2) and hd/2 + the same, SL = hd/4"""
    hs = hd // 8
    return np.concatenate([np.arange(wave * hs, (wave + 1) * hs), hd // 2 + np.arange(wave * hs, (wave + 1) * hs)])


def gqa_attention_f64(x, heads: int, kv_heads: int, hd: int, *, tables=None, causal: bool = True, drop_pair: int | None = None) -> np.ndarray:
    """llama_graphs.gqa_attn_graph on x [N, (H + 2 Hkv) hd, 1, L] -> y [N, D, 1, L] from the definition, in float64.  tables: (cos, sin) [L, hd]
    (None: no rotation).  drop_pair: the scores without the products of that wave's rotary half-slice pair (a wave whose partial tile is lost)"""
    n, _, _, l = x.shape
    d, dkv = heads * hd, kv_heads * hd
    rows = np.asarray(x, np.float64)[:, :, 0, :].transpose(0, 2, 1)
    q = rows[..., :d].reshape(n, l, heads, hd).transpose(0, 2, 1, 3)
    k = rows[..., d:d + dkv].reshape(n, l, kv_heads, hd).transpose(0, 2, 1, 3)
    v = rows[..., d + dkv:].reshape(n, l, kv_heads, hd).transpose(0, 2, 1, 3)
    if tables is not None:
        cos, sin = (np.asarray(t, np.float64) for t in tables)
        rot = lambda t: t * cos + np.concatenate([-t[..., hd // 2:], t[..., : hd // 2]], axis=-1) * sin  # noqa: E731
        q, k = rot(q), rot(k)
    k, v = (np.repeat(t, heads // kv_heads, axis=1) for t in (k, v))
    if drop_pair is not None:
        keep = np.ones(hd, bool)
        keep[rope_pair_elements(hd, drop_pair)] = False
        q, k = q[..., keep], k[..., keep]
    s = np.einsum("nhle,nhme->nhlm", q, k) * float(np.float32(1.0 / np.sqrt(hd)))
    if causal:
        s = s + np.triu(np.full((l, l), -np.inf), 1)
    p = np.exp(s - s.max(-1, keepdims=True))
    o = np.einsum("nhlm,nhme->nhle", p / p.sum(-1, keepdims=True), v)
    return o.transpose(0, 1, 3, 2).reshape(n, d, 1, l)


def narrow_llama_hd128(batch=2, **kw) -> bytes:
    """depth 2, dim 256, 2 heads of 128 over 1 K / V head, mlp 512, vocab 61; logits and last_hidden_state"""
    return models.llama(batch, **dict(dict(seq=40, vocab=61, dim=256, depth=2, heads=2, kv_heads=1, mlp=512, max_pos=64, last_hidden_state=True), **kw))


def parent_plan_cases() -> dict:
    """name -> (builder thunk, batch) of the graphs whose plan and weight digests tests/golden/attn_stream_causal_parent_plans.json holds as a build
    of the parent commit gave them: no step of theirs is a causal, rotary or grouped wide head, so they plan exactly as they did"""
    cases = {"gpt2_tiny": (lambda: models.gpt2_tiny(2), 2), "llama_tiny": (lambda: models.llama_tiny(2, last_hidden_state=True), 2),
             "vit_tiny_16": (lambda: models.vit_tiny_16(2), 2), "bert_tiny": (lambda: models.bert_tiny(4), 4)}
    for n, l, h, hd in W.GPU_SHAPES:         # the plain wide heads: tile 2 from MIN_TOKENS on, the generic kernel below
        cases["attn_wide_%dx%dx%dx%d" % (n, l, h, hd)] = (lambda n=n, l=l, h=h, hd=hd: G.attn_graph(n, l, h, hd), n)
    return cases
