"""Test graphs shared by the ViT plan and GPU tests, and what the tests know about the attention kernel's tiles."""
from __future__ import annotations

import functools

import numpy as np

from gpu_ai_inference_server_amd.modelgen import models
from gpu_ai_inference_server_amd.modelgen import onnx_pb as pb

UNBINDS = ("gather", "split")
SCALES = ("q", "s_mul", "s_div", "sdpa")
LDS_BUDGET = 160 * 1024


def attn_lds_bytes(l: int, hd: int, f16: bool) -> int:
    """K and V rows in LDS: L padded to whole 32-key tiles, every row padded by one 16-byte vector"""
    return 2 * ((l + 31) // 32 * 32) * (hd * (2 if f16 else 4) + 16)


def attn_mfma_ok(l: int, hd: int, d: int, f16: bool) -> bool:
    """tile 1 is eligible (the views of the test graphs have pitch = channels and offset 0)"""
    v = 8 if f16 else 4
    return hd in (32, 64) and d % v == 0 and attn_lds_bytes(l, hd, f16) <= LDS_BUDGET


def max_mfma_tokens(hd: int, f16: bool) -> int:
    """the largest L tile 1 takes"""
    l = 32
    while attn_lds_bytes(l + 32, hd, f16) <= LDS_BUDGET:
        l += 32
    return l


def attn_label(tile: int, f16: bool, hd: int) -> str:
    return "attention_generic_kernel" if tile == 0 else "attention_mfma_kernel<%s,%d>" % ("f16" if f16 else "f32", hd)


def narrow(batch=2, **kw) -> bytes:
    """a ViT of two layers on 64 channels and two heads over 32 x 32 images in 8 x 8 patches: L = 17, hd = 32"""
    kw = dict(dict(image=32, patch=8, dim=64, depth=2, heads=2, mlp=128, classes=10), **kw)
    return models.vit(batch, **kw)


def attn_graph(n: int, l: int, heads: int, hd: int, *, unbind: str = "gather", scale: str = "q", swap: bool = False, linear: bool = False) -> bytes:
    """x [n, 3 D, 1, l] -> Reshape [n, 3 D, l] -> Transpose [0,2,1] -> the attention pattern -> Transpose [0,2,1] -> Reshape [n, D, 1, l] -> y: the
    kernel sees the raw input as q | k | v.  linear: x [n, D, 1, l] and a Linear D -> 3 D makes the qkv rows"""
    d = heads * hd
    gb = models.GraphBuilder("attn", 5)
    t = models.vit_tokens(gb, "x", d if linear else 3 * d)
    y = models.vit_attention(gb, t, d, heads, "a", unbind=unbind, scale=scale, swap=swap, qkv=None if linear else t)
    y = gb.transpose(y, (0, 2, 1))
    gb.simple("Reshape", [y, gb.init("back_shape", np.array([0, d, 1, l], np.int64))], out="y")
    return gb.finish([("x", [n, d if linear else 3 * d, 1, l])], [("y", [n, d, 1, l])], opset=17)


def way_back_graph(n: int = 2) -> bytes:
    """tokens and back to a feature map: conv 4x4/s4 -> tokens [n, 16, 8] -> LayerNorm -> Transpose [0,2,1] -> Reshape [n, 8, 4, 4] -> conv 3x3"""
    gb = models.GraphBuilder("back", 6)
    t = gb.layernorm(models.vit_tokens(gb, gb.conv("x", 3, 8, 4, stride=4, bias=True, name="patch"), 8), 8, name="ln")
    y = gb.simple("Reshape", [gb.transpose(t, (0, 2, 1)), gb.init("map_shape", np.array([0, 8, 4, 4], np.int64))])
    gb.conv(y, 8, 8, 3, pad=1, bias=True, name="c3", out="y")
    return gb.finish([("x", [n, 3, 16, 16])], [("y", [n, 8, 4, 4])], opset=17)


def pack(q, k, v):
    """q, k, v [N, H, L, hd] -> x [N, 3 D, 1, L]: channel s * D + h * hd + e of token j is element e of head h of q / k / v"""
    n, h, l, hd = q.shape
    x = np.stack([q, k, v], 0).transpose(1, 0, 2, 4, 3).reshape(n, 3 * h * hd, 1, l)
    return np.ascontiguousarray(x, np.float32)


@functools.lru_cache(maxsize=None)
def make_input(n, l, h, hd, kind):
    st = np.random.RandomState(1000 * l + 10 * hd + h + len(kind))
    half = lambda a: a.astype(np.float16).astype(np.float32)  # noqa: E731
    v = half(st.randn(n, h, l, hd))
    if kind == "randn":
        q, k = st.randn(n, h, l, hd), st.randn(n, h, l, hd)
    elif kind == "peaked":
        k = st.randint(-2, 3, size=(n, h, l, hd)).astype(np.float64)
        q = 16.0 * k
    else:
        u = np.where(st.rand(n, h, 1, hd) < 0.5, -1.0, 1.0)
        step = 1.0 / 8.0 if kind == "ramp" else 1.0 / 128.0
        q = np.broadcast_to(u, (n, h, l, hd))
        k = u * (np.arange(l, dtype=np.float64) * step).reshape(1, 1, l, 1)
    x = pack(np.asarray(q, np.float32), np.asarray(k, np.float32), v)
    x.setflags(write=False)
    return x
