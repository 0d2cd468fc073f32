"""What the tests know about attention tile 2 (attention_stream_kernel: one wide head, K and V streamed in tiles of 32 keys, the head dim split over
the four waves of a workgroup), and float64 restatements of the attention with two ways of breaking that split."""
from __future__ import annotations

import numpy as np

import vit_graphs as G

MIN_TOKENS = 128                         # kernels.h kAttnStreamMinTokens: the planner's default is tile 2 from this many tokens on
WIDE_HEAD_DIMS = (128, 256, 512)
# (N, L, H, hd) of the GPU cases: fewer keys than a tile; exactly one tile and a second head's column offset; one key and one query into a second
# tile / second workgroup; a third query block with four accumulator blocks per wave; five key tiles at L >= MIN_TOKENS (the default is tile 2)
# and a batch stride; a tail tile of 16 keys
GPU_SHAPES = [(2, 5, 1, 128), (2, 32, 2, 128), (2, 33, 2, 256), (1, 65, 1, 512), (2, 160, 1, 512), (1, 144, 2, 256)]


def attn_stream_ok(l: int, hd: int, d: int, f16: bool, masked: bool = False) -> bool:
    """tile 2 is eligible (the views of the test graphs have pitch = channels and offset 0)"""
    return hd in WIDE_HEAD_DIMS and l >= 1 and not masked and d % (8 if f16 else 4) == 0


def attn_default_tile(l: int, hd: int, d: int, f16: bool, masked: bool = False) -> int:
    if not masked and G.attn_mfma_ok(l, hd, d, f16):
        return 1
    return 2 if attn_stream_ok(l, hd, d, f16, masked) and l >= MIN_TOKENS else 0


def attn_label(tile: int, f16: bool, hd: int) -> str:
    return "attention_stream_kernel<%s,%d>" % ("f16" if f16 else "f32", hd) if tile == 2 else G.attn_label(tile, f16, hd)


def unpack(x, h: int, hd: int):
    """x [N, 3 D, 1, L] (vit_graphs.pack) -> q, k, v [N, H, L, hd] in float64"""
    n, _, _, l = x.shape
    t = np.asarray(x, np.float64)[:, :, 0, :].transpose(0, 2, 1).reshape(n, l, 3, h, hd)
    return tuple(t[:, :, s].transpose(0, 2, 1, 3) for s in range(3))


def scores(q, k, drop_quarter: int | None = None):
    """scaled q k^T [N, H, L, L]; drop_quarter: without the products of that quarter of the head dim (a wave whose partial tile is lost)"""
    hd = q.shape[-1]
    if drop_quarter is not None:
        keep = np.ones(hd, bool)
        keep[drop_quarter * hd // 4:(drop_quarter + 1) * hd // 4] = False
        q, k = q[..., keep], k[..., keep]
    return np.einsum("nhle,nhme->nhlm", q, k) / np.sqrt(hd)


def attention_f64(x, h: int, hd: int, *, drop_quarter: int | None = None, swap_quarters: tuple[int, int] | None = None) -> np.ndarray:
    """the attention of vit_graphs.attn_graph on x -> y [N, D, 1, L]; swap_quarters: two head-dim quarters of every head's output trade places (a wave
    that stores to another wave's columns)"""
    q, k, v = unpack(x, h, hd)
    s = scores(q, k, drop_quarter)
    p = np.exp(s - s.max(-1, keepdims=True))
    o = np.einsum("nhlm,nhme->nhle", p / p.sum(-1, keepdims=True), v)
    if swap_quarters is not None:
        a, b = (slice(i * hd // 4, (i + 1) * hd // 4) for i in swap_quarters)
        o = o.copy()
        o[..., a], o[..., b] = o[..., b].copy(), o[..., a].copy()
    n, _, l, _ = o.shape
    return o.transpose(0, 1, 3, 2).reshape(n, h * hd, 1, l)
