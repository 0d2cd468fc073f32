"""Test graphs shared by the Swin plan and GPU tests, and what the tests know about the window-attention kernel's tiles."""
from __future__ import annotations

from gpu_ai_inference_server_amd.modelgen import models

UNBINDS = ("gather", "split")
SCALES = ("q", "s_mul", "s_div", "sdpa")
BLOCK = ["layer_norm", "conv", "window_attention", "conv", "layer_norm", "conv", "conv"]


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def wattn_mfma_ok(l: int, hd: int, d: int, f16: bool) -> bool:
    """tile 1 is eligible (the views of the test graphs have pitch = channels and offset 0)"""
    return hd == 32 and l <= 64 and d % (8 if f16 else 4) == 0


def wattn_label(tile: int, f16: bool, hd: int) -> str:
    return "window_attention_generic_kernel" if tile == 0 else "window_attention_mfma_kernel<%s,%d>" % ("f16" if f16 else "f32", hd)


def narrow(batch=2, **kw) -> bytes:
    """a Swin of two stages: 56 x 56 images, a 14 x 14 map on 32 channels and one head (a plain and a shifted block, four windows), then a 7 x 7 map on
    64 channels and two heads, where the window covers the map and the shift collapses"""
    kw = dict(dict(image=56, dims=(32, 64), depths=(2, 2), heads=(1, 2), window=7, classes=10), **kw)
    return models.swin(batch, **kw)


def collapsed_shift(hw, window, shift):
    """torchvision's rule: a dim's shift is 0 where the window is at least as large as the map in that dim"""
    return tuple(0 if w >= e else s for e, w, s in zip(hw, window, shift))


def wattn_graph(n: int, hw, window, shift, heads: int, hd: int, *, linear: bool = False, declared_hw=None, **kw) -> bytes:
    """x [n, 3 D, H, W] -> Transpose [0,2,3,1] -> the window region with no Linears -> Transpose [0,3,1,2] -> y [n, D, H, W]: the kernel sees the raw
    input as q | k | v.  linear: x [n, D, H, W], and the region's qkv and projection Linears are real (1x1 conv kernels write the qkv rows).  declared_hw: the extents the graph input declares, where they differ from what the region reshapes"""
    hw, window = _pair(hw), _pair(window)
    ihw = _pair(declared_hw) if declared_hw else hw
    shift = collapsed_shift(hw, window, _pair(shift))
    d = heads * hd
    gb = models.GraphBuilder("wattn", 9)
    t = gb.transpose("x", (0, 2, 3, 1))
    y = models.swin_window_attention(gb, t, d, heads, hw, window, shift, n, "w", linear=linear, **kw)
    gb.simple("Transpose", [y], [models.pb.attr_ints("perm", [0, 3, 1, 2])], out="y")
    return gb.finish([("x", [n, d if linear else 3 * d, ihw[0], ihw[1]])], [("y", [n, d, ihw[0], ihw[1]])], opset=17)


def merge_graph(n: int, c: int, hw) -> bytes:
    """x [n, c, H, W] -> Transpose [0,2,3,1] -> the eight Slices and the Concat of a patch merging -> Transpose [0,3,1,2] -> y [n, 4 c, H/2, W/2]"""
    hw = _pair(hw)
    gb = models.GraphBuilder("merge", 10)
    y = models.swin_patch_merge(gb, gb.transpose("x", (0, 2, 3, 1)), c, "m", reduce=False)
    gb.simple("Transpose", [y], [models.pb.attr_ints("perm", [0, 3, 1, 2])], out="y")
    return gb.finish([("x", [n, c, hw[0], hw[1]])], [("y", [n, 4 * c, hw[0] // 2, hw[1] // 2])], opset=17)
