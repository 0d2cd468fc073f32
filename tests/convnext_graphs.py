"""Test graphs shared by the ConvNeXt plan and GPU tests, and what the tests know about the layer-norm kernel's tiles."""
from __future__ import annotations

from gpu_ai_inference_server_amd.modelgen import models
from gpu_ai_inference_server_amd.modelgen import onnx_pb as pb

LANES = (0, 8, 16, 32, 64)               # lanes per pixel row of layer-norm tiles 0-4 (0: the generic kernel, a wave per row)
MAX_VECTORS = 6                          # 16-byte vectors (4 floats / 8 halfs) a lane of tiles 1-4 holds at most


def ln_tile_fits(c: int, f16: bool, tile: int) -> bool:
    v = 8 if f16 else 4
    return 1 <= tile <= 4 and c % v == 0 and c // v <= LANES[tile] * MAX_VECTORS


def ln_default_tile(c: int, f16: bool) -> int:
    """the smallest lane group that holds the row in at most three vectors per lane, else the smallest that holds it at all, else generic"""
    v = 8 if f16 else 4
    for t in (1, 2, 3, 4):
        if ln_tile_fits(c, f16, t) and c // v <= 3 * LANES[t]:
            return t
    for t in (1, 2, 3, 4):
        if ln_tile_fits(c, f16, t):
            return t
    return 0


def ln_label(tile: int, f16: bool) -> str:
    return "layernorm_generic_kernel" if tile == 0 else "layernorm_kernel<%s,%d>" % ("f16" if f16 else "f32", LANES[tile])


def narrow(batch=2, **kw) -> bytes:
    """a ConvNeXt of five blocks on 16 / 32 / 64 / 128 channels over 64 x 64 images"""
    return models.convnext(batch, depths=(1, 1, 2, 1), dims=(16, 32, 64, 128), image=64, **kw)


def ln_graph(n, c, h, w, eps=1e-6, axis=-1) -> bytes:
    """x [n, c, h, w] -> Transpose(0,2,3,1) -> LayerNormalization "ln" -> Transpose(0,3,1,2) -> y"""
    gb = models.GraphBuilder("ln", 9)
    y = gb.layernorm(gb.transpose("x", (0, 2, 3, 1)), c, eps=eps, axis=axis, name="ln")
    gb.nodes.append(pb.node("Transpose", [y], ["y"], "back", [pb.attr_ints("perm", [0, 3, 1, 2])]))
    return gb.finish([("x", [n, c, h, w])], [("y", [n, c, h, w])], opset=17)


def ln_concat_graph(n, c, h, w, eps=1e-6) -> bytes:
    """a = Conv1x1(x [n, 4, h, w]) -> y = Concat(a, layer norm of a): the norm reads channels [0, c) of the concat's pixel rows and writes [c, 2c)"""
    gb = models.GraphBuilder("lncat", 9)
    a = gb.conv("x", 4, c, 1, bias=True, name="pre")
    b = gb.transpose(gb.layernorm(gb.transpose(a, (0, 2, 3, 1)), c, eps=eps, name="ln"), (0, 3, 1, 2))
    gb.nodes.append(pb.node("Concat", [a, b], ["y"], "cat", [pb.attr_int("axis", 1)]))
    return gb.finish([("x", [n, 4, h, w])], [("y", [n, 2 * c, h, w])], opset=17)
