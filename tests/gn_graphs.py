"""Test graphs and data shared by the GroupNorm plan and GPU tests, what the tests know about the group-norm kernels' tiles, and a torch float64
restatement of the VAE decoder that reads the weights of models.vae_decoder's graph by name."""
from __future__ import annotations

import numpy as np

from gpu_ai_inference_server_amd.modelgen import models
from gpu_ai_inference_server_amd.modelgen import onnx_pb as pb
from oracle import onnx_oracle as O

OPSET = {"instancenorm": 17, "instance": 17, "op18": 18, "op21": 21}
BLOCK = 256                              # threads of a tile-1 workgroup: a lane keeps one 16-byte channel vector, so C / V <= BLOCK
MAX_SLABS = 256
WANT_BLOCKS = 2048
TILE1_MIN_GROUP_ELEMS = 2048             # the planner's default: tile 1 from this many elements per (image, group) on


def gn_tile_fits(c: int, groups: int, f16: bool, act: str | None = None) -> bool:
    """tile 1: whole 16-byte vectors (of the output type), one per lane, a vector inside one group or made of whole groups"""
    v = 8 if f16 else 4
    cpg = c // groups
    return c % v == 0 and c // v <= BLOCK and (cpg % v == 0 or v % cpg == 0) and act in (None, "silu", "relu", "sigmoid")


def gn_default_tile(c: int, groups: int, hw: int, f16: bool, act: str | None = None) -> int:
    return 1 if gn_tile_fits(c, groups, f16, act) and hw * (c // groups) >= TILE1_MIN_GROUP_ELEMS else 0


def gn_slabs(n: int, hw: int, c: int, f16: bool) -> tuple[int, int]:
    """(pixels per slab, slabs per image) of tile 1: at least about 64 KiB per slab, whole iterations of the workgroup, at most MAX_SLABS slabs per
    image and about WANT_BLOCKS workgroups in all"""
    v, es = (8, 2) if f16 else (4, 4)
    rows = BLOCK // (c // v)
    px = 65536 // (c * es)
    want = max(1, min(MAX_SLABS, WANT_BLOCKS // n))
    if px * want < hw:
        px = -(-hw // want)
    px = max(1, -(-px // rows) * rows)
    return px, -(-hw // px)


def gn_label(tile: int, f16: bool, act: str | None = None) -> str:
    t = "f16" if f16 else "f32"
    return "groupnorm_generic_kernel" if tile == 0 else f"groupnorm_stats_kernel<{t}> + groupnorm_apply_kernel<{t},{act or 'none'}>"


def _act(gb, y: str, act: str | None, out: str, swap: bool = False) -> None:
    if act is None:
        gb.simple("Identity", [y], out=out)
    elif act == "silu":
        g = gb.sigmoid(y)
        gb.simple("Mul", [g, y] if swap else [y, g], out=out)
    elif act == "relu":
        gb.simple("Relu", [y], out=out)
    elif act == "sigmoid":
        gb.simple("Sigmoid", [y], out=out)
    else:
        raise ValueError(act)


def gn_graph(n, c, h, w, groups, *, act: str | None = None, form: str = "instancenorm", back: str = "shape", eps: float = 1e-5, act_swap: bool = False,
             **kw) -> bytes:
    """x [n, c, h, w] -> group norm "gn" [-> act] -> y: the norm reads the NHWC staging copy of x, its result goes through the output copy.
    kw: GraphBuilder.group_norm's (swap, affine, per_group, inner)"""
    gb = models.GraphBuilder("gn", 31)
    y = gb.group_norm("x", c, groups, eps=eps, form=form, back=back, hw=(h, w), name="gn", **kw)
    _act(gb, y, act, "y", act_swap)
    return gb.finish([("x", [n, c, h, w])], [("y", [n, c, h, w])], opset=OPSET[form])


def gn_rank3_graph(n, c, h, w, groups, *, form: str = "instancenorm", back: str = "shape", eps: float = 1e-5) -> bytes:
    """x -> Reshape [0, c, -1] -> group norm on the flat form -> Transpose [0,2,1] -> Transpose [0,2,1] -> Reshape [0, c, h, w] -> y"""
    gb = models.GraphBuilder("gn3", 32)
    f = gb.simple("Reshape", ["x", gb.init("flat_shape", np.array([0, c, -1], np.int64))])
    y = gb.group_norm(f, c, groups, eps=eps, form=form, back=back, rank3=True, hw=(h, w), name="gn")
    y = gb.transpose(gb.transpose(y, (0, 2, 1)), (0, 2, 1))
    gb.simple("Reshape", [y, gb.init("back_shape", np.array([0, c, h, w], np.int64))], out="y")
    return gb.finish([("x", [n, c, h, w])], [("y", [n, c, h, w])], opset=OPSET[form])


def gn_alias_graph(n, c, h, w, groups, *, act: str | None = "silu") -> bytes:
    """x -> Conv1x1 "pre" -> group norm [-> act] -> Conv1x1 "post" -> y: the norm's input dies at the norm, so the step writes in place"""
    gb = models.GraphBuilder("gna", 33)
    a = gb.conv("x", c, c, 1, bias=True, name="pre")
    y = gb.group_norm(a, c, groups, back="shape", name="gn")
    if act == "silu":
        y = gb.silu(y)
    gb.conv(y, c, c, 1, bias=True, name="post", out="y")
    return gb.finish([("x", [n, c, h, w])], [("y", [n, c, h, w])], opset=17)


def gn_step(plan: dict) -> dict:
    (s,) = [s for s in plan["steps"] if s["kind"] == "group_norm"]
    return s


def half_exact(x) -> np.ndarray:
    """x rounded to half precision once, as float32: both precisions then read the same numbers, and the fp16 bound measures the kernels instead of
    the rounding of the graph input (a group of mean 8 and scale 0.25 alone would spend 2^-9 / 0.25 / 4.5 = 3.5e-3 of max|ref| on that)"""
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def data(kind: str, n: int, c: int, h: int, w: int, groups: int, seed: int = 0) -> np.ndarray:
    """"randn"; "distinct": every (image, group) its own mean in [-8, 8] and its own scale in [0.25, 4]; "mean100": 100 + N(0, 1).  Half-exact values"""
    st = np.random.RandomState(1000 * seed + 7 * c + h * w + groups)
    x = st.randn(n, c, h, w)
    if kind == "distinct":
        mean = st.uniform(-8.0, 8.0, (n, groups, 1, 1, 1))
        scale = np.exp(st.uniform(np.log(0.25), np.log(4.0), (n, groups, 1, 1, 1)))
        x = (x.reshape(n, groups, c // groups, h, w) * scale + mean).reshape(n, c, h, w)
    elif kind == "mean100":
        x = 100.0 + x
    elif kind != "randn":
        raise ValueError(kind)
    return half_exact(x)


def narrow_decoder(batch=2, **kw) -> bytes:
    """the VAE decoder on base 32 (channels 32 / 64 / 128 / 128, 8 groups), latents 8 x 8 -> 64 x 64 samples"""
    return models.vae_decoder(batch, **{**NARROW, **kw})


NARROW = dict(latent=8, base=32, mults=(1, 2, 4, 4), layers=2, groups=8, latent_ch=4)


def decoder_torch_f64(model_bytes: bytes, z, *, base: int, mults, layers: int, groups: int, **_) -> np.ndarray:
    """The decoder as diffusers computes it, in double precision with torch's own operators (F.group_norm, F.conv2d, F.interpolate(mode="nearest"),
    softmax), the weights taken from the "instancenorm" graph's initializers by name"""
    import torch
    import torch.nn.functional as F
    W = {k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in O.load_model(model_bytes).inits.items() if np.asarray(v).dtype.kind == "f"}
    eps = float(np.float32(1e-6))

    def conv(x, name, pad):
        return F.conv2d(x, W[name + "_w"], W[name + "_b"], padding=pad)

    def gn(x, name):
        return F.group_norm(x, groups, W[name + "_gamma"].reshape(-1), W[name + "_beta"].reshape(-1), eps)

    def res(x, tag):
        h = conv(F.silu(gn(x, tag + "_norm1")), tag + "_conv1", 1)
        h = conv(F.silu(gn(h, tag + "_norm2")), tag + "_conv2", 1)
        return (conv(x, tag + "_conv_shortcut", 0) if tag + "_conv_shortcut_w" in W else x) + h

    def lin(t, name):
        return t @ W[name + "_w"] + W[name + "_b"]

    def attn(x, tag):
        n, c, h, w = x.shape
        t = gn(x.reshape(n, c, h * w), tag + "_group_norm").transpose(1, 2)
        q, k, v = (lin(t, f"{tag}_to_{s}") for s in "qkv")
        p = torch.softmax((q @ k.transpose(1, 2)) * float(W[tag + "_sqrt_scale"]) ** 2, dim=-1)
        return lin(p @ v, tag + "_to_out").transpose(1, 2).reshape(n, c, h, w) + x

    with torch.no_grad():
        x = conv(conv(torch.from_numpy(np.asarray(z, np.float64)), "post_quant_conv", 0), "conv_in", 1)
        x = res(attn(res(x, "mid_res1"), "mid_attn"), "mid_res2")
        for bi in range(len(mults)):
            for li in range(layers + 1):
                x = res(x, f"up{bi}_res{li}")
            if bi + 1 < len(mults):
                x = conv(F.interpolate(x, scale_factor=2.0, mode="nearest"), f"up{bi}_upsample_conv", 1)
        return conv(F.silu(gn(x, "conv_norm_out")), "conv_out", 1).numpy()
