"""The float64 reference every parity test rests on: one walk of an ONNX graph in double precision, and the operator restatements it dispatches to.

Decoding is the oracle's own reader (O.load_model).  Floating-point initializers, feeds and constants become float64; integer ones stay integers
(so finfo(float32).min * (1 - mask) is the exact product a BERT graph asks for).  Arrays are numpy throughout; only Conv, ConvTranspose and MaxPool
go through torch's double-precision operators, behind an explicit F.pad (asymmetric pads work; MaxPool pads with -inf).  Everything else is
written out from its ONNX definition, not taken from a library's fused operator: LayerNormalization as (x - mean) / sqrt(var + epsilon) * scale + B
(ln_agrees_with_torch() checks it against F.layer_norm), GroupNormalization / InstanceNormalization through group_norm(), Resize through
resize_ref(), ConvTranspose with asymmetric pads through convt_scatter().

A new operator is one entry in OPS: a function of (inputs, attributes, model) that returns the output array (a list of arrays for several outputs).
tests/test_ref64.py pins the walk to the per-family walkers it replaced (tests/golden/ref64_parent.npz) and to the independent oracle.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import onnx_oracle as O

COORDS = ("half_pixel", "pytorch_half_pixel", "align_corners", "asymmetric")
NEAREST = ("round_prefer_floor", "round_prefer_ceil", "floor", "ceil")
_CAST = {1: np.float64, 6: np.int32, 7: np.int64, 9: np.bool_, 10: np.float64, 11: np.float64}
_erf = np.vectorize(math.erf, otypes=[np.float64])


def rel_err(y, ref) -> float:
    """max |y - ref| / max |ref|"""
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(y, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


def _s(v):
    return v.decode() if isinstance(v, bytes) else v


def _f64(v):
    v = np.asarray(v)
    return v.astype(np.float64) if v.dtype.kind == "f" else v


def _half(v):
    return np.asarray(v, np.float64).astype(np.float16).astype(np.float64)


def _t(v):
    return None if v is None else torch.from_numpy(np.ascontiguousarray(v))


def _opt(i, k):
    return i[k] if len(i) > k else None


# ---- the operator restatements ----------------------------------------------------------------------------------------------------------------
def softmax(x, axis: int = -1):
    e = np.exp(x - x.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def reshape(x, shape):
    shape = [int(x.shape[k]) if d == 0 else int(d) for k, d in enumerate(shape)]
    return x.reshape(shape)


def attention(qkv, heads: int, scale: float):
    """the attention step from its definition: qkv [N, L, 3 D] float64 -> [N, L, D]"""
    n, l, d3 = qkv.shape
    d = d3 // 3
    t = qkv.reshape(n, l, 3, heads, d // heads).transpose(2, 0, 3, 1, 4)
    p = softmax(scale * (t[0] @ t[1].transpose(0, 1, 3, 2)), -1)
    return (p @ t[2]).transpose(0, 2, 1, 3).reshape(n, l, d)


def gather(data, idx, axis: int = 0):
    """range-checked; negative indices count from the end, as ONNX defines"""
    idx = np.asarray(idx)
    n = data.shape[axis]
    if ((idx < -n) | (idx >= n)).any():
        raise IndexError("Gather index out of range")
    return np.take(data, np.where(idx < 0, idx + n, idx), axis=axis)


def slice_(x, starts, ends, axes=None, steps=None):
    """per axis x[start:end:step] with numpy's clamping, which is ONNX's"""
    axes = list(range(len(starts))) if axes is None else [int(a) for a in axes]
    steps = [1] * len(starts) if steps is None else [int(s) for s in steps]
    idx = [slice(None)] * x.ndim
    for st, en, ax, sp in zip(starts, ends, axes, steps):
        idx[ax] = slice(int(st), int(en), sp)
    return x[tuple(idx)]


def pad(x, pads, value=0.0):
    r = x.ndim
    return np.pad(x, [(int(pads[k]), int(pads[k + r])) for k in range(r)], mode="constant", constant_values=value)


def layer_norm(x, scale, bias=None, axis: int = -1, eps: float = 1e-5) -> np.ndarray:
    """ONNX LayerNormalization in float64: normalises over the axes [axis, rank)"""
    x = np.asarray(x, np.float64)
    if axis < 0:
        axis += x.ndim
    axes = tuple(range(axis, x.ndim))
    mean = x.mean(axis=axes, keepdims=True)
    d = x - mean
    var = (d * d).mean(axis=axes, keepdims=True)
    y = d / np.sqrt(var + eps) * np.asarray(scale, np.float64)
    return y if bias is None else y + np.asarray(bias, np.float64)


def ln_agrees_with_torch() -> float:
    """max |layer_norm - F.layer_norm| over a seeded [2, 3, 5, 24] tensor in double"""
    st = np.random.RandomState(11)
    x, g, b = 3.0 + st.randn(2, 3, 5, 24), st.randn(24), st.randn(24)
    t = F.layer_norm(torch.from_numpy(x), (24,), torch.from_numpy(g), torch.from_numpy(b), 1e-6).numpy()
    return float(np.abs(layer_norm(x, g, b, -1, 1e-6) - t).max())


def group_norm(x, groups: int, gamma=None, beta=None, eps: float = 1e-5, stats: str = "group", shift: int = 0) -> np.ndarray:
    """GroupNorm of x [N, C, *spatial] in float64; gamma / beta [C] or None.
    stats: "group" the definition; the broken variants "image" (one mean / variance per image), "batch" (per group, shared by all images).
    shift: the group boundaries moved by this many channels (a broken variant; the channels wrap around)"""
    x = np.asarray(x, np.float64)
    n, c = x.shape[:2]
    xs = np.roll(x, -shift, axis=1) if shift else x
    g = xs.reshape(n, groups, -1)
    if stats == "group":
        mean, var = g.mean(axis=2, keepdims=True), g.var(axis=2, keepdims=True)
    elif stats == "image":
        mean, var = g.mean(axis=(1, 2), keepdims=True), g.var(axis=(1, 2), keepdims=True)
    elif stats == "batch":
        mean, var = g.mean(axis=(0, 2), keepdims=True), g.var(axis=(0, 2), keepdims=True)
    else:
        raise ValueError(stats)
    y = ((g - mean) / np.sqrt(var + eps)).reshape(xs.shape)
    if shift:
        y = np.roll(y, shift, axis=1)
    tail = (1, c) + (1,) * (x.ndim - 2)
    if gamma is not None:
        y = y * np.asarray(gamma, np.float64).reshape(tail)
    if beta is not None:
        y = y + np.asarray(beta, np.float64).reshape(tail)
    return y


def _axis(in_len: int, out_len: int, scale: float, mode: str, coord: str, nearest: str):
    """Per output index along one axis: (i0, i1, w) with value = (1 - w) * in[i0] + w * in[i1] (nearest: w = 0)"""
    o = np.arange(out_len, dtype=np.float64)
    if coord == "half_pixel":
        x = (o + 0.5) / scale - 0.5
    elif coord == "pytorch_half_pixel":
        x = (o + 0.5) / scale - 0.5 if out_len > 1 else np.zeros_like(o)
    elif coord == "align_corners":
        x = o * (in_len - 1) / (out_len - 1) if out_len > 1 else np.zeros_like(o)
    elif coord == "asymmetric":
        x = o / scale
    else:
        raise ValueError(coord)
    if mode == "nearest":
        fl = np.floor(x)
        tie = x == fl + 0.5
        if nearest == "round_prefer_floor":
            r = np.where(tie, fl, np.rint(x))
        elif nearest == "round_prefer_ceil":
            r = np.where(tie, np.ceil(x), np.rint(x))
        elif nearest == "floor":
            r = fl
        else:
            r = np.ceil(x)
        i = np.clip(r, 0, in_len - 1).astype(np.int64)
        return i, i, np.zeros_like(x)
    fl = np.floor(x)
    w = x - fl
    i = fl.astype(np.int64)
    return np.clip(i, 0, in_len - 1), np.clip(i + 1, 0, in_len - 1), w


def resize_ref(x: np.ndarray, out_hw, scales_hw, mode: str, coord: str, nearest: str = "round_prefer_floor") -> np.ndarray:
    """ONNX Resize of an NCHW array to out_hw, the coordinate transform dividing by scales_hw (the given scales, or out / in for sizes)"""
    x = np.asarray(x, np.float64)
    iy0, iy1, wy = _axis(x.shape[2], out_hw[0], scales_hw[0], mode, coord, nearest)
    ix0, ix1, wx = _axis(x.shape[3], out_hw[1], scales_hw[1], mode, coord, nearest)
    top = x[:, :, iy0][:, :, :, ix0] * (1 - wx) + x[:, :, iy0][:, :, :, ix1] * wx
    bot = x[:, :, iy1][:, :, :, ix0] * (1 - wx) + x[:, :, iy1][:, :, :, ix1] * wx
    wy = wy[:, None]
    return top * (1 - wy) + bot * wy


def depthwise_s1(x, w, bias, pads):
    """stride-1 depthwise conv from its definition: the sum over the taps of the shifted, per-channel weighted input.  x [N, C, H, W],
    w [C, 1, kh, kw], pads = (top, left, bottom, right).  (torch's grouped double conv is ~20x slower)"""
    kh, kw = w.shape[2], w.shape[3]
    xp = np.pad(x, ((0, 0), (0, 0), (pads[0], pads[2]), (pads[1], pads[3])))
    oh, ow = xp.shape[2] - kh + 1, xp.shape[3] - kw + 1
    y = 0
    for ky in range(kh):
        for kx in range(kw):
            y = y + xp[:, :, ky:ky + oh, kx:kx + ow] * w[:, 0, ky, kx].reshape(1, -1, 1, 1)
    return y if bias is None else y + bias.reshape(1, -1, 1, 1)


def convt_out_hw(h, w, k, strides, pads, output_padding=(0, 0)):
    """ONNX ConvTranspose output extent: (H - 1) * s + k - p0 - p1 + output_padding per axis; pads = (top, left, bottom, right)"""
    return ((h - 1) * strides[0] + k[0] - pads[0] - pads[2] + output_padding[0], (w - 1) * strides[1] + k[1] - pads[1] - pads[3] + output_padding[1])


def convt_scatter(x, w, bias=None, strides=(1, 1), pads=(0, 0, 0, 0), output_padding=(0, 0)) -> np.ndarray:
    """The ONNX definition as a scatter, float64: every input pixel (iy, ix) adds x[n, c, iy, ix] * w[c, o, ky, kx] to the full output at
    (iy * sh + ky, ix * sw + kx); the pads then cut rows / columns off both ends and output_padding appends (zero) rows / columns at the
    bottom / right before the bias.  x [N, Cin, H, W], w [Cin, Cout, kh, kw], pads = (top, left, bottom, right)."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    n, cin, h, wd = x.shape
    _, cout, kh, kw = w.shape
    sh, sw = strides
    oh, ow = convt_out_hw(h, wd, (kh, kw), strides, pads, output_padding)
    full = np.zeros((n, cout, (h - 1) * sh + kh + output_padding[0], (wd - 1) * sw + kw + output_padding[1]))
    for ky in range(kh):
        for kx in range(kw):
            full[:, :, ky:ky + (h - 1) * sh + 1:sh, kx:kx + (wd - 1) * sw + 1:sw] += np.einsum("nchw,co->nohw", x, w[:, :, ky, kx])
    y = full[:, :, pads[0]:pads[0] + oh, pads[1]:pads[1] + ow]
    assert y.shape == (n, cout, oh, ow), (y.shape, (n, cout, oh, ow))
    if bias is not None:
        y = y + np.asarray(bias, np.float64).reshape(1, -1, 1, 1)
    return y


def convt_torch(x, w, bias=None, strides=(1, 1), pad=(0, 0), output_padding=(0, 0)) -> np.ndarray:
    """torch's double F.conv_transpose2d (symmetric pads only: pad = (rows, columns))"""
    t = lambda a: None if a is None else _t(np.asarray(a, np.float64))  # noqa: E731
    with torch.no_grad():
        return F.conv_transpose2d(t(x), t(w), t(bias), stride=tuple(strides), padding=tuple(pad), output_padding=tuple(output_padding)).numpy()


# ---- the operators of the walk: (inputs, attributes, model) -> output --------------------------------------------------------------------------
def _hw_pad(x, p, value=0.0):
    return F.pad(_t(x), (p[1], p[3], p[0], p[2]), value=value)


def _conv(i, a, m):
    x, w, b = i[0], i[1], _opt(i, 2)
    p, s, d, g = a.get("pads", [0, 0, 0, 0]), tuple(a.get("strides", [1, 1])), tuple(a.get("dilations", [1, 1])), a.get("group", 1)
    if g == x.shape[1] == w.shape[0] and w.shape[1] == 1 and s == (1, 1) and d == (1, 1):
        return depthwise_s1(x, w, b, p)
    return F.conv2d(_hw_pad(x, p), _t(w), _t(b), stride=s, dilation=d, groups=g).numpy()


def _conv_transpose(i, a, m):
    p, st, opad = a.get("pads", [0, 0, 0, 0]), tuple(a.get("strides", [1, 1])), tuple(a.get("output_padding", [0, 0]))
    assert a.get("group", 1) == 1 and tuple(a.get("dilations", [1, 1])) == (1, 1)
    if p[0] == p[2] and p[1] == p[3]:
        return convt_torch(i[0], i[1], _opt(i, 2), st, (p[0], p[1]), opad)
    return convt_scatter(i[0], i[1], _opt(i, 2), st, tuple(p), opad)      # (torch cannot express asymmetric pads)


def _max_pool(i, a, m):
    assert not a.get("ceil_mode", 0)
    return F.max_pool2d(_hw_pad(i[0], a.get("pads", [0, 0, 0, 0]), -np.inf), tuple(a["kernel_shape"]), stride=tuple(a.get("strides", [1, 1]))).numpy()


def _batch_norm(i, a, m):
    x, scale, bias, mean, var = i[:5]
    sh = (1, -1) + (1,) * (x.ndim - 2)
    return (x - mean.reshape(sh)) / np.sqrt(var.reshape(sh) + a.get("epsilon", 1e-5)) * scale.reshape(sh) + bias.reshape(sh)


def _eps(a):
    return float(np.float32(a.get("epsilon", 1e-5)))


def _group_normalization(i, a, m):
    g, c = a["num_groups"], i[0].shape[1]
    sc, bi = (i[1], i[2]) if m.opset >= 21 else (np.repeat(i[1], c // g), np.repeat(i[2], c // g))       # per group below opset 21
    return group_norm(i[0], g, sc, bi, _eps(a))


def _arith(f):
    def go(i, a, m):
        b = i[1]
        if 0 < m.opset < 7 and a.get("broadcast", 0) and "axis" in a:          # the opset-6 form: B's dims align with A's from `axis` on
            ax = a["axis"] + (i[0].ndim if a["axis"] < 0 else 0)
            b = b.reshape((1,) * ax + b.shape + (1,) * (i[0].ndim - ax - b.ndim))
        return f(i[0], b)
    return go


def _clip(i, a, m):
    lo = a["min"] if "min" in a else (float(np.ravel(i[1])[0]) if _opt(i, 1) is not None else None)
    hi = a["max"] if "max" in a else (float(np.ravel(i[2])[0]) if _opt(i, 2) is not None else None)
    y = i[0]
    if lo is not None:
        y = np.maximum(y, lo)
    if hi is not None:
        y = np.minimum(y, hi)
    return y


def _gelu(i, a, m):
    x = i[0]
    if _s(a.get("approximate", "none")) == "tanh":
        return 0.5 * x * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (x + 0.044715 * x ** 3)))
    return 0.5 * x * (1.0 + _erf(x / np.sqrt(2.0)))


def _gemm(i, a, m):
    A = i[0].T if a.get("transA", 0) else i[0]
    Bm = i[1].T if a.get("transB", 0) else i[1]
    y = a.get("alpha", 1.0) * (A @ Bm)
    return y if _opt(i, 2) is None else y + a.get("beta", 1.0) * i[2]


def _constant(i, a, m):
    (k, v), = a.items()
    return _f64(np.asarray(v, np.int64 if k.startswith("value_int") else None))


def _concat(i, a, m):
    if all(np.ndim(v) <= 1 for v in i):                                         # shape vectors (and the scalars Gather leaves of them)
        return np.concatenate([np.reshape(v, -1) for v in i])
    return np.concatenate(i, axis=a.get("axis", 1))


def _axes(i, a):
    axes = a["axes"] if "axes" in a else _opt(i, 1)
    return None if axes is None else [int(v) for v in axes]


def _unsqueeze(i, a, m):
    axes = _axes(i, a)
    rank = i[0].ndim + len(axes)
    y = i[0]
    for ax in sorted(v + rank if v < 0 else v for v in axes):
        y = np.expand_dims(y, ax)
    return y


def _squeeze(i, a, m):
    axes = _axes(i, a)
    return np.squeeze(i[0], None if axes is None else tuple(axes))


def _split(i, a, m):
    sizes = [int(v) for v in (a["split"] if "split" in a else i[1])]
    return list(np.split(i[0], np.cumsum(sizes)[:-1], axis=a.get("axis", 0)))


def _slice(i, a, m):
    r = lambda k: None if _opt(i, k) is None else np.ravel(i[k])  # noqa: E731
    return slice_(i[0], r(1), r(2), r(3), r(4))


def _pad(i, a, m):
    assert _s(a.get("mode", "constant")) == "constant"
    return pad(i[0], i[1], float(i[2]) if _opt(i, 2) is not None else 0.0)


def _flatten(i, a, m):
    ax = a.get("axis", 1)
    return i[0].reshape(int(np.prod(i[0].shape[:ax], dtype=np.int64)), -1)


def _resize(legacy_op):
    def go(i, a, m):
        x = i[0]
        legacy = legacy_op or m.opset < 11
        mode = _s(a.get("mode", "nearest"))
        mode = "linear" if mode == "bilinear" else mode
        coord = "asymmetric" if legacy else _s(a.get("coordinate_transformation_mode", "half_pixel"))
        nearest = "floor" if legacy else _s(a.get("nearest_mode", "round_prefer_floor"))
        sc = i[1] if legacy else _opt(i, 2)
        sz = None if legacy else _opt(i, 3)
        h, w = x.shape[2], x.shape[3]
        if sc is not None and np.asarray(sc).size:
            s = np.asarray(sc, np.float64).ravel()
            s = [float(np.float32(s[2])), float(np.float32(s[3]))]
            out = (int(np.floor(h * s[0])), int(np.floor(w * s[1])))
        else:
            z = np.asarray(sz).ravel()
            out = (int(z[2]), int(z[3]))
            s = [out[0] / h, out[1] / w]
        return resize_ref(x, out, s, mode, coord, nearest)
    return go


OPS = {
    "Constant": _constant,
    "Conv": _conv,
    "ConvTranspose": _conv_transpose,
    "BatchNormalization": _batch_norm,
    "MaxPool": _max_pool,
    "AveragePool": lambda i, a, m: O.avgpool(i[0], a["kernel_shape"], a.get("strides", [1, 1]), a.get("pads", [0, 0, 0, 0]), a.get("count_include_pad", 0)),
    "GlobalAveragePool": lambda i, a, m: i[0].mean(axis=(2, 3), keepdims=True),
    "Relu": lambda i, a, m: np.maximum(i[0], 0.0),
    "Sigmoid": lambda i, a, m: 1.0 / (1.0 + np.exp(-i[0])),
    "Tanh": lambda i, a, m: np.tanh(i[0]),
    "HardSigmoid": lambda i, a, m: np.clip(a.get("alpha", 0.2) * i[0] + a.get("beta", 0.5), 0.0, 1.0),
    "HardSwish": lambda i, a, m: i[0] * np.clip(i[0] / 6.0 + 0.5, 0.0, 1.0),
    "Erf": lambda i, a, m: _erf(i[0]),
    "Gelu": _gelu,
    "Clip": _clip,
    "Add": _arith(lambda x, y: x + y),
    "Sub": _arith(lambda x, y: x - y),
    "Mul": _arith(lambda x, y: x * y),
    "Div": _arith(lambda x, y: x / y),
    "Identity": lambda i, a, m: i[0],
    "Dropout": lambda i, a, m: i[0],
    "Gemm": _gemm,
    "MatMul": lambda i, a, m: np.matmul(i[0], i[1]),
    "Softmax": lambda i, a, m: softmax(i[0], a.get("axis", -1)),
    "LayerNormalization": lambda i, a, m: layer_norm(i[0], i[1], _opt(i, 2), a.get("axis", -1), _eps(a)),
    "InstanceNormalization": lambda i, a, m: group_norm(i[0], i[0].shape[1], i[1], i[2], _eps(a)),
    "GroupNormalization": _group_normalization,
    "Reshape": lambda i, a, m: reshape(i[0], list(i[1])),
    "Transpose": lambda i, a, m: i[0].transpose(*a["perm"]),
    "Expand": lambda i, a, m: i[0] * np.ones([int(d) for d in i[1]], i[0].dtype),
    "Shape": lambda i, a, m: np.array(i[0].shape, np.int64),
    "Flatten": _flatten,
    "Split": _split,
    "Pad": _pad,
    "Squeeze": _squeeze,
    "Unsqueeze": _unsqueeze,
    "Concat": _concat,
    "Gather": lambda i, a, m: gather(i[0], i[1], a.get("axis", 0)),
    "Slice": _slice,
    "Cast": lambda i, a, m: i[0].astype(_CAST[a["to"]]),
    "Resize": _resize(False),
    "Upsample": _resize(True),
}


def run_f64(model_bytes: bytes, feeds: dict, *, round_half: bool = False, overrides: dict | None = None) -> dict:
    """-> {output name: float64 array}.  A feed may name an initializer and then replaces it.
    round_half: every node's floating-point result and the weights of every Conv / Gemm / MatMul are rounded to half precision (the storage an
    fp16 plan gives them), the arithmetic staying double: what the number format alone costs an fp16 run of this depth.
    overrides: initializer name -> replacement of the same shape (the tests zero a bias or a mask with it)"""
    m = O.load_model(model_bytes)
    env = {k: _f64(v) for k, v in m.inits.items()}
    for k, v in (overrides or {}).items():
        assert k in env and np.shape(v) == env[k].shape, k
        env[k] = np.asarray(v, np.float64)
    if round_half:
        for n in m.nodes:
            if n.op in ("Conv", "Gemm", "MatMul") and n.inputs[1] in m.inits:
                env[n.inputs[1]] = _half(env[n.inputs[1]])
    env.update({k: _f64(v) for k, v in feeds.items()})
    for n in m.nodes:
        if n.op not in OPS:
            raise NotImplementedError(n.op)
        y = OPS[n.op]([env[x] if x else None for x in n.inputs], n.attrs, m)
        for name, v in zip(n.outputs, y if isinstance(y, list) else [y]):
            env[name] = _half(v) if round_half and np.asarray(v).dtype.kind == "f" else v
    return {name: np.asarray(env[name], np.float64) for name, _, _ in m.outputs}


def conv_macs(model_bytes: bytes, input_shape) -> dict:
    """{node name: multiply-accumulates} of every Conv (Cin / group per output, any dilation) and Gemm at the given input shape, walking shapes
    through the pools, Flatten, Concat, Resize and the broadcasting ops (whose result has the largest operand's shape)"""
    m = O.load_model(model_bytes)
    shapes = {m.inputs[0][0]: tuple(input_shape)}
    macs = {}
    for n in m.nodes:
        a = n.attrs
        known = [shapes[x] for x in n.inputs if x in shapes]
        xs = shapes.get(n.inputs[0]) if n.inputs else None
        if n.op in ("Add", "Sub", "Mul", "Div") and known:
            ys = max(known, key=lambda q: int(np.prod(q)))
        elif xs is None:
            continue
        elif n.op in ("Conv", "MaxPool"):
            if n.op == "Conv":
                co, cg, kh, kw = m.inits[n.inputs[1]].shape
            else:
                co, cg, (kh, kw) = xs[1], 0, a["kernel_shape"]
            d, p, s = a.get("dilations", [1, 1]), a.get("pads", [0, 0, 0, 0]), a.get("strides", [1, 1])
            oh = (xs[2] + p[0] + p[2] - ((kh - 1) * d[0] + 1)) // s[0] + 1
            ow = (xs[3] + p[1] + p[3] - ((kw - 1) * d[1] + 1)) // s[1] + 1
            if n.op == "Conv":
                macs[n.name or n.outputs[0]] = xs[0] * co * oh * ow * cg * kh * kw
            ys = (xs[0], co, oh, ow)
        elif n.op == "Gemm":
            w = m.inits[n.inputs[1]]
            nout = w.shape[0] if a.get("transB", 0) else w.shape[1]
            macs[n.name or n.outputs[0]] = xs[0] * xs[1] * nout
            ys = (xs[0], nout)
        elif n.op == "GlobalAveragePool":
            ys = (xs[0], xs[1], 1, 1)
        elif n.op == "Flatten":
            ys = (xs[0], int(np.prod(xs[1:])))
        elif n.op == "Concat":
            ys = (xs[0], sum(q[1] for q in known)) + tuple(xs[2:])
        elif n.op in ("Resize", "Upsample"):
            if len(n.inputs) > 3 and n.inputs[3] in m.inits:
                ys = tuple(int(v) for v in np.asarray(m.inits[n.inputs[3]]).ravel())
            else:
                sc = np.asarray(m.inits[n.inputs[2] if len(n.inputs) > 2 else n.inputs[1]], np.float64).ravel()
                ys = (xs[0], xs[1], int(np.floor(xs[2] * sc[2])), int(np.floor(xs[3] * sc[3])))
        else:
            ys = xs
        shapes[n.outputs[0]] = ys
    return macs
