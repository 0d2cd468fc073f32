"""Float64 reference for the ViT tests (token views, attention): a numpy walk of an ONNX graph in double precision, in the manner of
tests/convnext_ref.py.  Decoding is the oracle's own reader (O.load_model).

Reshape, Transpose, Expand, Concat, Gather, Split, Squeeze, Unsqueeze, Shape, Softmax and the N-D MatMul follow their ONNX definitions (Reshape's
0 / -1 entries, Expand's two-way broadcast, Softmax as exp(x - max) / sum along one axis).  LayerNormalization and GELU are convnext_ref's; Conv is
torch's double-precision conv2d.
"""
from __future__ import annotations

import math

import numpy as np

import convnext_ref
from oracle import onnx_oracle as O

layer_norm = convnext_ref.layer_norm
_s = convnext_ref._s


def rel_err(y, ref) -> float:
    """max |y - ref| / max |ref|"""
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(y, np.float64) - ref).max() / np.abs(ref).max())


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


def run_f64(model_bytes: bytes, feeds: dict) -> dict:
    import torch
    import torch.nn.functional as F
    m = O.load_model(model_bytes)
    env = {k: (np.asarray(v, np.float64) if np.asarray(v).dtype.kind == "f" else np.asarray(v)) for k, v in m.inits.items()}
    env.update({k: np.asarray(v, np.float64) for k, v in feeds.items()})
    erf = np.vectorize(math.erf, otypes=[np.float64])
    for n in m.nodes:
        a = n.attrs
        i = [env[x] if x else None for x in n.inputs]
        op = n.op
        if op == "Constant":
            (k, v), = a.items()
            y = np.asarray(v, np.int64 if k.startswith("value_int") else None)
            if y.dtype.kind == "f":
                y = y.astype(np.float64)
        elif op == "Conv":
            p = a.get("pads", [0, 0, 0, 0])
            t = [torch.from_numpy(np.ascontiguousarray(v)) if v is not None else None for v in i]
            y = F.conv2d(F.pad(t[0], (p[1], p[3], p[0], p[2])), t[1], t[2] if len(t) > 2 else None, stride=tuple(a.get("strides", [1, 1])),
                         dilation=tuple(a.get("dilations", [1, 1])), groups=a.get("group", 1)).numpy()
        elif op == "Reshape":
            y = reshape(i[0], list(i[1]))
        elif op == "Transpose":
            y = i[0].transpose(*a["perm"])
        elif op == "Expand":
            y = i[0] * np.ones([int(d) for d in i[1]], i[0].dtype)
        elif op == "Concat":
            y = np.concatenate(i, axis=a.get("axis", 1))
        elif op == "Shape":
            y = np.array(i[0].shape, np.int64)
        elif op == "Gather":
            y = np.take(i[0], i[1], axis=a.get("axis", 0))
        elif op == "Unsqueeze":
            axes = a["axes"] if "axes" in a else list(i[1])
            y = i[0]
            for ax in sorted(int(v) for v in axes):
                y = np.expand_dims(y, ax)
        elif op == "Squeeze":
            axes = a["axes"] if "axes" in a else list(i[1])
            y = np.squeeze(i[0], tuple(int(v) for v in axes))
        elif op == "Split":
            sizes = [int(v) for v in i[1]]
            parts = np.split(i[0], np.cumsum(sizes)[:-1], axis=a.get("axis", 0))
            for name, part in zip(n.outputs, parts):
                env[name] = part
            continue
        elif op == "Softmax":
            y = softmax(i[0], a.get("axis", -1))
        elif op == "MatMul":
            y = np.matmul(i[0], i[1])
        elif op == "LayerNormalization":
            y = layer_norm(i[0], i[1], i[2] if len(i) > 2 and i[2] is not None else None, a.get("axis", -1), float(np.float32(a.get("epsilon", 1e-5))))
        elif op == "Erf":
            y = erf(i[0])
        elif op == "Gelu":
            x = i[0]
            if _s(a.get("approximate", "none")) == "tanh":
                y = 0.5 * x * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (x + 0.044715 * x ** 3)))
            else:
                y = 0.5 * x * (1.0 + erf(x / np.sqrt(2.0)))
        elif op == "Gemm":
            A = i[0].T if a.get("transA", 0) else i[0]
            Bm = i[1].T if a.get("transB", 0) else i[1]
            y = a.get("alpha", 1.0) * (A @ Bm)
            if len(i) > 2 and i[2] is not None:
                y = y + a.get("beta", 1.0) * i[2]
        elif op == "Add":
            y = i[0] + i[1]
        elif op == "Mul":
            y = i[0] * i[1]
        elif op == "Div":
            y = i[0] / i[1]
        elif op == "Identity":
            y = i[0]
        else:
            raise NotImplementedError(op)
        env[n.outputs[0]] = y
    return {name: np.asarray(env[name], np.float64) for name, _, _ in m.outputs}
