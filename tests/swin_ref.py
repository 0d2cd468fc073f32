"""Float64 reference for the Swin tests (window attention, patch merging): a numpy walk of the literal ONNX nodes in double precision, in the manner
of tests/vit_ref.py and independent of the planner's matching: the roll is its two Slices and a Concat, the window partition its rank-6 Reshape and
Transpose, the patch merging its eight strided Slices.

Slice, Pad, Concat, Reshape, Transpose, Gather, Split, Squeeze, Unsqueeze, Softmax, GlobalAveragePool, Flatten and the N-D MatMul follow their ONNX
definitions (Slice: per axis x[start:end:step] with numpy's clamping, which is ONNX's; Pad: constant mode).  Softmax, Reshape and the error measure
are vit_ref's, LayerNormalization and GELU convnext_ref's, Conv torch's double-precision conv2d.
"""
from __future__ import annotations

import math

import numpy as np

import convnext_ref
import vit_ref
from oracle import onnx_oracle as O

rel_err = vit_ref.rel_err
softmax = vit_ref.softmax
reshape = vit_ref.reshape
layer_norm = convnext_ref.layer_norm
_s = convnext_ref._s


def slice_(x, starts, ends, axes=None, steps=None):
    axes = list(range(len(starts))) if axes is None else [int(a) for a in axes]
    steps = [1] * len(starts) if steps is None else [int(s) for s in steps]
    idx = [slice(None)] * x.ndim
    for st, en, ax, sp in zip(starts, ends, axes, steps):
        idx[ax] = slice(int(st), int(en), sp)
    return x[tuple(idx)]


def pad(x, pads, value=0.0):
    r = x.ndim
    return np.pad(x, [(int(pads[k]), int(pads[k + r])) for k in range(r)], mode="constant", constant_values=value)


def run_f64(model_bytes: bytes, feeds: dict, overrides: dict | None = None) -> dict:
    """overrides: initializer name -> replacement (the tests zero a bias or a mask with it)"""
    import torch
    import torch.nn.functional as F
    m = O.load_model(model_bytes)
    env = {k: (np.asarray(v, np.float64) if np.asarray(v).dtype.kind == "f" else np.asarray(v)) for k, v in m.inits.items()}
    for k, v in (overrides or {}).items():
        assert k in env and np.shape(v) == env[k].shape, k
        env[k] = np.asarray(v, np.float64)
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
        elif op == "Slice":
            y = slice_(i[0], i[1], i[2], i[3] if len(i) > 3 else None, i[4] if len(i) > 4 else None)
        elif op == "Pad":
            assert _s(a.get("mode", "constant")) == "constant"
            y = pad(i[0], i[1], float(i[2]) if len(i) > 2 and i[2] is not None else 0.0)
        elif op == "Reshape":
            y = reshape(i[0], list(i[1]))
        elif op == "Transpose":
            y = i[0].transpose(*a["perm"])
        elif op == "Concat":
            y = np.concatenate(i, axis=a.get("axis", 1))
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
            for name, part in zip(n.outputs, np.split(i[0], np.cumsum(sizes)[:-1], axis=a.get("axis", 0))):
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
        elif op == "GlobalAveragePool":
            y = i[0].mean(axis=(2, 3), keepdims=True)
        elif op == "Flatten":
            ax = a.get("axis", 1)
            y = i[0].reshape(int(np.prod(i[0].shape[:ax], dtype=np.int64)), -1)
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
        elif op == "Relu":
            y = np.maximum(i[0], 0.0)
        elif op == "Identity":
            y = i[0]
        else:
            raise NotImplementedError(op)
        env[n.outputs[0]] = y
    return {name: np.asarray(env[name], np.float64) for name, _, _ in m.outputs}
