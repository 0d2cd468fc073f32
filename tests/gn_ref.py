"""Float64 reference for the GroupNorm tests (GroupNorm ResNets, the diffusion VAE decoder): a numpy walk of an ONNX graph in double precision,
in the manner of tests/bert_ref.py, whose helpers it shares.  Decoding is the oracle's own reader (O.load_model).

InstanceNormalization and GroupNormalization are restated here from their ONNX definitions (the mean and the variance of the centred values
over the spatial axes of one channel / over the channels of one group and the spatial axes; GroupNormalization's scale and bias per group below
opset 21, per channel from it on).  group_norm() is the one function both go through; its `stats` argument exists for the tests' broken
variants.  Conv and the pools are torch's double-precision operators, Resize is seg_ref's restatement.
"""
from __future__ import annotations

import numpy as np

import seg_ref
import vit_ref
from oracle import onnx_oracle as O

rel_err = vit_ref.rel_err
softmax = vit_ref.softmax
_s = seg_ref._s


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


def run_f64(model_bytes: bytes, feeds: dict, round_half: bool = False) -> dict:
    """round_half: every node's floating-point result and the weights of every Conv / Gemm / MatMul are rounded to half precision (the storage an
    fp16 plan gives them), the arithmetic staying double: what the number format alone costs an fp16 run of this depth"""
    import torch
    import torch.nn.functional as F
    m = O.load_model(model_bytes)
    f64 = lambda v: np.asarray(v, np.float64) if np.asarray(v).dtype.kind == "f" else np.asarray(v)  # noqa: E731
    env = {k: f64(v) for k, v in m.inits.items()}
    env.update({k: f64(v) for k, v in feeds.items()})
    if round_half:
        for n in m.nodes:
            if n.op in ("Conv", "Gemm", "MatMul") and n.inputs[1] in m.inits:
                env[n.inputs[1]] = np.asarray(m.inits[n.inputs[1]]).astype(np.float16).astype(np.float64)
    tt = lambda v: torch.from_numpy(np.ascontiguousarray(v))  # noqa: E731
    for n in m.nodes:
        a = n.attrs
        i = [env[x] if x else None for x in n.inputs]
        op = n.op
        if op == "Constant":
            (k, v), = a.items()
            y = f64(np.asarray(v, np.int64 if k.startswith("value_int") else None))
        elif op == "Conv":
            p = a.get("pads", [0, 0, 0, 0])
            y = F.conv2d(F.pad(tt(i[0]), (p[1], p[3], p[0], p[2])), tt(i[1]), tt(i[2]) if len(i) > 2 and i[2] is not None else None,
                         stride=tuple(a.get("strides", [1, 1])), dilation=tuple(a.get("dilations", [1, 1])), groups=a.get("group", 1)).numpy()
        elif op == "InstanceNormalization":
            y = group_norm(i[0], i[0].shape[1], i[1], i[2], float(np.float32(a.get("epsilon", 1e-5))))
        elif op == "GroupNormalization":
            g, c = a["num_groups"], i[0].shape[1]
            sc, bi = (i[1], i[2]) if m.opset >= 21 else (np.repeat(i[1], c // g), np.repeat(i[2], c // g))
            y = group_norm(i[0], g, sc, bi, float(np.float32(a.get("epsilon", 1e-5))))
        elif op == "Reshape":
            y = vit_ref.reshape(i[0], list(i[1]))
        elif op == "Shape":
            y = np.array(i[0].shape, np.int64)
        elif op == "Transpose":
            y = i[0].transpose(*a["perm"])
        elif op == "Softmax":
            y = softmax(i[0], a.get("axis", -1))
        elif op == "MatMul":
            y = np.matmul(i[0], i[1])
        elif op == "Sigmoid":
            y = 1.0 / (1.0 + np.exp(-i[0]))
        elif op == "Relu":
            y = np.maximum(i[0], 0.0)
        elif op == "Add":
            y = i[0] + i[1]
        elif op == "Mul":
            y = i[0] * i[1]
        elif op == "Div":
            y = i[0] / i[1]
        elif op == "Identity":
            y = i[0]
        elif op == "Concat":
            y = np.concatenate(i, axis=a.get("axis", 1))
        elif op == "MaxPool":
            p = a.get("pads", [0, 0, 0, 0])
            y = F.max_pool2d(F.pad(tt(i[0]), (p[1], p[3], p[0], p[2]), value=-np.inf), tuple(a["kernel_shape"]), stride=tuple(a.get("strides", [1, 1]))).numpy()
        elif op == "GlobalAveragePool":
            y = i[0].mean(axis=(2, 3), keepdims=True)
        elif op == "Flatten":
            ax = a.get("axis", 1)
            y = i[0].reshape(int(np.prod(i[0].shape[:ax])), -1)
        elif op == "Gemm":
            A = i[0].T if a.get("transA", 0) else i[0]
            Bm = i[1].T if a.get("transB", 0) else i[1]
            y = a.get("alpha", 1.0) * (A @ Bm)
            if len(i) > 2 and i[2] is not None:
                y = y + a.get("beta", 1.0) * i[2]
        elif op == "Resize":
            sc = np.asarray(i[2], np.float64).ravel()
            s = [float(np.float32(sc[2])), float(np.float32(sc[3]))]
            out = (int(np.floor(i[0].shape[2] * s[0])), int(np.floor(i[0].shape[3] * s[1])))
            y = seg_ref.resize_ref(i[0], out, s, _s(a.get("mode", "nearest")), _s(a.get("coordinate_transformation_mode", "half_pixel")),
                                   _s(a.get("nearest_mode", "round_prefer_floor")))
        else:
            raise NotImplementedError(op)
        if round_half and np.asarray(y).dtype.kind == "f":
            y = np.asarray(y, np.float64).astype(np.float16).astype(np.float64)
        env[n.outputs[0]] = y
    return {name: np.asarray(env[name], np.float64) for name, _, _ in m.outputs}
