"""Float64 reference for the BERT tests (integer inputs, embedding tables, the key mask): a numpy walk of an ONNX graph in double precision, in the
manner of tests/vit_ref.py, whose helpers it shares.  Decoding is the oracle's own reader (O.load_model).

On top of vit_ref's operators: Gather with integer activations (negative indices count from the end, as ONNX defines), Cast, Sub, Slice (constant
starts / ends / axes / steps), Tanh.  Integer feeds stay integers; everything floating-point is float64, float32 constants included -- so
finfo(float32).min * (1 - mask) is the exact product the graph asks for.
"""
from __future__ import annotations

import math

import numpy as np

import vit_ref
from oracle import onnx_oracle as O

rel_err = vit_ref.rel_err
softmax = vit_ref.softmax
layer_norm = vit_ref.layer_norm

_CAST = {1: np.float64, 6: np.int32, 7: np.int64, 9: np.bool_, 10: np.float64, 11: np.float64}


def gather(data, idx, axis: int = 0):
    idx = np.asarray(idx)
    n = data.shape[axis]
    if ((idx < -n) | (idx >= n)).any():
        raise IndexError("Gather index out of range")
    return np.take(data, np.where(idx < 0, idx + n, idx), axis=axis)


def run_f64(model_bytes: bytes, feeds: dict) -> dict:
    m = O.load_model(model_bytes)
    f64 = lambda v: np.asarray(v, np.float64) if np.asarray(v).dtype.kind == "f" else np.asarray(v)  # noqa: E731
    env = {k: f64(v) for k, v in m.inits.items()}
    env.update({k: f64(v) for k, v in feeds.items()})
    erf = np.vectorize(math.erf, otypes=[np.float64])
    for n in m.nodes:
        a = n.attrs
        i = [env[x] if x else None for x in n.inputs]
        op = n.op
        if op == "Constant":
            (k, v), = a.items()
            y = f64(np.asarray(v, np.int64 if k.startswith("value_int") else None))
        elif op == "Gather":
            y = gather(i[0], i[1], a.get("axis", 0))
        elif op == "Slice":
            starts, ends = [int(v) for v in i[1]], [int(v) for v in i[2]]
            axes = [int(v) for v in i[3]] if len(i) > 3 and i[3] is not None else list(range(len(starts)))
            steps = [int(v) for v in i[4]] if len(i) > 4 and i[4] is not None else [1] * len(starts)
            sl = [slice(None)] * i[0].ndim
            for s, e, ax, st in zip(starts, ends, axes, steps):
                sl[ax] = slice(s, e, st)
            y = i[0][tuple(sl)]
        elif op == "Cast":
            y = i[0].astype(_CAST[a["to"]])
        elif op == "Sub":
            y = i[0] - i[1]
        elif op == "Tanh":
            y = np.tanh(i[0])
        elif op == "Reshape":
            y = vit_ref.reshape(i[0], list(i[1]))
        elif op == "Transpose":
            y = i[0].transpose(*a["perm"])
        elif op == "Unsqueeze":
            axes = a["axes"] if "axes" in a else list(i[1])
            y = i[0]
            for ax in sorted(int(v) for v in axes):
                y = np.expand_dims(y, ax)
        elif op == "Softmax":
            y = softmax(i[0], a.get("axis", -1))
        elif op == "MatMul":
            y = np.matmul(i[0], i[1])
        elif op == "LayerNormalization":
            y = layer_norm(i[0], i[1], i[2] if len(i) > 2 and i[2] is not None else None, a.get("axis", -1), float(np.float32(a.get("epsilon", 1e-5))))
        elif op == "Erf":
            y = erf(i[0])
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
