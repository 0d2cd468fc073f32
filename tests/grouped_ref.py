"""Float64 reference for the grouped-convolution tests: a torch-CPU walk of an ONNX graph in double precision.

dw_ref.py and se_ref.py do not handle MaxPool, which ResNeXt's stem needs, so the ResNeXt / RegNet tests evaluate their graphs here.  Decoding
is the oracle's own reader (O.load_model); the operators covered are those of ResNeXt, RegNetX / RegNetY and the random grouped graphs: Conv
(any group), BatchNormalization, Relu, Sigmoid, Mul, Add, Concat, MaxPool, GlobalAveragePool, Flatten, Identity, Gemm.
"""
from __future__ import annotations

import numpy as np

from oracle import onnx_oracle as O


def run_f64(model_bytes: bytes, feeds: dict) -> dict:
    import torch
    import torch.nn.functional as F
    m = O.load_model(model_bytes)
    env = {k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in m.inits.items()}
    env.update({k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in feeds.items()})
    with torch.no_grad():
        for n in m.nodes:
            a = n.attrs
            i = [env[x] if x else None for x in n.inputs]
            op = n.op
            if op == "Conv":
                p = a.get("pads", [0, 0, 0, 0])
                x = F.pad(i[0], (p[1], p[3], p[0], p[2]))
                y = F.conv2d(x, i[1], i[2] if len(i) > 2 else None, stride=tuple(a.get("strides", [1, 1])),
                             dilation=tuple(a.get("dilations", [1, 1])), groups=a.get("group", 1))
            elif op == "BatchNormalization":
                y = F.batch_norm(i[0], i[3], i[4], i[1], i[2], False, 0.0, a.get("epsilon", 1e-5))
            elif op == "Relu":
                y = torch.relu(i[0])
            elif op == "Sigmoid":
                y = torch.sigmoid(i[0])
            elif op == "Mul":
                y = i[0] * i[1]
            elif op == "Add":
                y = i[0] + i[1]
            elif op == "Concat":
                y = torch.cat(i, dim=a.get("axis", 1))
            elif op == "MaxPool":
                p = a.get("pads", [0, 0, 0, 0])
                x = F.pad(i[0], (p[1], p[3], p[0], p[2]), value=-np.inf)
                y = F.max_pool2d(x, tuple(a["kernel_shape"]), stride=tuple(a.get("strides", [1, 1])))
            elif op == "GlobalAveragePool":
                y = i[0].mean(dim=(2, 3), keepdim=True)
            elif op == "Flatten":
                y = i[0].flatten(a.get("axis", 1))
            elif op == "Identity":
                y = i[0]
            elif op == "Gemm":
                A = i[0].t() if a.get("transA", 0) else i[0]
                Bm = i[1].t() if a.get("transB", 0) else i[1]
                y = a.get("alpha", 1.0) * (A @ Bm)
                if len(i) > 2 and i[2] is not None:
                    y = y + a.get("beta", 1.0) * i[2]
            else:
                raise NotImplementedError(op)
            env[n.outputs[0]] = y
    return {name: env[name].numpy() for name, _, _ in m.outputs}


def conv_macs(model_bytes: bytes, input_shape) -> int:
    """Multiply-accumulates of every Conv (Cin / group per output) and Gemm of the graph at the given input shape, walking shapes through the
    ops above (MaxPool included)."""
    m = O.load_model(model_bytes)
    shapes = {m.inputs[0][0]: tuple(input_shape)}
    macs = 0
    for n in m.nodes:
        a = n.attrs
        xs = shapes.get(n.inputs[0])
        if n.op in ("Conv", "MaxPool"):
            if n.op == "Conv":
                co, cg, kh, kw = m.inits[n.inputs[1]].shape
            else:
                co, cg, (kh, kw) = xs[1], 0, a["kernel_shape"]
            p = a.get("pads", [0, 0, 0, 0])
            s = a.get("strides", [1, 1])
            oh = (xs[2] + p[0] + p[2] - kh) // s[0] + 1
            ow = (xs[3] + p[1] + p[3] - kw) // s[1] + 1
            macs += xs[0] * co * oh * ow * cg * kh * kw
            shapes[n.outputs[0]] = (xs[0], co, oh, ow)
        elif n.op == "Gemm":
            w = m.inits[n.inputs[1]]
            nout = w.shape[0] if a.get("transB", 0) else w.shape[1]
            macs += xs[0] * xs[1] * nout
            shapes[n.outputs[0]] = (xs[0], nout)
        elif n.op == "GlobalAveragePool":
            shapes[n.outputs[0]] = (xs[0], xs[1], 1, 1)
        elif n.op == "Flatten":
            shapes[n.outputs[0]] = (xs[0], int(np.prod(xs[1:])))
        elif n.op == "Concat":
            ss = [shapes[x] for x in n.inputs]
            shapes[n.outputs[0]] = (ss[0][0], sum(q[1] for q in ss)) + tuple(ss[0][2:])
        elif n.op == "Mul":
            shapes[n.outputs[0]] = max(xs, shapes.get(n.inputs[1]), key=lambda q: int(np.prod(q)))
        else:
            shapes[n.outputs[0]] = xs
    return int(macs)


def rel_err(y, ref) -> float:
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(y, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))
