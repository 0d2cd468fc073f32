"""Float64 reference for the ConvNeXt tests (channels-last views, LayerNormalization, GELU): a torch-CPU walk of an ONNX graph in double
precision, in the style of tests/unet_ref.py.  Decoding is the oracle's own reader (O.load_model).

Operators: those of models.convnext and the small test graphs -- Conv, Transpose, LayerNormalization, Erf, Gelu, MatMul, Gemm, Add, Mul, Div,
Flatten, GlobalAveragePool, Concat, Identity.  LayerNormalization is written out from the ONNX definition (mean over the normalised axes, the
variance of the centred values, (x - mean) / sqrt(var + epsilon) * scale + B), not taken from F.layer_norm; ln_agrees_with_torch() checks the
two against each other.
"""
from __future__ import annotations

import numpy as np

import seg_ref
from oracle import onnx_oracle as O

rel_err = seg_ref.rel_err
_s = seg_ref._s


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
    import torch
    import torch.nn.functional as F
    st = np.random.RandomState(11)
    x, g, b = 3.0 + st.randn(2, 3, 5, 24), st.randn(24), st.randn(24)
    t = F.layer_norm(torch.from_numpy(x), (24,), torch.from_numpy(g), torch.from_numpy(b), 1e-6).numpy()
    return float(np.abs(layer_norm(x, g, b, -1, 1e-6) - t).max())


def gelu(x, approximate: str = "none"):
    import torch
    if approximate == "tanh":
        return 0.5 * x * (1.0 + torch.tanh(np.sqrt(2.0 / np.pi) * (x + 0.044715 * x ** 3)))
    return 0.5 * x * (1.0 + torch.erf(x / np.sqrt(2.0)))


def depthwise_s1(x, w, bias, pads):
    """stride-1 depthwise conv from its definition: the sum over the taps of the shifted, per-channel weighted input.  x [N, C, H, W] and
    w [C, 1, kh, kw] double tensors, pads = (top, left, bottom, right)"""
    import torch.nn.functional as F
    kh, kw = w.shape[2], w.shape[3]
    xp = F.pad(x, (pads[1], pads[3], pads[0], pads[2]))
    oh, ow = xp.shape[2] - kh + 1, xp.shape[3] - kw + 1
    y = 0
    for ky in range(kh):
        for kx in range(kw):
            y = y + xp[:, :, ky:ky + oh, kx:kx + ow] * w[:, 0, ky, kx].reshape(1, -1, 1, 1)
    return y if bias is None else y + bias.reshape(1, -1, 1, 1)


def run_f64(model_bytes: bytes, feeds: dict) -> dict:
    import torch
    import torch.nn.functional as F
    m = O.load_model(model_bytes)
    env = {k: (torch.from_numpy(np.asarray(v, np.float64)) if np.asarray(v).dtype.kind == "f" else np.asarray(v)) for k, v in m.inits.items()}
    env.update({k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in feeds.items()})
    with torch.no_grad():
        for n in m.nodes:
            a = n.attrs
            i = [env[x] if x else None for x in n.inputs]
            op = n.op
            if op == "Conv":
                p = a.get("pads", [0, 0, 0, 0])
                if a.get("group", 1) == i[0].shape[1] == i[1].shape[0] and i[1].shape[1] == 1 and tuple(a.get("strides", [1, 1])) == (1, 1):
                    y = depthwise_s1(i[0], i[1], i[2] if len(i) > 2 else None, p)      # (torch's grouped double conv is ~20x slower)
                else:
                    y = F.conv2d(F.pad(i[0], (p[1], p[3], p[0], p[2])), i[1], i[2] if len(i) > 2 else None, stride=tuple(a.get("strides", [1, 1])),
                                 dilation=tuple(a.get("dilations", [1, 1])), groups=a.get("group", 1))
            elif op == "Transpose":
                y = i[0].permute(*a["perm"]).contiguous()
            elif op == "LayerNormalization":
                y = torch.from_numpy(layer_norm(i[0].numpy(), i[1].numpy(), i[2].numpy() if len(i) > 2 and i[2] is not None else None,
                                                a.get("axis", -1), float(np.float32(a.get("epsilon", 1e-5)))))
            elif op == "Erf":
                y = torch.erf(i[0])
            elif op == "Gelu":
                y = gelu(i[0], _s(a.get("approximate", "none")))
            elif op == "MatMul":
                y = torch.matmul(i[0], i[1])
            elif op == "Gemm":
                A = i[0].t() if a.get("transA", 0) else i[0]
                Bm = i[1].t() if a.get("transB", 0) else i[1]
                y = a.get("alpha", 1.0) * (A @ Bm)
                if len(i) > 2 and i[2] is not None:
                    y = y + a.get("beta", 1.0) * i[2]
            elif op == "Add":
                y = i[0] + i[1]
            elif op == "Mul":
                y = i[0] * i[1]
            elif op == "Div":
                y = i[0] / i[1]
            elif op == "Flatten":
                ax = a.get("axis", 1)
                y = i[0].reshape(int(np.prod(i[0].shape[:ax])), -1)
            elif op == "GlobalAveragePool":
                y = i[0].mean(dim=(2, 3), keepdim=True)
            elif op == "Concat":
                y = torch.cat(i, dim=a.get("axis", 1))
            elif op == "Identity":
                y = i[0]
            else:
                raise NotImplementedError(op)
            env[n.outputs[0]] = y
    return {name: env[name].numpy() for name, _, _ in m.outputs}
