"""Float64 reference for the segmentation tests (dilated convolutions, Resize / Upsample): a torch-CPU walk of an ONNX graph in double precision,
and a numpy restatement of the ONNX Resize formulas for every mode the engine accepts.

Decoding is the oracle's own reader (O.load_model).  Operators: those of FCN / DeepLabV3-ResNet50 and the random test graphs -- Conv (any
dilation), BatchNormalization, Relu, Add, Concat, MaxPool, GlobalAveragePool, Dropout, Identity, Resize, Upsample -- plus the int64 shape
arithmetic torch writes for an F.interpolate's sizes (Shape, Gather, Slice, Unsqueeze, Concat, Cast, Constant).
"""
from __future__ import annotations

import numpy as np

from oracle import onnx_oracle as O

COORDS = ("half_pixel", "pytorch_half_pixel", "align_corners", "asymmetric")
NEAREST = ("round_prefer_floor", "round_prefer_ceil", "floor", "ceil")


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


def _s(v):
    return v.decode() if isinstance(v, bytes) else v


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
            if op == "Constant":
                y = np.asarray(a["value_int"] if "value_int" in a else a["value"])
            elif op == "Shape":
                y = np.array(i[0].shape, np.int64)
            elif op == "Gather":
                y = np.asarray(i[0])[np.asarray(i[1])]
            elif op == "Slice":
                y = np.asarray(i[0])[int(np.asarray(i[1]).ravel()[0]):int(np.asarray(i[2]).ravel()[0])]
            elif op == "Unsqueeze":
                y = np.expand_dims(np.asarray(i[0]), tuple(a["axes"]))
            elif op == "Cast":
                y = np.asarray(i[0]).astype(np.int64)
            elif op == "Concat" and not torch.is_tensor(i[0]):
                y = np.concatenate([np.asarray(v).reshape(-1) for v in i])
            elif op == "Conv":
                p = a.get("pads", [0, 0, 0, 0])
                x = F.pad(i[0], (p[1], p[3], p[0], p[2]))
                y = F.conv2d(x, i[1], i[2] if len(i) > 2 else None, stride=tuple(a.get("strides", [1, 1])),
                             dilation=tuple(a.get("dilations", [1, 1])), groups=a.get("group", 1))
            elif op == "BatchNormalization":
                y = F.batch_norm(i[0], i[3], i[4], i[1], i[2], False, 0.0, a.get("epsilon", 1e-5))
            elif op == "Relu":
                y = torch.relu(i[0])
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
            elif op in ("Dropout", "Identity"):
                y = i[0]
            elif op in ("Resize", "Upsample"):
                x = i[0]
                legacy = op == "Upsample" or m.opset < 11
                mode = _s(a.get("mode", "nearest"))
                mode = "linear" if mode == "bilinear" else mode
                coord = "asymmetric" if legacy else _s(a.get("coordinate_transformation_mode", "half_pixel"))
                nearest = "floor" if legacy else _s(a.get("nearest_mode", "round_prefer_floor"))
                sc = i[1] if legacy else (i[2] if len(i) > 2 else None)
                sz = None if legacy else (i[3] if len(i) > 3 else None)
                h, w = x.shape[2], x.shape[3]
                if sc is not None and np.asarray(sc).size:
                    s = np.asarray(sc, np.float64).ravel()
                    s = [float(np.float32(s[2])), float(np.float32(s[3]))]
                    out = (int(np.floor(h * s[0])), int(np.floor(w * s[1])))
                else:
                    z = np.asarray(sz).ravel()
                    out = (int(z[2]), int(z[3]))
                    s = [out[0] / h, out[1] / w]
                y = torch.from_numpy(resize_ref(x.numpy(), out, s, mode, coord, nearest))
            else:
                raise NotImplementedError(op)
            env[n.outputs[0]] = y
    return {name: env[name].numpy() for name, _, _ in m.outputs}


def conv_macs(model_bytes: bytes, input_shape) -> dict:
    """Multiply-accumulates of every Conv at the given input shape ({node name: MACs}), walking shapes through the ops above"""
    m = O.load_model(model_bytes)
    shapes = {m.inputs[0][0]: tuple(input_shape)}
    macs = {}
    for n in m.nodes:
        a = n.attrs
        xs = shapes.get(n.inputs[0]) if n.inputs else None
        if n.op in ("Conv", "MaxPool"):
            if n.op == "Conv":
                co, cg, kh, kw = m.inits[n.inputs[1]].shape
            else:
                co, cg, (kh, kw) = xs[1], 0, a["kernel_shape"]
            d = a.get("dilations", [1, 1])
            p = a.get("pads", [0, 0, 0, 0])
            s = a.get("strides", [1, 1])
            oh = (xs[2] + p[0] + p[2] - ((kh - 1) * d[0] + 1)) // s[0] + 1
            ow = (xs[3] + p[1] + p[3] - ((kw - 1) * d[1] + 1)) // s[1] + 1
            if n.op == "Conv":
                macs[n.name] = xs[0] * co * oh * ow * cg * kh * kw
            shapes[n.outputs[0]] = (xs[0], co, oh, ow)
        elif n.op == "GlobalAveragePool":
            shapes[n.outputs[0]] = (xs[0], xs[1], 1, 1)
        elif n.op == "Concat" and xs is not None:
            ss = [shapes[x] for x in n.inputs]
            shapes[n.outputs[0]] = (ss[0][0], sum(q[1] for q in ss)) + tuple(ss[0][2:])
        elif n.op in ("Resize", "Upsample") and xs is not None:
            if len(n.inputs) > 3 and n.inputs[3] in m.inits:
                shapes[n.outputs[0]] = tuple(int(v) for v in np.asarray(m.inits[n.inputs[3]]).ravel())
            else:
                sc = np.asarray(m.inits[n.inputs[2] if len(n.inputs) > 2 else n.inputs[1]], np.float64).ravel()
                shapes[n.outputs[0]] = (xs[0], xs[1], int(np.floor(xs[2] * sc[2])), int(np.floor(xs[3] * sc[3])))
        elif xs is not None:
            shapes[n.outputs[0]] = xs
    return macs


def rel_err(y, ref) -> float:
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(y, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))
