"""Float64 reference for the transposed-convolution tests (ConvTranspose, U-Net): a torch-CPU walk of an ONNX graph in double precision, an
independent numpy restatement of the ONNX ConvTranspose definition (a scatter; also what the walk uses for asymmetric pads, which torch cannot
express), and the im2col form of the same op, which the per-element bound of tests/kernel_ref.py is computed on.

Decoding is the oracle's own reader (O.load_model).  Operators: those of models.unet and the random test graphs -- Conv, ConvTranspose,
BatchNormalization, Relu, Sigmoid, Concat, MaxPool, Resize, Identity, Dropout.  Resize is seg_ref's numpy restatement.
"""
from __future__ import annotations

import numpy as np

import kernel_ref as R
import seg_ref
from oracle import onnx_oracle as O

rel_err = seg_ref.rel_err


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


def convt_im2col(x, w, strides=(1, 1), pads=(0, 0, 0, 0), output_padding=(0, 0)):
    """The same op as an ordinary stride-1 convolution: kernel_ref.im2col of the zero-stuffed input (s - 1 zeros between neighbours) with pads
    k - 1 - p (plus output_padding at the bottom / right) against the spatially flipped, channel-swapped weights.  Needs pads < k.
    -> (cols [M, K], wm [Cout, K], (N, OH, OW)) in x's and w's dtypes."""
    x, w = np.asarray(x), np.asarray(w)
    n, cin, h, wd = x.shape
    _, cout, kh, kw = w.shape
    sh, sw = strides
    assert pads[0] < kh and pads[2] < kh and pads[1] < kw and pads[3] < kw
    xs = np.zeros((n, cin, (h - 1) * sh + 1, (wd - 1) * sw + 1), x.dtype)
    xs[:, :, ::sh, ::sw] = x
    ip = (kh - 1 - pads[0], kw - 1 - pads[1], kh - 1 - pads[2] + output_padding[0], kw - 1 - pads[3] + output_padding[1])
    # kernel_ref.im2col takes one kernel extent per axis and one stride
    cols = R.im2col(xs, kh, kw, 1, ip)
    wf = np.ascontiguousarray(w[:, :, ::-1, ::-1].transpose(1, 0, 2, 3))          # [Cout, Cin, kh, kw], flipped
    oh, ow = convt_out_hw(h, wd, (kh, kw), strides, pads, output_padding)
    assert cols.shape[:3] == (n, oh, ow), (cols.shape, (n, oh, ow))
    return cols.reshape(-1, kh * kw * cin), R.wmat(wf), (n, oh, ow)


def convt_torch(x, w, bias=None, strides=(1, 1), pad=(0, 0), output_padding=(0, 0)) -> np.ndarray:
    """torch's double F.conv_transpose2d (symmetric pads only: pad = (rows, columns))"""
    import torch
    import torch.nn.functional as F
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))  # noqa: E731
    with torch.no_grad():
        return F.conv_transpose2d(t(x), t(w), t(bias), stride=tuple(strides), padding=tuple(pad), output_padding=tuple(output_padding)).numpy()


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
                y = F.conv2d(F.pad(i[0], (p[1], p[3], p[0], p[2])), i[1], i[2] if len(i) > 2 else None, stride=tuple(a.get("strides", [1, 1])),
                             dilation=tuple(a.get("dilations", [1, 1])), groups=a.get("group", 1))
            elif op == "ConvTranspose":
                p = a.get("pads", [0, 0, 0, 0])
                st, opad = tuple(a.get("strides", [1, 1])), tuple(a.get("output_padding", [0, 0]))
                b = i[2] if len(i) > 2 else None
                assert a.get("group", 1) == 1 and tuple(a.get("dilations", [1, 1])) == (1, 1)
                if p[0] == p[2] and p[1] == p[3]:
                    y = F.conv_transpose2d(i[0], i[1], b, stride=st, padding=(p[0], p[1]), output_padding=opad)
                else:
                    y = torch.from_numpy(convt_scatter(i[0].numpy(), i[1].numpy(), None if b is None else b.numpy(), st, tuple(p), opad))
            elif op == "BatchNormalization":
                y = F.batch_norm(i[0], i[3], i[4], i[1], i[2], False, 0.0, a.get("epsilon", 1e-5))
            elif op == "Relu":
                y = torch.relu(i[0])
            elif op == "Sigmoid":
                y = torch.sigmoid(i[0])
            elif op == "Concat":
                y = torch.cat(i, dim=a.get("axis", 1))
            elif op == "MaxPool":
                p = a.get("pads", [0, 0, 0, 0])
                y = F.max_pool2d(F.pad(i[0], (p[1], p[3], p[0], p[2]), value=-np.inf), tuple(a["kernel_shape"]), stride=tuple(a.get("strides", [1, 1])))
            elif op in ("Dropout", "Identity"):
                y = i[0]
            elif op == "Resize":
                assert m.opset >= 11
                s = np.asarray(i[2], np.float64).ravel()
                s = [float(np.float32(s[2])), float(np.float32(s[3]))]
                x = i[0]
                out = (int(np.floor(x.shape[2] * s[0])), int(np.floor(x.shape[3] * s[1])))
                mode = seg_ref._s(a.get("mode", "nearest"))
                y = torch.from_numpy(seg_ref.resize_ref(x.numpy(), out, s, mode, seg_ref._s(a.get("coordinate_transformation_mode", "half_pixel")),
                                                        seg_ref._s(a.get("nearest_mode", "round_prefer_floor"))))
            else:
                raise NotImplementedError(op)
            env[n.outputs[0]] = y
    return {name: env[name].numpy() for name, _, _ in m.outputs}
