"""Synthetic ONNX model builders (DenseNet-121, ResNet-50, ResNeXt-50, MobileNetV2, MobileNetV3, EfficientNet-B0, RegNetX / RegNetY,
FCN-ResNet50, DeepLabV3-ResNet50, U-Net, ConvNeXt, ViT, Swin, BERT, GPT-2, GroupNorm ResNets, the diffusion VAE decoder and small test graphs).

The reference's `models/densenet_onnx/1/model.onnx` is not in the mount (.MISSING_LARGE_BLOBS:1), so the
benchmark model is rebuilt from its I/O contract (`models/densenet_onnx/1/config.json:5-20`: input `data_0`
[N,3,224,224] FLOAT32 -> output `fc6_1` [N,1000,1,1]) and the published DenseNet-121 architecture
(growth 32, blocks 6/12/24/16, stem 64, bottleneck 4*growth, final 1x1 conv 1024->1000 like the
Caffe-derived model-zoo file).  Weights come from the counter-based RNG in rng.py (seed 121).

`test_model()` rebuilds the reference's 543-byte MLP (scripts/create-test-model.py:25-29: weights are
`np.random.seed(42)` randn draws in the order weight1, bias1, weight2, bias2).
"""
from __future__ import annotations

import os
from typing import Sequence

import numpy as np

from . import onnx_pb as pb
from . import rng


class GraphBuilder:
    def __init__(self, name: str, seed: int):
        self.name = name
        self.seed = seed
        self.nodes: list[bytes] = []
        self.inits: list[bytes] = []
        self.n = 0

    def _uid(self, base: str) -> str:
        self.n += 1
        return f"{base}_{self.n}"

    def init(self, name: str, arr: np.ndarray, raw: bool = True) -> str:
        self.inits.append(pb.tensor(name, arr, raw=raw))
        return name

    # ---- ops ----
    def conv(self, x: str, cin: int, cout: int, k: int, stride: int = 1, pad: int | Sequence[int] = 0, bias: bool = False,
             name: str | None = None, w_scale: float | None = None, group: int = 1, dilation: int = 1, out: str | None = None) -> str:
        """pad: one value for all four sides or ONNX order [top, left, bottom, right]; out: the result's name (default: name + "_out")"""
        name = name or self._uid("conv")
        cg = cin // group                       # input channels per group (1 for a depthwise conv)
        fan_in = cg * k * k
        std = w_scale if w_scale is not None else float(np.sqrt(2.0 / fan_in))
        w = rng.gaussish(self.seed, name + "_w", cout * cg * k * k).reshape(cout, cg, k, k) * np.float32(std)
        ins = [x, self.init(name + "_w", w.astype(np.float32))]
        if bias:
            b = (rng.uniform(self.seed, name + "_b", cout) - np.float32(0.5)) * np.float32(0.2)
            ins.append(self.init(name + "_b", b.astype(np.float32)))
        y = out or name + "_out"
        self.nodes.append(pb.node("Conv", ins, [y], name, [
            pb.attr_ints("dilations", [dilation, dilation]), pb.attr_int("group", group),
            pb.attr_ints("kernel_shape", [k, k]), pb.attr_ints("pads", [pad] * 4 if isinstance(pad, int) else list(pad)),
            pb.attr_ints("strides", [stride, stride])]))
        return y

    def conv_transpose(self, x: str, cin: int, cout: int, k: int | Sequence[int], stride: int | Sequence[int], pad: int | Sequence[int] = 0,
                       output_padding: int | Sequence[int] = 0, bias: bool = False, name: str | None = None) -> str:
        """ONNX ConvTranspose, weights [cin, cout, kh, kw].  k, stride, output_padding: one value or [h, w]; pad: one value for all four sides or
        ONNX order [top, left, bottom, right].  The same named rng streams as conv()."""
        name = name or self._uid("convt")
        kh, kw = (k, k) if isinstance(k, int) else k
        sh, sw = (stride, stride) if isinstance(stride, int) else stride
        oph, opw = (output_padding, output_padding) if isinstance(output_padding, int) else output_padding
        # every output pixel sums about cin * kh * kw / (sh * sw) products
        std = float(np.sqrt(2.0 * sh * sw / (cin * kh * kw)))
        w = rng.gaussish(self.seed, name + "_w", cin * cout * kh * kw).reshape(cin, cout, kh, kw) * np.float32(std)
        ins = [x, self.init(name + "_w", w.astype(np.float32))]
        if bias:
            b = (rng.uniform(self.seed, name + "_b", cout) - np.float32(0.5)) * np.float32(0.2)
            ins.append(self.init(name + "_b", b.astype(np.float32)))
        y = name + "_out"
        attrs = [pb.attr_ints("dilations", [1, 1]), pb.attr_int("group", 1), pb.attr_ints("kernel_shape", [kh, kw])]
        if oph or opw:
            attrs.append(pb.attr_ints("output_padding", [oph, opw]))
        attrs += [pb.attr_ints("pads", [pad] * 4 if isinstance(pad, int) else list(pad)), pb.attr_ints("strides", [sh, sw])]
        self.nodes.append(pb.node("ConvTranspose", ins, [y], name, attrs))
        return y

    def clip(self, x: str, lo: float | None = 0.0, hi: float | None = 6.0, form: str = "initializer") -> str:
        """ONNX Clip in the forms exporters write (None = that bound absent):
          "attrs"        min / max attributes (opset < 11: build the model with finish(..., opset=6))
          "initializer"  scalar initializers as inputs 2 / 3 (opset >= 11; an absent min is the empty input name "")
          "constant"     the same inputs produced by Constant nodes
        """
        name = self._uid("clip")
        y = name + "_out"
        if form == "attrs":
            attrs = ([pb.attr_float("min", lo)] if lo is not None else []) + ([pb.attr_float("max", hi)] if hi is not None else [])
            self.nodes.append(pb.node("Clip", [x], [y], name, attrs))
            return y
        ins = [x]
        for tag, v in (("min", lo), ("max", hi)):
            if v is None:
                ins.append("")
            elif form == "initializer":
                ins.append(self.init(f"{name}_{tag}", np.array(v, np.float32)))
            elif form == "constant":
                self.nodes.append(pb.node("Constant", [], [f"{name}_{tag}"], f"{name}_{tag}_const",
                                          [pb.attr_tensor("value", np.array(v, np.float32))]))
                ins.append(f"{name}_{tag}")
            else:
                raise ValueError(form)
        while ins[-1] == "":
            ins.pop()
        self.nodes.append(pb.node("Clip", ins, [y], name))
        return y

    def bn(self, x: str, c: int, name: str | None = None, eps: float = 1e-5, g_center: float = 1.0) -> str:
        name = name or self._uid("bn")
        g = np.float32(g_center) + (rng.uniform(self.seed, name + "_g", c) - np.float32(0.5)) * np.float32(0.2)
        b = (rng.uniform(self.seed, name + "_b", c) - np.float32(0.5)) * np.float32(0.2)
        m = (rng.uniform(self.seed, name + "_m", c) - np.float32(0.5)) * np.float32(0.2)
        v = np.float32(0.5) + rng.uniform(self.seed, name + "_v", c)
        ins = [x] + [self.init(f"{name}_{s}", a.astype(np.float32)) for s, a in
                     (("scale", g), ("B", b), ("mean", m), ("var", v))]
        y = name + "_out"
        self.nodes.append(pb.node("BatchNormalization", ins, [y], name,
                                  [pb.attr_float("epsilon", eps), pb.attr_float("momentum", 0.9)]))
        return y

    def relu(self, x: str) -> str:
        name = self._uid("relu")
        self.nodes.append(pb.node("Relu", [x], [name + "_out"], name))
        return name + "_out"

    # ---- activations (MobileNetV3 / EfficientNet) ----
    def sigmoid(self, x: str) -> str:
        return self.simple("Sigmoid", [x])

    def hardsigmoid(self, x: str, alpha: float = 0.2, beta: float = 0.5) -> str:
        return self.simple("HardSigmoid", [x], [pb.attr_float("alpha", alpha), pb.attr_float("beta", beta)])

    def hardswish(self, x: str, form: str = "op") -> str:
        """x * hardsigmoid(x; 1/6, 1/2) in the forms exporters write:
          "op"               the HardSwish operator (opset >= 14)
          "hardsigmoid_mul"  Mul(x, HardSigmoid(x))  (torch's export below opset 14)
          "mul_hardsigmoid"  Mul(HardSigmoid(x), x)  (the same, operands swapped)
        """
        if form == "op":
            return self.simple("HardSwish", [x])
        g = self.hardsigmoid(x, 1.0 / 6.0, 0.5)
        if form == "hardsigmoid_mul":
            return self.simple("Mul", [x, g])
        if form == "mul_hardsigmoid":
            return self.simple("Mul", [g, x])
        raise ValueError(form)

    def silu(self, x: str, swap: bool = False) -> str:
        """SiLU as exporters write it: Mul(x, Sigmoid(x)) (swap: Mul(Sigmoid(x), x))."""
        g = self.sigmoid(x)
        return self.simple("Mul", [g, x] if swap else [x, g])

    # ---- ConvNeXt: channels-last views, layer norm, GELU, Linear ----
    def transpose(self, x: str, perm: Sequence[int]) -> str:
        return self.simple("Transpose", [x], [pb.attr_ints("perm", list(perm))])

    def layernorm(self, x: str, c: int, eps: float = 1e-6, axis: int = -1, name: str | None = None, bias: bool = True) -> str:
        """LayerNormalization-17 over the trailing axes from `axis`; scale / B are [c] initializers around 1 / 0."""
        name = name or self._uid("ln")
        g = np.float32(1.0) + (rng.uniform(self.seed, name + "_g", c) - np.float32(0.5)) * np.float32(0.2)
        ins = [x, self.init(name + "_scale", g.astype(np.float32))]
        if bias:
            b = (rng.uniform(self.seed, name + "_b", c) - np.float32(0.5)) * np.float32(0.2)
            ins.append(self.init(name + "_B", b.astype(np.float32)))
        y = name + "_out"
        self.nodes.append(pb.node("LayerNormalization", ins, [y], name, [pb.attr_int("axis", axis), pb.attr_float("epsilon", eps)]))
        return y

    def rmsnorm(self, x: str, c: int, eps: float = 1e-5, form: str = "pow", name: str | None = None, *, cast: bool = False, swap: bool = False,
                axes_input: bool = True, axis: int = -1, g: np.ndarray | None = None, out: str | None = None) -> str:
        """RMSNorm over the last axis, weight * (x * rsqrt(mean(x^2) + eps)), in the forms exporters write (HF's LlamaRMSNorm):
          "pow"         Pow(x, 2) -> ReduceMean(axes [-1], keepdims 1) -> Add eps -> Sqrt -> Div(1, .) -> Mul(x, .) -> Mul(weight, .)   (torch's rsqrt below opset 23)
          "mul"         the same with Mul(x, x) in place of the Pow
          "reciprocal"  the same with Reciprocal in place of Div(1, .);  "mul_reciprocal": both
          "op"          the opset-23 RMSNormalization operator (build the model with finish(..., opset=23))
        cast: the Cast(to = FLOAT) nodes of hidden_states.to(torch.float32) and of the cast back, on x and on the normalised value.  swap: every Mul /
        Add with its operands the other way round.  axes_input: the ReduceMean's axes as an input (opset >= 18), else as an attribute.  The weight [c]
        is drawn around 1 from the stream name_g (g: given instead)."""
        name = name or self._uid("rms")
        if g is None:
            g = np.float32(1.0) + (rng.uniform(self.seed, name + "_g", c) - np.float32(0.5)) * np.float32(0.2)
        w = self.init(name + "_weight", np.asarray(g, np.float32))
        y = out or name + "_out"
        if form == "op":
            self.nodes.append(pb.node("RMSNormalization", [x, w], [y], name, [pb.attr_int("axis", axis), pb.attr_float("epsilon", eps)]))
            return y
        if form not in ("pow", "mul", "reciprocal", "mul_reciprocal"):
            raise ValueError(form)
        two = lambda a, b: [b, a] if swap else [a, b]  # noqa: E731
        xf = self.simple("Cast", [x], [pb.attr_int("to", pb.FLOAT)]) if cast else x
        sq = self.simple("Mul", [xf, xf]) if form.startswith("mul") else self.simple("Pow", [xf, self.init(name + "_two", np.array(2.0, np.float32))])
        if axes_input:
            v = self.simple("ReduceMean", [sq, self.init(name + "_axes", np.array([axis], np.int64))], [pb.attr_int("keepdims", 1)])
        else:
            v = self.simple("ReduceMean", [sq], [pb.attr_ints("axes", [axis]), pb.attr_int("keepdims", 1)])
        r = self.simple("Sqrt", [self.simple("Add", two(v, self.init(name + "_eps", np.array(eps, np.float32))))])
        r = self.simple("Reciprocal", [r]) if form.endswith("reciprocal") else self.simple("Div", [self.init(name + "_one", np.array(1.0, np.float32)), r])
        h = self.simple("Mul", two(xf, r))
        if cast:
            h = self.simple("Cast", [h], [pb.attr_int("to", pb.FLOAT)])
        self.nodes.append(pb.node("Mul", two(w, h), [y], name + "_scale"))
        return y

    def swiglu(self, gate: str, up: str, act: str = "silu", swap: bool = False) -> str:
        """A gated unit, Mul(act(gate), up): act "silu" (Mul(x, Sigmoid(x)), SwiGLU as Llama's MLP writes it) or a GraphBuilder.gelu form (GeGLU).  swap:
        the operands of every Mul the other way round"""
        a = self.silu(gate, swap=swap) if act == "silu" else self.gelu(gate, act, swap=swap)
        return self.simple("Mul", [up, a] if swap else [a, up])

    def group_norm(self, x: str, c: int, groups: int, eps: float = 1e-5, form: str = "instancenorm", back: str = "const", rank3: bool = False,
                   *, hw: Sequence[int] | None = None, name: str | None = None, swap: bool = False, affine: bool = True, per_group: bool = False,
                   inner: str = "ones", out: str | None = None) -> str:
        """GroupNorm of x [N, c, H, W] (rank3: of its [N, c, H*W] reshape) in the forms exporters write:
          "instancenorm"  torch below opset 18: Reshape [0, groups, -1] -> InstanceNormalization(ones [groups], zeros [groups]) -> Reshape back ->
                          Mul(gamma [c, 1, 1]) -> Add(beta [c, 1, 1]) ([c, 1] for rank3).  back: "const" the constant [0, c, H, W] (needs hw = (H, W)) or
                          "shape" Shape(x), as the exporter writes it.  swap: the constants first.  affine False: no Mul / Add.
                          inner "random": scale and B of the InstanceNormalization are drawn, not ones and zeros (a test of their folding)
          "op18"          GroupNormalization with scale / bias [groups] (opset 18: build the model with finish(..., opset=18))
          "op21"          GroupNormalization with scale / bias [c] (opset 21)
          "instance"      InstanceNormalization directly on x with scale / B [c] (groups must equal c)
        gamma and beta are drawn around 1 and 0 from the streams name_g / name_b; per_group (always for "op18"): one draw per group, repeated over its
        channels, so that every form describes the same function."""
        name = name or self._uid("gn")
        k = groups if (per_group or form == "op18") else c
        g = np.float32(1.0) + (rng.uniform(self.seed, name + "_g", k) - np.float32(0.5)) * np.float32(0.2)
        b = (rng.uniform(self.seed, name + "_b", k) - np.float32(0.5)) * np.float32(0.2)
        y = out or name + "_out"
        if form in ("op18", "op21"):
            if form == "op21" and k != c:
                g, b = np.repeat(g, c // groups), np.repeat(b, c // groups)
            ins = [x, self.init(name + "_scale", g.astype(np.float32)), self.init(name + "_bias", b.astype(np.float32))]
            self.nodes.append(pb.node("GroupNormalization", ins, [y], name, [pb.attr_float("epsilon", eps), pb.attr_int("num_groups", groups)]))
            return y
        if k != c:
            g, b = np.repeat(g, c // groups), np.repeat(b, c // groups)
        if form == "instance":
            assert groups == c
            ins = [x, self.init(name + "_scale", g.astype(np.float32)), self.init(name + "_B", b.astype(np.float32))]
            self.nodes.append(pb.node("InstanceNormalization", ins, [y], name, [pb.attr_float("epsilon", eps)]))
            return y
        if form != "instancenorm":
            raise ValueError(form)
        r1 = name + "_r1"
        self.nodes.append(pb.node("Reshape", [x, self.init(name + "_shape1", np.array([0, groups, -1], np.int64))], [r1], r1))
        if inner == "ones":
            si, bi = np.ones(groups, np.float32), np.zeros(groups, np.float32)
        else:
            si = np.float32(1.0) + (rng.uniform(self.seed, name + "_is", groups) - np.float32(0.5))
            bi = rng.uniform(self.seed, name + "_ib", groups) - np.float32(0.5)
        ino = name + "_in"
        self.nodes.append(pb.node("InstanceNormalization", [r1, self.init(name + "_in_scale", si.astype(np.float32)), self.init(name + "_in_B", bi.astype(np.float32))],
                                  [ino], ino, [pb.attr_float("epsilon", eps)]))
        if back == "const":
            shp = self.init(name + "_shape2", np.array([0, c, hw[0] * hw[1]] if rank3 else [0, c, hw[0], hw[1]], np.int64))
        elif back == "shape":
            shp = name + "_xshape"
            self.nodes.append(pb.node("Shape", [x], [shp], shp))
        else:
            raise ValueError(back)
        r2 = name + "_r2" if affine else y
        self.nodes.append(pb.node("Reshape", [ino, shp], [r2], name + "_r2"))
        if not affine:
            return y
        tail = [c, 1] if rank3 else [c, 1, 1]
        gi, bi2 = self.init(name + "_gamma", g.astype(np.float32).reshape(tail)), self.init(name + "_beta", b.astype(np.float32).reshape(tail))
        mu = name + "_mul"
        self.nodes.append(pb.node("Mul", [gi, r2] if swap else [r2, gi], [mu], mu))
        self.nodes.append(pb.node("Add", [bi2, mu] if swap else [mu, bi2], [y], name + "_add"))
        return y

    def gelu(self, x: str, form: str = "erf", swap: bool = False, half: float = 0.5) -> str:
        """GELU in the forms exporters write:
          "erf"      Div(x, sqrt 2) -> Erf -> Add 1 -> Mul(x, .) -> Mul(., 0.5)   (torch below opset 20; swap: both Mul operand orders reversed)
          "erf_mul"  the same with Mul(x, 1 / sqrt 2) in place of the Div
          "op"       the opset-20 Gelu operator, approximate = "none";  "op_tanh": approximate = "tanh"
        half: the last constant (0.5 for a GELU; tests write near misses)."""
        if form in ("op", "op_tanh"):
            return self.simple("Gelu", [x], [pb.attr_str("approximate", "tanh" if form == "op_tanh" else "none")])
        name = self._uid("gelu")
        if form == "erf":
            y = self.simple("Div", [x, self.init(name + "_sqrt2", np.array(np.sqrt(2.0), np.float32))])
        elif form == "erf_mul":
            y = self.simple("Mul", [x, self.init(name + "_rsqrt2", np.array(1.0 / np.sqrt(2.0), np.float32))])
        else:
            raise ValueError(form)
        y = self.simple("Add", [self.simple("Erf", [y]), self.init(name + "_one", np.array(1.0, np.float32))])
        y = self.simple("Mul", [y, x] if swap else [x, y])
        h = self.init(name + "_half", np.array(half, np.float32))
        return self.simple("Mul", [h, y] if swap else [y, h])

    def linear(self, x: str, cin: int, cout: int, name: str | None = None, w_scale: float | None = None, bias: bool = True) -> str:
        """torch's Linear on a [..., cin] tensor as the exporter writes it: MatMul with a [cin, cout] initializer, then Add [cout] (bias False: the
        MatMul alone, as Llama's projections are)."""
        name = name or self._uid("fc")
        std = w_scale if w_scale is not None else float(np.sqrt(1.0 / cin))
        w = rng.gaussish(self.seed, name + "_w", cin * cout).reshape(cin, cout) * np.float32(std)
        y = self.simple("MatMul", [x, self.init(name + "_w", w.astype(np.float32))])
        if not bias:
            return y
        b = (rng.uniform(self.seed, name + "_b", cout) - np.float32(0.5)) * np.float32(0.2)
        return self.simple("Add", [y, self.init(name + "_b", b.astype(np.float32))])

    def act(self, x: str, kind: str, form: str = "op") -> str:
        """kind: relu | hardswish | silu | sigmoid | hardsigmoid | relu6 | none"""
        if kind == "relu":
            return self.relu(x)
        if kind == "hardswish":
            return self.hardswish(x, form)
        if kind == "silu":
            return self.silu(x, swap=form == "mul_hardsigmoid")
        if kind == "sigmoid":
            return self.sigmoid(x)
        if kind == "hardsigmoid":
            return self.hardsigmoid(x, 1.0 / 6.0, 0.5)
        if kind == "relu6":
            return self.clip(x, 0.0, 6.0)
        if kind == "none":
            return x
        raise ValueError(kind)

    def se(self, x: str, c: int, mid: int, act1: str = "relu", gate: str = "hardsigmoid", name: str | None = None, swap: bool = False,
           form: str = "op") -> str:
        """Squeeze-and-excitation: GlobalAveragePool -> Conv1x1(+bias) C -> mid -> act1 -> Conv1x1(+bias) mid -> C -> gate -> Mul(x, gate)
        (swap: Mul(gate, x))."""
        name = name or self._uid("se")
        s = self.gap(x)
        s = self.act(self.conv(s, c, mid, 1, bias=True, name=name + "_fc1", w_scale=float(np.sqrt(1.0 / c))), act1, form)
        s = self.act(self.conv(s, mid, c, 1, bias=True, name=name + "_fc2", w_scale=float(np.sqrt(1.0 / mid))), gate, form)
        return self.simple("Mul", [s, x] if swap else [x, s])

    def resize(self, x: str, in_shape: Sequence[int], *, sizes: Sequence[int] | None = None, scales: Sequence[float] | None = None,
               mode: str = "linear", coord: str = "pytorch_half_pixel", nearest: str | None = None, form: str = "sizes", opset: int = 11,
               name: str | None = None, out: str | None = None) -> str:
        """ONNX Resize of a 4-D tensor of `in_shape` to `sizes` [H, W] or by `scales` [sh, sw], in the forms exporters write:
        form "scales": Resize(x, roi "", scales [1, 1, sh, sw]); "sizes": Resize(x, "", "", sizes [N, C, H, W]) (a concrete batch);
        "shape": the sizes as torch exports them -- Shape(x) -> Gather(0), Gather(1) -> Unsqueeze -> Concat with [H, W] -> Cast;
        "upsample": Upsample-9 (x, scales), asymmetric.  opset 10: Resize(x, scales), asymmetric."""
        name = name or self._uid("resize")
        attrs = [pb.attr_str("mode", mode)]
        if form != "upsample" and opset >= 11:
            attrs.append(pb.attr_str("coordinate_transformation_mode", coord))
            if nearest is not None:
                attrs.append(pb.attr_str("nearest_mode", nearest))
        y = out or name + "_out"
        if form in ("scales", "upsample") or opset < 11:
            sc = self.init(name + "_scales", np.array([1.0, 1.0, *scales], np.float32))
            ins = [x, sc] if (form == "upsample" or opset < 11) else [x, "", sc]
            self.nodes.append(pb.node("Upsample" if form == "upsample" else "Resize", ins, [y], name, attrs))
            return y
        if form == "sizes":
            sz = self.init(name + "_sizes", np.array([in_shape[0], in_shape[1], *sizes], np.int64))
        elif form == "shape":
            self.nodes.append(pb.node("Shape", [x], [name + "_shape"], name + "_shape"))
            parts = []
            for i in (0, 1):
                idx = name + f"_i{i}"            # a scalar index (a Constant node: initializers here are at least 1-D)
                self.nodes.append(pb.node("Constant", [], [idx], idx, [pb.attr_int("value_int", i)]))
                self.nodes.append(pb.node("Gather", [name + "_shape", idx], [name + f"_g{i}"], name + f"_g{i}", [pb.attr_int("axis", 0)]))
                self.nodes.append(pb.node("Unsqueeze", [name + f"_g{i}"], [name + f"_u{i}"], name + f"_u{i}", [pb.attr_ints("axes", [0])]))
                parts.append(name + f"_u{i}")
            hw = self.init(name + "_hw", np.array(list(sizes), np.int64))
            self.nodes.append(pb.node("Concat", [*parts, hw], [name + "_cat"], name + "_cat", [pb.attr_int("axis", 0)]))
            self.nodes.append(pb.node("Cast", [name + "_cat"], [name + "_sizes"], name + "_cast", [pb.attr_int("to", 7)]))
            sz = name + "_sizes"
        else:
            raise ValueError(form)
        self.nodes.append(pb.node("Resize", [x, "", "", sz], [y], name, attrs))
        return y

    def concat(self, xs: Sequence[str], axis: int = 1) -> str:
        name = self._uid("concat")
        self.nodes.append(pb.node("Concat", xs, [name + "_out"], name, [pb.attr_int("axis", axis)]))
        return name + "_out"

    def pool(self, op: str, x: str, k: int, stride: int, pad: int = 0, extra: Sequence[bytes] = ()) -> str:
        name = self._uid(op.lower())
        self.nodes.append(pb.node(op, [x], [name + "_out"], name, [
            pb.attr_ints("kernel_shape", [k, k]), pb.attr_ints("pads", [pad] * 4),
            pb.attr_ints("strides", [stride, stride]), *extra]))
        return name + "_out"

    def gap(self, x: str) -> str:
        name = self._uid("gap")
        self.nodes.append(pb.node("GlobalAveragePool", [x], [name + "_out"], name))
        return name + "_out"

    def simple(self, op: str, xs: Sequence[str], attrs: Sequence[bytes] = (), out: str | None = None) -> str:
        name = self._uid(op.lower())
        y = out or name + "_out"
        self.nodes.append(pb.node(op, xs, [y], name, attrs))
        return y

    def finish(self, inputs: Sequence[tuple], outputs: Sequence[tuple], opset: int = 11) -> bytes:
        """inputs / outputs: (name, shape) or (name, shape, ONNX element type); FLOAT where it is not given"""
        g = pb.graph(self.name, self.nodes, self.inits,
                     [pb.value_info(*t) for t in inputs], [pb.value_info(*t) for t in outputs])
        return pb.model(g, opset=opset)


def densenet(batch: int | str = 1, *, growth: int = 32, blocks: Sequence[int] = (6, 12, 24, 16),
             stem: int = 64, bn_size: int = 4, image: int = 224, classes: int = 1000, seed: int = 121,
             in_name: str = "data_0", out_name: str = "fc6_1", caffe_scale: bool | str = False) -> bytes:
    """DenseNet-BC-style graph (DenseNet-121 with the defaults).

    caffe_scale follows each BatchNormalization with the Mul+Add of a Caffe Scale layer (SURVEY.md §2.3 last row), in the three
    forms exporters of the model-zoo Caffe2 DenseNet-121 produce:
      True            [C,1,1] initializers, numpy broadcasting
      "unsqueeze"     [C] initializers routed through Unsqueeze(axes=[1,2]) nodes (opset >= 7 exports)
      "legacy_axis"   [C] initializers with the opset-6 attributes broadcast=1, axis=1 (the whole model is then opset 6)
    """
    gb = GraphBuilder("densenet", seed)

    def norm(x: str, c: int) -> str:
        y = gb.bn(x, c)
        if caffe_scale:
            nm = gb._uid("scale")
            s = np.float32(1.0) + (rng.uniform(seed, nm + "_s", c) - np.float32(0.5)) * np.float32(0.1)
            t = (rng.uniform(seed, nm + "_t", c) - np.float32(0.5)) * np.float32(0.1)
            if caffe_scale == "unsqueeze":
                su = gb.simple("Unsqueeze", [gb.init(nm + "_s", s)], [pb.attr_ints("axes", [1, 2])])
                tu = gb.simple("Unsqueeze", [gb.init(nm + "_t", t)], [pb.attr_ints("axes", [1, 2])])
                y = gb.simple("Mul", [y, su])
                y = gb.simple("Add", [y, tu])
            elif caffe_scale == "legacy_axis":
                legacy = [pb.attr_int("axis", 1), pb.attr_int("broadcast", 1)]
                y = gb.simple("Mul", [y, gb.init(nm + "_s", s)], legacy)
                y = gb.simple("Add", [y, gb.init(nm + "_t", t)], legacy)
            else:
                y = gb.simple("Mul", [y, gb.init(nm + "_s", s.reshape(c, 1, 1))])
                y = gb.simple("Add", [y, gb.init(nm + "_t", t.reshape(c, 1, 1))])
        return y

    x = gb.conv(in_name, 3, stem, 7, stride=2, pad=3, name="conv1")
    x = gb.relu(norm(x, stem))
    x = gb.pool("MaxPool", x, 3, 2, 1)
    c = stem
    for bi, nl in enumerate(blocks):
        for _ in range(nl):
            y = gb.relu(norm(x, c))
            y = gb.conv(y, c, bn_size * growth, 1)
            y = gb.relu(norm(y, bn_size * growth))
            y = gb.conv(y, bn_size * growth, growth, 3, pad=1)
            x = gb.concat([x, y])
            c += growth
        if bi != len(blocks) - 1:
            y = gb.relu(norm(x, c))
            y = gb.conv(y, c, c // 2, 1)
            x = gb.pool("AveragePool", y, 2, 2, 0)
            c //= 2
    x = gb.relu(norm(x, c))
    x = gb.gap(x)
    # Final classifier as a 1x1 conv with bias so the output is [N, classes, 1, 1]
    # (models/densenet_onnx/1/config.json:17).  Smaller init keeps logits O(1).
    fc = "fc6"
    w = rng.gaussish(seed, fc + "_w", classes * c).reshape(classes, c, 1, 1) * np.float32(np.sqrt(1.0 / c))
    b = (rng.uniform(seed, fc + "_b", classes) - np.float32(0.5)) * np.float32(0.2)
    gb.nodes.append(pb.node("Conv", [x, gb.init(fc + "_w", w.astype(np.float32)), gb.init(fc + "_b", b)],
                            [out_name], fc, [pb.attr_ints("kernel_shape", [1, 1]), pb.attr_ints("pads", [0] * 4),
                                             pb.attr_ints("strides", [1, 1]), pb.attr_int("group", 1),
                                             pb.attr_ints("dilations", [1, 1])]))
    return gb.finish([(in_name, [batch, 3, image, image])], [(out_name, [batch, classes, 1, 1])],
                     opset=6 if caffe_scale == "legacy_axis" else 11)


def densenet121(batch: int | str = 1) -> bytes:
    return densenet(batch)


def test_model() -> bytes:
    """Re-creation of the reference's test MLP (same initializer values, names and node order)."""
    st = np.random.RandomState(42)
    w1 = st.randn(3, 5).astype(np.float32)
    b1 = st.randn(5).astype(np.float32)
    w2 = st.randn(5, 2).astype(np.float32)
    b2 = st.randn(2).astype(np.float32)
    nodes = [pb.node("MatMul", ["input", "weight1"], ["matmul1"], "matmul1"),
             pb.node("Add", ["matmul1", "bias1"], ["hidden"], "add1"),
             pb.node("Relu", ["hidden"], ["relu"], "relu"),
             pb.node("MatMul", ["relu", "weight2"], ["matmul2"], "matmul2"),
             pb.node("Add", ["matmul2", "bias2"], ["output"], "add2")]
    inits = [pb.tensor("weight1", w1), pb.tensor("bias1", b1), pb.tensor("weight2", w2), pb.tensor("bias2", b2)]
    g = pb.graph("test-model", nodes, inits, [pb.value_info("input", [1, 3])], [pb.value_info("output", [1, 2])])
    return pb.model(g, opset=12, ir_version=10, producer="GPU-AI-Inference-Server")


def gemm_mlp(batch: int | str = 4, din: int = 64, dh: int = 96, dout: int = 10, seed: int = 7) -> bytes:
    """Flatten -> Gemm(transB=1) -> Relu -> Gemm(transB=0, alpha/beta) : exercises Gemm attribute handling."""
    gb = GraphBuilder("gemm_mlp", seed)
    w1 = rng.gaussish(seed, "w1", dh * din).reshape(dh, din) * np.float32(np.sqrt(2.0 / din))
    b1 = (rng.uniform(seed, "b1", dh) - np.float32(0.5))
    w2 = rng.gaussish(seed, "w2", dh * dout).reshape(dh, dout) * np.float32(np.sqrt(1.0 / dh))
    b2 = (rng.uniform(seed, "b2", dout) - np.float32(0.5))
    x = gb.simple("Flatten", ["x"], [pb.attr_int("axis", 1)])
    x = gb.simple("Gemm", [x, gb.init("w1", w1), gb.init("b1", b1)], [pb.attr_int("transB", 1)])
    x = gb.relu(x)
    gb.simple("Gemm", [x, gb.init("w2", w2, raw=False), gb.init("b2", b2, raw=False)],
              [pb.attr_float("alpha", 0.5), pb.attr_float("beta", 2.0)], out="y")
    return gb.finish([("x", [batch, din, 1, 1])], [("y", [batch, dout])], opset=11)


def resnet_block(batch: int | str = 2, c: int = 32, image: int = 16, seed: int = 50) -> bytes:
    """conv3x3 s2 -> (conv-bn-relu-conv-bn) + identity -> relu -> maxpool -> output [N,C,H,W] (H,W>1).

    Exercises Conv->BN epilogue folding, residual Add, stand-alone Relu, strided 3x3, NCHW output transform.
    """
    gb = GraphBuilder("resnet_block", seed)
    x = gb.conv("x", 3, c, 3, stride=2, pad=1, bias=True)
    x = gb.relu(gb.bn(x, c))
    y = gb.conv(x, c, c, 3, pad=1)
    y = gb.relu(gb.bn(y, c))
    y = gb.conv(y, c, c, 3, pad=1)
    y = gb.bn(y, c)
    s = gb.simple("Add", [y, x])
    s = gb.relu(s)
    gb.nodes.append(pb.node("MaxPool", [s], ["y"], "final_pool", [
        pb.attr_ints("kernel_shape", [2, 2]), pb.attr_ints("pads", [0] * 4), pb.attr_ints("strides", [2, 2])]))
    return gb.finish([("x", [batch, 3, image, image])], [("y", [batch, c, image // 4, image // 4])], opset=11)


def preact_block(batch: int | str = 2, c: int = 32, image: int = 16, seed: int = 53, final_relu: bool = True) -> bytes:
    """Pre-activation (ResNet-v2) residual blocks: the Add of a block is followed by the NEXT block's BN, so the graph holds
    Conv -> Add -> BN(gamma != 1) -> ReLU chains, and ends in Add -> BN -> [ReLU] -> GlobalAveragePool.

    Regression graph for the planner: a BN that follows an absorbed residual Add must scale the shortcut too
    (relu(s*(conv+res)+t), not relu(s*conv+res+t)), so it cannot be folded into the conv's weights.
    """
    gb = GraphBuilder("preact_block", seed)
    x = gb.conv("x", 3, c, 3, pad=1, bias=True)
    for _ in range(2):
        y = gb.conv(gb.relu(gb.bn(x, c, g_center=1.6)), c, c, 3, pad=1)
        y = gb.conv(gb.relu(gb.bn(y, c, g_center=0.7)), c, c, 3, pad=1, bias=True)
        x = gb.simple("Add", [y, x])
    z = gb.bn(x, c, g_center=2.5)
    if final_relu:
        z = gb.relu(z)
    gb.nodes.append(pb.node("GlobalAveragePool", [z], ["y"], "final_gap"))
    return gb.finish([("x", [batch, 3, image, image])], [("y", [batch, c, 1, 1])], opset=11)


def two_input_graph(batch: int | str = 2, ca: int = 8, cb: int = 16, image: int = 12, seed: int = 54) -> bytes:
    """Two graph inputs declared in the order (b_in, a_in) with different channel counts, merged by Concat after one conv each.

    ModelInfer must place payloads by graph input NAME -> graph index (model.cpp:1174-1190), whatever order the caller lists them in.
    """
    gb = GraphBuilder("two_input", seed)
    ya = gb.relu(gb.conv("a_in", ca, 16, 3, pad=1, bias=True))
    yb = gb.relu(gb.conv("b_in", cb, 16, 1, bias=True))
    x = gb.concat([ya, yb])
    x = gb.conv(x, 32, 24, 3, pad=1)
    gb.nodes.append(pb.node("GlobalAveragePool", [x], ["y"], "final_gap"))
    return gb.finish([("b_in", [batch, cb, image, image]), ("a_in", [batch, ca, image, image])], [("y", [batch, 24, 1, 1])], opset=11)


def resnet(batch: int | str = 1, *, layers: Sequence[int] = (3, 4, 6, 3), width: int = 64, image: int = 224, classes: int = 1000,
           seed: int = 50, in_name: str = "data", out_name: str = "logits", groups: int = 1, width_per_group: int = 64,
           dilate: Sequence[bool] = (False, False, False), norm: str = "bn", gn_groups: int = 32) -> bytes:
    """ResNet-v1.5 bottleneck network (ResNet-50 with the defaults; BASELINE.json configs[4] names this architecture).

    groups / width_per_group give ResNeXt as torchvision builds it: the bottleneck's 3x3 is a grouped conv of
    int(planes * width_per_group / 64) * groups channels (planes = width * 2^stage; ResNeXt-50 32x4d: 128 / 256 / 512 / 1024).

    conv7x7/s2 -> BN -> ReLU -> maxpool3x3/s2 -> 4 stages of bottlenecks [1x1 -> 3x3 (stride on the 3x3) -> 1x1 (x4)] with a
    projection shortcut (1x1/stride conv + BN) on the first block of a stage and identity shortcuts elsewhere -> global average
    pool -> Flatten -> Gemm.  Exercises what DenseNet does not: residual Add + ReLU, strided 1x1 / 3x3 convs, Cout up to 2048,
    Conv->BN folding without a ReLU, a Gemm classifier.  The last BN of every block gets a small gamma (as zero-init-residual
    training leaves it) so activations stay O(1) through 16 residual additions.

    dilate[i] replaces the stride of stage i + 2 by a dilation, as torchvision's replace_stride_with_dilation does: the first block of a
    dilated stage keeps the previous dilation, the others use the doubled one (3x3 convs with pads = dilation).

    norm "gn": every BatchNormalization is a GroupNorm of gn_groups groups in torch's spelling below opset 18 (GraphBuilder.group_norm, back "shape"),
    as torchvision's resnet50(norm_layer=lambda c: GroupNorm(32, c)) exports.
    """
    gb = GraphBuilder("resnet", seed)
    x, cin = _resnet_body(gb, in_name, layers, width, groups, width_per_group, dilate, norm, gn_groups)
    x = gb.gap(x)
    x = gb.simple("Flatten", [x], [pb.attr_int("axis", 1)])
    wfc = rng.gaussish(seed, "fc_w", classes * cin).reshape(classes, cin) * np.float32(np.sqrt(1.0 / cin))
    bfc = (rng.uniform(seed, "fc_b", classes) - np.float32(0.5)) * np.float32(0.2)
    gb.simple("Gemm", [x, gb.init("fc_w", wfc.astype(np.float32)), gb.init("fc_b", bfc.astype(np.float32))],
              [pb.attr_int("transB", 1)], out=out_name)
    return gb.finish([(in_name, [batch, 3, image, image])], [(out_name, [batch, classes])], opset=11)


def _resnet_body(gb: GraphBuilder, in_name: str, layers: Sequence[int], width: int, groups: int, width_per_group: int,
                 dilate: Sequence[bool], norm: str = "bn", gn_groups: int = 32) -> tuple[str, int]:
    """The stem and the four bottleneck stages of resnet(); returns (feature map, its channels)"""
    if norm not in ("bn", "gn"):
        raise ValueError(norm)
    bn = gb.bn if norm == "bn" else (lambda x, c, name: gb.group_norm(x, c, gn_groups, back="shape", name=name))
    x = gb.conv(in_name, 3, width, 7, stride=2, pad=3, name="conv1")
    x = gb.relu(bn(x, width, name="bn1"))
    x = gb.pool("MaxPool", x, 3, 2, pad=1)
    cin = width
    dilation = 1
    for si, nblocks in enumerate(layers):
        planes = width * (2 ** si)
        mid = int(planes * (width_per_group / 64.0)) * groups
        cout = planes * 4
        first_dilation = dilation
        stage_stride = 2 if si > 0 else 1
        if si > 0 and dilate[si - 1]:
            dilation *= stage_stride
            stage_stride = 1
        for bi in range(nblocks):
            stride = stage_stride if bi == 0 else 1
            d = first_dilation if bi == 0 else dilation
            tag = f"s{si + 1}b{bi + 1}"
            y = gb.relu(bn(gb.conv(x, cin, mid, 1, name=tag + "_c1"), mid, name=tag + "_bn1"))
            y = gb.relu(bn(gb.conv(y, mid, mid, 3, stride=stride, pad=d, name=tag + "_c2", group=groups, dilation=d), mid, name=tag + "_bn2"))
            y = bn(gb.conv(y, mid, cout, 1, name=tag + "_c3", w_scale=float(0.5 * np.sqrt(2.0 / mid))), cout, name=tag + "_bn3")
            if bi == 0:
                sc = bn(gb.conv(x, cin, cout, 1, stride=stride, name=tag + "_proj"), cout, name=tag + "_bnp")
            else:
                sc = x
            x = gb.relu(gb.simple("Add", [y, sc]))
            cin = cout
    return x, cin


def _seg_head_out(gb: GraphBuilder, x: str, feat_shape: Sequence[int], batch: int | str, image: int, resize: str, coord: str, out_name: str) -> str:
    """The final upsampling of a segmentation net: the [N, classes, h, w] logits to the input's [image, image], bilinear"""
    if resize == "scales":
        return gb.resize(x, feat_shape, scales=[image / feat_shape[2], image / feat_shape[3]], coord=coord, form="scales", name="final_resize", out=out_name)
    return gb.resize(x, (batch, *feat_shape[1:]), sizes=[image, image], coord=coord, form=resize, name="final_resize", out=out_name)


def fcn_resnet50(batch: int | str = 1, *, image: int = 224, classes: int = 21, width: int = 64, resize: str = "sizes",
                 coord: str = "pytorch_half_pixel", seed: int = 95, in_name: str = "image", out_name: str = "out") -> bytes:
    """FCN-ResNet50 as torchvision builds it: the ResNet-50 body with stages 3 and 4 dilated (output stride 8) -> FCNHead [3x3 conv
    2048 -> 512 -> BN -> ReLU -> Dropout -> 1x1 conv -> classes (bias)] -> bilinear Resize to the input size ([N, classes, image, image]).
    width scales every channel count (64: the real net).  resize: "sizes" (a concrete batch), "scales", or "shape" (the sizes computed by
    Shape -> Gather -> Unsqueeze -> Concat -> Cast, as torch exports them); coord: pytorch_half_pixel (torch's align_corners=False) or half_pixel."""
    gb = GraphBuilder("fcn_resnet50", seed)
    x, cin = _resnet_body(gb, in_name, (3, 4, 6, 3), width, 1, 64, (False, True, True))
    inter = cin // 4
    y = gb.relu(gb.bn(gb.conv(x, cin, inter, 3, pad=1, name="head_c1"), inter, name="head_bn1"))
    y = gb.simple("Dropout", [y])
    y = gb.conv(y, inter, classes, 1, bias=True, name="head_cls")
    fh = (image + 7) // 8
    _seg_head_out(gb, y, (batch, classes, fh, fh), batch, image, resize, coord, out_name)
    return gb.finish([(in_name, [batch, 3, image, image])], [(out_name, [batch, classes, image, image])], opset=11)


def deeplabv3_resnet50(batch: int | str = 1, *, image: int = 224, classes: int = 21, width: int = 64, resize: str = "sizes",
                       coord: str = "pytorch_half_pixel", rates: Sequence[int] = (12, 24, 36), seed: int = 96, in_name: str = "image",
                       out_name: str = "out") -> bytes:
    """DeepLabV3-ResNet50 as torchvision builds it: the dilated ResNet-50 body (output stride 8) -> ASPP [1x1 conv; three 3x3 convs with
    dilation = pads = rate; pooling: GlobalAveragePool -> 1x1 conv -> BN -> ReLU -> Resize back to the map] (each branch 256 channels with BN
    and ReLU) -> Concat -> 1x1 projection -> BN -> ReLU -> Dropout -> 3x3 conv -> BN -> ReLU -> 1x1 classifier (bias) -> bilinear Resize to
    the input size.  width, resize and coord as fcn_resnet50 (the pooling branch's Resize takes the same export form)."""
    gb = GraphBuilder("deeplabv3_resnet50", seed)
    x, cin = _resnet_body(gb, in_name, (3, 4, 6, 3), width, 1, 64, (False, True, True))
    a = 4 * width
    fh = (image + 7) // 8
    branches = [gb.relu(gb.bn(gb.conv(x, cin, a, 1, name="aspp0"), a, name="aspp0_bn"))]
    for i, r in enumerate(rates):
        branches.append(gb.relu(gb.bn(gb.conv(x, cin, a, 3, pad=r, dilation=r, name=f"aspp{i + 1}"), a, name=f"aspp{i + 1}_bn")))
    p = gb.relu(gb.bn(gb.conv(gb.gap(x), cin, a, 1, name="aspp_pool"), a, name="aspp_pool_bn"))
    if resize == "scales":
        p = gb.resize(p, (batch, a, 1, 1), scales=[fh, fh], coord=coord, form="scales", name="aspp_pool_up")
    else:
        p = gb.resize(p, (batch, a, 1, 1), sizes=[fh, fh], coord=coord, form=resize, name="aspp_pool_up")
    branches.append(p)
    y = gb.concat(branches)
    y = gb.relu(gb.bn(gb.conv(y, 5 * a, a, 1, name="aspp_proj"), a, name="aspp_proj_bn"))
    y = gb.simple("Dropout", [y])
    y = gb.relu(gb.bn(gb.conv(y, a, a, 3, pad=1, name="head_c1"), a, name="head_bn1"))
    y = gb.conv(y, a, classes, 1, bias=True, name="head_cls")
    _seg_head_out(gb, y, (batch, classes, fh, fh), batch, image, resize, coord, out_name)
    return gb.finish([(in_name, [batch, 3, image, image])], [(out_name, [batch, classes, image, image])], opset=11)


def unet(batch: int | str = 1, *, image: int = 224, base: int = 64, depth: int = 4, classes: int = 2, up: str = "convtranspose", final: str = "none",
         seed: int = 97, in_name: str = "image", out_name: str = "out") -> bytes:
    """U-Net (Ronneberger et al. 2015) with BatchNorm and padded convs, as segmentation libraries build it: `depth` encoder levels of two
    [3x3/p1 conv -> BN -> ReLU] (base, 2 base, ... channels) each followed by a 2x2/s2 max pool, a bottleneck of two such convs (base * 2^depth
    channels), then per decoder level an upsampling that halves the channels, Concat [skip, up] and two [3x3/p1 conv -> BN -> ReLU]; a 1x1
    conv (bias) writes the [N, classes, image, image] logits.  up: "convtranspose" = 2x2/s2 ConvTranspose -> BN -> ReLU; "resize" = bilinear
    x2 Resize -> 1x1 conv -> BN -> ReLU (no transposed conv in the graph).  final: "none" or "sigmoid"."""
    assert image % 2 ** depth == 0, "the image extent must be a multiple of 2^depth"
    assert up in ("convtranspose", "resize") and final in ("none", "sigmoid")
    gb = GraphBuilder("unet", seed)

    def double(x: str, cin: int, cout: int, tag: str) -> str:
        x = gb.relu(gb.bn(gb.conv(x, cin, cout, 3, pad=1, name=tag + "_c1"), cout, name=tag + "_bn1"))
        return gb.relu(gb.bn(gb.conv(x, cout, cout, 3, pad=1, name=tag + "_c2"), cout, name=tag + "_bn2"))

    x, c, skips = in_name, 3, []
    for lv in range(depth):
        x = double(x, c, base << lv, f"enc{lv}")
        c = base << lv
        skips.append((x, c))
        x = gb.pool("MaxPool", x, 2, 2, 0)
    x = double(x, c, base << depth, "mid")
    c = base << depth
    for lv in reversed(range(depth)):
        skip, cs = skips[lv]
        hw = image >> (lv + 1)
        if up == "convtranspose":
            u = gb.conv_transpose(x, c, cs, 2, 2, name=f"up{lv}")
        else:
            u = gb.resize(x, (batch, c, hw, hw), scales=[2.0, 2.0], form="scales", name=f"up{lv}_resize")
            u = gb.conv(u, c, cs, 1, name=f"up{lv}")
        u = gb.relu(gb.bn(u, cs, name=f"up{lv}_bn"))
        x = double(gb.concat([skip, u]), 2 * cs, cs, f"dec{lv}")
        c = cs
    if final == "sigmoid":
        gb.simple("Sigmoid", [gb.conv(x, c, classes, 1, bias=True, name="head")], out=out_name)
    else:
        gb.conv(x, c, classes, 1, bias=True, name="head", out=out_name)
    return gb.finish([(in_name, [batch, 3, image, image])], [(out_name, [batch, classes, image, image])], opset=11)


def resnet50(batch: int | str = 1) -> bytes:
    return resnet(batch)


def resnet50_gn(batch: int | str = 1, **kw) -> bytes:
    """ResNet-50 with GroupNorm(32) in place of every BatchNorm (torchvision's resnet50(norm_layer=GroupNorm), detectron2 / BiT backbones)"""
    return resnet(batch, norm="gn", gn_groups=32, **kw)


def resnext50_32x4d(batch: int | str = 1, **kw) -> bytes:
    return resnet(batch, groups=32, width_per_group=4, **kw)


def regnet(batch: int | str = 1, *, depths: Sequence[int], widths: Sequence[int], group_width: int, se_ratio: float = 0.0, stem: int = 32,
           image: int = 224, classes: int = 1000, seed: int = 90, in_name: str = "data", out_name: str = "logits") -> bytes:
    """RegNet as torchvision builds it: conv3x3/s2 (stem) -> BN -> ReLU -> stages of residual bottlenecks [1x1 -> BN -> ReLU -> grouped 3x3
    (stride 2 on a stage's first block, group width `group_width`) -> BN -> ReLU [-> SE: squeeze round(se_ratio * block input width), ReLU,
    sigmoid] -> 1x1 -> BN] + shortcut (1x1/stride conv + BN where the width or the stride changes) -> ReLU -> global pool -> Flatten -> Gemm.
    The last 1x1 of every block gets half the He scale, as in resnet(), so activations stay O(1) through the residual additions."""
    gb = GraphBuilder("regnet", seed)
    x = gb.relu(gb.bn(gb.conv(in_name, 3, stem, 3, stride=2, pad=1, name="stem"), stem, name="stem_bn"))
    cin = stem
    for si, (depth, w) in enumerate(zip(depths, widths)):
        for bi in range(depth):
            stride = 2 if bi == 0 else 1
            tag = f"s{si + 1}b{bi + 1}"
            y = gb.relu(gb.bn(gb.conv(x, cin, w, 1, name=tag + "_a"), w, name=tag + "_a_bn"))
            y = gb.relu(gb.bn(gb.conv(y, w, w, 3, stride=stride, pad=1, name=tag + "_b", group=w // group_width), w, name=tag + "_b_bn"))
            if se_ratio > 0:
                y = gb.se(y, w, int(round(se_ratio * cin)), act1="relu", gate="sigmoid", name=tag + "_se")
            y = gb.bn(gb.conv(y, w, w, 1, name=tag + "_c", w_scale=float(0.5 * np.sqrt(2.0 / w))), w, name=tag + "_c_bn")
            if cin != w or stride != 1:
                sc = gb.bn(gb.conv(x, cin, w, 1, stride=stride, name=tag + "_proj"), w, name=tag + "_proj_bn")
            else:
                sc = x
            x = gb.relu(gb.simple("Add", [y, sc]))
            cin = w
    x = gb.gap(x)
    x = gb.simple("Flatten", [x], [pb.attr_int("axis", 1)])
    wfc = rng.gaussish(seed, "fc_w", classes * cin).reshape(classes, cin) * np.float32(np.sqrt(1.0 / cin))
    bfc = (rng.uniform(seed, "fc_b", classes) - np.float32(0.5)) * np.float32(0.2)
    gb.simple("Gemm", [x, gb.init("fc_w", wfc.astype(np.float32)), gb.init("fc_b", bfc.astype(np.float32))],
              [pb.attr_int("transB", 1)], out=out_name)
    return gb.finish([(in_name, [batch, 3, image, image])], [(out_name, [batch, classes])], opset=11)


def regnet_y_400mf(batch: int | str = 1, **kw) -> bytes:
    return regnet(batch, depths=(1, 3, 6, 6), widths=(48, 104, 208, 440), group_width=8, se_ratio=0.25, **kw)


def regnet_x_400mf(batch: int | str = 1, **kw) -> bytes:
    return regnet(batch, depths=(1, 2, 7, 12), widths=(32, 64, 160, 400), group_width=16, **kw)


# MobileNetV2 inverted-residual table (Sandler et al. 2018, Table 2): expansion t, output channels c, repeats n, first stride s
MOBILENET_V2_BLOCKS = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1))


def _divisible8(v: float) -> int:
    """Channel rounding of the published MobileNetV2 (nearest multiple of 8, never below 90 % of v)."""
    n = max(8, int(v + 4) // 8 * 8)
    return n + 8 if n < 0.9 * v else n


def mobilenet_v2(batch: int | str = 1, *, width_mult: float = 1.0, image: int = 224, classes: int = 1000, seed: int = 62,
                 clip_form: str = "initializer", in_name: str = "data", out_name: str = "logits") -> bytes:
    """MobileNetV2: conv3x3/s2 (32) -> BN -> ReLU6 -> 17 inverted-residual blocks -> conv1x1 (1280) -> BN -> ReLU6 -> global pool ->
    Flatten -> Gemm.  A block is [expand 1x1 -> BN -> ReLU6 ->] depthwise 3x3 (stride s) -> BN -> ReLU6 -> project 1x1 -> BN, plus an
    identity Add where the stride is 1 and the channel count is kept (10 of them); the first block has no expand conv.  ReLU6 is
    Clip(0, 6) in the given export form (GraphBuilder.clip).  The projection BNs get a small gamma (as trained networks end up with)
    so activations stay O(1) through the residual additions.
    """
    gb = GraphBuilder("mobilenet_v2", seed)
    c = _divisible8(32 * width_mult)
    last = _divisible8(1280 * max(1.0, width_mult))
    x = gb.clip(gb.bn(gb.conv(in_name, 3, c, 3, stride=2, pad=1, name="stem"), c, name="stem_bn"), 0.0, 6.0, clip_form)
    bi = 0
    for t, ch, n, s in MOBILENET_V2_BLOCKS:
        cout = _divisible8(ch * width_mult)
        for i in range(n):
            bi += 1
            stride = s if i == 0 else 1
            tag = f"b{bi}"
            hid = c * t
            y = x
            if t != 1:
                y = gb.clip(gb.bn(gb.conv(y, c, hid, 1, name=tag + "_expand"), hid, name=tag + "_bn1"), 0.0, 6.0, clip_form)
            y = gb.clip(gb.bn(gb.conv(y, hid, hid, 3, stride=stride, pad=1, group=hid, name=tag + "_dw"), hid, name=tag + "_bn2"), 0.0, 6.0, clip_form)
            y = gb.bn(gb.conv(y, hid, cout, 1, name=tag + "_project"), cout, name=tag + "_bn3", g_center=0.3)
            if stride == 1 and c == cout:
                y = gb.simple("Add", [y, x])
            x = y
            c = cout
    x = gb.clip(gb.bn(gb.conv(x, c, last, 1, name="head"), last, name="head_bn"), 0.0, 6.0, clip_form)
    x = gb.gap(x)
    x = gb.simple("Flatten", [x], [pb.attr_int("axis", 1)])
    wfc = rng.gaussish(seed, "fc_w", classes * last).reshape(classes, last) * np.float32(np.sqrt(1.0 / last))
    bfc = (rng.uniform(seed, "fc_b", classes) - np.float32(0.5)) * np.float32(0.2)
    gb.simple("Gemm", [x, gb.init("fc_w", wfc.astype(np.float32)), gb.init("fc_b", bfc.astype(np.float32))],
              [pb.attr_int("transB", 1)], out=out_name)
    return gb.finish([(in_name, [batch, 3, image, image])], [(out_name, [batch, classes])], opset=6 if clip_form == "attrs" else 11)


# torchvision's MobileNetV3 tables (Howard et al. 2019, Tables 1-2): input channels, kernel, expanded channels, output channels, SE, activation, stride
MOBILENET_V3_LARGE = ((16, 3, 16, 16, False, "RE", 1), (16, 3, 64, 24, False, "RE", 2), (24, 3, 72, 24, False, "RE", 1),
                      (24, 5, 72, 40, True, "RE", 2), (40, 5, 120, 40, True, "RE", 1), (40, 5, 120, 40, True, "RE", 1),
                      (40, 3, 240, 80, False, "HS", 2), (80, 3, 200, 80, False, "HS", 1), (80, 3, 184, 80, False, "HS", 1),
                      (80, 3, 184, 80, False, "HS", 1), (80, 3, 480, 112, True, "HS", 1), (112, 3, 672, 112, True, "HS", 1),
                      (112, 5, 672, 160, True, "HS", 2), (160, 5, 960, 160, True, "HS", 1), (160, 5, 960, 160, True, "HS", 1))
MOBILENET_V3_SMALL = ((16, 3, 16, 16, True, "RE", 2), (16, 3, 72, 24, False, "RE", 2), (24, 3, 88, 24, False, "RE", 1),
                      (24, 5, 96, 40, True, "HS", 2), (40, 5, 240, 40, True, "HS", 1), (40, 5, 240, 40, True, "HS", 1),
                      (40, 5, 120, 48, True, "HS", 1), (48, 5, 144, 48, True, "HS", 1), (48, 5, 288, 96, True, "HS", 2),
                      (96, 5, 576, 96, True, "HS", 1), (96, 5, 576, 96, True, "HS", 1))


def mobilenet_v3(batch: int | str = 1, *, variant: str = "large", width_mult: float = 1.0, image: int = 224, classes: int = 1000, seed: int = 73,
                 act_form: str = "op", in_name: str = "data", out_name: str = "logits") -> bytes:
    """MobileNetV3-Large / -Small as torchvision builds them: conv3x3/s2 (16) -> BN -> hardswish -> inverted-residual blocks [expand 1x1 -> BN ->
    act ->] depthwise k x k (stride s) -> BN -> act [-> SE: squeeze make_divisible(exp // 4, 8), ReLU, hardsigmoid] -> project 1x1 -> BN (+ identity
    where the stride is 1 and the channel count is kept) -> conv1x1 (6 x last block channels) -> BN -> hardswish -> global pool -> Flatten ->
    Gemm -> hardswish -> Dropout -> Gemm.  act_form: how HardSwish / HardSigmoid reach the graph (GraphBuilder.hardswish); the SE gate's
    HardSigmoid is the operator itself in every form.  Projection BNs get a small gamma so activations stay O(1) through the residual adds."""
    table = {"large": MOBILENET_V3_LARGE, "small": MOBILENET_V3_SMALL}[variant]
    last_channel = {"large": 1280, "small": 1024}[variant]
    gb = GraphBuilder("mobilenet_v3_" + variant, seed)

    def act(x: str, kind: str) -> str:
        return gb.relu(x) if kind == "RE" else gb.hardswish(x, act_form)
    ch = lambda v: _divisible8(v * width_mult)  # noqa: E731
    c = ch(16)
    x = act(gb.bn(gb.conv(in_name, 3, c, 3, stride=2, pad=1, name="stem"), c, name="stem_bn"), "HS")
    for bi, (cin, k, exp, cout, use_se, a, s) in enumerate(table, 1):
        tag = f"b{bi}"
        cin, exp, cout = ch(cin), ch(exp), ch(cout)
        assert cin == c
        y = x
        if exp != cin:
            y = act(gb.bn(gb.conv(y, cin, exp, 1, name=tag + "_expand"), exp, name=tag + "_bn1"), a)
        y = act(gb.bn(gb.conv(y, exp, exp, k, stride=s, pad=k // 2, group=exp, name=tag + "_dw"), exp, name=tag + "_bn2"), a)
        if use_se:
            y = gb.se(y, exp, _divisible8(exp // 4), "relu", "hardsigmoid", name=tag + "_se")
        y = gb.bn(gb.conv(y, exp, cout, 1, name=tag + "_project"), cout, name=tag + "_bn3", g_center=0.3)
        if s == 1 and cin == cout:
            y = gb.simple("Add", [y, x])
        x, c = y, cout
    head = 6 * c
    x = act(gb.bn(gb.conv(x, c, head, 1, name="head"), head, name="head_bn"), "HS")
    x = gb.simple("Flatten", [gb.gap(x)], [pb.attr_int("axis", 1)])
    w1 = rng.gaussish(seed, "fc1_w", last_channel * head).reshape(last_channel, head) * np.float32(np.sqrt(2.0 / head))
    b1 = (rng.uniform(seed, "fc1_b", last_channel) - np.float32(0.5)) * np.float32(0.2)
    x = gb.simple("Gemm", [x, gb.init("fc1_w", w1.astype(np.float32)), gb.init("fc1_b", b1.astype(np.float32))], [pb.attr_int("transB", 1)])
    x = gb.simple("Dropout", [gb.hardswish(x, act_form)])
    w2 = rng.gaussish(seed, "fc2_w", classes * last_channel).reshape(classes, last_channel) * np.float32(np.sqrt(1.0 / last_channel))
    b2 = (rng.uniform(seed, "fc2_b", classes) - np.float32(0.5)) * np.float32(0.2)
    gb.simple("Gemm", [x, gb.init("fc2_w", w2.astype(np.float32)), gb.init("fc2_b", b2.astype(np.float32))], [pb.attr_int("transB", 1)], out=out_name)
    return gb.finish([(in_name, [batch, 3, image, image])], [(out_name, [batch, classes])], opset=14 if act_form == "op" else 13)


# torchvision's EfficientNet-B0 stages (Tan & Le 2019, Table 1): expand ratio, kernel, first stride, input channels, output channels, layers
EFFICIENTNET_B0 = ((1, 3, 1, 32, 16, 1), (6, 3, 2, 16, 24, 2), (6, 5, 2, 24, 40, 2), (6, 3, 2, 40, 80, 3), (6, 5, 1, 80, 112, 3),
                   (6, 5, 2, 112, 192, 4), (6, 3, 1, 192, 320, 1))


def efficientnet_b0(batch: int | str = 1, *, width_mult: float = 1.0, image: int = 224, classes: int = 1000, seed: int = 80, swap_mul: bool = False,
                    in_name: str = "data", out_name: str = "logits") -> bytes:
    """EfficientNet-B0 as torchvision builds it: conv3x3/s2 (32) -> BN -> SiLU -> MBConv blocks [expand 1x1 -> BN -> SiLU ->] depthwise k x k ->
    BN -> SiLU -> SE (squeeze = block input channels // 4, SiLU, sigmoid) -> project 1x1 -> BN (+ identity where the stride is 1 and the
    channel count is kept) -> conv1x1 (1280) -> BN -> SiLU -> global pool -> Flatten -> Gemm.  SiLU is Mul(x, Sigmoid(x)) (swap_mul: Mul(Sigmoid(x), x),
    and the SE gate Mul with its operands swapped)."""
    gb = GraphBuilder("efficientnet_b0", seed)
    ch = lambda v: _divisible8(v * width_mult)  # noqa: E731
    c = ch(32)
    x = gb.silu(gb.bn(gb.conv(in_name, 3, c, 3, stride=2, pad=1, name="stem"), c, name="stem_bn"), swap_mul)
    bi = 0
    for t, k, s, cin, cout, n in EFFICIENTNET_B0:
        cout = ch(cout)
        for i in range(n):
            bi += 1
            tag = f"b{bi}"
            stride = s if i == 0 else 1
            exp = c * t
            y = x
            if t != 1:
                y = gb.silu(gb.bn(gb.conv(y, c, exp, 1, name=tag + "_expand"), exp, name=tag + "_bn1"), swap_mul)
            y = gb.silu(gb.bn(gb.conv(y, exp, exp, k, stride=stride, pad=k // 2, group=exp, name=tag + "_dw"), exp, name=tag + "_bn2"), swap_mul)
            y = gb.se(y, exp, max(1, c // 4), "silu", "sigmoid", name=tag + "_se", swap=swap_mul, form="mul_hardsigmoid" if swap_mul else "op")
            y = gb.bn(gb.conv(y, exp, cout, 1, name=tag + "_project"), cout, name=tag + "_bn3", g_center=0.3)
            if stride == 1 and c == cout:
                y = gb.simple("Add", [y, x])
            x, c = y, cout
    head = 4 * c
    x = gb.silu(gb.bn(gb.conv(x, c, head, 1, name="head"), head, name="head_bn"), swap_mul)
    x = gb.simple("Flatten", [gb.gap(x)], [pb.attr_int("axis", 1)])
    wfc = rng.gaussish(seed, "fc_w", classes * head).reshape(classes, head) * np.float32(np.sqrt(1.0 / head))
    bfc = (rng.uniform(seed, "fc_b", classes) - np.float32(0.5)) * np.float32(0.2)
    gb.simple("Gemm", [x, gb.init("fc_w", wfc.astype(np.float32)), gb.init("fc_b", bfc.astype(np.float32))], [pb.attr_int("transB", 1)], out=out_name)
    return gb.finish([(in_name, [batch, 3, image, image])], [(out_name, [batch, classes])], opset=13)


def _convnext_block(gb: GraphBuilder, x: str, c: int, tag: str, gelu: str, gelu_swap: bool, out: str | None = None) -> str:
    """depthwise 7x7 (bias) -> Transpose(0,2,3,1) -> LayerNorm -> Linear c -> 4c -> GELU -> Linear 4c -> c -> Transpose(0,3,1,2) -> layer scale [c,1,1] -> + x"""
    y = gb.conv(x, c, c, 7, pad=3, bias=True, group=c, name=tag + "_dw")
    y = gb.layernorm(gb.transpose(y, (0, 2, 3, 1)), c, name=tag + "_ln")
    y = gb.gelu(gb.linear(y, c, 4 * c, name=tag + "_fc1"), gelu, gelu_swap)
    y = gb.transpose(gb.linear(y, 4 * c, c, name=tag + "_fc2", w_scale=float(np.sqrt(2.0 / (4 * c)))), (0, 3, 1, 2))
    ls = np.float32(0.5) + rng.uniform(gb.seed, tag + "_scale", c)
    y = gb.simple("Mul", [gb.init(tag + "_scale", ls.reshape(c, 1, 1).astype(np.float32)), y])
    return gb.simple("Add", [y, x], out=out)


def convnext_block(batch: int | str, c: int, hw: int, *, gelu: str = "erf", gelu_swap: bool = False, seed: int = 7) -> bytes:
    """One ConvNeXt block alone: x [batch, c, hw, hw] -> y of the same shape."""
    gb = GraphBuilder("convnext_block", seed)
    _convnext_block(gb, "x", c, "blk", gelu, gelu_swap, out="y")
    return gb.finish([("x", [batch, c, hw, hw])], [("y", [batch, c, hw, hw])], opset=20 if gelu.startswith("op") else 17)


def convnext(batch: int | str = 1, *, depths: Sequence[int] = (3, 3, 9, 3), dims: Sequence[int] = (96, 192, 384, 768), image: int = 224,
             classes: int = 1000, gelu: str = "erf", gelu_swap: bool = False, seed: int = 2020, in_name: str = "input", out_name: str = "logits") -> bytes:
    """ConvNeXt (Liu et al. 2022) as torchvision's exporter writes it at opset 17: stem conv 4x4/s4 (bias) -> LayerNorm over the channels; per stage
    `depth` blocks [depthwise 7x7 (bias) -> LayerNorm -> Linear C -> 4C -> GELU -> Linear 4C -> C -> layer scale -> + input]; between the stages
    LayerNorm -> conv 2x2/s2 (bias); GlobalAveragePool -> LayerNorm -> Flatten -> Gemm.  torch's LayerNorm / Linear act on the last axis, so every
    LayerNorm and every block's MLP sits between Transpose(0,2,3,1) and Transpose(0,3,1,2).  gelu: a GraphBuilder.gelu form (the op forms need
    opset 20).  The layer scales are drawn from [0.5, 1.5), not torchvision's initial 1e-6, at which every block is the identity to seven digits
    and a broken block would pass every network test."""
    gb = GraphBuilder("convnext", seed)

    def ln2d(x: str, c: int, name: str) -> str:
        return gb.transpose(gb.layernorm(gb.transpose(x, (0, 2, 3, 1)), c, name=name), (0, 3, 1, 2))

    c = dims[0]
    x = ln2d(gb.conv(in_name, 3, c, 4, stride=4, bias=True, name="stem"), c, "stem_ln")
    for si, (depth, dim) in enumerate(zip(depths, dims)):
        if si > 0:
            x = gb.conv(ln2d(x, c, f"down{si}_ln"), c, dim, 2, stride=2, bias=True, name=f"down{si}")
            c = dim
        for bi in range(depth):
            x = _convnext_block(gb, x, c, f"s{si}b{bi}", gelu, gelu_swap)
    x = gb.simple("Flatten", [ln2d(gb.gap(x), c, "head_ln")], [pb.attr_int("axis", 1)])
    wfc = rng.gaussish(seed, "fc_w", classes * c).reshape(classes, c) * np.float32(np.sqrt(1.0 / c))
    bfc = (rng.uniform(seed, "fc_b", classes) - np.float32(0.5)) * np.float32(0.2)
    gb.simple("Gemm", [x, gb.init("fc_w", wfc.astype(np.float32)), gb.init("fc_b", bfc.astype(np.float32))], [pb.attr_int("transB", 1)], out=out_name)
    return gb.finish([(in_name, [batch, 3, image, image])], [(out_name, [batch, classes])], opset=20 if gelu.startswith("op") else 17)


def convnext_tiny(batch: int | str = 1, **kw) -> bytes:
    return convnext(batch, depths=(3, 3, 9, 3), dims=(96, 192, 384, 768), **kw)


def vit_attention(gb: GraphBuilder, x: str, dim: int, heads: int, tag: str, *, unbind: str = "gather", scale: str = "q", swap: bool = False,
                  qkv: str | None = None) -> str:
    """Multi-head self-attention on tokens x [N, L, dim] as torch's exporter writes it unfused: Linear dim -> 3 dim -> Reshape [N, L, 3, H, hd] ->
    Transpose [2,0,3,1,4] -> q, k, v -> MatMul(q, Transpose(k, [0,1,3,2])) -> Softmax(-1) -> MatMul(p, v) -> Transpose [0,2,1,3] -> Reshape [N, L, dim].
    unbind: "gather" (three Gather(axis 0, scalar index)) or "split" (Split(axis 0) into three, each followed by Squeeze(axes [0])).
    scale (c = hd^-0.5): "q" Mul(q, c); "s_mul" Mul(scores, c); "s_div" Div(scores, 1 / c); "sdpa" Mul(q, sqrt c) and Mul(kT, sqrt c).
    swap: the constant is the first operand of every Mul.  qkv: an existing [N, L, 3 dim] value instead of the Linear."""
    hd = dim // heads
    c = float(hd) ** -0.5

    def const(name: str, v: float) -> str:
        return gb.init(f"{tag}_{name}", np.array(v, np.float32))

    def mul(a: str, k: str) -> str:
        return gb.simple("Mul", [k, a] if swap else [a, k])

    y = qkv or gb.linear(x, dim, 3 * dim, name=tag + "_qkv")
    y = gb.simple("Reshape", [y, gb.init(tag + "_shape5", np.array([0, -1, 3, heads, hd], np.int64))])
    y = gb.transpose(y, (2, 0, 3, 1, 4))
    if unbind == "gather":
        parts = []
        for i in range(3):
            idx = f"{tag}_i{i}"            # a scalar index (a Constant node: initializers here are at least 1-D)
            gb.nodes.append(pb.node("Constant", [], [idx], idx, [pb.attr_int("value_int", i)]))
            parts.append(gb.simple("Gather", [y, idx], [pb.attr_int("axis", 0)]))
    elif unbind == "split":
        name = gb._uid("split")
        outs = [f"{name}_out{i}" for i in range(3)]
        gb.nodes.append(pb.node("Split", [y, gb.init(tag + "_split", np.array([1, 1, 1], np.int64))], outs, name, [pb.attr_int("axis", 0)]))
        ax = gb.init(tag + "_axes0", np.array([0], np.int64))
        parts = [gb.simple("Squeeze", [o, ax]) for o in outs]
    else:
        raise ValueError(unbind)
    q, k, v = parts
    if scale == "q":
        q = mul(q, const("scale", c))
    elif scale == "sdpa":
        q = mul(q, const("sqrt_scale_q", np.sqrt(c)))
    kt = gb.transpose(k, (0, 1, 3, 2))
    if scale == "sdpa":
        kt = mul(kt, const("sqrt_scale_k", np.sqrt(c)))
    s = gb.simple("MatMul", [q, kt])
    if scale == "s_mul":
        s = mul(s, const("scale", c))
    elif scale == "s_div":
        s = gb.simple("Div", [s, const("inv_scale", 1.0 / c)])
    elif scale not in ("q", "sdpa"):
        raise ValueError(scale)
    p = gb.simple("Softmax", [s], [pb.attr_int("axis", -1)])
    y = gb.transpose(gb.simple("MatMul", [p, v]), (0, 2, 1, 3))
    return gb.simple("Reshape", [y, gb.init(tag + "_shape3", np.array([0, -1, dim], np.int64))])


def vit_tokens(gb: GraphBuilder, x: str, dim: int) -> str:
    """[N, dim, h, w] -> tokens [N, h w, dim]: Reshape [0, dim, -1] -> Transpose [0,2,1]"""
    name = gb._uid("tok")
    return gb.transpose(gb.simple("Reshape", [x, gb.init(name + "_shape", np.array([0, dim, -1], np.int64))]), (0, 2, 1))


def vit(batch: int | str = 1, *, image: int = 224, patch: int = 16, dim: int = 768, depth: int = 12, heads: int = 12, mlp: int = 3072,
        classes: int = 1000, unbind: str = "gather", scale: str = "q", gelu: str = "erf", seed: int = 2021, in_name: str = "input",
        out_name: str = "logits") -> bytes:
    """The pre-norm Vision Transformer (Dosovitskiy et al. 2021) as torch's exporter writes it at opset 17 with an unfused attention: patch conv
    P x P / sP (bias) -> Reshape [N, D, G G] -> Transpose [0,2,1] -> Concat(axis 1)[Expand(class_token), tokens] -> Add pos_embedding; per layer
    LayerNorm -> attention (vit_attention) -> Linear -> + x, LayerNorm -> Linear D -> mlp -> GELU -> Linear mlp -> D -> + x; LayerNorm ->
    Gather(axis 1, index 0) -> Gemm.  The Expand's shape is a constant for an int batch and Shape(input) -> Gather 0 -> Unsqueeze -> Concat for a
    symbolic one.  class_token and pos_embedding are O(1) draws, not torchvision's 0 / 0.02 N(0,1), at which dropping either would move the logits
    by less than a test's tolerance."""
    gb = GraphBuilder("vit", seed)
    g = image // patch
    L = g * g + 1
    x = vit_tokens(gb, gb.conv(in_name, 3, dim, patch, stride=patch, bias=True, name="patch"), dim)
    cls = gb.init("class_token", (rng.gaussish(seed, "class_token", dim).reshape(1, 1, dim)).astype(np.float32))
    if isinstance(batch, int):
        shp = gb.init("cls_shape", np.array([batch, 1, dim], np.int64))
    else:
        gb.nodes.append(pb.node("Shape", [in_name], ["cls_in_shape"], "cls_in_shape"))
        gb.nodes.append(pb.node("Constant", [], ["cls_i0"], "cls_i0", [pb.attr_int("value_int", 0)]))
        gb.nodes.append(pb.node("Gather", ["cls_in_shape", "cls_i0"], ["cls_n"], "cls_n", [pb.attr_int("axis", 0)]))
        gb.nodes.append(pb.node("Unsqueeze", ["cls_n"], ["cls_n1"], "cls_n1", [pb.attr_ints("axes", [0])]))
        gb.nodes.append(pb.node("Concat", ["cls_n1", gb.init("cls_tail", np.array([1, dim], np.int64))], ["cls_shape"], "cls_shape_cat", [pb.attr_int("axis", 0)]))
        shp = "cls_shape"
    x = gb.concat([gb.simple("Expand", [cls, shp]), x], axis=1)
    pos = (np.float32(0.5) * rng.gaussish(seed, "pos_embedding", L * dim)).reshape(1, L, dim)
    x = gb.simple("Add", [x, gb.init("pos_embedding", pos.astype(np.float32))])
    for li in range(depth):
        tag = f"l{li}"
        y = vit_attention(gb, gb.layernorm(x, dim, name=tag + "_ln1"), dim, heads, tag + "_attn", unbind=unbind, scale=scale)
        x = gb.simple("Add", [gb.linear(y, dim, dim, name=tag + "_proj"), x])
        y = gb.gelu(gb.linear(gb.layernorm(x, dim, name=tag + "_ln2"), dim, mlp, name=tag + "_fc1"), gelu)
        x = gb.simple("Add", [gb.linear(y, mlp, dim, name=tag + "_fc2", w_scale=float(np.sqrt(2.0 / mlp))), x])
    x = gb.layernorm(x, dim, name="head_ln")
    gb.nodes.append(pb.node("Constant", [], ["head_i0"], "head_i0", [pb.attr_int("value_int", 0)]))
    x = gb.simple("Gather", [x, "head_i0"], [pb.attr_int("axis", 1)])
    wfc = rng.gaussish(seed, "fc_w", classes * dim).reshape(classes, dim) * np.float32(np.sqrt(1.0 / dim))
    bfc = (rng.uniform(seed, "fc_b", classes) - np.float32(0.5)) * np.float32(0.2)
    gb.simple("Gemm", [x, gb.init("fc_w", wfc.astype(np.float32)), gb.init("fc_b", bfc.astype(np.float32))], [pb.attr_int("transB", 1)], out=out_name)
    return gb.finish([(in_name, [batch, 3, image, image])], [(out_name, [batch, classes])], opset=20 if gelu.startswith("op") else 17)


def vit_b_16(batch: int | str = 1, **kw) -> bytes:
    return vit(batch, image=224, patch=16, dim=768, depth=12, heads=12, mlp=3072, **kw)


def vit_tiny_16(batch: int | str = 1, **kw) -> bytes:
    return vit(batch, image=224, patch=16, dim=192, depth=12, heads=3, mlp=768, **kw)


ONNX_INT64 = pb.INT64
FLOAT32_MIN = float(np.finfo(np.float32).min)


def bert_embeddings(gb: GraphBuilder, seq: int, vocab: int, dim: int, *, types: int = 2, max_pos: int = 512, pos: str | None = "const",
                    order: str = "wtp", eps: float = 1e-12, ids: str = "input_ids", type_ids: str = "token_type_ids", table_std: float = 1.0,
                    table_mean: float = 0.0) -> str:
    """BertEmbeddings as the exporter writes it: Gather(word [vocab, dim], ids) + Gather(type [types, dim], type_ids) + pos -> LayerNormalization.
    types = 0: no type table.  pos: "const" (the [1, seq, dim] rows as a constant), "gather" (Gather(position table [max_pos, dim],
    Slice(position_ids [1, max_pos], 0 : seq, axis 1))) or None.  order: which sum comes first, "wtp" (word + type) + pos, "wpt" (word + pos) + type,
    "ptw" pos + (type + word).  The tables are O(1) draws (table_mean + table_std * N(0,1)), not BERT's 0.02 N(0,1), at which dropping one of them
    would move the logits by less than a test's tolerance."""
    seed = gb.seed

    def table(name: str, rows: int) -> str:
        t = np.float32(table_mean) + np.float32(table_std) * rng.gaussish(seed, name, rows * dim).reshape(rows, dim)
        return gb.init(name, t.astype(np.float32))

    w = gb.simple("Gather", [table("word_embeddings", vocab), ids], [pb.attr_int("axis", 0)])
    t = gb.simple("Gather", [table("token_type_embeddings", types), type_ids], [pb.attr_int("axis", 0)]) if types else None
    p = None
    if pos == "const":
        rows = np.float32(table_mean) + np.float32(table_std) * rng.gaussish(seed, "position_embeddings", max_pos * dim).reshape(max_pos, dim)[:seq]
        p = gb.init("position_rows", rows.reshape(1, seq, dim).astype(np.float32))
    elif pos == "gather":
        pid = gb.init("position_ids", np.arange(max_pos, dtype=np.int64).reshape(1, max_pos))
        i64 = lambda name, v: gb.init(name, np.array(v, np.int64))  # noqa: E731
        sl = gb.simple("Slice", [pid, i64("pos_starts", [0]), i64("pos_ends", [seq]), i64("pos_axes", [1]), i64("pos_steps", [1])])
        p = gb.simple("Gather", [table("position_embeddings", max_pos), sl], [pb.attr_int("axis", 0)])
    elif pos is not None:
        raise ValueError(pos)
    parts = {"w": w, "t": t, "p": p}
    terms = [parts[k] for k in order if parts[k] is not None]
    if order == "ptw" and len(terms) == 3:
        x = gb.simple("Add", [terms[0], gb.simple("Add", [terms[1], terms[2]])])
    else:
        x = terms[0]
        for y in terms[1:]:
            x = gb.simple("Add", [x, y])
    return gb.layernorm(x, dim, eps=eps, name="emb_ln")


def bert_attention(gb: GraphBuilder, x: str, ext: str | None, dim: int, heads: int, tag: str, *, ktrans: str = "two", scale: str = "div",
                   mask_swap: bool = False, linear=None) -> str:
    """BertSelfAttention (eager): three Linears -> Reshape [N, L, H, hd] -> Transpose [0,2,1,3] (k: then [0,1,3,2] for ktrans "two", or the single
    [0,2,3,1] for "one") -> MatMul -> Div(sqrt hd) | Mul(1 / sqrt hd) -> Add(ext) (mask_swap: ext first) -> Softmax -> MatMul(., v) -> Transpose
    [0,2,1,3] -> Reshape [N, L, dim]"""
    hd = dim // heads
    shp = gb.init(tag + "_shape4", np.array([0, -1, heads, hd], np.int64))
    linear = linear or (lambda y, name: gb.linear(y, dim, dim, name=name))      # (tests pass Linears of their own)
    q, k, v = (gb.simple("Reshape", [linear(x, f"{tag}_{n}"), shp]) for n in ("query", "key", "value"))
    q, v = gb.transpose(q, (0, 2, 1, 3)), gb.transpose(v, (0, 2, 1, 3))
    kt = gb.transpose(gb.transpose(k, (0, 2, 1, 3)), (0, 1, 3, 2)) if ktrans == "two" else gb.transpose(k, (0, 2, 3, 1))
    s = gb.simple("MatMul", [q, kt])
    if scale == "div":
        s = gb.simple("Div", [s, gb.init(tag + "_sqrt_hd", np.array(np.sqrt(float(hd)), np.float32))])
    elif scale == "mul":
        s = gb.simple("Mul", [s, gb.init(tag + "_rsqrt_hd", np.array(1.0 / np.sqrt(float(hd)), np.float32))])
    else:
        raise ValueError(scale)
    if ext is not None:
        s = gb.simple("Add", [ext, s] if mask_swap else [s, ext])
    p = gb.simple("Softmax", [s], [pb.attr_int("axis", -1)])
    y = gb.transpose(gb.simple("MatMul", [p, v]), (0, 2, 1, 3))
    return gb.simple("Reshape", [y, gb.init(tag + "_shape3", np.array([0, -1, dim], np.int64))])


def bert_extended_mask(gb: GraphBuilder, mask: str = "attention_mask", *, mask_value: str | float = "min", unsqueeze: str = "two") -> str:
    """get_extended_attention_mask: Unsqueeze [1] -> Unsqueeze [2] (or one Unsqueeze [1, 2]) -> Cast FLOAT -> Sub(1.0, .) -> Mul(., c) = [N, 1, 1, L];
    c = finfo(float32).min ("min") or a float such as -10000.0"""
    c = FLOAT32_MIN if mask_value == "min" else float(mask_value)
    ax = lambda name, v: gb.init(name, np.array(v, np.int64))  # noqa: E731
    if unsqueeze == "two":
        m = gb.simple("Unsqueeze", [gb.simple("Unsqueeze", [mask, ax("mask_ax1", [1])]), ax("mask_ax2", [2])])
    elif unsqueeze == "one":
        m = gb.simple("Unsqueeze", [mask, ax("mask_ax12", [1, 2])])
    else:
        raise ValueError(unsqueeze)
    m = gb.simple("Cast", [m], [pb.attr_int("to", pb.FLOAT)])
    m = gb.simple("Sub", [gb.init("mask_one", np.array(1.0, np.float32)), m])
    return gb.simple("Mul", [m, gb.init("mask_value", np.array(c, np.float32))])


def bert(batch: int | str = 1, *, seq: int = 128, vocab: int = 30522, dim: int = 768, depth: int = 12, heads: int = 12, mlp: int = 3072,
         types: int = 2, max_pos: int = 512, classes: int = 2, mask_value: str | float = "min", eps: float = 1e-12, seed: int = 2018,
         pos: str | None = "const", order: str = "wtp", unsqueeze: str = "two", ktrans: str = "two", scale: str = "div", mask_swap: bool = False,
         mask: bool = True, pooler_output: bool = False, table_std: float = 1.0) -> bytes:
    """BertForSequenceClassification (post-LN encoder, Devlin et al. 2019) written from modeling_bert.py's eager attention and the TorchScript
    exporter's known lowerings at opset 17, as Swin's graph was: neither `transformers` nor ONNX Runtime is available to export or to run one, so the
    graph is this restatement, checked by two independent float64 evaluations (tests/ref64.py, tests/test_bert_plan.py).
    inputs input_ids, attention_mask, token_type_ids [N, seq] INT64; outputs logits [N, classes] and optionally pooler_output [N, dim]."""
    gb = GraphBuilder("bert", seed)
    x = bert_embeddings(gb, seq, vocab, dim, types=types, max_pos=max_pos, pos=pos, order=order, eps=eps, table_std=table_std)
    ext = bert_extended_mask(gb, mask_value=mask_value, unsqueeze=unsqueeze) if mask else None
    for li in range(depth):
        tag = f"l{li}"
        y = bert_attention(gb, x, ext, dim, heads, tag + "_attn", ktrans=ktrans, scale=scale, mask_swap=mask_swap)
        x = gb.layernorm(gb.simple("Add", [gb.linear(y, dim, dim, name=tag + "_out"), x]), dim, eps=eps, name=tag + "_ln1")
        y = gb.gelu(gb.linear(x, dim, mlp, name=tag + "_fc1"), "erf")
        x = gb.layernorm(gb.simple("Add", [gb.linear(y, mlp, dim, name=tag + "_fc2", w_scale=float(np.sqrt(2.0 / mlp))), x]), dim, eps=eps, name=tag + "_ln2")
    gb.nodes.append(pb.node("Constant", [], ["pool_i0"], "pool_i0", [pb.attr_int("value_int", 0)]))
    x = gb.simple("Gather", [x, "pool_i0"], [pb.attr_int("axis", 1)])

    def gemm(y: str, name: str, cin: int, cout: int, out: str | None = None) -> str:
        w = rng.gaussish(seed, name + "_w", cout * cin).reshape(cout, cin) * np.float32(np.sqrt(1.0 / cin))
        b = (rng.uniform(seed, name + "_b", cout) - np.float32(0.5)) * np.float32(0.2)
        return gb.simple("Gemm", [y, gb.init(name + "_w", w.astype(np.float32)), gb.init(name + "_b", b.astype(np.float32))], [pb.attr_int("transB", 1)], out=out)

    pooled = gb.simple("Tanh", [gemm(x, "pooler", dim, dim)], out="pooler_output" if pooler_output else None)
    gemm(pooled, "classifier", dim, classes, out="logits")
    ins = [("input_ids", [batch, seq], ONNX_INT64)] + ([("attention_mask", [batch, seq], ONNX_INT64)] if mask else []) + \
          ([("token_type_ids", [batch, seq], ONNX_INT64)] if types else [])
    outs = [("logits", [batch, classes])] + ([("pooler_output", [batch, dim])] if pooler_output else [])
    return gb.finish(ins, outs, opset=17)


def bert_base(batch: int | str = 1, **kw) -> bytes:
    return bert(batch, **dict(dict(seq=128, vocab=30522, dim=768, depth=12, heads=12, mlp=3072), **kw))


def bert_tiny(batch: int | str = 1, **kw) -> bytes:
    return bert(batch, **dict(dict(seq=128, vocab=30522, dim=128, depth=2, heads=2, mlp=512), **kw))


def causal_mask_constant(gb: GraphBuilder, seq: int, mask: str, max_pos: int, tag: str) -> str:
    """The causal mask of a GPT-2 attention as a name: "where_slice" GPT-2's `bias` buffer, BOOL tril [1, 1, max_pos, max_pos], cut to [1, 1, seq, seq]
    by two Slices (bias[:, :, key - query : key, :key]); "where_const" the BOOL tril [1, 1, seq, seq] itself; "add" the float mask [1, 1, seq, seq],
    0 on and below the diagonal and finfo(float32).min above it"""
    i64 = lambda name, v: gb.init(f"{tag}_{name}", np.array(v, np.int64))  # noqa: E731
    if mask == "where_slice":
        b = gb.init(tag + "_bias", np.tril(np.ones((max_pos, max_pos), np.bool_)).reshape(1, 1, max_pos, max_pos))
        b = gb.simple("Slice", [b, i64("q_starts", [0]), i64("q_ends", [seq]), i64("q_axes", [2]), i64("q_steps", [1])])
        return gb.simple("Slice", [b, i64("k_starts", [0]), i64("k_ends", [seq]), i64("k_axes", [3]), i64("k_steps", [1])])
    if mask == "where_const":
        return gb.init(tag + "_bias", np.tril(np.ones((seq, seq), np.bool_)).reshape(1, 1, seq, seq))
    if mask == "add":
        return gb.init(tag + "_mask", np.triu(np.full((seq, seq), FLOAT32_MIN, np.float32), 1).reshape(1, 1, seq, seq))
    raise ValueError(mask)


def chunk_causal_constant(gb: GraphBuilder, lq: int, past: int, tag: str, edit=None) -> str:
    """The constant _make_causal_mask gives for lq new tokens behind `past` cached rows: float [1, 1, lq, past + lq], 0 in the first `past` columns
    (every cached key is visible), in column past + j of row i 0 for j <= i and finfo(float32).min for j > i.  edit (i, j, value): one element
    overwritten (tests: a constant the planner refuses)"""
    c = np.zeros((lq, past + lq), np.float32)
    c[:, past:] = np.triu(np.full((lq, lq), FLOAT32_MIN, np.float32), 1)
    if edit is not None:
        c[edit[0], edit[1]] = edit[2]
    return gb.init(tag + "_mask", c.reshape(1, 1, lq, past + lq))


def chunk_causal_mask(gb: GraphBuilder, ext: str, lq: int, past: int, tag: str, *, form: str = "where", fill: float = FLOAT32_MIN, edit=None) -> str:
    """The 4-D mask of an extend step as AttentionMaskConverter.to_4d lowers it with a past: M = Where(Cast(ext, to=BOOL), finfo.min, C) [N, 1, lq,
    past + lq], ext = bert_extended_mask's [N, 1, 1, past + lq] chain (non-zero on a masked key), C = chunk_causal_constant (edit: its).  M holds only
    0 and finfo.min, never -inf.  form "add": Add(ext, C), which sums two finfo.min to -inf on a masked key of the future (a spelling the planner refuses)"""
    c = chunk_causal_constant(gb, lq, past, tag, edit)
    if form == "add":
        return gb.simple("Add", [ext, c])
    if form != "where":
        raise ValueError(form)
    cond = gb.simple("Cast", [ext], [pb.attr_int("to", pb.BOOL)])
    return gb.simple("Where", [cond, gb.init(tag + "_mask_fill", np.array(fill, np.float32)), c])


def gpt2_attention(gb: GraphBuilder, x: str, seq: int, dim: int, heads: int, tag: str, *, mask: str | None = "where_slice", scale: str = "div",
                   ktrans: str = "two", split_attr: bool = True, max_pos: int = 1024, linear=None, mask_swap: bool = False) -> str:
    """GPT2Attention (eager) behind its c_attn Linear: Split(axis 2) of the [N, L, 3 dim] rows (split_attr: the sizes as an input, else omitted as
    the exporter does for equal parts) -> per part Reshape [N, L, H, hd] -> Transpose [0,2,1,3] (k: then [0,1,3,2] for ktrans "two", or the single
    [0,2,3,1] for "one") -> MatMul -> Div(sqrt hd) | Mul(1 / sqrt hd) -> the causal mask (causal_mask_constant; Where(cond, scores, finfo.min) or
    Add(scores, M), mask_swap: M first; None: no mask) -> Softmax -> MatMul(., v) -> Transpose [0,2,1,3] -> Reshape [N, L, dim].  x: the c_attn result,
    or with `linear` the tokens it is applied to"""
    hd = dim // heads
    qkv = linear(x, tag + "_c_attn") if linear else x
    ins = [qkv] + ([gb.init(tag + "_split", np.array([dim, dim, dim], np.int64))] if split_attr else [])
    parts = [gb._uid(tag + "_part") for _ in range(3)]
    gb.nodes.append(pb.node("Split", ins, parts, tag + "_split_qkv", [pb.attr_int("axis", 2)]))
    shp = gb.init(tag + "_shape4", np.array([0, -1, heads, hd], np.int64))
    q, k, v = (gb.simple("Reshape", [p, shp]) for p in parts)
    q, v = gb.transpose(q, (0, 2, 1, 3)), gb.transpose(v, (0, 2, 1, 3))
    kt = gb.transpose(gb.transpose(k, (0, 2, 1, 3)), (0, 1, 3, 2)) if ktrans == "two" else gb.transpose(k, (0, 2, 3, 1))
    s = gb.simple("MatMul", [q, kt])
    if scale == "div":
        s = gb.simple("Div", [s, gb.init(tag + "_sqrt_hd", np.array(np.sqrt(float(hd)), np.float32))])
    elif scale == "mul":
        s = gb.simple("Mul", [s, gb.init(tag + "_rsqrt_hd", np.array(1.0 / np.sqrt(float(hd)), np.float32))])
    else:
        raise ValueError(scale)
    if mask in ("where_slice", "where_const"):
        s = gb.simple("Where", [causal_mask_constant(gb, seq, mask, max_pos, tag), s, gb.init(tag + "_mask_value", np.array(FLOAT32_MIN, np.float32))])
    elif mask is not None:
        m = causal_mask_constant(gb, seq, mask, max_pos, tag)
        s = gb.simple("Add", [m, s] if mask_swap else [s, m])
    p = gb.simple("Softmax", [s], [pb.attr_int("axis", -1)])
    y = gb.transpose(gb.simple("MatMul", [p, v]), (0, 2, 1, 3))
    return gb.simple("Reshape", [y, gb.init(tag + "_shape3", np.array([0, -1, dim], np.int64))])


def gelu_new(gb: GraphBuilder, x: str, form: str = "pow") -> str:
    """NewGELUActivation, 0.5 * x * (1 + tanh(sqrt(2 / pi) * (x + 0.044715 * x^3))), as the exporter writes it: "pow" with Pow(x, 3.0), "mulmul" with
    Mul(x, Mul(x, x)) in its place, "op" the opset-20 Gelu(approximate = "tanh")"""
    if form == "op":
        return gb.gelu(x, "op_tanh")
    name = gb._uid("gelu_new")
    c = lambda tag, v: gb.init(f"{name}_{tag}", np.array(v, np.float32))  # noqa: E731
    half = gb.simple("Mul", [x, c("half", 0.5)])
    if form == "pow":
        cube = gb.simple("Pow", [x, c("three", 3.0)])
    elif form == "mulmul":
        cube = gb.simple("Mul", [x, gb.simple("Mul", [x, x])])
    else:
        raise ValueError(form)
    inner = gb.simple("Add", [x, gb.simple("Mul", [cube, c("c2", 0.044715)])])
    t = gb.simple("Tanh", [gb.simple("Mul", [inner, c("c1", np.sqrt(2.0 / np.pi))])])
    return gb.simple("Mul", [half, gb.simple("Add", [t, c("one", 1.0)])])


def gpt2(batch: int | str = 1, *, seq: int = 128, vocab: int = 50257, dim: int = 768, depth: int = 12, heads: int = 12, mlp: int = 3072,
         max_pos: int = 1024, eps: float = 1e-5, seed: int = 2019, mask: str | None = "where_slice", scale: str = "div", ktrans: str = "two",
         linear: str = "conv1d", gelu: str = "pow", lm_head: str = "transpose", split_attr: bool = True, pos: str = "gather", logits: bool = True,
         last_hidden_state: bool = False, table_std: float = 1.0) -> bytes:
    """GPT2LMHeadModel as a prefill / scoring forward (pre-LN decoder, Radford et al. 2019), ids [N, seq] -> logits [N, seq, vocab], written from
    modeling_gpt2.py's eager attention and the TorchScript exporter's known lowerings, not from a real export (neither `transformers` nor ONNX
    Runtime is available here); checked by the float64 walk of tests/ref64.py.  The switches are the spellings the planner accepts:
      mask     "where_slice" | "where_const" | "add" (causal_mask_constant), None: the same graph without the mask
      linear   "conv1d" HF's Conv1D, Reshape [-1, D] -> Gemm -> Reshape [N, L, Dout]; "matmul" MatMul + Add
      gelu     "pow" | "mulmul" | "op" (gelu_new);  lm_head  "transpose" Transpose(wte, [1,0]) (the tied head) | "init" a [dim, vocab] initializer
      pos      "gather" Gather(wpe, Slice(position_ids)) | "const" the [1, seq, dim] rows;  split_attr: Split with its sizes, or without
    outputs: logits (optional), last_hidden_state [N, seq, dim] behind ln_f (optional; the engine takes it beside the logits, whose head reads it)"""
    gb = GraphBuilder("gpt2", seed)
    wte = np.float32(table_std) * rng.gaussish(seed, "wte", vocab * dim).reshape(vocab, dim).astype(np.float32)
    wpe = np.float32(table_std) * rng.gaussish(seed, "wpe", max_pos * dim).reshape(max_pos, dim).astype(np.float32)
    x = gb.simple("Gather", [gb.init("wte", wte), "input_ids"], [pb.attr_int("axis", 0)])
    if pos == "gather":
        i64 = lambda name, v: gb.init(name, np.array(v, np.int64))  # noqa: E731
        pid = gb.simple("Slice", [gb.init("position_ids", np.arange(max_pos, dtype=np.int64).reshape(1, max_pos)), i64("pos_starts", [0]), i64("pos_ends", [seq]),
                                  i64("pos_axes", [1]), i64("pos_steps", [1])])
        p = gb.simple("Gather", [gb.init("wpe", wpe), pid], [pb.attr_int("axis", 0)])
    elif pos == "const":
        p = gb.init("position_rows", wpe[:seq].reshape(1, seq, dim))
    else:
        raise ValueError(pos)
    x = gb.simple("Add", [x, p])

    def lin(y: str, name: str, cin: int, cout: int, w_scale: float | None = None) -> str:
        w = rng.gaussish(seed, name + "_w", cin * cout).reshape(cin, cout) * np.float32(w_scale if w_scale is not None else np.sqrt(1.0 / cin))
        b = (rng.uniform(seed, name + "_b", cout) - np.float32(0.5)) * np.float32(0.2)
        wn, bn = gb.init(name + "_w", w.astype(np.float32)), gb.init(name + "_b", b.astype(np.float32))
        if linear == "matmul":
            return gb.simple("Add", [gb.simple("MatMul", [y, wn]), bn])
        if linear != "conv1d":
            raise ValueError(linear)
        flat = gb.simple("Reshape", [y, gb.init(name + "_flat", np.array([-1, cin], np.int64))])
        g = gb.simple("Gemm", [flat, wn, bn], [pb.attr_float("alpha", 1.0), pb.attr_float("beta", 1.0)])
        return gb.simple("Reshape", [g, gb.init(name + "_back", np.array([-1 if isinstance(batch, str) else batch, seq, cout], np.int64))])

    for li in range(depth):
        tag = f"h{li}"
        y = gpt2_attention(gb, lin(gb.layernorm(x, dim, eps=eps, name=tag + "_ln_1"), tag + "_c_attn", dim, 3 * dim), seq, dim, heads, tag + "_attn",
                           mask=mask, scale=scale, ktrans=ktrans, split_attr=split_attr, max_pos=max_pos)
        x = gb.simple("Add", [lin(y, tag + "_c_proj", dim, dim), x])
        y = gelu_new(gb, lin(gb.layernorm(x, dim, eps=eps, name=tag + "_ln_2"), tag + "_c_fc", dim, mlp), gelu)
        x = gb.simple("Add", [x, lin(y, tag + "_mlp_proj", mlp, dim, w_scale=float(np.sqrt(2.0 / mlp)))])
    gb.nodes.append(pb.node("LayerNormalization", [x, gb.init("ln_f_g", np.ones(dim, np.float32)), gb.init("ln_f_b", np.zeros(dim, np.float32))],
                            ["last_hidden_state"], "ln_f", [pb.attr_int("axis", -1), pb.attr_float("epsilon", eps)]))
    if logits:
        head = gb.transpose("wte", (1, 0)) if lm_head == "transpose" else gb.init("lm_head_w", np.ascontiguousarray(wte.T))
        if lm_head not in ("transpose", "init"):
            raise ValueError(lm_head)
        gb.simple("MatMul", ["last_hidden_state", head], out="logits")
    outs = ([("logits", [batch, seq, vocab])] if logits else []) + ([("last_hidden_state", [batch, seq, dim])] if last_hidden_state or not logits else [])
    return gb.finish([("input_ids", [batch, seq], ONNX_INT64)], outs, opset=20 if gelu == "op" else 17)


def gpt2_small(batch: int | str = 1, **kw) -> bytes:
    return gpt2(batch, **dict(dict(seq=128, vocab=50257, dim=768, depth=12, heads=12, mlp=3072, max_pos=1024), **kw))


def gpt2_tiny(batch: int | str = 1, **kw) -> bytes:
    return gpt2(batch, **dict(dict(seq=40, vocab=61, dim=128, depth=2, heads=2, mlp=256, max_pos=64), **kw))


INT64_MAX = 9223372036854775807


def rope_tables(seq: int, hd: int, theta: float = 10000.0) -> tuple[np.ndarray, np.ndarray]:
    """LlamaRotaryEmbedding's cos / sin [seq, hd] in fp32: angle[i, e] = i * theta^(-2 (e mod hd/2) / hd), emb = cat(freqs, freqs)"""
    inv = 1.0 / (theta ** (np.arange(0, hd, 2, dtype=np.float64) / hd))
    ang = np.arange(seq, dtype=np.float64)[:, None] * inv[None, :]
    emb = np.concatenate([ang, ang], axis=1)
    return np.cos(emb).astype(np.float32), np.sin(emb).astype(np.float32)


def rope_constants(gb: GraphBuilder, seq: int, hd: int, tag: str, *, form: str = "init", max_pos: int | None = None, theta: float = 10000.0,
                   tables: tuple[np.ndarray, np.ndarray] | None = None) -> tuple[str, str]:
    """The names of cos and sin as an attention reads them, broadcasting as [1, 1, seq, hd]: "init" initializers of that shape; "unsqueeze" [seq, hd]
    initializers behind Unsqueeze(axes [0, 1]); "slice" [max_pos, hd] tables cut to their first seq rows by a Slice and then unsqueezed; "gather"
    the tables gathered by the constant positions 0 ... seq - 1 and then unsqueezed.  tables: (cos, sin) [rows, hd] given instead of rope_tables"""
    rows = seq if form in ("init", "unsqueeze") else (max_pos or seq)
    cs = tables if tables is not None else rope_tables(rows, hd, theta)
    out = []
    i64 = lambda name, v: gb.init(f"{tag}_{name}", np.array(v, np.int64))  # noqa: E731
    for which, t in zip(("cos", "sin"), cs):
        t = np.ascontiguousarray(t, np.float32)
        if form == "init":
            out.append(gb.init(f"{tag}_{which}", t[:seq].reshape(1, 1, seq, hd)))
            continue
        name = gb.init(f"{tag}_{which}_table", t)
        if form == "slice":
            name = gb.simple("Slice", [name, i64(which + "_starts", [0]), i64(which + "_ends", [seq]), i64(which + "_axes", [0]), i64(which + "_steps", [1])])
        elif form == "gather":
            name = gb.simple("Gather", [name, i64(which + "_positions", np.arange(seq))], [pb.attr_int("axis", 0)])
        elif form != "unsqueeze":
            raise ValueError(form)
        out.append(gb.simple("Unsqueeze", [name, i64(which + "_axes01", [0, 1])]))
    return out[0], out[1]


def rotate_half_rope(gb: GraphBuilder, t: str, cos: str, sin: str, hd: int, tag: str, *, swap: bool = False, order: str = "neg_first",
                     out: str | None = None) -> str:
    """apply_rotary_pos_emb on t [N, H, L, hd]: Add(Mul(t, cos), Mul(Concat(Neg(Slice(t, hd/2:)), Slice(t, :hd/2), axis -1), sin)); swap: every Mul /
    Add with its operands the other way round.  order "x1_first": the Concat as (x1, -x2), which is NOT rotate_half (tests: a refusal).  out: the
    result's name"""
    i64 = lambda name, v: gb.init(f"{tag}_{name}", np.array(v, np.int64))  # noqa: E731
    two = lambda a, b: [b, a] if swap else [a, b]  # noqa: E731
    x1 = gb.simple("Slice", [t, i64("lo_starts", [0]), i64("lo_ends", [hd // 2]), i64("lo_axes", [-1]), i64("lo_steps", [1])])
    x2 = gb.simple("Slice", [t, i64("hi_starts", [hd // 2]), i64("hi_ends", [INT64_MAX]), i64("hi_axes", [-1]), i64("hi_steps", [1])])
    if order == "neg_first":
        rot = gb.simple("Concat", [gb.simple("Neg", [x2]), x1], [pb.attr_int("axis", -1)])
    elif order == "x1_first":
        rot = gb.simple("Concat", [x1, gb.simple("Neg", [x2])], [pb.attr_int("axis", -1)])
    else:
        raise ValueError(order)
    return gb.simple("Add", two(gb.simple("Mul", two(t, cos)), gb.simple("Mul", two(rot, sin))), out=out)


def rope_gathered(gb: GraphBuilder, hd: int, tag: str, *, max_pos: int, theta: float = 10000.0, tables: tuple[np.ndarray, np.ndarray] | None = None,
                  positions: str = "position_ids") -> tuple[str, str]:
    """cos and sin of a decode step whose positions are run-time data: Unsqueeze(Gather(table [max_pos, hd], positions [N, Lq], axis 0), axes [1]),
    which broadcasts as [N, 1, Lq, hd] (LlamaRotaryEmbedding on position_ids, as the exporter lowers it).  tables: (cos, sin) [max_pos, hd] given
    instead of rope_tables"""
    cs = tables if tables is not None else rope_tables(max_pos, hd, theta)
    out = []
    for which, t in zip(("cos", "sin"), cs):
        name = gb.init(f"{tag}_{which}_table", np.ascontiguousarray(t, np.float32))
        g = gb.simple("Gather", [name, positions], [pb.attr_int("axis", 0)])
        out.append(gb.simple("Unsqueeze", [g, gb.init(f"{tag}_{which}_axes1", np.array([1], np.int64))]))
    return out[0], out[1]


def llama_attention(gb: GraphBuilder, x: str, seq: int, dim: int, heads: int, kv_heads: int, tag: str, *, batch: int = 1, rope: tuple[str, str] | None = None,
                    rope_k: tuple[str, str] | None = None, repeat: str = "auto", mask: str | None = "add", scale: str = "mul", bias: bool = False,
                    swap: bool = False, linear=None, rope_order: str = "neg_first", hd: int | None = None, past: tuple[str, str] | None = None,
                    past_len: int = 0, present: tuple[str, str] | None = None, key_mask: str | None = None, concat_order: str = "past_first",
                    present_after_repeat: bool = False) -> str:
    """LlamaAttention (eager): q / k / v Linears without a bias (dim -> H hd, Hkv hd, Hkv hd) -> Reshape [N, L, H | Hkv, hd] -> Transpose [0,2,1,3] ->
    rotary embedding on q and k (rope = the (cos, sin) names of rope_constants; rope_k: other names for k; None: no rotation) -> repeat_kv on k and v
    (Unsqueeze(axis 2) -> Expand [N, Hkv, g, L, hd] -> Reshape [N, H, L, hd]; repeat "auto": where g > 1, "always": also the g = 1 no-op, "never")
    -> MatMul(q, Transpose(k, [0,1,3,2])) -> Mul(1 / sqrt hd) | Div(sqrt hd) -> the causal mask ("add" the additive triangular constant, "where_const",
    None) -> Softmax -> MatMul(., v) -> Transpose [0,2,1,3] -> Reshape [N, L, H hd].  x: the tokens, or with `linear` = a function (x, name, cout)
    the q / k / v rows come from it (tests hand the kernel known operands that way).
    With a cache (modeling_llama.py's eager attention with DynamicCache.update, as the exporter lowers it): past = the names of the cached K / V inputs
    [N, Hkv, past_len, hd]: K = Concat(past k, rope(k), axis 2) and V = Concat(past v, v, axis 2) in front of repeat_kv, which then expands
    past_len + seq keys; present = the names these values (without a past: rope(k) and the transposed v) get, for the graph's `present.*` outputs;
    key_mask = the name of the additive [N, 1, 1, past_len + seq] mask (bert_extended_mask) put on the scores in place of the triangular constant.
    concat_order "new_first" and present_after_repeat are spellings the planner refuses (tests)"""
    hd = hd or dim // heads
    g = heads // max(kv_heads, 1)
    lin = linear or (lambda y, name, cout: gb.linear(y, dim, cout, name=name, bias=bias))
    i64 = lambda name, v: gb.init(f"{tag}_{name}", np.array(v, np.int64))  # noqa: E731
    q = gb.simple("Reshape", [lin(x, tag + "_q_proj", heads * hd), i64("shape_q", [0, -1, heads, hd])])
    k = gb.simple("Reshape", [lin(x, tag + "_k_proj", kv_heads * hd), i64("shape_k", [0, -1, kv_heads, hd])])
    v = gb.simple("Reshape", [lin(x, tag + "_v_proj", kv_heads * hd), i64("shape_v", [0, -1, kv_heads, hd])])
    # (a prefill's present: the rotated k -- without rope its Transpose -- and the transposed v carry the output names themselves)
    pk, pv = present if present is not None and past is None and not present_after_repeat else (None, None)
    tr = lambda t, out=None: gb.simple("Transpose", [t], [pb.attr_ints("perm", [0, 2, 1, 3])], out=out)  # noqa: E731
    q, k, v = tr(q), tr(k, None if rope is not None else pk), tr(v, pv)
    if rope is not None:
        q = rotate_half_rope(gb, q, rope[0], rope[1], hd, tag + "_rope_q", swap=swap, order=rope_order)
        kc = rope_k or rope
        k = rotate_half_rope(gb, k, kc[0], kc[1], hd, tag + "_rope_k", swap=swap, out=pk)
    kv_seq = seq + (past_len if past is not None else 0)
    if past is not None:
        names = present if present is not None and not present_after_repeat else (None, None)
        two = (lambda a, b: [b, a]) if concat_order == "new_first" else (lambda a, b: [a, b])
        k = gb.simple("Concat", two(past[0], k), [pb.attr_int("axis", 2)], out=names[0])
        v = gb.simple("Concat", two(past[1], v), [pb.attr_int("axis", 2)], out=names[1])
    if repeat == "always" or (repeat == "auto" and g > 1):
        def repeat_kv(t: str, which: str) -> str:
            u = gb.simple("Unsqueeze", [t, i64(which + "_rep_axis", [2])])
            e = gb.simple("Expand", [u, i64(which + "_rep_shape5", [batch, kv_heads, g, kv_seq, hd])])
            return gb.simple("Reshape", [e, i64(which + "_rep_shape4", [batch, heads, kv_seq, hd])], out=present[0 if which == "k" else 1] if present_after_repeat and present else None)
        k, v = repeat_kv(k, "k"), repeat_kv(v, "v")
    elif repeat not in ("auto", "never"):
        raise ValueError(repeat)
    s = gb.simple("MatMul", [q, gb.transpose(k, (0, 1, 3, 2))])
    if scale == "mul":
        s = gb.simple("Mul", [s, gb.init(tag + "_rsqrt_hd", np.array(1.0 / np.sqrt(float(hd)), np.float32))])
    elif scale == "div":
        s = gb.simple("Div", [s, gb.init(tag + "_sqrt_hd", np.array(np.sqrt(float(hd)), np.float32))])
    else:
        raise ValueError(scale)
    if key_mask is not None:
        s = gb.simple("Add", [s, key_mask])
    elif mask == "where_const":
        s = gb.simple("Where", [causal_mask_constant(gb, seq, mask, seq, tag), s, gb.init(tag + "_mask_value", np.array(FLOAT32_MIN, np.float32))])
    elif mask is not None:
        s = gb.simple("Add", [s, causal_mask_constant(gb, seq, mask, seq, tag)])
    p = gb.simple("Softmax", [s], [pb.attr_int("axis", -1)])
    y = gb.transpose(gb.simple("MatMul", [p, v]), (0, 2, 1, 3))
    return gb.simple("Reshape", [y, i64("shape3", [0, -1, heads * hd])])


def llama(batch: int = 1, *, seq: int = 128, vocab: int = 32000, dim: int = 576, depth: int = 30, heads: int = 9, kv_heads: int = 3, mlp: int = 1536,
          max_pos: int = 2048, rope_theta: float = 10000.0, eps: float = 1e-5, tied: bool = True, last_hidden_state: bool = False, seed: int = 2023,
          norm: str = "pow", cast: bool = False, swap: bool = False, rope: str = "slice", repeat: str = "auto", scale: str = "mul", mask: str = "add",
          w_scale: float | None = None, table_std: float = 1.0, present: bool = False, past: int | None = None, positions: str = "input") -> bytes:
    """LlamaForCausalLM as a prefill / scoring forward (Touvron et al. 2023; the shape of Llama 2 / 3, TinyLlama, SmolLM, Mistral and the dense Qwen
    models), ids [N, seq] -> logits [N, seq, vocab], written from modeling_llama.py's eager attention and the TorchScript exporter's known lowerings,
    NOT from a real export (neither `transformers` nor ONNX Runtime is available here); checked by the float64 walk of tests/ref64.py.
    Per layer: x += o_proj(attention(RMSNorm(x))) with rotary q / k and kv_heads grouped K / V heads (llama_attention), x += down(SiLU(gate(h)) * up(h))
    with h = RMSNorm(x); then the final RMSNorm and the vocabulary head (tied: Transpose(embed_tokens, [1,0])).  No Linear has a bias; attention_mask is
    not an input (the causal mask is the additive triangular constant).  The switches are the spellings the planner accepts:
      norm / cast / swap   GraphBuilder.rmsnorm's form, its Cast nodes, its operand order (swap also turns the rope's and the gated unit's Muls)
      rope     rope_constants' form: "init" | "unsqueeze" | "slice" | "gather" ("none": the same graph without the rope nodes, which is no Llama);  repeat: llama_attention's repeat_kv ("auto" | "always" | "never")
      scale    "mul" | "div";  mask: "add" | "where_const"
    outputs: logits, and last_hidden_state [N, seq, dim] behind the final norm (optional)
    The two halves of generation, both default off (the bytes of every graph above are then unchanged); like the prefill graph they are written from
    modeling_llama.py's eager attention -- here with DynamicCache -- and the exporter's known lowerings, not from a real export:
      present=True   prefill with a cache: per layer the outputs present.{i}.key (the rotated k; without rope its Transpose [0,2,1,3]) and
                     present.{i}.value (v's Transpose), both [N, Hkv, seq, hd], the values in front of repeat_kv; the rest of the graph is unchanged
      past=P         one decode step (seq is 1) over a cache of capacity P >= 1: inputs input_ids [N, 1], attention_mask [N, P + 1] INT64 (mask "input",
                     which "add" means here too; None: no mask input), position_ids [N, 1] INT64 (positions "input"; "const": none, the rotation
                     is row P of the tables in the form `rope` names) and per layer past_key_values.{i}.key / .value FLOAT [N, Hkv, P, hd].  Per layer
                     K = Concat(past key, rope(k), axis 2), V = Concat(past value, v, axis 2), both outputs present.{i}.* [N, Hkv, P + 1, hd] and both
                     read by repeat_kv; cos / sin = Unsqueeze(Gather(table [max_pos, hd], position_ids, axis 0), axes [1]); the mask is BERT's chain
                     Mul(Sub(1, Cast(Unsqueeze(attention_mask, [1, 2]))), finfo.min) added to the scores [N, H, 1, P + 1] (no triangular constant at
                     one query).  The client writes the last row of present.* into its cache at row `len`; valid rows may sit anywhere in the cache
      past=P, seq=Lq >= 2   an extend step (chunked prefill into a cache, the next turn of a conversation, scoring Lq drafted tokens): input_ids
                     [N, Lq], attention_mask [N, P + Lq], position_ids [N, Lq] (every token's own table row) and the same past inputs; logits
                     [N, Lq, V] and present.{i}.* [N, Hkv, P + Lq, hd].  K / V and cos / sin as in the decode graph (rope_gathered takes [N, Lq]
                     positions).  The mask is one model-level value, as AttentionMaskConverter.to_4d lowers it with a past: M = Where(Cast(ext, to=BOOL),
                     finfo.min, C) [N, 1, Lq, P + Lq] with ext the chain above and C = chunk_causal_constant (0 on the P cached columns, the causal
                     triangle of finfo.min on the Lq new ones); every layer adds M to its scores.  M holds only 0 and finfo.min, never -inf.  Causality
                     inside the chunk goes by chunk index, not by position_ids.  The client writes rows P .. P + Lq - 1 of present.* into its cache at
                     row `len`; right- and left-padded caches both work.  A ragged batch pads the chunk on the right with the padded tokens' own mask
                     columns 0: the output rows of such tokens are finite and otherwise unspecified (the graph gives a uniform average there, and
                     nobody reads it)"""
    gb = GraphBuilder("llama", seed)
    hd = dim // heads
    emb = np.float32(table_std) * rng.gaussish(seed, "embed_tokens", vocab * dim).reshape(vocab, dim).astype(np.float32)
    x = gb.simple("Gather", [gb.init("embed_tokens", emb), "input_ids"], [pb.attr_int("axis", 0)])
    ext = None
    if past is not None:
        if past < 1 or seq < 1:
            raise ValueError("a graph with a cache has past >= 1 cached rows and seq >= 1 new tokens")
        if mask in ("add", "input"):
            ext = bert_extended_mask(gb, unsqueeze="one")
        elif mask is not None:
            raise ValueError(mask)
        if seq > 1:
            if ext is None or rope == "none" or positions != "input":
                raise ValueError("an extend graph (past with seq > 1) has the attention_mask and position_ids inputs: without the mask its new tokens would see each other's future")
            ext = chunk_causal_mask(gb, ext, seq, past, "chunk")
        if rope == "none":
            cs = None
        elif positions == "input":
            cs = rope_gathered(gb, hd, "rotary", max_pos=max_pos, theta=rope_theta)
        elif positions == "const":
            full = rope_tables(max_pos, hd, rope_theta)
            cs = rope_constants(gb, 1, hd, "rotary", form=rope, tables=(full[0][past:past + 1], full[1][past:past + 1]))
        else:
            raise ValueError(positions)
    else:
        cs = rope_constants(gb, seq, hd, "rotary", form=rope, max_pos=max_pos, theta=rope_theta) if rope != "none" else None      # ("none": measurements only)
    opset = 23 if norm == "op" else 18

    def lin(y: str, name: str, cin: int, cout: int) -> str:
        return gb.linear(y, cin, cout, name=name, bias=False, w_scale=w_scale)

    for li in range(depth):
        tag = f"layers{li}"
        h = gb.rmsnorm(x, dim, eps=eps, form=norm, name=tag + "_input_layernorm", cast=cast, swap=swap)
        kv = {}
        if past is not None:
            kv = dict(past=(f"past_key_values.{li}.key", f"past_key_values.{li}.value"), past_len=past, key_mask=ext)
        if present or past is not None:
            kv["present"] = (f"present.{li}.key", f"present.{li}.value")
        y = llama_attention(gb, h, seq, dim, heads, kv_heads, tag + "_attn", batch=batch, rope=cs, repeat=repeat, scale=scale, mask=None if past is not None else mask,
                            swap=swap, linear=lambda t, name, cout: lin(t, name, dim, cout), **kv)
        x = gb.simple("Add", [x, lin(y, tag + "_o_proj", dim, dim)])
        h = gb.rmsnorm(x, dim, eps=eps, form=norm, name=tag + "_post_attention_layernorm", cast=cast, swap=swap)
        y = gb.swiglu(lin(h, tag + "_gate_proj", dim, mlp), lin(h, tag + "_up_proj", dim, mlp), swap=swap)
        x = gb.simple("Add", [x, lin(y, tag + "_down_proj", mlp, dim)])
    gb.rmsnorm(x, dim, eps=eps, form=norm, name="norm", cast=cast, swap=swap, out="last_hidden_state")
    head = gb.transpose("embed_tokens", (1, 0)) if tied else gb.init("lm_head_w", (rng.gaussish(seed, "lm_head", dim * vocab).reshape(dim, vocab) * np.float32(np.sqrt(1.0 / dim))).astype(np.float32))
    gb.simple("MatMul", ["last_hidden_state", head], out="logits")
    outs = [("logits", [batch, seq, vocab])] + ([("last_hidden_state", [batch, seq, dim])] if last_hidden_state else [])
    ins = [("input_ids", [batch, seq], ONNX_INT64)]
    if present or past is not None:
        rows = seq + (past or 0)
        for li in range(depth):
            outs += [(f"present.{li}.key", [batch, kv_heads, rows, hd]), (f"present.{li}.value", [batch, kv_heads, rows, hd])]
    if past is not None:
        ins += [("attention_mask", [batch, past + seq], ONNX_INT64)] if ext is not None else []
        ins += [("position_ids", [batch, seq], ONNX_INT64)] if cs is not None and positions == "input" else []
        for li in range(depth):
            ins += [(f"past_key_values.{li}.key", [batch, kv_heads, past, hd]), (f"past_key_values.{li}.value", [batch, kv_heads, past, hd])]
    return gb.finish(ins, outs, opset=opset)


def llama_135m(batch: int = 1, **kw) -> bytes:
    """SmolLM-135M's shape: 30 layers, dim 576, 9 heads of 64 over 3 K / V heads, mlp 1536, vocab 49152, tied head"""
    return llama(batch, **dict(dict(seq=128, vocab=49152, dim=576, depth=30, heads=9, kv_heads=3, mlp=1536, max_pos=2048), **kw))


def llama_3b_layers(batch: int = 1, depth: int = 2, **kw) -> bytes:
    """`depth` decoder layers of Llama-3.2-3B's shape: dim 3072, 24 heads of 128 over 8 K / V heads, mlp 8192, rope theta 500 000, behind a small
    vocabulary (1024 ids), for measurements of the layer: a layer is 101 M weights, so two of them serialize to 0.8 GB, well under protobuf's 2 GB,
    which the 28 layers and the 128 256-id embedding of the whole model are not"""
    return llama(batch, **dict(dict(seq=128, vocab=1024, dim=3072, depth=depth, heads=24, kv_heads=8, mlp=8192, max_pos=2048, rope_theta=500000.0), **kw))


def llama_tiny(batch: int = 1, **kw) -> bytes:
    return llama(batch, **dict(dict(seq=40, vocab=61, dim=128, depth=2, heads=4, kv_heads=2, mlp=256, max_pos=64), **kw))


def swin_relative_position_bias(seed: int, tag: str, window: Sequence[int], heads: int) -> np.ndarray:
    """torchvision's relative-position bias of one block, [1, heads, L, L]: a table [(2 wh - 1)(2 ww - 1), heads] gathered by the relative-position
    index of every (query, key) pair of a window.  The table is an O(1) draw, not 0.02 N(0,1): a dropped bias must move the logits."""
    wh, ww = window
    L = wh * ww
    table = rng.gaussish(seed, tag + "_rpb_table", (2 * wh - 1) * (2 * ww - 1) * heads).reshape(-1, heads)
    coords = np.stack(np.meshgrid(np.arange(wh), np.arange(ww), indexing="ij")).reshape(2, L)
    rel = (coords[:, :, None] - coords[:, None, :]).transpose(1, 2, 0).copy()
    rel[:, :, 0] += wh - 1
    rel[:, :, 1] += ww - 1
    rel[:, :, 0] *= 2 * ww - 1
    index = rel.sum(-1).reshape(-1)
    return np.ascontiguousarray(table[index].reshape(L, L, heads).transpose(2, 0, 1)[None], np.float32)


def swin_shift_mask(hw: Sequence[int], window: Sequence[int], shift: Sequence[int]) -> np.ndarray:
    """torchvision's shift mask [nW, L, L] (0 / -100) from its three-slice region labelling of the rolled map"""
    (H, W), (wh, ww), (sh, sw) = hw, window, shift
    lab = np.zeros((H, W), np.float32)
    count = 0
    for h in ((0, -wh), (-wh, -sh), (-sh, None)):
        for w in ((0, -ww), (-ww, -sw), (-sw, None)):
            lab[h[0]:h[1], w[0]:w[1]] = count
            count += 1
    lab = lab.reshape(H // wh, wh, W // ww, ww).transpose(0, 2, 1, 3).reshape(-1, wh * ww)
    d = lab[:, None, :] - lab[:, :, None]
    return np.where(d != 0, np.float32(-100.0), np.float32(0.0)).astype(np.float32)


def swin_window_attention(gb: GraphBuilder, x: str, dim: int, heads: int, hw: Sequence[int], window: Sequence[int], shift: Sequence[int],
                          batch: int | str, tag: str, *, pad: bool = False, mask: str = "init", unbind: str = "gather", scale: str = "q",
                          swap: bool = False, linear: bool = True, tweak: dict | None = None) -> str:
    """torchvision's shifted_window_attention on a channels-last map x [N, H, W, dim] (linear = False: [N, H, W, 3 dim], no Linears) as the
    TorchScript exporter lowers it: [Pad with zero pads] -> roll by -shift (per dim two Slices and a Concat) -> Reshape [N, H/wh, wh, W/ww, ww, C] ->
    Transpose [0,1,3,2,4,5] -> Reshape [N nW, L, C] -> qkv Linear -> the attention of vit_attention with Add bias [1, heads, L, L] and, in shifted
    blocks, Reshape [N, nW, heads, L, L] -> Add mask [1, nW, 1, L, L] -> Reshape [N nW, heads, L, L] in front of the Softmax -> proj Linear ->
    Reshape [N, H/wh, W/ww, wh, ww, C] -> Transpose [0,1,3,2,4,5] -> Reshape [N, H, W, C] -> roll by +shift [-> the identity Slice of the padding].
    The caller has already set a dim's shift to 0 where the window covers the map.  Batch-dependent shape entries are -1 for a symbolic batch.
    mask: "init" ([1, nW, 1, L, L] initializer) or "unsqueeze" ([nW, L, L] behind two Unsqueeze nodes).  unbind / scale / swap: as vit_attention.
    tweak: near misses for the tests (keys: pad_value, back_shift, back_axes, rev_window, rev_perm, bias_heads, bias_l, mask_nw, mask_l, mask_heads,
    second_reader, mask_without_roll, roll_without_mask, reverse_roll)."""
    tw = dict(tweak or {})
    (H, W), (wh, ww), (sh, sw) = hw, window, shift
    L, nW, hd = wh * ww, (H // wh) * (W // ww), dim // heads
    sym = not isinstance(batch, int)
    nb, nbw = (-1, -1) if sym else (batch, batch * nW)
    cin = dim if linear else 3 * dim

    def i64(name: str, v: Sequence[int]) -> str:
        return gb.init(f"{tag}_{name}", np.array(list(v), np.int64))

    def roll(y: str, sign: int, which: str, shifts: Sequence[int], axes: Sequence[int] = (1, 2)) -> str:
        for d, s in zip(axes, shifts):
            if s == 0:
                continue
            s = sign * s * (-1 if tw.get("reverse_roll") else 1)        # roll by -shift: x[s:] ++ x[:s]; roll by +shift: x[-s:] ++ x[:-s]
            a = gb.simple("Slice", [y, i64(f"{which}{d}_s0", [s]), i64(f"{which}{d}_e0", [INT64_MAX]), i64(f"{which}{d}_a0", [d])])
            b = gb.simple("Slice", [y, i64(f"{which}{d}_s1", [0]), i64(f"{which}{d}_e1", [s]), i64(f"{which}{d}_a1", [d])])
            y = gb.concat([a, b], axis=d)
        return y

    def const(name: str, v: float) -> str:
        return gb.init(f"{tag}_{name}", np.array(v, np.float32))

    def mul(a: str, k: str) -> str:
        return gb.simple("Mul", [k, a] if swap else [a, k])

    shifted = (sh != 0 or sw != 0)
    y = x
    if pad:
        pads = [0] * 8
        if "pad_value" in tw:
            pads[6] = int(tw["pad_value"])          # W's end pad
        y = gb.simple("Pad", [y, i64("pads", pads)], [pb.attr_str("mode", "constant")])
    if shifted and not tw.get("mask_without_roll"):
        y = roll(y, 1, "roll", (sh, sw))
    y = gb.simple("Reshape", [y, i64("part6", [nb, H // wh, wh, W // ww, ww, cin])])
    y = gb.transpose(y, (0, 1, 3, 2, 4, 5))
    y = gb.simple("Reshape", [y, i64("part3", [nbw, L, cin])])
    if linear:
        y = gb.linear(y, dim, 3 * dim, name=tag + "_qkv")
    y = gb.simple("Reshape", [y, i64("shape5", [nbw, L, 3, heads, hd])])
    y = gb.transpose(y, (2, 0, 3, 1, 4))
    if unbind == "gather":
        parts = []
        for i in range(3):
            idx = f"{tag}_i{i}"
            gb.nodes.append(pb.node("Constant", [], [idx], idx, [pb.attr_int("value_int", i)]))
            parts.append(gb.simple("Gather", [y, idx], [pb.attr_int("axis", 0)]))
    elif unbind == "split":
        name = gb._uid("split")
        outs = [f"{name}_out{i}" for i in range(3)]
        gb.nodes.append(pb.node("Split", [y, i64("split", [1, 1, 1])], outs, name, [pb.attr_int("axis", 0)]))
        ax = i64("axes0", [0])
        parts = [gb.simple("Squeeze", [o, ax]) for o in outs]
    else:
        raise ValueError(unbind)
    q, k, v = parts
    c = float(hd) ** -0.5
    if scale == "q":
        q = mul(q, const("scale", c))
    elif scale == "sdpa":
        q = mul(q, const("sqrt_scale_q", np.sqrt(c)))
    kt = gb.transpose(k, (0, 1, 3, 2))
    if scale == "sdpa":
        kt = mul(kt, const("sqrt_scale_k", np.sqrt(c)))
    s = gb.simple("MatMul", [q, kt])
    if scale == "s_mul":
        s = mul(s, const("scale", c))
    elif scale == "s_div":
        s = gb.simple("Div", [s, const("inv_scale", 1.0 / c)])
    elif scale not in ("q", "sdpa"):
        raise ValueError(scale)
    bias = swin_relative_position_bias(gb.seed, tag, (wh, ww), heads)
    if "bias_heads" in tw:
        bias = np.ascontiguousarray(np.resize(bias, (1, tw["bias_heads"], L, L)))
    if "bias_l" in tw:
        bias = np.ascontiguousarray(np.resize(bias, (1, heads, L, tw["bias_l"])))
    s = gb.simple("Add", [s, gb.init(tag + "_rpb", bias)])
    if tw.get("second_reader"):
        gb.simple("Relu", [s], out=tag + "_second_reader")
    if (shifted and not tw.get("roll_without_mask")) or tw.get("mask_without_roll"):
        mk = swin_shift_mask((H, W), (wh, ww), (sh, sw))
        if "mask_nw" in tw:
            mk = np.ascontiguousarray(np.resize(mk, (tw["mask_nw"], L, L)))
        if "mask_l" in tw:
            mk = np.ascontiguousarray(np.resize(mk, (nW, L, tw["mask_l"])))
        s = gb.simple("Reshape", [s, i64("mask5", [nb, nW, heads, L, L])])
        if mask == "init":
            mk5 = mk[None, :, None]
            if "mask_heads" in tw:
                mk5 = np.ascontiguousarray(np.repeat(mk5, tw["mask_heads"], axis=2))
            mname = gb.init(tag + "_mask", np.ascontiguousarray(mk5))
        elif mask == "unsqueeze":
            mname = gb.simple("Unsqueeze", [gb.init(tag + "_mask", mk), i64("mask_ax1", [1])])
            mname = gb.simple("Unsqueeze", [mname, i64("mask_ax0", [0])])
        else:
            raise ValueError(mask)
        s = gb.simple("Add", [s, mname])
        s = gb.simple("Reshape", [s, i64("mask4", [nbw, heads, L, L])])
    p = gb.simple("Softmax", [s], [pb.attr_int("axis", -1)])
    y = gb.transpose(gb.simple("MatMul", [p, v]), (0, 2, 1, 3))
    y = gb.simple("Reshape", [y, i64("shape3", [nbw, L, dim])])
    if linear:
        y = gb.linear(y, dim, dim, name=tag + "_proj")
    rwh, rww = tw.get("rev_window", (wh, ww))
    y = gb.simple("Reshape", [y, i64("rev6", [nb, H // rwh, W // rww, rwh, rww, dim])])
    y = gb.transpose(y, tw.get("rev_perm", (0, 1, 3, 2, 4, 5)))
    y = gb.simple("Reshape", [y, i64("rev4", [nb, H, W, dim])])
    if shifted and not tw.get("mask_without_roll"):
        y = roll(y, -1, "unroll", tw.get("back_shift", (sh, sw)), tw.get("back_axes", (1, 2)))
    if pad:
        y = gb.simple("Slice", [y, i64("crop_s", [0, 0]), i64("crop_e", [H, W]), i64("crop_a", [1, 2])])
    return y


def swin_patch_merge(gb: GraphBuilder, x: str, c: int, tag: str, reduce: bool = True) -> str:
    """torchvision's PatchMerging (V1) on a channels-last map [N, H, W, c]: x[..., a::2, b::2, :] for (a, b) = (0,0), (1,0), (0,1), (1,1), each two
    strided Slices -> Concat(axis -1) [N, H/2, W/2, 4c] -> LayerNorm -> Linear 4c -> 2c without a bias (reduce = False: the Concat alone)"""
    def i64(name: str, v: Sequence[int]) -> str:
        return gb.init(f"{tag}_{name}", np.array(list(v), np.int64))

    parts = []
    for k, (a, b) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
        y = gb.simple("Slice", [x, i64(f"h{k}_s", [a]), i64(f"h{k}_e", [INT64_MAX]), i64(f"h{k}_a", [1]), i64(f"h{k}_t", [2])])
        parts.append(gb.simple("Slice", [y, i64(f"w{k}_s", [b]), i64(f"w{k}_e", [INT64_MAX]), i64(f"w{k}_a", [2]), i64(f"w{k}_t", [2])]))
    y = gb.concat(parts, axis=-1)
    if not reduce:
        return y
    y = gb.layernorm(y, 4 * c, eps=1e-5, name=tag + "_ln")
    w = rng.gaussish(gb.seed, tag + "_red_w", 8 * c * c).reshape(4 * c, 2 * c) * np.float32(np.sqrt(1.0 / (4 * c)))
    return gb.simple("MatMul", [y, gb.init(tag + "_red_w", w.astype(np.float32))])


def swin(batch: int | str = 1, *, image: int = 224, patch: int = 4, dims: Sequence[int] = (96, 192, 384, 768), depths: Sequence[int] = (2, 2, 6, 2),
         heads: Sequence[int] = (3, 6, 12, 24), window: int = 7, classes: int = 1000, pad: bool = False, mask: str = "init", unbind: str = "gather",
         scale: str = "q", swap: bool = False, gelu: str = "erf", seed: int = 2103, in_name: str = "input", out_name: str = "logits",
         tweak: dict | None = None) -> bytes:
    """The Swin Transformer V1 (Liu et al. 2021) in the graph form torchvision's swin_transformer.py gives under the TorchScript exporter's known
    lowerings at opset 17 (written from the source: no real export was at hand): patch conv 4x4/s4 (bias) -> Transpose [0,2,3,1] -> LayerNorm; per
    block x += proj(window attention(LayerNorm(x))) (swin_window_attention; odd blocks of a stage shifted by window // 2, a dim's shift 0 where the
    window covers the map), x += Linear(GELU(Linear(LayerNorm(x)))) with mlp = 4 C; between the stages swin_patch_merge; LayerNorm ->
    Transpose [0,3,1,2] -> GlobalAveragePool -> Flatten -> Gemm."""
    gb = GraphBuilder("swin", seed)
    c = dims[0]
    hw = image // patch
    x = gb.layernorm(gb.transpose(gb.conv(in_name, 3, c, patch, stride=patch, bias=True, name="patch"), (0, 2, 3, 1)), c, eps=1e-5, name="patch_ln")
    for si, (depth, dim, nh) in enumerate(zip(depths, dims, heads)):
        if si > 0:
            x = swin_patch_merge(gb, x, c, f"merge{si}")
            c, hw = dim, hw // 2
        for bi in range(depth):
            tag = f"s{si}b{bi}"
            s = 0 if (bi % 2 == 0 or window >= hw) else window // 2
            y = swin_window_attention(gb, gb.layernorm(x, c, eps=1e-5, name=tag + "_ln1"), c, nh, (hw, hw), (window, window), (s, s), batch, tag + "_attn",
                                      pad=pad, mask=mask, unbind=unbind, scale=scale, swap=swap, tweak=tweak)
            x = gb.simple("Add", [x, y])
            y = gb.gelu(gb.linear(gb.layernorm(x, c, eps=1e-5, name=tag + "_ln2"), c, 4 * c, name=tag + "_fc1"), gelu)
            x = gb.simple("Add", [x, gb.linear(y, 4 * c, c, name=tag + "_fc2", w_scale=float(np.sqrt(2.0 / (4 * c))))])
    x = gb.transpose(gb.layernorm(x, c, eps=1e-5, name="head_ln"), (0, 3, 1, 2))
    x = gb.simple("Flatten", [gb.gap(x)], [pb.attr_int("axis", 1)])
    wfc = rng.gaussish(seed, "fc_w", classes * c).reshape(classes, c) * np.float32(np.sqrt(1.0 / c))
    bfc = (rng.uniform(seed, "fc_b", classes) - np.float32(0.5)) * np.float32(0.2)
    gb.simple("Gemm", [x, gb.init("fc_w", wfc.astype(np.float32)), gb.init("fc_b", bfc.astype(np.float32))], [pb.attr_int("transB", 1)], out=out_name)
    return gb.finish([(in_name, [batch, 3, image, image])], [(out_name, [batch, classes])], opset=20 if gelu.startswith("op") else 17)


def swin_t(batch: int | str = 1, **kw) -> bytes:
    return swin(batch, image=224, dims=(96, 192, 384, 768), depths=(2, 2, 6, 2), heads=(3, 6, 12, 24), window=7, **kw)


def vae_resnet_block(gb: GraphBuilder, x: str, cin: int, cout: int, hw: Sequence[int], tag: str, gn) -> str:
    """diffusers' ResnetBlock2D without a time embedding: norm1 -> SiLU -> conv1 3x3 -> norm2 -> SiLU -> conv2 3x3, the shortcut a 1x1 conv where the
    channel count changes, out = shortcut + h"""
    h = gb.conv(gb.silu(gn(x, cin, hw, tag + "_norm1")), cin, cout, 3, pad=1, bias=True, name=tag + "_conv1")
    h = gb.conv(gb.silu(gn(h, cout, hw, tag + "_norm2")), cout, cout, 3, pad=1, bias=True, name=tag + "_conv2", w_scale=float(0.5 * np.sqrt(2.0 / (9 * cout))))
    sc = x if cin == cout else gb.conv(x, cin, cout, 1, bias=True, name=tag + "_conv_shortcut")
    return gb.simple("Add", [sc, h])


def vae_attention(gb: GraphBuilder, x: str, c: int, hw: Sequence[int], tag: str, gn) -> str:
    """diffusers' Attention with AttnProcessor2_0 on a map x [N, c, h, w], one head of c channels: view [N, c, h w] -> transpose(1, 2) ->
    group_norm(. transpose(1, 2)).transpose(1, 2) (two Transposes back to back, as torch writes them) -> to_q / to_k / to_v -> view [N, L, 1, c] ->
    transpose(1, 2) -> scaled_dot_product_attention in the exporter's lowering (q and k^T each times sqrt(c^-0.5)) -> transpose(1, 2) -> reshape
    [N, L, c] -> to_out -> transpose(-1, -2) -> reshape [N, c, h, w] -> + residual"""
    t = vit_tokens(gb, x, c)
    g = gb.transpose(gn(gb.transpose(t, (0, 2, 1)), c, hw, tag + "_group_norm", rank3=True), (0, 2, 1))
    shp = gb.init(tag + "_shape4", np.array([0, -1, 1, c], np.int64))
    q, k, v = (gb.transpose(gb.simple("Reshape", [gb.linear(g, c, c, name=f"{tag}_to_{n}"), shp]), (0, 2, 1, 3)) for n in ("q", "k", "v"))
    rs = gb.init(tag + "_sqrt_scale", np.array(np.sqrt(float(c) ** -0.5), np.float32))
    s = gb.simple("MatMul", [gb.simple("Mul", [q, rs]), gb.simple("Mul", [gb.transpose(k, (0, 1, 3, 2)), rs])])
    p = gb.simple("Softmax", [s], [pb.attr_int("axis", -1)])
    y = gb.transpose(gb.simple("MatMul", [p, v]), (0, 2, 1, 3))
    y = gb.simple("Reshape", [y, gb.init(tag + "_shape3", np.array([0, -1, c], np.int64))])
    y = gb.linear(y, c, c, name=tag + "_to_out")
    y = gb.simple("Reshape", [gb.transpose(y, (0, 2, 1)), gb.init(tag + "_shape_back", np.array([0, c, hw[0], hw[1]], np.int64))])
    return gb.simple("Add", [y, x])


def vae_decoder(batch: int | str = 1, *, latent: int = 32, base: int = 128, mults: Sequence[int] = (1, 2, 4, 4), layers: int = 2, groups: int = 32,
                latent_ch: int = 4, gn_form: str = "instancenorm", seed: int = 860, in_name: str = "latent_sample", out_name: str = "sample") -> bytes:
    """The decoder of diffusers' AutoencoderKL as Stable Diffusion 1.x configures it: latents [N, latent_ch, latent, latent] -> sample
    [N, 3, 8 latent, 8 latent] (with four mults).  Written from diffusers' vae.py (Decoder, UNetMidBlock2D, UpDecoderBlock2D), resnet.py
    (ResnetBlock2D, Upsample2D), attention_processor.py (Attention, AttnProcessor2_0) and the exporter's known lowerings at opset 17; no file of
    that project is executed.

    post_quant_conv 1x1 -> conv_in 3x3 -> mid block (ResnetBlock, single-head self-attention, ResnetBlock) on base * mults[-1] channels -> one up
    block per entry of reversed(mults), each layers + 1 ResnetBlocks (a 1x1 conv shortcut where the channel count changes) and, but for the last,
    a nearest x2 Resize + 3x3 conv -> conv_norm_out -> SiLU -> conv_out 3x3.  Every norm is GroupNorm(groups, eps 1e-6) in the spelling gn_form:
    "instancenorm" (opset 17, the back-Reshape from Shape(x)), "op18" or "op21" (GroupNormalization, the model's opset 18 / 21).  SiLU is
    Mul(x, Sigmoid(x)).  The divisions by output_scale_factor = 1 and rescale_output_factor = 1 that the modules write are left out."""
    opset = {"instancenorm": 17, "op18": 18, "op21": 21}[gn_form]
    gb = GraphBuilder("vae_decoder", seed)

    def gn(x: str, c: int, hw: Sequence[int], name: str, rank3: bool = False) -> str:
        return gb.group_norm(x, c, groups, eps=1e-6, form=gn_form, back="shape", rank3=rank3, hw=hw, name=name)

    hw = (latent, latent)
    c = base * mults[-1]
    x = gb.conv(in_name, latent_ch, latent_ch, 1, bias=True, name="post_quant_conv", w_scale=float(np.sqrt(1.0 / latent_ch)))
    x = gb.conv(x, latent_ch, c, 3, pad=1, bias=True, name="conv_in", w_scale=float(np.sqrt(1.0 / (9 * latent_ch))))
    x = vae_resnet_block(gb, x, c, c, hw, "mid_res1", gn)
    x = vae_attention(gb, x, c, hw, "mid_attn", gn)
    x = vae_resnet_block(gb, x, c, c, hw, "mid_res2", gn)
    for bi, mult in enumerate(reversed(list(mults))):
        cout = base * mult
        for li in range(layers + 1):
            x = vae_resnet_block(gb, x, c, cout, hw, f"up{bi}_res{li}", gn)
            c = cout
        if bi + 1 < len(mults):
            x = gb.resize(x, [batch, c, hw[0], hw[1]], scales=[2.0, 2.0], mode="nearest", coord="asymmetric", nearest="floor", form="scales", name=f"up{bi}_upsample")
            hw = (2 * hw[0], 2 * hw[1])
            x = gb.conv(x, c, c, 3, pad=1, bias=True, name=f"up{bi}_upsample_conv")
    x = gb.silu(gn(x, c, hw, "conv_norm_out"))
    gb.conv(x, c, 3, 3, pad=1, bias=True, name="conv_out", out=out_name)
    return gb.finish([(in_name, [batch, latent_ch, latent, latent])], [(out_name, [batch, 3, hw[0], hw[1]])], opset=opset)


def write_repo(root: str, name: str, model_bytes: bytes, version: str = "1", config_json: str | None = None) -> str:
    d = os.path.join(root, name, version)
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, "model.onnx")
    tmp = path + f".tmp{os.getpid()}"
    with open(tmp, "wb") as f:
        f.write(model_bytes)
    os.replace(tmp, path)
    if config_json is not None:
        with open(os.path.join(d, "config.json"), "w") as f:
            f.write(config_json)
    return d


def synthetic_input(shape: Sequence[int], seed: int = 20250704, stream: str = "input") -> np.ndarray:
    """Synthetic images in [0,1) (the client's /255 convention: client/test_client.py:189).

    0.6 * (per-image, per-channel coarse grid of random levels, nearest-upsampled by `cell`) + 0.4 * U[0,1)
    fine noise, so different images give visibly different logits (pure white noise averages out through
    the pooling stages).  Only RNG draws, multiplies and adds: no libm dependence.
    """
    shape = tuple(int(d) for d in shape)
    n = int(np.prod(shape))
    fine = rng.uniform(seed, stream, n).reshape(shape)
    if len(shape) != 4 or shape[2] < 8 or shape[3] < 8:
        return fine
    b, c, h, w = shape
    cell = max(h // 7, 1)
    gh, gw = -(-h // cell), -(-w // cell)
    coarse = rng.uniform(seed, stream + "/coarse", b * c * gh * gw).reshape(b, c, gh, gw)
    up = np.repeat(np.repeat(coarse, cell, axis=2), cell, axis=3)[:, :, :h, :w]
    return (np.float32(0.6) * up + np.float32(0.4) * fine).astype(np.float32)
