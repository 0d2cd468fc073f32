"""Single-step ONNX graphs around ONE depthwise or grouped convolution whose operands the reference knows exactly (test infrastructure; used
by tests/test_kernel_ref.py, tests/test_channel_maps_plan.py and tests/test_channel_maps_gpu.py).  The style and the exact-input trick are
tests/kernel_graphs.py's (grid_input, lift_weights, lifted, _bn are reused):

    x (k/32 grid) -> lifting 1x1 conv 3 -> C -> [prologue] -> Conv(group) [+ bias] -> [BN] -> [+ lifted] -> [ReLU | Clip | activation] -> output form

What the planner makes of the pieces (checked with DescribeModel; tests/test_channel_maps_plan.py asserts it for every table entry):

  pre "bn"      BN -> ReLU in front of the conv.  With the lifted tensor as its only input it would fuse into the LIFTING conv's epilogue and
                never reach the kernel under test, so these cases always add the lifted tensor as the residual: a second consumer keeps the
                lift linear and the step plans as prebn+prerelu+conv+...+add with a prologue (pre, pre_relu) and in2 = the lift.
  pre "hswish" / "sigmoid"   lift -> activation -> depthwise, single consumers: an identity-scale prologue with pre_act on the depthwise step
                (Planner::FuseActivationPrologues; depthwise only).  The lift stays linear.
  pre "clip"    lift -> Clip(0, hi) -> depthwise, single consumers: Planner::FuseRelu6IntoDepthwise gives the lift the ReLU and the depthwise
                step pre_relu and pre_clip = hi (the spelling that sets pre_hi; depthwise only).  hi = 1.5 so that the bound bites on lifted
                values.  A BN -> Clip(0, 6) in front of a depthwise conv with a shared input is NOT this pattern (the clip stays an eltwise step).
  post          Conv -> [BN] -> [Add] -> HardSwish | HardSigmoid | Sigmoid fuses as act; Conv -> Clip(lo | None, hi | None) fuses as clip.
                ReLU followed by Clip does not fuse (the clip becomes an eltwise step), so no case builds it.
  out "cat2"    Concat(y, y): the step stores at pitch 2 C (the second copy is made by a copy step)
      "single"  y alone
      "offset"  Concat(8 lifted channels, y): the step stores at channel offset 8, pitch C + 8
  slice_in      the lifted tensor is the tail of Concat(8 lifted channels, lifted) which a side 1x1 conv also reads: the step READS at channel
                offset 8, pitch C + 8 (Slice is not a supported operator; this is test_depthwise_gpu._random_graph's way), and the side conv's 8
                channels follow y in the output.
  direct        the conv reads the NCHW graph input itself (C = 3; fp32 even in an fp16 plan: mixed element types, the generic kernel).
"""
import numpy as np

import kernel_graphs as G
import kernel_ref as R
from gpu_ai_inference_server_amd.modelgen import onnx_pb as pb

f32, f64 = np.float32, np.float64

PRE_CLIP_HI = 1.5
HSWISH_A, HSWISH_B = float(f32(1.0 / 6.0)), 0.5
HSIG_A, HSIG_B = float(f32(0.2)), 0.5
ACTS = {"sigmoid": (R.ACT_SIGMOID, 0.0, 0.0), "hardsigmoid": (R.ACT_HARDSIGMOID, HSIG_A, HSIG_B), "hswish": (R.ACT_HARDSWISH, HSWISH_A, HSWISH_B)}


def _act_node(kind, src, dst, name):
    if kind == "sigmoid":
        return pb.node("Sigmoid", [src], [dst], name)
    if kind == "hardsigmoid":
        return pb.node("HardSigmoid", [src], [dst], name, [pb.attr_float("alpha", 0.2), pb.attr_float("beta", 0.5)])
    assert kind == "hswish"
    return pb.node("HardSwish", [src], [dst], name)


def channel_case(seed, n, h, w, c, groups, cout, k=3, stride=1, pads=None, pre="", bias=False, post_bn=False, res=False, relu=False, clip=None,
                 act="", out="cat2", slice_in=False, half_w=False, direct=False):
    """k: int or (kh, kw); pads: (top, left, bottom, right), None = k // 2 all round.  Returns a dict: model bytes, first input, shapes, every
    parameter array."""
    kh, kw = (k, k) if isinstance(k, int) else k
    pads = (kh // 2, kw // 2, kh // 2, kw // 2) if pads is None else tuple(pads)
    assert c % groups == 0 and cout % groups == 0 and not (relu and clip) and not ((relu or clip) and act)
    assert pre != "bn" or res, "a BN + ReLU prologue needs the lifted tensor's second consumer (module docstring)"
    assert not (pre in ("hswish", "sigmoid", "clip") and (res or slice_in)), "the prologue activation / bound needs single consumers"
    rs = np.random.RandomState(seed)
    oh, ow = R.channel_out_hw(h, w, kh, kw, stride, pads)
    d = dict(seed=seed, n=n, h=h, w=w, c=c, groups=groups, cout=cout, kh=kh, kw=kw, stride=stride, pads=pads, pre=pre, bias=bias, post_bn=post_bn,
             res=res, relu=relu, clip=clip, act=act, out=out, slice_in=slice_in, half_w=half_w, direct=direct, oh=oh, ow=ow)
    d["x"] = G.grid_input(rs, n, h, w)
    nodes, inits = [], []
    if direct:
        assert c == 3 and not (pre or res or slice_in) and out != "offset"
        t = lift = "x"
    else:
        d["w0"] = G.lift_weights(rs, c)
        inits.append(pb.tensor("w0", d["w0"]))
        nodes.append(pb.node("Conv", ["x", "w0"], ["h0"], "lift", [pb.attr_ints("kernel_shape", [1, 1])]))
        t = lift = "h0"
    if slice_in or out == "offset":
        d["w8"] = G.lift_weights(rs, 8)
        inits.append(pb.tensor("w8", d["w8"]))
    if slice_in:
        assert (oh, ow) == ((h - 1) // stride + 1, (w - 1) // stride + 1) and out == "single"
        nodes.append(pb.node("Conv", ["x", "w8"], ["h8"], "lift8", [pb.attr_ints("kernel_shape", [1, 1])]))
        nodes.append(pb.node("Concat", ["h8", "h0"], ["cat0"], "cat_in", [pb.attr_int("axis", 1)]))
        d["ws"] = (rs.randn(8, c + 8, 1, 1) * np.sqrt(2.0 / (c + 8))).astype(f32)
        inits.append(pb.tensor("ws", d["ws"]))
        nodes.append(pb.node("Conv", ["cat0", "ws"], ["side"], "side", [pb.attr_ints("kernel_shape", [1, 1]), pb.attr_ints("strides", [stride, stride])]))
    if pre == "bn":
        d["pre_bn"] = G._bn(rs, c, "pre_", inits)
        nodes.append(pb.node("BatchNormalization", [t, "pre_g", "pre_b", "pre_m", "pre_v"], ["p0"], "prebn", [pb.attr_float("epsilon", 1e-5)]))
        nodes.append(pb.node("Relu", ["p0"], ["p1"], "prerelu"))
        t = "p1"
    elif pre == "clip":
        inits += [pb.tensor("pre_lo", np.array(0.0, f32)), pb.tensor("pre_hi", np.array(PRE_CLIP_HI, f32))]
        nodes.append(pb.node("Clip", [t, "pre_lo", "pre_hi"], ["p1"], "preclip"))
        t = "p1"
    elif pre:
        nodes.append(_act_node(pre, t, "p1", "preact"))
        t = "p1"
    cpg = c // groups
    wt = (rs.randn(cout, cpg, kh, kw) * np.sqrt(2.0 / (cpg * kh * kw))).astype(f32)
    d["wt"] = R.half_exact(wt) if half_w else wt
    inits.append(pb.tensor("w", d["wt"]))
    ins = [t, "w"]
    if bias:
        d["bvec"] = (0.2 * rs.randn(cout)).astype(f32)
        inits.append(pb.tensor("bvec", d["bvec"]))
        ins.append("bvec")
    nodes.append(pb.node("Conv", ins, ["y0"], "conv", [pb.attr_ints("kernel_shape", [kh, kw]), pb.attr_ints("pads", list(pads)),
                                                       pb.attr_ints("strides", [stride, stride]), pb.attr_int("group", groups)]))
    y = "y0"
    if post_bn:
        d["post_bn"] = G._bn(rs, cout, "post_", inits)
        nodes.append(pb.node("BatchNormalization", [y, "post_g", "post_b", "post_m", "post_v"], ["y1"], "postbn", [pb.attr_float("epsilon", 1e-5)]))
        y = "y1"
    if res:
        assert (cout, oh, ow) == (c, h, w)
        nodes.append(pb.node("Add", [y, lift], ["y2"], "add"))
        y = "y2"
    if relu:
        nodes.append(pb.node("Relu", [y], ["y3"], "postrelu"))
        y = "y3"
    if clip:
        lo, hi = clip
        cin_ = [y]
        for tag, v in (("post_lo", lo), ("post_hi", hi)):
            if v is None:
                cin_.append("")
            else:
                inits.append(pb.tensor(tag, np.array(v, f32)))
                cin_.append(tag)
        while cin_[-1] == "":
            cin_.pop()
        nodes.append(pb.node("Clip", cin_, ["y3"], "postclip"))
        y = "y3"
    if act:
        nodes.append(_act_node(act, y, "y3", "postact"))
        y = "y3"
    if slice_in:
        nodes.append(pb.node("Concat", [y, "side"], ["out"], "cat", [pb.attr_int("axis", 1)]))
        ctot, d["copies"] = cout + 8, [0]
    elif out == "cat2":
        nodes.append(pb.node("Concat", [y, y], ["out"], "cat", [pb.attr_int("axis", 1)]))
        ctot, d["copies"] = 2 * cout, [0, cout]
    elif out == "offset":
        assert (oh, ow) == (h, w)
        nodes.append(pb.node("Conv", ["x", "w8"], ["h8"], "lift8", [pb.attr_ints("kernel_shape", [1, 1])]))
        nodes.append(pb.node("Concat", ["h8", y], ["out"], "cat", [pb.attr_int("axis", 1)]))
        ctot, d["copies"] = cout + 8, [8]
    else:
        assert out == "single"
        nodes.append(pb.node("Identity", [y], ["out"], "ident"))
        ctot, d["copies"] = cout, [0]
    g = pb.graph(f"chcase{seed}", nodes, inits, [pb.value_info("x", [n, 3, h, w])], [pb.value_info("out", [n, ctot, oh, ow])])
    d.update(model=pb.model(g, opset=14), ishape=(n, 3, h, w), oshape=(n, ctot, oh, ow))
    return d


def channel_operands(d, x, f16=False, dot=False):
    """What the kernel of case `d` is given for the input x, as a dict:
      xh      the conv input after the prologue, NCHW: float32 (float64 where a prologue activation makes the reference's x_hat a real number)
      xh2     the two-rounding form of an affine prologue (as legal as the FMA), or None
      w, bias the folded weights [Cout, Cin / groups, kh, kw] and bias (None: none);  res: the residual (the lifted tensor) or None
      relu, lo, hi, act = (code, a, b)       the epilogue
      pre_act                                a prologue activation: every x_hat carries the activation's own relative error
      rounded                                fp16 mode: operands the step rounds to half itself (kernel_ref.half_terms).  As read from the kernels:
                                             conv_dw_kernel and both generic kernels read fp32 weights, bias and prologue constants and never round
                                             x_hat: 0.  conv_grouped_kernel on its v_dot2 path (`dot`: halfs, even channels per group) reads the half
                                             mirror of the weights (1 unless they are half-exact) and rounds x_hat to half (1 where a prologue made it
                                             inexact); with one channel per group it takes the fp32 path in fp16 mode too: 0."""
    src = np.asarray(x, f32) if d["direct"] else G.lifted(x, d["w0"])
    xh, xh2, pre_act = src, None, False
    if d["pre"] == "bn":
        p = d["pre_bn"]
        s, t = R.bn_affine(p["g"], p["b"], p["m"], p["v"])
        xh, xh2 = R.prologue32(src, s, t), R.prologue32(src, s, t, fused=False)
    elif d["pre"] == "clip":
        xh = np.minimum(np.maximum(src, f32(0)), f32(PRE_CLIP_HI))
    elif d["pre"]:
        xh, pre_act = R.act64(*((ACTS[d["pre"]][0], src) + ACTS[d["pre"]][1:])), True
    wt, b = d["wt"], d.get("bvec")
    if d["post_bn"]:
        p = d["post_bn"]
        wt, b = R.fold32(wt, b, *R.bn_affine(p["g"], p["b"], p["m"], p["v"]))
    rounded = 0
    if f16 and dot:
        rounded = int(not np.array_equal(R.half_exact(wt), wt)) + int(d["pre"] == "bn")
    lo, hi = d["clip"] if d["clip"] else (None, None)
    return dict(xh=xh, xh2=xh2, w=wt, bias=b, res=src if d["res"] else None, relu=d["relu"], lo=lo, hi=hi, act=ACTS[d["act"]] if d["act"] else (0, 0.0, 0.0),
                pre_act=pre_act, rounded=rounded)


def copies(d, y):
    """The graph output -> the conv's result, once per copy the graph stores, stacked along the channel axis"""
    return np.concatenate([y[:, o:o + d["cout"]] for o in d["copies"]], axis=1)


def tile_copies(d, a):
    return np.concatenate([a] * len(d["copies"]), axis=1)
