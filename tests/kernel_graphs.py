"""Single-step ONNX graphs whose operands the reference knows exactly (test infrastructure; used by tests/test_kernel_ref.py and
tests/test_kernel_maps_gpu.py).

    x (k/32 grid) -> lifting 1x1 conv 3 -> Cin (weights multiples of 1/4) -> [BN + ReLU] -> Conv [+ bias] -> [BN] -> [ReLU] -> Concat(y, y)

Every partial sum of the lifting conv is a multiple of 2^-7 (2^-8 beyond 728 channels) below 4: exact in fp32 and in half in any summation order, so the conv
under test reads a tensor that numpy reproduces bit for bit, and nothing upstream of it rounds.  The Concat stores the second copy of the
result at a channel offset into a wider buffer.  Pools read the lifted tensor directly.
"""
import numpy as np

import kernel_ref as R
from gpu_ai_inference_server_amd.modelgen import onnx_pb as pb

f32, f64 = np.float32, np.float64


def grid_input(rs, n, h, w):
    return (rs.randint(0, 32, size=(n, 3, h, w)) / 32.0).astype(f32)


def lift_weights(rs, cin):
    """[cin, 3, 1, 1], entries multiples of 1/4 in [-1, 1], a different non-zero triple per channel.  Beyond the 728 such triples (the
    K = 1008 / 1024 cases) multiples of 1/8: partial sums are then multiples of 2^-8 below 4, ten bits, still exact in half."""
    q = 4 if cin <= 9 ** 3 - 1 else 8
    m = 2 * q + 1
    assert cin <= m ** 3 - 1
    codes = rs.permutation(m ** 3)
    codes = codes[codes != (m ** 3) // 2][:cin]          # (the middle code is the all-zero triple)
    t = np.stack([codes // (m * m), codes // m % m, codes % m], axis=1)
    return ((t - q) / float(q)).astype(f32).reshape(cin, 3, 1, 1)


def lifted(x, w0):
    """The lifting conv in float64; the result is exactly representable in half."""
    y = np.einsum("nchw,oc->nohw", x.astype(f64), w0.reshape(w0.shape[0], 3).astype(f64))
    assert np.array_equal(y.astype(np.float16).astype(f64), y)
    return y.astype(f32)


def _bn(rs, c, prefix, inits):
    p = {}
    for nm, v in (("g", 1 + 0.1 * rs.randn(c)), ("b", 0.1 * rs.randn(c)), ("m", 0.1 * rs.randn(c)), ("v", 0.5 + rs.rand(c))):
        p[nm] = v.astype(f32)
        inits.append(pb.tensor(prefix + nm, p[nm]))
    return p


def conv_case(seed, n, h, w, cin, cout, k=1, stride=1, pad=0, pre=False, bias=False, post=0, half_w=False, dil=1):
    """post: 0 none, 1 ReLU, 2 BN + ReLU, 3 BN.  half_w: conv weights pre-rounded to half-representable values (the tight fp16 cases).
    Returns a dict: model bytes, input, shapes and every parameter array."""
    rs = np.random.RandomState(seed)
    x = grid_input(rs, n, h, w)
    w0 = lift_weights(rs, cin)
    nodes, inits = [], []
    inits.append(pb.tensor("w0", w0))
    nodes.append(pb.node("Conv", ["x", "w0"], ["h0"], "lift", [pb.attr_ints("kernel_shape", [1, 1])]))
    t = "h0"
    d = dict(seed=seed, n=n, h=h, w=w, cin=cin, cout=cout, k=k, stride=stride, pad=pad, pre=pre, bias=bias, post=post, half_w=half_w, dil=dil,
             x=x, w0=w0)
    if pre:
        d["pre_bn"] = _bn(rs, cin, "pre_", inits)
        nodes.append(pb.node("BatchNormalization", [t, "pre_g", "pre_b", "pre_m", "pre_v"], ["p0"], "prebn", [pb.attr_float("epsilon", 1e-5)]))
        nodes.append(pb.node("Relu", ["p0"], ["p1"], "prerelu"))
        t = "p1"
    wt = (rs.randn(cout, cin, k, k) * np.sqrt(2.0 / (cin * k * k))).astype(f32)
    if half_w:
        wt = R.half_exact(wt)
    d["wt"] = wt
    inits.append(pb.tensor("w", wt))
    ins = [t, "w"]
    if bias:
        d["bvec"] = (0.2 * rs.randn(cout)).astype(f32)
        inits.append(pb.tensor("bvec", d["bvec"]))
        ins.append("bvec")
    attrs = [pb.attr_ints("kernel_shape", [k, k]), pb.attr_ints("pads", [pad] * 4), pb.attr_ints("strides", [stride, stride])]
    if dil != 1:
        attrs.append(pb.attr_ints("dilations", [dil, dil]))
    nodes.append(pb.node("Conv", ins, ["y0"], "conv", attrs))
    y = "y0"
    if post >= 2:
        d["post_bn"] = _bn(rs, cout, "post_", inits)
        nodes.append(pb.node("BatchNormalization", [y, "post_g", "post_b", "post_m", "post_v"], ["y1"], "postbn", [pb.attr_float("epsilon", 1e-5)]))
        y = "y1"
    if post in (1, 2):
        nodes.append(pb.node("Relu", [y], ["y2"], "postrelu"))
        y = "y2"
    oh = (h + 2 * pad - dil * (k - 1) - 1) // stride + 1
    ow = (w + 2 * pad - dil * (k - 1) - 1) // stride + 1
    nodes.append(pb.node("Concat", [y, y], ["out"], "cat", [pb.attr_int("axis", 1)]))
    g = pb.graph(f"kcase{seed}", nodes, inits, [pb.value_info("x", [n, 3, h, w])], [pb.value_info("out", [n, 2 * cout, oh, ow])])
    d.update(model=pb.model(g), ishape=(n, 3, h, w), oshape=(n, 2 * cout, oh, ow), oh=oh, ow=ow)
    return d


def conv_operands(d, f16=False):
    """(cols [M, K], wm [Cout, K], bias or None, relu, rounded_operands) as the conv kernel of case `d` is given them.  fp16 mode: the
    prologue's scale / shift are the half mirror's values and the step rounds x_hat (with a prologue) and w' (unless it is
    half-representable already) to half itself: `rounded_operands` counts those for kernel_ref.half_terms."""
    xh = lifted(d["x"], d["w0"])
    rounded = 0
    if d["pre"]:
        p = d["pre_bn"]
        s, t = R.bn_affine(p["g"], p["b"], p["m"], p["v"])
        if f16:
            s, t = R.half_exact(s), R.half_exact(t)
            rounded += 1
        xh = R.prologue32(xh, s, t)
    wt, b = d["wt"], d.get("bvec")
    if d["post"] >= 2:
        p = d["post_bn"]
        wt, b = R.fold32(wt, b, *R.bn_affine(p["g"], p["b"], p["m"], p["v"]))
    if f16 and not np.array_equal(R.half_exact(wt), wt):
        rounded += 1
    cols = R.im2col(xh, d["k"], d["k"], d["stride"], (d["pad"],) * 4, d["dil"])
    return cols.reshape(-1, d["k"] * d["k"] * d["cin"]), R.wmat(wt), b, d["post"] in (1, 2), rounded


def conv_xhat(d):
    """The fp32 conv input after the prologue, NCHW (what wino32 takes)."""
    xh = lifted(d["x"], d["w0"])
    if d["pre"]:
        p = d["pre_bn"]
        xh = R.prologue32(xh, *R.bn_affine(p["g"], p["b"], p["m"], p["v"]))
    return xh


def two_copies(ym, d):
    """[M, Cout] -> the graph's output [N, 2 Cout, OH, OW]."""
    y = R.to_nchw(ym, (d["n"], d["oh"], d["ow"]))
    return np.concatenate([y, y], axis=1)


def lift_case(seed, n, h, w, cin):
    """The lifting conv alone, as graph output."""
    rs = np.random.RandomState(seed)
    x = grid_input(rs, n, h, w)
    w0 = lift_weights(rs, cin)
    nodes = [pb.node("Conv", ["x", "w0"], ["out"], "lift", [pb.attr_ints("kernel_shape", [1, 1])])]
    g = pb.graph(f"lift{seed}", nodes, [pb.tensor("w0", w0)], [pb.value_info("x", [n, 3, h, w])], [pb.value_info("out", [n, cin, h, w])])
    return dict(model=pb.model(g), x=x, w0=w0, ishape=(n, 3, h, w), oshape=(n, cin, h, w))


def pool_case(seed, n, h, w, c, k, stride, pads, is_max, count_include_pad=0):
    """Lifted tensor -> MaxPool / AveragePool as graph output; pads = (top, left, bottom, right)."""
    rs = np.random.RandomState(seed)
    x = grid_input(rs, n, h, w)
    w0 = lift_weights(rs, c)
    pt, pl, pb_, pr = pads
    attrs = [pb.attr_ints("kernel_shape", [k, k]), pb.attr_ints("pads", [pt, pl, pb_, pr]), pb.attr_ints("strides", [stride, stride])]
    if not is_max:
        attrs.append(pb.attr_int("count_include_pad", count_include_pad))
    nodes = [pb.node("Conv", ["x", "w0"], ["h0"], "lift", [pb.attr_ints("kernel_shape", [1, 1])]),
             pb.node("MaxPool" if is_max else "AveragePool", ["h0"], ["out"], "pool", attrs)]
    oh = (h + pt + pb_ - k) // stride + 1
    ow = (w + pl + pr - k) // stride + 1
    g = pb.graph(f"pool{seed}", nodes, [pb.tensor("w0", w0)], [pb.value_info("x", [n, 3, h, w])], [pb.value_info("out", [n, c, oh, ow])])
    return dict(model=pb.model(g), x=x, w0=w0, ishape=(n, 3, h, w), oshape=(n, c, oh, ow), k=k, stride=stride, pads=pads, is_max=is_max,
                count_include_pad=count_include_pad)


def dense_case(seed, n, h, w, c0, layers, tail, expose):
    """Lifted block input X0 (c0 channels) -> `layers` dense layers (BN-ReLU-1x1 to 128, BN-ReLU-3x3 to 32, Concat with the layer's input)
    [-> tail: the next layer's BN-ReLU-1x1-BN-ReLU] -- the smallest graph the dense-fusion (fp32) and dense-block (fp16) patterns of the
    planner accept.  Outputs: "cat" (the concat buffer), "bott" (the tail's bottleneck), and with `expose` every layer's bottleneck "b<l>"."""
    rs = np.random.RandomState(seed)
    x = grid_input(rs, n, h, w)
    w0 = lift_weights(rs, c0)
    nodes, inits, outs, L = [], [pb.tensor("w0", w0)], [], []
    nodes.append(pb.node("Conv", ["x", "w0"], ["x0"], "lift", [pb.attr_ints("kernel_shape", [1, 1])]))
    t, c = "x0", c0
    for l in range(1, layers + 1 + bool(tail)):
        P = dict(bn1=_bn(rs, c, f"l{l}a_", inits), w1=(rs.randn(128, c, 1, 1) * np.sqrt(2.0 / c)).astype(f32), cin=c)
        inits.append(pb.tensor(f"l{l}_w1", P["w1"]))
        nodes.append(pb.node("BatchNormalization", [t] + [f"l{l}a_{k}" for k in "gbmv"], [f"l{l}_n1"], f"l{l}_bn1", [pb.attr_float("epsilon", 1e-5)]))
        nodes.append(pb.node("Relu", [f"l{l}_n1"], [f"l{l}_r1"], f"l{l}_relu1"))
        nodes.append(pb.node("Conv", [f"l{l}_r1", f"l{l}_w1"], [f"l{l}_c1"], f"l{l}_conv1", [pb.attr_ints("kernel_shape", [1, 1])]))
        P["bn2"] = _bn(rs, 128, f"l{l}b_", inits)
        nodes.append(pb.node("BatchNormalization", [f"l{l}_c1"] + [f"l{l}b_{k}" for k in "gbmv"], [f"l{l}_n2"], f"l{l}_bn2", [pb.attr_float("epsilon", 1e-5)]))
        last = l == layers + 1
        bname = "bott" if last else f"b{l}"
        nodes.append(pb.node("Relu", [f"l{l}_n2"], [bname], f"l{l}_relu2"))
        if last or expose:
            outs.append(pb.value_info(bname, [n, 128, h, w]))
        if not last:
            P["w3"] = (rs.randn(32, 128, 3, 3) * np.sqrt(2.0 / (128 * 9))).astype(f32)
            inits.append(pb.tensor(f"l{l}_w3", P["w3"]))
            nodes.append(pb.node("Conv", [bname, f"l{l}_w3"], [f"l{l}_g"], f"l{l}_conv3", [pb.attr_ints("kernel_shape", [3, 3]), pb.attr_ints("pads", [1] * 4)]))
            cat = "cat" if l == layers else f"x{l}"
            nodes.append(pb.node("Concat", [t, f"l{l}_g"], [cat], f"l{l}_cat", [pb.attr_int("axis", 1)]))
            t, c = cat, c + 32
        L.append(P)
    outs.insert(0, pb.value_info("cat", [n, c, h, w]))
    g = pb.graph(f"dense{seed}", nodes, inits, [pb.value_info("x", [n, 3, h, w])], outs)
    names = ["cat"] + (["b%d" % l for l in range(1, layers + 1)] if expose else []) + (["bott"] if tail else [])
    return dict(model=pb.model(g), x=x, w0=w0, ishape=(n, 3, h, w), n=n, h=h, w=w, c0=c0, layers=L, nlayers=layers, ctot=c, seed=seed,
                outputs=[(nm, (n, c if nm == "cat" else 128, h, w)) for nm in names])
