"""Test graphs around one ConvTranspose (test infrastructure; used by tests/test_convt_plan.py, tests/test_convt_gpu.py and
tests/test_convt_maps_gpu.py).

random_case / random_graph: seeded random single ops inside a small graph.  Three seeds in five draw the non-overlapping geometry the MFMA
kernel takes (k == stride, no pads, no output_padding, Cin a multiple of 8); the others draw every attribute freely.
map_case: a single-step graph with exact operands, the ConvTranspose twin of kernel_graphs.conv_case.
"""
import numpy as np

import kernel_graphs as G
import kernel_ref as R
import ref64
from gpu_ai_inference_server_amd.modelgen import models
from gpu_ai_inference_server_amd.modelgen import onnx_pb as pb

f32 = np.float32
NUM_SEEDS = 30
CINS = [3, 6, 8, 16, 24, 64]
COUTS = [5, 16, 32, 40]


def random_case(seed):
    """Valid by construction: pads < k and H, W >= 5 keep every output extent (H - 1) * s + k - p0 - p1 + output_padding >= 1."""
    r = np.random.RandomState(4000 + seed)
    h, w = int(r.choice([5, 7, 9])), int(r.choice([5, 6, 11]))
    if seed % 5 < 3:
        s = [int(r.randint(1, 5)), int(r.randint(1, 5))]
        k, pads, op = list(s), [0, 0, 0, 0], [0, 0]
        cin = int(r.choice([16, 64, 16, 64, 8, 24]))
    else:
        k = [int(r.randint(1, 6)), int(r.randint(1, 6))]
        s = [int(r.randint(1, 5)), int(r.randint(1, 5))]
        pads = [int(r.randint(0, k[0])), int(r.randint(0, k[1])), int(r.randint(0, k[0])), int(r.randint(0, k[1]))]
        op = [int(r.randint(0, s[0])), int(r.randint(0, s[1]))]
        cin = int(r.choice(CINS))
    pre1x1 = bool(r.randint(2))
    return dict(seed=seed, h=h, w=w, k=k, s=s, pads=pads, op=op, cin=cin, cout=int(r.choice(COUTS)), pre1x1=pre1x1, cat_in=pre1x1 and bool(r.randint(2)),
                bias=bool(r.randint(2)), bn_relu=bool(r.randint(2)), cat_out=bool(r.randint(2)))


def random_graph(cfg, batch=2):
    """x [-> 1x1 conv a1 [-> concat with a side conv: a1 is read from a slice]] -> ConvTranspose "tconv" [-> BN -> ReLU] [-> concat with a side
    ConvTranspose: written into a slice] -> y.  Without the 1x1 conv the op reads the NCHW graph input (through the staging copy).
    -> (model bytes, input shape, output shape)"""
    gb = models.GraphBuilder("convt", 1900 + cfg["seed"])
    cin, cout = cfg["cin"], cfg["cout"]
    if cfg["pre1x1"]:
        u = gb.conv("x", 4, cin, 1, bias=True)
        if cfg["cat_in"]:
            gb.concat([gb.conv("x", 4, 8, 1, bias=True), u])
        ishape = (batch, 4, cfg["h"], cfg["w"])
    else:
        u, ishape = "x", (batch, cin, cfg["h"], cfg["w"])
    y = gb.conv_transpose(u, cin, cout, cfg["k"], cfg["s"], cfg["pads"], cfg["op"], bias=cfg["bias"], name="tconv")
    if cfg["bn_relu"]:
        y = gb.relu(gb.bn(y, cout))
    ctot = cout
    if cfg["cat_out"]:
        y = gb.concat([gb.conv_transpose(u, cin, 8, cfg["k"], cfg["s"], cfg["pads"], cfg["op"], bias=True, name="side"), y])
        ctot += 8
    gb.nodes.append(pb.node("Identity", [y], ["y"], "out"))
    oh, ow = ref64.convt_out_hw(cfg["h"], cfg["w"], cfg["k"], cfg["s"], cfg["pads"], cfg["op"])
    return gb.finish([("x", list(ishape))], [("y", [batch, ctot, oh, ow])]), ishape, (batch, ctot, oh, ow)


def tconv_step(plan):
    (st,) = [s for s in plan["steps"] if s["name"].split("+")[0] == "tconv"]
    return st


def map_case(seed, n, h, w, cin, cout, k, stride, pads=(0, 0, 0, 0), op=(0, 0), bias=False, post=0, half_w=False):
    """x (k/32 grid) -> lifting 1x1 conv 3 -> Cin (exact in half) -> ConvTranspose "conv" [+ bias] -> [BN] -> [ReLU] -> Concat(y, y).
    k, stride: (rows, columns); post: 0 none, 1 ReLU, 2 BN + ReLU, 3 BN; half_w: weights pre-rounded to half-representable values."""
    rs = np.random.RandomState(seed)
    x = G.grid_input(rs, n, h, w)
    w0 = G.lift_weights(rs, cin)
    inits = [pb.tensor("w0", w0)]
    nodes = [pb.node("Conv", ["x", "w0"], ["h0"], "lift", [pb.attr_ints("kernel_shape", [1, 1])])]
    wt = (rs.randn(cin, cout, k[0], k[1]) * np.sqrt(2.0 * stride[0] * stride[1] / (cin * k[0] * k[1]))).astype(f32)
    if half_w:
        wt = R.half_exact(wt)
    d = dict(seed=seed, n=n, h=h, w=w, cin=cin, cout=cout, k=tuple(k), stride=tuple(stride), pads=tuple(pads), op=tuple(op), bias=bias, post=post,
             half_w=half_w, x=x, w0=w0, wt=wt)
    inits.append(pb.tensor("w", wt))
    ins = ["h0", "w"]
    if bias:
        d["bvec"] = (0.2 * rs.randn(cout)).astype(f32)
        inits.append(pb.tensor("bvec", d["bvec"]))
        ins.append("bvec")
    nodes.append(pb.node("ConvTranspose", ins, ["y0"], "conv", [pb.attr_ints("kernel_shape", list(k)), pb.attr_ints("pads", list(pads)),
                                                                pb.attr_ints("strides", list(stride)), pb.attr_ints("output_padding", list(op))]))
    y = "y0"
    if post >= 2:
        d["post_bn"] = G._bn(rs, cout, "post_", inits)
        nodes.append(pb.node("BatchNormalization", [y, "post_g", "post_b", "post_m", "post_v"], ["y1"], "postbn", [pb.attr_float("epsilon", 1e-5)]))
        y = "y1"
    if post in (1, 2):
        nodes.append(pb.node("Relu", [y], ["y2"], "postrelu"))
        y = "y2"
    oh, ow = ref64.convt_out_hw(h, w, k, stride, pads, op)
    nodes.append(pb.node("Concat", [y, y], ["out"], "cat", [pb.attr_int("axis", 1)]))
    g = pb.graph(f"tcase{seed}", nodes, inits, [pb.value_info("x", [n, 3, h, w])], [pb.value_info("out", [n, 2 * cout, oh, ow])])
    d.update(model=pb.model(g), ishape=(n, 3, h, w), oshape=(n, 2 * cout, oh, ow), oh=oh, ow=ow)
    return d


def map_operands(d, x=None, half_weights=False):
    """(cols [M, K], wm [Cout, K], bias or None, relu, rounded_operands) of case `d` in the im2col form (convt_im2col), as the kernel is
    given them: the BN folded into weights and bias in float32 as the planner does it.  x: another input on the same grid (default d["x"]).
    half_weights: the kernel reads the half mirror of the weights, so the step rounds w' to half itself unless it is representable already."""
    xh = G.lifted(d["x"] if x is None else x, d["w0"])
    wt, b = d["wt"], d.get("bvec")
    if d["post"] >= 2:
        p = d["post_bn"]
        s, t = R.bn_affine(p["g"], p["b"], p["m"], p["v"])
        wt = (wt * s.reshape(1, -1, 1, 1)).astype(f32)
        b0 = np.zeros(d["cout"], f32) if b is None else b
        b = ((b0 * s).astype(f32) + t).astype(f32)
    rounded = 1 if half_weights and not np.array_equal(R.half_exact(wt), wt) else 0
    cols, wm, _ = convt_im2col(xh, wt, d["stride"], d["pads"], d["op"])
    return cols, wm, b, d["post"] in (1, 2), rounded


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
    oh, ow = ref64.convt_out_hw(h, wd, (kh, kw), strides, pads, output_padding)
    assert cols.shape[:3] == (n, oh, ow), (cols.shape, (n, oh, ow))
    return cols.reshape(-1, kh * kw * cin), R.wmat(wf), (n, oh, ow)
