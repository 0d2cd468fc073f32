"""Transition graphs for the pooled 1x1 conv kernel (test infrastructure; used by tests/test_pooled_conv_plan.py and tests/test_pooled_conv_gpu.py).

    x (k/32 grid) -> lifting 1x1 conv 3 -> K (exact, kernel_graphs) -> [BN [-> ReLU]] -> Conv 1x1 K -> Cout [+ bias] -> AveragePool 2x2 / s2 -> Concat(y, y)
                                                                 +-> GlobalAveragePool (second output: keeps the lifted tensor's buffer alive)

The planner's own swap (fusion 2c) turns the tail into pool (with the BN / ReLU prologue) -> conv on a quarter of the pixels: the pair the executor
may run as one launch.  `near_miss` builds the single-graph cases that look like the pair and must stay split.
"""
import numpy as np

import kernel_graphs as G
import kernel_ref as R
from gpu_ai_inference_server_amd.modelgen import onnx_pb as pb

f32, f64 = np.float32, np.float64


def transition_case(seed, n, h, w, k, cout, bn=True, relu=True, bias=False):
    rs = np.random.RandomState(seed)
    x = G.grid_input(rs, n, h, w)
    w0 = G.lift_weights(rs, k)
    inits = [pb.tensor("w0", w0)]
    nodes = [pb.node("Conv", ["x", "w0"], ["h0"], "lift", [pb.attr_ints("kernel_shape", [1, 1])])]
    d = dict(seed=seed, n=n, h=h, w=w, k=k, cout=cout, bn=bn, relu=relu and bn, bias=bias, x=x, w0=w0)
    t = "h0"
    if bn:
        d["pre_bn"] = G._bn(rs, k, "pre_", inits)
        nodes.append(pb.node("BatchNormalization", [t, "pre_g", "pre_b", "pre_m", "pre_v"], ["p0"], "prebn", [pb.attr_float("epsilon", 1e-5)]))
        t = "p0"
        if relu:
            nodes.append(pb.node("Relu", ["p0"], ["p1"], "prerelu"))
            t = "p1"
    d["wt"] = (rs.randn(cout, k, 1, 1) * np.sqrt(2.0 / k)).astype(f32)
    inits.append(pb.tensor("w", d["wt"]))
    ins = [t, "w"]
    if bias:
        d["bvec"] = (0.2 * rs.randn(cout)).astype(f32)
        inits.append(pb.tensor("bvec", d["bvec"]))
        ins.append("bvec")
    nodes.append(pb.node("Conv", ins, ["y0"], "conv", [pb.attr_ints("kernel_shape", [1, 1])]))
    nodes.append(pb.node("AveragePool", ["y0"], ["y1"], "pool", [pb.attr_ints("kernel_shape", [2, 2]), pb.attr_ints("strides", [2, 2])]))
    nodes.append(pb.node("Concat", ["y1", "y1"], ["out"], "cat", [pb.attr_int("axis", 1)]))
    # the lifted tensor stays alive behind the transition (a second output reads it last), so its buffer is not recycled for the conv's output: a
    # launch that reads the pool's input while it stores the conv's output could not run on a shared buffer, and the executor would leave it split
    nodes.append(pb.node("GlobalAveragePool", ["h0"], ["aux"], "aux"))
    oh, ow = h // 2, w // 2
    g = pb.graph(f"trans{seed}", nodes, inits, [pb.value_info("x", [n, 3, h, w])], [pb.value_info("out", [n, 2 * cout, oh, ow]), pb.value_info("aux", [n, k, 1, 1])])
    d.update(model=pb.model(g), ishape=(n, 3, h, w), oshape=(n, 2 * cout, oh, ow), oh=oh, ow=ow)
    return d


def _windows(a):
    """NCHW -> the four window positions (ky, kx) of a 2x2 / stride-2 pool, each [N, C, H/2, W/2]."""
    return [a[:, :, ky::2, kx::2] for ky in (0, 1) for kx in (0, 1)]


def pooled_operands(d):
    """What the conv behind the pool is given, per pooled activation [M, K]:
        cols32   the fp32 emulation of the pool step (fma prologue, ReLU, the window summed in (ky, kx) order from +0, times 0.25f)
        cols64   the float64 pooled activations of the graph's own BatchNormalization (what S is formed from)
        mabs64   mean |window| of the float64 activations (test_pool_maps' scale of the pool's own roundings)"""
    xh = G.lifted(d["x"], d["w0"])
    a32, a64 = xh, xh.astype(f64)
    if d["bn"]:
        p = d["pre_bn"]
        s, t = R.bn_affine(p["g"], p["b"], p["m"], p["v"])
        a32 = (xh.astype(f64) * s.reshape(1, -1, 1, 1).astype(f64) + t.reshape(1, -1, 1, 1).astype(f64)).astype(f32)      # one rounding: the FMA
        sc = p["g"].astype(f64) / np.sqrt(p["v"].astype(f64) + float(f32(1e-5)))
        a64 = (xh.astype(f64) - p["m"].astype(f64).reshape(1, -1, 1, 1)) * sc.reshape(1, -1, 1, 1) + p["b"].astype(f64).reshape(1, -1, 1, 1)
        if d["relu"]:
            a32, a64 = np.maximum(a32, f32(0)), np.maximum(a64, 0.0)
    acc = np.zeros_like(_windows(a32)[0])
    for win in _windows(a32):
        acc = (acc + win).astype(f32)
    p32 = (acc * f32(0.25)).astype(f32)
    p64 = sum(_windows(a64)) / 4.0
    m64 = sum(np.abs(v) for v in _windows(a64)) / 4.0
    flat = lambda t_: np.ascontiguousarray(t_.transpose(0, 2, 3, 1)).reshape(-1, d["k"])
    return flat(p32), flat(p64), flat(m64)


def two_copies(ym, d):
    y = R.to_nchw(ym, (d["n"], d["oh"], d["ow"]))
    return np.concatenate([y, y], axis=1)


# ---------------------------------------------------------------------------------------------------------------------
# near misses: graphs that resemble pool -> 1x1 conv and must not be paired
# ---------------------------------------------------------------------------------------------------------------------
def near_miss(kind, n=2, h=8, w=8, k=64, cout=64, seed=900):
    """kind: avg3s2 (3x3 / stride 2 average pool), max (max pool), padded (2x2 pool with padding), pool_output (the pooled value is also a graph
    output), residual (the conv has a residual Add).  The pool is written IN FRONT of the conv (no swap needed): lift -> BN -> ReLU -> pool -> conv."""
    rs = np.random.RandomState(seed)
    x = G.grid_input(rs, n, h, w)
    inits = [pb.tensor("w0", G.lift_weights(rs, k))]
    nodes = [pb.node("Conv", ["x", "w0"], ["h0"], "lift", [pb.attr_ints("kernel_shape", [1, 1])])]
    G._bn(rs, k, "pre_", inits)
    nodes.append(pb.node("BatchNormalization", ["h0", "pre_g", "pre_b", "pre_m", "pre_v"], ["p0"], "prebn", [pb.attr_float("epsilon", 1e-5)]))
    nodes.append(pb.node("Relu", ["p0"], ["p1"], "prerelu"))
    op, ks, st, pads = "AveragePool", 2, 2, [0, 0, 0, 0]
    if kind == "avg3s2":
        ks, pads = 3, [1, 1, 1, 1]
    elif kind == "max":
        op = "MaxPool"
    elif kind == "padded":
        pads = [1, 1, 1, 1]
    oh = (h + pads[0] + pads[2] - ks) // st + 1
    ow = (w + pads[1] + pads[3] - ks) // st + 1
    nodes.append(pb.node(op, ["p1"], ["pooled"], "pool", [pb.attr_ints("kernel_shape", [ks, ks]), pb.attr_ints("strides", [st, st]), pb.attr_ints("pads", pads)]))
    inits.append(pb.tensor("w", (rs.randn(cout, k, 1, 1) * np.sqrt(2.0 / k)).astype(f32)))
    nodes.append(pb.node("Conv", ["pooled", "w"], ["y0"], "conv", [pb.attr_ints("kernel_shape", [1, 1])]))
    outs = []
    y = "y0"
    if kind == "residual":
        assert cout == k
        nodes.append(pb.node("Add", ["y0", "pooled"], ["y1"], "add"))
        y = "y1"
    nodes.append(pb.node("Concat", [y, y], ["out"], "cat", [pb.attr_int("axis", 1)]))
    outs.append(pb.value_info("out", [n, 2 * cout, oh, ow]))
    if kind == "pool_output":
        outs.append(pb.value_info("pooled", [n, k, oh, ow]))
    g = pb.graph(f"miss_{kind}", nodes, inits, [pb.value_info("x", [n, 3, h, w])], outs)
    return dict(model=pb.model(g), x=x, ishape=(n, 3, h, w))


def entry_slice_case(n=2, h=8, w=8, k=64, seed=910):
    """A transition (BN -> ReLU -> Conv 1x1 k -> 128 -> AveragePool) whose result is concatenated BEHIND another tensor before the next
    BN -> ReLU -> Conv 1x1: the entry conv reads the whole concat buffer, a different view than the slice the transition conv writes."""
    rs = np.random.RandomState(seed)
    x = G.grid_input(rs, n, h, w)
    inits = [pb.tensor("w0", G.lift_weights(rs, k))]
    nodes = [pb.node("Conv", ["x", "w0"], ["h0"], "lift", [pb.attr_ints("kernel_shape", [1, 1])]),
             pb.node("MaxPool", ["h0"], ["other"], "side", [pb.attr_ints("kernel_shape", [2, 2]), pb.attr_ints("strides", [2, 2])])]
    G._bn(rs, k, "pre_", inits)
    nodes.append(pb.node("BatchNormalization", ["h0", "pre_g", "pre_b", "pre_m", "pre_v"], ["p0"], "prebn", [pb.attr_float("epsilon", 1e-5)]))
    nodes.append(pb.node("Relu", ["p0"], ["p1"], "prerelu"))
    inits.append(pb.tensor("w", (rs.randn(128, k, 1, 1) * np.sqrt(2.0 / k)).astype(f32)))
    nodes.append(pb.node("Conv", ["p1", "w"], ["y0"], "conv", [pb.attr_ints("kernel_shape", [1, 1])]))
    nodes.append(pb.node("AveragePool", ["y0"], ["y1"], "pool", [pb.attr_ints("kernel_shape", [2, 2]), pb.attr_ints("strides", [2, 2])]))
    nodes.append(pb.node("Concat", ["other", "y1"], ["cat"], "cat", [pb.attr_int("axis", 1)]))
    G._bn(rs, k + 128, "e_", inits)
    nodes.append(pb.node("BatchNormalization", ["cat", "e_g", "e_b", "e_m", "e_v"], ["e0"], "ebn", [pb.attr_float("epsilon", 1e-5)]))
    nodes.append(pb.node("Relu", ["e0"], ["e1"], "erelu"))
    inits.append(pb.tensor("we", (rs.randn(128, k + 128, 1, 1) * np.sqrt(2.0 / (k + 128))).astype(f32)))
    nodes.append(pb.node("Conv", ["e1", "we"], ["e2"], "entry", [pb.attr_ints("kernel_shape", [1, 1])]))
    nodes.append(pb.node("Concat", ["e2", "e2"], ["out"], "cat2", [pb.attr_int("axis", 1)]))
    g = pb.graph("miss_entry_slice", nodes, inits, [pb.value_info("x", [n, 3, h, w])], [pb.value_info("out", [n, 256, h // 2, w // 2])])
    return dict(model=pb.model(g), x=x, ishape=(n, 3, h, w))
