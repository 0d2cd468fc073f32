"""CPU: dilated convolutions and Resize / Upsample through the ONNX reader and the planner (EngineDescribeModel): FCN-ResNet50 and
DeepLabV3-ResNet50 step structures in fp32 and fp16, FLOP accounting, the Shape arithmetic of torch's interpolate exports, the refusals, and the
plans of the graphs that loaded before, which must stay byte-identical (tests/golden/plan_sha256_parent.json).  The numpy Resize reference of
ref64.py is checked against torch's F.interpolate where the two definitions coincide."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import ref64
from engine_run import describe
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models
from gpu_ai_inference_server_amd.modelgen import onnx_pb as pb

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_sha256_parent.json")
HASH_NETS = {"densenet121": models.densenet121, "resnet50": models.resnet50, "mobilenet_v2": models.mobilenet_v2,
             "mobilenet_v3_large": lambda b: models.mobilenet_v3(b, variant="large"), "efficientnet_b0": models.efficientnet_b0}


def plan_json(path, batch):
    """The plan's JSON text exactly as the engine writes it (the "plan" member of EngineDescribeModel's document, its last one)."""
    err = C.c_void_p()
    p = B.lib().EngineDescribeModel(path.encode(), batch, C.byref(err))
    if not p:
        raise RuntimeError(B._take_error(err))
    s = B._take_string(p)
    assert s.endswith("}")
    return s[s.index('"plan":') + len('"plan":'):-1]


@pytest.fixture(scope="module")
def nets(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("seg_nets"))
    out = {}
    for name, f in (("fcn", models.fcn_resnet50), ("deeplab", models.deeplabv3_resnet50)):
        mb = f(8)
        out[name] = (mb, models.write_repo(root, name, mb))
    return out


def _check_common(p, mb, batch):
    steps = p["steps"]
    dil = [s for s in steps if "dilations" in s]
    assert dil and all(s["algo"] in ("igemm_vec", "igemm_scalar", "naive") for s in dil)
    # no copies: the final Resize writes the dense NCHW fp32 output itself
    assert not [s for s in steps if s["kind"] == "copy"]
    fin = steps[-1]
    assert fin["kind"] == "resize" and fin["out"]["nchw"] and not fin["out"]["f16"] and (fin["out"]["c"], fin["out"]["h"]) == (21, 224)
    assert fin["resize"] == {"mode": "linear", "coord": "pytorch_half_pixel", "nearest": "round_prefer_floor", "scales": [8, 8]}
    assert p["outputs"][0]["view"]["buf"] == fin["out"]["buf"]
    # FLOPs: 2 x the graph's conv MACs (a collapsed conv counts as its 1x1), + 6 per linear Resize output element
    macs = ref64.conv_macs(mb, (batch, 3, 224, 224))
    convs = [s for s in steps if s["kind"] == "conv"]
    pool = sum(9 * s["out"]["n"] * s["out"]["c"] * s["out"]["h"] * s["out"]["w"] for s in convs if s["algo"] == "stem_pool")
    collapsed = sum(v * 8 // 9 for k, v in macs.items() if k == "aspp3")
    assert sum(s["flops"] for s in convs) - pool == 2 * (sum(macs.values()) - collapsed)
    for s in steps:
        if s["kind"] == "resize":
            assert s["flops"] == 6 * s["out"]["n"] * s["out"]["c"] * s["out"]["h"] * s["out"]["w"]
    return dil


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_fcn_plan(nets, monkeypatch, prec):
    mb, path = nets["fcn"]
    p = describe(path, 8, monkeypatch, prec)
    dil = _check_common(p, mb, 8)
    # stage 3: first block d = 1, five blocks d = 2; stage 4: first block d = 2, two blocks d = 4; all at 28x28, stride 1
    assert [s["dilations"][0] for s in dil] == [2] * 6 + [4] * 2
    assert all(s["out"]["h"] == 28 and s["stride"] == [1, 1] and s["pads"] == [s["dilations"][0]] * 4 for s in dil)
    assert all(s["in"]["f16"] == (prec == "fp16") for s in dil)
    assert len([s for s in p["steps"] if s["kind"] == "resize"]) == 1


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_deeplabv3_plan(nets, monkeypatch, prec):
    mb, path = nets["deeplab"]
    p = describe(path, 8, monkeypatch, prec)
    dil = _check_common(p, mb, 8)
    assert [s["dilations"][0] for s in dil] == [2] * 6 + [4] * 2 + [12, 24]
    steps = p["steps"]
    # the rate-36 branch at 28x28 reads only its centre tap: a 1x1 conv, no dilation
    a3 = [s for s in steps if s["name"].startswith("aspp3")]
    assert len(a3) == 1 and a3[0]["k"] == [1, 1] and a3[0]["pads"] == [0] * 4 and "dilations" not in a3[0]
    # the pooling branch: a [N, 256, 1, 1] input broadcast straight into its slice of the concat buffer
    up = [s for s in steps if s["kind"] == "resize" and s["name"] == "aspp_pool_up"]
    assert len(up) == 1
    u = up[0]
    assert (u["in"]["h"], u["in"]["w"], u["out"]["h"], u["out"]["c"], u["out"]["c_off"], u["out"]["pitch"]) == (1, 1, 28, 256, 1024, 1280)
    proj = [s for s in steps if s["name"].startswith("aspp_proj")][0]
    assert proj["in"]["buf"] == u["out"]["buf"] and proj["in"]["c"] == 1280


@pytest.mark.parametrize("net", [models.fcn_resnet50, models.deeplabv3_resnet50])
def test_shape_chain_plans_like_constant_sizes(tmp_path, net):
    """Shape -> Gather -> Unsqueeze -> Concat -> Cast (torch's export of interpolate(size=...)) plans to exactly the constant-sizes JSON"""
    a = models.write_repo(str(tmp_path), "a", net(4, width=8, image=64, resize="sizes"))
    b = models.write_repo(str(tmp_path), "b", net(4, width=8, image=64, resize="shape"))
    assert plan_json(a, 4) == plan_json(b, 4)


def test_parent_plans_unchanged(tmp_path, monkeypatch):
    golden = json.load(open(GOLDEN))
    paths = {}
    for key, h in golden.items():
        name, prec, b = key.split("/")
        if name not in paths:
            paths[name] = models.write_repo(str(tmp_path), name, HASH_NETS[name]("N"))
        monkeypatch.setenv("IE_PRECISION", prec)
        assert hashlib.sha256(plan_json(paths[name], int(b[1:])).encode()).hexdigest() == h, key


# ---- small graphs ----------------------------------------------------------------------------------------------------------------------
def _dil_graph(name, d, *, k=3, stride=1, pads=None, group=1, c=16, hw=12, ops=()):
    gb = models.GraphBuilder(name, 5)
    x = gb.conv("x", 4, c, 1)
    w = gb.init(name + "_w", np.full((c, c // group, k, k), 0.1, np.float32))
    pads = pads if pads is not None else [d * (k // 2)] * 4
    gb.nodes.append(pb.node("Conv", [x, w], ["y"], name, [pb.attr_ints("dilations", [d, d]), pb.attr_int("group", group),
                                                       pb.attr_ints("kernel_shape", [k, k]), pb.attr_ints("pads", pads),
                                                       pb.attr_ints("strides", [stride, stride])]))
    oh = (hw + pads[0] + pads[2] - (k - 1) * d - 1) // stride + 1
    return gb.finish([("x", [2, 4, hw, hw])], [("y", [2, c, oh, oh])])


def test_dilated_conv_steps_and_forcing(tmp_path, monkeypatch):
    path = models.write_repo(str(tmp_path), "d3", _dil_graph("dconv", 3))
    monkeypatch.setenv("IE_PRECISION", "fp32")
    s = [q for q in B.DescribeModel(path, 2)["plan"]["steps"] if q["name"].startswith("dconv")][0]
    assert s["dilations"] == [3, 3] and s["out"]["h"] == 12 and s["algo"] in ("igemm_vec", "naive")
    assert s["flops"] == 2 * 2 * 12 * 12 * 16 * 9 * 16
    for algo in ("direct", "raster", "wino", "ws", "x6"):       # a forced algo that cannot dilate leaves the planner's choice
        monkeypatch.setenv("IE_FORCE_ALGO", algo)
        q = [q for q in B.DescribeModel(path, 2)["plan"]["steps"] if q["name"].startswith("dconv")][0]
        assert q["algo"] == s["algo"], algo
    monkeypatch.setenv("IE_FORCE_ALGO", "igemm")
    for t in range(16):
        monkeypatch.setenv("IE_FORCE_TILE", str(t))
        q = [q for q in B.DescribeModel(path, 2)["plan"]["steps"] if q["name"].startswith("dconv")][0]
        assert q["algo"] == "igemm_vec" and q["tile"] < 7, t     # the dilated instantiations are the base tiles
    # a 1x1 conv with any dilation is an undilated 1x1; a collapsed conv (d >= H, W) too
    for d, k in ((5, 1), (12, 3)):
        p = models.write_repo(str(tmp_path), f"n{d}", _dil_graph(f"c{d}", d, k=k))
        q = [q for q in B.DescribeModel(p, 2)["plan"]["steps"] if q["name"].startswith(f"c{d}")][0]
        assert q["k"] == [1, 1] and "dilations" not in q and q["pads"] == [0] * 4


@pytest.mark.parametrize("case,match", [
    (dict(group=16), r"Conv dconv: dilated depthwise convolutions are not supported"),
    (dict(group=2), r"Conv dconv: dilated grouped convolutions are not supported"),
])
def test_dilated_group_conv_refused(tmp_path, monkeypatch, case, match):
    monkeypatch.setenv("IE_GROUPED_CONV", "1")
    path = models.write_repo(str(tmp_path), "g", _dil_graph("dconv", 2, **case))
    with pytest.raises(RuntimeError, match=match):
        B.DescribeModel(path, 2)


def test_pool_dilation_refused(tmp_path):
    gb = models.GraphBuilder("pd", 1)
    x = gb.conv("x", 4, 8, 1)
    gb.nodes.append(pb.node("MaxPool", [x], ["y"], "mp", [pb.attr_ints("kernel_shape", [3, 3]), pb.attr_ints("dilations", [2, 2])]))
    path = models.write_repo(str(tmp_path), "pd", gb.finish([("x", [2, 4, 12, 12])], [("y", [2, 8, 8, 8])]))
    with pytest.raises(RuntimeError, match=r"MaxPool mp: dilations != 1 are only supported on Conv"):
        B.DescribeModel(path, 2)


def test_fp8_refusals(tmp_path, monkeypatch):
    monkeypatch.setenv("IE_PRECISION", "fp8")
    path = models.write_repo(str(tmp_path), "d8", _dil_graph("dconv", 2))
    with pytest.raises(RuntimeError, match=r"dilated convolution is not supported in fp8 mode \(Conv dconv\)"):
        B.DescribeModel(path, 2)
    gb = models.GraphBuilder("r8", 1)
    x = gb.conv("x", 4, 16, 1)
    gb.resize(x, (2, 16, 8, 8), sizes=[16, 16], form="sizes", name="up", out="y")
    path = models.write_repo(str(tmp_path), "r8", gb.finish([("x", [2, 4, 8, 8])], [("y", [2, 16, 16, 16])]))
    with pytest.raises(RuntimeError, match=r"Resize is not supported in fp8 mode \(node up\)"):
        B.DescribeModel(path, 2)


def _resize_graph(attrs, extra_inputs, out_hw=(16, 16), op="Resize", opset=13):
    gb = models.GraphBuilder("rz", 1)
    x = gb.conv("x", 4, 16, 1)
    ins = [x] + [gb.init(f"rz_in{i}", v) if v is not None else "" for i, v in enumerate(extra_inputs)]
    gb.nodes.append(pb.node(op, ins, ["y"], "rz", attrs))
    return gb.finish([("x", [2, 4, 8, 8])], [("y", [2, 16, *out_hw])], opset=opset)


@pytest.mark.parametrize("attrs,extra,match", [
    ([pb.attr_str("mode", "cubic")], [None, None, np.array([2, 16, 16, 16], np.int64)], r"rz: mode 'cubic' is not supported"),
    ([pb.attr_str("coordinate_transformation_mode", "tf_crop_and_resize")], [None, None, np.array([2, 16, 16, 16], np.int64)],
     r"rz: coordinate_transformation_mode 'tf_crop_and_resize' is not supported"),
    ([pb.attr_int("antialias", 1)], [None, None, np.array([2, 16, 16, 16], np.int64)], r"rz: antialias = 1 is not supported"),
    ([pb.attr_ints("axes", [1, 2])], [None, None, np.array([16, 16], np.int64)], r"rz: axes must be a subset of \{2, 3\}"),
    ([pb.attr_str("keep_aspect_ratio_policy", "not_larger")], [None, None, np.array([2, 16, 16, 16], np.int64)],
     r"rz: keep_aspect_ratio_policy 'not_larger' is not supported"),
    ([], [None, None, np.array([2, 8, 16, 16], np.int64)], r"rz: only the spatial axes"),
])
def test_resize_refusals(tmp_path, attrs, extra, match):
    path = models.write_repo(str(tmp_path), "rz", _resize_graph(attrs, extra, opset=19))
    with pytest.raises(RuntimeError, match=match):
        B.DescribeModel(path, 2)


def test_resize_forms_and_shape_refusal(tmp_path, monkeypatch):
    # axes = [2, 3] with 2-entry sizes (opset 18+), Resize-10 and Upsample-9 scales: all accepted, asymmetric for the legacy forms
    for name, mb in (("ax", _resize_graph([pb.attr_ints("axes", [2, 3])], [None, None, np.array([16, 16], np.int64)], opset=19)),
                     ("r10", _resize_graph([], [np.array([1, 1, 2, 2], np.float32)], opset=10)),
                     ("u9", _resize_graph([], [np.array([1, 1, 2, 2], np.float32)], op="Upsample", opset=9))):
        p = B.DescribeModel(models.write_repo(str(tmp_path), name, mb), 2)["plan"]
        r = [s for s in p["steps"] if s["kind"] == "resize"][0]
        assert r["out"]["h"] == 16 and r["resize"]["scales"] == [2, 2]
        assert r["resize"]["coord"] == ("half_pixel" if name == "ax" else "asymmetric"), name
    # Shape of an activation feeding anything but a Resize's sizes stays refused
    gb = models.GraphBuilder("sh", 1)
    x = gb.conv("x", 4, 16, 1)
    gb.nodes.append(pb.node("Shape", [x], ["s"], "shp"))
    gb.nodes.append(pb.node("Reshape", [x, "s"], ["y"], "rs"))
    path = models.write_repo(str(tmp_path), "sh", gb.finish([("x", [2, 4, 8, 8])], [("y", [2, 16, 8, 8])]))
    with pytest.raises(RuntimeError, match=r"rs: reads the shape arithmetic of a Shape node"):
        B.DescribeModel(path, 2)


# ---- the numpy Resize reference against torch where the definitions coincide --------------------------------------------------------------
@pytest.mark.parametrize("hw,out", [((7, 9), (21, 27)), ((12, 10), (5, 4)), ((6, 6), (13, 17)), ((1, 1), (5, 6))])
def test_resize_ref_matches_torch(hw, out):
    import torch
    import torch.nn.functional as F
    x = np.random.RandomState(hw[0] * 31 + out[1]).randn(2, 3, *hw)
    t = torch.from_numpy(x)
    sc = (out[0] / hw[0], out[1] / hw[1])
    # bilinear, align_corners=False == pytorch_half_pixel (and half_pixel when the output is not 1 wide)
    ref = F.interpolate(t, size=out, mode="bilinear", align_corners=False).numpy()
    np.testing.assert_allclose(ref64.resize_ref(x, out, sc, "linear", "pytorch_half_pixel"), ref, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(ref64.resize_ref(x, out, sc, "linear", "half_pixel"), ref, rtol=1e-12, atol=1e-12)
    ref = F.interpolate(t, size=out, mode="bilinear", align_corners=True).numpy()
    np.testing.assert_allclose(ref64.resize_ref(x, out, sc, "linear", "align_corners"), ref, rtol=1e-12, atol=1e-12)
    # torch's "nearest" is asymmetric + floor with scale in / out
    ref = F.interpolate(t, size=out, mode="nearest").numpy()
    np.testing.assert_array_equal(ref64.resize_ref(x, out, sc, "nearest", "asymmetric", "floor"), ref)
    # "nearest-exact" is half_pixel + round half up (ties never occur away from x.5 boundaries): round_prefer_ceil
    ref = F.interpolate(t, size=out, mode="nearest-exact").numpy()
    np.testing.assert_array_equal(ref64.resize_ref(x, out, sc, "nearest", "half_pixel", "round_prefer_ceil"), ref)
