"""CPU: depthwise convolutions and Clip through the ONNX reader and the planner (EngineDescribeModel): MobileNetV2's step structure,
FLOP accounting, every Clip export form, and the refusals (non-depthwise groups, fp8)."""
import os

import numpy as np
import pytest

import ref64
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models
from gpu_ai_inference_server_amd.modelgen import onnx_pb as pb


@pytest.fixture(scope="module")
def mnv2(tmp_path_factory):
    mb = models.mobilenet_v2("N")
    return mb, models.write_repo(str(tmp_path_factory.mktemp("mnv2")), "mobilenet_v2", mb)


def _structure(p):
    return [(s["kind"], s.get("algo") == "depthwise", s.get("residual", False), s["relu"], s.get("clip"), s.get("pre_clip"), s["k"], s["stride"])
            for s in p["steps"]]


def _check_mobilenet_plan(p, mb, batch):
    steps = p["steps"]
    convs = [s for s in steps if s["kind"] == "conv"]
    gemm = [s for s in convs if s["in"]["h"] * s["in"]["w"] == 1]
    dws = [s for s in convs if s["algo"] == "depthwise"]
    # 52 convolutions (stem, 17 depthwise, 16 expand, 17 project, head) + the classifier Gemm, which the planner also runs as a conv step
    assert len(convs) - len(gemm) == 52 and len(gemm) == 1
    assert len(dws) == 17 and all(s["k"] == [3, 3] and s["pads"] == [1, 1, 1, 1] for s in dws)
    assert sorted(s["stride"][0] for s in dws) == [1] * 13 + [2] * 4
    assert sum(s["residual"] for s in convs) == 10 and not any(s["residual"] for s in dws)      # the identity Adds ride on the projections
    assert all(s["kind"] != "eltwise" or s["clip"] == [0, 6] for s in steps)
    assert sum(s["kind"] == "eltwise" for s in steps) <= 1                                         # (the ReLU6 in front of the global pool)
    # every depthwise conv: its own ReLU6 in the epilogue; the expanded input's ReLU6 split over the producer's ReLU and the prologue bound
    assert all(s["clip"] == [0, 6] and s["bias"] for s in dws)
    assert all(s["pre"] and s["pre_relu"] and s["pre_clip"] == 6 for s in dws)
    producers = [steps[s["in_src"]] for s in dws]
    assert all(q["kind"] == "conv" and q["relu"] and "clip" not in q for q in producers)
    assert not any("clip" in s or "pre_clip" in s for s in convs if s["algo"] != "depthwise")
    # FLOPs: 2 x the MACs of the ONNX graph's convs and Gemm
    macs = sum(ref64.conv_macs(mb, (batch, 3, 224, 224)).values())
    conv_flops = sum(s["flops"] for s in convs)
    assert abs(conv_flops / (2 * macs) - 1) < 1e-6
    assert p["total_flops"] >= conv_flops and abs(p["total_flops"] / (2 * macs) - 1) < 0.01
    for s in dws:
        assert s["flops"] == 2 * s["out"]["n"] * s["out"]["c"] * s["out"]["h"] * s["out"]["w"] * 9
        esz = 2 if s["in"]["f16"] else 4
        assert s["bytes"] == (s["in"]["n"] * s["in"]["c"] * s["in"]["h"] * s["in"]["w"] + s["out"]["n"] * s["out"]["c"] * s["out"]["h"] * s["out"]["w"]) * esz + 4 * 9 * s["out"]["c"]


def test_mobilenet_v2_plan_fp32(mnv2):
    mb, path = mnv2
    d = B.DescribeModel(path, 32)
    p = d["plan"]
    assert p["precision"] == "fp32"
    _check_mobilenet_plan(p, mb, 32)
    # the fast channel-vector variants take every depthwise conv of the network (all channel counts are multiples of 8)
    assert all(s["tile"] in (1, 2, 3) for s in p["steps"] if s.get("algo") == "depthwise")


def test_mobilenet_v2_plan_fp16_same_structure(mnv2, monkeypatch):
    mb, path = mnv2
    p32 = B.DescribeModel(path, 32)["plan"]
    monkeypatch.setenv("IE_PRECISION", "fp16")
    p16 = B.DescribeModel(path, 32)["plan"]
    assert p16["precision"] == "fp16"
    assert _structure(p16) == _structure(p32)
    _check_mobilenet_plan(p16, mb, 32)
    assert all(s["in"]["f16"] and s["out"]["f16"] for s in p16["steps"] if s.get("algo") == "depthwise")


def test_clip_export_forms_plan_identically(tmp_path):
    ref = None
    for form in ("initializer", "constant", "attrs"):
        path = models.write_repo(str(tmp_path), "m_" + form, models.mobilenet_v2("N", width_mult=0.5, image=64, classes=10, clip_form=form))
        p = B.DescribeModel(path, 2)["plan"]
        st = _structure(p)
        assert ref is None or st == ref, form
        ref = st
    # min-only / max-only, as attributes, initializers and Constant nodes: a stand-alone clamp with the missing bound open
    for form in ("attrs", "initializer", "constant"):
        for lo, hi, want in ((0.25, None, [0.25, None]), (None, 1.5, [None, 1.5])):
            gb = models.GraphBuilder("clip1", 3)
            y = gb.clip(gb.conv("x", 8, 8, 1, bias=True), lo, hi, form)
            gb.nodes.append(pb.node("GlobalAveragePool", [y], ["y"], "gap"))
            mb = gb.finish([("x", [2, 8, 6, 6])], [("y", [2, 8, 1, 1])], opset=6 if form == "attrs" else 13)
            path = models.write_repo(str(tmp_path), f"c_{form}_{lo}_{hi}", mb)
            steps = B.DescribeModel(path, 2)["plan"]["steps"]
            elt = [s for s in steps if s["kind"] == "eltwise"]
            assert len(elt) == 1 and elt[0]["clip"] == want and not elt[0]["relu"], (form, steps)


def test_clip_into_depthwise_epilogue_and_prologue(tmp_path):
    """The three placements: a depthwise conv's epilogue, ReLU6 split between a conv's ReLU and a depthwise prologue, a stand-alone step."""
    gb = models.GraphBuilder("place", 4)
    a = gb.clip(gb.conv("x", 16, 16, 1, bias=True), 0.0, 6.0)                  # -> conv ReLU + depthwise prologue bound
    d = gb.clip(gb.conv(a, 16, 16, 3, pad=1, group=16, bias=True), -1.0, 2.0)   # -> depthwise epilogue [-1, 2]
    e = gb.clip(gb.conv(d, 16, 16, 1, bias=True), -0.5, 0.5)                   # dense conv: stand-alone clamp
    gb.nodes.append(pb.node("GlobalAveragePool", [e], ["y"], "gap"))
    path = models.write_repo(str(tmp_path), "place", gb.finish([("x", [2, 16, 9, 9])], [("y", [2, 16, 1, 1])]))
    s = B.DescribeModel(path, 2)["plan"]["steps"]
    assert [q["kind"] for q in s] == ["conv", "conv", "conv", "eltwise", "gap"]
    assert s[0]["relu"] and "clip" not in s[0]
    assert s[1]["algo"] == "depthwise" and s[1]["pre_relu"] and s[1]["pre_clip"] == 6 and s[1]["clip"] == [-1, 2]
    assert s[3]["clip"] == [-0.5, 0.5]


def test_depthwise_fusions_and_slices(tmp_path):
    """Pre-activation BN + ReLU as the prologue, BN folded, a residual Add in the epilogue, input and output in concat slices."""
    gb = models.GraphBuilder("dwfuse", 5)
    a1 = gb.conv("x", 8, 24, 1, bias=True)
    a2 = gb.conv("x", 8, 8, 1, bias=True)
    cat0 = gb.concat([a2, a1])
    u = gb.relu(gb.bn(a1, 24))
    d = gb.bn(gb.conv(u, 24, 24, 5, pad=2, group=24), 24)
    d = gb.simple("Add", [d, a1])
    side = gb.conv(cat0, 32, 8, 1)
    gb.concat([d, side])
    gb.nodes[-1] = pb.node("Concat", [d, side], ["y"], "cat_out", [pb.attr_int("axis", 1)])
    path = models.write_repo(str(tmp_path), "dwfuse", gb.finish([("x", [2, 8, 11, 11])], [("y", [2, 32, 11, 11])]))
    steps = B.DescribeModel(path, 2)["plan"]["steps"]
    (dw,) = [s for s in steps if s.get("algo") == "depthwise"]
    assert dw["pre"] and dw["pre_relu"] and "pre_clip" not in dw and dw["bias"] and dw["residual"] and "clip" not in dw
    assert dw["in"]["c_off"] == 8 and dw["in"]["pitch"] == 32 and dw["in2"]["c_off"] == 8
    assert dw["out"]["c_off"] == 0 and dw["out"]["pitch"] == 32 and dw["k"] == [5, 5] and dw["tile"] in (1, 2, 3)


def test_non_depthwise_group_is_refused(tmp_path):
    gb = models.GraphBuilder("grouped", 6)
    y = gb.conv("x", 8, 8, 3, pad=1, group=2)
    gb.nodes.append(pb.node("GlobalAveragePool", [y], ["y"], "gap"))
    path = models.write_repo(str(tmp_path), "grouped", gb.finish([("x", [1, 8, 6, 6])], [("y", [1, 8, 1, 1])]))
    with pytest.raises(RuntimeError, match=r"group = 2 is not supported \(only depthwise grouped convolutions"):
        B.DescribeModel(path, 1)


def test_clip_bound_must_be_a_scalar_constant(tmp_path):
    gb = models.GraphBuilder("badclip", 7)
    y = gb.conv("x", 4, 4, 1)
    gb.nodes.append(pb.node("Clip", [y, gb.init("lo2", np.zeros(4, np.float32))], ["y"], "clip_vec"))
    path = models.write_repo(str(tmp_path), "badclip", gb.finish([("x", [1, 4, 1, 1])], [("y", [1, 4, 1, 1])]))
    with pytest.raises(RuntimeError, match="Clip clip_vec: the min bound must be a floating-point scalar"):
        B.DescribeModel(path, 1)
    gb = models.GraphBuilder("badclip2", 7)
    y = gb.conv("x", 4, 4, 1)
    gb.nodes.append(pb.node("Clip", [y, "x"], ["y"], "clip_act"))
    path = models.write_repo(str(tmp_path), "badclip2", gb.finish([("x", [1, 4, 1, 1])], [("y", [1, 4, 1, 1])]))
    with pytest.raises(RuntimeError, match="Clip clip_act: the min bound must be a constant"):
        B.DescribeModel(path, 1)


def test_fp8_plan_of_a_depthwise_graph_is_refused(mnv2, monkeypatch):
    monkeypatch.setenv("IE_PRECISION", "fp8")
    with pytest.raises(RuntimeError, match="depthwise convolution is not supported in fp8 mode"):
        B.DescribeModel(mnv2[1], 4)


def test_forced_switches_keep_depthwise_steps_on_the_depthwise_kernel(mnv2, monkeypatch):
    path = mnv2[1]
    for algo in ("naive", "igemm", "ws", "direct", "raster"):
        monkeypatch.setenv("IE_FORCE_ALGO", algo)
        steps = B.DescribeModel(path, 2)["plan"]["steps"]
        assert sum(s.get("algo") == "depthwise" for s in steps) == 17, algo
    monkeypatch.delenv("IE_FORCE_ALGO")
    for t in (0, 1, 2, 3, 7):
        monkeypatch.setenv("IE_FORCE_TILE", str(t))
        dws = [s for s in B.DescribeModel(path, 2)["plan"]["steps"] if s.get("algo") == "depthwise"]
        assert len(dws) == 17 and all(s["tile"] == (t if t < 4 else (3 if s["out"]["w"] >= 14 else 2)) for s in dws), t
