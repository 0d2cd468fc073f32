"""CPU: squeeze-excite blocks, HardSwish / HardSigmoid / Sigmoid / SiLU and activation Mul / Div through the ONNX reader and the planner
(EngineDescribeModel): MobileNetV3-Large / -Small and EfficientNet-B0 step structures, FLOP accounting, the export forms, IE_NO_SE_FUSE and the
refusals."""
import numpy as np
import pytest

import ref64
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models
from gpu_ai_inference_server_amd.modelgen import onnx_pb as pb

# SE blocks of the published networks: MobileNetV3-Large 8, -Small 9, EfficientNet-B0 16 (every MBConv block)
NETS = {
    "mnv3_large": (lambda **kw: models.mobilenet_v3("N", variant="large", **kw), 8, 15),
    "mnv3_small": (lambda **kw: models.mobilenet_v3("N", variant="small", **kw), 9, 11),
    "effnet_b0": (lambda **kw: models.efficientnet_b0("N", **kw), 16, 16),
}


@pytest.fixture(scope="module")
def nets(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("senets"))
    return {k: (mb := f(), models.write_repo(root, k, mb)) for k, (f, _, _) in NETS.items()}


def _act(s, key="act"):
    return s.get(key, [None])[0]


def _structure(p):
    return [(s["kind"], s.get("algo") == "depthwise", s.get("residual", False), s["relu"], s.get("clip"), s.get("act"), s.get("pre_act"), s.get("mul", False),
             s.get("se"), s["k"], s["stride"], s["pre"]) for s in p["steps"]]


def _check_plan(name, p, mb, batch):
    _, n_se, n_dw = NETS[name]
    steps = p["steps"]
    ses = [s for s in steps if s["kind"] == "squeeze_excite"]
    dws = [s for s in steps if s.get("algo") == "depthwise"]
    assert len(ses) == n_se and len(dws) == n_dw
    elt = [s for s in steps if s["kind"] == "eltwise"]
    if name == "effnet_b0":
        assert elt == []
        assert all(s["se"]["act1"][0] == "silu" and _act(s) == "sigmoid" for s in ses)
        assert all(_act(s) == "silu" for s in dws)                              # the depthwise epilogues
        assert all(_act(s, "pre_act") == "silu" for s in dws)                   # the expand conv's (or the stem's) SiLU in the prologue
    else:
        # the classifier's Gemm -> HardSwish; MobileNetV3-Large also materialises the stem's hardswish, which its first block reads twice
        # (depthwise conv and identity Add), so it cannot ride on one reader
        assert [_act(s) for s in elt] == ["hardswish"] * (2 if name == "mnv3_large" else 1)
        assert elt[-1]["in"]["h"] * elt[-1]["in"]["w"] == 1
        assert all(s["se"]["act1"][0] == "relu" and s["act"][0] == "hardsigmoid" for s in ses)
        assert all(s["act"][1:] == pytest.approx([1 / 6, 0.5]) for s in ses)
        assert {_act(s) for s in dws} <= {"hardswish", None}
        assert any(_act(s, "pre_act") == "hardswish" for s in dws)
    # an SE reads the depthwise conv's output, its output feeds the projection conv
    for s in ses:
        src = steps[s["in_src"]]
        assert src.get("algo") == "depthwise" and s["in"]["c"] == s["out"]["c"] == src["out"]["c"]
        assert any(q["in_src"] == s["idx"] and q["kind"] == "conv" for q in steps)
    # no eltwise step between an expand conv and its depthwise conv (MobileNetV3-Large's first depthwise conv reads the stem's activation)
    srcs = [steps[d["in_src"]]["kind"] for d in dws]
    assert srcs == ["eltwise" if name == "mnv3_large" else "conv"] + ["conv"] * (n_dw - 1)
    # the head's activation in front of the global pool: its prologue
    (gap,) = [s for s in steps if s["kind"] == "gap"]
    assert _act(gap, "pre_act") == ("silu" if name == "effnet_b0" else "hardswish")
    # FLOPs: the conv steps plus the SE blocks' two FCs = 2 x the MACs of the ONNX graph's convs and Gemms
    macs = sum(ref64.conv_macs(mb, (batch, 3, 224, 224)).values())
    fc = sum(4 * s["in"]["n"] * s["in"]["c"] * s["se"]["mid"] for s in ses)
    assert abs((sum(s["flops"] for s in steps if s["kind"] == "conv") + fc) / (2 * macs) - 1) < 1e-6
    for s in ses:
        esz = 2 if s["in"]["f16"] else 4
        n, c, hw, mid = s["in"]["n"], s["in"]["c"], s["in"]["h"] * s["in"]["w"], s["se"]["mid"]
        assert s["bytes"] == 3 * n * c * hw * esz + 4 * (2 * c * mid + c + mid)
        assert s["se"]["chunks"] >= 1 and s["flops"] > 4 * n * c * mid


@pytest.mark.parametrize("name", list(NETS))
def test_plan_fp32_and_fp16(nets, name, monkeypatch):
    mb, path = nets[name]
    p32 = B.DescribeModel(path, 32)["plan"]
    _check_plan(name, p32, mb, 32)
    monkeypatch.setenv("IE_PRECISION", "fp16")
    p16 = B.DescribeModel(path, 32)["plan"]
    assert p16["precision"] == "fp16"
    _check_plan(name, p16, mb, 32)
    assert _structure(p16) == _structure(p32)


def test_large_maps_split_the_squeeze(nets):
    """EfficientNet's first SE (112 x 112 x 32) at batch 32: 32 workgroups per pixel chunk level are far too few for 256 CUs."""
    steps = B.DescribeModel(nets["effnet_b0"][1], 32)["plan"]["steps"]
    first = [s for s in steps if s["kind"] == "squeeze_excite"][0]
    assert first["in"]["h"] == 112 and first["in"]["c"] == 32 and first["se"]["mid"] == 8
    assert first["se"]["chunks"] * 32 >= 512
    last = [s for s in steps if s["kind"] == "squeeze_excite"][-1]
    assert last["in"]["h"] == 7 and last["se"]["chunks"] == 1


def test_hardswish_export_forms_plan_identically(tmp_path):
    ref = None
    for form in ("op", "hardsigmoid_mul", "mul_hardsigmoid"):
        path = models.write_repo(str(tmp_path), "m_" + form, models.mobilenet_v3("N", variant="small", width_mult=0.5, image=64, classes=10,
                                                                                  act_form=form))
        st = _structure(B.DescribeModel(path, 2)["plan"])
        assert ref is None or st == ref, form
        ref = st


def test_silu_operand_orders_plan_identically(tmp_path):
    ref = None
    for swap in (False, True):
        path = models.write_repo(str(tmp_path), f"e_{swap}", models.efficientnet_b0("N", width_mult=0.5, image=64, classes=10, swap_mul=swap))
        st = _structure(B.DescribeModel(path, 2)["plan"])
        assert ref is None or st == ref, swap
        ref = st
    assert sum(s[0] == "squeeze_excite" for s in ref) == 16


def test_no_se_fuse_gives_the_separate_steps(nets, monkeypatch):
    monkeypatch.setenv("IE_NO_SE_FUSE", "1")
    for name, (_, n_se, _) in NETS.items():
        steps = B.DescribeModel(nets[name][1], 4)["plan"]["steps"]
        assert not any(s["kind"] == "squeeze_excite" for s in steps)
        gates = [s for s in steps if s["kind"] == "eltwise" and s.get("mul")]
        assert len(gates) == n_se and all(s["in2"]["h"] == s["in2"]["w"] == 1 and s["in"]["h"] * s["in"]["w"] > 1 for s in gates)
        assert sum(s["kind"] == "gap" for s in steps) == n_se + 1
        acts = [_act(s) for s in steps if s["kind"] == "eltwise" and not s.get("mul")]
        want_gate = "sigmoid" if name == "effnet_b0" else "hardsigmoid"
        assert acts.count(want_gate) == n_se
        if name == "effnet_b0":
            assert acts.count("silu") == n_se                    # the FC1's SiLU (a Gemm-like conv has no activation epilogue)
        else:
            fc1 = [s for s in steps if s["kind"] == "conv" and s["in"]["h"] * s["in"]["w"] == 1 and s["relu"]]
            assert len(fc1) == n_se


def test_activation_placements(tmp_path):
    """Epilogue of a depthwise conv, prologue of a depthwise conv (the producer runs linear), prologue of a global pool, a stand-alone step;
    Div by a constant is an affine step."""
    gb = models.GraphBuilder("place", 4)
    a = gb.hardswish(gb.bn(gb.conv("x", 16, 16, 1), 16))                          # -> depthwise prologue
    d = gb.silu(gb.conv(a, 16, 16, 3, pad=1, group=16, bias=True))               # -> depthwise epilogue
    e = gb.sigmoid(gb.conv(d, 16, 16, 1, bias=True))                              # dense conv: stand-alone step
    e = gb.simple("Div", [e, gb.init("six", np.array(6.0, np.float32))])
    f = gb.hardsigmoid(gb.conv(e, 16, 16, 1, bias=True), 0.3, 0.4)               # -> the pool's prologue
    gb.nodes.append(pb.node("GlobalAveragePool", [f], ["y"], "gap"))
    path = models.write_repo(str(tmp_path), "place", gb.finish([("x", [2, 16, 9, 9])], [("y", [2, 16, 1, 1])], opset=14))
    s = B.DescribeModel(path, 2)["plan"]["steps"]
    assert [q["kind"] for q in s] == ["conv", "conv", "conv", "eltwise", "conv", "gap"]
    assert "act" not in s[0] and not s[0]["relu"]
    assert s[1]["algo"] == "depthwise" and s[1]["pre_act"] == ["hardswish", pytest.approx(1 / 6), 0.5] and s[1]["act"][0] == "silu"
    assert _act(s[3]) == "sigmoid" and "act" not in s[2]
    assert s[4]["pre"] and "act" not in s[4] and "pre_act" not in s[4]        # the "/ 6" as the next conv's prologue scale
    assert s[5]["pre_act"] == ["hardsigmoid", pytest.approx(0.3), pytest.approx(0.4)]


def test_same_shape_mul_of_two_activations(tmp_path):
    gb = models.GraphBuilder("mul2", 5)
    a = gb.conv("x", 8, 8, 1, bias=True)
    b = gb.conv("x", 8, 8, 3, pad=1, bias=True)
    gb.simple("Mul", [a, b], out="y")
    path = models.write_repo(str(tmp_path), "mul2", gb.finish([("x", [2, 8, 5, 5])], [("y", [2, 8, 5, 5])]))
    (m,) = [q for q in B.DescribeModel(path, 2)["plan"]["steps"] if q["kind"] == "eltwise"]
    assert m["mul"] and m["in2"]["h"] == 5 and "act" not in m


def test_non_broadcastable_mul_is_refused(tmp_path):
    gb = models.GraphBuilder("badmul", 6)
    a = gb.conv("x", 8, 8, 1)
    b = gb.gap(gb.conv("x", 8, 4, 1))
    gb.nodes.append(pb.node("Mul", [a, b], ["y"], "mul_bad"))
    path = models.write_repo(str(tmp_path), "badmul", gb.finish([("x", [1, 8, 6, 6])], [("y", [1, 8, 6, 6])]))
    with pytest.raises(RuntimeError, match=r"Mul mul_bad: only same-shape activations or \[N,C,H,W\] x \[N,C,1,1\] broadcasting"):
        B.DescribeModel(path, 1)


def test_div_by_an_activation_is_refused(tmp_path):
    gb = models.GraphBuilder("baddiv", 6)
    a = gb.conv("x", 8, 8, 1)
    gb.nodes.append(pb.node("Div", [a, a], ["y"], "div_bad"))
    path = models.write_repo(str(tmp_path), "baddiv", gb.finish([("x", [1, 8, 6, 6])], [("y", [1, 8, 6, 6])]))
    with pytest.raises(RuntimeError, match="Div div_bad: only the division of an activation by a constant is supported"):
        B.DescribeModel(path, 1)


@pytest.mark.parametrize("name", list(NETS))
def test_fp8_plan_is_refused(nets, name, monkeypatch):
    monkeypatch.setenv("IE_PRECISION", "fp8")
    with pytest.raises(RuntimeError, match="not supported in fp8 mode"):
        B.DescribeModel(nets[name][1], 4)


def test_activation_graph_without_depthwise_is_refused_in_fp8(tmp_path, monkeypatch):
    gb = models.GraphBuilder("act8", 7)
    y = gb.hardswish(gb.conv("x", 16, 16, 3, pad=1), "op")
    gb.nodes.append(pb.node("GlobalAveragePool", [y], ["y"], "gap"))
    path = models.write_repo(str(tmp_path), "act8", gb.finish([("x", [2, 16, 8, 8])], [("y", [2, 16, 1, 1])], opset=14))
    monkeypatch.setenv("IE_PRECISION", "fp8")
    with pytest.raises(RuntimeError, match=r"activation and squeeze-excite nodes .* are not supported in fp8 mode \(node hardswish_2\)"):
        B.DescribeModel(path, 2)
