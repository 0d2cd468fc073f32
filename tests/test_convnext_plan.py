"""CPU: ConvNeXt through the ONNX reader and the planner (EngineDescribeModel): the channels-last views (a Transpose is never a step), the
layer-norm steps and their tiles, the block's two Linear layers as 1x1 convs with the bias, the layer scale and the residual folded into the
second, the GELU spellings, the refusals, and plan digests.  tests/golden/plan_digests_convnext.json pins ConvNeXt-Tiny's plans and weight blob.
The float64 reference of tests/ref64.py is checked against torch's own layer norm.

    python tests/test_convnext_plan.py            # rewrites tests/golden/plan_digests_convnext.json from the built library
"""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    from _pkg import load_package
    load_package()

import ref64  # noqa: E402
from convnext_graphs import LANES, ln_default_tile, ln_graph, ln_tile_fits, narrow  # noqa: E402
import test_plan_digests as D  # noqa: E402
from engine_run import describe  # noqa: E402
from gpu_ai_inference_server_amd import binding as B  # noqa: E402
from gpu_ai_inference_server_amd.modelgen import models  # noqa: E402
from gpu_ai_inference_server_amd.modelgen import onnx_pb as pb  # noqa: E402
from oracle import onnx_oracle as O  # noqa: E402
from refusals import refused  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "plan_digests_convnext.json")
PRECS = ("fp32", "fp16")
DEPTHS, DIMS = (3, 3, 9, 3), (96, 192, 384, 768)


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    mb = models.convnext_tiny("N")
    return models.write_repo(str(tmp_path_factory.mktemp("convnext")), "convnext_tiny", mb), mb


# ---- ConvNeXt-Tiny -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("batch", [1, 32])
def test_convnext_tiny_plan(tiny, monkeypatch, prec, batch):
    path, _ = tiny
    p = describe(path, batch, monkeypatch, prec)
    steps = p["steps"]
    f16 = prec == "fp16"
    # a Transpose is a view: no copy anywhere (the stem conv reads the NCHW input itself, the [N, classes] output needs none), and the only
    # eltwise steps are the blocks' GELUs
    assert [s["name"] for s in steps if s["kind"] == "copy"] == []
    assert "transpose" not in json.dumps([s["name"] for s in steps]).lower()
    elt = [s for s in steps if s["kind"] == "eltwise"]
    assert len(elt) == sum(DEPTHS) and all(s["act"] == ["gelu", 0, 0] and not s["pre"] and not s["relu"] and "in2" not in s for s in elt)
    lns = [s for s in steps if s["kind"] == "layer_norm"]
    assert len(lns) == sum(DEPTHS) + 3 + 2                  # one per block, one per downsample, the stem's and the head's
    assert [s["kind"] for s in steps].count("gap") == 1
    i = 0

    def take(kind):
        nonlocal i
        s = steps[i]
        i += 1
        assert s["kind"] == kind, (i - 1, s["kind"], kind, s["name"])
        return s

    def check_ln(s, name, c, hw, eps=1e-6):
        assert s["name"] == name and s["eps"] == float(np.float32(eps)) and s["bias"] and s["w_off"] >= 0 and s["bias_off"] >= 0
        assert (s["in"]["n"], s["in"]["c"], s["in"]["h"], s["in"]["w"]) == (batch, c, hw, hw) == (s["out"]["n"], s["out"]["c"], s["out"]["h"], s["out"]["w"])
        assert s["tile"] == ln_default_tile(c, s["out"]["f16"]) and s["in"]["f16"] == s["out"]["f16"]
        assert s["flops"] == 8 * batch * hw * hw * c and s["bytes"] == 2 * (2 if s["out"]["f16"] else 4) * batch * hw * hw * c

    stem = take("conv")
    assert stem["name"] == "stem" and stem["k"] == [4, 4] and stem["stride"] == [4, 4] and stem["bias"] and stem["in"]["nchw"]
    check_ln(take("layer_norm"), "stem_ln", 96, 56)
    hw = 56
    for si, (depth, c) in enumerate(zip(DEPTHS, DIMS)):
        if si:
            check_ln(take("layer_norm"), f"down{si}_ln", DIMS[si - 1], hw)
            d = take("conv")
            hw //= 2
            assert d["name"] == f"down{si}" and d["k"] == [2, 2] and d["stride"] == [2, 2] and d["bias"] and (d["out"]["c"], d["out"]["h"]) == (c, hw)
        for bi in range(depth):
            tag = f"s{si}b{bi}"
            dw = take("conv")
            assert dw["name"] == tag + "_dw" and dw["algo"] == "depthwise" and dw["k"] == [7, 7] and dw["pads"] == [3, 3, 3, 3] and dw["bias"] and not dw["residual"]
            assert dw["tile"] == 0                                           # the channel-vector tiles stop at k = 5
            check_ln(take("layer_norm"), tag + "_ln", c, hw)
            fc1 = take("conv")
            assert fc1["k"] == [1, 1] and fc1["algo"] not in ("depthwise", "grouped") and fc1["bias"] and not fc1["residual"] and not fc1["relu"]
            assert (fc1["in"]["c"], fc1["out"]["c"], fc1["out"]["h"], fc1["out"]["w"]) == (c, 4 * c, hw, hw) and fc1["name"].count("+") == 1
            g = take("eltwise")
            assert g["in"]["c"] == 4 * c and g["name"].count("+") == 4
            fc2 = take("conv")
            # Add b2, the layer scale and the block's shortcut all ride in the second Linear layer
            assert fc2["k"] == [1, 1] and fc2["bias"] and fc2["residual"] and not fc2["relu"] and fc2["name"].count("+") == 3
            assert (fc2["in"]["c"], fc2["out"]["c"], fc2["in2"]["c"], fc2["in2"]["h"]) == (4 * c, c, c, hw)
            assert fc2["in2"]["buf"] == dw["in"]["buf"] and fc2["in2"]["c_off"] == dw["in"]["c_off"]
    assert take("gap")["out"]["c"] == 768
    head = take("layer_norm")                                                # the [N, C, 1, 1] head
    assert head["name"] == "head_ln" and (head["in"]["n"], head["in"]["c"], head["in"]["h"], head["in"]["w"]) == (batch, 768, 1, 1)
    assert head["tile"] == ln_default_tile(768, head["out"]["f16"])
    fc = take("conv")
    assert fc["out"]["c"] == 1000 and i == len(steps)
    assert p["outputs"][0]["dims"] == [batch, 1000]
    assert all(s["in"]["f16"] == f16 for s in lns[:-1])


def test_layer_scale_folds_into_the_second_linear(tiny, monkeypatch):
    """fc2's planned weights are diag(scale) . W2^T and its bias scale * b2, computed here from the file's initializers"""
    path, mb = tiny
    p = describe(path, 1, monkeypatch, "fp32")
    blob = B.PlanWeights(path, 1)
    inits = O.load_model(mb).inits
    for tag in ("s0b0", "s2b4"):
        (ln,) = [k for k, s in enumerate(p["steps"]) if s["name"] == tag + "_ln"]
        fc1, fc2 = p["steps"][ln + 1], p["steps"][ln + 3]
        c = fc2["out"]["c"]
        scale = inits[tag + "_scale"].reshape(c).astype(np.float32)
        w2 = (scale[:, None] * inits[tag + "_fc2_w"].T.astype(np.float32)).astype(np.float32)                 # [Cout][Cin]
        np.testing.assert_allclose(blob[fc2["w_off"]:fc2["w_off"] + 4 * c * c].reshape(c, 4 * c), w2, rtol=1e-6, atol=0)
        np.testing.assert_allclose(blob[fc2["bias_off"]:fc2["bias_off"] + c], scale * inits[tag + "_fc2_b"], rtol=1e-6, atol=1e-9)
        np.testing.assert_array_equal(blob[fc1["w_off"]:fc1["w_off"] + 4 * c * c].reshape(4 * c, c), inits[tag + "_fc1_w"].T)
        np.testing.assert_array_equal(blob[fc1["bias_off"]:fc1["bias_off"] + 4 * c], inits[tag + "_fc1_b"])
        lnp = p["steps"][ln]
        np.testing.assert_array_equal(blob[lnp["w_off"]:lnp["w_off"] + c], inits[tag + "_ln_scale"])
        np.testing.assert_array_equal(blob[lnp["bias_off"]:lnp["bias_off"] + c], inits[tag + "_ln_B"])


# ---- GELU spellings ----------------------------------------------------------------------------------------------------------------------
def test_gelu_spellings_give_the_same_activation(tmp_path, monkeypatch):
    plans = {}
    for form, swap in (("erf", False), ("erf", True), ("erf_mul", False), ("erf_mul", True), ("op", False), ("op_tanh", False)):
        path = models.write_repo(str(tmp_path), f"g_{form}_{int(swap)}", narrow(gelu=form, gelu_swap=swap))
        steps = describe(path, 2, monkeypatch, "fp32")["steps"]
        plans[form, swap] = [(s["kind"], s.get("act"), s.get("algo"), s.get("tile"), s["in"]["c"], s["out"]["c"], s.get("residual")) for s in steps]
        acts = [s["act"] for s in steps if s["kind"] == "eltwise"]
        assert acts == [["gelu_tanh" if form == "op_tanh" else "gelu", 0, 0]] * 5, (form, swap, acts)
    exact = [v for k, v in plans.items() if k[0] != "op_tanh"]
    assert all(v == exact[0] for v in exact)


def test_near_miss_of_the_erf_pattern_is_refused(tmp_path, monkeypatch):
    """0.6 in place of 0.5 is not a GELU: the Erf stays, and Erf alone is not an operator the engine runs"""
    gb = models.GraphBuilder("g", 3)
    y = gb.gelu(gb.conv("x", 4, 8, 1), "erf", half=0.6)
    gb.nodes.append(pb.node("Identity", [y], ["y"], "out"))
    path = models.write_repo(str(tmp_path), "near", gb.finish([("x", [2, 4, 6, 6])], [("y", [2, 8, 6, 6])], opset=17))
    refused(path, 2, monkeypatch, match=r"Unsupported ONNX operator: Erf \(node erf_\d+\)")
    # the same graph with 0.5 plans; an Erf whose Div output has a second reader does not
    gb = models.GraphBuilder("g", 3)
    y = gb.gelu(gb.conv("x", 4, 8, 1), "erf")
    gb.nodes.append(pb.node("Identity", [y], ["y"], "out"))
    path = models.write_repo(str(tmp_path), "hit", gb.finish([("x", [2, 4, 6, 6])], [("y", [2, 8, 6, 6])], opset=17))
    assert [s.get("act") for s in describe(path, 2, monkeypatch, "fp32")["steps"] if s["kind"] == "eltwise"] == [["gelu", 0, 0]]
    gb = models.GraphBuilder("g", 3)
    x = gb.conv("x", 4, 8, 1)
    d = gb.simple("Div", [x, gb.init("sqrt2", np.array(np.sqrt(2.0), np.float32))])
    e = gb.simple("Add", [gb.simple("Erf", [d]), gb.init("one", np.array(1.0, np.float32))])
    y = gb.simple("Mul", [gb.simple("Mul", [x, e]), gb.init("half", np.array(0.5, np.float32))])
    gb.nodes.append(pb.node("Add", [y, d], ["y"], "out"))
    path = models.write_repo(str(tmp_path), "shared", gb.finish([("x", [2, 4, 6, 6])], [("y", [2, 8, 6, 6])], opset=17))
    refused(path, 2, monkeypatch, match="Unsupported ONNX operator: Erf")


def test_gelu_behind_a_depthwise_conv_takes_the_generic_tile(tmp_path, monkeypatch):
    """The depthwise conv absorbs the activation; its channel-vector tiles know the sigmoid family only, so the step runs on tile 0"""
    for act, want in (("gelu", 0), ("silu", 3)):
        gb = models.GraphBuilder("g", 3)
        y = gb.conv(gb.conv("x", 4, 16, 1), 16, 16, 3, pad=1, group=16, name="dw")
        y = gb.gelu(y, "op") if act == "gelu" else gb.silu(y)
        gb.nodes.append(pb.node("Identity", [y], ["y"], "out"))
        path = models.write_repo(str(tmp_path), "dw" + act, gb.finish([("x", [2, 4, 16, 16])], [("y", [2, 16, 16, 16])], opset=20))
        for forced in (None, "2"):
            (dw,) = [s for s in describe(path, 2, monkeypatch, "fp32", **({} if forced is None else {"IE_FORCE_TILE": forced}))["steps"] if s.get("algo") == "depthwise"]
            assert dw["act"][0] == act and dw["tile"] == (0 if act == "gelu" else int(forced or want)), (act, forced, dw["tile"])


# ---- layer-norm tiles -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_layer_norm_tiles(tmp_path, monkeypatch, prec):
    """default tile and IE_FORCE_TILE per channel count: an ineligible forced tile is the generic kernel, a value past the table changes nothing"""
    for c in (6, 8, 96, 100, 768, 1536, 1540):
        path = models.write_repo(str(tmp_path), f"ln{c}", ln_graph(2, c, 3, 5))
        got = {}
        for forced in (None, "0", "1", "2", "3", "4", "5"):
            steps = describe(path, 2, monkeypatch, prec, **({} if forced is None else {"IE_FORCE_TILE": forced}))["steps"]
            assert [s["kind"] for s in steps] == ["copy", "layer_norm", "copy"]         # the NCHW graph input and output; nothing for the Transposes
            got[forced] = steps[1]["tile"]
        fits = [t for t in (1, 2, 3, 4) if ln_tile_fits(c, prec == "fp16", t)]
        assert got[None] == got["5"] == ln_default_tile(c, prec == "fp16"), (c, got)
        assert [got[str(t)] for t in range(5)] == [0] + [t if t in fits else 0 for t in (1, 2, 3, 4)], (c, got)
    assert ln_default_tile(96, False) == 1 and ln_default_tile(768, True) == 3 and ln_default_tile(1536, False) == 4 and ln_default_tile(1540, False) == 0


def test_layer_norm_on_a_matrix(tmp_path, monkeypatch):
    """[N, C] values take axis -1 or 1"""
    for axis in (-1, 1):
        gb = models.GraphBuilder("ln2", 9)
        y = gb.layernorm(gb.simple("Flatten", [gb.gap(gb.conv("x", 4, 24, 1))], [pb.attr_int("axis", 1)]), 24, axis=axis, name="ln")
        gb.nodes.append(pb.node("Identity", [y], ["y"], "out"))
        path = models.write_repo(str(tmp_path), f"m{axis}", gb.finish([("x", [3, 4, 6, 6])], [("y", [3, 24])], opset=17))
        (ln,) = [s for s in describe(path, 3, monkeypatch, "fp32")["steps"] if s["kind"] == "layer_norm"]
        assert (ln["in"]["n"], ln["in"]["c"], ln["in"]["h"], ln["in"]["w"]) == (3, 24, 1, 1)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def _refused(tmp_path, monkeypatch, name, build, ishape, oshape, match, prec="fp32"):
    gb = models.GraphBuilder("r", 3)
    y = build(gb)
    gb.nodes.append(pb.node("Identity", [y], ["y"], "out"))
    path = models.write_repo(str(tmp_path), name, gb.finish([("x", ishape)], [("y", oshape)], opset=17))
    refused(path, ishape[0], monkeypatch, prec=prec, match=match)


def test_refusals(tmp_path, monkeypatch):
    x4, c = [2, 8, 6, 6], 8
    _refused(tmp_path, monkeypatch, "perm", lambda gb: gb.transpose("x", (0, 2, 1, 3)), x4, [2, 6, 8, 6],
             r"Transpose transpose_\d+: perm \[0,2,1,3\] on an NCHW value of rank 4 is not supported \(only \[0,2,3,1\] on a 4-D NCHW value and \[0,3,1,2\] on its channels-last view are\)")
    _refused(tmp_path, monkeypatch, "twice", lambda gb: gb.transpose(gb.transpose("x", (0, 2, 3, 1)), (0, 2, 3, 1)), x4, x4,
             r"Transpose transpose_\d+: perm \[0,2,3,1\] on a channels-last view is not supported")
    _refused(tmp_path, monkeypatch, "back", lambda gb: gb.transpose("x", (0, 3, 1, 2)), x4, x4,
             r"Transpose transpose_\d+: perm \[0,3,1,2\] on an NCHW value of rank 4 is not supported")
    _refused(tmp_path, monkeypatch, "conv", lambda gb: gb.conv(gb.transpose("x", (0, 2, 3, 1)), 6, 4, 1, name="c"), x4, [2, 4, 8, 6],
             r"Conv c: input transpose_\d+_out is a channels-last view \(a Transpose with perm \[0,2,3,1\]\); only LayerNormalization, MatMul, Add, Mul, Div, Erf, Gelu and "
             r"Transpose may read one")
    _refused(tmp_path, monkeypatch, "pool", lambda gb: gb.gap(gb.transpose("x", (0, 2, 3, 1))), x4, [2, 6, 1, 1], r"GlobalAveragePool gap_\d+: input transpose_\d+_out is a channels-last view")
    _refused(tmp_path, monkeypatch, "concat", lambda gb: gb.concat([gb.transpose("x", (0, 2, 3, 1)), gb.transpose("x", (0, 2, 3, 1))]), x4, [2, 12, 6, 8],
             r"Concat concat_\d+: input transpose_\d+_out is a channels-last view")
    # (the folded ops too: Shape of a view would be folded from the value's NCHW dims)
    def shape_of_view(gb):
        gb.nodes.append(pb.node("Shape", [gb.transpose("x", (0, 2, 3, 1))], ["shp"], "shape_of_view"))
        return "x"
    _refused(tmp_path, monkeypatch, "shape", shape_of_view, x4, x4,
             r"Shape shape_of_view: input transpose_\d+_out is a channels-last view \(a Transpose with perm \[0,2,3,1\]\)")
    _refused(tmp_path, monkeypatch, "flatten", lambda gb: gb.simple("Flatten", [gb.transpose("x", (0, 2, 3, 1))], [pb.attr_int("axis", 1)]), [2, 8, 1, 1], [2, 8],
             r"Flatten flatten_\d+: input transpose_\d+_out is a channels-last view")
    _refused(tmp_path, monkeypatch, "output", lambda gb: gb.layernorm(gb.transpose("x", (0, 2, 3, 1)), c), x4, [2, 6, 6, 8],
             r"Identity out: input ln_\d+_out is a channels-last view")
    _refused(tmp_path, monkeypatch, "axis1", lambda gb: gb.layernorm("x", 8, axis=1, name="ln"), x4, x4,
             r"LayerNormalization ln: axis = 1 on an NCHW value of rank 4 is not supported \(only the channel axis alone is normalised: the last axis of a channels-last view "
             r"or of an \[N, C\] value\)")
    _refused(tmp_path, monkeypatch, "axis2", lambda gb: gb.transpose(gb.layernorm(gb.transpose("x", (0, 2, 3, 1)), 8, axis=2, name="ln"), (0, 3, 1, 2)), x4, x4,
             r"LayerNormalization ln: axis = 2 on a channels-last view is not supported")
    _refused(tmp_path, monkeypatch, "bcast", lambda gb: gb.transpose(gb.simple("Mul", [gb.transpose("x", (0, 2, 3, 1)), gb.init("s", np.ones((8, 1, 1), np.float32))]), (0, 3, 1, 2)),
             x4, x4, r"Mul mul_\d+: constant operand must broadcast along the last axis of the channels-last view transpose_\d+_out")
    _refused(tmp_path, monkeypatch, "mixed", lambda gb: gb.transpose(gb.simple("Add", [gb.transpose("x", (0, 2, 3, 1)), gb.conv("x", 8, 6, 1, name="c")]), (0, 3, 1, 2)),
             [2, 8, 8, 6], [2, 8, 8, 6], r"Add add_\d+: the operands mix a channels-last view and an NCHW value")


def test_channels_last_graph_output_is_refused(tmp_path, monkeypatch):
    gb = models.GraphBuilder("r", 3)
    y = gb.layernorm(gb.transpose("x", (0, 2, 3, 1)), 8, name="ln")
    path = models.write_repo(str(tmp_path), "clout", gb.finish([("x", [2, 8, 6, 6])], [(y, [2, 6, 6, 8])], opset=17))
    refused(path, 2, monkeypatch, match=r"graph output ln_out is a channels-last view")


def test_fp8_is_refused(tiny, tmp_path, monkeypatch):
    path, _ = tiny
    refused(path, 1, monkeypatch, prec="fp8", match=r"^LayerNormalization is not supported in fp8 mode \(node stem_ln\)$")
    # without a LayerNormalization in front of it, a GELU falls under the activation refusal
    gb = models.GraphBuilder("g", 3)
    y = gb.gelu(gb.conv("x", 16, 16, 1), "erf")
    gb.nodes.append(pb.node("Identity", [y], ["y"], "out"))
    p8 = models.write_repo(str(tmp_path), "g8", gb.finish([("x", [2, 16, 6, 6])], [("y", [2, 16, 6, 6])], opset=17))
    refused(p8, 2, monkeypatch, prec="fp8", match=r"^activation and squeeze-excite nodes .* are not supported in fp8 mode")


# ---- the reference ------------------------------------------------------------------------------------------------------------------------
def test_reference_layer_norm_is_torchs():
    assert ref64.ln_agrees_with_torch() < 1e-12
    # and the walk of a block: the op spelling and the Erf pattern are the same function
    x = np.random.RandomState(0).randn(2, 8, 6, 6)
    ys = [ref64.run_f64(models.convnext_block(2, 8, 6, gelu=g, gelu_swap=sw), {"x": x})["y"] for g, sw in (("erf", False), ("erf_mul", True), ("op", False))]
    assert ys[0].shape == (2, 8, 6, 6) and ref64.rel_err(ys[1], ys[0]) < 1e-7 and ref64.rel_err(ys[2], ys[0]) < 1e-7     # (the constants are float32)


# ---- digests ------------------------------------------------------------------------------------------------------------------------------
def _entries():
    """(key, batch, switches): ConvNeXt-Tiny in every precision at batch 1 and 32, and IE_FORCE_TILE 0-4 (the layer-norm tiles) at batch 32"""
    out = [(f"convnext_tiny/{prec}/b{b}", b, {"IE_PRECISION": prec}) for prec in ("fp32", "fp16", "fp8") for b in (1, 32)]
    out += [(f"convnext_tiny/{prec}/b32/IE_FORCE_TILE={t}", 32, {"IE_PRECISION": prec, "IE_FORCE_TILE": str(t)}) for prec in PRECS for t in range(5)]
    return out


def _digests(path):
    return {key: D.digest(path, batch, sw) for key, batch, sw in _entries()}


def test_convnext_plan_digests(tiny, engine_lib):
    want = D.load_golden(GOLDEN)
    got = _digests(tiny[0])
    assert sorted(got) == sorted(want)
    bad = {k: (want[k], v) for k, v in got.items() if want[k] != v}
    assert not bad, "%d of %d entries differ from %s (golden, now): %s" % (len(bad), len(got), os.path.basename(GOLDEN), json.dumps(bad, indent=1)[:4000])
    assert sum("error" in v for v in got.values()) == 2               # the two fp8 entries: refusals


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as root:
        D.save_golden(_digests(models.write_repo(root, "convnext_tiny", models.convnext_tiny("N"))), sys.argv[1] if len(sys.argv) > 1 else GOLDEN)
    print(GOLDEN)
