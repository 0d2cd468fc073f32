"""CPU: ConvTranspose through the ONNX reader and the planner (EngineDescribeModel): U-Net's step structure in fp32 and fp16, the fusions the
transposed step takes and leaves, FLOP accounting, the refusals, the forcing switches, the random test graphs' eligibility for the MFMA kernel,
and plan digests.  tests/golden/plan_digests_unet.json pins U-Net's plans and weight blob; tests/golden/plan_digests_unet_resize_parent.json
pins the bilinear-upsample variant (no transposed conv in the graph) as the commit BEFORE this operator planned it: it must not move.
The references of tests/ref64.py are checked against each other.

    python tests/test_convt_plan.py            # rewrites tests/golden/plan_digests_unet.json from the built library
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

import convt_graphs as TG  # noqa: E402
import kernel_ref as R  # noqa: E402
import test_plan_digests as D  # noqa: E402
import ref64  # noqa: E402
from engine_run import describe  # noqa: E402
from gpu_ai_inference_server_amd import binding as B  # noqa: E402
from gpu_ai_inference_server_amd.modelgen import models  # noqa: E402
from gpu_ai_inference_server_amd.modelgen import onnx_pb as pb  # noqa: E402

GOLDEN_UNET = os.path.join(HERE, "golden", "plan_digests_unet.json")
GOLDEN_RESIZE = os.path.join(HERE, "golden", "plan_digests_unet_resize_parent.json")
PRECS = ("fp32", "fp16")


@pytest.fixture(scope="module")
def unet_path(tmp_path_factory):
    return models.write_repo(str(tmp_path_factory.mktemp("unet")), "unet", models.unet("N"))


# ---- U-Net ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("batch", [1, 8])
def test_unet_plan(unet_path, monkeypatch, prec, batch):
    p = describe(unet_path, batch, monkeypatch, prec)
    steps = p["steps"]
    ts = [s for s in steps if s.get("algo") == "transposed"]
    assert len(ts) == 4 and all(s["name"].startswith(f"up{lv}+up{lv}_bn+relu_") for s, lv in zip(ts, (3, 2, 1, 0))), [s["name"] for s in ts]
    for s, lv in zip(ts, (3, 2, 1, 0)):
        c, hw = 64 << lv, 224 >> lv
        assert s["kind"] == "conv" and s["k"] == [2, 2] and s["stride"] == [2, 2] and s["pads"] == [0, 0, 0, 0] and s["output_padding"] == [0, 0]
        assert (s["in"]["n"], s["in"]["c"], s["in"]["h"], s["in"]["w"]) == (batch, 2 * c, hw // 2, hw // 2)
        assert (s["out"]["n"], s["out"]["c"], s["out"]["h"], s["out"]["w"]) == (batch, c, hw, hw)
        # BatchNorm folded into weights and bias, the ReLU in the epilogue, nothing else fused
        assert s["relu"] and s["bias"] and not s["pre"] and not s["pre_relu"] and not s["residual"] and "act" not in s and "clip" not in s
        # the second member of the skip concat [skip, up]: written straight into the concat's buffer
        assert (s["out"]["c_off"], s["out"]["pitch"]) == (c, 2 * c)
        skip = [q for q in steps if q["name"].startswith(f"enc{lv}_c2")]
        assert len(skip) == 1 and skip[0]["out"]["buf"] == s["out"]["buf"] and (skip[0]["out"]["c_off"], skip[0]["out"]["pitch"]) == (0, 2 * c)
        assert s["in"]["f16"] == s["out"]["f16"] == (prec == "fp16")
        assert s["tile"] in (1, 2) and s["splitk"] == 1                       # Cin 128 .. 1024: the MFMA kernel
        assert s["flops"] == 2 * batch * (hw // 2) ** 2 * 2 * c * c * 4
        assert s["bytes"] == (4 if prec == "fp32" else 2) * (batch * 2 * c * (hw // 2) ** 2 + batch * c * hw * hw + 2 * c * c * 4)
    # the only copy: the NCHW graph output
    assert [s["name"] for s in steps if s["kind"] == "copy"] == ["to_output(out)"]
    assert "output_padding" not in json.dumps([s for s in steps if s.get("algo") != "transposed"])
    assert p["outputs"][0]["dims"] == [batch, 2, 224, 224]


@pytest.mark.parametrize("prec", PRECS)
def test_unet_sigmoid_and_small(tmp_path, monkeypatch, prec):
    path = models.write_repo(str(tmp_path), "us", models.unet(2, image=96, base=16, final="sigmoid"))
    p = describe(path, 2, monkeypatch, prec)
    ts = [s for s in p["steps"] if s.get("algo") == "transposed"]
    assert len(ts) == 4 and [s["out"]["h"] for s in ts] == [12, 24, 48, 96]
    # fp32 K-step 8, fp16 K-step 16: Cin = 256 .. 32 all take the MFMA kernel
    assert all(s["tile"] >= 1 for s in ts)
    assert [s for s in p["steps"] if s["kind"] == "eltwise" and s.get("act", [""])[0] == "sigmoid"]


def test_forcing_switches(unet_path, monkeypatch):
    """IE_FORCE_ALGO is ignored for transposed steps; IE_FORCE_TILE picks the variant where eligible, other values leave the planner's choice"""
    base = [s["tile"] for s in describe(unet_path, 8, monkeypatch, "fp32")["steps"] if s.get("algo") == "transposed"]
    assert base == [1, 1, 1, 2]
    for algo in ("naive", "igemm", "ws", "direct", "raster"):
        got = [(s["algo"], s["tile"]) for s in describe(unet_path, 8, monkeypatch, "fp32", IE_FORCE_ALGO=algo)["steps"] if s["name"].startswith("up")]
        assert got == [("transposed", t) for t in base], algo
    monkeypatch.delenv("IE_FORCE_ALGO")
    for t in (0, 1, 2):
        got = [s["tile"] for s in describe(unet_path, 8, monkeypatch, "fp32", IE_FORCE_TILE=str(t))["steps"] if s.get("algo") == "transposed"]
        assert got == [t] * 4
    got = [s["tile"] for s in describe(unet_path, 8, monkeypatch, "fp32", IE_FORCE_TILE="3")["steps"] if s.get("algo") == "transposed"]
    assert got == base


def test_fast_tile_needs_the_non_overlapping_geometry(tmp_path, monkeypatch):
    """3x3/s2/p1/op1, 4x4/s2/p1 and a 64x64/s32 FCN head stay on the generic kernel, forced tile or not; 4x4/s4 and (2, 4)/(2, 4) are eligible"""
    for name, (k, s, p, op, want) in dict(a=(3, 2, 1, 1, 0), b=(4, 2, 1, 0, 0), c=(64, 32, 16, 0, 0), d=(4, 4, 0, 0, 1), e=((2, 4), (2, 4), 0, 0, 1),
                                          f=(8, 8, 0, 0, 0)).items():
        gb = models.GraphBuilder("g", 3)
        y = gb.conv_transpose(gb.conv("x", 4, 16, 1), 16, 8, k, s, p, op, name="tconv")
        gb.nodes.append(pb.node("Identity", [y], ["y"], "out"))
        kk, ss = (k, k) if isinstance(k, int) else k, (s, s) if isinstance(s, int) else s
        oh, ow = ref64.convt_out_hw(6, 6, kk, ss, (p,) * 4, (op, op))
        path = models.write_repo(str(tmp_path), name, gb.finish([("x", [2, 4, 6, 6])], [("y", [2, 8, oh, ow])]))
        for forced in (None, "1", "2"):
            env = {} if forced is None else dict(IE_FORCE_TILE=forced)
            st = TG.tconv_step(describe(path, 2, monkeypatch, "fp32", **env))
            monkeypatch.delenv("IE_FORCE_TILE", raising=False)
            assert (st["out"]["h"], st["out"]["w"]) == (oh, ow)
            assert st["tile"] == (0 if not want else int(forced or 1)), (name, forced, st["tile"])


def test_fusions_not_taken(tmp_path, monkeypatch):
    """A pre-activation BN -> ReLU in front, a residual Add, a Clip and an activation behind a transposed conv stay separate steps; a
    transposed conv over the NCHW graph input reads a staged NHWC copy"""
    gb = models.GraphBuilder("nf", 5)
    a = gb.conv("x", 4, 16, 1, bias=True)
    t1 = gb.conv_transpose(gb.relu(gb.bn(a, 16)), 16, 16, 2, 2, name="t1")
    t2 = gb.conv_transpose(a, 16, 16, 2, 2, name="t2")
    s = gb.simple("Add", [t2, t1])
    t3 = gb.clip(gb.conv_transpose(s, 16, 16, 1, 1, name="t3"), 0.0, 6.0)
    t4 = gb.sigmoid(gb.conv_transpose(t3, 16, 8, 3, 1, 1, name="t4"))
    t5 = gb.conv_transpose("x", 4, 8, 3, 1, 1, name="t5")
    gb.nodes.append(pb.node("Identity", [t4], ["y"], "out"))
    gb.nodes.append(pb.node("Identity", [t5], ["z"], "out2"))
    path = models.write_repo(str(tmp_path), "nf", gb.finish([("x", [2, 4, 6, 6])], [("y", [2, 8, 12, 12]), ("z", [2, 8, 6, 6])]))
    for prec in PRECS:
        steps = describe(path, 2, monkeypatch, prec)["steps"]
        ts = {s["name"]: s for s in steps if s.get("algo") == "transposed"}
        assert sorted(ts) == ["t1", "t2", "t3", "t4", "t5"], sorted(ts)             # nothing rode along
        for s in ts.values():
            assert not s["pre"] and not s["pre_relu"] and not s["residual"] and not s["relu"] and "clip" not in s and "act" not in s and not s["in"]["nchw"]
        kinds = [(s["kind"], s["name"]) for s in steps if s["kind"] in ("eltwise", "copy")]
        assert ("copy", "nchw_to_nhwc(x)") in kinds
        assert sum(k == "eltwise" for k, _ in kinds) == 4, kinds                    # BN + ReLU, Add, Clip, Sigmoid


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def _one_node(attrs, weight="init", wshape=(8, 6, 3, 3), out_hw=(13, 13)):
    gb = models.GraphBuilder("r", 1)
    rs = np.random.RandomState(0)
    ins = ["x"]
    if weight == "init":
        ins.append(gb.init("w", rs.randn(*wshape).astype(np.float32)))
    else:           # the weight is a second graph input
        ins.append("w")
    gb.nodes.append(pb.node("ConvTranspose", ins, ["y"], "ct", attrs))
    return gb.finish([("x", [2, 8, 6, 6])] + ([] if weight == "init" else [("w", list(wshape))]), [("y", [2, wshape[1], *out_hw])])


S2 = [pb.attr_ints("strides", [2, 2])]


@pytest.mark.parametrize("attrs,kw,match", [
    (S2 + [pb.attr_int("group", 2)], dict(wshape=(8, 3, 3, 3)), r"ConvTranspose ct: group = 2 is not supported"),
    (S2 + [pb.attr_ints("dilations", [2, 1])], {}, r"ConvTranspose ct: dilated transposed convolutions are not supported \(dilations 2x1\)"),
    (S2 + [pb.attr_str("auto_pad", "SAME_UPPER")], {}, r"ConvTranspose ct: auto_pad SAME_UPPER is not supported"),
    (S2 + [pb.attr_str("auto_pad", "SAME_LOWER")], {}, r"ConvTranspose ct: auto_pad SAME_LOWER is not supported"),
    (S2 + [pb.attr_ints("output_shape", [12, 12])], {}, r"ConvTranspose ct: the output_shape attribute is not supported"),
    (S2 + [pb.attr_ints("output_padding", [2, 0])], {}, r"ConvTranspose ct: output_padding 2x0 must be smaller than the strides 2x2"),
    ([pb.attr_ints("output_padding", [0, 1])], {}, r"ConvTranspose ct: output_padding 0x1 must be smaller than the strides 1x1"),
    (S2, dict(weight="input"), r"ConvTranspose ct: weights must be a 4-D initializer"),
    ([pb.attr_ints("pads", [4, 0, 4, 0])], dict(wshape=(8, 6, 3, 3)), r"ConvTranspose ct: the output would be empty \(0x8\)"),
])
def test_refusals(tmp_path, attrs, kw, match):
    path = models.write_repo(str(tmp_path), "r", _one_node(attrs, **kw))
    with pytest.raises(RuntimeError, match=match):
        B.DescribeModel(path, 2)


def test_accepted_attribute_forms(tmp_path, monkeypatch):
    """auto_pad NOTSET / VALID (VALID ignores the pads), kernel_shape absent, a bias"""
    for i, (attrs, hw) in enumerate([(S2 + [pb.attr_str("auto_pad", "NOTSET"), pb.attr_ints("pads", [1, 1, 1, 1])], 11),
                                     (S2 + [pb.attr_str("auto_pad", "VALID"), pb.attr_ints("pads", [1, 1, 1, 1])], 13),
                                     (S2 + [pb.attr_ints("kernel_shape", [3, 3]), pb.attr_ints("output_padding", [1, 1])], 14)]):
        path = models.write_repo(str(tmp_path), f"ok{i}", _one_node(attrs, out_hw=(hw, hw)))
        (st,) = [s for s in describe(path, 2, monkeypatch, "fp32")["steps"] if s.get("algo") == "transposed"]
        assert (st["out"]["h"], st["out"]["w"], st["out"]["c"]) == (hw, hw, 6)


def test_fp8_refusal(tmp_path, monkeypatch):
    monkeypatch.setenv("IE_PRECISION", "fp8")
    path = models.write_repo(str(tmp_path), "r8", _one_node(S2))
    with pytest.raises(RuntimeError, match=r"ConvTranspose is not supported in fp8 mode \(node ct\)"):
        B.DescribeModel(path, 2)
    path = models.write_repo(str(tmp_path), "u8", models.unet("N", image=32, base=16, depth=2))
    with pytest.raises(RuntimeError, match=r"ConvTranspose is not supported in fp8 mode \(node up1\)"):
        B.DescribeModel(path, 2)


# ---- the random graphs of the GPU test ------------------------------------------------------------------------------------------------------
def test_random_cases_are_valid_and_a_third_is_eligible(tmp_path, monkeypatch):
    """Every generated case plans (no invalid shape), with the planned output extents; at least a third of the cases of each precision take
    the MFMA kernel by the planner's choice, and IE_FORCE_TILE=0 moves every one of them to the generic kernel"""
    for prec in PRECS:
        fast = 0
        for seed in range(TG.NUM_SEEDS):
            cfg = TG.random_case(seed)
            mb, ishape, oshape = TG.random_graph(cfg)
            assert min(oshape) >= 1
            path = models.write_repo(str(tmp_path), f"c{seed}", mb)
            st = TG.tconv_step(describe(path, 2, monkeypatch, prec))
            assert st["algo"] == "transposed" and (st["out"]["h"], st["out"]["w"]) == oshape[2:] and st["output_padding"] == cfg["op"]
            assert st["relu"] == cfg["bn_relu"] and st["bias"] == (cfg["bias"] or cfg["bn_relu"])
            assert (st["out"]["pitch"] > st["out"]["c"]) == cfg["cat_out"] and (st["in"]["pitch"] > st["in"]["c"]) == cfg["cat_in"]
            fast += st["tile"] > 0
            if st["tile"] > 0:
                assert cfg["k"] == cfg["s"] and cfg["pads"] == [0] * 4 and cfg["op"] == [0, 0] and cfg["cin"] % (16 if prec == "fp16" else 8) == 0
            assert TG.tconv_step(describe(path, 2, monkeypatch, prec, IE_FORCE_TILE="0"))["tile"] == 0
            monkeypatch.delenv("IE_FORCE_TILE")
        assert 3 * fast >= TG.NUM_SEEDS, (prec, fast)
    assert TG.NUM_SEEDS >= 24
    cases = [TG.random_case(s) for s in range(TG.NUM_SEEDS)]
    assert any(c["pads"][0] != c["pads"][2] or c["pads"][1] != c["pads"][3] for c in cases) and any(c["op"] != [0, 0] for c in cases)
    assert {c["cin"] for c in cases} >= {3, 8, 16, 64} and {c["cout"] for c in cases} == set(TG.COUTS)


# ---- the references against each other ----------------------------------------------------------------------------------------------------
def _ref_case(seed):
    r = np.random.RandomState(7000 + seed)
    k = (int(r.randint(1, 6)), int(r.randint(1, 6)))
    s = (int(r.randint(1, 5)), int(r.randint(1, 5)))
    sym = seed % 2 == 0
    pt, pl = int(r.randint(0, k[0])), int(r.randint(0, k[1]))
    pads = (pt, pl, pt, pl) if sym else (pt, pl, int(r.randint(0, k[0])), int(r.randint(0, k[1])))
    op = (int(r.randint(0, s[0])), int(r.randint(0, s[1])))
    n, cin, cout, h, w = int(r.randint(1, 3)), int(r.randint(1, 7)), int(r.randint(1, 6)), int(r.randint(3, 8)), int(r.randint(3, 8))
    return dict(k=k, s=s, pads=pads, op=op, sym=sym, x=r.randn(n, cin, h, w), w=r.randn(cin, cout, *k), b=r.randn(cout))


@pytest.mark.parametrize("seed", range(40))
def test_references_agree(seed):
    """numpy scatter == torch double F.conv_transpose2d (symmetric pads) == the im2col form the bound is computed on, to 1e-12"""
    c = _ref_case(seed)
    y = ref64.convt_scatter(c["x"], c["w"], c["b"], c["s"], c["pads"], c["op"])
    scale = np.abs(y).max()
    if c["sym"]:
        yt = ref64.convt_torch(c["x"], c["w"], c["b"], c["s"], c["pads"][:2], c["op"])
        assert yt.shape == y.shape and np.abs(yt - y).max() <= 1e-12 * scale
    cols, wm, shape = TG.convt_im2col(c["x"], c["w"], c["s"], c["pads"], c["op"])
    ref, S = R.ref64_S(cols, wm, c["b"])
    assert np.abs(R.to_nchw(ref, shape) - y).max() <= 1e-12 * scale
    assert np.all(R.to_nchw(S, shape) >= np.abs(y) - 1e-12 * scale)


def test_float64_walk_uses_the_scatter_for_asymmetric_pads():
    cfg = dict(TG.random_case(3), k=[3, 2], s=[2, 3], pads=[0, 1, 2, 0], op=[1, 2], cin=6, cout=5, pre1x1=False, cat_in=False, bias=True, bn_relu=False,
               cat_out=False)
    mb, ishape, oshape = TG.random_graph(cfg)
    x = np.random.RandomState(1).randn(*ishape)
    from oracle import onnx_oracle as O
    m = O.load_model(mb)
    y = ref64.run_f64(mb, {"x": x})["y"]
    assert y.shape == oshape
    np.testing.assert_allclose(y, ref64.convt_scatter(x, m.inits["tconv_w"], m.inits["tconv_b"], (2, 3), (0, 1, 2, 0), (1, 2)), rtol=0, atol=1e-12)


# ---- digests ------------------------------------------------------------------------------------------------------------------------------
def _unet_entries(up):
    """(key, file key, builder, batch, switches): the full net at batch 1 / 8 / 32, a narrow one with the forcing switches"""
    out = []
    for prec in ("fp32", "fp16", "fp8"):
        for b in (1, 8, 32):
            out.append((f"unet_{up}/{prec}/b{b}", f"unet_{up}", lambda: models.unet("N", up=up), b, {"IE_PRECISION": prec}))
    for prec in PRECS:
        for sw in ({"IE_FORCE_TILE": "0"}, {"IE_FORCE_TILE": "1"}, {"IE_FORCE_TILE": "2"}, {"IE_FORCE_TILE": "9"}, {"IE_FORCE_ALGO": "naive"}, {"IE_FORCE_ALGO": "igemm"}):
            key = "/".join([f"unet_{up}_w16", prec, "b8"] + ["%s=%s" % kv for kv in sorted(sw.items())])
            out.append((key, f"unet_{up}_w16", lambda: models.unet("N", up=up, base=16, image=64), 8, {"IE_PRECISION": prec, **sw}))
    return out


def _unet_digests(up, root):
    paths, out = {}, {}
    for key, fk, thunk, batch, sw in _unet_entries(up):
        if fk not in paths:
            paths[fk] = models.write_repo(root, fk, thunk())
        out[key] = D.digest(paths[fk], batch, sw)
    return out


@pytest.mark.parametrize("up,golden", [("convtranspose", GOLDEN_UNET), ("resize", GOLDEN_RESIZE)])
def test_unet_plan_digests(tmp_path, engine_lib, up, golden):
    want = D.load_golden(golden)
    got = _unet_digests(up, str(tmp_path))
    assert sorted(got) == sorted(want)
    bad = {k: (want[k], v) for k, v in got.items() if want[k] != v}
    assert not bad, "%d of %d entries differ from %s (golden, now): %s" % (len(bad), len(got), os.path.basename(golden), json.dumps(bad, indent=1)[:4000])
    if up == "convtranspose":
        assert sum("error" in v for v in got.values()) == 3           # the three fp8 entries: refusals


# sha256 of the files the builders wrote before conv() grew its `out` argument and the module its ConvTranspose writer
BUILDER_BYTES = {
    "densenet121": (lambda: models.densenet121("N"), "1a8fc423addde537a914ab54f6f91db1bb4f43304b1db055206d061006bb8e82"),
    "resnet50": (lambda: models.resnet50("N"), "156ee79e8d0ca121001e26cd10a9679790c4c3c0d3d0f2bc70246b3f4767abd3"),
    "mobilenet_v2": (lambda: models.mobilenet_v2("N"), "d87075c150507554a3101eab10acf0bbc6a39456548eb3d899905abaf183586b"),
    "mobilenet_v3_small": (lambda: models.mobilenet_v3("N", variant="small"), "72db75ad19ebb7b5f342f2df5a0de4e334a54849c39b633a3cbed5af4f95eb1a"),
    "regnet_y_400mf": (lambda: models.regnet_y_400mf("N"), "6ceb3a531c902535431056e3fb8ec1644b5ff61dfb994f39180d406bdae0fd12"),
    "fcn_resnet50_w16": (lambda: models.fcn_resnet50(8, width=16, image=64), "f52dfeb735f8c9fe93334a927b192a0bd11d02d267c42f2ef7db818d6325102f"),
    "deeplabv3_resnet50_w16": (lambda: models.deeplabv3_resnet50(8, width=16, image=64, resize="shape"),
                               "aa8f4d04eee4e98040a49d2712289860846f33a0db52f0581fa8f7cd8ee11f30"),
    "resnet_block": (lambda: models.resnet_block(2), "7a8cdcb09d5c90542ea82674f84def8d7223cc9aa32411f457f6a9498af94fd6"),
    "gemm_mlp": (lambda: models.gemm_mlp(4), "0e0556f824cdd380fbc0a506e15d3be30ac11d73849bce57ab30f2196f65d564"),
}


@pytest.mark.parametrize("name", sorted(BUILDER_BYTES))
def test_existing_builders_keep_their_bytes(name):
    import hashlib
    thunk, want = BUILDER_BYTES[name]
    assert hashlib.sha256(thunk()).hexdigest() == want


if __name__ == "__main__":
    import tempfile
    up, path = (sys.argv[1], sys.argv[2]) if len(sys.argv) > 2 else ("convtranspose", GOLDEN_UNET)
    with tempfile.TemporaryDirectory() as root:
        D.save_golden(_unet_digests(up, root), path)
    print(path)
