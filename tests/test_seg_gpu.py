"""GPU (-m gpu): dilated convolutions and Resize on the MI355X against a float64 torch-CPU walk of the same ONNX graph (tests/ref64.py).
Bounds as tests/test_gpu_parity.py: fp32 within 2e-4 of max|ref|, fp16 within 3e-3."""

import numpy as np
import pytest

import ref64
from engine_run import infer, plan_of, RTOL, run_model, with_env
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models
from gpu_ai_inference_server_amd.modelgen import onnx_pb as pb

pytestmark = pytest.mark.gpu


# ---- seeded random dilated convs ---------------------------------------------------------------------------------------------------------
DILS = [1, 2, 3, 4, 5, 6, 12]


def _dil_case(seed):
    r = np.random.RandomState(seed)
    d = DILS[seed % len(DILS)]
    k = int(r.choice([3, 5]))
    s = int(r.choice([1, 2]))
    pads = [int(v) for v in r.randint(0, d * (k // 2) + 2, size=4)]
    cin = int(r.choice([8, 16, 24, 12, 6]))            # multiples of 4 (vector staging) and not
    h = int(r.choice([9, 14, 17])) + (k - 1) * d
    w = int(r.choice([8, 13, 16])) + (k - 1) * d
    res = bool(r.randint(2))
    if res:                                            # a residual epilogue needs the output grid of the input: stride 1, "same" pads
        s, pads = 1, [d * (k // 2)] * 4
    return dict(seed=seed, d=d, k=k, s=s, pads=pads, cin=cin, cout=int(r.choice([16, 32, 40])), h=h, w=w, pre=bool(r.randint(2)),
                res=res, cat_in=bool(r.randint(2)), cat_out=bool(r.randint(2)), tile=int(r.randint(7)),
                splitk=int(r.choice([1, 2, 4])))


def _dil_graph(cfg):
    """x -> 1x1 a1 [-> concat (a1 read from a slice)] -> [BN -> ReLU] -> dilated conv -> BN [+ 1x1 of x, the residual] [-> concat with a side
    conv: written into a slice] -> y"""
    gb = models.GraphBuilder("dil", 1500 + cfg["seed"])
    cin, cout, k, s, d, p = cfg["cin"], cfg["cout"], cfg["k"], cfg["s"], cfg["d"], cfg["pads"]
    a1 = gb.conv("x", 4, cin, 1, bias=True)
    if cfg["cat_in"]:
        gb.concat([gb.conv("x", 4, 8, 1, bias=True), a1])
    u = gb.relu(gb.bn(a1, cin)) if cfg["pre"] else a1
    y = gb.bn(gb.conv(u, cin, cout, k, stride=s, pad=p, dilation=d, name="dconv"), cout)
    oh = (cfg["h"] + p[0] + p[2] - (k - 1) * d - 1) // s + 1
    ow = (cfg["w"] + p[1] + p[3] - (k - 1) * d - 1) // s + 1
    if cfg["res"] and (oh, ow) == (cfg["h"], cfg["w"]):
        y = gb.simple("Add", [y, gb.conv("x", 4, cout, 1, bias=True)])
    ctot = cout
    if cfg["cat_out"]:
        side = gb.conv(u, cin, 8, k, stride=s, pad=p, dilation=d, bias=True)
        y = gb.concat([side, y])
        ctot += 8
    gb.nodes.append(pb.node("Identity", [gb.relu(y)], ["y"], "out"))
    return gb.finish([("x", [2, 4, cfg["h"], cfg["w"]])], [("y", [2, ctot, oh, ow])]), (2, ctot, oh, ow)


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("seed", range(14))
def test_random_dilated_convs(tmp_path, seed, prec):
    cfg = _dil_case(seed)
    mb, oshape = _dil_graph(cfg)
    path = models.write_repo(str(tmp_path), "dil", mb)
    x = models.synthetic_input((2, 4, cfg["h"], cfg["w"]), stream=f"dil{seed}")
    ref = ref64.run_f64(mb, {"x": x})["y"]
    for env in (dict(), dict(IE_FORCE_ALGO="igemm", IE_FORCE_TILE=str(cfg["tile"]), IE_FORCE_SPLITK=str(cfg["splitk"])), dict(IE_FORCE_ALGO="naive")):
        plan = plan_of(path, 2, dict(IE_PRECISION=prec, **env))
        dsteps = [s for s in plan["steps"] if s["name"].startswith("dconv") or "dconv" in s["name"]]
        assert dsteps and all(s["algo"] in ("igemm_vec", "igemm_scalar", "naive") for s in plan["steps"] if "dilations" in s)
        y, _ = run_model(path, "dil", dict(IE_PRECISION=prec, **env), {"x": x}, "y", oshape)
        assert ref64.rel_err(y, ref) < RTOL[prec], (cfg, env)


# ---- seeded random Resize cases ----------------------------------------------------------------------------------------------------------
def _resize_case(seed):
    r = np.random.RandomState(seed)
    mode = ["nearest", "linear"][seed % 2]
    coord = ref64.COORDS[(seed // 2) % 4]
    nearest = ref64.NEAREST[(seed // 8) % 4]
    h, w = int(r.choice([1, 5, 7, 12])), int(r.choice([1, 6, 9, 14]))
    form = ["scales", "sizes"][(seed // 3) % 2]
    c = int(r.choice([8, 16, 21, 24]))
    if form == "scales":
        sc = [float(np.float32(r.choice([0.5, 1.5, 2.0, 2.5, 3.0, 0.75]))) for _ in range(2)]
        out = [int(np.floor(h * sc[0])), int(np.floor(w * sc[1]))]
        if min(out) < 1:
            sc, out = [2.0, 2.0], [2 * h, 2 * w]
    else:
        out = [int(r.choice([3, 8, 13, 20, 28])), int(r.choice([4, 9, 17, 28]))]
        sc = None
    return dict(seed=seed, mode=mode, coord=coord, nearest=nearest, h=h, w=w, c=c, form=form, sc=sc, out=out, where=["out", "cat", "nchw"][seed % 3])


def _resize_graph(cfg):
    """x -> 1x1 conv (c channels, NHWC) -> Resize -> {a 1x1 conv reading it ("out"), a concat slice ("cat"), the NCHW graph output ("nchw")}"""
    gb = models.GraphBuilder("rz", 1700 + cfg["seed"])
    a = gb.conv("x", 4, cfg["c"], 1, bias=True)
    kw = dict(mode=cfg["mode"], coord=cfg["coord"], nearest=cfg["nearest"] if cfg["mode"] == "nearest" else None, name="rz",
              out="y" if cfg["where"] == "nchw" else None)
    if cfg["form"] == "scales":
        r = gb.resize(a, (2, cfg["c"], cfg["h"], cfg["w"]), scales=cfg["sc"], form="scales", **kw)
    else:
        r = gb.resize(a, (2, cfg["c"], cfg["h"], cfg["w"]), sizes=cfg["out"], form="sizes", **kw)
    oh, ow = cfg["out"]
    if cfg["where"] == "nchw":
        return gb.finish([("x", [2, 4, cfg["h"], cfg["w"]])], [("y", [2, cfg["c"], oh, ow])], opset=13), (2, cfg["c"], oh, ow)
    if cfg["where"] == "cat":
        side = gb.resize(gb.conv("x", 4, 8, 1, bias=True), (2, 8, cfg["h"], cfg["w"]), sizes=cfg["out"], form="sizes", mode="nearest", name="rz_side")
        y = gb.concat([side, r])
        c = cfg["c"] + 8
    else:
        y, c = r, cfg["c"]
    gb.nodes.append(pb.node("Conv", [y, gb.init("ow", np.eye(c, dtype=np.float32).reshape(c, c, 1, 1))], ["y"], "post"))
    return gb.finish([("x", [2, 4, cfg["h"], cfg["w"]])], [("y", [2, c, oh, ow])], opset=13), (2, c, oh, ow)


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("seed", range(32))
def test_random_resize(tmp_path, seed, prec):
    cfg = _resize_case(seed)
    mb, oshape = _resize_graph(cfg)
    path = models.write_repo(str(tmp_path), "rz", mb)
    x = models.synthetic_input((2, 4, cfg["h"], cfg["w"]), stream=f"rz{seed}")
    ref = ref64.run_f64(mb, {"x": x})["y"]
    y, kern = run_model(path, "rz", dict(IE_PRECISION=prec), {"x": x}, "y", oshape)
    assert ref64.rel_err(y, ref) < RTOL[prec], cfg
    assert any(q.startswith("resize_") for q in kern), kern


def test_resize_graph_output_is_written_by_the_resize(tmp_path):
    cfg = dict(seed=0, mode="linear", coord="pytorch_half_pixel", nearest=None, h=7, w=7, c=21, form="sizes", sc=None, out=[56, 56], where="nchw")
    mb, oshape = _resize_graph(cfg)
    path = models.write_repo(str(tmp_path), "rzo", mb)
    x = models.synthetic_input((2, 4, 7, 7), stream="rzo")
    y, kern = run_model(path, "rzo", dict(IE_PRECISION="fp16"), {"x": x}, "y", oshape)
    assert ref64.rel_err(y, ref64.run_f64(mb, {"x": x})["y"]) < RTOL["fp16"]
    assert "resize_nchw_kernel<f16>" in kern and "copy_kernel" not in kern, kern


# ---- whole networks ------------------------------------------------------------------------------------------------------------------------
NETS = {"fcn": models.fcn_resnet50, "deeplab": models.deeplabv3_resnet50}


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("net", ["fcn", "deeplab"])
def test_network_vs_float64(tmp_path, net, prec):
    mb = NETS[net](2, width=16, image=96, resize="shape")
    path = models.write_repo(str(tmp_path), net, mb)
    x = models.synthetic_input((2, 3, 96, 96), stream=net)
    ref = ref64.run_f64(mb, {"image": x})["out"]
    y, kern = run_model(path, net, dict(IE_PRECISION=prec), {"image": x}, "out", (2, 21, 96, 96))
    assert ref64.rel_err(y, ref) < RTOL[prec]
    assert (y.argmax(1) == ref.argmax(1)).mean() > (0.999 if prec == "fp32" else 0.99)      # (fp16: near-ties among 21 classes)
    assert "copy_kernel" not in kern and sum(q.startswith("resize_") for q in kern) == (1 if net == "fcn" else 2), kern


@pytest.mark.parametrize("net", ["fcn", "deeplab"])
def test_network_at_224(tmp_path, net):
    """The full-width nets at 224 x 224 (the rate-36 branch collapses at 28 x 28), fp32 batch 1 against float64"""
    mb = NETS[net](1)
    path = models.write_repo(str(tmp_path), net, mb)
    x = models.synthetic_input((1, 3, 224, 224), stream=net + "224")
    ref = ref64.run_f64(mb, {"image": x})["out"]
    y, _ = run_model(path, net, dict(IE_PRECISION="fp32"), {"image": x}, "out", (1, 21, 224, 224))
    assert ref64.rel_err(y, ref) < RTOL["fp32"]


def test_replay_and_batch_independence(tmp_path):
    mb = models.deeplabv3_resnet50("N", width=8, image=64, resize="scales")
    path = models.write_repo(str(tmp_path), "dlr", mb)
    x = models.synthetic_input((2, 3, 64, 64), stream="dlr")

    def go():
        m = B.CreateModel(path, "dlr")
        try:
            y_host = infer(m, {"image": x}, "out", (2, 21, 64, 64))
            din, dout = B.Prepare(m, [[2, 3, 64, 64]], 1)
            B.CopyToDevice(m, din[0], x)
            B.RunPrepared(m, 2, True)                                              # graph replay
            y = np.empty((2, 21, 64, 64), np.float32)
            B.CopyToHost(m, y, dout[0])
            np.testing.assert_array_equal(y, y_host)
            y1 = infer(m, {"image": x[:1]}, "out", (1, 21, 64, 64))
            assert ref64.rel_err(y_host[0], y1[0]) < RTOL["fp32"]
        finally:
            m.Destroy()
    with_env(dict(IE_AUTOTUNE="0"), go)


def test_fp8_load_is_refused(tmp_path):
    path = models.write_repo(str(tmp_path), "dl8", models.deeplabv3_resnet50("N", width=8, image=64, resize="scales"))
    with pytest.raises(Exception, match="dilated convolution is not supported in fp8 mode"):
        with_env(dict(IE_PRECISION="fp8", IE_AUTOTUNE="0"), lambda: B.CreateModel(path, "dl8"))
