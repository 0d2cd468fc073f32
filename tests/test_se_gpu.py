"""GPU (-m gpu): squeeze-excite blocks and the MobileNetV3 / EfficientNet activations on the MI355X against a float64 torch-CPU walk of the same
ONNX graph (tests/ref64.py), the fused SE step against its IE_NO_SE_FUSE=1 form.  Bounds as tests/test_depthwise_gpu.py: fp32 within 2e-4 of
max|ref|, fp16 within 3e-3."""

import numpy as np
import pytest

import ref64
from engine_run import infer, plan_of, RTOL, run_model, with_env
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models
from gpu_ai_inference_server_amd.modelgen import onnx_pb as pb

pytestmark = pytest.mark.gpu
SE_KERNELS = "se_squeeze_kernel + se_fc1_kernel + se_fc2_kernel + se_apply_kernel"


# ---- seeded random SE / activation graphs ---------------------------------------------------------------------------------------------
ACTS = ["none", "hardswish", "silu", "sigmoid", "hardsigmoid"]


def _random_case(seed):
    r = np.random.RandomState(seed)
    k = int(r.choice([3, 5]))
    s = int(r.choice([1, 2], p=[0.6, 0.4]))
    hw = [1, 3, 7, 14, 28, 56][seed % 6]
    return dict(seed=seed, k=k, s=s, c=[8, 20, 36, 96, 144][seed % 5], mid=[1, 5, 6, 10, 28][(seed // 2) % 5], h=hw, w=hw + (seed % 3 == 1),
                pre=ACTS[seed % 5], post=ACTS[(seed // 5 + seed) % 5], act1=["relu", "silu", "hardswish", "sigmoid"][seed % 4],
                gate=["sigmoid", "hardsigmoid"][(seed // 3) % 2], form=["op", "hardsigmoid_mul", "mul_hardsigmoid"][seed % 3], swap=bool(seed % 2))


def _random_graph(cfg):
    """x -> 1x1 conv [-> BN] -> pre act -> depthwise k x k (stride s) -> BN -> post act -> SE(C, mid, act1, gate) -> 1x1 conv -> y"""
    c, k, s = cfg["c"], cfg["k"], cfg["s"]
    gb = models.GraphBuilder("serand", 700 + cfg["seed"])
    a = gb.act(gb.bn(gb.conv("x", 4, c, 1, bias=True), c), cfg["pre"], cfg["form"])
    d = gb.act(gb.bn(gb.conv(a, c, c, k, stride=s, pad=k // 2, group=c), c), cfg["post"], cfg["form"])
    y = gb.se(d, c, cfg["mid"], cfg["act1"], cfg["gate"], swap=cfg["swap"], form=cfg["form"])
    gb.nodes.append(pb.node("Conv", [y, gb.init("proj_w", (np.random.RandomState(cfg["seed"]).randn(8, c, 1, 1) / np.sqrt(c)).astype(np.float32))],
                            ["y"], "proj", [pb.attr_ints("kernel_shape", [1, 1])]))
    oh = (cfg["h"] + 2 * (k // 2) - k) // s + 1
    ow = (cfg["w"] + 2 * (k // 2) - k) // s + 1
    return gb.finish([("x", [2, 4, cfg["h"], cfg["w"]])], [("y", [2, 8, oh, ow])], opset=14), (2, 8, oh, ow)


CASES = [_random_case(sd) for sd in range(12)]


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("cfg", CASES, ids=[f"c{c['c']}r{c['mid']}hw{c['h']}k{c['k']}s{c['s']}_{c['seed']}" for c in CASES])
def test_random_se_graphs(tmp_path, cfg, prec):
    mb, oshape = _random_graph(cfg)
    path = models.write_repo(str(tmp_path), "se", mb)
    x = models.synthetic_input((2, 4, cfg["h"], cfg["w"]), stream=f"se{cfg['seed']}")
    ref = ref64.run_f64(mb, {"x": x})["y"]
    plan = plan_of(path, 2, dict(IE_PRECISION=prec))
    fused = any(st["kind"] == "squeeze_excite" for st in plan["steps"])
    oh, ow = oshape[2:]
    assert fused == (oh * ow > 1)                 # (a 1x1 map: the gate Mul has two [N,C,1,1] operands, an eltwise step)
    dws = [st for st in plan["steps"] if st.get("algo") == "depthwise"]
    tiles = ["0"] + (["1", "2", "3"] if dws and dws[0]["tile"] != 0 else [])
    outs = {}
    for t in tiles:
        y, kern = run_model(path, "se", dict(IE_PRECISION=prec, IE_FORCE_TILE=t), {"x": x}, "y", oshape)
        assert (SE_KERNELS in " ".join(kern)) == fused, kern
        err = ref64.rel_err(y, ref)
        assert err < RTOL[prec], (cfg, prec, t, err)
        outs[t] = y
    y_unf, kern = run_model(path, "se", dict(IE_PRECISION=prec, IE_NO_SE_FUSE="1"), {"x": x}, "y", oshape)
    assert not any(SE_KERNELS in q for q in kern)
    assert ref64.rel_err(y_unf, ref) < RTOL[prec], (cfg, prec, "unfused")
    assert ref64.rel_err(outs["0"], y_unf) < RTOL[prec]


# ---- the networks -----------------------------------------------------------------------------------------------------------------------
NETS = {
    "mnv3_large": lambda **kw: models.mobilenet_v3("N", variant="large", **kw),
    "mnv3_small": lambda **kw: models.mobilenet_v3("N", variant="small", **kw),
    "effnet_b0": lambda **kw: models.efficientnet_b0("N", **kw),
}


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("name", list(NETS))
def test_mini_networks(tmp_path, name, prec):
    mb = NETS[name](width_mult=0.5, image=64, classes=50, seed=91)
    path = models.write_repo(str(tmp_path), "mini_" + name, mb)
    x = models.synthetic_input((2, 3, 64, 64), stream="mini_" + name)
    ref = ref64.run_f64(mb, {"data": x})["logits"]
    y, kern = run_model(path, "mini_" + name, dict(IE_PRECISION=prec), {"data": x}, "logits", (2, 50))
    assert sum(SE_KERNELS in q for q in kern) == {"mnv3_large": 8, "mnv3_small": 9, "effnet_b0": 16}[name], kern
    assert ref64.rel_err(y, ref) < RTOL[prec]


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("name", list(NETS))
def test_full_networks_vs_float64(tmp_path, name, prec):
    mb = NETS[name]()
    path = models.write_repo(str(tmp_path), name, mb)
    x = models.synthetic_input((2, 3, 224, 224), stream=name)
    ref = ref64.run_f64(mb, {"data": x})["logits"]
    y, kern = run_model(path, name, dict(IE_PRECISION=prec), {"data": x}, "logits", (2, 1000))
    # fused activations launch nothing of their own: the only eltwise launches are the classifier's hardswish (and MobileNetV3-Large's stem
    # activation, read by a depthwise conv and an identity Add)
    assert sum(q == "eltwise_kernel" for q in kern) == {"mnv3_large": 2, "mnv3_small": 1, "effnet_b0": 0}[name], kern
    assert ref64.rel_err(y, ref) < RTOL[prec]
    if prec == "fp32":
        assert (y.argmax(1) == ref.argmax(1)).all()


@pytest.fixture(scope="module")
def effnet(tmp_path_factory):
    mb = models.efficientnet_b0("N", width_mult=0.5, image=96, classes=100, seed=92)
    path = models.write_repo(str(tmp_path_factory.mktemp("effnet")), "effnet", mb)
    m = with_env(dict(IE_AUTOTUNE="0"), lambda: B.CreateModel(path, "effnet"))
    yield mb, path, m
    m.Destroy()


def test_batch_independence(effnet):
    """Image i of a batch of 8 against the same image alone: a per-(n, c) indexing slip in the gate shows here."""
    _, _, m = effnet
    x = models.synthetic_input((8, 3, 96, 96), stream="effb")
    y8 = infer(m, {"data": x}, "logits", (8, 100))
    for i in (0, 3, 7):
        y1 = infer(m, {"data": x[i:i + 1]}, "logits", (1, 100))
        assert ref64.rel_err(y8[i], y1[0]) < RTOL["fp32"], i


def test_graph_replay_matches_model_infer_and_runs_are_bit_identical(effnet):
    _, _, m = effnet
    x = models.synthetic_input((4, 3, 96, 96), stream="effr")
    y_host = infer(m, {"data": x}, "logits", (4, 100))
    np.testing.assert_array_equal(infer(m, {"data": x}, "logits", (4, 100)), y_host)      # no atomics: two runs agree bit for bit
    din, dout = B.Prepare(m, [[4, 3, 96, 96]], 1)
    B.CopyToDevice(m, din[0], x)
    B.RunPrepared(m, 2, True)
    y = np.empty((4, 100), np.float32)
    B.CopyToHost(m, y, dout[0])
    np.testing.assert_array_equal(y, y_host)


def test_mobilenet_v3_large_fp16_batch_independence(tmp_path):
    mb = models.mobilenet_v3("N", variant="large", width_mult=0.75, image=96, classes=40, seed=93, act_form="hardsigmoid_mul")
    path = models.write_repo(str(tmp_path), "mnv3", mb)
    x = models.synthetic_input((8, 3, 96, 96), stream="mnv3b")

    def go():
        m = B.CreateModel(path, "mnv3")
        try:
            y8 = infer(m, {"data": x}, "logits", (8, 40))
            return y8, [infer(m, {"data": x[i:i + 1]}, "logits", (1, 40))[0] for i in (1, 6)]
        finally:
            m.Destroy()
    y8, singles = with_env(dict(IE_AUTOTUNE="0", IE_PRECISION="fp16"), go)
    for i, y1 in zip((1, 6), singles):
        assert ref64.rel_err(y8[i], y1) < RTOL["fp16"], i
    ref = ref64.run_f64(mb, {"data": x})["logits"]
    assert ref64.rel_err(y8, ref) < RTOL["fp16"]
