"""GPU (-m gpu): depthwise convolutions and Clip on the MI355X against a float64 torch-CPU walk of the same ONNX graph (tests/ref64.py).
Bounds as tests/test_gpu_parity.py: fp32 within 2e-4 of max|ref|, fp16 within 3e-3.
The per-kernel checks (every instantiation forced, each element held to its own bound) are in tests/test_channel_maps_gpu.py."""
import os

import numpy as np
import pytest

import ref64
from engine_run import infer, plan_of, RTOL, run_model, with_env
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models
from gpu_ai_inference_server_amd.modelgen import onnx_pb as pb

pytestmark = pytest.mark.gpu


# ---- seeded random depthwise graphs ------------------------------------------------------------------------------------------------
def _random_case(seed):
    r = np.random.RandomState(seed)
    k = int(r.choice([3, 5, 7], p=[0.4, 0.4, 0.2]))
    s = int(r.choice([1, 2], p=[0.6, 0.4]))
    pad = int(r.choice([0, k // 2], p=[0.3, 0.7]))
    c = int([1, 3, 20, 96, 144][seed % 5])
    h = int(r.choice([7, 9, 13])) + (k if pad == 0 else 0)
    w = int(r.choice([5, 11, 15])) + (k if pad == 0 else 0)
    lo, hi = [(0.0, 6.0), (-0.5, 0.8), (None, 0.7), (-0.3, None)][r.randint(4)]
    return dict(seed=seed, k=k, s=s, pad=pad, c=c, h=h, w=w, pre=bool(r.randint(2)), post_bn=bool(r.randint(2)), clip=bool(r.randint(2)),
                lo=lo, hi=hi, res=bool(r.randint(2)) and s == 1 and pad == k // 2, cat=pad == k // 2 and bool(r.randint(2)),
                slice_in=bool(r.randint(2)))


def _random_graph(cfg):
    """x -> 1x1 conv a1 [-> (concat with 8 more channels: a1 read from a slice)] -> [BN -> ReLU] -> depthwise -> [BN] [+ a1] [-> Clip]
    [-> concat with a side conv: written into a slice] -> y"""
    c, k, s, pad = cfg["c"], cfg["k"], cfg["s"], cfg["pad"]
    gb = models.GraphBuilder("dwrand", 900 + cfg["seed"])
    a1 = gb.conv("x", 4, c, 1, bias=True)
    src = a1
    if cfg["slice_in"]:
        src = gb.concat([gb.conv("x", 4, 8, 1, bias=True), a1])
    u = gb.relu(gb.bn(a1, c)) if cfg["pre"] else a1
    d = gb.conv(u, c, c, k, stride=s, pad=pad, group=c, bias=not cfg["post_bn"])
    if cfg["post_bn"]:
        d = gb.bn(d, c)
    if cfg["res"]:
        d = gb.simple("Add", [d, a1])
    if cfg["clip"]:
        d = gb.clip(d, cfg["lo"], cfg["hi"])
    oh = (cfg["h"] + 2 * pad - k) // s + 1
    ow = (cfg["w"] + 2 * pad - k) // s + 1
    cout = c
    if cfg["cat"]:
        side = gb.conv(src, c + 8 if cfg["slice_in"] else c, 8, 1, stride=s)
        gb.nodes.append(pb.node("Concat", [d, side], ["y"], "cat_out", [pb.attr_int("axis", 1)]))
        cout = c + 8
    else:
        gb.nodes.append(pb.node("Identity", [d], ["y"], "out"))
    return gb.finish([("x", [2, 4, cfg["h"], cfg["w"]])], [("y", [2, cout, oh, ow])]), (2, cout, oh, ow)


CASES = [_random_case(sd) for sd in range(20)]


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("cfg", CASES, ids=[f"k{c['k']}s{c['s']}p{c['pad']}c{c['c']}_{c['seed']}" for c in CASES])
def test_random_depthwise_graphs(tmp_path, cfg, prec):
    mb, oshape = _random_graph(cfg)
    path = models.write_repo(str(tmp_path), "dw", mb)
    x = models.synthetic_input((2, 4, cfg["h"], cfg["w"]), stream=f"dw{cfg['seed']}")
    ref = ref64.run_f64(mb, {"x": x})["y"]
    plan = plan_of(path, 2, dict(IE_PRECISION=prec))
    dws = [st for st in plan["steps"] if st.get("algo") == "depthwise"]
    assert len(dws) == (1 if cfg["c"] > 1 else 0)          # (C = 1: group 1, an ordinary conv)
    fast_ok = bool(dws) and dws[0]["tile"] != 0
    tiles = ["0"] + ([str(1 + cfg["seed"] % 3)] if fast_ok else [])      # the generic kernel, and a channel-vector variant where one applies
    for t in tiles:
        y, kern = run_model(path, "dw", dict(IE_PRECISION=prec, IE_FORCE_TILE=t), {"x": x}, "y", oshape)
        if dws:
            assert any(q.startswith("conv_dw_generic_kernel" if t == "0" else "conv_dw_kernel<") for q in kern), kern
        err = ref64.rel_err(y, ref)
        assert err < RTOL[prec], (cfg, prec, t, err)


# ---- MobileNetV2 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_mini_mobilenet_v2(tmp_path, prec):
    mb = models.mobilenet_v2("N", image=64, classes=50, seed=63)
    path = models.write_repo(str(tmp_path), "mini_mnv2", mb)
    x = models.synthetic_input((3, 3, 64, 64), stream="mini_mnv2")
    ref = ref64.run_f64(mb, {"data": x})["logits"]
    y, kern = run_model(path, "mini_mnv2", dict(IE_PRECISION=prec), {"data": x}, "logits", (3, 50))
    assert sum(q.startswith("conv_dw_kernel<") for q in kern) == 17, kern
    assert ref64.rel_err(y, ref) < RTOL[prec]


@pytest.fixture(scope="module")
def mnv2(tmp_path_factory):
    mb = models.mobilenet_v2("N")
    path = models.write_repo(str(tmp_path_factory.mktemp("mnv2")), "mobilenet_v2", mb)
    m = with_env(dict(IE_AUTOTUNE="0"), lambda: B.CreateModel(path, "mobilenet_v2"))
    yield mb, path, m
    m.Destroy()


def test_full_mobilenet_v2_fp32_vs_float64(mnv2):
    mb, _, m = mnv2
    x = models.synthetic_input((2, 3, 224, 224), stream="mnv2")
    ref = ref64.run_f64(mb, {"data": x})["logits"]
    y = infer(m, {"data": x}, "logits", (2, 1000))
    assert ref64.rel_err(y, ref) < RTOL["fp32"]
    assert (y.argmax(1) == ref.argmax(1)).all()


def test_mobilenet_v2_batch_independence(mnv2):
    _, _, m = mnv2
    x = models.synthetic_input((32, 3, 224, 224), stream="mnv2b")
    y32 = infer(m, {"data": x}, "logits", (32, 1000))
    for i in (0, 13, 31):
        y1 = infer(m, {"data": x[i:i + 1]}, "logits", (1, 1000))
        assert ref64.rel_err(y32[i], y1[0]) < RTOL["fp32"], i


def test_mobilenet_v2_graph_replay_matches_model_infer(mnv2):
    _, _, m = mnv2
    x = models.synthetic_input((4, 3, 224, 224), stream="mnv2r")
    y_host = infer(m, {"data": x}, "logits", (4, 1000))
    din, dout = B.Prepare(m, [[4, 3, 224, 224]], 1)
    B.CopyToDevice(m, din[0], x)
    B.RunPrepared(m, 2, True)
    y = np.empty((4, 1000), np.float32)
    B.CopyToHost(m, y, dout[0])
    np.testing.assert_array_equal(y, y_host)


def test_depthwise_choices_survive_a_restart(tmp_path):
    """The search times the depthwise variants (tune-file codes 700 + tile, 16-number signatures); a second model of the same directory
    finds them in the file, searches nothing (the file is not rewritten) and runs the same kernels."""
    mb = models.mobilenet_v2("N", width_mult=0.5, image=64, classes=10, seed=64)
    path = models.write_repo(str(tmp_path), "tuned_dw", mb, config_json='{"tune_batches": [4]}')
    x = models.synthetic_input((4, 3, 64, 64), stream="tuned_dw")

    def kernels():
        m = B.CreateModel(path, "tuned_dw")
        try:
            din, _ = B.Prepare(m, [[4, 3, 64, 64]], 1)
            B.CopyToDevice(m, din[0], x)
            B.RunPrepared(m, 1, True)
            return [p["kernel"] for p in B.Profile(m, 1)]
        finally:
            m.Destroy()
    first = with_env(dict(IE_AUTOTUNE="1"), kernels)
    caches = [f for f in os.listdir(path) if f.startswith(".ie_tune")]
    assert len(caches) == 1, caches
    cache = os.path.join(path, caches[0])
    stamp = (os.stat(cache).st_mtime_ns, open(cache).read())
    entries = [(k.split(), int(v.split()[0])) for k, v in (ln.split(":") for ln in stamp[1].splitlines()[1:])]
    assert sum(len(k) == 16 and 700 <= code < 704 for k, code in entries) >= 5, entries
    second = with_env(dict(IE_AUTOTUNE="1"), kernels)
    assert (os.stat(cache).st_mtime_ns, open(cache).read()) == stamp
    assert second == first and sum("conv_dw" in q for q in first) == 17


def test_fp8_model_with_depthwise_conv_is_refused(tmp_path):
    path = models.write_repo(str(tmp_path), "mnv2_f8", models.mobilenet_v2("N", width_mult=0.5, image=64, classes=10))
    with pytest.raises(Exception, match="depthwise convolution is not supported in fp8 mode"):
        with_env(dict(IE_PRECISION="fp8", IE_AUTOTUNE="0"), lambda: B.CreateModel(path, "mnv2_f8"))
