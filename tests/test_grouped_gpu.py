"""GPU (-m gpu): grouped convolutions on the MI355X against a float64 torch-CPU walk of the same ONNX graph (tests/ref64.py).
Bounds as tests/test_gpu_parity.py: fp32 within 2e-4 of max|ref|, fp16 within 3e-3.
The per-kernel checks (every instantiation forced, each element held to its own bound) are in tests/test_channel_maps_gpu.py."""
import os

import numpy as np
import pytest

import ref64
from engine_run import infer, RTOL, run_model, with_env
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models
from gpu_ai_inference_server_amd.modelgen import onnx_pb as pb

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def grouped_on(monkeypatch):
    """Grouped convolutions are opt-in (IE_GROUPED_CONV=1)."""
    monkeypatch.setenv("IE_GROUPED_CONV", "1")


# ---- seeded random grouped graphs ------------------------------------------------------------------------------------------------------
CPG = [1, 2, 3, 4, 8, 16, 24, 32, 64]


def _random_case(seed):
    r = np.random.RandomState(seed)
    cpg = CPG[seed % len(CPG)]
    k = int(r.choice([1, 3, 5], p=[0.2, 0.6, 0.2]))
    s = int(r.choice([1, 2], p=[0.6, 0.4]))
    pad = int(r.choice([0, k // 2], p=[0.3, 0.7]))
    groups = int(r.choice([2, 3, 5, 6, 13])) if cpg <= 8 else int(r.choice([2, 3]))
    mult = 2 if cpg == 1 else 1                  # Cin / group = 1: a channel multiplier (Cout = 2 Cin)
    h = int(r.choice([5, 7, 9])) + (k if pad == 0 else 0)
    w = int(r.choice([6, 11, 14])) + (k if pad == 0 else 0)
    return dict(seed=seed, cpg=cpg, k=k, s=s, pad=pad, groups=groups, mult=mult, h=h, w=w, pre=bool(r.randint(2)), post_bn=bool(r.randint(2)),
                res=bool(r.randint(2)) and s == 1 and pad == k // 2 and mult == 1, cat=pad == k // 2 and bool(r.randint(2)),
                slice_in=bool(r.randint(2)))


def _random_graph(cfg):
    """x -> 1x1 conv a1 [-> (concat with 8 more channels: a1 read from a slice)] -> [BN -> ReLU] -> grouped conv -> [BN] [+ a1]
    [-> concat with a side conv: written into a slice] -> y"""
    cin = cfg["cpg"] * cfg["groups"]
    cout = cin * cfg["mult"]
    k, s, pad = cfg["k"], cfg["s"], cfg["pad"]
    gb = models.GraphBuilder("grand", 1300 + cfg["seed"])
    a1 = gb.conv("x", 4, cin, 1, bias=True)
    src = a1
    if cfg["slice_in"]:
        src = gb.concat([gb.conv("x", 4, 8, 1, bias=True), a1])
    u = gb.relu(gb.bn(a1, cin)) if cfg["pre"] else a1
    d = gb.conv(u, cin, cout, k, stride=s, pad=pad, group=cfg["groups"], bias=not cfg["post_bn"])
    if cfg["post_bn"]:
        d = gb.bn(d, cout)
    if cfg["res"]:
        d = gb.simple("Add", [d, a1])
    oh = (cfg["h"] + 2 * pad - k) // s + 1
    ow = (cfg["w"] + 2 * pad - k) // s + 1
    ctot = cout
    if cfg["cat"]:
        side = gb.conv(src, cin + 8 if cfg["slice_in"] else cin, 8, 1, stride=s)
        gb.nodes.append(pb.node("Concat", [d, side], ["y"], "cat_out", [pb.attr_int("axis", 1)]))
        ctot = cout + 8
    else:
        gb.nodes.append(pb.node("Identity", [d], ["y"], "out"))
    return gb.finish([("x", [2, 4, cfg["h"], cfg["w"]])], [("y", [2, ctot, oh, ow])]), (2, ctot, oh, ow)


CASES = [_random_case(sd) for sd in range(27)]


def _eligible_tiles(path, prec):
    """IE_FORCE_TILE values the planner keeps for the graph's grouped step (it falls back to its default for a tile the views do not admit)."""
    out = []
    for t in range(4):
        plan = with_env(dict(IE_PRECISION=prec, IE_FORCE_TILE=str(t)), lambda: B.DescribeModel(path, 2)["plan"])
        (g,) = [st for st in plan["steps"] if st.get("algo") == "grouped"]
        if g["tile"] == t:
            out.append(t)
    return out


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("cfg", CASES, ids=[f"cpg{c['cpg']}g{c['groups']}k{c['k']}s{c['s']}p{c['pad']}_{c['seed']}" for c in CASES])
def test_random_grouped_graphs(tmp_path, cfg, prec):
    mb, oshape = _random_graph(cfg)
    path = models.write_repo(str(tmp_path), "grp", mb)
    x = models.synthetic_input((2, 4, cfg["h"], cfg["w"]), stream=f"grp{cfg['seed']}")
    ref = ref64.run_f64(mb, {"x": x})["y"]
    tiles = _eligible_tiles(path, prec)
    assert 0 in tiles
    for t in tiles:
        y, kern = run_model(path, "grp", dict(IE_PRECISION=prec, IE_FORCE_TILE=str(t)), {"x": x}, "y", oshape)
        want = "conv_grouped_generic_kernel" if t == 0 else "conv_grouped_kernel<"
        assert any(q.startswith(want) for q in kern) and (t == 0 or f"px{[0, 1, 2, 4][t]}>" in " ".join(kern)), (t, kern)
        err = ref64.rel_err(y, ref)
        assert err < RTOL[prec], (cfg, prec, t, err)


# ---- the stock networks at batch 2 --------------------------------------------------------------------------------------------------------
NETS = {"resnext50": models.resnext50_32x4d, "regnet_y": models.regnet_y_400mf}


@pytest.fixture(scope="module")
def nets(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("gnets"))
    out = {}
    for name, f in NETS.items():
        mb = f("N")
        x = models.synthetic_input((2, 3, 224, 224), stream=name)
        out[name] = (mb, models.write_repo(root, name, mb), x, ref64.run_f64(mb, {"data": x})["logits"])
    return out


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("name", list(NETS))
def test_networks_vs_float64(nets, name, prec):
    _, path, x, ref = nets[name]
    y, kern = run_model(path, name, dict(IE_PRECISION=prec), {"data": x}, "logits", (2, 1000))
    assert ref64.rel_err(y, ref) < RTOL[prec]
    assert (y.argmax(1) == ref.argmax(1)).all()
    grouped = [q for q in kern if q.startswith("conv_grouped")]
    assert len(grouped) == 16 and not any("generic" in q for q in grouped), kern


def test_resnext50_searched_set_fp32_b32(tmp_path):
    """One load with the search on (IE_AUTOTUNE=1) at batch 32: the chosen kernels are checked against float64 like the defaults."""
    mb = models.resnext50_32x4d("N")
    path = models.write_repo(str(tmp_path), "rx_tuned", mb, config_json='{"tune_batches": [32]}')
    x = models.synthetic_input((32, 3, 224, 224), stream="rx_tuned")
    ref = ref64.run_f64(mb, {"data": x[:4]})["logits"]

    def go():
        m = B.CreateModel(path, "rx_tuned")
        try:
            y = infer(m, {"data": x}, "logits", (32, 1000))
            return y, [p["kernel"] for p in B.Profile(m, 1)]
        finally:
            m.Destroy()
    y, kern = with_env(dict(IE_AUTOTUNE="1"), go)
    assert ref64.rel_err(y[:4], ref) < RTOL["fp32"]
    assert (y[:4].argmax(1) == ref.argmax(1)).all()
    assert sum(q.startswith("conv_grouped") for q in kern) == 16


# ---- determinism, replay, batch independence, tune file -----------------------------------------------------------------------------------
def _mini_resnext():
    return models.resnext50_32x4d("N", layers=(1, 1, 1, 1), image=64, classes=20, seed=51)


@pytest.mark.parametrize("tile", ["1", "2"])
def test_replay_reruns_and_batch_independence(tmp_path, tile):
    mb = _mini_resnext()
    path = models.write_repo(str(tmp_path), "mrx", mb)
    x = models.synthetic_input((4, 3, 64, 64), stream="mrx")

    def go():
        m = B.CreateModel(path, "mrx")
        try:
            y_host = infer(m, {"data": x}, "logits", (4, 20))
            again = infer(m, {"data": x}, "logits", (4, 20))
            np.testing.assert_array_equal(y_host, again)                           # reruns are bit-identical
            din, dout = B.Prepare(m, [[4, 3, 64, 64]], 1)
            B.CopyToDevice(m, din[0], x)
            B.RunPrepared(m, 2, True)                                              # graph replay
            y = np.empty((4, 20), np.float32)
            B.CopyToHost(m, y, dout[0])
            np.testing.assert_array_equal(y, y_host)
            for i in (0, 3):
                y1 = infer(m, {"data": x[i:i + 1]}, "logits", (1, 20))
                assert ref64.rel_err(y_host[i], y1[0]) < RTOL["fp32"], i
            return [p["kernel"] for p in B.Profile(m, 1)]
        finally:
            m.Destroy()
    kern = with_env(dict(IE_AUTOTUNE="0", IE_FORCE_TILE=tile), go)
    assert sum(q.startswith("conv_grouped_kernel<") and q.endswith(f"px{[0, 1, 2, 4][int(tile)]}>") for q in kern) == 4, kern


def test_grouped_choices_survive_a_restart(tmp_path):
    """The search times the grouped variants (tune-file codes 800 + tile, 18-number signatures); a second model of the same directory finds
    them in the file, searches nothing (the file is not rewritten) and runs the same kernels."""
    mb = _mini_resnext()
    path = models.write_repo(str(tmp_path), "tuned_grp", mb, config_json='{"tune_batches": [4]}')
    x = models.synthetic_input((4, 3, 64, 64), stream="tuned_grp")

    def kernels():
        m = B.CreateModel(path, "tuned_grp")
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
    assert sum(len(k) == 18 and 800 <= code < 804 for k, code in entries) >= 4, entries        # 4 grouped convs per tuned batch size
    second = with_env(dict(IE_AUTOTUNE="1"), kernels)
    assert (os.stat(cache).st_mtime_ns, open(cache).read()) == stamp
    assert second == first and sum(q.startswith("conv_grouped") for q in first) == 4


def test_fp8_model_with_grouped_conv_is_refused(tmp_path):
    path = models.write_repo(str(tmp_path), "rx_f8", _mini_resnext())
    with pytest.raises(Exception, match="grouped convolution is not supported in fp8 mode"):
        with_env(dict(IE_PRECISION="fp8", IE_AUTOTUNE="0"), lambda: B.CreateModel(path, "rx_f8"))
