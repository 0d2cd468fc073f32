"""GPU (-m gpu): the launches of the executor pinned by label.  For every entry of a graph x precision x forcing-switch matrix,
tests/golden/launch_labels.json holds the (step name, kernel label) list that B.Profile reports under IE_AUTOTUNE=0 (engine_run.run_model), or --
where the engine refuses the combination -- the refusal's text.  The forced values are chosen so that many specialised launchers decline at these
shapes (IE_NO_FRAG_WEIGHTS=1 takes the fp32 weight mirrors away under an unchanged plan, so the fused dense layers, the direct family and Winograd all
decline): what is recorded is then the hand-over of DeviceModel::LaunchedStep, beside entries where the specialised kernel runs.  An executor change
that is meant to preserve behaviour must leave the file alone; one that is meant to change a launch regenerates it and shows the moved keys:

    python tests/test_launch_labels_gpu.py            # rewrites tests/golden/launch_labels.json from the built library (on the GPU)

Every entry also holds its output to the float64 walk of tests/ref64.py within engine_run.RTOL (fp8: test_gpu_parity.py's F8_RTOL_MINI, the bound
of the 16-channel mini ResNets), so a label that stays while the launch goes wrong is still caught."""
import functools
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    from _pkg import load_package
    load_package()

import attn_wide_graphs  # noqa: E402
import bert_graphs  # noqa: E402
import convt_graphs  # noqa: E402
import gn_graphs  # noqa: E402
import kernel_graphs  # noqa: E402
import ref64  # noqa: E402
import swin_graphs  # noqa: E402
import vit_graphs  # noqa: E402
from conftest import MINI  # noqa: E402
from engine_run import RTOL, run_model  # noqa: E402
from gpu_ai_inference_server_amd.modelgen import models  # noqa: E402
from oracle import onnx_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden", "launch_labels.json")
BOUND = dict(RTOL, fp8=0.12)             # fp8: test_gpu_parity.py F8_RTOL_MINI
ALGOS = ("igemm", "raster", "ws", "direct", "wino", "x6", "naive")
TILES = ("0", "1", "3", "9", "12", "15", "102", "203")
FORCED = [{"IE_FORCE_ALGO": a} for a in ALGOS] + [{"IE_FORCE_TILE": t} for t in TILES]
FEW = [{"IE_FORCE_ALGO": a} for a in ("ws", "direct", "naive")] + [{"IE_FORCE_TILE": t} for t in ("0", "1", "3")]
TILES_013 = [{"IE_FORCE_TILE": t} for t in ("0", "1", "3")]
ATTN = [{"IE_ATTN_TILE": t} for t in ("0", "1", "2")]


def _dw_graph():
    """a MobileNet block: 1x1 expand -> ReLU6 -> depthwise 3x3 -> ReLU6 -> 1x1 project, plus the input (stride 1)"""
    gb = models.GraphBuilder("dwblock", 41)
    a = gb.clip(gb.conv("x", 8, 48, 1, bias=True))
    d = gb.clip(gb.conv(a, 48, 48, 3, pad=1, group=48, bias=True))
    gb.simple("Add", [gb.conv(d, 48, 8, 1, bias=True), "x"], out="y")
    return gb.finish([("x", [2, 8, 9, 11])], [("y", [2, 8, 9, 11])])


def _grouped_graph():
    """a ResNeXt block's middle: 1x1 -> ReLU -> grouped 3x3 (4 groups of 8) -> ReLU -> 1x1"""
    gb = models.GraphBuilder("grpblock", 43)
    a = gb.relu(gb.conv("x", 8, 32, 1, bias=True))
    d = gb.relu(gb.conv(a, 32, 32, 3, pad=1, group=4, bias=True))
    gb.conv(d, 32, 8, 1, bias=True, out="y")
    return gb.finish([("x", [2, 8, 9, 11])], [("y", [2, 8, 9, 11])])


def _resize_graph():
    """1x1 conv -> bilinear Resize 7x9 -> 14x18 -> 1x1 conv"""
    gb = models.GraphBuilder("rzblock", 47)
    r = gb.resize(gb.conv("x", 4, 16, 1, bias=True), (2, 16, 7, 9), sizes=[14, 18], form="sizes", name="rz")
    gb.conv(r, 16, 8, 1, bias=True, out="y")
    return gb.finish([("x", [2, 4, 7, 9])], [("y", [2, 8, 14, 18])], opset=13)


def _mini(name):
    mk, iname, ishape = MINI[name]
    return lambda: (mk(models), {iname: models.synthetic_input(ishape, stream=name)})


def _attn(n, l, h, hd):
    return lambda: (vit_graphs.attn_graph(n, l, h, hd), {"x": np.array(vit_graphs.make_input(n, l, h, hd, "randn"))})


def _wattn():
    hw, heads, hd = (14, 14), 2, 32
    x = np.array(vit_graphs.make_input(2, hw[0] * hw[1], heads, hd, "randn")).reshape(2, 3 * heads * hd, *hw)
    return swin_graphs.wattn_graph(2, hw, (7, 7), (3, 3), heads, hd), {"x": x}


def _convt(seed):
    def go():
        mb, ishape, _ = convt_graphs.random_graph(convt_graphs.random_case(seed))
        return mb, {"x": models.synthetic_input(ishape, stream="convt%d" % seed)}
    return go


def _resnet_f8():
    """test_gpu_parity.py's shallow bottleneck ResNet, the smallest graph the fp8 planner takes (7x7 stem; at width 16 no shortcut becomes a dual 1x1)"""
    return models.resnet(3, layers=(2, 1), width=16, image=64, classes=20, seed=51), {"data": models.synthetic_input((3, 3, 64, 64), stream="resnet_f8")}


def _dense(seed, n, h, w, c0, layers, tail):
    """kernel_graphs.dense_case: the smallest graph the dense-fusion (fp32) and dense-block (fp16) patterns of the planner accept; the run's output is its concat buffer"""
    def go():
        d = kernel_graphs.dense_case(seed, n, h, w, c0, layers, tail=tail, expose=False)
        return d["model"], {"x": d["x"]}
    return go


def _resnet_dual_f8():
    """test_gpu_parity.py's bottleneck ResNet of width 32: its projection shortcuts become dual 1x1 steps in fp8"""
    return models.resnet(2, layers=(2, 2), width=32, image=64, classes=20, seed=53), {"data": models.synthetic_input((2, 3, 64, 64), stream="tuned8")}


def _gn():
    return gn_graphs.gn_graph(2, 32, 8, 8, 8, act="silu"), {"x": gn_graphs.data("randn", 2, 32, 8, 8, 8).astype(np.float32)}


# name -> (thunk -> (model bytes, feeds), precisions, switch sets beyond the plain run, environment of every run)
GRAPHS = {
    "mini_densenet": (_mini("mini_densenet"), ("fp32", "fp16"), FORCED + [{"IE_NO_FRAG_WEIGHTS": "1"}, {"IE_NO_FRAG_WEIGHTS": "1", "IE_FORCE_ALGO": "wino"}], {}),
    "mini_densenet_scale": (_mini("mini_densenet_scale"), ("fp32", "fp16"), FEW, {}),
    "mini_resnet_block": (_mini("mini_resnet_block"), ("fp32", "fp16"), FORCED, {}),
    "mini_resnet_block_f8": (_mini("mini_resnet_block"), ("fp8",), [], {}),          # (no 7x7 stem: the planner refuses it in fp8, recorded as text)
    "resnet_f8": (_resnet_f8, ("fp8",), [{"IE_FORCE_TILE": t} for t in ("0", "3", "102", "203")], {}),
    "resnet_dual_f8": (_resnet_dual_f8, ("fp8",), [{"IE_FORCE_TILE": t} for t in ("102", "109", "203")], {}),
    # fused dense layers (fp32; a case of test_fused_nsplit_gpu.py): every fused tile; without the fragment-major weight mirror every fused tile declines
    # and the parts run, which hand over in turn; the bf16x6 kernel on the layers' 1x1 convs
    "dense_fused": (_dense(60, 3, 4, 4, 64, 2, True), ("fp32",), [{"IE_FUSE_PB": str(t)} for t in range(1, 7)] + [{"IE_FORCE_TILE": "0"}, {"IE_NO_DENSE_FUSE": "1"},
                    {"IE_NO_FRAG_WEIGHTS": "1"}, {"IE_NO_FRAG_WEIGHTS": "1", "IE_FUSE_PB": "4"}, {"IE_NO_FRAG_WEIGHTS": "1", "IE_NO_DENSE_FUSE": "1"},
                    {"IE_FP32_SPLIT": "1", "IE_FORCE_ALGO": "x6"}, {"IE_FP32_SPLIT": "1", "IE_FORCE_ALGO": "x6", "IE_FORCE_TILE": "1"}], {}),
    # dense-block chains (fp16; a case of test_kernel_maps_gpu.py DENSE16, and a 16 x 16 map that only chains in band mode)
    "dense_block": (_dense(70, 3, 4, 4, 64, 3, False), ("fp16",), [{"IE_FORCE_TILE": "0"}, {"IE_NO_DENSE_BLOCK": "1"}], {}),
    "dense_block_16x16": (_dense(64, 2, 16, 16, 64, 2, False), ("fp16",), [{"IE_DENSE_BAND": "1"}], {}),
    "mini_densenet_stem": (_mini("mini_densenet"), ("fp32", "fp16"), [], {"IE_NO_STEM_POOL": "1"}),
    "mini_preact": (_mini("mini_preact"), ("fp32", "fp16"), FORCED, {}),
    "mini_gemm_mlp": (_mini("mini_gemm_mlp"), ("fp32", "fp16"), FEW, {}),
    "vit": (lambda: (vit_graphs.narrow(2), {"input": models.synthetic_input((2, 3, 32, 32), stream="vit")}), ("fp32", "fp16"), TILES_013 + ATTN, {}),
    "attn": (_attn(2, 17, 2, 32), ("fp32", "fp16"), TILES_013 + ATTN, {}),
    "attn_wide": (_attn(*attn_wide_graphs.GPU_SHAPES[0]), ("fp32", "fp16"), TILES_013 + ATTN, {}),
    "swin": (lambda: (swin_graphs.narrow(2), {"input": models.synthetic_input((2, 3, 56, 56), stream="swin")}), ("fp32", "fp16"), TILES_013, {}),
    "wattn": (_wattn, ("fp32", "fp16"), TILES_013, {}),
    "bert": (lambda: (bert_graphs.narrow_bert(3), dict(bert_graphs.narrow_feeds())), ("fp32", "fp16"), TILES_013 + ATTN, {}),
    "gn": (_gn, ("fp32", "fp16"), TILES_013 + [{"IE_GN_TILE": "0"}, {"IE_GN_TILE": "1"}], {}),
    "convt_phase": (_convt(0), ("fp32", "fp16"), TILES_013, {}),
    "convt_overlap": (_convt(3), ("fp32", "fp16"), TILES_013, {}),
    "dw": (lambda: (_dw_graph(), {"x": models.synthetic_input((2, 8, 9, 11), stream="dwblock")}), ("fp32", "fp16"), FEW, {}),
    "grouped": (lambda: (_grouped_graph(), {"x": models.synthetic_input((2, 8, 9, 11), stream="grpblock")}), ("fp32", "fp16"), FEW, {"IE_GROUPED_CONV": "1"}),
    "resize": (lambda: (_resize_graph(), {"x": models.synthetic_input((2, 4, 7, 9), stream="rzblock")}), ("fp32", "fp16"), FEW, {}),
}


def entries(name):
    """[(key, environment)] of one graph: every precision plain and under each switch set"""
    _, precs, switches, base = GRAPHS[name]
    return [("/".join([name, p] + ["%s=%s" % kv for kv in sorted(sw.items())]), dict(base, IE_PRECISION=p, **sw)) for p in precs for sw in [{}] + switches]


@functools.lru_cache(maxsize=None)
def graph(name):
    """(model bytes, feeds, output name, output shape, float64 reference): built and walked once per graph, read-only"""
    mb, feeds = GRAPHS[name][0]()
    oname, oshape, _ = O.load_model(mb).outputs[0]
    ref = ref64.run_f64(mb, feeds)[oname]
    ref.setflags(write=False)
    return mb, feeds, oname, tuple(int(d) for d in oshape), ref


def run_graph(name, root):
    """{key: {"labels": [[step, kernel], ...], "err": rel. error against float64} or {"error": the refusal's text}}"""
    mb, feeds, oname, oshape, ref = graph(name)
    path = models.write_repo(root, name, mb)
    out = {}
    for key, env in entries(name):
        try:
            y, kern = run_model(path, name, env, feeds, oname, oshape, by_step=True)
            out[key] = {"labels": [list(p) for p in kern], "err": ref64.rel_err(y, ref)}
        except RuntimeError as e:
            out[key] = {"error": str(e)}
    return out


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def golden():
    return load_golden()["entries"]


def test_golden_covers_the_matrix(golden):
    keys = [k for name in GRAPHS for k, _ in entries(name)]
    assert len(keys) == len(set(keys)) and sorted(keys) == sorted(golden)


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_launch_labels(name, golden, tmp_path):
    got = run_graph(name, str(tmp_path))
    want = {k: golden.get(k) for k in got}
    moved = {k: (want[k], v.get("labels", v)) for k, v in got.items() if want[k] != v.get("labels", v)}
    assert not moved, "%d of %d entries differ from tests/golden/launch_labels.json (golden, now): %s" % (len(moved), len(got), json.dumps(moved, indent=1)[:4000])
    for k, v in got.items():
        if "err" in v:
            print("%s: rel err %.3e" % (k, v["err"]))
            assert v["err"] < BOUND[k.split("/")[1]], (k, v["err"])


if __name__ == "__main__":
    import time
    result = {}
    for name in sorted(GRAPHS):
        t0 = time.time()
        with tempfile.TemporaryDirectory() as root:
            for k, v in run_graph(name, root).items():
                result[k] = v.get("labels", v)
                if "err" in v:
                    assert v["err"] < BOUND[k.split("/")[1]], (k, v["err"])
        print("%-22s %4d entries so far, %.1f s" % (name, len(result), time.time() - t0), flush=True)
    rev = subprocess.run(["git", "rev-parse", "HEAD"], cwd=HERE, capture_output=True, text=True).stdout.strip()
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    with open(out, "w") as f:      # one line per entry
        f.write('{"generated_at_commit":' + json.dumps(sys.argv[2] if len(sys.argv) > 2 else rev) + ',\n"entries":{\n')
        f.write(",\n".join(json.dumps(k) + ":" + json.dumps(result[k], separators=(",", ":")) for k in sorted(result)) + "\n}}\n")
    print("wrote", out, len(result), "entries")
