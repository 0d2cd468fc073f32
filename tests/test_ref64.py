"""CPU: tests/ref64.py, the one float64 reference, is what the per-family walkers it replaced were, and agrees with the independent oracle.

tests/golden/ref64_parent.npz holds what those walkers (dw_ref, grouped_ref, se_ref, seg_ref, unet_ref, convnext_ref, vit_ref, swin_ref, bert_ref,
gn_ref at the commit before they were merged) gave on the graphs of CASES with the feeds of feeds_of(): vectors in full, maps as y[..., ::8, ::8]
with y.sum() and (y * y).sum().  The walkers that were numpy already must be reproduced bitwise; the torch ones within 1e-12 of max|stored|, the
tightest tolerance the suite applies to these references (what remains is double rounding: F.batch_norm against the definition, torch's mean and
sigmoid against numpy's).
"""
import os

import numpy as np
import pytest

import bert_graphs
import gn_graphs
import ref64
import swin_graphs
import vit_graphs
from conftest import MINI, ROOT
from gpu_ai_inference_server_amd.modelgen import models
from gpu_ai_inference_server_amd.modelgen import onnx_pb as pb
from oracle import onnx_oracle as O

RTOL = 1e-12
BERT = dict(seq=40, vocab=50, dim=64, depth=2, heads=2, mlp=128, max_pos=64, pooler_output=True)

# name -> (graph, bitwise, run_f64 options)
CASES = {
    "vit": (lambda: vit_graphs.narrow(2), True, {}),
    "swin": (lambda: swin_graphs.narrow(2), True, {}),
    "bert": (lambda: models.bert(3, **BERT), True, {}),
    "gn_resnet": (lambda: models.resnet(2, norm="gn", gn_groups=8, width=16, image=64, classes=10), True, {}),
    "gn_resnet_half": (lambda: models.resnet(2, norm="gn", gn_groups=8, width=16, image=64, classes=10), True, dict(round_half=True)),
    "vae_decoder": (lambda: gn_graphs.narrow_decoder(1), True, {}),
    "wattn_no_bias": (lambda: swin_graphs.wattn_graph(2, 8, 4, 2, 2, 4), True, dict(overrides={"w_rpb": np.zeros((1, 2, 16, 16))})),
    "mobilenet_v2": (lambda: models.mobilenet_v2("N", width_mult=0.5, image=64, classes=10, seed=64), False, {}),
    "efficientnet_b0": (lambda: models.efficientnet_b0("N", width_mult=0.5, image=96, classes=100, seed=92), False, {}),
    "mobilenet_v3": (lambda: models.mobilenet_v3("N", variant="large", width_mult=0.75, image=96, classes=40, seed=93, act_form="hardsigmoid_mul"), False, {}),
    "resnext": (lambda: models.resnext50_32x4d("N", layers=(1, 1, 1, 1), image=64, classes=20, seed=51), False, {}),
    "deeplab_scales": (lambda: models.deeplabv3_resnet50("N", width=8, image=64, resize="scales"), False, {}),
    "deeplab_sizes": (lambda: models.deeplabv3_resnet50(2, width=8, image=64), False, {}),
    "unet": (lambda: models.unet(2, image=64, base=16, final="sigmoid"), False, {}),
    "convnext": (lambda: models.convnext(2, depths=(1, 1, 2, 1), dims=(16, 32, 64, 128), image=64), False, {}),
}


def feeds_of(name, mb):
    """BERT: the narrow net's ids / mask / types; else RandomState(0).randn per input as float32, a symbolic batch being 2"""
    if name == "bert":
        return bert_graphs.narrow_feeds()
    st = np.random.RandomState(0)
    return {k: st.randn(*[d if d > 0 else 2 for d in shape]).astype(np.float32) for k, shape, _ in O.load_model(mb).inputs}


def stored_form(y):
    """{suffix: array}: a vector output in full; a map as its every-8th pixel, its sum and its sum of squares"""
    if y.ndim == 4 and y.shape[2] * y.shape[3] > 64:
        return {"": y[..., ::8, ::8], ".sum": y.sum(), ".sumsq": (y * y).sum()}
    return {"": y}


@pytest.fixture(scope="module")
def parent():
    with np.load(os.path.join(ROOT, "tests", "golden", "ref64_parent.npz")) as z:
        return {k: z[k] for k in z.files}


def test_fixture_holds_every_case(parent):
    assert {k.split("/")[0] for k in parent} == set(CASES)
    assert all(v.dtype == np.float64 for v in parent.values())


@pytest.mark.parametrize("name", list(CASES))
def test_reproduces_the_walkers_it_replaced(parent, name):
    make, bitwise, opts = CASES[name]
    mb = make()
    got = ref64.run_f64(mb, feeds_of(name, mb), **opts)
    assert got and all(v.dtype == np.float64 for v in got.values())
    for out, y in got.items():
        for suffix, v in stored_form(y).items():
            want = parent[f"{name}/{out}{suffix}"]
            err = ref64.rel_err(v, want)
            print(f"{name} {out}{suffix}: {err:.2e} of max|stored|")
            assert np.shape(v) == want.shape
            if bitwise:
                np.testing.assert_array_equal(v, want)
            assert err < RTOL


@pytest.mark.parametrize("name", list(MINI))
def test_agrees_with_the_oracle(name):
    """the oracle's own float64 run is independent of ref64 (its Conv is an im2col matmul, its pools strided views)"""
    make, iname, shape = MINI[name]
    mb = make(models)
    x = np.random.RandomState(0).randn(*shape).astype(np.float32)
    want = O.run(O.load_model(mb), {iname: x}, dtype=np.float64)
    got = ref64.run_f64(mb, {iname: x})
    assert set(got) == set(want)
    for k in want:
        assert got[k].shape == want[k].shape
        err = ref64.rel_err(got[k], want[k])
        print(f"{name} {k}: {err:.2e}")
        assert err < RTOL


def test_unknown_operator_is_named():
    gb = models.GraphBuilder("unknown", 1)
    gb.simple("Relu", [gb.simple("Celu", ["x"], [pb.attr_float("alpha", 1.0)])], out="y")
    mb = gb.finish([("x", [1, 4])], [("y", [1, 4])], opset=17)
    with pytest.raises(NotImplementedError, match="^Celu$"):
        ref64.run_f64(mb, {"x": np.zeros((1, 4), np.float32)})
