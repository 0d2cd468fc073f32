"""GPU (-m gpu): ViT on the MI355X against the float64 walk of tests/ref64.py.  Bounds as tests/test_gpu_parity.py: fp32 within 2e-4 of
max|ref|, fp16 within 3e-3."""

import numpy as np
import pytest

import vit_graphs as G
import ref64
from engine_run import infer, RTOL, run_model, with_env
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def narrow_net(tmp_path_factory):
    mb = G.narrow("N")
    x = models.synthetic_input((2, 3, 32, 32), stream="vit")
    return models.write_repo(str(tmp_path_factory.mktemp("vit")), "vit", mb), mb, x, ref64.run_f64(mb, {"input": x})["logits"]


def _check_labels(kern, depth, attn_prefix):
    assert sum(k.startswith("attention_") for k in kern) == depth and all(k.startswith(attn_prefix) for k in kern if k.startswith("attention_")), kern
    assert sum(k.startswith("token_assemble_kernel") for k in kern) == 1, kern
    assert "copy_kernel" not in kern, kern                   # the patch conv reads the NCHW input itself: no copy at all


@pytest.mark.parametrize("tile", [None, 0])
@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_narrow_net_vs_float64(narrow_net, prec, tile):
    path, mb, x, ref = narrow_net
    y, kern = run_model(path, "vit", dict(IE_PRECISION=prec, **({} if tile is None else {"IE_FORCE_TILE": "0"})), {"input": x}, "logits", (2, 10))
    err = ref64.rel_err(y, ref)
    print(f"narrow ViT {prec} forced tile {tile}: rel err {err:.3e}; {kern}")
    assert err < RTOL[prec]
    _check_labels(kern, 2, "attention_mfma_kernel<%s,32>" % ("f32" if prec == "fp32" else "f16") if tile is None else "attention_generic_kernel")


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_head_dim_64_net_vs_float64(tmp_path, prec):
    mb = G.narrow(2, dim=128, mlp=256)
    path = models.write_repo(str(tmp_path), "vit64", mb)
    x = models.synthetic_input((2, 3, 32, 32), stream="vit64")
    ref = ref64.run_f64(mb, {"input": x})["logits"]
    y, kern = run_model(path, "vit64", dict(IE_PRECISION=prec), {"input": x}, "logits", (2, 10))
    err = ref64.rel_err(y, ref)
    print(f"narrow ViT, hd 64, {prec}: rel err {err:.3e}")
    assert err < RTOL[prec]
    _check_labels(kern, 2, "attention_mfma_kernel<%s,64>" % ("f32" if prec == "fp32" else "f16"))


def test_vit_tiny_at_224(tmp_path):
    mb = models.vit_tiny_16(1)
    path = models.write_repo(str(tmp_path), "tiny", mb)
    x = models.synthetic_input((1, 3, 224, 224), stream="vit_tiny")
    ref = ref64.run_f64(mb, {"input": x})["logits"]
    y, kern = run_model(path, "tiny", dict(IE_PRECISION="fp32"), {"input": x}, "logits", (1, 1000))
    err = ref64.rel_err(y, ref)
    print(f"ViT-Tiny/16 fp32: rel err {err:.3e}")
    assert err < RTOL["fp32"]
    _check_labels(kern, 12, "attention_mfma_kernel<f32,64>")


def test_replay_and_batch_independence(narrow_net):
    path, _, x, ref = narrow_net

    def go():
        m = B.CreateModel(path, "vit")
        try:
            y_host = infer(m, {"input": x}, "logits", (2, 10))
            din, dout = B.Prepare(m, [[2, 3, 32, 32]], 1)
            B.CopyToDevice(m, din[0], x)
            B.RunPrepared(m, 2, True)                                              # graph replay
            y = np.empty((2, 10), np.float32)
            B.CopyToHost(m, y, dout[0])
            np.testing.assert_array_equal(y, y_host)
            y1 = infer(m, {"input": x[:1]}, "logits", (1, 10))
            assert ref64.rel_err(y_host[0], y1[0]) < RTOL["fp32"]
            assert ref64.rel_err(y_host, ref) < RTOL["fp32"]
        finally:
            m.Destroy()
    with_env(dict(IE_AUTOTUNE="0"), go)


def test_autotuned_net_matches(narrow_net):
    """The load-time search has no attention family: it leaves those steps alone and the plan computes the same function"""
    path, _, x, ref = narrow_net

    def go():
        m = B.CreateModel(path, "vit")
        try:
            y = infer(m, {"input": x}, "logits", (2, 10))
            return y, [p["kernel"] for p in B.Profile(m, 1)]
        finally:
            m.Destroy()
    y, kern = with_env(dict(IE_TUNE_CACHE="0", IE_TUNE_BATCHES="2"), go)      # the search runs at load
    assert ref64.rel_err(y, ref) < RTOL["fp32"]
    assert sum(k.startswith("attention_mfma_kernel<f32,32>") for k in kern) == 2


def test_fp8_load_is_refused(narrow_net):
    with pytest.raises(Exception, match="LayerNormalization is not supported in fp8 mode"):
        with_env(dict(IE_PRECISION="fp8", IE_AUTOTUNE="0"), lambda: B.CreateModel(narrow_net[0], "vit"))
