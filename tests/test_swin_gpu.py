"""GPU (-m gpu): the narrow Swin end to end against the float64 walk of its literal ONNX nodes (tests/ref64.py), on the default tiles and on the
generic kernels, with the project's bounds (fp32 2e-4, fp16 3e-3 of max|ref|); graph replay; the load-time search leaves the new steps alone; patch
merging alone, exact against the reference's gather."""
import numpy as np
import pytest

import swin_graphs as G
import ref64
from engine_run import infer, RTOL, run_model, with_env
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def narrow_net(tmp_path_factory):
    mb = G.narrow("N")
    x = models.synthetic_input((2, 3, 56, 56), stream="swin")
    return models.write_repo(str(tmp_path_factory.mktemp("swin")), "swin", mb), mb, x, ref64.run_f64(mb, {"input": x})["logits"]


def _check_labels(kern, prefix):
    assert sum(k.startswith("window_attention_") for k in kern) == 4 and all(k.startswith(prefix) for k in kern if k.startswith("window_attention_")), kern
    assert sum(k.startswith("patch_merge_kernel") for k in kern) == 1 and "copy_kernel" not in kern, kern


@pytest.mark.parametrize("tile", [None, 0])
@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_narrow_net_vs_float64(narrow_net, prec, tile):
    path, mb, x, ref = narrow_net
    y, kern = run_model(path, "swin", dict(IE_PRECISION=prec, **({} if tile is None else {"IE_FORCE_TILE": "0"})), {"input": x}, "logits", (2, 10))
    err = ref64.rel_err(y, ref)
    print(f"narrow Swin {prec} forced tile {tile}: rel err {err:.3e}; {kern}")
    assert err < RTOL[prec]
    _check_labels(kern, "window_attention_mfma_kernel<%s,32>" % ("f32" if prec == "fp32" else "f16") if tile is None else "window_attention_generic_kernel")
    assert ("patch_merge_kernel<%s>" % ("f32,4" if prec == "fp32" else "f16,8")) in kern


def test_replay_and_batch_independence(narrow_net):
    path, _, x, ref = narrow_net

    def go():
        m = B.CreateModel(path, "swin")
        try:
            y_host = infer(m, {"input": x}, "logits", (2, 10))
            din, dout = B.Prepare(m, [[2, 3, 56, 56]], 1)
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
    """The load-time search has no family for the new steps: it leaves them alone and the plan computes the same function"""
    path, _, x, ref = narrow_net

    def go():
        m = B.CreateModel(path, "swin")
        try:
            y = infer(m, {"input": x}, "logits", (2, 10))
            return y, [p["kernel"] for p in B.Profile(m, 1)]
        finally:
            m.Destroy()
    y, kern = with_env(dict(IE_TUNE_CACHE="0", IE_TUNE_BATCHES="2"), go)      # the search runs at load
    assert ref64.rel_err(y, ref) < RTOL["fp32"]
    _check_labels(kern, "window_attention_mfma_kernel<f32,32>")


def test_fp8_load_is_refused(narrow_net):
    with pytest.raises(Exception, match="LayerNormalization is not supported in fp8 mode"):
        with_env(dict(IE_PRECISION="fp8", IE_AUTOTUNE="0"), lambda: B.CreateModel(narrow_net[0], "swin"))


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("c,vec", [(8, True), (5, False)])
def test_patch_merge_alone(tmp_path, c, vec, prec):
    """6 x 10 x C: C = 8 takes the 16-byte vector path, C = 5 the element path; a pure gather, so fp32 is bit-equal to the reference and fp16 bit-equal
    after rounding the input to fp16"""
    n, hw = 2, (6, 10)
    mb = G.merge_graph(n, c, hw)
    path = models.write_repo(str(tmp_path), "merge", mb)
    x = np.random.RandomState(c).randn(n, c, *hw).astype(np.float32)
    xin = x.astype(np.float16).astype(np.float32) if prec == "fp16" else x
    ref = ref64.run_f64(mb, {"x": xin})["y"]
    np.testing.assert_array_equal(ref[:, c:2 * c], xin[:, :, 1::2, 0::2])             # torchvision's x1 = x[..., 1::2, 0::2, :]

    def go():
        m = B.CreateModel(path, "merge")
        try:
            y = infer(m, {"x": x}, "y", (n, 4 * c, 3, 5))
            return y, [p["kernel"] for p in B.Profile(m, 1)]
        finally:
            m.Destroy()
    y, kern = with_env(dict(IE_AUTOTUNE="0", IE_PRECISION=prec), go)
    want = "patch_merge_kernel<%s,%d>" % ("f16" if prec == "fp16" else "f32", (8 if prec == "fp16" else 4) if vec and (prec == "fp32" or c % 8 == 0) else 1)
    assert kern == ["copy_kernel", want, "copy_kernel"], kern
    np.testing.assert_array_equal(y, ref.astype(np.float32))
