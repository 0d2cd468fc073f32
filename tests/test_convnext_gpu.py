"""GPU (-m gpu): ConvNeXt on the MI355X against the float64 walk of tests/ref64.py.  Bounds as tests/test_gpu_parity.py: fp32 within
2e-4 of max|ref|, fp16 within 3e-3."""

import numpy as np
import pytest

import convnext_graphs as G
import ref64
from engine_run import infer, RTOL, run_model, with_env
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models
from gpu_ai_inference_server_amd.modelgen import onnx_pb as pb

pytestmark = pytest.mark.gpu


# ---- one block ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("gelu,swap", [("erf", False), ("erf", True), ("erf_mul", False), ("op", False), ("op_tanh", False)])
@pytest.mark.parametrize("c", [8, 96])
def test_block(tmp_path, c, gelu, swap, prec):
    mb = models.convnext_block(2, c, 6, gelu=gelu, gelu_swap=swap)
    path = models.write_repo(str(tmp_path), "blk", mb)
    x = np.random.RandomState(c).randn(2, c, 6, 6).astype(np.float32)
    ref = ref64.run_f64(mb, {"x": x})["y"]
    y, kern = run_model(path, "blk", dict(IE_PRECISION=prec), {"x": x}, "y", (2, c, 6, 6), by_step=True)
    err = ref64.rel_err(y, ref)
    print(f"block C {c} {gelu} swap {swap} {prec}: rel err {err:.3e}; {[k for _, k in kern]}")
    assert err < RTOL[prec]
    labels = [k for _, k in kern]
    # NCHW input -> NHWC, depthwise, layer norm, fc1, GELU, fc2 (+ bias + layer scale), the shortcut Add (its other operand is the graph input,
    # which no conv epilogue reads), NHWC -> NCHW output
    assert [k.split("<")[0] for k in labels[:3]] == ["copy_kernel", "conv_dw_generic_kernel", "layernorm_kernel"], kern
    assert len(labels) == 8 and labels[4] == labels[6] == "eltwise_kernel" and labels[7] == "copy_kernel", kern


def test_gelu_fused_into_a_depthwise_conv(tmp_path):
    """a GELU behind a depthwise conv is the conv's epilogue, on the generic kernel"""
    gb = models.GraphBuilder("g", 3)
    y = gb.gelu(gb.conv(gb.conv("x", 4, 16, 1), 16, 16, 3, pad=1, group=16, name="dw"), "op")
    gb.nodes.append(pb.node("Identity", [y], ["y"], "out"))
    mb = gb.finish([("x", [2, 4, 9, 9])], [("y", [2, 16, 9, 9])], opset=20)
    path = models.write_repo(str(tmp_path), "dwg", mb)
    x = np.random.RandomState(1).randn(2, 4, 9, 9).astype(np.float32)
    ref = ref64.run_f64(mb, {"x": x})["y"]
    y, kern = run_model(path, "dwg", dict(IE_PRECISION="fp32"), {"x": x}, "y", (2, 16, 9, 9), by_step=True)
    assert ref64.rel_err(y, ref) < RTOL["fp32"]
    assert "conv_dw_generic_kernel" in [k for _, k in kern] and "eltwise_kernel" not in [k for _, k in kern], kern


# ---- whole networks --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def narrow_net(tmp_path_factory):
    mb = G.narrow("N")
    x = models.synthetic_input((2, 3, 64, 64), stream="convnext")
    return models.write_repo(str(tmp_path_factory.mktemp("cnx")), "cnx", mb), mb, x, ref64.run_f64(mb, {"input": x})["logits"]


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_narrow_net_vs_float64(narrow_net, prec):
    path, mb, x, ref = narrow_net
    y, kern = run_model(path, "cnx", dict(IE_PRECISION=prec), {"input": x}, "logits", (2, 1000), by_step=True)
    err = ref64.rel_err(y, ref)
    print(f"narrow ConvNeXt {prec}: rel err {err:.3e}; layer norms {[k for _, k in kern if k.startswith('layernorm_')]}")
    assert err < RTOL[prec]
    labels = [k for _, k in kern]
    # the Transposes cost nothing: no copy at all (the [N, classes] output needs none), one layer-norm launch per LayerNormalization node
    assert "copy_kernel" not in labels, kern
    assert sum(k.startswith("layernorm_") for k in labels) == 5 + 3 + 2 and labels.count("eltwise_kernel") == 5, kern


def test_convnext_tiny_at_224(tmp_path):
    mb = models.convnext_tiny(1)
    path = models.write_repo(str(tmp_path), "tiny", mb)
    x = models.synthetic_input((1, 3, 224, 224), stream="convnext_tiny")
    ref = ref64.run_f64(mb, {"input": x})["logits"]
    y, kern = run_model(path, "tiny", dict(IE_PRECISION="fp32"), {"input": x}, "logits", (1, 1000), by_step=True)
    err = ref64.rel_err(y, ref)
    print(f"ConvNeXt-Tiny fp32: rel err {err:.3e}")
    assert err < RTOL["fp32"]
    assert sum(k.startswith("layernorm_kernel<f32") for _, k in kern) == 23 and "copy_kernel" not in [k for _, k in kern]


def test_replay_and_batch_independence(narrow_net):
    path, _, x, ref = narrow_net

    def go():
        m = B.CreateModel(path, "cnx")
        try:
            y_host = infer(m, {"input": x}, "logits", (2, 1000))
            din, dout = B.Prepare(m, [[2, 3, 64, 64]], 1)
            B.CopyToDevice(m, din[0], x)
            B.RunPrepared(m, 2, True)                                              # graph replay
            y = np.empty((2, 1000), np.float32)
            B.CopyToHost(m, y, dout[0])
            np.testing.assert_array_equal(y, y_host)
            y1 = infer(m, {"input": x[:1]}, "logits", (1, 1000))
            assert ref64.rel_err(y_host[0], y1[0]) < RTOL["fp32"]
            assert ref64.rel_err(y_host, ref) < RTOL["fp32"]
        finally:
            m.Destroy()
    with_env(dict(IE_AUTOTUNE="0"), go)


def test_autotuned_net_matches(narrow_net):
    """The autotune search over the eligible layer-norm tiles (tune family 1000) and the conv kernels leaves a plan that computes the same function"""
    path, _, x, ref = narrow_net

    def go():
        m = B.CreateModel(path, "cnx")
        try:
            y = infer(m, {"input": x}, "logits", (2, 1000))
            return y, [p["kernel"] for p in B.Profile(m, 1)]
        finally:
            m.Destroy()
    y, kern = with_env(dict(IE_TUNE_CACHE="0", IE_TUNE_BATCHES="2"), go)      # the search runs at load
    assert ref64.rel_err(y, ref) < RTOL["fp32"]
    assert sum(k.startswith("layernorm_") for k in kern) == 10


def test_fp8_load_is_refused(narrow_net):
    with pytest.raises(Exception, match="LayerNormalization is not supported in fp8 mode"):
        with_env(dict(IE_PRECISION="fp8", IE_AUTOTUNE="0"), lambda: B.CreateModel(narrow_net[0], "cnx"))
