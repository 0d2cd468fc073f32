"""GPU (-m gpu): ConvTranspose on the MI355X against the float64 reference of tests/ref64.py (a torch-CPU double walk; the numpy scatter for
asymmetric pads).  Bounds as tests/test_gpu_parity.py and tests/test_seg_gpu.py: fp32 within 2e-4 of max|ref|, fp16 within 3e-3."""

import numpy as np
import pytest

import convt_graphs as TG
import ref64
from engine_run import infer, plan_of, RTOL, run_model, with_env
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models

pytestmark = pytest.mark.gpu


# ---- seeded random single ops ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("seed", range(TG.NUM_SEEDS))
def test_random_transposed_convs(tmp_path, seed, prec):
    cfg = TG.random_case(seed)
    mb, ishape, oshape = TG.random_graph(cfg)
    path = models.write_repo(str(tmp_path), "ct", mb)
    x = models.synthetic_input(ishape, stream=f"ct{seed}")
    ref = ref64.run_f64(mb, {"x": x})["y"]
    assert ref.shape == oshape
    for env in (dict(), dict(IE_FORCE_TILE="0")):
        st = TG.tconv_step(plan_of(path, 2, dict(IE_PRECISION=prec, **env)))
        y, kern = run_model(path, "ct", dict(IE_PRECISION=prec, **env), {"x": x}, "y", oshape, by_step=True)
        err = ref64.rel_err(y, ref)
        (label,) = [k for n, k in kern if n == st["name"]]
        print(f"seed {seed} {prec} {env} tile {st['tile']} {label}: rel err {err:.3e}")
        assert label.startswith("convt_phase_kernel<" + ("f16" if prec == "fp16" else "f32")) if st["tile"] > 0 else label == "convt_generic_kernel", (cfg, env, label)
        assert err < RTOL[prec], (cfg, env, err)


# ---- whole networks --------------------------------------------------------------------------------------------------------------------------
def _check_unet(mb, path, name, x, oshape, prec):
    ref = ref64.run_f64(mb, {"image": x})["out"]
    y, kern = run_model(path, name, dict(IE_PRECISION=prec), {"image": x}, "out", oshape, by_step=True)
    err = ref64.rel_err(y, ref)
    print(f"{name} {prec}: rel err {err:.3e}; transposed steps {[k for n, k in kern if k.startswith('convt_')]}")
    assert err < RTOL[prec]
    labels = [k for _, k in kern]
    # the skip concats cost nothing: the only copy is the NCHW graph output
    assert labels.count("copy_kernel") <= 1 and [n for n, k in kern if k == "copy_kernel"] == ["to_output(out)"], kern
    assert sum(k.startswith("convt_phase_kernel") for k in labels) == 4 and "convt_generic_kernel" not in labels, kern
    return y, ref


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_unet_vs_float64(tmp_path, prec):
    mb = models.unet(2, image=96, base=16)
    path = models.write_repo(str(tmp_path), "unet", mb)
    x = models.synthetic_input((2, 3, 96, 96), stream="unet")
    _check_unet(mb, path, "unet", x, (2, 2, 96, 96), prec)


def test_unet_sigmoid(tmp_path):
    mb = models.unet(2, image=96, base=16, final="sigmoid")
    path = models.write_repo(str(tmp_path), "unets", mb)
    x = models.synthetic_input((2, 3, 96, 96), stream="unets")
    y, ref = _check_unet(mb, path, "unets", x, (2, 2, 96, 96), "fp32")
    assert y.min() >= 0.0 and y.max() <= 1.0 and ref.min() > 0.0


def test_unet_full_width_at_224(tmp_path):
    mb = models.unet(1)
    path = models.write_repo(str(tmp_path), "unet224", mb)
    x = models.synthetic_input((1, 3, 224, 224), stream="unet224")
    _check_unet(mb, path, "unet224", x, (1, 2, 224, 224), "fp32")


def test_replay_and_batch_independence(tmp_path):
    mb = models.unet("N", image=64, base=16)
    path = models.write_repo(str(tmp_path), "unetr", mb)
    x = models.synthetic_input((2, 3, 64, 64), stream="unetr")

    def go():
        m = B.CreateModel(path, "unetr")
        try:
            y_host = infer(m, {"image": x}, "out", (2, 2, 64, 64))
            din, dout = B.Prepare(m, [[2, 3, 64, 64]], 1)
            B.CopyToDevice(m, din[0], x)
            B.RunPrepared(m, 2, True)                                              # graph replay
            y = np.empty((2, 2, 64, 64), np.float32)
            B.CopyToHost(m, y, dout[0])
            np.testing.assert_array_equal(y, y_host)
            y1 = infer(m, {"image": x[:1]}, "out", (1, 2, 64, 64))
            assert ref64.rel_err(y_host[0], y1[0]) < RTOL["fp32"]
        finally:
            m.Destroy()
    with_env(dict(IE_AUTOTUNE="0"), go)


def test_autotuned_unet_matches(tmp_path):
    """The autotune search over the eligible tiles (tune family 900) leaves a plan that computes the same function"""
    mb = models.unet(2, image=64, base=16)
    path = models.write_repo(str(tmp_path), "unett", mb)
    x = models.synthetic_input((2, 3, 64, 64), stream="unett")
    ref = ref64.run_f64(mb, {"image": x})["out"]

    def go():
        m = B.CreateModel(path, "unett")
        try:
            y = infer(m, {"image": x}, "out", (2, 2, 64, 64))
            return y, [p["kernel"] for p in B.Profile(m, 1)]
        finally:
            m.Destroy()
    y, kern = with_env(dict(IE_TUNE_CACHE="0", IE_TUNE_BATCHES="2"), go)      # the search runs at load
    assert ref64.rel_err(y, ref) < RTOL["fp32"]
    assert sum(k.startswith("convt_") for k in kern) == 4


def test_fp8_load_is_refused(tmp_path):
    path = models.write_repo(str(tmp_path), "unet8", models.unet("N", image=64, base=16))
    with pytest.raises(Exception, match="ConvTranspose is not supported in fp8 mode"):
        with_env(dict(IE_PRECISION="fp8", IE_AUTOTUNE="0"), lambda: B.CreateModel(path, "unet8"))
