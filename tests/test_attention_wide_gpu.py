"""GPU (-m gpu): attention tile 2 (attention_stream_kernel: one wide head, hd 128 / 256 / 512) on the MI355X against the float64 walk of tests/ref64.py,
with the project's bounds (tests/engine_run.py RTOL: fp32 within 2e-4 of max|ref|, fp16 within 3e-3), in the pattern of tests/test_attention_gpu.py.

Every case runs on the planner's default tile, on IE_ATTN_TILE=0 (the generic kernel, the cross-check) and on IE_ATTN_TILE=2; the Profile label must be
the kernel the plan's tile names, and every output must be finite.  Shapes: attn_wide_graphs.GPU_SHAPES.  Data: vit_graphs.make_input's four kinds
(tests/test_attention_wide_plan.py asserts what they reach at these head dims, and that a lost or misplaced head-dim quarter would show)."""
import functools

import numpy as np
import pytest

import attn_wide_graphs as W
import gn_graphs as GN
import ref64
import vit_graphs as G
from engine_run import plan_of, RTOL, run_model
from gpu_ai_inference_server_amd.modelgen import models

pytestmark = pytest.mark.gpu
KINDS = ("randn", "peaked", "ramp", "ramp16")
PRECS = ("fp32", "fp16")


@functools.lru_cache(maxsize=None)
def reference(n, l, h, hd, kind):
    """the float64 walk of the graph, computed once per input"""
    ref = ref64.run_f64(G.attn_graph(n, l, h, hd), {"x": G.make_input(n, l, h, hd, kind)})["y"]
    ref.setflags(write=False)
    return ref


def _attn_step(path, batch, env):
    steps = plan_of(path, batch, env)["steps"]
    (at,) = [s for s in steps if s["kind"] == "attention"]
    return at, steps


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", W.GPU_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_wide_attention(tmp_path, shape, kind, prec):
    n, l, h, hd = shape
    path = models.write_repo(str(tmp_path), "attn", G.attn_graph(n, l, h, hd))
    x, ref = np.array(G.make_input(n, l, h, hd, kind)), reference(n, l, h, hd, kind)
    ran = []
    for pinned in (None, "0", "2"):
        env = dict(IE_PRECISION=prec, **({} if pinned is None else {"IE_ATTN_TILE": pinned}))
        at, steps = _attn_step(path, n, env)
        assert at["tile"] == (W.attn_default_tile(l, hd, h * hd, prec == "fp16") if pinned is None else int(pinned))
        y, kern = run_model(path, "attn", env, {"x": x}, "y", (n, h * hd, 1, l))
        (label,) = [k for k in kern if k.startswith("attention_")]
        assert label == W.attn_label(at["tile"], at["out"]["f16"], hd), (pinned, at["tile"], label)
        assert kern.count("copy_kernel") == 2 and len(kern) == len(steps), kern          # the NCHW graph input and output only
        assert np.isfinite(y).all(), (kind, at["tile"])
        err = ref64.rel_err(y, ref)
        print(f"N {n} L {l} H {h} hd {hd} {kind} {prec} IE_ATTN_TILE {pinned} tile {at['tile']}: max err / max|ref| {err:.3e}")
        assert err < RTOL[prec], (shape, kind, prec, at["tile"], err)
        ran.append(at["tile"])
    assert ran == [2 if l >= W.MIN_TOKENS else 0, 0, 2]


@pytest.mark.parametrize("prec", PRECS)
def test_qkv_from_a_linear(tmp_path, prec):
    """the qkv rows come from a real Linear (a 1x1 conv kernel wrote them, pitch 3 D)"""
    n, l, h, hd = 2, 33, 1, 128
    mb = G.attn_graph(n, l, h, hd, linear=True)
    path = models.write_repo(str(tmp_path), "lin", mb)
    x = np.random.RandomState(4).randn(n, h * hd, 1, l).astype(np.float32)
    ref = ref64.run_f64(mb, {"x": x})["y"]
    for tile in (0, 2):
        env = dict(IE_PRECISION=prec, IE_ATTN_TILE=str(tile))
        steps = plan_of(path, n, env)["steps"]
        assert [s["kind"] for s in steps] == ["conv", "attention", "copy"]
        at = steps[1]
        assert at["tile"] == tile and (at["in"]["buf"], at["in"]["pitch"], at["in"]["c"]) == (steps[0]["out"]["buf"], 3 * h * hd, 3 * h * hd)
        y, kern = run_model(path, "lin", env, {"x": x}, "y", (n, h * hd, 1, l))
        err = ref64.rel_err(y, ref)
        print(f"qkv from a Linear {prec} tile {tile}: max err / max|ref| {err:.3e}; {kern}")
        assert np.isfinite(y).all() and err < RTOL[prec] and W.attn_label(tile, prec == "fp16", hd) in kern


@pytest.mark.parametrize("prec", PRECS)
def test_batch_independence(tmp_path, prec):
    """image 1 of an N = 2 run equals the N = 1 run of that image, on tile 2"""
    n, l, h, hd = 2, 33, 2, 256
    x = np.array(G.make_input(n, l, h, hd, "randn"))
    env = dict(IE_PRECISION=prec, IE_ATTN_TILE="2")
    y2, k2 = run_model(models.write_repo(str(tmp_path), "a2", G.attn_graph(2, l, h, hd)), "a2", env, {"x": x}, "y", (2, h * hd, 1, l))
    y1, k1 = run_model(models.write_repo(str(tmp_path), "a1", G.attn_graph(1, l, h, hd)), "a1", env, {"x": x[1:]}, "y", (1, h * hd, 1, l))
    assert W.attn_label(2, prec == "fp16", hd) in k2 and W.attn_label(2, prec == "fp16", hd) in k1
    np.testing.assert_array_equal(y2[1], y1[0])         # one workgroup per (image, head, query block) and nothing shared between them
    assert ref64.rel_err(y2, reference(n, l, h, hd, "randn")) < RTOL[prec]


@pytest.mark.parametrize("prec", PRECS)
def test_two_requests_are_bit_equal(tmp_path, prec):
    """no atomics and one fixed order for the four partial score tiles: the same input gives the same bits"""
    n, l, h, hd = 2, 160, 1, 512
    path = models.write_repo(str(tmp_path), "det", G.attn_graph(n, l, h, hd))
    x = np.array(G.make_input(n, l, h, hd, "randn"))
    (y1, y2), kern = run_model(path, "det", dict(IE_PRECISION=prec, IE_ATTN_TILE="2"), [{"x": x}, {"x": x}], "y", (n, h * hd, 1, l))
    assert W.attn_label(2, prec == "fp16", hd) in kern
    assert np.array_equal(y1, y2)
    assert ref64.rel_err(y1, reference(n, l, h, hd, "randn")) < RTOL[prec]


@pytest.fixture(scope="module")
def decoder12(tmp_path_factory):
    """the narrow decoder on latents 12 x 12 (attention: hd 128, L = 144), one input and the float64 output (a walk of two seconds); read-only"""
    mb = GN.narrow_decoder(1, latent=12)
    z = GN.half_exact(np.random.RandomState(22).randn(1, 4, 12, 12))
    ref = ref64.run_f64(mb, {"latent_sample": z})["sample"]
    ref.setflags(write=False)
    return models.write_repo(str(tmp_path_factory.mktemp("dec12")), "dec12", mb), z, ref


@pytest.mark.parametrize("prec", PRECS)
def test_vae_decoder_vs_float64(decoder12, prec):
    path, z, ref = decoder12
    y, kern = run_model(path, "dec12", dict(IE_PRECISION=prec), {"latent_sample": z}, "sample", ref.shape)
    assert np.isfinite(y).all()
    err = ref64.rel_err(y, ref)
    print(f"vae_decoder latent 12 {prec}: max err / max|ref| {err:.3e}")
    assert W.attn_label(2, prec == "fp16", 128) in kern and not any(k.startswith("attention_generic") for k in kern)
    assert err < RTOL[prec], (prec, err)
