"""GPU (-m gpu): the attention kernels on the MI355X against the float64 walk of tests/ref64.py, with the project's bounds
(tests/test_gpu_parity.py): fp32 within 2e-4 of max|ref|, fp16 within 3e-3.

Graph: x [N, 3 D, 1, L] -> Reshape [N, 3 D, L] -> Transpose [0,2,1] -> the attention pattern -> Transpose [0,2,1] -> Reshape [N, D, 1, L] -> y, so the
kernel sees the raw input as q | k | v.  Every case runs on the planner's default tile and on every forced tile the plan accepts (IE_FORCE_TILE 0 / 1),
and the Profile label must be the kernel the plan's tile names.

Shapes (N, L, H, hd): fewer keys than one 32-key tile; exactly one; one key and one query into a second tile (zero-filled padding that is not masked
would move the result by tens of percent); ViT-B/32's L = 50; one query into the second 128-query workgroup; ViT's own 197; hd = 20 (generic kernel
only); the largest L inside the MFMA kernel's LDS budget and the first past it (generic only), per precision.
Data: randn; peaked (integer k in [-2, 2], q = 16 k: scores of several hundred, exp overflows without the max subtraction; exact in fp16); two ramps
(score of key j = j, resp. j / 16, for hd = 64: the running maximum grows in every key tile, by 32 or by 2, so the online rescale always fires and,
with the slow ramp, every tile still contributes)."""
import functools

import numpy as np
import pytest

import vit_graphs as G
import ref64
from engine_run import plan_of, RTOL, run_model
from gpu_ai_inference_server_amd.modelgen import models

pytestmark = pytest.mark.gpu
KINDS = ("randn", "peaked", "ramp", "ramp16")
LMAX = {prec: G.max_mfma_tokens(64, prec == "fp16") for prec in RTOL}
SHAPES = [(2, 5, 1, 32), (2, 32, 2, 64), (2, 33, 3, 64), (1, 50, 2, 32), (1, 129, 2, 64), (2, 197, 3, 64), (2, 7, 2, 20)]


@functools.lru_cache(maxsize=None)
def reference(n, l, h, hd, kind):
    """the float64 walk of the graph (the spelling does not matter to it: tests/test_vit_plan.py), computed once per input"""
    ref = ref64.run_f64(G.attn_graph(n, l, h, hd), {"x": G.make_input(n, l, h, hd, kind)})["y"]
    ref.setflags(write=False)
    return ref


def _every_tile(path, name, prec, x, oshape, hd, check, expect_mfma=None):
    """check(y, tile, forced) on the default tile and on each forced tile the plan accepts; -> the tiles that ran"""
    ran = []
    for forced in (None, 0, 1):
        env = dict(IE_PRECISION=prec, **({} if forced is None else {"IE_FORCE_TILE": str(forced)}))
        steps = plan_of(path, x.shape[0], env)["steps"]
        (at,) = [s for s in steps if s["kind"] == "attention"]
        if forced is not None and at["tile"] != forced:
            assert at["tile"] == 0                      # not eligible: the generic kernel, which forced tile 0 runs
            continue
        y, kern = run_model(path, name, env, {"x": x}, "y", oshape)
        (label,) = [k for k in kern if k.startswith("attention_")]
        assert label == G.attn_label(at["tile"], at["out"]["f16"], hd), (forced, at["tile"], label)
        assert kern.count("copy_kernel") == 2 and len(kern) == len(steps), kern          # the NCHW graph input and output only
        check(y, at["tile"], forced)
        ran.append(at["tile"])
    if expect_mfma is not None:
        assert sorted(set(ran)) == ([0, 1] if expect_mfma else [0]), ran
        assert ran[0] == int(expect_mfma)               # the default
    return ran


def _case(tmp_path, n, l, h, hd, kind, prec, **graph_kw):
    mb = G.attn_graph(n, l, h, hd, **graph_kw)
    path = models.write_repo(str(tmp_path), "attn", mb)
    x, ref = G.make_input(n, l, h, hd, kind), reference(n, l, h, hd, kind)

    def check(y, tile, forced):
        assert np.isfinite(y).all(), (kind, tile)
        err = ref64.rel_err(y, ref)
        print(f"N {n} L {l} H {h} hd {hd} {kind} {prec} {graph_kw or ''} forced {forced} tile {tile}: max err / max|ref| {err:.3e}")
        assert err < RTOL[prec], (n, l, h, hd, kind, prec, tile, err)

    _every_tile(path, "attn", prec, np.array(x), (n, h * hd, 1, l), hd, check, expect_mfma=G.attn_mfma_ok(l, hd, h * hd, prec == "fp16"))


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_attention(tmp_path, shape, kind, prec):
    _case(tmp_path, *shape, kind, prec)


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("past", [0, 1])
def test_attention_at_the_lds_budget(tmp_path, past, kind, prec):
    """L = the largest sequence the MFMA kernel takes (288 in fp32, 544 in fp16, hd = 64) and one more (generic kernel only)"""
    assert LMAX == {"fp32": 288, "fp16": 544}
    _case(tmp_path, 1, LMAX[prec] + past, 1, 64, kind, prec)


def test_peaked_scores_are_as_large_as_claimed():
    x = G.make_input(2, 197, 3, 64, "peaked").astype(np.float64)[:, :, 0, :].transpose(0, 2, 1).reshape(2, 197, 3, 3, 64)
    s = np.einsum("nlhe,nmhe->nhlm", x[:, :, 0], x[:, :, 1]) / 8.0
    assert 200 < np.abs(s).max() < 400
    r = G.make_input(1, 129, 2, 64, "ramp").astype(np.float64)[:, :, 0, :].transpose(0, 2, 1).reshape(1, 129, 3, 2, 64)
    s = np.einsum("nlhe,nmhe->nhlm", r[:, :, 0], r[:, :, 1]) / 8.0
    np.testing.assert_array_equal(s[0, 0, 5], np.arange(129.0))          # the score of key j is exactly j


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("scale", G.SCALES)
def test_scale_forms(tmp_path, scale, swap, prec):
    _case(tmp_path, 2, 33, 3, 64, "randn", prec, scale=scale, swap=swap)


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_split_unbind(tmp_path, prec):
    _case(tmp_path, 2, 33, 3, 64, "randn", prec, unbind="split", scale="s_div")


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("tile", [0, 1])
def test_batch_independence(tmp_path, tile, prec):
    """image 1 of an N = 2 run equals the N = 1 run of that image"""
    n, l, h, hd = 2, 50, 2, 32
    x = np.array(G.make_input(n, l, h, hd, "randn"))
    env = dict(IE_PRECISION=prec, IE_FORCE_TILE=str(tile))
    y2, _ = run_model(models.write_repo(str(tmp_path), "a2", G.attn_graph(2, l, h, hd)), "a2", env, {"x": x}, "y", (2, h * hd, 1, l))
    y1, _ = run_model(models.write_repo(str(tmp_path), "a1", G.attn_graph(1, l, h, hd)), "a1", env, {"x": x[1:]}, "y", (1, h * hd, 1, l))
    assert ref64.rel_err(y2[1], y1[0]) < RTOL[prec]
    assert ref64.rel_err(y2, reference(n, l, h, hd, "randn")) < RTOL[prec]


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_qkv_from_a_linear(tmp_path, prec):
    """the qkv rows come from a real Linear (a 1x1 conv kernel wrote them), and the result feeds nothing but the output copy"""
    n, l, h, hd = 2, 33, 2, 32
    mb = G.attn_graph(n, l, h, hd, linear=True)
    path = models.write_repo(str(tmp_path), "lin", mb)
    x = np.random.RandomState(4).randn(n, h * hd, 1, l).astype(np.float32)
    ref = ref64.run_f64(mb, {"x": x})["y"]
    for tile in (0, 1):
        env = dict(IE_PRECISION=prec, IE_FORCE_TILE=str(tile))
        steps = plan_of(path, n, env)["steps"]
        assert [s["kind"] for s in steps] == ["conv", "attention", "copy"]             # (the conv reads the NCHW input itself)
        at = steps[1]
        assert at["tile"] == tile and (at["in"]["buf"], at["in"]["pitch"], at["in"]["c"]) == (steps[0]["out"]["buf"], 3 * h * hd, 3 * h * hd)
        y, kern = run_model(path, "lin", env, {"x": x}, "y", (n, h * hd, 1, l))
        err = ref64.rel_err(y, ref)
        print(f"qkv from a Linear {prec} tile {tile}: max err / max|ref| {err:.3e}; {kern}")
        assert err < RTOL[prec] and G.attn_label(tile, prec == "fp16", hd) in kern
