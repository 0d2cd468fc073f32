"""GPU (-m gpu): the window-attention kernels on the MI355X against the float64 walk of the literal ONNX nodes (tests/ref64.py), with the
project's bounds (tests/test_gpu_parity.py): fp32 within 2e-4 of max|ref|, fp16 within 3e-3.

Graph: x [N, 3 D, H, W] -> Transpose [0,2,3,1] -> the window region without Linears (roll, partition, attention + bias [+ mask], reverse, roll back)
-> Transpose [0,3,1,2] -> y, so the kernel sees the raw input as q | k | v.  Every case runs on the planner's default tile and on every forced tile the
plan accepts (IE_FORCE_TILE 0 / 1), and the Profile label must be the kernel the plan's tile names.

Shapes (N, H x W, window, shift, heads, hd): L = 16, below one 32-key tile; a rectangular window on a rectangular map with L = 32, exactly one tile;
L = 49 unshifted and shifted (17 real keys in the second tile, all nine mask regions); H != W with three heads (swapped index arithmetic); L = 64,
exactly two tiles; one window per image; hd = 20 (generic kernel only).
Data (tests/vit_graphs.py's generators, the L = H W tokens laid out row by row): randn; peaked (integer k in [-2, 2], q = 16 k: scores of
several hundred, exp overflows without the max subtraction; exact in fp16)."""
import functools

import numpy as np
import pytest

import ref64
import swin_graphs as G
import vit_graphs
from engine_run import plan_of, RTOL, run_model, with_env
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models

pytestmark = pytest.mark.gpu
KINDS = ("randn", "peaked")
SHAPES = [(2, (8, 8), (4, 4), (2, 2), 2, 32), (2, (8, 16), (4, 8), (2, 4), 2, 32), (2, (14, 14), (7, 7), (0, 0), 2, 32), (2, (14, 14), (7, 7), (3, 3), 2, 32),
          (1, (14, 21), (7, 7), (3, 3), 3, 32), (2, (16, 16), (8, 8), (4, 4), 1, 32), (2, (7, 7), (7, 7), (0, 0), 2, 32), (1, (8, 8), (4, 4), (2, 2), 2, 20)]


def _id(s):
    n, hw, win, sh, h, hd = s
    return f"{n}x{hw[0]}x{hw[1]}_w{win[0]}x{win[1]}_s{sh[0]}x{sh[1]}_h{h}_hd{hd}"


@functools.lru_cache(maxsize=None)
def make_input(n, hw, heads, hd, kind):
    """[N, 3 D, H, W]: token y W + x of the attention generators is the map's pixel (y, x)"""
    x = np.array(vit_graphs.make_input(n, hw[0] * hw[1], heads, hd, kind)).reshape(n, 3 * heads * hd, hw[0], hw[1])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(n, hw, win, sh, heads, hd, kind):
    """the float64 walk of the graph, computed once per input"""
    ref = ref64.run_f64(G.wattn_graph(n, hw, win, sh, heads, hd), {"x": make_input(n, hw, heads, hd, kind)})["y"]
    ref.setflags(write=False)
    return ref


def _every_tile(path, name, prec, x, oshape, hd, check, expect_mfma):
    """check(y, tile, forced) on the default tile and on each forced tile the plan accepts"""
    ran = []
    for forced in (None, 0, 1):
        env = dict(IE_PRECISION=prec, **({} if forced is None else {"IE_FORCE_TILE": str(forced)}))
        steps = plan_of(path, x.shape[0], env)["steps"]
        (at,) = [s for s in steps if s["kind"] == "window_attention"]
        if forced is not None and at["tile"] != forced:
            assert at["tile"] == 0                      # not eligible: the generic kernel, which forced tile 0 runs
            continue
        y, kern = run_model(path, name, env, {"x": x}, "y", oshape)
        (label,) = [k for k in kern if k.startswith("window_attention_")]
        assert label == G.wattn_label(at["tile"], at["out"]["f16"], hd), (forced, at["tile"], label)
        assert kern.count("copy_kernel") == 2 and len(kern) == len(steps) == 3, kern          # the NCHW graph input and output only
        check(y, at["tile"], forced)
        ran.append(at["tile"])
    assert sorted(set(ran)) == ([0, 1] if expect_mfma else [0]), ran
    assert ran[0] == int(expect_mfma)                   # the default


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_window_attention(tmp_path, shape, kind, prec):
    n, hw, win, sh, heads, hd = shape
    path = models.write_repo(str(tmp_path), "wattn", G.wattn_graph(n, hw, win, sh, heads, hd))
    x, ref = make_input(n, hw, heads, hd, kind), reference(n, hw, win, sh, heads, hd, kind)

    def check(y, tile, forced):
        assert np.isfinite(y).all(), (kind, tile)
        err = ref64.rel_err(y, ref)
        print(f"{_id(shape)} {kind} {prec} forced {forced} tile {tile}: max err / max|ref| {err:.3e}")
        assert err < RTOL[prec], (shape, kind, prec, tile, err)

    _every_tile(path, "wattn", prec, np.array(x), (n, heads * hd, hw[0], hw[1]), hd, check, G.wattn_mfma_ok(win[0] * win[1], hd, heads * hd, prec == "fp16"))


def test_peaked_scores_are_as_large_as_claimed():
    x = make_input(2, (14, 14), 2, 32, "peaked").astype(np.float64).reshape(2, 3, 2, 32, 196)
    s = np.einsum("nhel,nhem->nhlm", x[:, 0], x[:, 1]) / np.sqrt(32.0)
    assert 200 < np.abs(s).max() < 600


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("tile", [0, 1])
def test_batch_independence(tmp_path, tile, prec):
    """image 1 of an N = 2 run equals the N = 1 run of that image"""
    hw, win, sh, heads, hd = (14, 14), (7, 7), (3, 3), 2, 32
    x = np.array(make_input(2, hw, heads, hd, "randn"))
    env = dict(IE_PRECISION=prec, IE_FORCE_TILE=str(tile))
    y2, _ = run_model(models.write_repo(str(tmp_path), "a2", G.wattn_graph(2, hw, win, sh, heads, hd)), "a2", env, {"x": x}, "y", (2, heads * hd, 14, 14))
    y1, _ = run_model(models.write_repo(str(tmp_path), "a1", G.wattn_graph(1, hw, win, sh, heads, hd)), "a1", env, {"x": x[1:]}, "y", (1, heads * hd, 14, 14))
    np.testing.assert_array_equal(y2[1], y1[0])
    assert ref64.rel_err(y2, reference(2, hw, win, sh, heads, hd, "randn")) < RTOL[prec]


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("tile", [0, 1])
def test_graph_replay_is_bit_identical(tmp_path, tile, prec):
    hw, win, sh, heads, hd = (14, 14), (7, 7), (3, 3), 2, 32
    x = np.array(make_input(2, hw, heads, hd, "randn"))
    path = models.write_repo(str(tmp_path), "rp", G.wattn_graph(2, hw, win, sh, heads, hd))
    oshape = (2, heads * hd, 14, 14)

    def go():
        m = B.CreateModel(path, "rp")
        try:
            r = m.Infer([B.TensorData("x", B.DataTypeFloat32, B.Shape(list(x.shape)), x)], [B.OutputConfig("y", Shape=list(oshape), DataType="FLOAT32")])
            y_host = r[0].Data.reshape(oshape)
            din, dout = B.Prepare(m, [list(x.shape)], 1)
            B.CopyToDevice(m, din[0], x)
            B.RunPrepared(m, 2, True)                                              # graph replay
            y = np.empty(oshape, np.float32)
            B.CopyToHost(m, y, dout[0])
            np.testing.assert_array_equal(y, y_host)
        finally:
            m.Destroy()
    with_env(dict(IE_AUTOTUNE="0", IE_PRECISION=prec, IE_FORCE_TILE=str(tile)), go)


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_qkv_from_a_linear(tmp_path, prec):
    """the qkv rows come from a real Linear (a 1x1 conv kernel wrote them into a 3 D-wide map) and the result feeds the projection Linear"""
    n, hw, win, sh, heads, hd = 2, (14, 14), (7, 7), (3, 3), 2, 32
    mb = G.wattn_graph(n, hw, win, sh, heads, hd, linear=True)
    path = models.write_repo(str(tmp_path), "lin", mb)
    x = np.random.RandomState(4).randn(n, heads * hd, 14, 14).astype(np.float32)
    ref = ref64.run_f64(mb, {"x": x})["y"]
    for tile in (0, 1):
        env = dict(IE_PRECISION=prec, IE_FORCE_TILE=str(tile))
        steps = plan_of(path, n, env)["steps"]
        assert [s["kind"] for s in steps] == ["conv", "window_attention", "conv", "copy"]
        at = steps[1]
        assert at["tile"] == tile and (at["in"]["buf"], at["in"]["pitch"], at["in"]["c"]) == (steps[0]["out"]["buf"], 3 * heads * hd, 3 * heads * hd)
        y, kern = run_model(path, "lin", env, {"x": x}, "y", (n, heads * hd, 14, 14))
        err = ref64.rel_err(y, ref)
        print(f"qkv from a Linear {prec} tile {tile}: max err / max|ref| {err:.3e}; {kern}")
        assert err < RTOL[prec] and G.wattn_label(tile, prec == "fp16", hd) in kern
