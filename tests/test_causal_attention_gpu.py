"""GPU (-m gpu): causal attention on the MI355X -- the CAUSAL forms of tile 0 (attention_generic_kernel) and tile 1 (attention_mfma_kernel) and tile 3
(attention_chunk_kernel, causal and not) -- against the float64 walk of tests/ref64.py with the project's bounds (tests/engine_run.py RTOL: fp32 within
2e-4 of max|ref|, fp16 within 3e-3), in the pattern of tests/test_attention_wide_gpu.py.

The graph is gpt2_graphs.causal_attn_graph: the raw input as q | k | v, GPT-2's Split spelling, the causal mask as Where(cond, scores, finfo.min).  Data:
vit_graphs.make_input's four kinds, all four as requests on one model.  Every case runs on the planner's default tile, on IE_ATTN_TILE=0 (the generic
kernel, the cross-check) and on the pinned MFMA tile; the Profile label must be the kernel the plan's tile names, and every output must be finite.
Shapes (N, L, H) = (2, L, 2), hd 32 and 64:
  tiles 0 / 1: L = 1, 5 (one partial tile), 32 (an exact tile), 33 (the first query whose diagonal tile is the second), 129 and 160 (a second query block
               with a wave at q0 >= 128)
  tile 3:      L = 5, 33, KC, KC + 1, 2 KC + 33 with KC = kAttnChunkKeys: a chunk boundary, waves idle in late chunks, waves past the end; causal and not"""
import functools

import numpy as np
import pytest

import gpt2_graphs as GG
import ref64
import vit_graphs as G
from engine_run import plan_of, RTOL, run_model
from gpu_ai_inference_server_amd.modelgen import models

pytestmark = pytest.mark.gpu
KINDS = ("randn", "peaked", "ramp", "ramp16")
PRECS = ("fp32", "fp16")
N, H = 2, 2


def _attn_step(path, env):
    steps = plan_of(path, N, env)["steps"]
    (at,) = [s for s in steps if s["kind"] == "attention"]
    return at, steps


@functools.lru_cache(maxsize=None)
def _graph(l, hd, causal):
    return GG.causal_attn_graph(N, l, H, hd, mask="where_const" if causal else None)


def _run_case(tmp_path, l, hd, prec, causal, pins):
    """the four kinds on each of `pins` (None: the default tile) -> {pin: [output per kind]}; asserts the tile, the label, finiteness and the bound"""
    xs = [np.array(G.make_input(N, l, H, hd, kind)) for kind in KINDS]
    f16, d = prec == "fp16", H * hd
    if l == 1:      # no feature map reshapes to one token: the qkv rows of all kinds sit in a table, and ids pick a request's rows (gpt2_graphs)
        mb = GG.causal_attn_graph_one_token(np.concatenate([x.reshape(N, 3 * d) for x in xs]), N, H, hd, mask="where_const" if causal else None)
        feeds = [{"input_ids": (N * k + np.arange(N, dtype=np.int64)).reshape(N, 1)} for k in range(len(KINDS))]
    else:
        mb, feeds = _graph(l, hd, causal), [{"x": x} for x in xs]
    path = models.write_repo(str(tmp_path), "cattn", mb)
    out = {}
    for pin in pins:
        env = dict(IE_PRECISION=prec, **({} if pin is None else {"IE_ATTN_TILE": str(pin)}))
        at, steps = _attn_step(path, env)
        default = GG.causal_default_tile(l, hd, d, f16) if causal else (1 if G.attn_mfma_ok(l, hd, d, f16) else 0)
        want = default if pin is None else (pin if pin != 1 or G.attn_mfma_ok(l, hd, d, f16) else 0)
        assert at["tile"] == want and at.get("causal", False) is causal, (pin, at["tile"], want)
        ys, kern = run_model(path, "cattn", env, feeds, "y", (N, d, 1, l))               # (L = 1: [N, 1, D] is the same memory)
        (label,) = [k for k in kern if k.startswith("attention_")]
        assert label == GG.attn_label(at["tile"], at["out"]["f16"], hd, causal), (pin, at["tile"], label)
        assert kern.count("copy_kernel") == (0 if l == 1 else 2) and len(kern) == len(steps), kern      # the NCHW graph input and output only
        for kind, y in zip(KINDS, ys):
            assert np.isfinite(y).all(), (kind, at["tile"])
            err = ref64.rel_err(y, GG.causal_reference(N, l, H, hd, kind, causal))
            print(f"L {l} hd {hd} {kind} {prec} causal {causal} IE_ATTN_TILE {pin} tile {at['tile']}: max err / max|ref| {err:.3e}")
            assert err < RTOL[prec], (l, hd, kind, prec, causal, at["tile"], err)
        out[pin] = ys
    return out


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("hd", (32, 64))
@pytest.mark.parametrize("l", (1, 5, 32, 33, 129, 160))
def test_causal_tiles_0_and_1(tmp_path, l, hd, prec):
    _run_case(tmp_path, l, hd, prec, True, (None, 0, 1))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("causal", (True, False), ids=("causal", "full"))
@pytest.mark.parametrize("hd", (32, 64))
@pytest.mark.parametrize("l", (5, 33, GG.KC, GG.KC + 1, 2 * GG.KC + 33))
def test_tile_3(tmp_path, l, hd, causal, prec):
    """tile 3 against float64, against the generic kernel's run and -- where tile 1 holds the sequence -- against tile 1 on the same input: both within
    the bound, and bit-equal, since the two kernels share one key-tile routine and walk the tiles in one order"""
    ys = _run_case(tmp_path, l, hd, prec, causal, (None, 0, 3, 1))
    if G.attn_mfma_ok(l, hd, H * hd, prec == "fp16"):
        for kind, y1, y3 in zip(KINDS, ys[1], ys[3]):
            assert np.array_equal(y1, y3), (kind, float(np.abs(y1 - y3).max()))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("tile, l, ps", [(0, 160, (40, 127)), (1, 160, (40, 127)), (3, 160, (40, 127)), (3, 2 * GG.KC + 33, (127, GG.KC + 40, 2 * GG.KC + 5))])
def test_causality_without_a_reference(tmp_path, tile, l, ps, prec):
    """every token row behind position p changed (q, k and v): the output rows <= p keep their bits.  p in the middle of a key tile, p = 127 (the last
    query of a workgroup), and on tile 3 positions in the second and third chunk"""
    hd = 64
    path = models.write_repo(str(tmp_path), "cattn", _graph(l, hd, True))
    x = np.array(G.make_input(N, l, H, hd, "randn"))
    feeds = [{"x": x}]
    for p in ps:
        x2 = x.copy()
        x2[..., p + 1:] = np.random.RandomState(p).randn(*x2[..., p + 1:].shape).astype(np.float32) * 3.0
        feeds.append({"x": x2})
    ys, kern = run_model(path, "cattn", dict(IE_PRECISION=prec, IE_ATTN_TILE=str(tile)), feeds, "y", (N, H * hd, 1, l))
    assert GG.attn_label(tile, prec == "fp16", hd, True) in kern
    for p, y in zip(ps, ys[1:]):
        assert np.array_equal(y[..., :p + 1], ys[0][..., :p + 1]), (tile, p)
        assert not np.array_equal(y[..., p + 1:], ys[0][..., p + 1:])


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("tile, l", [(1, 160), (3, GG.KC + 33)])
def test_batch_independence_and_repeat(tmp_path, tile, l, prec):
    """image 1 of an N = 2 run equals the N = 1 run of that image, and the same request twice gives the same bits"""
    hd = 64
    x = np.array(G.make_input(N, l, H, hd, "randn"))
    env = dict(IE_PRECISION=prec, IE_ATTN_TILE=str(tile))
    (y2, y2b), k2 = run_model(models.write_repo(str(tmp_path), "a2", _graph(l, hd, True)), "a2", env, [{"x": x}, {"x": x}], "y", (2, H * hd, 1, l))
    y1, k1 = run_model(models.write_repo(str(tmp_path), "a1", GG.causal_attn_graph(1, l, H, hd)), "a1", env, {"x": x[1:]}, "y", (1, H * hd, 1, l))
    label = GG.attn_label(tile, prec == "fp16", hd, True)
    assert label in k2 and label in k1
    np.testing.assert_array_equal(y2[1], y1[0])
    assert np.array_equal(y2, y2b)
    assert ref64.rel_err(y2, GG.causal_reference(N, l, H, hd, "randn")) < RTOL[prec]


@pytest.mark.parametrize("prec", PRECS)
def test_qkv_from_a_linear(tmp_path, prec):
    """the qkv rows come from a real Linear (a 1x1 conv kernel wrote them, pitch 3 D)"""
    l, hd = 33, 64
    mb = GG.causal_attn_graph(N, l, H, hd, linear=True)
    path = models.write_repo(str(tmp_path), "lin", mb)
    x = np.random.RandomState(4).randn(N, H * hd, 1, l).astype(np.float32)
    ref = ref64.run_f64(mb, {"x": x})["y"]
    for tile in (0, 1, 3):
        env = dict(IE_PRECISION=prec, IE_ATTN_TILE=str(tile))
        steps = plan_of(path, N, env)["steps"]
        assert [s["kind"] for s in steps] == ["conv", "attention", "copy"]
        at = steps[1]
        assert at["tile"] == tile and at["causal"] is True and (at["in"]["buf"], at["in"]["pitch"], at["in"]["c"]) == (steps[0]["out"]["buf"], 3 * H * hd, 3 * H * hd)
        y, kern = run_model(path, "lin", env, {"x": x}, "y", (N, H * hd, 1, l))
        err = ref64.rel_err(y, ref)
        print(f"qkv from a Linear {prec} tile {tile}: max err / max|ref| {err:.3e}; {kern}")
        assert np.isfinite(y).all() and err < RTOL[prec] and GG.attn_label(tile, prec == "fp16", hd, True) in kern
