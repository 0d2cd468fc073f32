"""GPU (-m gpu): rotary positions and grouped K / V heads inside the attention kernels, on the attention subgraph alone, against the float64 walk of
the same graph (tests/ref64.py), per element, with the project's bounds: fp32 within 2e-4 of max|ref|, fp16 within 3e-3.

The graph is llama_graphs.gqa_attn_graph: the raw input as q (D) | k (Dkv) | v (Dkv) (the q / k / v "Linears" pick its columns with 0 / 1 weights), Llama's
rotary embedding on q and k, repeat_kv, the causal mask as the additive triangular constant.  K and V heads are independent draws, so a query head that
read another K / V head than h / group would miss the bound by orders of magnitude.  (heads, kv_heads): (4, 4), (4, 2), (4, 1).
Tile 1: hd 32 and 64; L = 40 (a tail tile with padded keys), L = 129 (a second query block, and the causal staging limit of the first).  Tile 3, pinned with
IE_ATTN_TILE=3: L = kAttnChunkKeys + 8 = 264, so the keys of the second chunk must be rotated at their global position.  Tile 0: hd 48 (L = 5, and L = 1 through
an id input, since no feature map reshapes to one token), and a non-causal rope graph.  One case per tile has cos / sin tables of independent random values in BOTH halves of a row instead of true rope tables."""

import numpy as np
import pytest

import llama_graphs as LG
import ref64
from engine_run import plan_of, RTOL, run_model
from gpu_ai_inference_server_amd.modelgen import models

pytestmark = pytest.mark.gpu
N, H = 2, 4


def _run(tmp_path, prec, l, kvh, hd, *, env=None, tile, causal=True, rope="init", tables=None, name="gqa"):
    mb = LG.gqa_attn_graph(N, l, H, kvh, hd, rope=rope, tables=tables, causal=causal)
    path = models.write_repo(str(tmp_path), name, mb)
    x = LG.gqa_input(N, l, H, kvh, hd)
    ref = ref64.run_f64(mb, {"x": x})["y"]
    e = dict(IE_PRECISION=prec, **(env or {}))
    (at,) = [s for s in plan_of(path, N, e)["steps"] if s["kind"] == "attention"]
    assert at["tile"] == tile and at.get("rope", False) is (rope is not None) and at.get("kv_heads", H) == kvh and at.get("causal", False) is causal, at
    y, kern = run_model(path, name, e, {"x": x}, "y", (N, H * hd, 1, l))
    assert LG.attn_label(tile, prec == "fp16", hd, causal, rope is not None) in kern, kern
    err = ref64.rel_err(y, ref)
    print(f"attention L {l} heads {H}/{kvh} hd {hd} {prec} tile {tile} causal {causal} rope {rope} tables {'random' if tables else 'rope'}: max err / max|ref| {err:.3e}")
    assert np.isfinite(y).all() and err < RTOL[prec], (l, kvh, hd, prec, tile, err)
    return y


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("kvh", [4, 2, 1])
@pytest.mark.parametrize("l, hd", [(40, 64), (129, 32), (129, 64), (40, 32)])
def test_tile1(tmp_path, l, hd, kvh, prec):
    assert LG.rope_default_tile(l, hd, H, kvh, prec == "fp16") == 1
    _run(tmp_path, prec, l, kvh, hd, tile=1)


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("kvh, hd", [(4, 64), (2, 32), (1, 64)])
def test_tile3_second_chunk_at_its_global_position(tmp_path, kvh, hd, prec):
    _run(tmp_path, prec, LG.KC + 8, kvh, hd, env={"IE_ATTN_TILE": "3"}, tile=3)


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_tile0(tmp_path, prec):
    assert LG.rope_default_tile(5, 48, H, 2, prec == "fp16") == 0
    _run(tmp_path, prec, 5, 2, 48, tile=0)                                    # hd 48: no MFMA tile
    _run(tmp_path, prec, 40, 2, 64, tile=0, causal=False, name="nc")          # non-causal rope: the generic kernel, whatever the head dim
    _run(tmp_path, prec, 40, 1, 64, env={"IE_FORCE_TILE": "0"}, tile=0, name="f0")      # the cross-check of tile 1's case


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_one_token(tmp_path, prec):
    """L = 1 (hd 48, tile 0): the only key is the query's own, so the answer is v's row of the head's group whatever the rotation does to q and k; the
    tables are random ones, so a NaN or a wrong row out of the rotation would show"""
    import gpt2_graphs as GG
    kvh, hd, r = 2, 48, 7
    c = (H + 2 * kvh) * hd
    rows = np.random.RandomState(9).randn(r, c).astype(np.float32)
    ids = np.array([[3], [6]], np.int64)
    mb = LG.gqa_attn_graph_one_token(rows, N, H, kvh, hd, tables=LG.random_tables(1, hd))
    ref = ref64.run_f64(mb, {"input_ids": ids})
    (oname, ref), = ref.items()
    path = models.write_repo(str(tmp_path), "one", mb)
    env = dict(IE_PRECISION=prec)
    (at,) = [s for s in plan_of(path, N, env)["steps"] if s["kind"] == "attention"]
    assert at["tile"] == 0 and at["rope"] is True and at["kv_heads"] == kvh and at["in"]["w"] == 1
    ys, shapes, kern = GG.run_outputs(path, "one", env, {"input_ids": ids}, {oname: (N, 1, H * hd)})
    assert "attention_generic_kernel<causal>" in kern and shapes == {oname: [N, 1, H * hd]}
    err = ref64.rel_err(ys[oname], ref)
    print(f"one token hd {hd} {prec}: max err / max|ref| {err:.3e}")
    assert np.isfinite(ys[oname]).all() and err < RTOL[prec]


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("tile, l, hd, env", [(1, 40, 64, {}), (3, LG.KC + 8, 32, {"IE_ATTN_TILE": "3"}), (0, 40, 64, {"IE_FORCE_TILE": "0"})])
def test_tables_with_independent_halves(tmp_path, tile, l, hd, env, prec):
    """cos / sin of independent random values in both halves of every row: a kernel that reads only half a table row (true rope tables repeat theirs) shows"""
    _run(tmp_path, prec, l, 2, hd, env=env, tile=tile, tables=LG.random_tables(l, hd), rope="unsqueeze")


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_grouped_heads_without_rope(tmp_path, prec):
    _run(tmp_path, prec, 129, 2, 64, tile=1, rope=None)
    _run(tmp_path, prec, LG.KC + 8, 1, 32, env={"IE_ATTN_TILE": "3"}, tile=3, rope=None, name="g3")
    _run(tmp_path, prec, 40, 2, 48, tile=0, rope=None, name="g0")


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_full_heads_without_rope_equal_gpt2s_reference(tmp_path, prec):
    """kv_heads == heads and no rope through the new spelling: the operand layout is GPT-2's q | k | v, and so is the answer"""
    import gpt2_graphs as GG
    l, hd = 40, 64
    mb = LG.gqa_attn_graph(N, l, H, H, hd, rope=None)
    x = GG.G.make_input(N, l, H, hd, "randn")
    ref = GG.causal_reference(N, l, H, hd, "randn")
    assert ref64.rel_err(ref64.run_f64(mb, {"x": x})["y"], ref) < 1e-12
    path = models.write_repo(str(tmp_path), "mha", mb)
    env = dict(IE_PRECISION=prec)
    y, kern = run_model(path, "mha", env, {"x": x}, "y", (N, H * hd, 1, l))
    assert GG.attn_label(1, prec == "fp16", hd, True) in kern
    err = ref64.rel_err(y, ref)
    print(f"full heads, no rope, L {l} hd {hd} {prec}: max err / max|ref| {err:.3e}")
    assert err < RTOL[prec]
