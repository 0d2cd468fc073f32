"""GPU (-m gpu): the causal, rotary and grouped forms of attention tile 2 (attention_stream_kernel<T, HD, CAUSAL, ROPE>: one wide head, hd 128 / 256 /
512) on the MI355X, on the attention subgraph alone, against the float64 walk of the same graph (tests/ref64.py), per element, with the project's
bounds (tests/engine_run.py RTOL: fp32 within 2e-4 of max|ref|, fp16 within 3e-3).  N = 2.  Every case asserts the plan's tile and the Profile label.

Causal alone (gpt2_graphs.causal_attn_graph, IE_ATTN_TILE=2 and the generic kernel as the cross-check): (L, hd) = (5, 128) one tile, the diagonal one,
with padded keys and queries; (32, 256) exactly one full tile; (33, 128) a second query block of one query whose diagonal tile holds one real key;
(72, 512) full tiles under the diagonal, a diagonal tile and a tail; and the unpinned default at L = kAttnStreamCausalMinTokens + 8.
Rope and grouped heads (llama_graphs.gqa_attn_graph, H = 4): kv_heads 4, 2 and 1 at hd 128, L = 40 (the second tile's keys are rotated at positions
32 - 39); kv_heads 2 at hd 256, L = 72; tables of independent values in both halves of a row; grouped heads without rope, causal and not; the
unpinned default.  K and V heads are independent draws, so a wrong head mapping misses the bound by orders of magnitude; what a lost rotary half-slice
pair would do is pinned on the CPU (tests/test_attention_stream_causal_plan.py).  Causality and determinism are checked bit for bit."""
import numpy as np
import pytest

import attn_stream_causal_graphs as SC
import gpt2_graphs as GG
import llama_graphs as LG
import ref64
import vit_graphs as G
from engine_run import plan_of, RTOL, run_model
from gpu_ai_inference_server_amd.modelgen import models

pytestmark = pytest.mark.gpu
PRECS = ("fp32", "fp16")
N, H = 2, 4
T = SC.CAUSAL_MIN_TOKENS


def _check(path, name, env, x, ref, oshape, *, tile, hd, causal, rope, what):
    (at,) = [s for s in plan_of(path, N, env)["steps"] if s["kind"] == "attention"]
    assert at["tile"] == tile and at.get("causal", False) is causal and at.get("rope", False) is rope, at
    y, kern = run_model(path, name, env, {"x": x}, "y", oshape)
    (label,) = [k for k in kern if k.startswith("attention_")]
    assert label == SC.attn_label(tile, env["IE_PRECISION"] == "fp16", hd, causal, rope), (what, label)
    err = ref64.rel_err(y, ref)
    print(f"{what} {env['IE_PRECISION']} tile {tile} ({label}): max err / max|ref| {err:.3e}")
    assert np.isfinite(y).all() and err < RTOL[env["IE_PRECISION"]], (what, env, err)
    return y


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("l, hd, pinned", [(5, 128, True), (32, 256, True), (33, 128, True), (72, 512, True), (T + 8, 128, False)],
                         ids=("L5_hd128", "L32_hd256", "L33_hd128", "L72_hd512", "default_hd128"))
def test_causal(tmp_path, l, hd, pinned, prec):
    h = 2 if hd == 128 else 1
    path = models.write_repo(str(tmp_path), "c", GG.causal_attn_graph(N, l, h, hd))
    x, ref = np.array(G.make_input(N, l, h, hd, "randn")), GG.causal_reference(N, l, h, hd, "randn")
    if not pinned:
        assert SC.default_tile(l, hd, h, h, prec == "fp16") == 2
    for env_tile, tile in (({"IE_ATTN_TILE": "2"} if pinned else {}, 2), ({"IE_ATTN_TILE": "0"}, 0)):
        _check(path, "c", dict(IE_PRECISION=prec, **env_tile), x, ref, (N, h * hd, 1, l), tile=tile, hd=hd, causal=True, rope=False,
               what=f"causal L {l} H {h} hd {hd}")


def _gqa(tmp_path, prec, l, kvh, hd, *, pinned=True, tile=2, causal=True, rope="init", tables=None, name="gqa"):
    mb = LG.gqa_attn_graph(N, l, H, kvh, hd, rope=rope, tables=tables, causal=causal)
    path = models.write_repo(str(tmp_path), name, mb)
    x = LG.gqa_input(N, l, H, kvh, hd)
    ref = ref64.run_f64(mb, {"x": x})["y"]
    env = dict(IE_PRECISION=prec, **({"IE_ATTN_TILE": str(tile)} if pinned else {}))
    (at,) = [s for s in plan_of(path, N, env)["steps"] if s["kind"] == "attention"]
    assert at.get("kv_heads", H) == kvh
    return _check(path, name, env, x, ref, (N, H * hd, 1, l), tile=tile, hd=hd, causal=causal, rope=rope is not None,
                  what=f"L {l} heads {H}/{kvh} hd {hd} causal {causal} rope {rope} tables {'random' if tables else 'rope'}")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("l, kvh, hd", [(40, 4, 128), (40, 2, 128), (40, 1, 128), (72, 2, 256)])
def test_rope_and_grouped_heads(tmp_path, l, kvh, hd, prec):
    _gqa(tmp_path, prec, l, kvh, hd)


@pytest.mark.parametrize("prec", PRECS)
def test_rope_cross_check_on_the_generic_kernel(tmp_path, prec):
    _gqa(tmp_path, prec, 40, 2, 128, tile=0)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("l, hd", [(40, 128), (72, 256)])
def test_tables_with_independent_halves(tmp_path, l, hd, prec):
    """cos / sin of independent random values in both halves of every row: a kernel that reads only half a table row (true rope tables repeat theirs) shows"""
    _gqa(tmp_path, prec, l, 2, hd, tables=LG.random_tables(l, hd), rope="unsqueeze")


@pytest.mark.parametrize("prec", PRECS)
def test_grouped_heads_without_rope(tmp_path, prec):
    _gqa(tmp_path, prec, 40, 2, 128, rope=None, name="gc")
    _gqa(tmp_path, prec, 40, 1, 128, rope=None, causal=False, name="gn")


@pytest.mark.parametrize("prec", PRECS)
def test_default_tile_of_a_rotary_grouped_step(tmp_path, prec):
    assert SC.default_tile(T + 8, 128, H, 2, prec == "fp16", rope=True) == 2
    _gqa(tmp_path, prec, T + 8, 2, 128, pinned=False)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("rope", [None, "init"], ids=("causal", "causal_rope"))
def test_causality_and_determinism_bitwise(tmp_path, rope, prec):
    """two requests whose inputs differ only in the tokens >= 40 of L = 72: the output rows < 40 are the same bits (a key above the diagonal is replaced
    before anything depends on it), the rows >= 40 are not; and the first request again gives the same bits (no atomics, one order of the four partial
    score tiles)"""
    l, kvh, hd = 72, 2, 128
    path = models.write_repo(str(tmp_path), "cb", LG.gqa_attn_graph(N, l, H, kvh, hd, rope=rope))
    x = LG.gqa_input(N, l, H, kvh, hd)
    x2 = x.copy()
    x2[..., 40:] = LG.gqa_input(N, l, H, kvh, hd, seed=1)[..., 40:]
    (y1, y2, y3), kern = run_model(path, "cb", dict(IE_PRECISION=prec, IE_ATTN_TILE="2"), [{"x": x}, {"x": x2}, {"x": x}], "y", (N, H * hd, 1, l))
    assert SC.attn_label(2, prec == "fp16", hd, True, rope is not None) in kern, kern
    assert np.array_equal(y1[..., :40], y2[..., :40])
    assert all(not np.array_equal(y1[..., j], y2[..., j]) for j in range(40, l))
    assert np.array_equal(y1, y3)
