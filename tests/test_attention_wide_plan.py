"""CPU: attention tile 2 (the streaming kernel for one wide head) through the planner: where the default picks it, what IE_ATTN_TILE and
IE_FORCE_TILE make of it, which steps never get it, and the VAE decoder at the size from which its attention takes it.  The float64 restatement of
tests/attn_wide_graphs.py is checked against tests/ref64.py, and the GPU test's data against two broken ways of splitting the head dim."""
import numpy as np
import pytest

import attn_wide_graphs as W
import bert_graphs as BG
import gn_graphs as GN
import ref64
import vit_graphs as G
from engine_run import describe, RTOL
from gpu_ai_inference_server_amd.modelgen import models

PRECS = ("fp32", "fp16")
# (IE_FORCE_TILE, IE_ATTN_TILE)
SETTINGS = [(None, None), (None, "2"), (None, "0"), (None, "1"), ("0", None), ("1", None), ("2", None), ("0", "2")]


def _tile(path, batch, monkeypatch, prec, force=None, attn=None):
    """the tile of the model's one attention step under IE_FORCE_TILE = force and IE_ATTN_TILE = attn (None: unset)"""
    monkeypatch.delenv("IE_ATTN_TILE", raising=False)
    env = {k: v for k, v in (("IE_FORCE_TILE", force), ("IE_ATTN_TILE", attn)) if v is not None}
    (at,) = [s for s in describe(path, batch, monkeypatch, prec, **env)["steps"] if s["kind"] == "attention"]
    return at["tile"]


def _tiles(path, monkeypatch, prec):
    return {st: _tile(path, 2, monkeypatch, prec, *st) for st in SETTINGS}


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("heads", [1, 2])
@pytest.mark.parametrize("hd", W.WIDE_HEAD_DIMS)
def test_wide_head_tiles(tmp_path, monkeypatch, hd, heads, prec):
    assert W.MIN_TOKENS > 64
    for l in (5, 64, W.MIN_TOKENS - 1, W.MIN_TOKENS, 160):
        path = models.write_repo(str(tmp_path), f"a{l}", G.attn_graph(2, l, heads, hd))
        dflt = 2 if l >= W.MIN_TOKENS else 0
        assert W.attn_default_tile(l, hd, heads * hd, prec == "fp16") == dflt
        want = {(None, None): dflt, (None, "2"): 2, (None, "0"): 0, (None, "1"): 0, ("0", None): 0, ("1", None): 0, ("2", None): dflt, ("0", "2"): 0}
        assert _tiles(path, monkeypatch, prec) == want, (l, heads, hd)


@pytest.mark.parametrize("prec", PRECS)
def test_other_head_dims_stay_off_tile_2(tmp_path, monkeypatch, prec):
    for l, heads, hd in ((160, 2, 96), (160, 2, 20)):
        path = models.write_repo(str(tmp_path), f"a{hd}", G.attn_graph(2, l, heads, hd))
        assert set(_tiles(path, monkeypatch, prec).values()) == {0}, hd
    path = models.write_repo(str(tmp_path), "a64", G.attn_graph(2, 33, 3, 64))
    assert _tile(path, 2, monkeypatch, prec) == 1 and _tile(path, 2, monkeypatch, prec, attn="2") == 0
    assert _tile(path, 2, monkeypatch, prec, attn="1") == 1 and _tile(path, 2, monkeypatch, prec, attn="0") == 0
    # a narrow head past tile 1's LDS budget keeps the generic kernel
    lmax = G.max_mfma_tokens(64, prec == "fp16")
    path = models.write_repo(str(tmp_path), "along", G.attn_graph(2, lmax + 1, 1, 64))
    assert set(_tiles(path, monkeypatch, prec).values()) == {0}


@pytest.mark.parametrize("prec", PRECS)
def test_masked_wide_head_stays_generic(tmp_path, monkeypatch, prec):
    path = models.write_repo(str(tmp_path), "m128", BG.masked_attn_graph(2, 160, 1, 128))
    assert _tile(path, 2, monkeypatch, prec) == 0 and _tile(path, 2, monkeypatch, prec, attn="2") == 0


@pytest.mark.parametrize("prec", PRECS)
def test_decoder_attention_takes_tile_2(tmp_path, monkeypatch, prec):
    """latents 12 x 12: hd 128, L = 144 >= MIN_TOKENS.  Every other count as tests/test_groupnorm_plan.py::test_vae_decoder_plan has them"""
    monkeypatch.delenv("IE_ATTN_TILE", raising=False)
    steps = describe(models.write_repo(str(tmp_path), "dec12", GN.narrow_decoder("N", latent=12)), 2, monkeypatch, prec)["steps"]
    kinds = [s["kind"] for s in steps]
    layers, nm = GN.NARROW["layers"], len(GN.NARROW["mults"])
    blocks = 2 + nm * (layers + 1)
    assert kinds.count("group_norm") == 2 * blocks + 2 and kinds.count("conv") == 2 * blocks + 2 + 3 + 3 + 2
    assert kinds.count("resize") == nm - 1 and kinds.count("attention") == 1 and kinds.count("copy") == 1 and kinds.count("eltwise") == 1
    (at,) = [s for s in steps if s["kind"] == "attention"]
    assert (at["heads"], at["head_dim"], at["tile"], at["in"]["w"]) == (1, 128, 2, 144)
    # the narrow decoder of the other tests (L = 64) keeps the generic kernel
    assert _tile(models.write_repo(str(tmp_path), "dec8", GN.narrow_decoder("N")), 2, monkeypatch, prec) == 0


def test_restatement_is_the_graphs_attention():
    n, l, h, hd = 2, 33, 2, 128
    x = G.make_input(n, l, h, hd, "randn")
    ref = ref64.run_f64(G.attn_graph(n, l, h, hd), {"x": x})["y"]
    assert ref64.rel_err(W.attention_f64(x, h, hd), ref) < 1e-6          # (the graph's scale constant is a float32)


@pytest.mark.parametrize("shape", W.GPU_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_broken_splits_are_visible(shape):
    """a lost partial score tile, or two waves' output slices swapped, moves the result by more than 30 x the fp16 bound at every GPU shape: the GPU
    test cannot pass with either"""
    n, l, h, hd = shape
    x = G.make_input(n, l, h, hd, "randn")
    ref = W.attention_f64(x, h, hd)
    for quarter in range(4):
        assert ref64.rel_err(W.attention_f64(x, h, hd, drop_quarter=quarter), ref) > 30 * RTOL["fp16"], (shape, quarter)
    for pair in ((0, 1), (1, 2), (2, 3), (0, 3)):
        assert ref64.rel_err(W.attention_f64(x, h, hd, swap_quarters=pair), ref) > 30 * RTOL["fp16"], (shape, pair)


def test_peaked_and_ramp_scores_are_as_claimed():
    """hd 512: peaked scores of about 700 (exp overflows without the max subtraction: fp32 exp gives inf from 88.7 on); the ramp's score of key j is
    a multiple of j that grows the running maximum in every tile of 32 keys, in both ramps"""
    q, k, _ = W.unpack(G.make_input(2, 160, 1, 512, "peaked"), 1, 512)
    s = W.scores(q, k)
    assert 500 < np.abs(s).max() < 1500
    assert s.max(-1).min() > 88.7                                        # every row overflows
    for kind, step in (("ramp", 1.0 / 8.0), ("ramp16", 1.0 / 128.0)):
        for l, hd in ((160, 512), (144, 256), (33, 128)):
            q, k, _ = W.unpack(G.make_input(2, l, 2 if hd == 256 else 1, hd, kind), 2 if hd == 256 else 1, hd)
            s = W.scores(q, k)
            np.testing.assert_allclose(s[0, 0, 5], np.arange(float(l)) * step * np.sqrt(hd), rtol=1e-12)
            tile_max = [s[0, 0, 5, j:j + 32].max() for j in range(0, l, 32)]
            assert all(b > a for a, b in zip(tile_max, tile_max[1:]))
