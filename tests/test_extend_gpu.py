"""GPU (-m gpu): extend steps (a past of P rows and Lq >= 2 new tokens) against the float64 walk of the same graph on the same feeds (tests/ref64.py), with
the project's bounds: fp32 within 2e-4 of max|ref|, fp16 within 3e-3.

The attention subgraph alone (extend_graphs.extend_attn_graph): `out` and both `present` outputs, N = 2.  Every K / V head and cache row is another draw.
Image 0 is valid in 3 cache rows only.  The rope tables have independent random values in both halves of a row, the positions differ per image and run
backwards inside the chunk, so a kernel that adds the token's index to one position fails.  In every case the plan's tile and the launched kernel are
asserted, the rows of `out` whose own key is valid are compared and the rest checked finite, `present` rows >= P are compared against float64 and rows
< P with the `past` input bit for bit.  Then the narrow Llama end to end (prefill, extend, decode) and an out-of-range position through ModelInfer.

Both tiles: 0 (kv_append_kernel + attention_extend_generic_kernel) and 5 (kv_append_kernel + attention_extend_kernel, with key splits and the
combine), fp32 and fp16."""
import numpy as np
import pytest

import extend_graphs as EG
import gpt2_graphs as GG
import kv_graphs as KG
import ref64
from engine_run import plan_of, RTOL, tensor, with_env
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models

pytestmark = pytest.mark.gpu
N = 2
PRECS = ("fp32", "fp16")
TILES = (0, EG.EXTEND_TILE)
MAX_POS = 64


def _outs(h, kvh, hd, past, lq):
    return {"out": (N, lq, h * hd), "present.0.key": (N, kvh, past + lq, hd), "present.0.value": (N, kvh, past + lq, hd)}


def _check(ys, ref, feeds, past, prec, what):
    for k in ("present.0.key", "present.0.value"):
        assert np.array_equal(ys[k][:, :, :past], feeds[k.replace("present", "past_key_values")]), (what, k, "rows < P are not the past, bit for bit")
        err = ref64.rel_err(ys[k][:, :, past:], ref[k][:, :, past:])
        print(f"{what} {k} rows >= P: max err / max|ref| {err:.3e}")
        assert np.isfinite(ys[k]).all() and err < RTOL[prec], (what, k, err)
    own = EG.own_key_valid(feeds, past)
    assert np.isfinite(ys["out"]).all(), (what, "out is not finite")
    err = ref64.rel_err(ys["out"][own], ref["out"][own])
    print(f"{what} out ({own.sum()} of {own.size} rows): max err / max|ref| {err:.3e}")
    assert err < RTOL[prec], (what, "out", err)


def _run(tmp_path, prec, h, kvh, hd, past, lq, *, tile=0, env=None, rope="input", valid=(3, None), chunk_valid=None, left=False, name="ext", splits=None):
    """one extend step of the subgraph under `env`, the plan's tile and splits and the launched kernel asserted, every output checked against float64"""
    rows, feeds = EG.extend_feeds(N, h, kvh, hd, past, lq, valid=valid, chunk_valid=chunk_valid, left=left, rope=rope, max_pos=MAX_POS)
    assert rope is None or (lq < 2 or feeds["position_ids"][0, 0] != feeds["position_ids"][0, 1] - 1)
    mb = EG.extend_attn_graph(rows, N, h, kvh, hd, past, lq, rope=rope, tables=KG.LG.random_tables(MAX_POS, hd) if rope else None, max_pos=MAX_POS)
    ref = ref64.run_f64(mb, feeds)
    path = models.write_repo(str(tmp_path), name, mb)
    e = dict(IE_PRECISION=prec, **(env or {}))
    (at,) = [s for s in plan_of(path, N, e)["steps"] if s["kind"] == "attention"]
    assert (at["tile"], at["past_len"], at["new_len"], at["chunk_causal"], at["key_mask"], at.get("rope", False)) == (tile, past, lq, True, True, rope is not None), at
    want = None if tile == 0 else (splits or EG.default_splits(N, kvh, (h // kvh) * lq, past + lq))
    assert at.get("splits") == want, at
    outs = _outs(h, kvh, hd, past, lq)
    ys, shapes, kern = GG.run_outputs(path, name, e, feeds, outs)
    assert EG.extend_label(tile, prec == "fp16", hd, want or 1) in kern, kern
    assert shapes == {k: list(v) for k, v in outs.items()}
    _check(ys, ref, feeds, past, prec, f"extend H {h}/{kvh} hd {hd} P {past} Lq {lq} {prec} tile {tile} S {want} rope {rope}")
    return ys


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("h, kvh", ((4, 4), (4, 2), (4, 1), (6, 2)))
@pytest.mark.parametrize("hd", (32, 64))
def test_heads_and_head_dims(tmp_path, hd, h, kvh, tile, prec):
    _run(tmp_path, prec, h, kvh, hd, 33, 5, tile=tile, env={"IE_ATTN_TILE": str(tile)})


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("past", (1, 31, 32, 33, 255, 256, 257))
def test_cache_lengths(tmp_path, past, tile, prec):
    """P round a 32-key tile and a 256-key chunk"""
    _run(tmp_path, prec, 4, 2, 64, past, 5, tile=tile, env={"IE_ATTN_TILE": str(tile)})


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("h, lq", ((4, 2), (4, 16), (4, 17), (4, 64), (4, 65), (6, 43)))
def test_chunk_lengths(tmp_path, h, lq, tile, prec):
    """g Lq = 4 ... 130 query rows at g = 2 and 129 at g = 3: round a 32-row wave and a 128-row block"""
    _run(tmp_path, prec, h, 2, 64, 40, lq, tile=tile, env={"IE_ATTN_TILE": str(tile)})


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("form", ("no rope", "rope", "left-padded", "ragged"))
def test_forms(tmp_path, form, tile, prec):
    kw = {"no rope": dict(rope=None), "rope": {}, "left-padded": dict(left=True), "ragged": dict(chunk_valid=(6, 4))}[form]
    _run(tmp_path, prec, 4, 2, 32, 40, 6, tile=tile, env={"IE_ATTN_TILE": str(tile)}, **kw)


@pytest.mark.parametrize("prec", PRECS)
def test_generic_route(tmp_path, prec):
    """hd 48 fits no fast kernel: the default plan and a pinned tile 5 are both the generic pair"""
    assert not EG.fast_fits(48, 4, 2)
    _run(tmp_path, prec, 4, 2, 48, 21, 5)
    _run(tmp_path, prec, 4, 2, 48, 21, 5, env={"IE_ATTN_TILE": "5"}, name="pin")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("splits", (1, 3, None))
def test_long_cache_and_splits(tmp_path, splits, prec):
    """P = 300, Lq = 8 with IE_ATTN_SPLITS 1, 3 and the default (2): image 0 is valid in 3 cache rows, so at S = 3 its first split holds them, its second
    masked keys only, and both must leave the combine with the right weights; the default plan (no pin) runs attention_extend_kernel"""
    _run(tmp_path, prec, 4, 2, 64, 300, 8, tile=EG.EXTEND_TILE, env={} if splits is None else {"IE_ATTN_SPLITS": str(splits)}, splits=splits)


@pytest.mark.parametrize("prec", PRECS)
def test_a_split_wholly_beyond_the_causal_limit(tmp_path, prec):
    """P = 40, Lq = 64 at 3 splits over 4 key tiles (2 per split: keys 0 - 63, 64 - 103, none): tokens 0 - 23 cannot see the second split and nobody has
    a key in the third; such records are (-FLT_MAX, 0, 0) and leave the combine with weight 0, not NaN"""
    _run(tmp_path, prec, 4, 2, 64, 40, 64, tile=EG.EXTEND_TILE, env={"IE_ATTN_SPLITS": "3"}, splits=3)


@pytest.mark.parametrize("prec", PRECS)
def test_two_requests_are_bit_equal_at_three_splits(tmp_path, prec):
    h, kvh, hd, past, lq = 4, 2, 64, 300, 8
    rows, feeds = EG.extend_feeds(N, h, kvh, hd, past, lq, valid=[3, past], max_pos=MAX_POS)
    path = models.write_repo(str(tmp_path), "rep", EG.extend_attn_graph(rows, N, h, kvh, hd, past, lq, max_pos=MAX_POS))
    outs = _outs(h, kvh, hd, past, lq)

    def go():
        m = B.CreateModel(path, "rep")
        try:
            res = []
            for _ in range(2):
                r = m.Infer([tensor(k, v) for k, v in feeds.items()], [B.OutputConfig(k, Shape=list(s), DataType="FLOAT32") for k, s in outs.items()])
                res.append({t.Name: t.Data.reshape(outs[t.Name]).copy() for t in r})
            return res, [p["kernel"] for p in B.Profile(m, 1)]
        finally:
            m.Destroy()
    (a, b), kern = with_env(dict(IE_AUTOTUNE="0", IE_PRECISION=prec, IE_ATTN_SPLITS="3"), go)
    assert EG.extend_label(EG.EXTEND_TILE, prec == "fp16", hd, 3) in kern, kern
    for k in outs:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("prec", PRECS)
def test_narrow_llama_prefill_extend_decode(tmp_path, prec):
    """prefill 5 tokens with present=True, a cache of capacity 12 from the engine's own outputs, extend by 4, rows 12-15 into the cache, one decode step,
    through ModelInfer: every call against the float64 walk of its graph on the same feeds, the last logits against the float64 prefill of all 10 tokens"""
    P, V, hkv, hd, LQ = KG.NARROW_P, KG.NARROW["vocab"], KG.NARROW["kv_heads"], KG.NARROW["dim"] // KG.NARROW["heads"], 4
    ids = np.random.RandomState(7).randint(0, V, (N, 10)).astype(np.int64)
    names = KG.present_names()
    graphs = {"pre": KG.narrow(seq=5, present=True), "ext": KG.narrow(seq=LQ, past=P), "dec": KG.narrow(seq=1, past=P)}
    paths = {k: models.write_repo(str(tmp_path), k, mb) for k, mb in graphs.items()}
    env = dict(IE_PRECISION=prec)

    def call(which, feeds, rows, lq):
        outs = dict({"logits": (N, lq, V)}, **{k: (N, hkv, rows, hd) for k in names})
        ys, _, kern = GG.run_outputs(paths[which], which, env, feeds, outs)
        want = ref64.run_f64(graphs[which], feeds)
        for k in outs:
            err = ref64.rel_err(ys[k], want[k])
            print(f"narrow llama {prec} {which} {k}: max err / max|ref| {err:.3e}")
            assert err < RTOL[prec], (which, k, err)
        return ys, kern

    pre, _ = call("pre", {"input_ids": ids[:, :5]}, 5, 5)
    cache = KG.cache_from({k: pre[k] for k in names}, (5, 5))
    feeds = dict({"input_ids": ids[:, 5:9].copy(), "attention_mask": EG.chunk_mask((5, 5), (LQ, LQ), P, LQ), "position_ids": np.tile(np.arange(5, 9, dtype=np.int64), (N, 1))}, **cache)
    ext, kern = call("ext", feeds, P + LQ, LQ)
    assert sum(EG.extend_label(EG.EXTEND_TILE, prec == "fp16", hd) in k for k in kern) == KG.NARROW["depth"], kern
    for k in names:              # the client's part: rows P .. P + Lq - 1 go into the cache at row `len`
        cache[k.replace("present", "past_key_values")][:, :, 5:9] = ext[k][:, :, P:]
    feeds = dict({"input_ids": ids[:, 9:10].copy(), "attention_mask": KG.cache_mask((9, 9)), "position_ids": np.full((N, 1), 9, np.int64)}, **cache)
    dec, _ = call("dec", feeds, P + 1, 1)
    full = ref64.run_f64(KG.narrow(seq=10), {"input_ids": ids})["logits"]
    err = ref64.rel_err(dec["logits"][:, 0], full[:, 9])
    print(f"narrow llama {prec}: the decode step behind the extend step against the float64 prefill of 10 tokens: {err:.3e}")
    assert err < RTOL[prec]


def test_position_out_of_range_is_an_error_and_nothing_runs(tmp_path):
    h, kvh, hd, past, lq = 4, 2, 32, 12, 4
    rows, feeds = EG.extend_feeds(N, h, kvh, hd, past, lq)
    mb = EG.extend_attn_graph(rows, N, h, kvh, hd, past, lq, max_pos=MAX_POS)
    path = models.write_repo(str(tmp_path), "oor", mb)
    outs = _outs(h, kvh, hd, past, lq)

    def go():
        m = B.CreateModel(path, "oor")
        try:
            pos = feeds["position_ids"].copy()
            pos[1, 2] = MAX_POS
            with pytest.raises(RuntimeError) as e:
                m.Infer([tensor(k, v) for k, v in dict(feeds, position_ids=pos).items()], [B.OutputConfig(k, Shape=list(s), DataType="FLOAT32") for k, s in outs.items()])
            assert "Index out of range for input: position_ids at position [1, 2]" in str(e.value) and "value 64" in str(e.value), str(e.value)
            r = m.Infer([tensor(k, v) for k, v in feeds.items()], [B.OutputConfig(k, Shape=list(s), DataType="FLOAT32") for k, s in outs.items()])
            return {t.Name: t.Data.reshape(outs[t.Name]).copy() for t in r}
        finally:
            m.Destroy()
    ys = with_env(dict(IE_AUTOTUNE="0", IE_PRECISION="fp32"), go)
    _check(ys, ref64.run_f64(mb, feeds), feeds, past, "fp32", "after the refused request")
