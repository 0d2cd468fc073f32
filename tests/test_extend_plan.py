"""CPU: extend steps (a past of P rows and Lq >= 2 new tokens: chunked prefill into a cache) through modelgen, the float64 walk and the planner.

The extend graph means what it should: a `present=True` prefill of 5 tokens in float64, its present.* copied into a cache of capacity 12 (right- and
left-padded), one `seq=4, past=12` extend step, its rows 12-15 copied into the cache, one decode step: logits and cache rows equal the float64 prefill
of all 10 tokens to 1e-10; then a ragged batch (5 + 4 and 3 + 2 tokens, the chunk right-padded).  Then the plan of that model (one attention step per
layer with past_len, new_len, key_mask, chunk_causal, rope and the expected tile and splits), the tile and split switches, the digests a build of the
parent commit gave for the graphs that loaded before, every refusal by its message, and what the half format alone costs the narrow model on the GPU
test's inputs."""
import itertools
import json
import os

import numpy as np
import pytest

import extend_graphs as EG
import kv_graphs as KG
import ref64
import test_plan_digests as TPD
from engine_run import describe, RTOL
from gpu_ai_inference_server_amd.modelgen import models
from refusals import refused

N, P, LQ = KG.NARROW_N, KG.NARROW_P, 4
D, H, HKV, V, DEPTH = KG.NARROW["dim"], KG.NARROW["heads"], KG.NARROW["kv_heads"], KG.NARROW["vocab"], KG.NARROW["depth"]
HD = D // H
IDS = np.random.RandomState(7).randint(0, V, (N, 10)).astype(np.int64)      # (its first 5 columns are test_kv_cache_*'s prompt)


def _plan(tmp_path, monkeypatch, mb, name="g", batch=N, prec="fp32", **env):
    return describe(models.write_repo(str(tmp_path), name, mb), batch, monkeypatch, prec, **env)


def _refused(tmp_path, monkeypatch, mb, *matches, batch=N, prec="fp32"):
    """the load is refused, and the text holds every one of `matches` (the node and the rule)"""
    refused(mb, batch, monkeypatch, *matches, prec=prec)


def test_seq_1_builds_the_decode_graph_and_seq_2_needs_its_inputs():
    assert KG.narrow(seq=1, past=P) != KG.narrow(seq=2, past=P)
    for kw in (dict(mask=None), dict(positions="const"), dict(rope="none")):
        with pytest.raises(ValueError):
            KG.narrow(seq=2, past=P, **kw)


def test_chunk_causal_constant():
    """0 in the first P columns; in column P + j of row i 0 for j <= i and finfo.min for j > i; never -inf"""
    mb = EG.extend_attn_graph(np.zeros((7, 4 * 32), np.float32), 1, 2, 1, 32, 5, 3)
    c = ref64.O.load_model(mb).inits["chunk_mask"]
    assert c.shape == (1, 1, 3, 8) and c.dtype == np.float32 and np.isfinite(c).all()
    for i, j in itertools.product(range(3), range(8)):
        assert c[0, 0, i, j] == (0.0 if j <= 5 + i else models.FLOAT32_MIN), (i, j)


@pytest.mark.parametrize("left", (False, True))
def test_extend_graph_is_the_prefill_of_the_longer_sequence(left):
    pre = ref64.run_f64(KG.narrow(seq=5, present=True), {"input_ids": IDS[:, :5]})
    names = KG.present_names()
    feeds = {"input_ids": IDS[:, 5:9], "attention_mask": EG.chunk_mask((5, 5), (LQ, LQ), P, LQ, left), "position_ids": np.tile(np.arange(5, 9, dtype=np.int64), (N, 1))}
    feeds.update(KG.cache_from({k: pre[k] for k in names}, (5, 5), left=left, dtype=np.float64))      # (float64 rows: the walk is exact)
    ext = ref64.run_f64(KG.narrow(seq=LQ, past=P), feeds)
    assert ext["logits"].shape == (N, LQ, V) and ext[names[0]].shape == (N, HKV, P + LQ, HD)
    # the client's part: rows P .. P + Lq - 1 go into the cache behind its 5 rows; then one decode step on the 9 rows
    rows9 = {k: np.concatenate([pre[k], ext[k][:, :, P:]], axis=2) for k in names}
    dfeeds = {"input_ids": IDS[:, 9:10], "attention_mask": KG.cache_mask((9, 9), left=left), "position_ids": np.full((N, 1), 9, np.int64)}
    dfeeds.update(KG.cache_from(rows9, (9, 9), left=left, dtype=np.float64))
    dec = ref64.run_f64(KG.narrow(seq=1, past=P), dfeeds)
    full = ref64.run_f64(KG.narrow(seq=10, present=True), {"input_ids": IDS})
    scale = np.abs(full["logits"]).max()
    assert np.abs(ext["logits"] - full["logits"][:, 5:9]).max() < 1e-10 * scale
    assert np.abs(dec["logits"][:, 0] - full["logits"][:, 9]).max() < 1e-10 * scale
    for k in names:
        assert np.abs(ext[k][:, :, P:] - full[k][:, :, 5:9]).max() < 1e-10 and np.abs(dec[k][:, :, P] - full[k][:, :, 9]).max() < 1e-10


def test_ragged_chunk():
    """image 0 has 5 + 4 tokens, image 1 has 3 + 2 with its chunk right-padded and its own mask columns 0: the rows whose own key is valid are the
    prefill's; the others (2 of the 8) are finite"""
    lengths, news = (5, 3), (4, 2)
    pre = ref64.run_f64(KG.narrow(seq=5, present=True), {"input_ids": IDS[:, :5]})
    names = KG.present_names()
    feeds = {"input_ids": np.stack([IDS[i, ln:ln + LQ] for i, ln in enumerate(lengths)]), "attention_mask": EG.chunk_mask(lengths, news, P, LQ),
             "position_ids": np.stack([np.arange(ln, ln + LQ, dtype=np.int64) for ln in lengths])}
    feeds.update(KG.cache_from({k: pre[k] for k in names}, lengths, dtype=np.float64))
    ext = ref64.run_f64(KG.narrow(seq=LQ, past=P), feeds)
    own = EG.own_key_valid(feeds, P)
    assert own.size - own.sum() == 2 and np.isfinite(ext["logits"]).all()
    for i, (ln, nw) in enumerate(zip(lengths, news)):
        full = ref64.run_f64(KG.narrow(1, seq=ln + nw, present=True), {"input_ids": IDS[i:i + 1, :ln + nw]})
        assert np.abs(ext["logits"][i, :nw] - full["logits"][0, ln:]).max() < 1e-10 * np.abs(full["logits"]).max()
        for k in names:
            assert np.abs(ext[k][i, :, P:P + nw] - full[k][0, :, ln:]).max() < 1e-10


@pytest.mark.parametrize("prec", ("fp32", "fp16"))
def test_extend_plan(tmp_path, monkeypatch, prec, engine_lib):
    """narrow(seq=4, past=12) loads (the parent refused it by name)"""
    p = _plan(tmp_path, monkeypatch, KG.narrow(seq=LQ, past=P), prec=prec)
    layer = ["layer_norm", "conv", "attention", "conv", "layer_norm", "conv", "conv", "eltwise", "conv"]
    assert [s["kind"] for s in p["steps"]] == ["embed"] + DEPTH * layer + ["layer_norm", "conv"]      # the Where and the Cast import nothing
    ins = {i["name"]: i for i in p["inputs"]}
    outs = {o["name"]: o for o in p["outputs"]}
    assert ins["attention_mask"]["dims"] == [N, P + LQ] and ins["position_ids"]["dims"] == [N, LQ]
    assert [o["dims"] for o in p["outputs"]] == [[N, LQ, V]] + 2 * DEPTH * [[N, HKV, P + LQ, HD]]
    ats = [s for s in p["steps"] if s["kind"] == "attention"]
    assert len(ats) == DEPTH
    for li, at in enumerate(ats):
        assert (at["past_len"], at["new_len"], at["key_mask"], at["chunk_causal"], at["rope"], at["kv_heads"], at["heads"], at["head_dim"]) == (P, LQ, True, True, True, HKV, H, HD)
        assert at["tile"] == EG.EXTEND_TILE and at["splits"] == EG.default_splits(N, HKV, (H // HKV) * LQ, P + LQ) == 1 and "causal" not in at and at["mask_value"] == pytest.approx(models.FLOAT32_MIN) and at["rope_rows"] == KG.NARROW["max_pos"]
        assert at["in"]["w"] == LQ and at["positions"] == ins["position_ids"]["view"] and at["in2"] == ins["attention_mask"]["view"]
        for which, name in (("k", "key"), ("v", "value")):
            assert at["past_" + which] == ins[f"past_key_values.{li}.{name}"]["view"] and at["present_" + which] == outs[f"present.{li}.{name}"]["view"]
        kv, inner = at["parts"]
        assert kv["kind"] == "kv_append" and kv["past_len"] == P and kv["new_len"] == LQ and kv["positions"] == at["positions"] and kv["present_k"] == at["present_k"]
        assert inner["kind"] == "attention" and inner["tile"] == 0 and inner["chunk_causal"] is True and "parts" not in inner
    for at in (s for s in _plan(tmp_path, monkeypatch, KG.narrow(seq=LQ, past=P), prec=prec, IE_ATTN_TILE="0")["steps"] if s["kind"] == "attention"):
        assert at["tile"] == 0 and "splits" not in at and [q["kind"] for q in at["parts"]] == ["kv_append", "attention"]


def _ext(past=12, lq=LQ, hd=32, kvh=2, **kw):
    rows, _ = EG.extend_feeds(N, H, kvh, hd, past, lq)
    return EG.extend_attn_graph(rows, N, H, kvh, hd, past, lq, **kw)


def test_subgraph_plans(tmp_path, monkeypatch, engine_lib):
    at = lambda p: [s for s in p["steps"] if s["kind"] == "attention"][0]  # noqa: E731
    for hd, rope in ((32, "input"), (64, None)):
        a = at(_plan(tmp_path, monkeypatch, _ext(hd=hd, rope=rope)))
        assert (a["tile"], a["past_len"], a["new_len"], a["chunk_causal"], a["key_mask"], a.get("rope", False), a["head_dim"]) == (EG.EXTEND_TILE, 12, LQ, True, True, rope is not None, hd)
    # tile 5 is the default from kAttnExtendMinRows query rows on, which is the fewest there are: g = 1, Lq = 2
    assert EG.MIN_ROWS == 2 and at(_plan(tmp_path, monkeypatch, _ext(lq=2, kvh=4)))["tile"] == EG.EXTEND_TILE
    # the tile and split switches: a long cache of few workgroups is split; a pin shows in the plan and is capped at one 32-key tile per split
    mb = _ext(past=300, lq=8, hd=64)
    a = at(_plan(tmp_path, monkeypatch, mb))
    assert a["tile"] == EG.EXTEND_TILE and a["splits"] == EG.default_splits(N, 2, 2 * 8, 308) == 2
    assert at(_plan(tmp_path, monkeypatch, mb, IE_ATTN_SPLITS="3"))["splits"] == 3
    assert at(_plan(tmp_path, monkeypatch, mb, IE_ATTN_SPLITS="1000"))["splits"] == -(-308 // 32)
    a = at(_plan(tmp_path, monkeypatch, mb, IE_ATTN_TILE="0"))
    assert a["tile"] == 0 and "splits" not in a and [q["kind"] for q in a["parts"]] == ["kv_append", "attention"]
    assert at(_plan(tmp_path, monkeypatch, mb, IE_ATTN_TILE="5"))["tile"] == EG.EXTEND_TILE
    assert at(_plan(tmp_path, monkeypatch, mb, IE_ATTN_TILE="4"))["tile"] == EG.EXTEND_TILE      # (a decode step's tile is no pin of an extend step)
    # an ineligible pin is the generic pair: hd 48 and hd 128 (wide heads are the follow-up)
    for hd in (48, 128):
        for env in ({}, {"IE_ATTN_TILE": "5"}):
            a = at(_plan(tmp_path, monkeypatch, _ext(past=20, hd=hd), **env))
            assert a["tile"] == 0 and "splits" not in a and a["chunk_causal"] is True
    assert not EG.fast_fits(48, H, 2) and not EG.fast_fits(128, H, 2) and not EG.fast_fits(64, H, 2, -10000.0) and EG.fast_fits(64, H, 2)
    assert EG.default_splits(1, 3, 3 * 8, 4103) == 32 and EG.default_splits(8, 3, 3 * 128, 1151) == 4
    # one new token behind the same mask (C is a row of zeros) is the decode step it always was
    a = at(_plan(tmp_path, monkeypatch, _ext(lq=1)))
    assert a["tile"] == KG.DECODE_TILE and a["past_len"] == 12 and "new_len" not in a and "chunk_causal" not in a and a["key_mask"] is True


def test_parent_plans_are_unchanged(tmp_path, monkeypatch, engine_lib):
    """tests/golden/extend_parent_plans.json: the plan and blob digests (test_plan_digests.digest's form) a build of the parent commit gave for the
    decode graph, the prefill with present outputs and llama_tiny: what loaded before plans exactly as it did"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "extend_parent_plans.json")) as f:
        parent = json.load(f)
    cases = {"narrow_decode": (lambda: KG.narrow(seq=1, past=P), N), "narrow_prefill_present": (lambda: KG.narrow(seq=5, present=True), N), "llama_tiny": (lambda: models.llama_tiny(2), 2)}
    assert sorted(parent) == sorted(f"{n}/{p}" for n, p in itertools.product(cases, ("fp32", "fp16")))
    for name, (mk, b) in cases.items():
        path = models.write_repo(str(tmp_path), name, mk())
        for prec in ("fp32", "fp16"):
            d = TPD.digest(path, b, {"IE_PRECISION": prec})
            assert " ".join(d[k] for k in ("plan", "weights") if k in d) == parent[f"{name}/{prec}"], (name, prec)


def test_refusals(tmp_path, monkeypatch, engine_lib):
    r = lambda mb, *m: _refused(tmp_path, monkeypatch, mb, *m)  # noqa: E731
    r(_ext(mask="add"), "is Add(ext, C) of a key mask and a constant", "finfo.min + finfo.min = -inf", "supported: Where(Cast(ext, to BOOL), finfo.min, C)")
    r(_ext(c_past=11), "the chunk mask Where", "its constant is [1, 1, 4, 15], not [1, 1, Lq, P + Lq] = [1, 1, 4, 16] of this step")
    r(_ext(c_edit=(1, 14, 0.0)), "its constant is not the chunk's causal mask (0 where j <= P + i, <= -1e30 above): element [1, 14] is 0.000000 at P = 12")
    r(_ext(c_edit=(2, 3, models.FLOAT32_MIN)), "its constant is not the chunk's causal mask", "element [2, 3] is -3402823")
    r(_ext(fill=-10000.0), "the value -10000.000000 of a masked key is above -1e30")
    r(_ext(with_past=False, rope=None), "the chunk mask Where", "a key mask and a causal constant in one value without a past (no Concat(past, k, axis 2)) is not supported")
    r(_ext(mask_width=15), "the key mask attention_mask is [2, 15]; its width must be P + Lq = 16 (the 12 cached rows and the 4 new keys)")
    r(_ext(pos_dims=[N, 1]), "the position ids position_ids of the rope table are [2, 1]", "takes an INT64 graph input [N, Lq] = [2, 4], every token's own table row")
    r(_ext(pos_dims=[N, 5]), "the position ids position_ids of the rope table are [2, 5]", "[N, Lq] = [2, 4]")
    for mask, what in (("key", "a key mask alone"), (None, "no mask")):
        r(_ext(mask=mask, lq=2), "with Lq = 2 new tokens (chunked prefill into a cache) needs the chunk's causal mask", what + ": the new tokens would see each other's future", "Lq = 1")
    # the refusals of graphs that were refused before keep their words
    rows, _ = KG.decode_feeds(N, H, 2, 32, 12)
    r(KG.decode_attn_graph(rows, N, H, 2, 32, 12, lq=2, rope=None), "Lq = 2", "chunked prefill into a cache", "Lq = 1")
    r(KG.decode_attn_graph(rows, N, H, 2, 32, 12, pos_dims=[N, 2]), "the position ids position_ids of the rope table are neither a constant nor an INT64 graph input [N, 1]")
    r(KG.decode_attn_graph(rows, N, H, 2, 32, 12, mask_width=12), "the key mask attention_mask is [2, 12]; its width must be P + 1 = 13")
    # fp8 refuses the graph as it refuses Llama
    path = models.write_repo(str(tmp_path), "f8", KG.narrow(seq=LQ, past=P))
    refused(path, N, monkeypatch, prec="fp8")


def test_fp16_headroom():
    """the GPU test's narrow model on its inputs (the cache from the prefill's fp32 rows, the extend step, the decode step behind it): what the half
    format alone costs stays under half of the fp16 bound"""
    names = KG.present_names()
    pre = ref64.run_f64(KG.narrow(seq=5, present=True), {"input_ids": IDS[:, :5]})
    feeds = {"input_ids": IDS[:, 5:9], "attention_mask": EG.chunk_mask((5, 5), (LQ, LQ), P, LQ), "position_ids": np.tile(np.arange(5, 9, dtype=np.int64), (N, 1))}
    feeds.update(KG.cache_from({k: pre[k].astype(np.float32) for k in names}, (5, 5)))
    mb = KG.narrow(seq=LQ, past=P)
    ref, half = ref64.run_f64(mb, feeds), ref64.run_f64(mb, feeds, round_half=True)
    for k in ["logits"] + names:
        err = ref64.rel_err(half[k], ref[k])
        print(f"extend {k}: half storage alone {err:.3e} of max|ref|")
        assert err < RTOL["fp16"] / 2, (k, err)
    rows9 = {k: np.concatenate([pre[k], ref[k][:, :, P:]], axis=2).astype(np.float32) for k in names}
    dfeeds = {"input_ids": IDS[:, 9:10], "attention_mask": KG.cache_mask((9, 9)), "position_ids": np.full((N, 1), 9, np.int64)}
    dfeeds.update(KG.cache_from(rows9, (9, 9)))
    mb = KG.narrow(seq=1, past=P)
    ref, half = ref64.run_f64(mb, dfeeds), ref64.run_f64(mb, dfeeds, round_half=True)
    for k in ["logits"] + names:
        assert ref64.rel_err(half[k], ref[k]) < RTOL["fp16"] / 2, k
