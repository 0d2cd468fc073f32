"""CPU: the KV cache through modelgen, the float64 walk and the planner (EngineDescribeModel).

The decode graph means what it should: a `present=True` prefill of 5 tokens in float64, its present.* copied into a cache of capacity 12 (right- and
left-padded, the two images with 5 and 3 valid rows), one `past=12` decode step with the matching mask and positions: logits and the new cache row equal
the float64 prefill of the 6- resp. 4-token sequence at its last position to 1e-10.  Then the plan of that model (one decode attention step per layer
that carries a kv_append part; the past inputs read in place; the present outputs dense; the whole rope tables in the blob), the prefill-with-present
plan (today's plan plus one kv_append step per layer), every refusal by its message, the tile and split switches, and what the half format alone costs
the narrow model of the GPU test."""
import numpy as np
import pytest

import kv_graphs as KG
import ref64
from engine_run import describe, RTOL
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models
from refusals import refused

N, P = KG.NARROW_N, KG.NARROW_P
D, H, HKV, V, DEPTH = KG.NARROW["dim"], KG.NARROW["heads"], KG.NARROW["kv_heads"], KG.NARROW["vocab"], KG.NARROW["depth"]
HD = D // H
IDS = np.random.RandomState(7).randint(0, V, (N, 8)).astype(np.int64)


def _plan(tmp_path, monkeypatch, mb, name="g", batch=N, prec="fp32", **env):
    return describe(models.write_repo(str(tmp_path), name, mb), batch, monkeypatch, prec, **env)


def _refused(tmp_path, monkeypatch, mb, *matches, batch=N, prec="fp32"):
    """the load is refused, and the text holds every one of `matches` (the node and the rule)"""
    refused(mb, batch, monkeypatch, *matches, prec=prec)


def test_switches_off_leave_the_graphs_alone():
    """the bytes of the graphs written before the switches existed: the defaults are the old call"""
    assert models.llama_tiny(N) == models.llama_tiny(N, present=False, past=None)
    assert KG.narrow(seq=5) != KG.narrow(seq=5, present=True)


@pytest.mark.parametrize("left", (False, True))
def test_decode_graph_is_the_prefill_of_the_longer_sequence(left):
    lengths = (5, 3)
    pre = ref64.run_f64(KG.narrow(seq=5, present=True), {"input_ids": IDS[:, :5]})
    assert pre["present.0.key"].shape == (N, HKV, 5, HD)
    feeds = {"input_ids": np.stack([IDS[i, ln:ln + 1] for i, ln in enumerate(lengths)]), "attention_mask": KG.cache_mask(lengths, left=left),
             "position_ids": np.array(lengths, np.int64).reshape(N, 1)}
    feeds.update(KG.cache_from({k: pre[k] for k in KG.present_names()}, lengths, left=left, dtype=np.float64))      # (float64 rows: the walk is exact)
    dec = ref64.run_f64(KG.narrow(seq=1, past=P), feeds)
    for i, ln in enumerate(lengths):
        full = ref64.run_f64(KG.narrow(1, seq=ln + 1, present=True), {"input_ids": IDS[i:i + 1, :ln + 1]})
        assert np.abs(dec["logits"][i, 0] - full["logits"][0, ln]).max() < 1e-10 * np.abs(full["logits"]).max()
        for k in KG.present_names():
            assert dec[k].shape == (N, HKV, P + 1, HD)
            assert np.abs(dec[k][i, :, P] - full[k][0, :, ln]).max() < 1e-10


@pytest.mark.parametrize("prec", ("fp32", "fp16"))
def test_decode_plan(tmp_path, monkeypatch, prec, engine_lib):
    path = models.write_repo(str(tmp_path), "dec", KG.narrow(seq=1, past=P))
    p = describe(path, N, monkeypatch, prec)
    layer = ["layer_norm", "conv", "attention", "conv", "layer_norm", "conv", "conv", "eltwise", "conv"]
    assert [s["kind"] for s in p["steps"]] == ["embed"] + DEPTH * layer + ["layer_norm", "conv"]      # no staging copy of a past input, no copy to an output
    ins = {i["name"]: i for i in p["inputs"]}
    outs = {o["name"]: o for o in p["outputs"]}
    assert [o["dims"] for o in p["outputs"]] == [[N, 1, V]] + 2 * DEPTH * [[N, HKV, P + 1, HD]]
    ats = [s for s in p["steps"] if s["kind"] == "attention"]
    offs = set()
    for li, at in enumerate(ats):
        assert (at["past_len"], at["kv_heads"], at["rope"], at["key_mask"], at["heads"], at["head_dim"]) == (P, HKV, True, True, H, HD)
        assert at["tile"] == KG.DECODE_TILE and at["splits"] == KG.default_splits(N, HKV, P + 1, HD) == 1 and at["rope_rows"] == KG.NARROW["max_pos"]
        assert "causal" not in at and at["in"]["w"] == 1 and at["in"]["c"] == (H + 2 * HKV) * HD
        # the past inputs are read in place, the present outputs written dense, both fp32 in [N][Hkv][rows][hd] order
        for which, name in (("k", "key"), ("v", "value")):
            assert at["past_" + which] == ins[f"past_key_values.{li}.{name}"]["view"] and at["past_" + which]["nchw"] is True and at["past_" + which]["f16"] is False
            assert at["present_" + which] == outs[f"present.{li}.{name}"]["view"] and at["present_" + which]["nchw"] is True and at["present_" + which]["f16"] is False
        assert at["positions"] == ins["position_ids"]["view"] and at["in2"] == ins["attention_mask"]["view"]
        kv, inner = at["parts"]
        assert kv["kind"] == "kv_append" and inner["kind"] == "attention" and inner["tile"] == 0 and "parts" not in inner and "splits" not in inner
        assert kv["past_len"] == P and kv["present_k"] == at["present_k"] and kv["present_v"] == at["present_v"] and kv["past_k"] == at["past_k"] and kv["positions"] == at["positions"]
        offs.add((at["w_off"], at["w2_off"], kv["w_off"], kv["w2_off"]))
    # the whole [max_pos, hd] tables ride in the blob, once for all layers
    (off,) = offs
    assert off[0] == off[2] and off[1] == off[3]
    blob = B.PlanWeights(path, N)
    cos, sin = models.rope_tables(KG.NARROW["max_pos"], HD)
    assert np.array_equal(blob[off[0]:off[0] + cos.size].reshape(cos.shape), cos) and np.array_equal(blob[off[1]:off[1] + sin.size].reshape(sin.shape), sin)


@pytest.mark.parametrize("prec", ("fp32", "fp16"))
def test_prefill_with_present_is_todays_plan_plus_a_kv_append_step_per_layer(tmp_path, monkeypatch, prec, engine_lib):
    base = _plan(tmp_path, monkeypatch, KG.narrow(seq=40), name="base", prec=prec)
    pres = _plan(tmp_path, monkeypatch, KG.narrow(seq=40, present=True), name="pres", prec=prec)
    kinds = [s["kind"] for s in pres["steps"]]
    assert kinds.count("kv_append") == DEPTH and [k for k in kinds if k != "kv_append"] == [s["kind"] for s in base["steps"]]
    a0 = [s for s in base["steps"] if s["kind"] == "attention"]
    a1 = [s for s in pres["steps"] if s["kind"] == "attention"]
    for x, y in zip(a0, a1):
        assert (x["tile"], x["causal"], x["rope"], x["kv_heads"]) == (y["tile"], y["causal"], y["rope"], y["kv_heads"]) and y["tile"] == 1 and "past_len" not in y and "parts" not in y
    outs = {o["name"]: o for o in pres["outputs"]}
    for li, kv in enumerate(s for s in pres["steps"] if s["kind"] == "kv_append"):
        assert "past_len" not in kv and "past_k" not in kv and kv["rope"] is True and kv["rope_rows"] == 40 and kv["kv_heads"] == HKV
        assert kv["present_k"] == outs[f"present.{li}.key"]["view"] and kv["present_v"] == outs[f"present.{li}.value"]["view"]
        assert outs[f"present.{li}.key"]["dims"] == [N, HKV, 40, HD] and kv["present_k"]["nchw"] is True and kv["present_k"]["f16"] is False


def _dec(past=12, hd=32, kvh=2, **kw):
    rows, _ = KG.decode_feeds(N, H, kvh, hd, past)
    return KG.decode_attn_graph(rows, N, H, kvh, hd, past, **kw)


def test_refusals(tmp_path, monkeypatch, engine_lib):
    r = lambda mb, *m: _refused(tmp_path, monkeypatch, mb, *m)  # noqa: E731
    r(_dec(lq=2, rope=None), "Lq = 2", "chunked prefill into a cache", "Lq = 1")
    r(_dec(past_k_dims=[N, 3, 12, 32]), "past_key_values.0.key is [2, 3, 12, 32], not [N, Hkv, P, hd] = [2, 2, P, 32]")
    r(_dec(past_k_dims=[N, 2, 12, 16]), "past_key_values.0.key is [2, 2, 12, 16], not [N, Hkv, P, hd]")
    r(_dec(past_v_rows=11), "the K and V pasts differ in their rows P", "past_key_values.0.value is [2, 2, 11, 32]")
    r(_dec(concat_order="new_first"), "the cache of k (Concat", "in the order (k, past)", "supported: Concat(past, k, axis 2)")
    r(_dec(extra_reader=True), "the past input past_key_values.0.key has 2 readers, not 1", "read by this Concat alone")
    r(_dec(present_after_repeat=True), "repeat_kv of k", "the graph output present.0.key is the value behind repeat_kv", "[N, Hkv, rows, hd]")
    r(_dec(pos_dims=[N, 2]), "the position ids position_ids of the rope table are neither a constant nor an INT64 graph input [N, 1]")
    r(_dec(k_positions=True), "the positions of k (", "position_ids_k", "are not the positions of q (", "position_ids)")
    r(_dec(mask_width=12), "the key mask attention_mask is [2, 12]; its width must be P + 1 = 13")
    r(KG.gpt2_decode_attn_graph(N, H, 32, 12), "behind the Split of one qkv Linear (GPT-2's spelling) is not supported")
    # rope together with a key mask stays refused in the prefill form, and fp8 refuses these graphs as it refuses Llama
    path = models.write_repo(str(tmp_path), "f8", KG.narrow(seq=1, past=P))
    refused(path, N, monkeypatch, prec="fp8")


def test_tile_and_split_switches_show_in_the_plan(tmp_path, monkeypatch, engine_lib):
    at = lambda p: [s for s in p["steps"] if s["kind"] == "attention"][0]  # noqa: E731
    mb = _dec(past=200, hd=64)
    a = at(_plan(tmp_path, monkeypatch, mb))
    assert a["tile"] == KG.DECODE_TILE and a["splits"] == KG.default_splits(N, 2, 201, 64) == 1
    assert at(_plan(tmp_path, monkeypatch, mb, IE_ATTN_SPLITS="3"))["splits"] == 3
    assert at(_plan(tmp_path, monkeypatch, mb, IE_ATTN_SPLITS="1000"))["splits"] == -(-201 // KG.key_tile(64))      # (at most one key tile per split)
    a = at(_plan(tmp_path, monkeypatch, mb, IE_ATTN_TILE="0"))
    assert a["tile"] == 0 and "splits" not in a and [q["kind"] for q in a["parts"]] == ["kv_append", "attention"]
    assert at(_plan(tmp_path, monkeypatch, mb, IE_ATTN_TILE="4"))["tile"] == KG.DECODE_TILE
    # an ineligible pin is the generic route: hd 48, and a mask constant an fp32 sum keeps a score beside
    for bad in (_dec(past=20, hd=48), _dec(past=20, hd=64, mask_value=-10000.0)):
        for env in ({}, {"IE_ATTN_TILE": "4"}):
            a = at(_plan(tmp_path, monkeypatch, bad, **env))
            assert a["tile"] == 0 and "splits" not in a
    assert not KG.fast_fits(48, H, 2) and not KG.fast_fits(64, H, 2, True, -10000.0) and KG.fast_fits(64, H, 2, True)
    # a long cache of few heads is split to fill the device
    assert KG.default_splits(1, 8, 4096, 128) == 32 and KG.default_splits(8, 3, 1024, 64) == 8 and KG.default_splits(8, 8, 1024, 128) == 8


def test_fp16_headroom():
    """the GPU test's narrow model on its inputs with random tables: what the half format alone costs stays under half of the fp16 bound"""
    pre = ref64.run_f64(KG.narrow(seq=5, present=True), {"input_ids": IDS[:, :5]})
    feeds = {"input_ids": IDS[:, 5:6], "attention_mask": KG.cache_mask((5, 5)), "position_ids": np.full((N, 1), 5, np.int64)}
    feeds.update(KG.cache_from({k: pre[k].astype(np.float32) for k in KG.present_names()}, (5, 5)))
    mb = KG.narrow(seq=1, past=P)
    ref, half = ref64.run_f64(mb, feeds), ref64.run_f64(mb, feeds, round_half=True)
    for k in ["logits"] + KG.present_names():
        err = ref64.rel_err(half[k], ref[k])
        print(f"{k}: half storage alone {err:.3e} of max|ref|")
        assert err < RTOL["fp16"] / 2, (k, err)
    half = ref64.run_f64(KG.narrow(seq=5, present=True), {"input_ids": IDS[:, :5]}, round_half=True)
    for k in ["logits"] + KG.present_names():
        assert ref64.rel_err(half[k], pre[k]) < RTOL["fp16"] / 2, k
