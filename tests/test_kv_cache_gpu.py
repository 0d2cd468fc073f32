"""GPU (-m gpu): the KV cache kernels against the float64 walk of the same graph on the same feeds (tests/ref64.py), with the project's bounds: fp32 within
2e-4 of max|ref|, fp16 within 3e-3.

The decode attention subgraph alone (kv_graphs.decode_attn_graph: input_ids pick q | k | v rows, the cache comes in as past_key_values.0.*): `out` and
both `present` outputs, on tile 0 (kv_append_kernel + attention_decode_generic_kernel) and tile 4 (attention_decode_kernel), fp32 and fp16, N = 2.
Every K / V head and every cache row is another draw, so a wrong head mapping or a wrong row shows by orders of magnitude.  Image 0 is valid in 3 cache
rows only (whole key tiles and whole splits of it are masked), image 1 in all.  `present` rows < P are compared with the `past` input bit for bit in
every case.  Then the prefill-with-present subgraph, the narrow Llama end to end (prefill, cache from the engine's own outputs, three greedy decode
steps) and an out-of-range position through ModelInfer."""
import numpy as np
import pytest

import gpt2_graphs as GG
import kv_graphs as KG
import ref64
from engine_run import plan_of, RTOL, tensor, with_env
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models

pytestmark = pytest.mark.gpu
N, H = 2, 4
PRECS = ("fp32", "fp16")


def _outs(kvh, hd, past):
    return {"out": (N, 1, H * hd), "present.0.key": (N, kvh, past + 1, hd), "present.0.value": (N, kvh, past + 1, hd)}


def _check(ys, ref, feeds, past, prec, what):
    for k in ("present.0.key", "present.0.value"):
        assert np.array_equal(ys[k][:, :, :past], feeds[k.replace("present", "past_key_values")]), (what, k, "rows < P are not the past, bit for bit")
    for k, y in ys.items():
        err = ref64.rel_err(y, ref[k])
        print(f"{what} {k}: max err / max|ref| {err:.3e}")
        assert np.isfinite(y).all() and err < RTOL[prec], (what, k, err)


def _run(tmp_path, prec, kvh, hd, past, *, tile, env=None, rope="input", tables=None, mask=True, valid=(3, None), positions=None, splits=None, name="dec", mask_value="min"):
    """one decode step of the subgraph under `env`, the plan's tile / splits and the launched kernel asserted, every output checked against float64"""
    valid = [past if v is None else min(v, past) for v in valid]
    positions = positions if positions is not None else [v for v in valid]      # (differing per image)
    rows, feeds = KG.decode_feeds(N, H, kvh, hd, past, valid=valid, positions=positions, mask=mask, rope=rope)
    mb = KG.decode_attn_graph(rows, N, H, kvh, hd, past, rope=rope, tables=tables, mask=mask, max_pos=max(64, past + 8), mask_value=mask_value)
    ref = ref64.run_f64(mb, feeds)
    path = models.write_repo(str(tmp_path), name, mb)
    e = dict(IE_PRECISION=prec, **(env or {}))
    (at,) = [s for s in plan_of(path, N, e)["steps"] if s["kind"] == "attention"]
    assert at["tile"] == tile and at["past_len"] == past and at.get("rope", False) is (rope is not None) and at.get("key_mask", False) is mask, at
    if splits is not None:
        assert at["splits"] == splits, at
    ys, shapes, kern = GG.run_outputs(path, name, e, feeds, _outs(kvh, hd, past))
    assert KG.decode_label(tile, prec == "fp16", hd, at.get("splits", 1)) in kern, kern
    assert shapes == {k: list(v) for k, v in _outs(kvh, hd, past).items()}
    _check(ys, ref, feeds, past, prec, f"decode H {H}/{kvh} hd {hd} P {past} {prec} tile {tile} S {at.get('splits', 1)} rope {rope} mask {mask}")
    return ys


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("tile", (0, 4))
@pytest.mark.parametrize("kvh", (4, 2, 1))
@pytest.mark.parametrize("hd", (32, 64, 128))
def test_heads_and_head_dims(tmp_path, hd, kvh, tile, prec):
    """(H, Hkv) = (4, 4), (4, 2), (4, 1) at every fast head dim, one key beyond a key tile, true rope tables at run-time positions that differ per image"""
    assert KG.fast_fits(hd, H, kvh, True)
    _run(tmp_path, prec, kvh, hd, KG.key_tile(hd) + 1, tile=tile, env={"IE_ATTN_TILE": str(tile)})


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("tile", (0, 4))
@pytest.mark.parametrize("past", (1, 15, 16, 17))
def test_cache_lengths_around_the_key_tile(tmp_path, past, tile, prec):
    """P = 1, the key tile - 1, the key tile, the key tile + 1 (hd 64: 16 keys), tables of independent random values in both halves of a row"""
    assert KG.key_tile(64) == 16
    _run(tmp_path, prec, 2, 64, past, tile=tile, env={"IE_ATTN_TILE": str(tile)}, tables=KG.LG.random_tables(64 + 16, 64))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kvh, hd", ((2, 64), (1, 128), (4, 32)))
@pytest.mark.parametrize("splits", (1, 3, None))
def test_long_cache_and_splits(tmp_path, splits, kvh, hd, prec):
    """P = 200 with IE_ATTN_SPLITS 1, 3 and the default: image 0 is valid in 3 rows, so at S = 3 two of its splits hold masked keys only and must leave the
    combine with weight 0; the default plan (no pin) runs attention_decode_kernel"""
    env = {} if splits is None else {"IE_ATTN_SPLITS": str(splits)}
    _run(tmp_path, prec, kvh, hd, 200, tile=4, env=env, splits=splits or KG.default_splits(N, kvh, 201, hd))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("tile", (0, 4))
@pytest.mark.parametrize("rope, mask", ((None, True), (None, False), ("const", True), ("const", False), ("input", False)))
def test_rope_and_mask_forms(tmp_path, rope, mask, tile, prec):
    """without rope, with constant positions (the one table row P) and with run-time ones; with and without the mask (no mask: every cache row is valid)"""
    _run(tmp_path, prec, 2, 32, 40, tile=tile, env={"IE_ATTN_TILE": str(tile)}, rope=rope, mask=mask, tables=KG.LG.random_tables(72, 32) if rope else None)


@pytest.mark.parametrize("prec", PRECS)
def test_generic_route(tmp_path, prec):
    """hd 48 fits no fast kernel: the default plan and a pinned tile 4 are both the generic pair; so is a mask constant of -10000"""
    assert not KG.fast_fits(48, H, 2)
    _run(tmp_path, prec, 2, 48, 21, tile=0)
    _run(tmp_path, prec, 2, 48, 21, tile=0, env={"IE_ATTN_TILE": "4"}, name="pin")
    _run(tmp_path, prec, 2, 64, 21, tile=0, mask_value=-10000.0, name="m1e4")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("tile, splits", ((0, None), (4, 1), (4, 3)))
def test_fully_masked_row(tmp_path, tile, splits, prec):
    """image 0's mask is 0 everywhere, the new key included: the graph gives the uniform average of V (every biased score rounds to finfo.min), and so do the
    kernels, finite"""
    kvh, hd, past = 2, 64, 70
    rows, feeds = KG.decode_feeds(N, H, kvh, hd, past, valid=[0, past], positions=[5, past])
    feeds["attention_mask"][0, :] = 0
    mb = KG.decode_attn_graph(rows, N, H, kvh, hd, past, max_pos=96)
    ref = ref64.run_f64(mb, feeds)
    assert np.allclose(ref["out"][0, 0, :hd], ref["present.0.value"][0, 0].mean(axis=0), rtol=0, atol=1e-12)
    path = models.write_repo(str(tmp_path), "fm", mb)
    env = dict(IE_PRECISION=prec, IE_ATTN_TILE=str(tile), **({"IE_ATTN_SPLITS": str(splits)} if splits else {}))
    ys, _, kern = GG.run_outputs(path, "fm", env, feeds, _outs(kvh, hd, past))
    assert KG.decode_label(tile, prec == "fp16", hd, splits or 1) in kern, kern
    _check(ys, ref, feeds, past, prec, f"fully masked row tile {tile} S {splits} {prec}")


@pytest.mark.parametrize("prec", PRECS)
def test_two_requests_are_bit_equal_at_three_splits(tmp_path, prec):
    kvh, hd, past = 2, 64, 200
    rows, feeds = KG.decode_feeds(N, H, kvh, hd, past, valid=[3, past], positions=[3, past])
    path = models.write_repo(str(tmp_path), "rep", KG.decode_attn_graph(rows, N, H, kvh, hd, past, max_pos=256))
    outs = _outs(kvh, hd, past)

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
    assert KG.decode_label(4, prec == "fp16", hd, 3) in kern, kern
    for k in outs:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("rope", ("init", None))
@pytest.mark.parametrize("l", (5, 40, 129))
def test_prefill_with_present(tmp_path, l, rope, prec):
    """present.key / present.value of a prefill against float64, and `y` bit-equal to the same graph without the two outputs (its attention step is untouched)"""
    kvh, hd = 2, 32
    x = KG.LG.gqa_input(N, l, H, kvh, hd)
    mb = KG.prefill_attn_graph(N, l, H, kvh, hd, rope=rope)
    ref = ref64.run_f64(mb, {"x": x})
    env = dict(IE_PRECISION=prec)
    path = models.write_repo(str(tmp_path), "pre", mb)
    kinds = [s["kind"] for s in plan_of(path, N, env)["steps"]]
    assert kinds.count("kv_append") == 1 and kinds.count("attention") == 1, kinds
    outs = {"y": (N, H * hd, 1, l), "present.0.key": (N, kvh, l, hd), "present.0.value": (N, kvh, l, hd)}
    ys, shapes, kern = GG.run_outputs(path, "pre", env, {"x": x}, outs)
    assert "kv_append_kernel<%s>" % ("f16" if prec == "fp16" else "f32") in kern, kern
    for k, y in ys.items():
        err = ref64.rel_err(y, ref[k])
        print(f"prefill L {l} rope {rope} {prec} {k}: max err / max|ref| {err:.3e}")
        assert np.isfinite(y).all() and err < RTOL[prec], (k, err)
    plain = models.write_repo(str(tmp_path), "plain", KG.prefill_attn_graph(N, l, H, kvh, hd, rope=rope, present=False))
    y0, _, _ = GG.run_outputs(plain, "plain", env, {"x": x}, {"y": outs["y"]})
    assert np.array_equal(y0["y"], ys["y"])


@pytest.mark.parametrize("prec", PRECS)
def test_narrow_llama_generates(tmp_path, prec):
    """prefill 5 tokens with present=True, a right-padded cache of capacity 12 from the engine's own outputs, three greedy decode steps through ModelInfer:
    every step's logits against the float64 walk of the decode graph on the same feeds, the last against the float64 prefill of all 8 tokens"""
    P, V, hkv, hd = KG.NARROW_P, KG.NARROW["vocab"], KG.NARROW["kv_heads"], KG.NARROW["dim"] // KG.NARROW["heads"]
    ids = np.random.RandomState(7).randint(0, V, (N, 5)).astype(np.int64)
    pre_mb, dec_mb = KG.narrow(seq=5, present=True), KG.narrow(seq=1, past=P)
    pre_path, dec_path = models.write_repo(str(tmp_path), "pre", pre_mb), models.write_repo(str(tmp_path), "dec", dec_mb)
    env = dict(IE_PRECISION=prec)
    names = KG.present_names()
    ys, _, _ = GG.run_outputs(pre_path, "pre", env, {"input_ids": ids}, dict({"logits": (N, 5, V)}, **{k: (N, hkv, 5, hd) for k in names}))
    ref = ref64.run_f64(pre_mb, {"input_ids": ids})
    for k in ["logits"] + names:
        assert ref64.rel_err(ys[k], ref[k]) < RTOL[prec], k
    cache = KG.cache_from({k: ys[k] for k in names}, (5, 5))
    seq = np.concatenate([ids, ys["logits"][:, -1].argmax(-1).reshape(N, 1)], axis=1)
    outs = dict({"logits": (N, 1, V)}, **{k: (N, hkv, P + 1, hd) for k in names})

    def go():
        nonlocal seq
        m = B.CreateModel(dec_path, "dec")
        try:
            for step in range(3):
                ln = 5 + step
                feeds = dict({"input_ids": seq[:, ln:ln + 1].copy(), "attention_mask": KG.cache_mask((ln, ln)), "position_ids": np.full((N, 1), ln, np.int64)}, **cache)
                r = m.Infer([tensor(k, v) for k, v in feeds.items()], [B.OutputConfig(k, Shape=list(s), DataType="FLOAT32") for k, s in outs.items()])
                got = {t.Name: t.Data.reshape(outs[t.Name]).copy() for t in r}
                want = ref64.run_f64(dec_mb, feeds)
                for k in outs:
                    err = ref64.rel_err(got[k], want[k])
                    print(f"narrow llama {prec} step {step} {k}: max err / max|ref| {err:.3e}")
                    assert err < RTOL[prec], (step, k, err)
                for k in names:          # the client's part: the new row goes into the cache at row `len`
                    cache[k.replace("present", "past_key_values")][:, :, ln] = got[k][:, :, P]
                seq = np.concatenate([seq, got["logits"][:, 0].argmax(-1).reshape(N, 1)], axis=1)
            kern = [p["kernel"] for p in B.Profile(m, 1)]
            return got["logits"], kern
        finally:
            m.Destroy()
    logits, kern = with_env(dict(IE_AUTOTUNE="0", **env), go)
    assert sum(KG.decode_label(4, prec == "fp16", hd) in k for k in kern) == KG.NARROW["depth"], kern
    full = ref64.run_f64(KG.narrow(seq=8), {"input_ids": seq[:, :8]})["logits"]
    err = ref64.rel_err(logits[:, 0], full[:, 7])
    print(f"narrow llama {prec}: the third decode step against the float64 prefill of 8 tokens: {err:.3e}")
    assert err < RTOL[prec]


def test_position_out_of_range_is_an_error_and_nothing_runs(tmp_path):
    kvh, hd, past = 2, 32, 12
    rows, feeds = KG.decode_feeds(N, H, kvh, hd, past)
    path = models.write_repo(str(tmp_path), "oor", KG.decode_attn_graph(rows, N, H, kvh, hd, past, max_pos=64))
    outs = _outs(kvh, hd, past)

    def go():
        m = B.CreateModel(path, "oor")
        try:
            bad = dict(feeds, position_ids=np.array([[3], [64]], np.int64))
            with pytest.raises(RuntimeError) as e:
                m.Infer([tensor(k, v) for k, v in bad.items()], [B.OutputConfig(k, Shape=list(s), DataType="FLOAT32") for k, s in outs.items()])
            assert "Index out of range for input: position_ids" in str(e.value) and "value 64" in str(e.value), str(e.value)
            r = m.Infer([tensor(k, v) for k, v in feeds.items()], [B.OutputConfig(k, Shape=list(s), DataType="FLOAT32") for k, s in outs.items()])
            return {t.Name: t.Data.reshape(outs[t.Name]).copy() for t in r}
        finally:
            m.Destroy()
    ys = with_env(dict(IE_AUTOTUNE="0", IE_PRECISION="fp32"), go)
    _check(ys, ref64.run_f64(KG.decode_attn_graph(rows, N, H, kvh, hd, past, max_pos=64), feeds), feeds, past, "fp32", "after the refused request")
