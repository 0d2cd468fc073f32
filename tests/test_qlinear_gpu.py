"""GPU: the 4-bit Linear kernels (kernels_qlinear.hip) element by element against float64 on the dense twin's weights, and an int4 Llama through prefill,
decode and extend, unbound and bound to a resident cache, against the float64 walk of its dense twin.

The bounds, with S = sum_k |x_k| |w_k| (+ |r| where a residual r is added: it enters like one more product, r * 1) and ref in float64:
  fp32   |y - ref| <= (K + 1) 2^-24 S                               every term passes at most K + 1 fp32 roundings; the weights (q - z) * s are the twin's own
  fp16   |y - ref| <= (2^-10 + 2^-22 + K 2^-24) S + 2^-11 |ref|     x and w each rounded once to half, fp32 accumulation, the result rounded once
Every term is a worst case; no element is exempt.  The cases cover every value the kernels branch on -- rows 1 / 8 / 16 / 17 / 70 (one row, a decode batch,
a full MFMA tile, one over it, past a 64-row block), K 128 / 576 (one k-step; a tail that is a multiple of 32 only), N 80 / 960 (an odd count of
16-column tiles; llama_135m's merged qkv), blocks 32 / 64 / 128, with and without zero points and residual -- as a covering set, not the full product.
Codes and zero points are uniform over 0..15 and the scales vary fourfold from block to block, so a swapped nibble, a scale one block off or a
dropped zero point misses the bound by orders of magnitude."""
import numpy as np
import pytest

import kv_graphs as KG
import resident_graphs as RG
import test_resident_cache_gpu as TRC
from engine_run import run_model
from gpu_ai_inference_server_amd.modelgen import models

#        rows, K,  N,  block, zero points, residual
CASES = [(1, 128, 80, 32, True, False), (8, 128, 80, 128, False, True), (8, 576, 960, 32, True, True), (16, 576, 80, 64, False, False),
         (17, 576, 960, 64, True, False), (70, 576, 80, 32, False, True), (70, 128, 960, 64, True, True), (16, 128, 960, 128, True, False),
         (1, 576, 960, 32, False, True), (17, 128, 80, 32, True, True)]
_cache = {}


def _codes(zero):
    def draw(name, cout, nblk, block):
        r = np.random.RandomState(cout + 7 * nblk + block)
        q = r.randint(0, 16, (cout, nblk, block)).astype(np.uint8)
        z = r.randint(0, 16, (cout, nblk)).astype(np.uint8) if zero else np.full((cout, nblk), 8, np.uint8)
        s = (np.float32(0.01) * np.exp2(r.uniform(0.0, 2.0, (cout, nblk)))).astype(np.float32)
        return q, z, s
    return draw


def _case(case):
    """(feeds, ref, S, the nbits model) of a case, computed once: ref and S in float64 from the float32 weights (q - z) * s of the dense twin"""
    if case not in _cache:
        rows, k, n, block, zero, res = case
        q, z, s = _codes(zero)("fc", n, k // block, block)
        w = ((q.astype(np.float32) - z[:, :, None].astype(np.float32)) * s[:, :, None]).reshape(n, k).astype(np.float64)
        r = np.random.RandomState(rows + k + n)
        feeds = {"x": r.randn(rows, k).astype(np.float32)}
        if res:
            feeds["r"] = r.randn(rows, n).astype(np.float32)
        x = feeds["x"].astype(np.float64)
        ref = x @ w.T + (feeds["r"].astype(np.float64) if res else 0.0)
        S = np.abs(x) @ np.abs(w).T + (np.abs(feeds["r"].astype(np.float64)) if res else 0.0)
        mb = models.qlinear(rows, k, n, q_block=block, q_zero=zero, residual=res, q_codes=_codes(zero))
        _cache[case] = (feeds, ref, S, mb, w)
    return _cache[case]


def _bound(prec, k, S, ref):
    return (k + 1) * 2.0 ** -24 * S if prec == "fp32" else (2.0 ** -10 + 2.0 ** -22 + k * 2.0 ** -24) * S + 2.0 ** -11 * np.abs(ref)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_float32_twin_is_inside_the_fp32_bound(case):
    feeds, ref, S, _, w = _case(case)
    y = feeds["x"] @ w.astype(np.float32).T + (feeds["r"] if "r" in feeds else np.float32(0))
    assert (np.abs(y - ref) <= _bound("fp32", case[1], S, ref)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ("fp32", "fp16"))
@pytest.mark.parametrize("case", CASES, ids=str)
def test_linear_alone(tmp_path, case, prec):
    rows, k, n, block, zero, res = case
    feeds, ref, S, mb, _ = _case(case)
    path = models.write_repo(str(tmp_path), "q", mb)
    form = "b%d,%s>" % (block, "zp" if zero else "sym")
    want = {"fp32": "qlinear_generic_kernel<f32," + form, "fp16": "qlinear_mfma_kernel<" + form}[prec]      # (every case is eligible for tile 1 in fp16)
    runs = [(want, {})] + ([("qlinear_generic_kernel<f16," + form, {"IE_QLINEAR_TILE": "0"})] if prec == "fp16" else [])
    for label, env in runs:
        (y, again), kern = run_model(path, "q", dict(IE_PRECISION=prec, **env), [feeds, feeds], "y", (rows, n))
        assert label in kern, (label, kern)
        excess = np.abs(y - ref) / _bound(prec, k, S, ref)
        print(f"{case} {prec} {label}: max |y - ref| / bound {excess.max():.3f}")
        assert np.isfinite(y).all() and (excess <= 1.0).all(), (label, float(excess.max()))
        assert (RG.bits(y) == RG.bits(again)).all(), label + ": two runs differ"


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ("fp32", "fp16"))
def test_int4_llama_unbound(tmp_path, prec):
    """prefill with present, then one decode step and one extend step on the prefill's cache, the client holding it"""
    n, p, v = KG.NARROW_N, KG.NARROW_P, KG.NARROW["vocab"]
    ids = np.random.RandomState(3).randint(0, v, (n, 8)).astype(np.int64)
    outs = {"logits": (n, 8, v), **{k: (n, KG.NARROW["kv_heads"], 8, 32) for k in KG.present_names()}}
    with RG.session(dict(IE_PRECISION=prec), {f"s{lq}": models.write_repo(str(tmp_path), f"s{lq}", KG.narrow(quant="int4", **kw))
                                              for lq, kw in ((8, dict(seq=8, present=True)), (1, dict(seq=1, past=p)), (4, dict(seq=4, past=p)))}) as (ms, _):
        ref = TRC.ref64.run_f64(KG.narrow(quant="int4", q_form="dense", seq=8, present=True), {"input_ids": ids})
        got = RG.request(ms["s8"], {"input_ids": ids}, outs)
        assert sum("qlinear" in s for s in TRC._kernels(ms["s8"])) == 5 * KG.NARROW["depth"]
        for k in outs:
            TRC._close(got[k].reshape(n, -1, got[k].shape[-1]), ref[k].reshape(n, -1, ref[k].shape[-1]), prec, f"int4 llama {prec} prefill {k}")
        cache = KG.cache_from({k: ref[k].astype(np.float32) for k in KG.present_names()}, [8, 5])
        for lq in (1, 4):
            new = np.random.RandomState(lq).randint(0, v, (n, lq)).astype(np.int64)
            f = dict({"input_ids": new, "attention_mask": TRC.EG.chunk_mask([8, 5], (lq, lq), p, lq), "position_ids": np.array([[8 + i for i in range(lq)], [5 + i for i in range(lq)]], np.int64)}, **cache)
            want = TRC.ref64.run_f64(KG.narrow(quant="int4", q_form="dense", seq=lq, past=p), f)["logits"]
            TRC._close(RG.request(ms[f"s{lq}"], f, {"logits": (n, lq, v)})["logits"], want, prec, f"int4 llama {prec} {'decode' if lq == 1 else 'extend'}")


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ("fp32", "fp16"))
def test_int4_llama_bound_to_a_resident_cache(tmp_path, prec, monkeypatch):
    """the ragged extend and three greedy decode steps of the resident-cache tests, with the int4 models bound to one cache (fp16: a half cache) and the
    float64 walk on their dense twins"""
    narrow = KG.narrow
    paths = {"ext": models.write_repo(str(tmp_path), "ext", narrow(seq=4, past=KG.NARROW_P, quant="int4")), "dec": models.write_repo(str(tmp_path), "dec", narrow(seq=1, past=KG.NARROW_P, quant="int4"))}
    monkeypatch.setattr(KG, "narrow", lambda *a, **kw: narrow(*a, **dict(kw, quant="int4", q_form="dense")))      # (the walk's reference graphs: the twins)
    dims = (KG.NARROW["depth"], KG.NARROW_N, KG.NARROW["kv_heads"], KG.NARROW_P, 32) + ((0, "f16") if prec == "fp16" else ())
    with RG.session(dict(IE_PRECISION=prec), paths, dims) as (ms, kc):
        TRC._generate(ms, kc, prec)
        assert sum("qlinear" in s for s in TRC._kernels(ms["dec"])) == 5 * KG.NARROW["depth"]
