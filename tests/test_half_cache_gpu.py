"""GPU (-m gpu): fp16 models bound to a HALF resident KV cache (B.KvCache(..., dtype="f16")) against the float64 walk of the same ONNX graph
(tests/ref64.py) fed the equivalent client-held cache ROUNDED TO HALF, within engine_run.RTOL["fp16"] of max|ref|.  N = 2, and H = 4 where a case names no other.

As in test_resident_cache_gpu.py the cache a test writes holds NaN at and beyond an image's length; after a step the untouched rows are compared bit for bit
with what was written, the appended rows with the reference's `present` rows, and they must be exactly half-representable."""
import numpy as np
import pytest

import extend_graphs as EG
import kv_graphs as KG
import ref64
import resident_graphs as RG
from engine_run import RTOL
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models

pytestmark = pytest.mark.gpu
N, H = 2, 4
TOL = RTOL["fp16"]


def _h(x):
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def _half_past(feeds):
    return {k: _h(v) if k.startswith("past_key_values.") else v for k, v in feeds.items()}


def _kv16(label):
    """launch.cpp kernel_label of the same step over a half cache"""
    out = label.replace(",inplace>", ",inplace,kv16>").replace("generic_kernel<f16>", "generic_kernel<f16,kv16>")
    assert "inplace" in out and "kv16" in out
    return out


def _kernels(m):
    return [p["kernel"] for p in B.Profile(m, 1)]


def _dims(layers, kvh, past, hd):
    return (layers, N, kvh, past, hd, 0, "f16")


def _check_cache(kc, written, ref, lens, new, past, what):
    for which, name in enumerate(("present.0.key", "present.0.value")):
        got, was = kc.read(0, which), written[(0, which)]
        for n, (ln, c) in enumerate(zip(lens, new)):
            assert np.array_equal(RG.bits(got[n, :, :ln]), RG.bits(was[n, :, :ln])), (what, name, n, "rows below len changed")
            assert np.array_equal(RG.bits(got[n, :, ln + c:]), RG.bits(was[n, :, ln + c:])), (what, name, n, "rows beyond the appended ones changed")
            if c:
                r = got[n, :, ln:ln + c]
                err = ref64.rel_err(r, ref[name][n, :, past:past + c])
                print(f"{what} {name} image {n}: appended rows, max err / max|ref| {err:.3e}")
                assert np.array_equal(r, _h(r)) and err < TOL, (what, name, n, err)
    assert kc.lengths() == [ln + c for ln, c in zip(lens, new)], (what, kc.lengths())


def _decode(tmp_path, kvh, hd, past, lens, *, tile, env=None, splits=None, twice=False, H=H):
    rows, feeds = KG.decode_feeds(N, H, kvh, hd, past, valid=list(lens), positions=list(lens))
    feeds = _half_past(feeds)
    mb = KG.decode_attn_graph(rows, N, H, kvh, hd, past, max_pos=max(64, past + 8))
    ref = ref64.run_f64(mb, feeds)
    path = models.write_repo(str(tmp_path), "dec", mb)
    what = f"half cache decode H {H}/{kvh} hd {hd} P {past} len {tuple(lens)} tile {tile} S {splits}"
    with RG.session(dict(IE_PRECISION="fp16", **(env or {})), {"dec": path}, _dims(1, kvh, past, hd)) as (ms, kc):
        runs = []
        for _ in range(2 if twice else 1):
            written = RG.fill(kc, feeds, lens)
            y = RG.request(ms["dec"], RG.unbound(feeds), {"out": (N, 1, H * hd)})["out"]
            err = ref64.rel_err(y, ref["out"])
            print(f"{what} out: max err / max|ref| {err:.3e}")
            assert np.isfinite(y).all() and err < TOL, (what, err)
            _check_cache(kc, written, ref, lens, (1, 1), past, what)
            runs.append((y, kc.read(0, 0), kc.read(0, 1)))
        kern = _kernels(ms["dec"])
    assert _kv16(RG.decode_label(tile, True, hd, splits or 1)) in kern, kern
    for a, b in zip(runs[0], runs[-1]):
        assert np.array_equal(RG.bits(a), RG.bits(b)), what


@pytest.mark.parametrize("tile", (0, 4))
@pytest.mark.parametrize("kvh", (4, 2, 1))
@pytest.mark.parametrize("hd", (32, 64, 128))
def test_decode_heads_and_head_dims(tmp_path, hd, kvh, tile):
    """groups of 1, 2 and 4 heads at every fast head dim, two keys beyond the half key tile (P = 66 / 34 / 18); image 0 holds 3 rows, image 1 all but one"""
    past = 2048 // hd + 2
    _decode(tmp_path, kvh, hd, past, (3, past - 1), tile=tile, env={"IE_ATTN_TILE": str(tile)})


@pytest.mark.parametrize("ln", (0, 1, 31, 32, 33))
def test_decode_lengths_around_the_key_tile(tmp_path, ln):
    """hd 64, whose half key tile is 32 keys: len = 0 (the new key is the only one), 1, the tile - 1, the tile, the tile + 1 in a cache of 72 rows"""
    _decode(tmp_path, 2, 64, 72, (ln, ln), tile=4)


@pytest.mark.parametrize("splits", (1, 3, None))
def test_decode_long_cache_and_splits(tmp_path, splits):
    """P = 200 at IE_ATTN_SPLITS 1, 3 and the default; image 0 holds 3 rows, so at S = 3 two of its splits have no keys.  At S = 3 the step runs twice from
    the same cache state: out and cache are bit-equal"""
    kvh, hd = 2, 64
    env = {} if splits is None else {"IE_ATTN_SPLITS": str(splits)}
    _decode(tmp_path, kvh, hd, 200, (3, 199), tile=4, env=env, splits=splits or KG.default_splits(N, kvh, 201, hd), twice=splits == 3)


@pytest.mark.parametrize("hd", (48, 36, 34))
def test_decode_generic_route(tmp_path, hd):
    """head dims that fit no fast kernel run the generic wave over half K / V; the append takes 16-byte stores at hd 48, 8-byte ones at 36, scalar ones at 34"""
    assert not KG.fast_fits(hd, H, 2)
    _decode(tmp_path, 2, hd, 21, (3, 20), tile=0)


@pytest.mark.parametrize("heads,kvh", ((8, 1), (6, 2)))
def test_decode_wide_and_unfilled_groups(tmp_path, heads, kvh):
    """beyond the H = 4 cases: a group of 8 heads (the G = 8 form, the one with the most registers) and a group of 3 on the G = 4 form, hd 128 and 32"""
    for hd in (128, 32):
        past = 2048 // hd + 2
        _decode(tmp_path, kvh, hd, past, (3, past - 1), tile=4, H=heads)


@pytest.mark.parametrize("tile", (0, 5))
@pytest.mark.parametrize("lq", (2, 5, 33))
def test_extend(tmp_path, lq, tile):
    """Lq = 2, 5 (ragged: image 0 takes 2 of its 5 tokens) and 33 new tokens over a cache of 70 rows, hd 64, 2 K / V heads"""
    kvh, hd, past = 2, 64, 70
    lens, new = (3, past - lq), ((2, lq) if lq == 5 else (lq, lq))
    rows, feeds = EG.extend_feeds(N, H, kvh, hd, past, lq, valid=list(lens), chunk_valid=list(new), max_pos=128)
    feeds = _half_past(feeds)
    mb = EG.extend_attn_graph(rows, N, H, kvh, hd, past, lq, max_pos=128)
    ref = ref64.run_f64(mb, feeds)
    path = models.write_repo(str(tmp_path), "ext", mb)
    what = f"half cache extend Lq {lq} tile {tile}"
    with RG.session(dict(IE_PRECISION="fp16", IE_ATTN_TILE=str(tile)), {"ext": path}, _dims(1, kvh, past, hd)) as (ms, kc):
        written = RG.fill(kc, feeds, lens)
        y = RG.request(ms["ext"], RG.unbound(feeds), {"out": (N, lq, H * hd)})["out"]
        _check_cache(kc, written, ref, lens, new, past, what)
        kern = _kernels(ms["ext"])
    valid = EG.own_key_valid(feeds, past)
    err = float(np.abs(y[valid] - ref["out"][valid]).max() / np.abs(ref["out"]).max())
    print(f"{what} out at the valid tokens: max err / max|ref| {err:.3e}")
    assert np.isfinite(y).all() and err < TOL, (what, err)
    assert _kv16(RG.extend_label(tile, True, hd)) in kern, kern


def _close(got, want, what, rows=None):
    rows = np.ones(got.shape[:2], bool) if rows is None else rows
    err = float(np.abs(got[rows] - want[rows]).max() / np.abs(want).max())
    print(f"{what}: max err / max|ref| {err:.3e}")
    assert np.isfinite(got).all() and err < TOL, (what, err)


class _HalfWalk:
    """the client-held equivalent of a half cache in float64's own outputs, re-rounded to half after every step: what ref64 is fed"""

    def __init__(self):
        self.P, self.V = KG.NARROW_P, KG.NARROW["vocab"]
        hkv, hd = KG.NARROW["kv_heads"], KG.NARROW["dim"] // KG.NARROW["heads"]
        self.cache = {k.replace("present", "past_key_values"): np.zeros((N, hkv, self.P, hd), np.float32) for k in KG.present_names()}
        self.lens = [0, 0]

    def step(self, ids, new):
        lq = ids.shape[1]
        pos = np.array([[ln + i for i in range(lq)] for ln in self.lens], np.int64)
        f = dict({"input_ids": ids, "attention_mask": EG.chunk_mask(self.lens, new, self.P, lq), "position_ids": pos}, **self.cache)
        ref = ref64.run_f64(KG.narrow(seq=lq, past=self.P), f)
        for k in KG.present_names():
            for n, c in enumerate(new):
                self.cache[k.replace("present", "past_key_values")][n, :, self.lens[n]:self.lens[n] + c] = _h(ref[k][n, :, self.P:self.P + c])
        self.lens = [ln + c for ln, c in zip(self.lens, new)]
        return f, ref["logits"]


def test_narrow_llama_end_to_end(tmp_path):
    """the extend and the decode model of the narrow Llama on ONE half cache: a ragged prompt (4 and 3 tokens), then three greedy steps"""
    P, depth = KG.NARROW_P, KG.NARROW["depth"]
    hkv, hd = KG.NARROW["kv_heads"], KG.NARROW["dim"] // KG.NARROW["heads"]
    paths = {"ext": models.write_repo(str(tmp_path), "ext", KG.narrow(seq=4, past=P)), "dec": models.write_repo(str(tmp_path), "dec", KG.narrow(seq=1, past=P))}
    with RG.session(dict(IE_PRECISION="fp16"), paths, _dims(depth, hkv, P, hd)) as (ms, kc):
        w = _HalfWalk()
        ids, new = np.random.RandomState(11).randint(0, w.V, (N, 4)).astype(np.int64), (4, 3)
        f, want = w.step(ids, new)
        got = RG.request(ms["ext"], RG.unbound(f), {"logits": (N, 4, w.V)})["logits"]
        _close(got, want, "narrow llama on a half cache, ragged extend", EG.own_key_valid(f, P))
        nxt = np.array([[got[n, c - 1].argmax()] for n, c in enumerate(new)], np.int64)
        for s in range(3):
            f, want = w.step(nxt, (1, 1))
            got = RG.request(ms["dec"], RG.unbound(f), {"logits": (N, 1, w.V)})["logits"]
            _close(got, want, f"narrow llama on a half cache, decode step {s}")
            nxt = got[:, 0].argmax(-1).reshape(N, 1).astype(np.int64)
        assert kc.lengths() == w.lens == [7, 6]
        info = B.RuntimeInfo(ms["dec"])["kv_cache"]
        assert info["dtype"] == "f16" and info["bytes"] == 2 * depth * N * hkv * P * hd * 2, info
        kd, ke = _kernels(ms["dec"]), _kernels(ms["ext"])
    assert sum(_kv16(RG.decode_label(4, True, hd)) in k for k in kd) == depth, kd
    assert sum("attention_extend_kernel" in k and ",inplace,kv16>" in k for k in ke) == depth, ke


def test_an_fp32_model_is_refused_by_name(tmp_path):
    kvh, hd, past, lens = 2, 32, 12, (3, 11)
    rows, feeds = KG.decode_feeds(N, H, kvh, hd, past, valid=list(lens), positions=list(lens))
    path = models.write_repo(str(tmp_path), "f32", KG.decode_attn_graph(rows, N, H, kvh, hd, past, max_pos=64))
    with RG.session(dict(IE_PRECISION="fp32"), {"f32": path}) as (ms, _):
        kc = B.KvCache(*_dims(1, kvh, past, hd))
        try:
            written = RG.fill(kc, _half_past(feeds), lens)
            with pytest.raises(RuntimeError, match="the cache stores f16 and the model runs in fp32 precision.*IE_PRECISION=fp16"):
                kc.bind(ms["f32"])
            assert kc.lengths() == list(lens) and "kv_cache" not in B.RuntimeInfo(ms["f32"])
            for which in (0, 1):
                assert np.array_equal(RG.bits(kc.read(0, which)), RG.bits(written[(0, which)]))
        finally:
            kc.destroy()
