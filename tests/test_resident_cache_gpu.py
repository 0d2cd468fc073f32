"""GPU (-m gpu): models bound to a resident KV cache (B.KvCache) against the float64 walk of the same ONNX graph (tests/ref64.py) fed the equivalent
right-padded client-held cache and mask, with the project's bounds (engine_run.RTOL of max|ref|).  N = 2, H = 4 everywhere.

The cache a test writes holds NaN in every row at or beyond an image's length, so a kernel that reads beyond `len` shows in `out`; after a step the rows
below `len` and the rows above the appended ones are compared bit for bit with what was written (the NaN rows included), the appended rows with the
reference's `present` rows."""
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
PRECS = ("fp32", "fp16")


def _kernels(m):
    return [p["kernel"] for p in B.Profile(m, 1)]


def _check_cache(kc, written, ref, lens, new, past, prec, what):
    """rows < len and rows >= len + c as written, bit for bit; the c appended rows against the reference's present rows past ..; the lengths advanced"""
    for which, name in enumerate(("present.0.key", "present.0.value")):
        got, was = kc.read(0, which), written[(0, which)]
        for n, (ln, c) in enumerate(zip(lens, new)):
            assert np.array_equal(RG.bits(got[n, :, :ln]), RG.bits(was[n, :, :ln])), (what, name, n, "rows below len changed")
            assert np.array_equal(RG.bits(got[n, :, ln + c:]), RG.bits(was[n, :, ln + c:])), (what, name, n, "rows beyond the appended ones changed")
            if c:
                err = ref64.rel_err(got[n, :, ln:ln + c], ref[name][n, :, past:past + c])
                print(f"{what} {name} image {n}: appended rows, max err / max|ref| {err:.3e}")
                assert err < RTOL[prec], (what, name, n, err)
    assert kc.lengths() == [ln + c for ln, c in zip(lens, new)], (what, kc.lengths())


def _decode(tmp_path, prec, kvh, hd, past, lens, *, tile, env=None, splits=None, name="dec"):
    """one bound decode step of the attention subgraph: `out`, the cache afterwards, the lengths and the launched kernel"""
    rows, feeds = KG.decode_feeds(N, H, kvh, hd, past, valid=list(lens), positions=list(lens))
    mb = KG.decode_attn_graph(rows, N, H, kvh, hd, past, max_pos=max(64, past + 8))
    ref = ref64.run_f64(mb, feeds)
    path = models.write_repo(str(tmp_path), name, mb)
    what = f"bound decode H {H}/{kvh} hd {hd} P {past} len {tuple(lens)} {prec} tile {tile} S {splits}"
    with RG.session(dict(IE_PRECISION=prec, **(env or {})), {name: path}, (1, N, kvh, past, hd)) as (ms, kc):
        written = RG.fill(kc, feeds, lens)
        y = RG.request(ms[name], RG.unbound(feeds), {"out": (N, 1, H * hd)})["out"]
        err = ref64.rel_err(y, ref["out"])
        print(f"{what} out: max err / max|ref| {err:.3e}")
        assert np.isfinite(y).all() and err < RTOL[prec], (what, err)
        _check_cache(kc, written, ref, lens, (1, 1), past, prec, what)
        kern = _kernels(ms[name])
    label = RG.decode_label(tile, prec == "fp16", hd, splits or 1)
    assert label in kern and "inplace" in label, (label, kern)
    return y


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("tile", (0, 4))
@pytest.mark.parametrize("kvh", (4, 2, 1))
@pytest.mark.parametrize("hd", (32, 64, 128))
def test_decode_heads_and_head_dims(tmp_path, hd, kvh, tile, prec):
    """(H, Hkv) = (4, 4), (4, 2), (4, 1) at every fast head dim, two keys beyond a key tile; image 0 holds 3 rows, image 1 all but one"""
    past = KG.key_tile(hd) + 2
    _decode(tmp_path, prec, kvh, hd, past, (3, past - 1), tile=tile, env={"IE_ATTN_TILE": str(tile)})


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("tile", (0, 4))
@pytest.mark.parametrize("ln", (0, 1, 15, 16, 17))
def test_decode_lengths_around_the_key_tile(tmp_path, ln, tile, prec):
    """len = 0 (the new key is the only one), 1, the key tile - 1, the key tile, the key tile + 1 (hd 64: 16 keys) in a cache of 40 rows"""
    assert KG.key_tile(64) == 16
    _decode(tmp_path, prec, 2, 64, 40, (ln, ln), tile=tile, env={"IE_ATTN_TILE": str(tile)})


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("splits", (1, 3, None))
def test_decode_long_cache_and_splits(tmp_path, splits, prec):
    """P = 200 with IE_ATTN_SPLITS 1, 3 and the default: image 0 holds 3 rows, so at S = 3 two of its splits have no keys and leave the combine with weight 0"""
    kvh, hd = 2, 64
    env = {} if splits is None else {"IE_ATTN_SPLITS": str(splits)}
    _decode(tmp_path, prec, kvh, hd, 200, (3, 199), tile=4, env=env, splits=splits or KG.default_splits(N, kvh, 201, hd))


@pytest.mark.parametrize("prec", PRECS)
def test_decode_generic_route(tmp_path, prec):
    """hd 48 fits no fast kernel: the default plan and a pinned tile 4 both run the generic in-place pair"""
    assert not KG.fast_fits(48, H, 2)
    _decode(tmp_path, prec, 2, 48, 21, (3, 20), tile=0)
    _decode(tmp_path, prec, 2, 48, 21, (3, 20), tile=0, env={"IE_ATTN_TILE": "4"}, name="pin")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("tile", (0, 5))
@pytest.mark.parametrize("lq", (2, 5, 33))
def test_extend(tmp_path, lq, tile, prec):
    """Lq = 2, 5 and 33 new tokens over a cache of 70 rows, image 0 holding 3 rows and image 1 all but Lq; at Lq = 5 image 0's chunk is ragged (2 of 5 tokens):
    its padded tokens' rows in the cache stay as written, its length advances by 2, valid tokens are within the bound, padded ones finite"""
    kvh, hd, past = 2, 64, 70
    lens, new = (3, past - lq), ((2, lq) if lq == 5 else (lq, lq))
    rows, feeds = EG.extend_feeds(N, H, kvh, hd, past, lq, valid=list(lens), chunk_valid=list(new), max_pos=128)
    mb = EG.extend_attn_graph(rows, N, H, kvh, hd, past, lq, max_pos=128)
    ref = ref64.run_f64(mb, feeds)
    path = models.write_repo(str(tmp_path), "ext", mb)
    what = f"bound extend Lq {lq} {prec} tile {tile}"
    with RG.session(dict(IE_PRECISION=prec, IE_ATTN_TILE=str(tile)), {"ext": path}, (1, N, kvh, past, hd)) as (ms, kc):
        written = RG.fill(kc, feeds, lens)
        y = RG.request(ms["ext"], RG.unbound(feeds), {"out": (N, lq, H * hd)})["out"]
        _check_cache(kc, written, ref, lens, new, past, prec, what)
        kern = _kernels(ms["ext"])
    valid = EG.own_key_valid(feeds, past)
    assert np.isfinite(y).all(), what
    err = float(np.abs(y[valid] - ref["out"][valid]).max() / np.abs(ref["out"]).max())
    print(f"{what} out at the valid tokens: max err / max|ref| {err:.3e}")
    assert err < RTOL[prec], (what, err)
    assert EG.default_splits(N, kvh, (H // kvh) * lq, past + lq) == 1
    label = RG.extend_label(tile, prec == "fp16", hd)
    assert label in kern and "inplace" in label, (label, kern)


def _narrow_session(tmp_path, prec, extra=None):
    P = KG.NARROW_P
    paths = {"ext": models.write_repo(str(tmp_path), "ext", KG.narrow(seq=4, past=P)), "dec": models.write_repo(str(tmp_path), "dec", KG.narrow(seq=1, past=P))}
    paths.update(extra or {})
    hkv, hd = KG.NARROW["kv_heads"], KG.NARROW["dim"] // KG.NARROW["heads"]
    return RG.session(dict(IE_PRECISION=prec), paths, (KG.NARROW["depth"], N, hkv, P, hd))


class _Walk:
    """the client-held equivalent of the resident cache, in float64's own outputs: what ref64 is fed and what the engine's logits are held against"""

    def __init__(self):
        self.P, self.V = KG.NARROW_P, KG.NARROW["vocab"]
        hkv, hd = KG.NARROW["kv_heads"], KG.NARROW["dim"] // KG.NARROW["heads"]
        self.cache = {k.replace("present", "past_key_values"): np.zeros((N, hkv, self.P, hd), np.float32) for k in KG.present_names()}
        self.lens = [0, 0]
        self.mb = {1: KG.narrow(seq=1, past=self.P), 4: KG.narrow(seq=4, past=self.P)}

    def feeds(self, ids, new):
        lq = ids.shape[1]
        pos = np.array([[ln + i for i in range(lq)] for ln in self.lens], np.int64)
        return dict({"input_ids": ids, "attention_mask": EG.chunk_mask(self.lens, new, self.P, lq), "position_ids": pos}, **self.cache)

    def step(self, ids, new):
        """float64 of one call on the client-held cache; the cache and lengths then take the call's new rows (in float32, as a client would hold them)"""
        f = self.feeds(ids, new)
        ref = ref64.run_f64(self.mb[ids.shape[1]], f)
        for k in KG.present_names():
            for n, c in enumerate(new):
                self.cache[k.replace("present", "past_key_values")][n, :, self.lens[n]:self.lens[n] + c] = ref[k][n, :, self.P:self.P + c]
        self.lens = [ln + c for ln, c in zip(self.lens, new)]
        return f, ref["logits"]


def _close(got, want, prec, what, rows=None):
    rows = np.ones(got.shape[:2], bool) if rows is None else rows
    err = float(np.abs(got[rows] - want[rows]).max() / np.abs(want).max())
    print(f"{what}: max err / max|ref| {err:.3e}")
    assert np.isfinite(got).all() and err < RTOL[prec], (what, err)


def _generate(ms, kc, prec, steps=3):
    """empty cache, an extend of a ragged prompt (4 and 3 tokens), then `steps` greedy decode steps: every call's logits at valid tokens against the walk.
    -> (the walk, the sequences, the last logits)"""
    w = _Walk()
    ids = np.random.RandomState(11).randint(0, w.V, (N, 4)).astype(np.int64)
    new = (4, 3)
    f, want = w.step(ids, new)
    got = RG.request(ms["ext"], RG.unbound(f), {"logits": (N, 4, w.V)})["logits"]
    _close(got, want, prec, f"narrow llama {prec} ragged extend", EG.own_key_valid(f, w.P))
    assert kc.lengths() == [4, 3]
    seqs = [list(ids[n, :c]) for n, c in enumerate(new)]
    nxt = np.array([[got[n, c - 1].argmax()] for n, c in enumerate(new)], np.int64)
    for s in range(steps):
        for n in range(N):
            seqs[n].append(int(nxt[n, 0]))
        f, want = w.step(nxt, (1, 1))
        got = RG.request(ms["dec"], RG.unbound(f), {"logits": (N, 1, w.V)})["logits"]
        _close(got, want, prec, f"narrow llama {prec} decode step {s}")
        nxt = got[:, 0].argmax(-1).reshape(N, 1).astype(np.int64)
    assert kc.lengths() == w.lens
    return w, seqs, got


@pytest.mark.parametrize("prec", PRECS)
def test_narrow_llama_end_to_end(tmp_path, prec):
    """the extend model (seq 4) and the decode model (seq 1) of the narrow Llama bound to ONE cache; the last step also against the float64 prefill of each
    image's whole sequence; the in-place kernels once per layer in both profiles"""
    depth, hd = KG.NARROW["depth"], KG.NARROW["dim"] // KG.NARROW["heads"]
    with _narrow_session(tmp_path, prec) as (ms, kc):
        w, seqs, last = _generate(ms, kc, prec)
        info = B.RuntimeInfo(ms["dec"])["kv_cache"]
        assert (info["layers"], info["batch"], info["capacity"], info["lengths"], info["models_bound"]) == (depth, N, KG.NARROW_P, w.lens, 2), info
        kd, ke = _kernels(ms["dec"]), _kernels(ms["ext"])
    assert sum(RG.decode_label(4, prec == "fp16", hd) in k for k in kd) == depth, kd
    assert sum("attention_extend_kernel" in k and "inplace" in k for k in ke) == depth, ke
    for n, seq in enumerate(seqs):
        full = ref64.run_f64(KG.narrow(batch=1, seq=len(seq)), {"input_ids": np.array([seq], np.int64)})["logits"]
        _close(last[n:n + 1, 0], full[:, -1], prec, f"narrow llama {prec} image {n}: the last step against the float64 prefill of its {len(seq)} tokens")


@pytest.mark.parametrize("prec", PRECS)
def test_bound_prefill_fills_an_empty_cache(tmp_path, prec):
    """the prefill graph with `present` outputs bound to an empty cache writes rows 0..4 of every layer; on a cache that holds rows it is refused"""
    P, V, depth = KG.NARROW_P, KG.NARROW["vocab"], KG.NARROW["depth"]
    hkv, hd = KG.NARROW["kv_heads"], KG.NARROW["dim"] // KG.NARROW["heads"]
    mb = KG.narrow(seq=5, present=True)
    ids = np.random.RandomState(7).randint(0, V, (N, 5)).astype(np.int64)
    ref = ref64.run_f64(mb, {"input_ids": ids})
    path = models.write_repo(str(tmp_path), "pre", mb)
    with RG.session(dict(IE_PRECISION=prec), {"pre": path}, (depth, N, hkv, P, hd)) as (ms, kc):
        got = RG.request(ms["pre"], {"input_ids": ids}, {"logits": (N, 5, V)})["logits"]
        _close(got, ref["logits"], prec, f"bound prefill {prec} logits")
        assert kc.lengths() == [5, 5]
        for layer in range(depth):
            for which, wname in enumerate(("key", "value")):
                c = kc.read(layer, which)
                _close(c[:, :, :5], ref[f"present.{layer}.{wname}"], prec, f"bound prefill {prec} layer {layer} {wname}")
                assert not c[:, :, 5:].any(), "rows beyond the prompt are the zeros of creation"
        with pytest.raises(RuntimeError, match="needs an empty cache: image 0 holds 5 rows"):
            RG.request(ms["pre"], {"input_ids": ids}, {"logits": (N, 5, V)})
        assert kc.lengths() == [5, 5]
        assert any("kv_append_rows_kernel" in k and "inplace" in k for k in _kernels(ms["pre"]))


@pytest.mark.parametrize("prec", PRECS)
def test_roll_back(tmp_path, prec):
    """after three decode steps the lengths go back by two (two rejected drafts): the next step is the float64 walk's over the shorter cache"""
    with _narrow_session(tmp_path, prec) as (ms, kc):
        w, seqs, _ = _generate(ms, kc, prec)
        w.lens = [ln - 2 for ln in w.lens]
        kc.set_lengths(w.lens)
        nxt = np.array([[5], [9]], np.int64)
        f, want = w.step(nxt, (1, 1))
        got = RG.request(ms["dec"], RG.unbound(f), {"logits": (N, 1, w.V)})["logits"]
        _close(got, want, prec, f"narrow llama {prec} after the roll-back")
        assert kc.lengths() == w.lens


def test_refusals(tmp_path):
    """every refused request leaves lengths and cache bytes as they were, and a correct request then gives the right result; every refused Bind names
    its reason"""
    kvh, hd, past = 2, 32, 12
    lens = (3, 11)
    rows, feeds = KG.decode_feeds(N, H, kvh, hd, past, valid=list(lens), positions=list(lens))
    mb = KG.decode_attn_graph(rows, N, H, kvh, hd, past, max_pos=64)
    ref = ref64.run_f64(mb, feeds)
    path = models.write_repo(str(tmp_path), "ref", mb)
    out = {"out": (N, 1, H * hd)}
    with RG.session(dict(IE_PRECISION="fp32"), {"ref": path}, (1, N, kvh, past, hd)) as (ms, kc):
        m = ms["ref"]
        written = RG.fill(kc, feeds, lens)
        good = RG.unbound(feeds)

        def refused(f, outs, *texts, now=lens):
            with pytest.raises(RuntimeError) as e:
                RG.request(m, f, outs)
            for t in texts:
                assert t in str(e.value), (t, str(e.value))
            assert kc.lengths() == list(now)
            for which in (0, 1):
                assert np.array_equal(RG.bits(kc.read(0, which)), RG.bits(written[(0, which)])), "a refused request wrote to the cache"

        bad = good["attention_mask"].copy()
        bad[0, 5] = 1
        refused(dict(good, attention_mask=bad), out, "image 0 has a one in cache column 5", "cached length 3")
        kc.set_lengths((3, past))
        refused(dict(good, attention_mask=KG.cache_mask((3, past), past)), out, f"The KV cache is full: image 1 holds {past} of {past} rows", now=(3, past))
        kc.set_lengths(lens)
        refused(good, dict(out, **{"present.0.key": (N, kvh, past + 1, hd)}), "Output present.0.key is not available from a model bound to a KV cache")
        refused(feeds, out, "Expected 3 inputs, got 5")
        swapped = {k: v for k, v in good.items() if k != "position_ids"}
        swapped["past_key_values.0.key"] = feeds["past_key_values.0.key"]
        refused(swapped, out, "Unexpected input name: past_key_values.0.key")
        # a Bind that does not fit, dimension by dimension; the model stays bound to its cache
        for dims, text in (((1, N, 4, past, hd), "geometry mismatch in kv_heads: the model has 2, the cache 4"), ((1, N, kvh, past + 1, hd), "geometry mismatch in capacity"),
                           ((1, N, kvh, past, 64), "geometry mismatch in head_dim: the model has 32, the cache 64"), ((2, N, kvh, past, hd), "geometry mismatch in layers: the model has 1, the cache 2")):
            other = B.KvCache(*dims)
            try:
                with pytest.raises(RuntimeError, match=text):
                    other.bind(m)
            finally:
                other.destroy()
        y = RG.request(m, good, out)["out"]
        assert ref64.rel_err(y, ref["out"]) < RTOL["fp32"]
        _check_cache(kc, written, ref, lens, (1, 1), past, "fp32", "after the refusals")


def test_extend_mask_must_be_a_prefix(tmp_path):
    kvh, hd, past, lq = 2, 32, 20, 4
    lens = (3, 9)
    rows, feeds = EG.extend_feeds(N, H, kvh, hd, past, lq, valid=list(lens))
    path = models.write_repo(str(tmp_path), "ext", EG.extend_attn_graph(rows, N, H, kvh, hd, past, lq))
    with RG.session(dict(IE_PRECISION="fp32"), {"ext": path}, (1, N, kvh, past, hd)) as (ms, kc):
        kc.set_lengths(lens)
        bad = feeds["attention_mask"].copy()
        bad[1, past + 1] = 0
        with pytest.raises(RuntimeError, match=r"image 1 has a one in new-token column 22 behind a zero in column 21"):
            RG.request(ms["ext"], dict(RG.unbound(feeds), attention_mask=bad), {"out": (N, lq, H * hd)})
        assert kc.lengths() == list(lens)
        kc.set_lengths((3, 18))
        with pytest.raises(RuntimeError, match=r"The KV cache is full: image 1 holds 18 of 20 rows and the request appends 4"):
            RG.request(ms["ext"], RG.unbound(feeds), {"out": (N, lq, H * hd)})
        assert kc.lengths() == [3, 18]


def test_bind_refusals_by_model(tmp_path):
    """a model without a cache, and a model with two execution lanes"""
    P = KG.NARROW_P
    hkv, hd, depth = KG.NARROW["kv_heads"], KG.NARROW["dim"] // KG.NARROW["heads"], KG.NARROW["depth"]
    plain = models.write_repo(str(tmp_path), "plain", KG.narrow(seq=8))
    two = models.write_repo(str(tmp_path), "two", KG.narrow(seq=1, past=P), config_json='{"instance_count": 2}')
    with RG.session(dict(IE_PRECISION="fp32"), {"plain": plain, "two": two}) as (ms, _):
        kc = B.KvCache(depth, N, hkv, P, hd)
        try:
            with pytest.raises(RuntimeError, match="the model has no cache: neither past_key_values.\\* inputs nor present.\\* outputs"):
                kc.bind(ms["plain"])
            with pytest.raises(RuntimeError, match="the model has 2 execution lanes"):
                kc.bind(ms["two"])
            assert "kv_cache" not in B.RuntimeInfo(ms["two"])
        finally:
            kc.destroy()


@pytest.mark.parametrize("prec", PRECS)
def test_two_sequences_from_a_reset_cache_are_bit_equal_at_three_splits(tmp_path, prec):
    kvh, hd, past = 2, 64, 200
    lens = (3, 197)
    rows, feeds = KG.decode_feeds(N, H, kvh, hd, past, valid=list(lens), positions=list(lens))
    path = models.write_repo(str(tmp_path), "rep", KG.decode_attn_graph(rows, N, H, kvh, hd, past, max_pos=256))
    with RG.session(dict(IE_PRECISION=prec, IE_ATTN_SPLITS="3"), {"rep": path}, (1, N, kvh, past, hd)) as (ms, kc):
        runs = []
        for _ in range(2):
            RG.fill(kc, feeds, lens)
            ys = []
            for step in range(3):
                f = dict(RG.unbound(feeds), attention_mask=KG.cache_mask([ln + step for ln in lens], past))
                ys.append(RG.request(ms["rep"], f, {"out": (N, 1, H * hd)})["out"])
            runs.append((ys, kc.read(0, 0), kc.read(0, 1)))
            assert kc.lengths() == [ln + 3 for ln in lens]
        kern = _kernels(ms["rep"])
    assert RG.decode_label(4, prec == "fp16", hd, 3) in kern, kern
    for a, b in zip(runs[0][0], runs[1][0]):
        assert np.array_equal(a, b)
    assert np.array_equal(RG.bits(runs[0][1]), RG.bits(runs[1][1])) and np.array_equal(RG.bits(runs[0][2]), RG.bits(runs[1][2]))


def test_unbind_gives_the_graph_its_cache_back(tmp_path):
    """an unbound model takes past / gives present again, and its result is a never-bound model's bit for bit"""
    kvh, hd, past = 2, 64, 40
    rows, feeds = KG.decode_feeds(N, H, kvh, hd, past, valid=[3, past], positions=[3, past])
    path = models.write_repo(str(tmp_path), "ub", KG.decode_attn_graph(rows, N, H, kvh, hd, past, max_pos=64))
    outs = {"out": (N, 1, H * hd), "present.0.key": (N, kvh, past + 1, hd), "present.0.value": (N, kvh, past + 1, hd)}
    with RG.session(dict(IE_PRECISION="fp32"), {"a": path, "never": path}) as (ms, _):
        kc = B.KvCache(1, N, kvh, past, hd)
        try:
            kc.bind(ms["a"])
            RG.fill(kc, feeds, (3, past - 1))
            RG.request(ms["a"], dict(RG.unbound(feeds), attention_mask=KG.cache_mask((3, past - 1), past)), {"out": outs["out"]})
            assert "kv_cache" in B.RuntimeInfo(ms["a"])
            B.KvCache.unbind(ms["a"])
            assert "kv_cache" not in B.RuntimeInfo(ms["a"])
            a, b = RG.request(ms["a"], feeds, outs), RG.request(ms["never"], feeds, outs)
            assert not any("inplace" in k for k in _kernels(ms["a"]))
        finally:
            kc.destroy()
    for k in outs:
        assert np.array_equal(a[k], b[k]), k
