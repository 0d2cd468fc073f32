"""GPU (-m gpu): the attention kernels held row by row and element by element to the derived bound of tests/attn_ref.py,

    |y - ref| <= MARGIN c_emul u B + 2u E (+ the kernel's half terms in fp16 mode),

on the data of tests/attn_row_cases.py: N = 2, H = 4, a flat ("even") and a peaked softmax, both run as two requests on one model.  In every case the
plan's tile (and splits) and the launched kernel label are asserted, every element of every row whose own key is valid is held to the bound, the
other rows are checked finite, and c = max |y - ref| / (u B) (fp16: of what is left beyond the half terms) is printed per (image, kind of row).  The appended K / V rows are held to
attn_ref.appended_check: v and an unrotated k bit for bit, a rotated k within 2u of its magnitude; every other cache row bit for bit.

The cases that exist today (tests/test_kv_cache_gpu.py, test_extend_gpu.py, test_rope_attention_gpu.py, test_attention_stream_causal_gpu.py) are
re-measured; the in-place cases (a model bound to a B.KvCache whose rows beyond `len` are NaN) are new: tile 5 at three splits and over more than one
row block, c = 0 in an extend and in a decode step, tile 4 at three splits over an empty image."""
import numpy as np
import pytest

import attn_ref as AR
import attn_row_cases as RC
import attn_stream_causal_graphs as SC
import extend_graphs as EG
import kv_graphs as KG
import llama_graphs as LG
import resident_graphs as RG
from engine_run import plan_of
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models

pytestmark = pytest.mark.gpu
N, H = RC.N, RC.H
PRECS = ("fp32", "fp16")


def _groups(case, st):
    """{name: [N, Lq] bool} of the rows that are held to the bound, per image and kind of row"""
    own = AR.own_key_valid(st)
    if case.form == "prefill":
        i = np.arange(case.lq)[None, :]
        g = {"first 32": own & (i < 32), "last 32": own & (i >= case.lq - 32)}
        if case.lq > 64:
            g["between"] = own & (i >= 32) & (i < case.lq - 32)
        return g
    return {f"image {n}": own & (np.arange(N)[:, None] == n) for n in range(N)}


def _hold(y, case, kind, prec, tile, splits, what):
    """every valid row of y within the bound, the rest finite; prints c per group.  c_emul of a tile 4 case includes the key-slot form"""
    st = case.step(kind, prec)
    r, ce, _ = case.yard(kind, prec, splits, KG.key_tile(case.hd) if tile == KG.DECODE_TILE else 0)
    yr = RC.out_rows(y, case)
    assert np.isfinite(yr).all(), (what, "out is not finite")
    extra = AR.half_allowance(r, tile, st.rope) if prec == "fp16" else 0.0
    for name, rows in _groups(case, st).items():
        if rows.any():
            print(f"ATTN_ROWS {what} | {kind} | {name}: c {AR.c_stat(yr, r, rows, extra):.2f} c_emul {ce:.2f} of the bound {AR.worst_ratio(yr, r, ce, rows, extra):.3f}")
    worst = AR.worst_ratio(yr, r, ce, AR.own_key_valid(st), extra)
    assert worst <= 1.0, (what, kind, worst)


def _appended(case, kind, prec, got_k, got_v, what):
    """got_k / got_v [N, Hkv, >= c, hd]: the rows a kernel appended for the image's first c new tokens"""
    st = case.step(kind, prec)
    for n, c in enumerate(case.new[kind]):
        ok, worst = AR.appended_check(st, got_k[n, :, :c], got_v[n, :, :c], n, c)
        print(f"ATTN_ROWS {what} | {kind} | image {n}: {c} appended rows, rotated k within {worst:.2f} u of its magnitude")
        assert ok, (what, kind, n, worst)


def _label(bound, lq, tile, f16, hd, splits):
    if bound:
        return RG.decode_label(tile, f16, hd, splits) if lq == 1 else RG.extend_label(tile, f16, hd, splits)
    return KG.decode_label(tile, f16, hd, splits) if lq == 1 else EG.extend_label(tile, f16, hd, splits)


def _env(prec, tile, splits):
    return dict(IE_PRECISION=prec, IE_ATTN_TILE=str(tile), **({"IE_ATTN_SPLITS": str(splits)} if tile else {}))


def _plan(path, env, tile, splits, past, lq):
    (at,) = [s for s in plan_of(path, N, env)["steps"] if s["kind"] == "attention"]
    assert (at["tile"], at["past_len"], at.get("new_len", 1)) == (tile, past, lq), at
    if tile:
        assert at["splits"] == splits, at


def _client_held(tmp_path, case, prec, tile, splits=1):
    """the graph with past_key_values inputs and present outputs: both data kinds on one model"""
    past, lq, hd, kvh = case.past, case.lq, case.hd, case.kvh
    path = models.write_repo(str(tmp_path), "m", case.mb)
    env = _env(prec, tile, splits)
    _plan(path, env, tile, splits, past, lq)
    outs = {"out": (N, lq, H * hd), "present.0.key": (N, kvh, past + lq, hd), "present.0.value": (N, kvh, past + lq, hd)}
    what = f"{'decode' if lq == 1 else 'extend'} tile {tile} hd {hd} H {H}/{kvh} P {past} Lq {lq} S {splits} {prec}"
    with RG.session(env, {"m": path}) as (ms, _):
        for kind in RC.KINDS:
            f = case.feeds[kind]
            ys = RG.request(ms["m"], f, outs)
            for w in ("key", "value"):
                assert np.array_equal(ys[f"present.0.{w}"][:, :, :past], f[f"past_key_values.0.{w}"]), (what, kind, w, "rows < P are not the past, bit for bit")
            _appended(case, kind, prec, ys["present.0.key"][:, :, past:], ys["present.0.value"][:, :, past:], what)
            _hold(ys["out"], case, kind, prec, tile, splits, what)
        kern = [p["kernel"] for p in B.Profile(ms["m"], 1)]
    assert _label(False, lq, tile, prec == "fp16", hd, splits) in kern, kern


def _resident(tmp_path, case, prec, tile, splits=1):
    """the model bound to a B.KvCache of case.past rows, NaN beyond every image's length: both data kinds on one model and one cache"""
    past, lq, hd, kvh = case.past, case.lq, case.hd, case.kvh
    path = models.write_repo(str(tmp_path), "m", case.mb)
    env = _env(prec, tile, splits)
    _plan(path, env, tile, splits, past, lq)
    what = f"resident {'decode' if lq == 1 else 'extend'} tile {tile} hd {hd} H {H}/{kvh} cache {past} Lq {lq} S {splits} {prec}"
    with RG.session(env, {"m": path}, (1, N, kvh, past, hd)) as (ms, kc):
        for kind in RC.KINDS:
            lens, new = case.lens[kind], case.new[kind]
            written = RG.fill(kc, case.feeds[kind], lens)
            y = RG.request(ms["m"], RG.unbound(case.feeds[kind]), {"out": (N, lq, H * hd)})["out"]
            got = [kc.read(0, 0), kc.read(0, 1)]
            for which in (0, 1):
                for n, (ln, c) in enumerate(zip(lens, new)):
                    was = written[(0, which)]
                    assert np.array_equal(RG.bits(got[which][n, :, :ln]), RG.bits(was[n, :, :ln])), (what, kind, which, n, "rows below len changed")
                    assert np.array_equal(RG.bits(got[which][n, :, ln + c:]), RG.bits(was[n, :, ln + c:])), (what, kind, which, n, "rows beyond the appended ones changed")
            assert kc.lengths() == [ln + c for ln, c in zip(lens, new)], (what, kind, kc.lengths())
            rows = max(new)
            app = [np.stack([np.pad(g[n, :, ln:ln + c], ((0, 0), (0, rows - c), (0, 0))) for n, (ln, c) in enumerate(zip(lens, new))]) for g in got]
            _appended(case, kind, prec, app[0], app[1], what)
            _hold(y, case, kind, prec, tile, splits, f"{what} len {lens} c {new}")
        kern = [p["kernel"] for p in B.Profile(ms["m"], 1)]
    label = _label(True, lq, tile, prec == "fp16", hd, splits)
    assert label in kern and "inplace" in label, (label, kern)


# ---- the cases that exist today, per element -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("tile", (0, KG.DECODE_TILE))
@pytest.mark.parametrize("kvh, hd, past", RC.DECODE)
def test_decode(tmp_path, kvh, hd, past, tile, prec):
    """hd 32, 64, 128 at (H, Hkv) = (4, 4) and (4, 1), P = the key tile - 1 and + 1"""
    _client_held(tmp_path, RC.cache_case(kvh, hd, past, 1, *RC.lens_pair(past)), prec, tile)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("tile, splits", ((0, 1), (4, 1), (4, 3)))
def test_decode_long_cache(tmp_path, tile, splits, prec):
    _client_held(tmp_path, RC.cache_case(2, 64, 200, 1, *RC.lens_pair(200)), prec, tile, splits)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("tile", (0, EG.EXTEND_TILE))
@pytest.mark.parametrize("hd, past, lq", RC.EXTEND)
def test_extend(tmp_path, hd, past, lq, tile, prec):
    """hd 32 and 64; P round a key tile and the 256-key chunk at Lq = 5; 130 query rows (two row blocks) at (40, 65)"""
    _client_held(tmp_path, RC.cache_case(2, hd, past, lq, *RC.lens_pair(past)), prec, tile)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("tile, splits", ((0, 1), (5, 1), (5, 3)))
def test_extend_long_cache(tmp_path, tile, splits, prec):
    _client_held(tmp_path, RC.cache_case(2, 64, 300, 8, *RC.lens_pair(300)), prec, tile, splits)


@pytest.mark.parametrize("prec", PRECS)
def test_extend_a_split_beyond_the_causal_limit(tmp_path, prec):
    """P = 40, Lq = 64 at three splits over four key tiles: nobody has a key in the third"""
    _client_held(tmp_path, RC.cache_case(2, 64, 40, 64, *RC.lens_pair(40)), prec, 5, 3)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("tile, kvh, hd, l", RC.PREFILL)
def test_causal_rope_prefill(tmp_path, tile, kvh, hd, l, prec):
    """tile 1 at L = 40 and 129, tile 3 pinned at L = 264, tile 2 pinned at hd 128 and L = 40; the rows in groups of the first and the last 32"""
    case = RC.prefill_case(kvh, hd, l)
    path = models.write_repo(str(tmp_path), "m", case.mb)
    env = dict(IE_PRECISION=prec, **({} if tile == 1 else {"IE_ATTN_TILE": str(tile)}))
    if tile == 1:
        assert LG.rope_default_tile(l, hd, H, kvh, prec == "fp16") == 1
    (at,) = [s for s in plan_of(path, N, env)["steps"] if s["kind"] == "attention"]
    assert at["tile"] == tile and at.get("rope", False) and at.get("causal", False) and at.get("kv_heads", H) == kvh, at
    what = f"prefill tile {tile} hd {hd} H {H}/{kvh} L {l} {prec}"
    with RG.session(env, {"m": path}) as (ms, _):
        for kind in RC.KINDS:
            y = RG.request(ms["m"], case.feeds[kind], {"y": (N, H * hd, 1, l)})["y"]
            _hold(y, case, kind, prec, tile, 1, what)
        kern = [p["kernel"] for p in B.Profile(ms["m"], 1)]
    assert SC.attn_label(tile, prec == "fp16", hd, True, True) in kern, kern


# ---- in place: a model bound to a resident cache -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("lens", ((3, 292), (255, 256), (257, 290)))
def test_resident_extend_three_splits(tmp_path, lens, prec):
    """attention_extend_kernel<.., true> at S = 3 and its combine, a cache of 300 rows, Lq = 8.  (3, 292): image 0 has 11 keys, one key tile, so its
    second and third splits hold nothing and write (-FLT_MAX, 0, 0); (255, 256) and (257, 290): the lengths round the 256-key chunk"""
    _resident(tmp_path, RC.cache_case(2, 64, 300, 8, lens, lens), prec, 5, 3)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("splits", (1, 3))
def test_resident_extend_two_row_blocks(tmp_path, splits, prec):
    """Lq = 65 at g = 2: 130 query rows, a second row block of 2 rows, lens (3, 40) in a cache of 110 rows"""
    _resident(tmp_path, RC.cache_case(2, 64, 110, 65, (3, 40), (3, 40)), prec, 5, splits)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("tile", (0, 5))
@pytest.mark.parametrize("lens", ((7, 30), (0, 30)))
def test_resident_extend_appends_nothing_for_one_image(tmp_path, lens, tile, prec):
    """c = (0, 5): all of image 0's new tokens are padded.  Its output is finite, its cache untouched, its length unchanged (_resident checks every row
    outside the c appended ones bit for bit); image 1 is within the bound.  lens (0, 30): nothing at all is visible to image 0"""
    _resident(tmp_path, RC.cache_case(2, 64, 40, 5, lens, lens, new=(0, 5)), prec, tile)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("tile", (0, 4))
@pytest.mark.parametrize("ln", (7, 0))
def test_resident_decode_appends_nothing_for_one_image(tmp_path, ln, tile, prec):
    """a decode step whose image 0 is a padded token (c = 0) over 7 cached rows and over none"""
    _resident(tmp_path, RC.cache_case(2, 64, 40, 1, (ln, 30), (ln, 30), new=(0, 1)), prec, tile)


@pytest.mark.parametrize("prec", PRECS)
def test_resident_decode_three_splits_over_an_empty_image(tmp_path, prec):
    """tile 4 in place at S = 3, lens (0, 199) in a cache of 200: image 0 has no key tile (per = 0), its last split owns the new row"""
    _resident(tmp_path, RC.cache_case(2, 64, 200, 1, (0, 199), (0, 199)), prec, 4, 3)
