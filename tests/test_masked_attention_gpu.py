"""GPU (-m gpu): the key-masked attention kernels on the MI355X against the float64 walk of tests/bert_ref.py, with the project's bounds
(tests/test_attention_gpu.py): fp32 within 2e-4 of max|ref|, fp16 within 3e-3.

Graph (tests/bert_graphs.py masked_attn_graph): x [N, 3 D, 1, L] -> tokens -> BERT's attention (separate q / k / v Linears that select their third of the
row, the key mask of attention_mask [N, L]) -> y [N, D, 1, L].  Every case runs on the planner's default tile and on every forced tile the plan accepts
(IE_FORCE_TILE 0 / 1), and the Profile label must be the kernel the plan's tile names.

Shapes (N, L, H, hd): (2, 5, 1, 32), (2, 33, 3, 64), (1, 129, 2, 64), (2, 7, 2, 20) generic only, the largest masked L inside the MFMA kernel's LDS
budget per precision (288 / 544 at hd 64) and the first past it (generic only).
Data: randn and peaked (integer k in [-2, 2], q = 16 k + 16: scores of several hundred).  Every q has a component along the all-ones vector and the keys
a mask row hides are multiples of it, so the hidden keys hold the largest raw scores: a dropped mask is far outside the bound (checked on the CPU).
Mask rows, dealt over the images of as many requests as it takes: all ones; lengths 1, 31, 32, 33 and L; a hole in the middle; fully masked.
c = finfo(float32).min and -10000.  Outputs are finite everywhere."""
import functools
import os

import numpy as np
import pytest

import bert_graphs as G
import bert_ref
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models

pytestmark = pytest.mark.gpu
RTOL = {"fp32": 2e-4, "fp16": 3e-3}
KINDS = ("randn", "peaked")
CS = ("min", -10000.0)
LMAX = {prec: G.max_masked_mfma_tokens(64, prec == "fp16") for prec in RTOL}
SHAPES = [(2, 5, 1, 32), (2, 33, 3, 64), (1, 129, 2, 64), (2, 7, 2, 20)]


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def mask_rows(l):
    """the eight mask rows of the test, [8, l]"""
    rows = []
    for ln in (1, 31, 32, 33, l):
        r = np.zeros(l, np.int64)
        r[:min(ln, l)] = 1
        rows.append(r)
    hole = np.ones(l, np.int64)
    hole[l // 3: max(l // 3 + 1, 2 * l // 3)] = 0
    return np.stack(rows + [hole, np.zeros(l, np.int64), np.ones(l, np.int64)])


def requests(n, l):
    """the mask rows dealt over requests of n images: [requests, n, l], and per request the index of each image's mask row"""
    rows = mask_rows(l)
    idx = np.arange(8).reshape(8 // n, n)
    return rows[idx], idx


@functools.lru_cache(maxsize=None)
def make_input(n, l, h, hd, kind, row):
    """x [n, 3 D, 1, l] for the images whose mask rows are `row` (a tuple): hidden keys are multiples of the all-ones vector"""
    st = np.random.RandomState(1000 * l + 10 * hd + h + len(kind))
    half = lambda a: a.astype(np.float16).astype(np.float32)  # noqa: E731
    v = half(st.randn(n, h, l, hd))
    if kind == "randn":
        q, k, big = half(st.randn(n, h, l, hd) + 0.5), half(st.randn(n, h, l, hd)), 2.0
    else:
        k = st.randint(-2, 3, size=(n, h, l, hd)).astype(np.float32)
        q, big = 16.0 * k + 16.0, 4.0
    rows = mask_rows(l)
    for i, r in enumerate(row):
        if rows[r].any():                              # (a fully masked image keeps its keys: nothing is hidden from anything)
            k[i][:, rows[r] == 0, :] = big
    x = np.stack([q, k, v], 0).transpose(1, 0, 2, 4, 3).reshape(n, 3 * h * hd, 1, l)
    x = np.ascontiguousarray(x, np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(n, l, h, hd, kind, c, row, masked=True):
    m = mask_rows(l)[list(row)] if masked else np.ones((n, l), np.int64)
    ref = bert_ref.run_f64(G.masked_attn_graph(n, l, h, hd, mask_value=c), {"x": make_input(n, l, h, hd, kind, row), "attention_mask": m})["y"]
    ref.setflags(write=False)
    return ref


def _model_run(path, name, env, feeds, oshape):
    """one model, every request: -> (outputs, launched kernels)"""
    def go():
        m = B.CreateModel(path, name)
        try:
            ys = []
            for x, mask in feeds:
                r = m.Infer([B.TensorData("x", B.DataTypeFloat32, B.Shape(list(x.shape)), x),
                             B.TensorData("attention_mask", B.DataTypeInt64, B.Shape(list(mask.shape)), mask)], [B.OutputConfig("y", Shape=list(oshape), DataType="FLOAT32")])
                ys.append(r[0].Data.reshape(oshape).copy())
            return ys, [p["kernel"] for p in B.Profile(m, 1)]
        finally:
            m.Destroy()
    return _with_env(dict(IE_AUTOTUNE="0", **env), go)


def _case(tmp_path, n, l, h, hd, kind, c, prec, **graph_kw):
    path = models.write_repo(str(tmp_path), "mattn", G.masked_attn_graph(n, l, h, hd, mask_value=c, **graph_kw))
    masks, idx = requests(n, l)
    feeds = [(np.array(make_input(n, l, h, hd, kind, tuple(r))), np.array(mk)) for mk, r in zip(masks, idx)]
    f16 = prec == "fp16"
    ran = []
    for forced in (None, 0, 1):
        env = dict(IE_PRECISION=prec, **({} if forced is None else {"IE_FORCE_TILE": str(forced)}))
        steps = _with_env(env, lambda: B.DescribeModel(path, n)["plan"])["steps"]
        (at,) = [s for s in steps if s["kind"] == "attention"]
        assert at["key_mask"] is True and at["in2"]["i64"] and at["mask_value"] == float(np.float32(np.finfo(np.float32).min if c == "min" else c))
        if forced is not None and at["tile"] != forced:
            assert at["tile"] == 0
            continue
        ys, kern = _model_run(path, "mattn", env, feeds, (n, h * hd, 1, l))
        (label,) = [k for k in kern if k.startswith("attention_")]
        assert label == G.masked_attn_label(at["tile"], f16, hd), (forced, at["tile"], label)
        worst = 0.0
        for y, r in zip(ys, idx):
            assert np.isfinite(y).all(), (kind, c, at["tile"], r)
            ref = reference(n, l, h, hd, kind, c, tuple(r))
            err = float(np.abs(y - ref).max() / np.abs(ref).max())
            worst = max(worst, err)
            assert err < RTOL[prec], (n, l, h, hd, kind, c, prec, at["tile"], list(r), err)
        print(f"N {n} L {l} H {h} hd {hd} {kind} c {c} {prec} {graph_kw or ''} forced {forced} tile {at['tile']}: max err / max|ref| {worst:.3e}")
        ran.append(at["tile"])
    mfma = G.masked_attn_mfma_ok(l, hd, h * hd, f16)
    assert sorted(set(ran)) == ([0, 1] if mfma else [0]) and ran[0] == int(mfma), ran


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("c", CS, ids=str)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_masked_attention(tmp_path, shape, kind, c, prec):
    _case(tmp_path, *shape, kind, c, prec)


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("c", CS, ids=str)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("past", [0, 1])
def test_masked_attention_at_the_lds_budget(tmp_path, past, kind, c, prec):
    """L = the largest sequence the masked MFMA kernel takes at hd = 64 (288 in fp32, 544 in fp16: the unmasked limits) and one more (generic only)"""
    assert LMAX == {"fp32": 288, "fp16": 544}
    _case(tmp_path, 1, LMAX[prec] + past, 1, 64, kind, c, prec)


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("kw", [dict(unsqueeze="one"), dict(ktrans="one"), dict(scale="mul"), dict(mask_swap=True)], ids=lambda k: "-".join(map(str, *k.items())))
def test_spellings(tmp_path, kw, prec):
    _case(tmp_path, 2, 33, 3, 64, "randn", "min", prec, **kw)


def check_a_dropped_mask_is_far_outside_the_bound(kind, c):
    """(run by tests/test_bert_plan.py, on the CPU) float64: ignoring the mask moves every partly masked image by more than 30 x the fp16 bound"""
    n, l, h, hd = 2, 33, 3, 64
    _, idx = requests(n, l)
    for r in idx:
        ref, bare = reference(n, l, h, hd, kind, c, tuple(r)), reference(n, l, h, hd, kind, c, tuple(r), masked=False)
        for i, row in enumerate(r):
            hidden = mask_rows(l)[row]
            if hidden.all() or not hidden.any():
                continue
            moved = float(np.abs(bare[i] - ref[i]).max() / np.abs(ref).max())
            assert moved > 30 * RTOL["fp16"], (kind, c, row, moved)


def check_fully_masked_rows_are_what_the_graph_gives():
    """(run by tests/test_bert_plan.py, on the CPU) float64: with c = min a fully masked image is the uniform average of V; with c = -10000 the unmasked softmax"""
    n, l, h, hd = 2, 33, 3, 64
    _, idx = requests(n, l)
    (r,) = [r for r in idx if 6 in r]
    i = list(r).index(6)
    x = make_input(n, l, h, hd, "randn", tuple(r)).astype(np.float64)[i, :, 0, :].T.reshape(l, 3, h, hd)
    uniform = x[:, 2].mean(0).reshape(h * hd)
    y = reference(n, l, h, hd, "randn", "min", tuple(r))[i, :, 0, :]
    assert np.abs(y - uniform[:, None]).max() < 1e-12
    y = reference(n, l, h, hd, "randn", -10000.0, tuple(r))[i]
    bare = reference(n, l, h, hd, "randn", -10000.0, tuple(r), masked=False)[i]
    assert np.abs(y - bare).max() < 1e-9
