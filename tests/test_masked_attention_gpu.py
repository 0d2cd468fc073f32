"""GPU (-m gpu): the key-masked attention kernels on the MI355X against the float64 walk of tests/ref64.py, with the project's bounds
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

import numpy as np
import pytest

import bert_graphs as G
from engine_run import plan_of, RTOL, run_model
from gpu_ai_inference_server_amd.modelgen import models

pytestmark = pytest.mark.gpu
LMAX = {prec: G.max_masked_mfma_tokens(64, prec == "fp16") for prec in RTOL}
SHAPES = [(2, 5, 1, 32), (2, 33, 3, 64), (1, 129, 2, 64), (2, 7, 2, 20)]


def _case(tmp_path, n, l, h, hd, kind, c, prec, **graph_kw):
    path = models.write_repo(str(tmp_path), "mattn", G.masked_attn_graph(n, l, h, hd, mask_value=c, **graph_kw))
    masks, idx = G.mask_requests(n, l)
    feeds = [{"x": np.array(G.masked_input(n, l, h, hd, kind, tuple(r))), "attention_mask": np.array(mk)} for mk, r in zip(masks, idx)]
    f16 = prec == "fp16"
    ran = []
    for forced in (None, 0, 1):
        env = dict(IE_PRECISION=prec, **({} if forced is None else {"IE_FORCE_TILE": str(forced)}))
        steps = plan_of(path, n, env)["steps"]
        (at,) = [s for s in steps if s["kind"] == "attention"]
        assert at["key_mask"] is True and at["in2"]["i64"] and at["mask_value"] == float(np.float32(np.finfo(np.float32).min if c == "min" else c))
        if forced is not None and at["tile"] != forced:
            assert at["tile"] == 0
            continue
        ys, kern = run_model(path, "mattn", env, feeds, "y", (n, h * hd, 1, l))
        (label,) = [k for k in kern if k.startswith("attention_")]
        assert label == G.masked_attn_label(at["tile"], f16, hd), (forced, at["tile"], label)
        worst = 0.0
        for y, r in zip(ys, idx):
            assert np.isfinite(y).all(), (kind, c, at["tile"], r)
            ref = G.masked_reference(n, l, h, hd, kind, c, tuple(r))
            err = float(np.abs(y - ref).max() / np.abs(ref).max())
            worst = max(worst, err)
            assert err < RTOL[prec], (n, l, h, hd, kind, c, prec, at["tile"], list(r), err)
        print(f"N {n} L {l} H {h} hd {hd} {kind} c {c} {prec} {graph_kw or ''} forced {forced} tile {at['tile']}: max err / max|ref| {worst:.3e}")
        ran.append(at["tile"])
    mfma = G.masked_attn_mfma_ok(l, hd, h * hd, f16)
    assert sorted(set(ran)) == ([0, 1] if mfma else [0]) and ran[0] == int(mfma), ran


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("c", G.MASK_VALUES, ids=str)
@pytest.mark.parametrize("kind", G.MASKED_KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_masked_attention(tmp_path, shape, kind, c, prec):
    _case(tmp_path, *shape, kind, c, prec)


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("c", G.MASK_VALUES, ids=str)
@pytest.mark.parametrize("kind", G.MASKED_KINDS)
@pytest.mark.parametrize("past", [0, 1])
def test_masked_attention_at_the_lds_budget(tmp_path, past, kind, c, prec):
    """L = the largest sequence the masked MFMA kernel takes at hd = 64 (288 in fp32, 544 in fp16: the unmasked limits) and one more (generic only)"""
    assert LMAX == {"fp32": 288, "fp16": 544}
    _case(tmp_path, 1, LMAX[prec] + past, 1, 64, kind, c, prec)


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("kw", [dict(unsqueeze="one"), dict(ktrans="one"), dict(scale="mul"), dict(mask_swap=True)], ids=lambda k: "-".join(map(str, *k.items())))
def test_spellings(tmp_path, kw, prec):
    _case(tmp_path, 2, 33, 3, 64, "randn", "min", prec, **kw)
