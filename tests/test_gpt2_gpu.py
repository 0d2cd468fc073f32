"""GPU (-m gpu): GPT-2 on the MI355X against the float64 walk of tests/ref64.py with the project's bounds (tests/engine_run.py RTOL: fp32 within 2e-4
of max|ref|, fp16 within 3e-3): the embedding sum without a LayerNormalization alone (embed_sum_kernel on every lane-group tile and the generic form),
a narrow GPT-2 whose two token outputs come back through ModelInfer with rank-3 shapes, the same model with tile 3 inside it, and an out-of-range id.

What the half format alone costs the narrow model (tests/test_gpt2_plan.py test_fp16_format_cost_of_the_narrow_model, every stored value rounded to half,
arithmetic in double): logits 4.5e-4 / last_hidden_state 7.9e-4 of max|ref| at seq 40, 5.1e-4 / 9.9e-4 at seq 264: under half of the fp16 bound."""
import functools

import numpy as np
import pytest

import bert_graphs as BG
import gpt2_graphs as GG
import ref64
from engine_run import plan_of, RTOL, tensor, with_env
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models

pytestmark = pytest.mark.gpu
PRECS = ("fp32", "fp16")
N, V, D = 2, 61, 128


@functools.lru_cache(maxsize=None)
def _embed_case(l, v, d, pos):
    """the graph, its ids (0 and V - 1 among them) and the float64 outputs, computed once; read-only"""
    mb = GG.embed_sum_graph(N, l, v, d, pos=pos)
    ids = GG.gpt2_ids(N, l, v)
    ref = ref64.run_f64(mb, {"input_ids": ids})
    for r in ref.values():
        r.setflags(write=False)
    return mb, ids, ref


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("tile", (None, 0, 1, 2, 3, 4))
@pytest.mark.parametrize("l, v, d, pos", [(5, 37, 64, "gather"), (33, 50, 256, "const"), (7, 37, 50, "gather")], ids=("d64", "d256", "d50"))
def test_embed_sum(tmp_path, l, v, d, pos, tile, prec):
    """the sum has two readers (a LayerNormalization and the residual Add), so it is a step of its own: outputs `sum` (the step's result itself, a token
    output) and LayerNormalization(sum) + sum (back as NCHW).  D = 50 is no multiple of a vector: the generic form whatever is forced"""
    mb, ids, ref = _embed_case(l, v, d, pos)
    path = models.write_repo(str(tmp_path), "esum", mb)
    f16 = prec == "fp16"
    env = dict(IE_PRECISION=prec, **({} if tile is None else {"IE_FORCE_TILE": str(tile)}))
    st = plan_of(path, N, env)["steps"][0]
    want = BG.embed_default_tile(d, f16) if tile is None else (tile if tile == 0 or BG.embed_tile_fits(d, f16, tile) else 0)
    assert st["kind"] == "embed" and st["ln"] is False and st["tile"] == want and st["out"]["f16"] is f16
    ys, shapes, kern = GG.run_outputs(path, "esum", env, {"input_ids": ids}, {"sum": (N, l, d), "y": (N, d, 1, l)})
    assert kern[0] == GG.embed_sum_label(want, f16), kern
    assert shapes == {"sum": [N, l, d], "y": [N, d, 1, l]}
    for k in ("sum", "y"):
        assert np.isfinite(ys[k]).all()
        err = ref64.rel_err(ys[k], ref[k])
        print(f"embed sum L {l} V {v} D {d} {prec} tile {want} {k}: max err / max|ref| {err:.3e}")
        assert err < RTOL[prec], (k, err)
    if not f16:      # the fp32 sum of two fp32 rows is the correctly rounded float64 sum
        assert np.array_equal(ys["sum"], ref["sum"].astype(np.float32))


@functools.lru_cache(maxsize=None)
def _narrow(seq):
    mb = GG.narrow_gpt2(N, seq=seq, max_pos=seq + 8)
    ids = GG.gpt2_ids(N, seq, V)
    ref = ref64.run_f64(mb, {"input_ids": ids})
    for r in ref.values():
        r.setflags(write=False)
    return mb, ids, ref


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("seq, env, tile", [(40, {}, 1), (GG.KC + 8, {"IE_ATTN_TILE": "3"}, 3)], ids=("seq40", "seq264_tile3"))
def test_narrow_gpt2_vs_float64(tmp_path, seq, env, tile, prec):
    """depth 2, dim 128, 2 heads of 64, vocab 61, N = 2: logits [2, L, 61] and last_hidden_state [2, L, 128] through ModelInfer, rank 3.  KC + 8 tokens
    still fit tile 1's LDS, so the second case pins tile 3 to run it inside a model"""
    mb, ids, ref = _narrow(seq)
    path = models.write_repo(str(tmp_path), "gpt2", mb)
    env = dict(IE_PRECISION=prec, **env)
    outs = {"logits": (N, seq, V), "last_hidden_state": (N, seq, D)}
    ys, shapes, kern = GG.run_outputs(path, "gpt2", env, {"input_ids": ids}, outs)
    assert shapes == {k: list(s) for k, s in outs.items()}
    f16 = prec == "fp16"
    assert kern[0] == GG.embed_sum_label(BG.embed_default_tile(D, f16), f16)
    assert kern.count(GG.attn_label(tile, f16, 64, True)) == 2 and not any(k.startswith("attention_generic") for k in kern), kern
    for k in outs:
        assert np.isfinite(ys[k]).all()
        err = ref64.rel_err(ys[k], ref[k])
        print(f"narrow GPT-2 seq {seq} {prec} tile {tile} {k}: max err / max|ref| {err:.3e}")
        assert err < RTOL[prec], (k, prec, err)


def test_rows_of_a_token_output_per_image(tmp_path):
    """the row arithmetic of ModelInfer with N >= 2: image 1 of the N = 2 answer is the N = 1 answer for those ids (L * V floats per image)"""
    mb, ids, ref = _narrow(40)
    outs2, outs1 = {"logits": (2, 40, V)}, {"logits": (1, 40, V)}
    y2, _, _ = GG.run_outputs(models.write_repo(str(tmp_path), "g2", mb), "g2", dict(IE_PRECISION="fp32"), {"input_ids": ids}, outs2)
    y1, s1, _ = GG.run_outputs(models.write_repo(str(tmp_path), "g1", GG.narrow_gpt2(1, seq=40, max_pos=48)), "g1", dict(IE_PRECISION="fp32"), {"input_ids": ids[1:]}, outs1)
    assert s1 == {"logits": [1, 40, V]}
    assert ref64.rel_err(y1["logits"][0], ref["logits"][1]) < RTOL["fp32"] and ref64.rel_err(y2["logits"][1], y1["logits"][0]) < RTOL["fp32"]


def test_out_of_range_id_is_refused(tmp_path):
    """ModelInfer names the input, the position, the value and the range before anything is enqueued; the model answers the next valid request"""
    mb, ids, ref = _narrow(40)
    path = models.write_repo(str(tmp_path), "gpt2", mb)
    out = [B.OutputConfig("logits", Shape=[N, 40, V], DataType="FLOAT32")]

    def go():
        m = B.CreateModel(path, "gpt2")
        try:
            for bad, where in ((V, (1, 2)), (-V - 1, (0, 39))):
                x = ids.copy()
                x[where] = bad
                with pytest.raises(RuntimeError, match=r"Index out of range for input: input_ids at position \[%d, %d\]: value %d is outside the valid range \[-61, 60\]" % (*where, bad)):
                    m.Infer([tensor("input_ids", x)], out)
            y = m.Infer([tensor("input_ids", ids)], out)[0].Data.reshape(N, 40, V)
            assert ref64.rel_err(y, ref["logits"]) < RTOL["fp32"]
        finally:
            m.Destroy()
    with_env(dict(IE_AUTOTUNE="0", IE_PRECISION="fp32"), go)
