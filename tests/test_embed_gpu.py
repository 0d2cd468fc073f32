"""GPU (-m gpu): the embed kernels (token + type + position embedding and the LayerNormalization behind them, one step) on the MI355X against the
float64 walk of tests/ref64.py, with the project's bounds (tests/test_gpu_parity.py): fp32 within 2e-4 of max|ref|, fp16 within 3e-3.

Graph: input_ids (, token_type_ids) [N, L] INT64 -> the embedding sum -> LayerNormalization -> Transpose [0,2,1] -> Reshape [N, D, 1, L] -> y, so every
token row the step writes reaches the output.  Every case runs on the planner's default tile and on every forced tile the plan accepts
(IE_FORCE_TILE 0 ... 4), and the Profile label must be the kernel the plan's tile names.

Shapes (N, L, V, D): D = 8 (one vector per lane in fp32 and fp16); D = 20 (whole fp32 vectors, no whole half vector: fp16 runs the generic kernel);
D = 7 (generic only); D = 768 (BERT's own width: three vectors per lane on the 64-lane group in fp32); D = 3080 (past the register budget of the
widest group in both precisions: generic only).
Ids: 0, V - 1, -1 (= V - 1), -V (= 0), repeats; type ids of both rows.  Tables: randn, and mean 100 / std 1 (the variance of the centred values
survives; E[x^2] - mean^2 would not)."""

import numpy as np
import pytest

import bert_graphs as G
import ref64
from engine_run import plan_of, RTOL, run_model, tensor, with_env
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models

pytestmark = pytest.mark.gpu
SHAPES = [(2, 5, 37, 8), (2, 5, 37, 20), (1, 3, 5, 7), (2, 4, 11, 768), (1, 3, 5, 3080)]


def _tensors(ids, tt, types):
    return [tensor(k, v) for k, v in G.embed_feeds(ids, tt, types).items()]


def _case(tmp_path, n, l, v, d, kind, prec, types=2, pos="const"):
    mb, ref = G.embed_graph_and_reference(n, l, v, d, kind, types, pos)
    path = models.write_repo(str(tmp_path), "embed", mb)
    ids, tt = G.make_ids(n, l, v, types)
    f16 = prec == "fp16"
    ran = []
    for forced in (None, 0, 1, 2, 3, 4):
        env = dict(IE_PRECISION=prec, **({} if forced is None else {"IE_FORCE_TILE": str(forced)}))
        steps = plan_of(path, n, env)["steps"]
        assert [s["kind"] for s in steps] == ["embed", "copy"]
        em = steps[0]
        assert em["out"]["f16"] == f16 and em["tables"] == (2 if types else 1) and em["vocab"] == ([v, types] if types else [v])
        if forced is None:
            assert em["tile"] == G.embed_default_tile(d, f16), (d, prec, em["tile"])
        elif em["tile"] != forced:
            assert em["tile"] == 0 and not G.embed_tile_fits(d, f16, forced)        # not eligible: the generic kernel, which forced tile 0 runs
            continue
        y, kern = run_model(path, "embed", env, G.embed_feeds(ids, tt, types), "y", (n, d, 1, l))
        assert kern == [G.embed_label(em["tile"], f16), "copy_kernel"], (forced, em["tile"], kern)
        assert np.isfinite(y).all()
        err = ref64.rel_err(y, ref)
        print(f"N {n} L {l} V {v} D {d} {kind} {prec} types {types} pos {pos} forced {forced} tile {em['tile']}: max err / max|ref| {err:.3e}")
        assert err < RTOL[prec], (n, l, v, d, kind, prec, em["tile"], err)
        ran.append(em["tile"])
    want = sorted({0} | {t for t in range(1, 5) if G.embed_tile_fits(d, f16, t)})
    assert sorted(set(ran)) == want, (ran, want)


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("kind", list(G.TABLE_MEANS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_embed(tmp_path, shape, kind, prec):
    _case(tmp_path, *shape, kind, prec)


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("pos", ["const", "gather", None])
@pytest.mark.parametrize("types", [2, 0])
def test_embed_variants(tmp_path, types, pos, prec):
    """with and without the type gather, with the position rows as a constant, as Gather + Slice, and without them"""
    _case(tmp_path, 2, 5, 37, 8, "randn", prec, types=types, pos=pos)


def test_out_of_range_id_is_refused(tmp_path):
    """ModelInfer names the input, the position, the value and the range; nothing ran, and the model answers the next valid request"""
    n, l, v, d = 2, 5, 37, 8
    mb, ref = G.embed_graph_and_reference(n, l, v, d, "randn", 2, "const")
    path = models.write_repo(str(tmp_path), "embed", mb)
    ids, tt = G.make_ids(n, l, v)
    out = [B.OutputConfig("y", Shape=[n, d, 1, l], DataType="FLOAT32")]

    def go():
        m = B.CreateModel(path, "embed")
        try:
            for bad, where in ((v, (1, 2)), (-v - 1, (0, 4))):
                x = ids.copy()
                x[where] = bad
                with pytest.raises(RuntimeError, match=r"Index out of range for input: input_ids at position \[%d, %d\]: value %d is outside the valid range \[-37, 36\]" % (*where, bad)):
                    m.Infer(_tensors(x, tt, 2), out)
            x = tt.copy()
            x[1, 0] = 2
            with pytest.raises(RuntimeError, match=r"Index out of range for input: token_type_ids at position \[1, 0\]: value 2 is outside the valid range \[-2, 1\]"):
                m.Infer(_tensors(ids, x, 2), out)
            y = m.Infer(_tensors(ids, tt, 2), out)[0].Data.reshape(n, d, 1, l)
            assert ref64.rel_err(y, ref) < RTOL["fp32"]
        finally:
            m.Destroy()
    with_env(dict(IE_AUTOTUNE="0", IE_PRECISION="fp32"), go)
