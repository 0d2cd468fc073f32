"""GPU (-m gpu): a narrow Llama on the MI355X against the float64 walk of tests/ref64.py with the project's bounds (tests/engine_run.py RTOL: fp32
within 2e-4 of max|ref|, fp16 within 3e-3): depth 2, dim 128, 2 heads of 64 over 1 K / V head, mlp 256, vocab 61, N = 2; logits and last_hidden_state
come back through ModelInfer as rank-3 outputs.  seq 40 runs on the default tile 1, seq 264 under IE_ATTN_TILE=3 (the second chunk's keys are rotated at
their global position inside a model).

What the half format alone costs this model is pinned on the CPU by tests/test_llama_plan.py test_fp16_format_cost_of_the_narrow_model."""
import functools

import numpy as np
import pytest

import bert_graphs as BG
import gpt2_graphs as GG
import llama_graphs as LG
import ref64
from engine_run import RTOL, tensor, with_env
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models

pytestmark = pytest.mark.gpu
PRECS = ("fp32", "fp16")
N, V, D = 2, 61, 128


@functools.lru_cache(maxsize=None)
def _narrow(seq):
    """the graph, its ids and the float64 outputs, computed once; read-only"""
    mb = LG.narrow_llama(N, seq=seq, max_pos=seq + 8)
    ids = GG.gpt2_ids(N, seq, V)
    ref = ref64.run_f64(mb, {"input_ids": ids})
    for r in ref.values():
        r.setflags(write=False)
    return mb, ids, ref


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("seq, env, tile", [(40, {}, 1), (LG.KC + 8, {"IE_ATTN_TILE": "3"}, 3)], ids=("seq40", "seq264_tile3"))
def test_narrow_llama_vs_float64(tmp_path, seq, env, tile, prec):
    mb, ids, ref = _narrow(seq)
    path = models.write_repo(str(tmp_path), "llama", mb)
    env = dict(IE_PRECISION=prec, **env)
    outs = {"logits": (N, seq, V), "last_hidden_state": (N, seq, D)}
    ys, shapes, kern = GG.run_outputs(path, "llama", env, {"input_ids": ids}, outs)
    assert shapes == {k: list(s) for k, s in outs.items()}
    f16 = prec == "fp16"
    assert kern[0] == GG.embed_sum_label(BG.embed_default_tile(D, f16), f16), kern
    assert kern.count(LG.attn_label(tile, f16, 64, True, True)) == 2 and not any(k.startswith("attention_generic") for k in kern), kern
    assert kern.count(LG.rms_label(LG.CG.ln_default_tile(D, f16), f16)) == 5 and not any(k.startswith("layernorm") for k in kern), kern
    assert kern.count("eltwise_kernel") == 2                  # the two gated units; every residual Add rides in a projection's epilogue
    for k in outs:
        assert np.isfinite(ys[k]).all()
        err = ref64.rel_err(ys[k], ref[k])
        print(f"narrow Llama seq {seq} {prec} tile {tile} {k}: max err / max|ref| {err:.3e}")
        assert err < RTOL[prec], (k, prec, err)


def test_rows_of_a_token_output_per_image(tmp_path):
    """image 1 of the N = 2 answer is the N = 1 answer for those ids"""
    mb, ids, ref = _narrow(40)
    outs2, outs1 = {"logits": (2, 40, V)}, {"logits": (1, 40, V)}
    y2, _, _ = GG.run_outputs(models.write_repo(str(tmp_path), "l2", mb), "l2", dict(IE_PRECISION="fp32"), {"input_ids": ids}, outs2)
    y1, s1, _ = GG.run_outputs(models.write_repo(str(tmp_path), "l1", LG.narrow_llama(1, seq=40, max_pos=48)), "l1", dict(IE_PRECISION="fp32"), {"input_ids": ids[1:]}, outs1)
    assert s1 == {"logits": [1, 40, V]}
    assert ref64.rel_err(y1["logits"][0], ref["logits"][1]) < RTOL["fp32"] and ref64.rel_err(y2["logits"][1], y1["logits"][0]) < RTOL["fp32"]


def test_out_of_range_id_is_refused(tmp_path):
    """ModelInfer names the input, the position, the value and the range before anything is enqueued; the model answers the next valid request"""
    mb, ids, ref = _narrow(40)
    path = models.write_repo(str(tmp_path), "llama", mb)
    out = [B.OutputConfig("logits", Shape=[N, 40, V], DataType="FLOAT32")]

    def go():
        m = B.CreateModel(path, "llama")
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
