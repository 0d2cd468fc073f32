"""GPU (-m gpu): a narrow Llama with heads of 128 on the MI355X against the float64 walk of tests/ref64.py with the project's bounds
(tests/engine_run.py RTOL: fp32 within 2e-4 of max|ref|, fp16 within 3e-3): depth 2, dim 256, 2 heads of 128 over 1 K / V head, mlp 512, vocab 61,
N = 2; logits and last_hidden_state.  seq 40 runs under IE_ATTN_TILE=2, seq kAttnStreamCausalMinTokens + 8 on the default tile; both attention steps
must report the rotary form of the streaming kernel.

What the half format alone costs this model is pinned on the CPU by
tests/test_attention_stream_causal_plan.py::test_fp16_format_cost_of_the_narrow_model_with_heads_of_128."""
import functools

import numpy as np
import pytest

import attn_stream_causal_graphs as SC
import gpt2_graphs as GG
import ref64
from engine_run import plan_of, RTOL
from gpu_ai_inference_server_amd.modelgen import models

pytestmark = pytest.mark.gpu
PRECS = ("fp32", "fp16")
N, V, D, HD = 2, 61, 256, 128


@functools.lru_cache(maxsize=None)
def _narrow(seq):
    """the graph, its ids and the float64 outputs, computed once; read-only"""
    mb = SC.narrow_llama_hd128(N, seq=seq, max_pos=seq + 8)
    ids = GG.gpt2_ids(N, seq, V)
    ref = ref64.run_f64(mb, {"input_ids": ids})
    for r in ref.values():
        r.setflags(write=False)
    return mb, ids, ref


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("seq, env", [(40, {"IE_ATTN_TILE": "2"}), (SC.CAUSAL_MIN_TOKENS + 8, {})], ids=("seq40_pinned", "default"))
def test_narrow_llama_hd128_vs_float64(tmp_path, seq, env, prec):
    mb, ids, ref = _narrow(seq)
    path = models.write_repo(str(tmp_path), "llama", mb)
    env = dict(IE_PRECISION=prec, **env)
    f16 = prec == "fp16"
    ats = [s for s in plan_of(path, N, env)["steps"] if s["kind"] == "attention"]
    assert [(s["tile"], s["rope"], s["causal"], s["kv_heads"], s["head_dim"]) for s in ats] == 2 * [(2, True, True, 1, HD)]
    outs = {"logits": (N, seq, V), "last_hidden_state": (N, seq, D)}
    ys, shapes, kern = GG.run_outputs(path, "llama", env, {"input_ids": ids}, outs)
    assert shapes == {k: list(s) for k, s in outs.items()}
    assert kern.count(SC.attn_label(2, f16, HD, True, True)) == 2 and not any(k.startswith("attention_generic") for k in kern), kern
    for k in outs:
        assert np.isfinite(ys[k]).all()
        err = ref64.rel_err(ys[k], ref[k])
        print(f"narrow Llama hd 128 seq {seq} {prec} {k}: max err / max|ref| {err:.3e}")
        assert err < RTOL[prec], (k, prec, err)
