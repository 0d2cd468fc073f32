"""GPU: tile 2 of the mixture-of-experts step (moe_gemm_up_kernel / moe_gemm_down_kernel) element by element against float64, the mean
row count per expert at which the planner takes it, and a narrow Llama-MoE prefill pinned to it.

The reference and the bound are test_moe_gpu's (moe_f64, u = 2^-11) unchanged: the bound assumes no summation order, so it holds for this tile's K order.
An entry is 128 sorted rows, a K-step 64, a column tile 64 (gated) or 128 columns.  The covering list: one row (ONE K-step, nothing prefetched; a gated
tile plus a 32-column tail; three empty experts); every expert 130 rows (a full entry plus a 2-row one; the plain tile over two column tiles; K = 160 =
two steps + 32; down N = 160 = a tile + a 32 tail; biases); one expert of 129 rows beside experts of 13 to 31 (residual); experts without a token (the -1
entries); K = 96 (one step + 32) with a gated I = 160 (two tiles + a tail) and every bias."""
import numpy as np
import pytest

import kv_graphs as KG
import resident_graphs as RG
import test_resident_cache_gpu as TRC
from engine_run import run_model
from gpu_ai_inference_server_amd.modelgen import models
from test_moe_gpu import IDS, MOE, _case, _walk, moe_f64  # noqa: F401  (moe_f64: what _case computes the reference and the bound with)

MIN_SLOTS = 64      # kernels.h kMoeGemmMinSlotsPerExpert
#        rows, E, k, D,  I,   act,   gated, bias, residual, normalize, routing
CASES = [(1, 4, 1, 64, 96, "silu", True, False, False, True, None), (130, 4, 4, 160, 256, "gelu", False, True, False, False, None),
         (129, 8, 2, 160, 96, "silu", True, False, True, True, "all"), (8, 8, 1, 64, 256, "gelu", False, True, True, False, "skip"),
         (70, 8, 4, 96, 160, "relu", True, True, True, True, None)]
DEFAULT = [(2 * MIN_SLOTS, 4, 2, 64, 96, "silu", True, False, True, True, None), (2 * MIN_SLOTS - 1, 4, 2, 64, 96, "silu", True, False, True, True, None)]


def _run(tmp_path, case, label, env):
    rows, D, act, gated = case[0], case[3], case[5], case[6]
    feeds, mb, refs, _ = _case(case)
    ref, bound = refs[2.0 ** -11]
    label += act + (",gated>" if gated else ",plain>")
    (y, again), kern = run_model(models.write_repo(str(tmp_path), "m", mb), "m", dict(IE_PRECISION="fp16", **env), [feeds, feeds], "y", (rows, D))
    assert label in kern, (label, kern)
    excess = np.abs(y - ref) / bound
    print(f"{case} {label}: max |y - ref| / bound {excess.max():.3f}")
    assert np.isfinite(y).all() and (excess <= 1.0).all(), (label, float(excess.max()))
    assert (RG.bits(y) == RG.bits(again)).all(), label + ": two runs differ"


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=str)
def test_moe_alone(tmp_path, case):
    _run(tmp_path, case, "moe_gemm_kernel<", {"IE_MOE_TILE": "2"})


@pytest.mark.gpu
@pytest.mark.parametrize("case,label", zip(DEFAULT, ("moe_gemm_kernel<", "moe_up_kernel<")), ids=str)
def test_default_selection(tmp_path, case, label):
    """with no pin, tile 2 from kMoeGemmMinSlotsPerExpert mean rows per expert on and tile 1 one row below"""
    _run(tmp_path, case, label, {})


@pytest.mark.gpu
def test_llama_moe_prefill(tmp_path):
    """the folded residual and a token view on tile 2: every moe launch of the narrow Llama-MoE's prefill"""
    n, v = KG.NARROW_N, KG.NARROW["vocab"]
    ref = _walk()[0]
    outs = {"logits": (n, 8, v), **{k: (n, KG.NARROW["kv_heads"], 8, 32) for k in KG.present_names()}}
    path = models.write_repo(str(tmp_path), "s8", KG.narrow(seq=8, present=True, **MOE))
    with RG.session(dict(IE_PRECISION="fp16", IE_MOE_TILE="2"), {"s8": path}) as (ms, _):
        got = RG.request(ms["s8"], {"input_ids": IDS}, outs)
        moe = [s for s in TRC._kernels(ms["s8"]) if "moe_" in s]
        assert len(moe) == KG.NARROW["depth"] and all("moe_gemm_kernel<" in s for s in moe), moe
        for k in outs:
            TRC._close(got[k].reshape(n, -1, got[k].shape[-1]), ref[k].reshape(n, -1, ref[k].shape[-1]), "fp16", f"llama-moe on tile 2, prefill {k}")
