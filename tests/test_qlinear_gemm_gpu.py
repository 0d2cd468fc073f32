"""GPU: tile 2 of the 4-bit Linear family (qlinear_gemm_kernel) element by element against float64 on the dense twin's weights, the row
count at which the planner takes it, and an int4 Llama prefill pinned to it.

The bound is test_qlinear_gpu's fp16 one, |y - ref| <= (2^-10 + 2^-22 + K 2^-24) S + 2^-11 |ref|, unchanged: the weights are rounded exactly as in tile 1,
the sum is fp32 and the result is rounded once.  The tile is 128 rows x 128 columns and a K-step is 64, so the covering list takes rows 1 / 128 / 129 /
328 (one live row, a full tile, one row into a second block, three blocks with a partial last), N 80 / 960 (narrower than a tile with an odd count of
16-column groups; eight tiles with a half-empty last) and K 128 / 576 (two steps, nine steps) plus the two edges of this K-step: 64 (ONE step: nothing
is prefetched) and 96 (one step plus 32: the second step's upper half is past K).  Blocks 32 / 64 / 128, with and without zero points and residual."""
import numpy as np
import pytest

import kv_graphs as KG
import resident_graphs as RG
import test_resident_cache_gpu as TRC
from engine_run import run_model
from gpu_ai_inference_server_amd.modelgen import models
from test_qlinear_gpu import _bound, _case, _codes  # noqa: F401  (_codes: what _case draws the operands with)

MIN_ROWS = 4096     # kernels.h kQLinearGemmMinRows
#        rows, K,  N,  block, zero points, residual
CASES = [(1, 128, 80, 32, True, False), (128, 576, 960, 64, False, True), (129, 128, 960, 128, True, True), (328, 576, 80, 32, False, False),
         (328, 128, 960, 64, True, False), (128, 128, 80, 128, False, True), (129, 576, 80, 32, True, True), (1, 576, 960, 64, False, True),
         (129, 96, 80, 32, True, True), (128, 64, 960, 64, True, False), (328, 96, 960, 32, False, False)]
DEFAULT = [(MIN_ROWS, 576, 960, 32, True, False), (MIN_ROWS - 1, 576, 960, 32, True, False)]


def _run(tmp_path, case, label, env):
    rows, k, n, block, zero, _ = case
    feeds, ref, S, mb, _ = _case(case)
    (y, again), kern = run_model(models.write_repo(str(tmp_path), "q", mb), "q", dict(IE_PRECISION="fp16", **env), [feeds, feeds], "y", (rows, n))
    assert label + "b%d,%s>" % (block, "zp" if zero else "sym") in kern, (label, kern)
    excess = np.abs(y - ref) / _bound("fp16", k, S, ref)
    print(f"{case} {label}: max |y - ref| / bound {excess.max():.3f}")
    assert np.isfinite(y).all() and (excess <= 1.0).all(), float(excess.max())
    assert (RG.bits(y) == RG.bits(again)).all(), "two runs differ"


@pytest.mark.parametrize("case", CASES + DEFAULT, ids=str)
def test_float32_twin_is_inside_the_fp32_bound(case):
    feeds, ref, S, _, w = _case(case)
    y = feeds["x"] @ w.astype(np.float32).T + (feeds["r"] if "r" in feeds else np.float32(0))
    assert (np.abs(y - ref) <= _bound("fp32", case[1], S, ref)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=str)
def test_linear_alone(tmp_path, case):
    _run(tmp_path, case, "qlinear_gemm_kernel<", {"IE_QLINEAR_TILE": "2"})


@pytest.mark.gpu
@pytest.mark.parametrize("case,label", zip(DEFAULT, ("qlinear_gemm_kernel<", "qlinear_mfma_kernel<")), ids=str)
def test_default_selection(tmp_path, case, label):
    """with no pin, tile 2 from kQLinearGemmMinRows rows on and tile 1 one row below"""
    _run(tmp_path, case, label, {})


@pytest.mark.gpu
def test_int4_llama_prefill(tmp_path):
    """the merged qkv, the folded residuals and a token view on tile 2: every qlinear launch of the narrow Llama's prefill"""
    n, v = KG.NARROW_N, KG.NARROW["vocab"]
    ids = np.random.RandomState(3).randint(0, v, (n, 8)).astype(np.int64)
    outs = {"logits": (n, 8, v), **{k: (n, KG.NARROW["kv_heads"], 8, 32) for k in KG.present_names()}}
    path = models.write_repo(str(tmp_path), "s8", KG.narrow(quant="int4", seq=8, present=True))
    with RG.session(dict(IE_PRECISION="fp16", IE_QLINEAR_TILE="2"), {"s8": path}) as (ms, _):
        ref = TRC.ref64.run_f64(KG.narrow(quant="int4", q_form="dense", seq=8, present=True), {"input_ids": ids})
        got = RG.request(ms["s8"], {"input_ids": ids}, outs)
        ql = [s for s in TRC._kernels(ms["s8"]) if "qlinear" in s]
        assert len(ql) == 5 * KG.NARROW["depth"] and all("qlinear_gemm_kernel<" in s for s in ql), ql
        for k in outs:
            TRC._close(got[k].reshape(n, -1, got[k].shape[-1]), ref[k].reshape(n, -1, ref[k].shape[-1]), "fp16", f"int4 llama on tile 2, prefill {k}")
