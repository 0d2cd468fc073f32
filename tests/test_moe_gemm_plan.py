"""CPU: which tile the planner gives a mixture-of-experts step by mean rows per expert, precision and pin (tile 2, moe_gemm_kernel: DESIGN 3.41)."""
import pytest

import kv_graphs as KG
from engine_run import describe
from gpu_ai_inference_server_amd.modelgen import models

MIN_SLOTS = 64      # kernels.h kMoeGemmMinSlotsPerExpert
E, K = 4, 2
AT = MIN_SLOTS * E // K      # the row count whose mean rows per expert is the constant


def _tiles(plan):
    return [s["tile"] for s in plan["steps"] if s["kind"] == "moe"]


@pytest.mark.parametrize("rows,prec,env,tile", (
    (AT, "fp16", {}, 2), (AT + 133, "fp16", {}, 2), (AT - 1, "fp16", {}, 1), (8, "fp16", {"IE_MOE_TILE": "2"}, 2), (8, "fp16", {"IE_FORCE_TILE": "2"}, 2),
    (AT, "fp32", {}, 0), (AT, "fp32", {"IE_MOE_TILE": "2"}, 0), (AT, "fp16", {"IE_MOE_TILE": "1"}, 1), (AT, "fp16", {"IE_MOE_TILE": "0"}, 0)), ids=str)
def test_tile_by_mean_rows_precision_and_pin(tmp_path, monkeypatch, engine_lib, rows, prec, env, tile):
    d, inter = 64, 96
    plan = describe(models.write_repo(str(tmp_path), "g", models.moe(rows, d, inter, E, K, residual=True)), rows, monkeypatch, prec, **env)
    m = [s for s in plan["steps"] if s["kind"] == "moe"]
    assert [s["tile"] for s in m] == [tile]
    # the activations once (x, r, y and the router row), the min(E, rows * k) experts' weights once: halfs on tiles 1 and 2
    es = 2 if prec == "fp16" else 4
    assert m[0]["bytes"] == es * rows * (3 * d + E) + min(E, rows * K) * 3 * d * inter * (2 if tile >= 1 else 4)


@pytest.mark.parametrize("d,inter", ((48, 96), (64, 40)))
def test_a_width_that_is_no_multiple_of_32_declines_the_pin(tmp_path, monkeypatch, engine_lib, d, inter):
    plan = describe(models.write_repo(str(tmp_path), "g", models.moe(AT, d, inter, E, K)), AT, monkeypatch, "fp16", IE_MOE_TILE="2")
    assert _tiles(plan) == [0]


def test_the_pin_leaves_the_other_steps_alone(tmp_path, monkeypatch, engine_lib):
    path = models.write_repo(str(tmp_path), "g", KG.narrow(experts=4, top_k=2, seq=8, present=True))
    plain, pinned = describe(path, 2, monkeypatch, "fp16"), describe(path, 2, monkeypatch, "fp16", IE_MOE_TILE="2")
    assert set(_tiles(plain)) == {1} and set(_tiles(pinned)) == {2}
    assert [s.get("tile") for s in pinned["steps"] if s["kind"] != "moe"] == [s.get("tile") for s in plain["steps"] if s["kind"] != "moe"]
