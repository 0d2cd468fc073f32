"""CPU: which tile the planner gives a 4-bit Linear step by row count, precision and pin (tile 2, qlinear_gemm_kernel: DESIGN 3.39)."""
import pytest

from engine_run import describe
from gpu_ai_inference_server_amd.modelgen import models

MIN_ROWS = 4096     # kernels.h kQLinearGemmMinRows


@pytest.mark.parametrize("rows,prec,env,tile", (
    (MIN_ROWS, "fp16", {}, 2), (MIN_ROWS + 133, "fp16", {}, 2), (MIN_ROWS - 1, "fp16", {}, 1), (8, "fp16", {"IE_QLINEAR_TILE": "2"}, 2),
    (MIN_ROWS, "fp32", {}, 0), (MIN_ROWS, "fp32", {"IE_QLINEAR_TILE": "2"}, 0), (MIN_ROWS, "fp16", {"IE_QLINEAR_TILE": "1"}, 1),
    (MIN_ROWS, "fp16", {"IE_QLINEAR_TILE": "0"}, 0)), ids=str)
def test_tile_by_rows_precision_and_pin(tmp_path, monkeypatch, engine_lib, rows, prec, env, tile):
    plan = describe(models.write_repo(str(tmp_path), "g", models.qlinear(rows, 576, 960, residual=True)), rows, monkeypatch, prec, **env)
    assert [s["tile"] for s in plan["steps"] if s["kind"] == "qlinear"] == [tile]


def test_the_pin_leaves_the_other_steps_alone(tmp_path, monkeypatch, engine_lib):
    path = models.write_repo(str(tmp_path), "g", models.llama_tiny(2, quant="int4", seq=8, present=True))
    plain, pinned = describe(path, 2, monkeypatch, "fp16"), describe(path, 2, monkeypatch, "fp16", IE_QLINEAR_TILE="2")
    assert {s["tile"] for s in plain["steps"] if s["kind"] == "qlinear"} == {1} and {s["tile"] for s in pinned["steps"] if s["kind"] == "qlinear"} == {2}
    assert [s.get("tile") for s in pinned["steps"] if s["kind"] != "qlinear"] == [s.get("tile") for s in plain["steps"] if s["kind"] != "qlinear"]
