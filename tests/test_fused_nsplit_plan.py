"""CPU: IE_FUSE_PB=6 plans the dense-fused steps of a small DenseNet-shaped graph onto fused tile 6 (the N-split tile of
csrc/kernels_fused.hip) with both parts kept; values the planner does not know leave the default plan as it is."""
import json

import kernel_graphs as G
import test_kernel_maps_gpu as KM
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models


def plan_of(tmp_path, env):
    d = G.dense_case(61, 5, 7, 7, 64, 3, tail=True, expose=False)
    path = models.write_repo(str(tmp_path), "k", d["model"])
    return KM.with_env(dict(IE_AUTOTUNE="0", **env), lambda: B.DescribeModel(path, d["ishape"][0])["plan"])


def fused_steps(plan):
    return [s for s in plan["steps"] if s.get("algo") == "dense_fused"]


def test_fuse_pb_6_plans_the_nsplit_tile(tmp_path):
    plan = plan_of(tmp_path, dict(IE_FUSE_PB="6"))
    fused = fused_steps(plan)
    assert len(fused) == 3, [s["name"] for s in plan["steps"]]
    for s in fused:
        assert s["tile"] == 6, (s["name"], s["tile"])
        assert len(s["parts"]) == 2 and " | " in s["name"], s


def test_default_plan_is_unchanged(tmp_path):
    base = plan_of(tmp_path, {})
    assert [s["tile"] for s in fused_steps(base)] == [1, 1, 1]          # M = 245 <= 2048: 16-pixel tiles
    for other in ("0", "7", ""):
        assert json.dumps(plan_of(tmp_path, dict(IE_FUSE_PB=other)), sort_keys=True) == json.dumps(base, sort_keys=True), other
