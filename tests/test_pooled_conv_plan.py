"""CPU: which transitions the executor may run as one launch of conv1x1_pooled_kernel (EngineDescribeModel's `paired_launches`, decided from
shapes and views alone; csrc/tune.cpp FindPairedLaunches), and that the plan itself never moves with IE_POOL_CONV.

DenseNet-121 fp32 has three transitions (256 -> 128, 512 -> 256, 1024 -> 512 channels): all three pair, the first two can also chain the next
block's entry 1x1 (chain tiles of 128 and 256 channels; no 512-channel chain tile is built).  Half and e4m3 plans list nothing.  The near
misses -- a 3x3 / stride-2 average pool, a max pool, a padded 2x2 pool, a pooled tensor that is also a graph output, a conv with a residual,
an entry conv that reads another slice than the transition conv writes -- are listed with the reason and stay split."""
import os

import pytest

import kernel_graphs  # noqa: F401  (transition_graphs builds on it)
import test_kernel_maps_gpu as KM
import transition_graphs as T
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models

SWITCHES = [None, "0", "1", "2", "2:0"]


def describe(path, batch, **env):
    return KM.with_env({k: v for k, v in env.items() if v is not None}, lambda: B.DescribeModel(path, batch))


def plan_never_moves(path, batch):
    docs = [describe(path, batch, IE_POOL_CONV=v) for v in SWITCHES]
    for d in docs[1:]:
        assert d["plan"] == docs[0]["plan"]
        assert d["paired_launches"] == docs[0]["paired_launches"]
    return docs[0]


@pytest.mark.parametrize("batch", [1, 32])
def test_densenet121_transitions(densenet_repo, batch):
    d = plan_never_moves(os.path.join(densenet_repo, "densenet_onnx", "1"), batch)
    steps, pl = d["plan"]["steps"], d["paired_launches"]
    print([(e["steps"], e["kind"], e["tiles"], e["chain_tiles"], e["reason"]) for e in pl])
    assert [e["kind"] for e in pl] == ["pool_conv_chain", "pool_conv_chain", "pool_conv"]
    for e, (k, co) in zip(pl, [(256, 128), (512, 256), (1024, 512)]):
        i = e["steps"][0]
        assert e["steps"] == list(range(i, i + len(e["steps"])))
        assert steps[i]["kind"] == "pool" and steps[i + 1]["kind"] == "conv"
        assert (steps[i + 1]["in"]["c"], steps[i + 1]["out"]["c"]) == (k, co)
        assert steps[i + 1]["in"] == steps[i]["out"] and steps[i]["in"]["pitch"] >= k
        assert e["tiles"], e
    assert pl[0]["chain_tiles"] == [0, 6] and len(pl[0]["steps"]) == 3       # 128 channels: the {8 waves, 16 ch, 32 px} tile and its 16-pixel form
    assert pl[1]["chain_tiles"] == [2, 7] and len(pl[1]["steps"]) == 3       # 256 channels: {8, 32, 32} and {8, 32, 16}
    assert pl[2]["chain_tiles"] == [] and len(pl[2]["steps"]) == 2 and "512" in pl[2]["reason"]
    for e in pl[:2]:
        en = steps[e["steps"][2]]
        assert en["kind"] == "conv" and en["out"]["c"] == 128 and en["in"] == steps[e["steps"][1]]["out"] and en["in"]["pitch"] > en["in"]["c"]


def test_half_and_e4m3_plans_list_none(densenet_repo, tmp_path):
    assert describe(os.path.join(densenet_repo, "densenet_onnx", "1"), 32, IE_PRECISION="fp16")["paired_launches"] == []
    # (pre-activation graphs do not plan in fp8 mode: ResNet-50 is the fp8 model of this project)
    rn = models.write_repo(str(tmp_path), "rn50", models.resnet50("N"))
    for prec in ("fp16", "fp8"):
        assert describe(rn, 4, IE_PRECISION=prec)["paired_launches"] == []


@pytest.mark.parametrize("kind,words", [("avg3s2", "3x3"), ("max", "max pool"), ("padded", "padding"), ("pool_output", "pooled tensor"), ("residual", "residual")])
def test_near_misses_are_listed_and_not_paired(tmp_path, kind, words):
    path = models.write_repo(str(tmp_path), "miss", T.near_miss(kind)["model"])
    d = plan_never_moves(path, 2)
    (e,) = d["paired_launches"]
    print(kind, e)
    steps = d["plan"]["steps"]
    assert steps[e["steps"][0]]["kind"] == "pool" and steps[e["steps"][1]]["kind"] == "conv" and len(e["steps"]) == 2
    assert e["kind"] is None and e["tiles"] == [] and e["chain_tiles"] == []
    assert words in e["reason"], e


def test_entry_conv_on_another_slice_is_not_chained(tmp_path):
    path = models.write_repo(str(tmp_path), "miss", T.entry_slice_case()["model"])
    d = plan_never_moves(path, 2)
    pl = [e for e in d["paired_launches"] if e["kind"] is not None]
    print(d["paired_launches"])
    (e,) = pl
    steps = d["plan"]["steps"]
    conv, entry = steps[e["steps"][1]], steps[e["steps"][1] + 1]
    assert entry["kind"] == "conv" and entry["in"]["buf"] == conv["out"]["buf"] and entry["in"] != conv["out"]
    assert e["kind"] == "pool_conv" and len(e["steps"]) == 2 and e["chain_tiles"] == [] and "another view" in e["reason"], e


def test_swapped_transition_graph_pairs(tmp_path):
    """The GPU test's graph: the planner's own swap produces pool -> conv; 144 -> 128 channels fits the 128-, 64- and 16-channel tiles (not the 256-channel ones)."""
    path = models.write_repo(str(tmp_path), "t", T.transition_case(1, 2, 6, 10, 144, 128)["model"])
    (e,) = plan_never_moves(path, 2)["paired_launches"]
    assert e["kind"] == "pool_conv" and e["tiles"] == [0, 1, 3, 4, 5, 6], e
