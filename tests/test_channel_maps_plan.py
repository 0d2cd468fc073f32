"""CPU: every entry of the case tables of tests/test_channel_maps_gpu.py plans onto the kernel, tile and Profile() label it names, in both
precisions (the planner's eligibility predicates decide; no GPU is needed to see that), with the fusions tests/channel_graphs.py says the
step under test carries; the three inputs of every case without ReLU, Clip or activation are distinguishable at every element; the
second-round cases exceed the grid; and the label mirrors spell out the step-down of DwLanePixels and the tiles GroupedTileFits refuses."""
import numpy as np
import pytest

import channel_graphs as CG
import kernel_ref as R
import test_channel_maps_gpu as M
from engine_run import plan_of
from gpu_ai_inference_server_amd.modelgen import models


def planned(tmp_path, d, prec, tile=None):
    path = models.write_repo(str(tmp_path), "t", d["model"])
    env = dict(IE_AUTOTUNE="0", IE_GROUPED_CONV="1", IE_PRECISION=prec, **({} if tile is None else dict(IE_FORCE_TILE=str(tile))))
    steps = plan_of(path, d["ishape"][0], env)["steps"]
    return M.conv_step(steps), steps


def fusions_ok(d, st, steps):
    """the step under test carries what channel_graphs.channel_case built around the conv, and nothing became a step of its own"""
    assert [s["kind"] for s in steps if s["kind"] not in ("conv", "copy")] == [], [s["name"] for s in steps]
    assert st["pre"] == (d["pre"] != "") and st["pre_relu"] == (d["pre"] in ("bn", "clip")) and st["relu"] == d["relu"]
    assert st["residual"] == d["res"] and st["bias"] == bool(d["bias"] or d["post_bn"])
    assert st.get("pre_clip") == (CG.PRE_CLIP_HI if d["pre"] == "clip" else None)
    assert (st.get("pre_act") or [None])[0] == {"hswish": "hardswish", "sigmoid": "sigmoid"}.get(d["pre"])
    assert (st.get("act") or [None])[0] == {"hswish": "hardswish", "sigmoid": "sigmoid", "hardsigmoid": "hardsigmoid"}.get(d["act"])
    if st.get("act"):
        assert tuple(np.float32(st["act"][1:])) == tuple(np.float32(CG.ACTS[d["act"]][1:]))
    if d["clip"]:
        assert [None if v is None else np.float32(v) for v in st["clip"]] == [None if v is None else np.float32(v) for v in d["clip"]]
    else:
        assert "clip" not in st
    if d["res"]:
        assert st["in2_src"] == st["in_src"] and steps[st["in_src"]]["name"] == "lift" and not steps[st["in_src"]]["relu"]
    if d["pre"] in ("hswish", "sigmoid"):
        assert not steps[st["in_src"]]["relu"] and "act" not in steps[st["in_src"]]          # the lift stays linear
    want_out = (8, d["cout"] + 8) if d["out"] == "offset" else (0, d["cout"] * len(d["copies"]) + (8 if d["slice_in"] else 0))
    assert (st["out"]["c_off"], st["out"]["pitch"]) == want_out
    assert (st["in"]["c_off"], st["in"]["pitch"]) == ((8, d["c"] + 8) if d["slice_in"] else (0, 3 if d["direct"] else d["c"]))


@pytest.mark.parametrize("prec", M.PRECS)
def test_depthwise_tables(tmp_path, prec):
    for case in M.DW_PLAIN + M.DW_ACT + M.DW_EDGE:
        d = M.build(case)
        for tile in (1, 2, 3):
            st, steps = planned(tmp_path, d, prec, tile)
            assert (st["algo"], st["tile"]) == ("depthwise", tile), (case, prec, tile, st["tile"])
            fusions_ok(d, st, steps)
    for case in M.DW_GENERIC + [M.DW_PLAIN[0], M.DW_ACT[3]]:
        d = M.build(case)
        st, steps = planned(tmp_path, d, prec, 0)
        assert (st["algo"], st["tile"]) == ("depthwise", 0), (case, prec)
        fusions_ok(d, st, steps)
        if d["direct"]:
            assert st["in"]["nchw"] and not st["in"]["f16"] and st["out"]["f16"] == (prec == "fp16")
    for case in M.DW_GENERIC:
        d = M.build(case)
        if d["c"] % 8 or d["kh"] != d["kw"] or d["kh"] == 7 or d["direct"]:      # no fast kernel in fp16 (nor, but for C = 20, in fp32): a forced fast tile plans tile 0
            assert planned(tmp_path, d, "fp16", 2)[0]["tile"] == 0, case


def test_depthwise_c20_and_second_round(tmp_path):
    d = M.build(M.DW_C20)
    for tile in (1, 2, 3):
        assert planned(tmp_path, d, "fp16", tile)[0]["tile"] == 0 and planned(tmp_path, d, "fp32", tile)[0]["tile"] == tile
    for case, prec, tile in M.DW_ROUND2:
        d = M.build(case)
        st, steps = planned(tmp_path, d, prec, tile)
        assert (st["algo"], st["tile"]) == ("depthwise", tile) and [s["kind"] for s in steps] == ["conv", "conv", "copy"]
        groups, nslots = M.round2_groups_and_slots(d, prec, tile)
        assert groups > nslots and nslots == (4096 if prec == "fp16" else 2048), (case, groups, nslots)
        assert M.dw_label(d, prec, tile) == f"conv_dw_kernel<{'f16' if prec == 'fp16' else 'f32'},k3,s1,px{M.DW_PX[tile]}>"


@pytest.mark.parametrize("prec", M.PRECS)
def test_grouped_tables(tmp_path, prec):
    cfgs = []
    for case in M.GROUPED + M.GROUPED_MORE:
        d = M.build(case)
        cfg = M.grouped_cfg_for(d["c"], d["cout"], d["groups"])
        cfgs.append(cfg)
        default = planned(tmp_path, d, prec)[0]["tile"]
        assert default >= 1
        for tile in (1, 2, 3):
            st, steps = planned(tmp_path, d, prec, tile)
            fits = M.grouped_tile_fits(cfg, prec == "fp16", tile)
            assert (st["algo"], st["tile"], st["group"]) == ("grouped", tile if fits else default, d["groups"]), (case, prec, tile, st["tile"])
            key = (d["c"] // d["groups"], prec, tile)
            assert (key in M.GROUPED_FALLBACK) == (not fits) and (fits or st["tile"] == M.GROUPED_FALLBACK[key]), (key, st["tile"])
            fusions_ok(d, st, steps)
        assert (d["oh"], d["ow"], d["n"]) == (5, 7, 2)                # M = 70: one full 64-pixel row and a tail of 6
    assert cfgs[:8] == list(range(8))                                 # one case per entry of kGroupedCfgs, in its order
    d = M.build(M.GROUPED_MORE[0])
    cpg, opb, gpb = M.GROUPED_CFGS[cfgs[8]]
    assert gpb == 1 and d["cout"] // d["groups"] == 2 * opb           # two channel blocks read the same group
    for case in M.GROUPED_GENERIC + [M.GROUPED[1], M.GROUPED[4]]:
        d = M.build(case)
        st, steps = planned(tmp_path, d, prec, 0)
        assert (st["algo"], st["tile"]) == ("grouped", 0)
        fusions_ok(d, st, steps)
    for case in M.GROUPED_GENERIC[:2]:                                # no fast configuration: a forced fast tile plans the generic kernel
        d = M.build(case)
        assert M.grouped_cfg_for(d["c"], d["cout"], d["groups"]) == -1 and planned(tmp_path, d, prec, 2)[0]["tile"] == 0


def test_fp16_grouped_cases_have_both_rounded_operand_counts():
    counts = set()
    for case in M.GROUPED + M.GROUPED_MORE:
        d = M.build(case)
        dot = (d["c"] // d["groups"]) % 2 == 0
        counts.add((dot, CG.channel_operands(d, d["x"], True, dot)["rounded"]))
    assert counts == {(False, 0), (True, 0), (True, 1), (True, 2)} or counts == {(False, 0), (True, 0), (True, 1)}, counts
    assert {c for dt, c in counts if dt} >= {0, 1}


def test_label_mirrors():
    d = M.build(M.DW_ACT[4])
    assert (d["kh"], d["stride"], d["act"]) == (5, 2, "hswish")
    assert M.dw_label(d, "fp32", 3) == "conv_dw_kernel<f32,k5,s2,px2,act>" and M.dw_label(d, "fp16", 3) == "conv_dw_kernel<f16,k5,s2,px1,act>"
    assert M.dw_label(M.build(M.DW_PLAIN[3]), "fp16", 3) == "conv_dw_kernel<f16,k5,s2,px4>"
    assert M.grouped_label(M.build(M.GROUPED[3]), "fp16", 2) == "conv_grouped_kernel<f16,c8,o8x2,px2>"
    assert M.grouped_label(M.build(M.GROUPED[4]), "fp32", 1) == "conv_grouped_kernel<f32,c8,o8x1,px1>"
    # fp32 cpg 32 has no tile 3, cpg 64 no tiles 2 and 3; fp16 cpg 64 no tile 3; everything else fits
    missing = {(cpg, f16, t) for i, (cpg, _, _) in enumerate(M.GROUPED_CFGS) for f16 in (False, True) for t in (1, 2, 3) if not M.grouped_tile_fits(i, f16, t)}
    assert missing == {(32, False, 3), (64, False, 2), (64, False, 3), (64, True, 3)}
    # the labels the GPU module's tables can reach are all the labels there are
    reach = set()
    for prec in M.PRECS:
        for case in M.DW_PLAIN + M.DW_ACT + M.DW_EDGE:
            reach |= {M.dw_label(M.build(case), prec, t) for t in (1, 2, 3)}
        for case in M.GROUPED + M.GROUPED_MORE:
            d = M.build(case)
            cfg = M.grouped_cfg_for(d["c"], d["cout"], d["groups"])
            reach |= {M.grouped_label(d, prec, t) for t in (1, 2, 3) if M.grouped_tile_fits(cfg, prec == "fp16", t)}
    assert reach >= M.all_dw_labels() | M.all_grouped_labels(), sorted((M.all_dw_labels() | M.all_grouped_labels()) - reach)
    assert len(M.all_grouped_labels()) == 2 * 8 * 3 - 4


@pytest.mark.parametrize("prec", M.PRECS)
def test_three_inputs_are_distinguishable_everywhere(prec):
    """The cases on which the GPU test asserts written_check_is_conclusive meet it (a property of the data, known before any GPU run)"""
    n = 0
    for case in M.DW_PLAIN + M.DW_ACT + M.DW_EDGE + M.DW_GENERIC + [M.DW_C20] + M.GROUPED + M.GROUPED_MORE + M.GROUPED_GENERIC:
        d = M.build(case)
        if not M.written_check_applies(d):
            continue
        dot = d["groups"] != d["c"] and prec == "fp16" and (d["c"] // d["groups"]) % 2 == 0
        refs = [M.reference(case, run, prec, dot) for run in range(3)]
        assert R.written_check_is_conclusive([(a["ref"], a["S"], a["extra"], a["ce"]) for a in refs]), (case, prec)
        n += 1
    assert n >= 20


def test_dilated_table(tmp_path):
    K = M.KM
    seen = set()
    for case in M.DILATED:
        d = K.build(case)
        seen.add((d["dil"], d["pad"] == d["dil"], d["stride"], d["cin"]))
        assert (d["k"], d["cout"], d["n"], d["h"], d["w"]) == (3, 40, 2, 13, 11) and d["pad"] in (0, d["dil"])
        for prec in M.PRECS:
            for t in range(7):
                st = M.dilated_step(tmp_path, d, dict(IE_FORCE_ALGO="igemm", IE_FORCE_TILE=str(t)), prec)
                if prec == "fp16" and d["cin"] % 8:          # the fp16 MFMA loader reads 8-channel chunks: Cin = 20 runs on the naive kernel
                    assert (st["algo"], st["dilations"]) == ("naive", [d["dil"]] * 2)
                    continue
                assert (st["algo"], st["tile"], st["dilations"]) == ("igemm_vec", t, [d["dil"]] * 2), (case, prec, t, st["algo"], st["tile"])
        st = M.dilated_step(tmp_path, d, dict(IE_FORCE_ALGO="scalar", IE_FORCE_TILE="0"), "fp32")
        assert (st["algo"], st["tile"], st["dilations"]) == ("igemm_scalar", 0, [d["dil"]] * 2)
        st = M.dilated_step(tmp_path, d, dict(IE_FORCE_ALGO="naive", IE_FORCE_TILE="0"), "fp32")
        assert (st["algo"], st["dilations"]) == ("naive", [d["dil"]] * 2)
    assert {s[0] for s in seen} == {2, 4} and {s[1] for s in seen} == {True, False} and {s[2] for s in seen} == {1, 2} and {s[3] for s in seen} == {20, 64}
    # the undilated tables are the tuples they were
    assert all(len(c) == 13 for c in K.IGEMM32 + K.SCALAR32 + K.NAIVE) and all(len(c) == 14 for c in M.DILATED)
