"""CPU: every entry of the case tables of tests/test_fp8_maps_gpu.py plans onto the step kinds, algo and tile it names, and pins enough of
every e4m3 map for the GPU test to mean something.

Without a GPU there are no calibrated scales, so the chain is walked with the plan emulation (oracle.fp8.emulate_step, every step from
what the emulation of the step before wrote) and stand-in scales 2 * max |float64 value of the step on the case's own input| / 448 -- the
engine's formula applied to the test input.  Per step the conditions of tests/fp8_graphs.py are asserted from the reference alone: at most
1 % of the elements undecided between two codes, no interval over more than two adjacent e4m3 values, at least 25 % of the map pinned to
one non-zero code, at most 1 % clamped at +-448.  The planned kernel and tile, c_emul and the shares are printed per step."""
import pytest

import fp8_graphs as G
import test_fp8_maps_gpu as M


def plan_and_walk(tmp_path, tag, case, env, algo=None, tile=None):
    _, plan, blob = G.planned(tmp_path, case, env)
    st = M.under_test(plan)
    if algo is not None:
        assert (st.get("algo", st["kind"]), st.get("tile")) == (algo, tile), (tag, case, st["name"], st.get("algo"), st.get("tile"))
    assert plan["steps"][-1]["kind"] == "gap" and plan["steps"][0].get("algo") in ("stem", "stem_pool")
    assert all(s["out"]["f8"] for s in plan["steps"][:-1]) and not plan["steps"][-1]["out"]["f8"]
    for line in G.walk(tag, case, plan, blob):
        print(line)
    return plan


def test_tiled_conv_table(tmp_path):
    kept = set()
    for tile in range(7):
        for case in M.IGEMM:
            want = M.igemm_tile(tmp_path, case, tile)
            kept.add((tile, want)) if want != tile else None
            plan_and_walk(tmp_path, f"igemm_f8 t{tile}", case, dict(IE_FORCE_TILE=str(tile)), "igemm_f8", want)
    # the wide tiles (bn > 32) were refused for the 16- and 32-channel outputs, and only for them
    assert {t for t, _ in kept} == {t for t in range(7) if G.F8_TILES[t][1] > 32}, kept


def test_weights_stationary_1x1_table(tmp_path):
    for tile in range(100, 110):
        accepted = 0
        for case in M.ws1x1_cases(tile):
            plan = plan_and_walk(tmp_path, f"ws1x1_f8 t{tile}", case, dict(IE_FORCE_TILE=str(tile)), "igemm_f8", tile)
            st = M.under_test(plan)
            accepted += G.ws1x1_accepts(st, tile - 100)
            if st["in"]["c"] % 32:
                assert G.launched_label(st) == "conv_igemm_f8_kernel<"          # K % 32 == 16: declined at launch, the tiled kernel runs
        assert accepted >= 4, tile
    for case in M.DUAL:
        plan = plan_and_walk(tmp_path, "dual_f8", case, {}, "dual_f8", 1)
        pj, cv = M.under_test(plan)["parts"]
        assert pj["stride"] == [case[10][1]] * 2 and cv["stride"] == [1, 1] and pj["in"]["c"] != cv["in"]["c"]


def test_weights_stationary_3x3_table(tmp_path):
    for tile in range(200, 208):
        for case in M.WS3X3:
            plan = plan_and_walk(tmp_path, f"ws3x3_f8 t{tile}", case, dict(IE_FORCE_TILE=str(tile)), "igemm_f8", tile)
            print(f"ws3x3_f8 t{tile} case {case[0]}: launches {G.launched_label(M.under_test(plan))}")


def test_pool_stem_and_gap_tables(tmp_path):
    for case in M.POOLS:
        plan = plan_and_walk(tmp_path, "pool_f8", case, {}, "pool", None)
        st = M.under_test(plan)
        assert st["max"] == (case[11][0] == "max") and st["k"] == [case[11][1]] * 2 and st["count_include_pad"] == bool(case[11][4])
    for case in M.STEMS:
        assert plan_and_walk(tmp_path, "stem+pool", case, {}, "stem_pool", 1)["steps"][0]["algo"] == "stem_pool"
        plan = plan_and_walk(tmp_path, "stem", case, dict(IE_NO_STEM_POOL="1"), "pool", None)
        assert [s.get("algo", s["kind"]) for s in plan["steps"]] == ["stem", "pool", "gap"]
    shapes = set()
    for case in M.GAPS:
        g = plan_and_walk(tmp_path, "gap_f8", case, {})["steps"][-1]
        shapes.add((g["in"]["c"], g["in"]["h"] * g["in"]["w"]))
    assert shapes == {(80, 3), (16, 3), (80, 285)}, shapes


def test_keep_buffers_gives_every_value_its_own_buffer(tmp_path):
    """IE_KEEP_BUFFERS=1 recycles nothing (every step's views stay readable); unset, the same graph's plan reuses a buffer and is otherwise the same."""
    case = M.IGEMM[3]          # the strided conv's map fits the buffer the stem's output left
    _, kept, _ = G.planned(tmp_path, case, {})
    G.assert_readable(kept)
    _, plain, _ = G.planned(tmp_path, case, dict(IE_KEEP_BUFFERS="0"))
    assert len(plain["buffers"]) < len(kept["buffers"])
    with pytest.raises(AssertionError):
        G.assert_readable(plain)
    strip = lambda p: [{k: v for k, v in s.items() if k not in ("in", "in2", "out")} for s in p["steps"]]
    assert strip(plain) == strip(kept)


def test_run_plan_applies_the_prologue_of_every_step_kind(tmp_path):
    """A stand-alone BatchNormalization behind a ReLU (and one behind an Add) becomes an eltwise step that carries the affine as its prologue,
    and a BN + ReLU in front of a pool or a global pool becomes that step's prologue: run_plan, rebuilt on emulate_step, applies all of
    them, as the ONNX-operator oracle does."""
    import numpy as np

    from gpu_ai_inference_server_amd import binding as B
    from gpu_ai_inference_server_amd.modelgen import models
    from gpu_ai_inference_server_amd.modelgen import onnx_pb as pb
    from oracle import fp8 as F
    from oracle import onnx_oracle as O

    def affine(gb):
        return gb.bn(gb.relu(gb.conv("x", 8, 12, 3, pad=1, bias=True, name="c")), 12, name="bn"), [2, 12, 6, 5]

    def affine_add(gb):
        a = gb.relu(gb.conv("x", 8, 12, 1, name="c"))
        return gb.bn(gb.simple("Add", [gb.bn(a, 12, name="bn_a"), a]), 12, name="bn_b"), [2, 12, 6, 5]

    def pooled(gb):
        a = gb.relu(gb.bn(gb.conv("x", 8, 12, 1, name="c"), 12, name="bn_a"))
        a = gb.pool("MaxPool", gb.relu(gb.bn(gb.conv(a, 12, 12, 1, name="d"), 12, name="bn_b")), 2, 2)
        return gb.gap(gb.relu(gb.bn(a, 12, name="bn_c"))), [2, 12, 1, 1]
    kinds = set()
    for i, mk in enumerate((affine, affine_add, pooled)):
        gb = models.GraphBuilder("affine", 90 + i)
        y, oshape = mk(gb)
        mb = gb.finish([("x", [2, 8, 6, 5])], [(y, oshape)])
        path = models.write_repo(str(tmp_path), f"affine{i}", mb)
        plan, blob = B.DescribeModel(path, 2)["plan"], B.PlanWeights(path, 2)
        kinds.update(s["kind"] for s in plan["steps"] if s["pre"])
        x = models.synthetic_input((2, 8, 6, 5), stream=f"affine{i}")
        (ref,) = O.run(O.load_model(mb), {"x": x}, dtype=np.float64).values()
        (got,) = F.run_plan(plan, blob, {"x": x}).values()
        assert got.shape == ref.shape and np.abs(got - ref).max() / np.abs(ref).max() < 5e-7, (mk.__name__, [(s["kind"], s["pre"]) for s in plan["steps"]])
    assert "eltwise" in kinds, kinds          # the step kind whose prologue a rebuilt run_plan once dropped
    print("steps with a prologue:", sorted(kinds))
