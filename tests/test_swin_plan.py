"""CPU: Swin through the ONNX reader and the planner (EngineDescribeModel): the shifted-window attention region (roll, partition, attention with its
relative-position bias and shift mask, reverse, roll back) as ONE window_attention step between two ordinary 1x1 convs, patch merging as one
patch_merge step, no copy anywhere, every spelling the same plan, every near miss refused by name, and the float64 reference's sensitivity to the
bias, the mask and the roll's direction.

The step sequence of a block is layer_norm, conv, window_attention, conv, layer_norm, conv, conv, with the MLP's GELU as the eltwise step between
the last two convs that the same MLP has in the ViT and ConvNeXt plans (tests/test_vit_plan.py pins it there): the sequence is compared with the
GELU steps set aside, and the GELU steps are checked on their own.
Swin-T has 12 window_attention steps of which FIVE are shifted and masked: the odd blocks of the stages of depth 2 / 2 / 6 / 2 are 1 + 1 + 3 + 1 = 6,
and the last stage's (7 x 7 map, window 7) collapses to shift 0 as torchvision's rule says.
"""
import numpy as np
import pytest

import swin_graphs as G
import ref64
from engine_run import describe
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models
from oracle import onnx_oracle as O
from refusals import refused

PRECS = ("fp32", "fp16")
BATCH = 2


def _same_view(a, b):
    return all(a[k] == b[k] for k in ("buf", "n", "c", "h", "w", "c_off", "pitch", "f16"))


def _check_net(steps, batch, image, dims, depths, heads, window, f16):
    """the whole step list of a Swin: returns the window_attention steps"""
    kinds = [s["kind"] for s in steps]
    assert "copy" not in kinds, [(s["kind"], s["name"]) for s in steps]          # the patch conv reads the NCHW input itself; no view costs a copy
    gelus = [k for k, s in enumerate(steps) if s["kind"] == "eltwise"]
    for k in gelus:          # the MLP's GELU, alone between fc1 and fc2
        assert steps[k]["act"] == ["gelu", 0, 0] and steps[k - 1]["kind"] == steps[k + 1]["kind"] == "conv" and _same_view(steps[k]["in"], steps[k - 1]["out"])
    assert len(gelus) == sum(depths)
    rest = [s for s in steps if s["kind"] != "eltwise"]
    want = ["conv", "layer_norm"]
    for si, depth in enumerate(depths):
        want += (["patch_merge", "layer_norm", "conv"] if si else []) + G.BLOCK * depth
    want += ["layer_norm", "gap", "conv"]
    assert [s["kind"] for s in rest] == want, [(s["kind"], s["name"]) for s in rest]
    assert rest[0]["k"] == [4, 4] and rest[0]["stride"] == [4, 4] and rest[0]["in"]["nchw"]
    pos, hw, out = 2, image // 4, []
    for si, (depth, c, nh) in enumerate(zip(depths, dims, heads)):
        if si:
            mg, ln, red = rest[pos:pos + 3]
            pos += 3
            assert (mg["in"]["c"], mg["in"]["h"], mg["out"]["c"], mg["out"]["h"], mg["out"]["w"]) == (dims[si - 1], hw, 4 * dims[si - 1], hw // 2, hw // 2)
            assert (red["in"]["c"], red["out"]["c"], red["k"]) == (4 * dims[si - 1], c, [1, 1]) and not red["bias"] and not red["residual"]
            assert _same_view(ln["in"], mg["out"]) and mg["bytes"] == (2 if f16 else 4) * 2 * batch * hw * hw * dims[si - 1] and mg["flops"] == 0
            hw //= 2
        for bi in range(depth):
            ln1, qkv, at, proj, ln2, fc1, fc2 = rest[pos:pos + 7]
            pos += 7
            shift = 0 if bi % 2 == 0 or window >= hw else window // 2
            L, nW, hd = window * window, (hw // window) ** 2, c // nh
            assert ln1["name"] == f"s{si}b{bi}_ln1" and ln1["eps"] == float(np.float32(1e-5))
            assert (qkv["in"]["c"], qkv["out"]["c"], qkv["out"]["h"], qkv["out"]["w"], qkv["k"]) == (c, 3 * c, hw, hw, [1, 1]) and qkv["bias"] and not qkv["residual"]
            assert (at["heads"], at["head_dim"], at["window"], at["shift"], at["masked"]) == (nh, hd, [window, window], [shift, shift], shift != 0)
            assert abs(at["scale"] / hd ** -0.5 - 1) < 1e-6
            assert _same_view(at["in"], qkv["out"]) and _same_view(at["out"], proj["in"])
            assert (at["out"]["n"], at["out"]["c"], at["out"]["h"], at["out"]["w"]) == (batch, c, hw, hw)
            lp = (L + 31) // 32 * 32
            assert at["flops"] == 4 * batch * nW * nh * L * L * hd
            assert at["bytes"] == (2 if f16 else 4) * batch * hw * hw * 4 * c + 4 * lp * lp * (nh + (nW if shift else 0))
            assert at["tile"] == int(G.wattn_mfma_ok(L, hd, c, f16)) and at["in"]["f16"] == at["out"]["f16"] == f16
            assert proj["residual"] and proj["bias"] and fc2["residual"] and fc2["bias"] and not fc1["residual"]
            assert _same_view(proj["in2"], ln1["in"]) and _same_view(fc2["in2"], proj["out"]) and (fc1["out"]["c"], fc2["in"]["c"]) == (4 * c, 4 * c)
            out.append(at)
    assert pos == len(rest) - 3
    return out


@pytest.mark.parametrize("prec", PRECS)
def test_narrow_swin_plan(tmp_path, monkeypatch, prec):
    """fails on a planner without the window matcher, which refuses the graph at its first Slice"""
    path = models.write_repo(str(tmp_path), "swin", G.narrow(BATCH))
    p = describe(path, BATCH, monkeypatch, prec)
    ats = _check_net(p["steps"], BATCH, 56, (32, 64), (2, 2), (1, 2), 7, prec == "fp16")
    assert [(a["shift"], a["masked"]) for a in ats] == [([0, 0], False), ([3, 3], True), ([0, 0], False), ([0, 0], False)]
    assert p["outputs"][0]["dims"] == [BATCH, 10]


def test_swin_t_plan(tmp_path, monkeypatch):
    path = models.write_repo(str(tmp_path), "swin_t", models.swin_t(1))
    p = describe(path, 1, monkeypatch)
    ats = _check_net(p["steps"], 1, 224, (96, 192, 384, 768), (2, 2, 6, 2), (3, 6, 12, 24), 7, False)
    assert len(ats) == 12 and sum(a["masked"] for a in ats) == 5 and all(a["masked"] == (a["shift"] != [0, 0]) for a in ats)
    assert [a["heads"] for a in ats] == [3, 3, 6, 6] + [12] * 6 + [24, 24] and all(a["head_dim"] == 32 and a["tile"] == 1 for a in ats)
    assert [a["shift"][0] for a in ats] == [0, 3, 0, 3, 0, 3, 0, 3, 0, 3, 0, 0]
    assert sum(s["kind"] == "patch_merge" for s in p["steps"]) == 3


def _plan_key(steps):
    return [(s["kind"], s.get("algo"), s.get("tile"), s["in"], s["out"], s.get("residual"), s.get("heads"), s.get("window"), s.get("shift"), s.get("masked"),
             s["w_off"]) for s in steps]


def test_spellings_give_the_same_plan(tmp_path, monkeypatch):
    variants = [dict()] + [dict(pad=True), dict(mask="unsqueeze"), dict(swap=True), dict(pad=True, mask="unsqueeze", unbind="split", scale="sdpa", swap=True)]
    variants += [dict(unbind=u, scale=sc) for u in G.UNBINDS for sc in G.SCALES]
    first = blob = None
    for k, kw in enumerate(variants):
        path = models.write_repo(str(tmp_path), f"v{k}", G.narrow(BATCH, **kw))
        key = _plan_key(describe(path, BATCH, monkeypatch)["steps"])
        w = B.PlanWeights(path, BATCH)
        if first is None:
            first, blob = key, w
        assert key == first, kw
        if kw.get("scale", "q") == "q":          # (the scale is a step field, the blob holds the Linears and the tables)
            assert np.array_equal(w, blob), kw


def test_symbolic_batch(tmp_path, monkeypatch):
    """batch "N": every batch-dependent shape entry is -1; the plan is that of the constant shapes"""
    a = describe(models.write_repo(str(tmp_path), "sym", G.narrow("N")), 3, monkeypatch)
    b = describe(models.write_repo(str(tmp_path), "con", G.narrow(3)), 3, monkeypatch)
    assert _plan_key(a["steps"]) == _plan_key(b["steps"])
    assert np.array_equal(B.PlanWeights(str(tmp_path / "sym" / "1"), 3), B.PlanWeights(str(tmp_path / "con" / "1"), 3))
    shapes = [v for k, v in O.load_model(G.narrow("N")).inits.items() if k.endswith(("part6", "part3", "shape5", "mask5", "mask4", "shape3", "rev6", "rev4"))]
    assert shapes and all((np.asarray(v) == -1).sum() == 1 for v in shapes)


def test_tables_are_in_the_blob(tmp_path, monkeypatch):
    """the bias and the mask are the graph's constants, repacked [.][Lp][Lp] with the query index fastest and -inf on the padded keys"""
    mb = G.narrow(BATCH)
    path = models.write_repo(str(tmp_path), "swin", mb)
    at = [s for s in describe(path, BATCH, monkeypatch, "fp16")["steps"] if s["kind"] == "window_attention"][1]
    inits = O.load_model(mb).inits
    blob = B.PlanWeights(path, BATCH)
    L, lp = 49, 64
    bias = blob[at["w_off"]:at["w_off"] + lp * lp].reshape(lp, lp)          # one head: [key][query]
    np.testing.assert_array_equal(bias[:L, :L], inits["s0b1_attn_rpb"].reshape(L, L).T)
    assert np.all(np.isneginf(bias[L:])) and np.all(bias[:L, L:] == 0)
    m = inits["s0b1_attn_mask"]
    assert m.shape == (1, 4, 1, L, L) and set(np.unique(m)) == {-100.0, 0.0} and all((m[0, w] != 0).any() == (w != 0) for w in range(4))
    mask = blob[at["w_off"] + lp * lp:at["w_off"] + 5 * lp * lp].reshape(4, lp, lp)          # the mask table follows the one head's bias table
    np.testing.assert_array_equal(mask[:, :L, :L], m.reshape(4, L, L).transpose(0, 2, 1))
    assert np.all(mask[:, L:] == 0) and np.all(mask[:, :, L:] == 0)
    assert np.abs(inits["s0b1_attn_rpb"]).max() > 0.5                        # O(1): a dropped bias is visible


@pytest.mark.parametrize("prec", PRECS)
def test_window_attention_tiles(tmp_path, monkeypatch, prec):
    """default tile and IE_FORCE_TILE: hd 32 with at most 64 tokens per window takes the MFMA kernel, everything else the generic one whatever is forced"""
    for hw, win, heads, hd, ok in (((8, 8), 4, 2, 32, True), ((16, 16), 8, 1, 32, True), ((8, 8), 4, 2, 20, False), ((9, 9), 9, 1, 32, False), ((8, 8), 4, 1, 64, False)):
        path = models.write_repo(str(tmp_path), f"w{hw[0]}_{win}_{hd}", G.wattn_graph(2, hw, win, win // 2, heads, hd))
        got = {}
        for forced in (None, "0", "1", "2"):
            steps = describe(path, 2, monkeypatch, prec, **({} if forced is None else {"IE_FORCE_TILE": forced}))["steps"]
            assert [s["kind"] for s in steps] == ["copy", "window_attention", "copy"]          # the NCHW graph input and output; nothing for the views
            got[forced] = steps[1]["tile"]
        assert G.wattn_mfma_ok(win * win, hd, heads * hd, prec == "fp16") == ok
        assert got == {None: int(ok), "0": 0, "1": int(ok), "2": int(ok)}, (hw, win, hd, got)          # (2 is no tile: the default)


def test_linear_region_plan(tmp_path, monkeypatch):
    path = models.write_repo(str(tmp_path), "lin", G.wattn_graph(2, (14, 14), 7, 3, 2, 32, linear=True))
    steps = describe(path, 2, monkeypatch)["steps"]
    assert [s["kind"] for s in steps] == ["conv", "window_attention", "conv", "copy"]          # (the qkv conv reads the NCHW input itself)


def test_patch_merge_plan(tmp_path, monkeypatch):
    for c, label in ((8, "patch_merge_kernel<f32,4>"), (5, "patch_merge_kernel<f32,1>")):
        path = models.write_repo(str(tmp_path), f"m{c}", G.merge_graph(2, c, (6, 10)))
        steps = describe(path, 2, monkeypatch)["steps"]
        assert [s["kind"] for s in steps] == ["copy", "patch_merge", "copy"]
        assert (steps[1]["out"]["c"], steps[1]["out"]["h"], steps[1]["out"]["w"]) == (4 * c, 3, 5)


# ---- refusals: every near miss names its node and its rule ----------------------------------------------------------------------------------
NEAR_MISSES = [
    (dict(pad=True, tweak=dict(pad_value=1)), "Pad ", "non-zero window padding"),
    (dict(tweak=dict(back_shift=(2, 3))), "Softmax ", "the roll back does not undo the roll: axis 1"),
    (dict(tweak=dict(back_axes=(2, 1)), shift=(3, 2)), "Softmax ", "the roll back does not undo the roll"),
    (dict(tweak=dict(reverse_roll=True)), "Concat ", "rolls the map forward"),
    (dict(tweak=dict(rev_window=(2, 2))), "Reshape ", "the reverse has the window grid"),
    (dict(tweak=dict(rev_perm=(0, 3, 1, 2, 4, 5))), "Transpose ", "is not Transpose(perm [0,1,3,2,4,5]), the partition's"),
    (dict(tweak=dict(bias_heads=3)), "Add ", "the relative-position bias must have the shape [1, heads, L, L] = [1, 2, 49, 49]"),
    (dict(tweak=dict(bias_l=48)), "Add ", "the relative-position bias must have the shape"),
    (dict(tweak=dict(mask_nw=3)), "Add ", "the shift mask holds 3 windows, the partition 4"),
    (dict(tweak=dict(mask_l=48)), "Add ", "the shift mask must have the shape [1, nW, 1, L, L]"),
    (dict(tweak=dict(mask_heads=2)), "Add ", "the shift mask must broadcast along the head axis"),
    (dict(tweak=dict(second_reader=True)), "Add ", "has 2 readers, not 1"),
    (dict(tweak=dict(mask_without_roll=True)), "Add ", "is added to the scores but the map is not rolled"),
    (dict(tweak=dict(roll_without_mask=True)), "Softmax ", "but no shift mask is added to the scores"),
]


@pytest.mark.parametrize("kw,node,rule", NEAR_MISSES, ids=[str(sorted(k.get("tweak", {}))[0]) + ("_b" if "shift" in k else "") for k, _, _ in NEAR_MISSES])
def test_refusals(tmp_path, monkeypatch, kw, node, rule):
    kw = dict(kw)
    shift = kw.pop("shift", 3)
    path = models.write_repo(str(tmp_path), "bad", G.wattn_graph(2, (14, 14), 7, shift, 2, 32, linear=True, **kw))
    refused(path, 2, monkeypatch, rule, node, "window-attention pattern")


def test_refusals_at_import(tmp_path, monkeypatch):
    """what needs the map's extents: a map that is no multiple of the window, a shift as large as the window, an odd map under a patch merging"""
    for name, mb, rule in (
            ("odd", G.wattn_graph(2, (14, 14), 7, 0, 2, 32, declared_hw=(15, 14)), "the map 15 x 14 is no multiple of the window 7 x 7"),
            ("big", G.wattn_graph(2, (14, 14), 7, 7, 2, 32), "the shift 7 x 7 is not smaller than the window 7 x 7"),
            ("merge", G.merge_graph(2, 8, (7, 10)), "patch merging of an odd map (7 x 10) is not supported")):
        refused(models.write_repo(str(tmp_path), name, mb), 2, monkeypatch, rule)


def test_a_plain_attention_with_a_mask_is_still_refused_by_name(tmp_path, monkeypatch):
    """an Add in front of the Softmax of a token attention is no window attention: MatchAttention's refusal text stands"""
    from gpu_ai_inference_server_amd.modelgen import onnx_pb as pb
    gb = models.GraphBuilder("masked", 5)
    t = models.vit_tokens(gb, "x", 3 * 64)
    y = gb.simple("Reshape", [t, gb.init("s5", np.array([0, -1, 3, 2, 32], np.int64))])
    y = gb.transpose(y, (2, 0, 3, 1, 4))
    parts = []
    for i in range(3):
        gb.nodes.append(pb.node("Constant", [], [f"i{i}"], f"i{i}", [pb.attr_int("value_int", i)]))
        parts.append(gb.simple("Gather", [y, f"i{i}"], [pb.attr_int("axis", 0)]))
    s = gb.simple("MatMul", [parts[0], gb.transpose(parts[1], (0, 1, 3, 2))])
    s = gb.simple("Add", [s, gb.init("m", np.zeros((1, 2, 5, 5), np.float32))])
    y = gb.transpose(gb.simple("MatMul", [gb.simple("Softmax", [s], [pb.attr_int("axis", -1)]), parts[2]]), (0, 2, 1, 3))
    y = gb.transpose(gb.simple("Reshape", [y, gb.init("s3", np.array([0, -1, 64], np.int64))]), (0, 2, 1))
    gb.simple("Reshape", [y, gb.init("back", np.array([0, 64, 1, 5], np.int64))], out="y")
    path = models.write_repo(str(tmp_path), "masked", gb.finish([("x", [2, 192, 1, 5])], [("y", [2, 64, 1, 5])], opset=17))
    refused(path, 2, monkeypatch, match="an additive mask")


# ---- the float64 reference notices what a broken kernel would drop --------------------------------------------------------------------------
def test_reference_sensitivity():
    """zeroing the bias, zeroing the mask and reversing the roll each move the narrow net's float64 logits by more than 5 %"""
    mb = G.narrow(BATCH)
    # noise plus a coarse grid of 8-pixel cells (two tokens) at twice the amplitude: neighbouring windows then differ, which is what the mask and
    # the roll act on (on smooth images every token of a window carries nearly the same v, and the global pool averages the rest away)
    st = np.random.RandomState(1)
    x = (st.randn(BATCH, 3, 56, 56) + 2.0 * np.repeat(np.repeat(st.randn(BATCH, 3, 7, 7), 8, 2), 8, 3)).astype(np.float32)
    ref = ref64.run_f64(mb, {"input": x})["logits"]
    inits = O.load_model(mb).inits
    zero = lambda suffix: {k: np.zeros_like(v) for k, v in inits.items() if k.endswith(suffix)}  # noqa: E731
    assert len(zero("_rpb")) == 4 and len(zero("_mask")) == 1
    moved = {
        "bias": ref64.rel_err(ref64.run_f64(mb, {"input": x}, overrides=zero("_rpb"))["logits"], ref),
        "mask": ref64.rel_err(ref64.run_f64(mb, {"input": x}, overrides=zero("_mask"))["logits"], ref),
        "roll": ref64.rel_err(ref64.run_f64(G.narrow(BATCH, tweak=dict(reverse_roll=True)), {"input": x})["logits"], ref),
    }
    print(moved)
    assert all(v > 0.05 for v in moved.values()), moved
