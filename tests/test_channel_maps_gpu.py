"""GPU (-m gpu): the depthwise kernels (csrc/kernels_dw.hip) and the grouped kernels (csrc/kernels_grouped.hip) checked per element on the
feature map they write, the way tests/test_kernel_maps_gpu.py checks the dense conv families and tests/test_convt_maps_gpu.py the transposed
ones; and the dilated taps of the implicit GEMMs through test_kernel_maps_gpu.check_conv.

Each case is a single-step graph with exact operands (tests/channel_graphs.py).  It runs THREE different inputs on one model under
IE_AUTOTUNE=0 with the tile forced, asserts the plan's algo and tile and the full Profile() label (which mirrors kernels.h's DwLanePixels /
kGroupedCfgs / GroupedTileFits, copied below), and holds each of the three outputs to its own bound
|y - ref| <= 2 * c_emul * u * S + allowance  (kernel_ref.channel_allowance: the half terms of fp16 mode, and behind a fused activation
L * delta + E with E = engine_run.RTOL[prec] * |f(ref_z)|, the project's own relative figure per element -- generous for an exp and a
divide, see DESIGN.md for the measured ratios).  c_emul comes from CPU emulations of the case's own data, never from engine output.  A
failure names kernel, case, c, c_emul and the worst (n, channel, row, col) with its position class.  The engine reuses buffers across
requests, so an element a kernel never wrote could hold the previous request's correct value: with three inputs it cannot meet all three
bounds where two references are further apart than their bounds together, which is asserted for every element of the cases without ReLU,
Clip or activation (kernel_ref.written_check_is_conclusive).

The case tables are literal; tests/test_channel_maps_plan.py checks on the CPU that every entry plans onto the tile and label it names."""
import functools

import numpy as np
import pytest

import channel_graphs as CG
import kernel_graphs as G
import kernel_ref as R
import test_kernel_maps_gpu as KM
from engine_run import plan_of, RTOL, run_model
from gpu_ai_inference_server_amd.modelgen import models

pytestmark = pytest.mark.gpu

PRECS = ("fp32", "fp16")

# ---- mirrors of csrc/kernels.h ------------------------------------------------------------------------------------------------------------
DW_PX = (0, 1, 2, 4)                                  # kDwPx: requested output pixels per lane of tiles 0-3
GROUPED_CFGS = [(1, 2, 8), (2, 2, 8), (4, 4, 4), (8, 8, 2), (8, 8, 1), (16, 16, 1), (32, 16, 1), (64, 16, 1)]      # kGroupedCfgs: (cpg, opb, gpb)
GROUPED_PX = (0, 1, 2, 4)                             # kGroupedPx


def dw_lane_pixels(px, f16, k, s, act):
    """DwLanePixels: with a fused activation the wide variants step down"""
    v = 8 if f16 else 4
    if not act:
        return px
    return 4 if px >= 4 and k * (3 * s + k) * v <= 200 else 2 if px >= 2 and k * (s + k) * v <= 200 else 1


def grouped_cfg_for(cin, cout, groups):
    if groups < 2 or cin % groups or cout % groups:
        return -1
    cpg, opg = cin // groups, cout // groups
    for i, (c, opb, gpb) in enumerate(GROUPED_CFGS):
        if c == cpg and ((opg == opb and groups % gpb == 0) if gpb > 1 else opg % opb == 0):
            return i
    return -1


def grouped_tile_fits(cfg, f16, tile):
    if cfg < 0 or not 1 <= tile <= 3:
        return False
    cpg, opb, gpb = GROUPED_CFGS[cfg]
    in_regs = cpg * gpb // 2 if f16 and cpg % 2 == 0 else cpg * gpb
    return GROUPED_PX[tile] * (opb * gpb + in_regs) <= 128


def dw_label(d, prec, tile):
    if tile == 0:
        return "conv_dw_generic_kernel"
    act = bool(d["act"]) or d["pre"] in ("hswish", "sigmoid")
    f16 = prec == "fp16"
    return f"conv_dw_kernel<{'f16' if f16 else 'f32'},k{d['kh']},s{d['stride']},px{dw_lane_pixels(DW_PX[tile], f16, d['kh'], d['stride'], act)}{',act' if act else ''}>"


def grouped_label(d, prec, tile):
    cfg = grouped_cfg_for(d["c"], d["cout"], d["groups"])
    if tile == 0 or cfg < 0:
        return "conv_grouped_generic_kernel"
    cpg, opb, gpb = GROUPED_CFGS[cfg]
    return f"conv_grouped_kernel<{'f16' if prec == 'fp16' else 'f32'},c{cpg},o{opb}x{gpb},px{GROUPED_PX[tile]}>"


def all_dw_labels():
    """every fast label DwLanePixels can produce"""
    return {f"conv_dw_kernel<{t},k{k},s{s},px{dw_lane_pixels(px, t == 'f16', k, s, act)}{',act' if act else ''}>"
            for t in ("f32", "f16") for k in (3, 5) for s in (1, 2) for act in (False, True) for px in (1, 2, 4)}


def all_grouped_labels():
    """every configuration x admitted pixels-per-lane"""
    return {f"conv_grouped_kernel<{t},c{cpg},o{opb}x{gpb},px{GROUPED_PX[tile]}>" for t in ("f32", "f16") for i, (cpg, opb, gpb) in enumerate(GROUPED_CFGS)
            for tile in (1, 2, 3) if grouped_tile_fits(i, t == "f16", tile)}


# ---- case tables ---------------------------------------------------------------------------------------------------------------------------
def K(seed, n, h, w, c, groups, cout, **kw):
    """One case (channel_graphs.channel_case arguments), hashable"""
    return (seed, n, h, w, c, groups, cout, tuple(sorted(kw.items())))


@functools.lru_cache(maxsize=None)
def build(case):
    return CG.channel_case(*case[:7], **dict(case[7]))


def DW(seed, c=24, n=2, h=9, w=7, **kw):
    return K(seed, n, h, w, c, c, c, **kw)


# the fast depthwise kernel: N = 2, 9 x 7, C = 24.  OW = 7 (4 at stride 2) is ragged against PX = 2 and 4 and pixel groups cross the image boundary.
# Every (k, s) without an activation ...
DW_PLAIN = [DW(1, k=3, stride=1, pre="bn", res=True, bias=True, relu=True), DW(2, k=3, stride=2, post_bn=True, clip=(0.0, 6.0)),
            DW(3, k=5, stride=1, bias=True, clip=(None, 0.7)), DW(4, k=5, stride=2, post_bn=True)]
# ... and with a fused one: hardswish, sigmoid and a prologue activation each appear for k = 3 and for k = 5
DW_ACT = [DW(5, k=3, stride=1, post_bn=True, res=True, act="hswish"), DW(6, k=3, stride=2, bias=True, act="sigmoid"), DW(7, k=3, stride=1, pre="sigmoid", bias=True),
          DW(8, k=5, stride=1, pre="hswish", bias=True), DW(9, k=5, stride=2, bias=True, act="hswish"), DW(10, k=5, stride=2, post_bn=True, act="sigmoid"),
          DW(11, k=3, stride=2, pre="hswish"), DW(12, k=5, stride=1, act="hardsigmoid", bias=True)]
# edges: OW = 2 < PX on one fp16 vector; asymmetric SAME pads at stride 2; (1, 0, 2, 1) at k5; pad 0; the prologue's upper bound (pre_clip);
# a store at channel offset 8 (pitch C + 8), a read at channel offset 8 of a wider buffer, a single output
DW_EDGE = [DW(13, c=8, n=1, h=3, w=3, k=3, stride=2, bias=True), DW(14, k=3, stride=2, pads=(0, 0, 1, 1), bias=True), DW(15, k=3, stride=2, pads=(1, 1, 0, 0), bias=True),
           DW(16, k=5, stride=1, pads=(1, 0, 2, 1), bias=True, clip=(-0.3, None)), DW(17, k=3, stride=1, pads=(0, 0, 0, 0), bias=True),
           DW(18, k=3, stride=1, pre="clip", bias=True), DW(19, k=3, stride=1, bias=True, out="offset"), DW(20, k=5, stride=1, post_bn=True, slice_in=True, out="single"),
           DW(21, k=5, stride=2, bias=True, out="single")]
# the second round of the grid-stride loop: (case, precision, tile).  C = 1024: cvn = 256 (fp32) / 128 (fp16) channel vectors, so the grid holds at
# most 2048 / 4096 pixel groups; single output, no Concat.  (lift_weights stays exact up to 1330 channels.)
DW_ROUND2 = [(DW(22, c=1024, h=33, w=33, k=3, bias=True, out="single"), "fp32", 1), (DW(23, c=1024, h=47, w=47, k=3, bias=True, out="single"), "fp32", 2),
             (DW(24, c=1024, h=66, w=66, k=3, bias=True, out="single"), "fp32", 3), (DW(25, c=1024, h=65, w=65, k=3, bias=True, out="single"), "fp16", 1)]
# C = 20 is no multiple of fp16's 8-channel vector: a forced fast tile must plan the generic kernel there (fp32's vector is 4: it stays fast)
DW_C20 = DW(26, c=20, k=3, bias=True)
# the generic kernel only: C = 5, k = 7, kh != kw, the NCHW graph input itself (fp32 in an fp16 plan: mixed element types)
DW_GENERIC = [DW(27, c=5, k=3, stride=2, bias=True), DW(28, c=8, k=7, post_bn=True, relu=True), DW(29, c=8, k=(3, 5), bias=True),
              DW(30, c=3, k=3, direct=True, bias=True, out="single"), DW(31, c=3, k=5, stride=2, direct=True)]


def GR(seed, cpg, groups, cout, n=2, h=5, w=7, **kw):
    return K(seed, n, h, w, cpg * groups, groups, cout, **kw)


# the fast grouped kernel, one case per entry of kGroupedCfgs in its order: N = 2, 5 x 7, M = 70 = one full 64-pixel row and a tail of 6 (at PX = 4
# three of the four pixel slots are empty).  k in {1, 3, 5}; stride 2 with asymmetric pads (on a 10 x 14 input: the same 5 x 7 output); prologue +
# residual + ReLU; BN; an activation; half-exact weights on half of the cases (fp16: both rounded_operands counts)
GROUPED = [GR(40, 1, 16, 32, k=3, bias=True), GR(41, 2, 8, 16, k=3, pre="bn", res=True, relu=True, half_w=True), GR(42, 4, 8, 32, k=5, post_bn=True),
           GR(43, 8, 2, 16, h=10, w=14, k=3, stride=2, pads=(0, 0, 1, 1), bias=True, half_w=True), GR(44, 8, 3, 24, k=1, act="hswish", bias=True),
           GR(45, 16, 2, 32, k=3, bias=True, half_w=True), GR(46, 32, 2, 32, k=1, post_bn=True), GR(47, 64, 2, 32, k=3, half_w=True)]
# gpb = 1 with Cout / groups = 2 * opb: two channel blocks read the same group; a store at a channel offset and a read from a slice
GROUPED_MORE = [GR(48, 16, 2, 64, k=3, bias=True), GR(49, 4, 8, 32, k=3, bias=True, out="offset"), GR(50, 8, 2, 16, k=3, post_bn=True, slice_in=True, out="single", half_w=True)]
# the generic kernel: 3 channels per group (no fast configuration), 13 groups, k = 7
GROUPED_GENERIC = [GR(51, 3, 4, 8, k=3, bias=True), GR(52, 2, 13, 26, k=3, stride=2, post_bn=True, relu=True), GR(53, 8, 2, 16, k=7, bias=True)]
# a forced tile the registers do not admit falls back to the planner's default: (cpg, precision, forced tile) -> planned tile
GROUPED_FALLBACK = {(32, "fp32", 3): 1, (64, "fp32", 2): 1, (64, "fp32", 3): 1, (64, "fp16", 3): 2}

# dilated taps on the implicit GEMMs (test_kernel_maps_gpu.check_conv): k = 3, dilation 2 and 4 with pad = dilation and pad 0, stride 1 and 2,
# Cin 20 and 64, Cout 40, N = 2, 13 x 11
DILATED = [KM.C(70, 2, 13, 11, 20, 40, k=3, p=2, bias=1, post=1, dil=2), KM.C(71, 2, 13, 11, 64, 40, k=3, s=2, p=0, pre=1, dil=2),
           KM.C(72, 2, 13, 11, 20, 40, k=3, s=2, p=4, post=2, dil=4), KM.C(73, 2, 13, 11, 64, 40, k=3, p=0, bias=1, dil=4),
           KM.C(74, 2, 13, 11, 64, 40, k=3, p=2, pre=1, post=3, hw=1, dil=2)]

SEEN = set()          # every label a test of this module saw launched


# ---- reference, runner ---------------------------------------------------------------------------------------------------------------------
def inputs(d):
    return [d["x"]] + [G.grid_input(np.random.RandomState(9000 * i + d["seed"]), d["n"], d["h"], d["w"]) for i in (1, 2)]


@functools.lru_cache(maxsize=None)
def reference(case, run, prec, dot):
    """The yardstick of input `run` of a case, in the shape of channel_graphs.copies(): dict(ref, S, extra, L_rest, ce, parts)"""
    d = build(case)
    op = CG.channel_operands(d, inputs(d)[run], prec == "fp16", dot)
    args = (op["w"], d["groups"], d["stride"], d["pads"], op["bias"], op["res"])
    ref_S = R.channel_ref64_S(op["xh"], *args)
    # (an affine prologue that rounds s * x before it adds t is as legal as the FMA: one more order)
    runs = [R.channel_chain32(op["xh2"], *args)] if op["xh2"] is not None else []
    ce, parts = R.channel_c_emul(op["xh"], *args, seed=d["seed"], extra_runs=runs, ref_S=ref_S)
    a = R.channel_allowance(*ref_S, ce, op["relu"], op["lo"], op["hi"], op["act"], op["rounded"], op["pre_act"], prec == "fp16", RTOL[prec])
    out = {k: CG.tile_copies(d, v) for k, v in a.items()}
    out.update(ce=ce, parts=parts)
    return out


def conv_step(steps):
    (st,) = [s for s in steps if "conv" in s["name"].split("+")]
    return st


def run_all(tmp_path, d, xs, env, prec):
    """-> (the step under test, its default tile, one output per input, its launched kernel): one model, one request per input"""
    path = models.write_repo(str(tmp_path), "t", d["model"])
    base = dict(IE_AUTOTUNE="0", IE_GROUPED_CONV="1", IE_PRECISION=prec)
    default = conv_step(plan_of(path, d["ishape"][0], base)["steps"])["tile"]
    st = conv_step(plan_of(path, d["ishape"][0], dict(base, **env))["steps"])
    run_env = {k: v for k, v in dict(base, **env).items() if k != "IE_AUTOTUNE"}          # (run_model sets IE_AUTOTUNE=0 itself)
    ys, kern = run_model(path, "t", run_env, [{"x": x} for x in xs], "out", d["oshape"], by_step=True)
    return st, default, ys, dict(kern)[st["name"]]


def written_check_applies(d):
    """Cases without ReLU, Clip or activation, in the epilogue or the prologue: a clamped or saturated value need not differ between inputs (and
    a prologue activation's allowance is a fraction of S, not of u S)"""
    return not (d["relu"] or d["clip"] or d["act"] or d["pre"])


def check(tmp_path, case, tile, prec, algo, want_tile=None, written_vector=1, keep=True):
    """want_tile: the tile the plan must name (None: the forced one); written_vector: kernel_ref.written_check_is_conclusive's granularity;
    keep: leave the references in the cache for the other tiles of the case (not the maps of millions of elements, which run once)"""
    d = build(case)
    xs = inputs(d)
    st, default, ys, label = run_all(tmp_path, d, xs, dict(IE_FORCE_TILE=str(tile)), prec)
    want_tile = tile if want_tile is None else default if want_tile == "default" else want_tile
    want_label = (dw_label if algo == "depthwise" else grouped_label)(d, prec, want_tile)
    assert st["algo"] == algo and st["tile"] == want_tile and label == want_label, (case, prec, st["algo"], st["tile"], label, want_label)
    SEEN.add(label)
    dot = algo == "grouped" and want_tile > 0 and prec == "fp16" and (d["c"] // d["groups"]) % 2 == 0
    refs = [(reference if keep else reference.__wrapped__)(case, run, prec, dot) for run in range(3)]
    shape = (d["n"], d["cout"], d["oh"], d["ow"])
    for run, (yfull, a) in enumerate(zip(ys, refs)):
        y = CG.copies(d, yfull)
        c, at = R.c_stat(y, a["ref"], a["S"], a["extra"])
        cls = R.position_class((at[0], at[1] % d["cout"], at[2], at[3]), shape, block=4 if algo == "depthwise" else 64)
        msg = f"{label} {prec} case {case[0]} run {run}: c {c:.2f} c_emul {a['ce']:.2f} worst {at} ({cls})"
        beyond = np.abs(y - a["ref"]) - R.MARGIN * a["ce"] * R.U * a["S"] - a["half"]          # (fp16: the half result's own rounding taken off)
        if d["act"]:
            ratio = float(((beyond - a["L_rest"]) / np.maximum(R.U * np.abs(a["ref"]), 1e-300)).max())
            msg += f"; activation ratio (|y - f(ref_z)| - L delta) / (u |f(ref_z)|) {ratio:.2f} of the {RTOL[prec] / R.U:.0f} allowed"
        if d["pre"] in ("hswish", "sigmoid"):
            ratio = float((beyond / (R.U * a["S"])).max())
            msg += f"; prologue activation ratio (|y - ref| - 2 c_emul u S) / (u S) {ratio:.2f} of the {RTOL[prec] / R.U:.0f} allowed"
        print(msg)
        assert c <= R.MARGIN * a["ce"], (f"{msg}: c > 2 x c_emul {a['parts']} at (n, channel, row, col) = {at}: got {y[at]!r}, ref64 {a['ref'][at]!r}, "
                                         f"S {a['S'][at]:.3e}, case {case}")
        if d["out"] == "offset":
            np.testing.assert_array_equal(yfull[:, :8], G.lifted(xs[run], d["w8"]))
    if written_check_applies(d):
        assert R.written_check_is_conclusive([(a["ref"], a["S"], a["extra"], a["ce"]) for a in refs], written_vector), "two of the three inputs must give distinguishable results at every element"
    return st


# ---- depthwise ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("tile", [1, 2, 3])
@pytest.mark.parametrize("case", DW_PLAIN + DW_ACT, ids=lambda c: f"case{c[0]}")
def test_depthwise_fast_kernel(tmp_path, case, tile, prec):
    check(tmp_path, case, tile, prec, "depthwise")


def test_depthwise_labels_step_down_with_an_activation():
    """fp32 k5 s2 with an activation forced to tile 3 reports px2, the fp16 version px1; without one both report px4"""
    d = build(DW_ACT[4])
    assert (d["kh"], d["stride"], d["act"]) == (5, 2, "hswish")
    assert dw_label(d, "fp32", 3) == "conv_dw_kernel<f32,k5,s2,px2,act>" and dw_label(d, "fp16", 3) == "conv_dw_kernel<f16,k5,s2,px1,act>"
    assert dw_label(build(DW_PLAIN[3]), "fp16", 3) == "conv_dw_kernel<f16,k5,s2,px4>"


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("tile", [1, 2, 3])
@pytest.mark.parametrize("case", DW_EDGE, ids=lambda c: f"case{c[0]}")
def test_depthwise_fast_kernel_edges(tmp_path, case, tile, prec):
    st = check(tmp_path, case, tile, prec, "depthwise")
    d = build(case)
    if d["out"] == "offset":
        assert (st["out"]["c_off"], st["out"]["pitch"]) == (8, d["c"] + 8)
    if d["slice_in"]:
        assert (st["in"]["c_off"], st["in"]["pitch"]) == (8, d["c"] + 8)
    if d["pre"] == "clip":
        assert st["pre_clip"] == CG.PRE_CLIP_HI and st["pre_relu"]


def round2_groups_and_slots(d, prec, tile):
    """launch_fast's formula: pixel groups, and the lanes-per-channel-vector the grid holds"""
    cvn = d["c"] // (8 if prec == "fp16" else 4)
    groups = d["n"] * d["oh"] * -(-d["ow"] // DW_PX[tile])
    return groups, max(1, min(groups, (256 * 2048 + cvn - 1) // cvn))


@pytest.mark.parametrize("case,prec,tile", DW_ROUND2, ids=[f"case{c[0]}_{p}_t{t}" for c, p, t in DW_ROUND2])
def test_depthwise_second_round_of_the_grid_stride_loop(tmp_path, case, prec, tile):
    groups, nslots = round2_groups_and_slots(build(case), prec, tile)
    assert groups > nslots, (groups, nslots)
    # fp16: 8.6 million half results.  Three half-precision bounds overlap at about one element per million by chance, so the written check is
    # made per 16-byte store of conv_dw_kernel<f16> (8 channels of a pixel), the unit the kernel writes or skips; fp32: per element
    check(tmp_path, case, tile, prec, "depthwise", written_vector=8 if prec == "fp16" else 1, keep=False)


@pytest.mark.parametrize("tile", [1, 2, 3])
def test_depthwise_c20_has_no_fp16_vector(tmp_path, tile):
    check(tmp_path, DW_C20, tile, "fp16", "depthwise", want_tile=0)
    check(tmp_path, DW_C20, tile, "fp32", "depthwise")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", DW_GENERIC + [DW_PLAIN[0], DW_ACT[3]], ids=lambda c: f"case{c[0]}")
def test_depthwise_generic_kernel(tmp_path, case, prec):
    st = check(tmp_path, case, 0, prec, "depthwise")
    if build(case)["direct"]:
        assert st["in"]["nchw"] and not st["in"]["f16"] and st["out"]["f16"] == (prec == "fp16")


# ---- grouped --------------------------------------------------------------------------------------------------------------------------------
def grouped_want_tile(case, prec, tile):
    d = build(case)
    return None if grouped_tile_fits(grouped_cfg_for(d["c"], d["cout"], d["groups"]), prec == "fp16", tile) else "default"


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("tile", [1, 2, 3])
@pytest.mark.parametrize("case", GROUPED + GROUPED_MORE, ids=lambda c: f"case{c[0]}")
def test_grouped_fast_kernel(tmp_path, case, tile, prec):
    d = build(case)
    st = check(tmp_path, case, tile, prec, "grouped", want_tile=grouped_want_tile(case, prec, tile))
    key = (d["c"] // d["groups"], prec, tile)
    if key in GROUPED_FALLBACK:
        assert st["tile"] == GROUPED_FALLBACK[key], (key, st["tile"])
    else:
        assert st["tile"] == tile
    if d["out"] == "offset":
        assert (st["out"]["c_off"], st["out"]["pitch"]) == (8, d["cout"] + 8)
    if d["slice_in"]:
        assert (st["in"]["c_off"], st["in"]["pitch"]) == (8, d["c"] + 8)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", GROUPED_GENERIC + [GROUPED[1], GROUPED[4]], ids=lambda c: f"case{c[0]}")
def test_grouped_generic_kernel(tmp_path, case, prec):
    check(tmp_path, case, 0, prec, "grouped")


# ---- dilated taps ----------------------------------------------------------------------------------------------------------------------------
def dilated_step(tmp_path, d, env, prec):
    path = models.write_repo(str(tmp_path), "k", d["model"])
    env = dict(env, **(dict(IE_PRECISION="fp16") if prec == "fp16" else {}))
    return KM.conv_step(plan_of(path, d["ishape"][0], env)["steps"])


def check_dilated(tmp_path, case, env, prec, tag, algo, tile):
    KM.check_conv(tmp_path, case, env, prec, tag, algo, tile)
    d = KM.build(case)
    st = dilated_step(tmp_path, d, env, prec)
    assert st["dilations"] == [d["dil"], d["dil"]], st


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("tile", range(7))
def test_dilated_igemm_vector_loader(tmp_path, tile, prec):
    """fp16: the MFMA loader takes 8-channel chunks, so the planner gives the Cin = 20 cases the naive kernel whatever is forced: they are checked
    on it, once"""
    for case in DILATED:
        if prec == "fp16" and KM.build(case)["cin"] % 8:
            if tile == 0:
                check_dilated(tmp_path, case, dict(IE_FORCE_ALGO="igemm", IE_FORCE_TILE="0"), prec, "dilated igemm (Cin % 8: naive)", "naive", None)
            continue
        check_dilated(tmp_path, case, dict(IE_FORCE_ALGO="igemm", IE_FORCE_TILE=str(tile)), prec, f"dilated igemm t{tile}", "igemm_vec", tile)


@pytest.mark.parametrize("algo,want", [("scalar", "igemm_scalar"), ("naive", "naive")])
def test_dilated_scalar_loader_and_naive(tmp_path, algo, want):
    for case in DILATED:
        check_dilated(tmp_path, case, dict(IE_FORCE_ALGO=algo, IE_FORCE_TILE="0"), "fp32", f"dilated {algo}", want, 0 if algo == "scalar" else None)


# ---- coverage: this test runs last ---------------------------------------------------------------------------------------------------------
def test_every_fast_instantiation_was_launched():
    """Every conv_dw_kernel<...> label DwLanePixels can produce and every conv_grouped_kernel<...> configuration x admitted px appeared in the
    Profile() labels the tests above collected (run the whole module: alone, this test has seen nothing)."""
    missing = (all_dw_labels() | all_grouped_labels()) - SEEN
    assert not missing, sorted(missing)
