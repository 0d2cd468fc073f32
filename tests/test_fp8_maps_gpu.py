"""GPU (-m gpu): the fp8 kernels checked code by code on the e4m3 maps they write.

Every case is one small graph of the only chain the fp8 mode admits (tests/fp8_graphs.py), planned with IE_KEEP_BUFFERS=1 so that every
step's input, shortcut and output can be read back with EngineReadBuffer.  Every step of it -- the stem, the expander, the step the case is
named after, the global pool -- is held to the interval oracle.fp8.emulate_step gives from the input the GPU itself wrote: the device's
code must be one the reference rounds to, which away from a rounding boundary is ONE code.  Profile() names the kernel that ran, tile
included; where a weights-stationary launcher declines a step, the tiled kernel's label is asserted instead and the map is still checked.
Each model runs twice and the two runs must agree byte for byte.  The case tables are literal; tests/test_fp8_maps_plan.py checks on the
CPU that every entry plans onto the kernel and tile it names and pins enough of every map."""
import numpy as np
import pytest

import fp8_graphs as G
from fp8_graphs import K

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------------------------------
# case tables: N = 3 on a 19 x 15 map (M = 855: a ragged last 32-pixel block, blocks that straddle images), K(seed, n, ih, iw, c0, ...)
# ---------------------------------------------------------------------------------------------------------------------
# conv_igemm_f8_kernel, each under every tile 0-6
IGEMM = [K(1, 3, 38, 30, 16, conv=(16, 1, 1, 0, 0, 1)),                      # 1x1, 16 -> 16: half an N block stored
         K(2, 3, 38, 30, 16, exp=144, conv=(48, 3, 1, 1, 1, 1)),             # 3x3, Cin 144: a 16-channel second K slice per tap, ragged N, bias
         K(3, 3, 38, 30, 64, exp=64, conv=(64, 1, 1, 0, 0, 0), short=1),     # identity shortcut from the stem output, its own scale
         K(4, 3, 38, 30, 16, exp=16, conv=(32, 5, 2, 2, 0, 1)),              # 5x5 / s2 / p2 on the odd map: 25 taps, border masks
         K(5, 3, 38, 30, 32, conv=(80, 3, 2, 1, 1, 1))]                      # 3x3 / s2 / p1, 32 -> 80


def ws1x1_cases(tile):
    """conv1x1_ws_f8_kernel: Cout = 32 * (tn / 2) + 16, the smallest the variant accepts, with a ragged last N tile.  The kernel takes input
    channels in multiples of 32 only, so Cin 16 and 272 (K % 32 == 16) are declined at launch and run tiled (asserted); Cin 32 and 288 run it."""
    cout = 32 * (G.WS8_TN[tile % 5] // 2) + 16
    return [K(6, 3, 38, 30, 16, conv=(cout, 1, 1, 0, 1, 1)), K(7, 3, 38, 30, 16, exp=272, conv=(cout, 1, 1, 0, 0, 1)),
            K(8, 3, 38, 30, 32, conv=(cout, 1, 1, 0, 1, 1)), K(9, 3, 38, 30, 32, exp=288, conv=(cout, 1, 1, 0, 0, 1)),
            K(10, 3, 38, 30, 48, exp=64, conv=(48, 1, 1, 0, 0, 0), short=1),          # shortcut from the stem (48 output channels: the tn = 2 variants take it)
            K(35, 3, 38, 30, 32, exp=cout + 16, conv=(cout + 16, 1, 1, 0, 0, 0), short=2),  # shortcut from the expander, 64 / 96 / 160 channels: every variant takes it
            K(11, 3, 38, 30, 32, conv=(cout, 1, 2, 0, 1, 1))]                          # STR: stride 2 from the odd 19 x 15 map


# DUAL: a projection block, projection stride 1 and 2, 32 channels on the projection's input and 64 on the other.  Without the search the
# dual step runs variant t1 (tn = 4) whatever IE_FORCE_TILE says
DUAL = [K(12, 3, 38, 30, 32, exp=64, dual=(96, 1)), K(13, 3, 38, 30, 32, exp=64, xs=2, dual=(96, 2))]
# conv3x3_ws_f8_kernel, each under every tile 200-207: Cin 32 / 160, Cout 16 / 48, map widths 15 / 8, raster rows that straddle images
WS3X3 = [K(14, 3, 38, 30, 32, conv=(16, 3, 1, 1, 1, 1)), K(15, 3, 38, 30, 32, pool=1, exp=160, conv=(48, 3, 1, 1, 0, 1)),
         K(16, 3, 38, 30, 32, exp=160, conv=(16, 3, 1, 1, 0, 1)), K(17, 3, 38, 30, 32, pool=1, conv=(48, 3, 1, 1, 1, 0))]
# pool_f8_kernel: max 3x3/s2/p1 on the odd map; average 2x2/s2 and 3x3/s1/p1, count_include_pad both ways; C = 16 and 48
POOLS = [K(18, 3, 38, 30, 16, exp=16, pl=("max", 3, 2, 1, 0)), K(19, 3, 38, 30, 48, exp=48, pl=("max", 3, 2, 1, 0)),
         K(20, 3, 38, 30, 48, exp=48, pl=("avg", 2, 2, 0, 0)), K(30, 3, 38, 30, 16, exp=16, pl=("avg", 2, 2, 0, 1)),
         K(22, 3, 38, 30, 48, exp=48, pl=("avg", 3, 1, 1, 0)), K(33, 3, 38, 30, 16, exp=16, pl=("avg", 3, 1, 1, 1))]
# (an average of a few e4m3 numbers lands EXACTLY on a rounding boundary whenever the ratio of the two tensor scales is a simple fraction, and with
# the CPU test's stand-in scales it is one: seeds 21 and 23 left 2.4 % and 1.4 % of their 16-channel maps undecided that way, so those two cases
# draw their data from seeds 30 and 33)
# the stem's e4m3 epilogues, alone and as stem + pool: C0 16 / 48 / 64 / 32, conv maps 20 x 15, 17 x 19, 16 x 17, 19 x 20.  Image widths 30 / 38 / 33 are no
# multiple of 4: the non-vector loader (kernels_stem.hip, stem_vec_ok); width 40: the 16-byte loader, the one a 224-pixel image takes
STEMS = [K(24, 3, 40, 30, 16, pool=1), K(25, 3, 33, 38, 48, pool=1), K(26, 2, 32, 33, 64, pool=1), K(34, 3, 38, 40, 32, pool=1)]
# gap_f8_kernel: C = 16 and 80 (a ragged second 64-channel block), HW = 285 and 3 (fewer pixels than its four pixel groups)
GAPS = [K(27, 3, 38, 30, 16, pool=1, exp=80, pl=("max", 8, 1, 0, 0)), K(28, 3, 38, 30, 16, pool=1, exp=16, pl=("max", 8, 1, 0, 0)), K(29, 3, 38, 30, 16, exp=80)]


def igemm_tile(tmp_path, case, tile):
    """The tile a forced tile gives the conv under test: tiles with bn > 32 keep the planner's own for Cout <= 32."""
    cout = case[8][0]
    if G.F8_TILES[tile][1] > 32 and cout <= 32:
        return under_test(G.planned(tmp_path, case, {})[1])["tile"]
    return tile


def under_test(plan):
    return plan["steps"][-2]          # the step in front of the global pool


def run_case(tmp_path, tag, case, env, algo=None, tile=None):
    path, plan, blob = G.planned(tmp_path, case, env)
    st = under_test(plan)
    if algo is not None:
        assert (st.get("algo", st["kind"]), st.get("tile")) == (algo, tile), (tag, case, st["name"], st.get("algo"), st.get("tile"))
    labels, scales, runs = G.device_run(path, case, env)
    assert len(labels) == len(plan["steps"]) == len(scales)
    base = G.planned(tmp_path, case, {k: v for k, v in env.items() if k != "IE_FORCE_TILE"})[1]["steps"]          # the heuristic tiles: what a declined step falls back to
    assert [b["name"] for b in base] == [s["name"] for s in plan["steps"]]
    for s, b, got in zip(plan["steps"], base, labels):
        want = G.launched_label(s, b)
        assert got.startswith(want) if want.endswith("<") else got == want, (tag, case, s["name"], "launched", got, "expected", want)
    for line in G.walk(tag, case, plan, blob, labels, scales, runs[0]):
        print(line)
    for b in runs[0]:
        np.testing.assert_array_equal(runs[0][b], runs[1][b])
    return plan, labels


@pytest.mark.parametrize("tile", range(7))
def test_tiled_fp8_conv(tmp_path, tile):
    for case in IGEMM:
        run_case(tmp_path, f"igemm_f8 t{tile}", case, dict(IE_FORCE_TILE=str(tile)), "igemm_f8", igemm_tile(tmp_path, case, tile))


@pytest.mark.parametrize("tile", range(100, 110))
def test_weights_stationary_1x1_fp8(tmp_path, tile):
    ran = 0
    for case in ws1x1_cases(tile):
        plan, labels = run_case(tmp_path, f"ws1x1_f8 t{tile}", case, dict(IE_FORCE_TILE=str(tile)), "igemm_f8", tile)
        ran += labels[-2] == f"conv1x1_ws_f8_kernel<t{tile - 100}>"
    assert ran >= 4          # Cin 32, Cin 288, the strided case and the shortcut from the expander


def test_dual_1x1_fp8(tmp_path):
    for case in DUAL:
        _, labels = run_case(tmp_path, "dual_f8", case, {}, "dual_f8", 1)
        assert labels[-2] == "conv1x1_ws_f8_kernel<dual,t1>"


@pytest.mark.parametrize("tile", range(200, 208))
def test_weights_stationary_3x3_fp8(tmp_path, tile):
    for case in WS3X3:
        run_case(tmp_path, f"ws3x3_f8 t{tile}", case, dict(IE_FORCE_TILE=str(tile)), "igemm_f8", tile)


@pytest.mark.parametrize("case", POOLS, ids=[f"k{c[0]}" for c in POOLS])
def test_pool_fp8(tmp_path, case):
    _, labels = run_case(tmp_path, "pool_f8", case, {}, "pool", None)
    assert labels[-2] == "pool_f8_kernel"


@pytest.mark.parametrize("fused", [True, False], ids=["stem+pool", "stem"])
@pytest.mark.parametrize("case", STEMS, ids=[f"k{c[0]}" for c in STEMS])
def test_stem_e4m3_epilogues(tmp_path, case, fused):
    _, labels = run_case(tmp_path, "stem", case, {} if fused else dict(IE_NO_STEM_POOL="1"), "stem_pool" if fused else "pool", 1 if fused else None)
    assert labels[0] == ("conv_stem_kernel<f16,pool,e4m3 out>" if fused else "conv_stem_kernel<f16,e4m3 out>")


@pytest.mark.parametrize("case", GAPS, ids=[f"k{c[0]}" for c in GAPS])
def test_global_pool_fp8(tmp_path, case):
    _, labels = run_case(tmp_path, "gap_f8", case, {})
    assert labels[-1] == "gap_f8_kernel"
