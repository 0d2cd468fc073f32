"""GPU (-m gpu): every convolution kernel family and tile, and the pooling kernel, checked per element on the feature map it writes.

Each case is a single-step graph with exact operands (tests/kernel_graphs.py): it forces the family and tile with the engine's knobs,
asserts through Profile() -- which names the kernel that was LAUNCHED, not the one that was planned -- that this kernel, tile and split-K
ran, and holds every element the kernel wrote to  |y - ref64| <= 2 * c_emul * u * S  (tests/kernel_ref.py; c_emul is computed here on
the CPU from emulations of the case's own data, never from engine output), plus the derived half-rounding terms in fp16 mode.  A
failure names family, tile, c, c_emul and the worst (n, channel, row, col) with its position class.  The case tables are literal;
tests/test_kernel_maps_plan.py checks on the CPU that every entry plans onto the family and tile it names."""
import functools
import os

import numpy as np
import pytest

import kernel_graphs as G
import kernel_ref as R
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models

pytestmark = pytest.mark.gpu

# mirror of csrc/igemm_tiles.h (bm, bn, K groups, deep): what the igemm labels spell out
IGEMM_TILES = [(128, 128, 1, 0), (128, 64, 1, 0), (128, 32, 1, 0), (64, 64, 1, 0), (64, 32, 1, 0), (32, 32, 1, 0), (256, 32, 1, 0), (64, 64, 2, 0),
               (64, 64, 4, 0), (32, 32, 4, 0), (128, 64, 2, 0), (64, 64, 1, 1), (64, 64, 2, 1), (64, 64, 4, 1), (32, 32, 4, 1), (64, 32, 1, 1)]
NUM_IGEMM_BASE_TILES = 7          # the scalar loader has the K-group-free tiles only: a forced tile beyond them plans the heuristic one


def C(seed, n, h, w, cin, cout, k=1, s=1, p=0, pre=0, bias=0, post=0, hw=0, dil=1):
    """One conv case (kernel_graphs.conv_case arguments); post: 0 none, 1 ReLU, 2 BN + ReLU, 3 BN; hw: half-representable weights; a dilation
    other than 1 is a 14th entry (the undilated cases stay the 13-tuples they were)."""
    return (seed, n, h, w, cin, cout, k, s, p, bool(pre), bool(bias), post, bool(hw)) + ((dil,) if dil != 1 else ())


@functools.lru_cache(maxsize=None)
def build(case):
    seed, n, h, w, cin, cout, k, s, p, pre, bias, post, hw = case[:13]
    return G.conv_case(seed, n, h, w, cin, cout, k, s, p, pre, bias, post, hw, *case[13:])


# ---------------------------------------------------------------------------------------------------------------------
# case tables.  Every family has: a ragged last pixel block and a pixel block that straddles two images (N >= 2, H * W not a multiple
# of 16), the family's smallest K and one near its largest, Cout of one channel block and of several, and the prologue / bias / BN /
# ReLU variants the family supports (plan.cpp, ConvFacts::*_ok).
# ---------------------------------------------------------------------------------------------------------------------
IGEMM32 = [C(1, 2, 9, 7, 4, 5, pre=1, bias=1, post=1), C(2, 3, 7, 11, 96, 40, k=3, p=1, post=2), C(3, 2, 13, 10, 20, 130, k=5, s=2, p=2, bias=1),
           C(4, 2, 11, 9, 64, 64, k=3, s=2, pre=1, post=3), C(5, 1, 6, 5, 256, 32, k=3, p=1, bias=1, post=1)]
SCALAR32 = [C(6, 2, 9, 7, 3, 5, k=3, p=1, bias=1, post=1), C(7, 3, 12, 11, 18, 40, k=7, s=2, p=3, post=2), C(8, 2, 7, 9, 7, 130, bias=1),
            C(9, 1, 10, 9, 40, 32, k=5, p=2, pre=1, post=1)]
SPLITK = [C(2, 3, 7, 11, 96, 40, k=3, p=1, post=2), C(4, 2, 11, 9, 64, 64, k=3, s=2, pre=1, post=3), C(10, 2, 9, 7, 448, 24, pre=1, bias=1)]
IGEMM16 = [C(11, 2, 9, 7, 8, 16, hw=1), C(12, 3, 7, 11, 96, 40, k=3, p=1, bias=1, post=1, hw=1), C(13, 2, 13, 10, 24, 72, k=5, s=2, p=2, pre=1, post=2),
           C(14, 1, 6, 5, 256, 32, k=3, p=1, hw=1)]
RASTER = [C(15, 2, 5, 4, 8, 12, k=3, p=1), C(16, 2, 7, 33, 32, 32, k=3, p=1, bias=1, post=1), C(17, 3, 10, 9, 64, 48, k=3, p=1, post=2)]
WINO = [C(18, 2, 6, 6, 32, 32, k=3, p=1), C(19, 3, 10, 14, 64, 32, k=3, p=1, bias=1, post=1), C(20, 1, 28, 12, 256, 32, k=3, p=1, post=2)]
# fp32 weights-stationary 1x1: per tile (smallest K, largest K of the weight slice that fits the LDS); 68 / 132 output channels: more than
# the 64 a four-block variant refuses, % 4, ragged
WS32_K = {0: (16, 288), 1: (16, 288), 2: (16, 592), 3: (16, 592), 4: (16, 1008), 5: (16, 1008), 6: (16, 288), 7: (16, 288), 8: (16, 592), 9: (16, 592),
          10: (16, 1008), 11: (16, 1008), 12: (128, 1008), 13: (64, 1008), 14: (16, 288), 15: (16, 288), 16: (16, 592), 17: (16, 592), 18: (16, 1008),
          19: (16, 1008)}


def ws32_cases(tile):
    kmin, kmax = WS32_K[tile]
    return [C(21, 2, 9, 7, kmin, 68, pre=1, bias=1, post=1), C(22, 2, 13, 11, kmax, 132, post=2),
            C(23, 2, 95, 91, kmin, 68, bias=1)]          # 541 row blocks of 32: several rounds of the persistent loop


WS16_K = {t: (32, (288, 288, 608, 608, 1024, 1024)[t % 6]) for t in range(18)}


def ws16_cases(tile):
    kmin, kmax = WS16_K[tile]
    return [C(24, 2, 9, 7, kmin, 72, hw=1), C(25, 2, 13, 11, kmax, 136, pre=1, bias=1, post=1), C(26, 2, 95, 91, kmin, 72, bias=1, hw=1)]


WS16_3X3 = [C(27, 2, 9, 7, 8, 16, k=3, p=1, hw=1), C(28, 3, 10, 14, 64, 40, k=3, p=1, bias=1, post=2), C(29, 1, 6, 5, 128, 32, k=3, p=1, hw=1)]
# direct split-K: (waves, max chunks per wave) per tile; a chunk is 16 (fp32) / 32 (fp16) channels of one tap.  Per tile: (k, chunks) of a
# case with exactly `waves` chunks and of one near waves * max chunks
DIRECT_CHUNKS = {0: ((1, 8), (3, 63)), 1: ((1, 16), (3, 63)), 2: ((3, 9), (3, 72)), 3: ((1, 4), (3, 27)), 4: ((1, 12), (3, 72)), 5: ((1, 8), (1, 32))}
DIRECT_WAVES = {0: 8, 1: 16, 2: 9, 3: 4, 4: 12, 5: 8, 6: 8, 7: 8, 8: 4, 9: 4}


def direct_cases(tile, prec):
    cw = 32 if prec == "fp16" else 16
    (k0, c0), (k1, c1) = DIRECT_CHUNKS[tile]
    return [C(30, 2, 9, 7, cw * c0 // (k0 * k0), 34, k=k0, p=k0 // 2, pre=(k0 == 1), bias=1, post=1),
            C(31, 3, 7, 5, cw * c1 // (k1 * k1), 66, k=k1, p=k1 // 2, post=2, hw=(prec == "fp16"))]


WINDOW = [C(40, 2, 9, 7, 128, 32, pre=1, bias=1, post=1), C(41, 3, 7, 11, 128, 64, k=3, p=1, post=2), C(42, 2, 10, 9, 32, 96, k=5, p=2, bias=1)]
AS_COUT = {10: 128, 11: 64, 12: 256, 13: 64, 14: 64}


def as_cases(tile):
    co = AS_COUT[tile]
    return [C(43, 1, 5, 7, 16, co, bias=1, post=1), C(44, 2, 7, 13, 1008, co, pre=1), C(45, 3, 9, 9, 144, 2 * co, pre=1, bias=1, post=1)]


X6 = [C(46, 2, 9, 7, 32, 128, pre=1, bias=1, post=1), C(47, 3, 7, 11, 224, 256, post=1), C(48, 1, 6, 5, 1024, 128, pre=1)]
NAIVE = [C(49, 3, 7, 5, 5, 7, k=3, s=2, p=1, bias=1, post=1)]

# the 14 shapes test_gpu_parity._random_conv_graph draws for its seed 0 (RandomState(1000)), rebuilt with exact operands:
# (n, k, stride, pad, cin, cout, h, w, pre, post, bias)
RANDOM14 = [(5, 1, 2, 0, 4, 64, 3, 16, 0, 1, 0), (5, 3, 2, 1, 4, 1, 20, 21, 0, 2, 0), (3, 1, 1, 0, 96, 5, 18, 7, 1, 2, 1), (1, 1, 1, 0, 32, 64, 3, 11, 1, 0, 1),
            (5, 1, 2, 0, 12, 5, 5, 14, 0, 0, 1), (5, 1, 2, 0, 3, 40, 17, 11, 0, 0, 1), (5, 7, 1, 0, 32, 1, 14, 23, 1, 1, 0), (2, 3, 1, 0, 4, 128, 8, 17, 0, 2, 0),
            (3, 5, 1, 0, 64, 5, 10, 12, 0, 2, 0), (5, 5, 2, 0, 64, 100, 19, 9, 0, 0, 1), (2, 3, 2, 0, 64, 128, 6, 22, 1, 1, 1), (3, 5, 1, 2, 36, 40, 21, 10, 0, 2, 1),
            (5, 5, 1, 0, 36, 1, 10, 21, 0, 1, 0), (5, 1, 1, 0, 12, 5, 3, 8, 0, 0, 0)]


def random14_case(i):
    n, k, s, p, cin, cout, h, w, pre, post, bias = RANDOM14[i]
    return C(100 + i, n, h, w, cin, cout, k=k, s=s, p=p, pre=pre, bias=bias, post=post)


# (seed, n, h, w, c, k, stride, (top, left, bottom, right), count_include_pad): odd sizes, C = 3 / 20 / 64, symmetric and asymmetric pads
POOLS = [(1, 2, 7, 9, 3, 2, 2, (0, 0, 0, 0), 0), (2, 2, 7, 9, 20, 3, 2, (1, 1, 1, 1), 0), (3, 3, 11, 13, 64, 3, 1, (1, 1, 1, 1), 1), (4, 2, 8, 5, 20, 2, 1, (0, 0, 1, 1), 0),
         (5, 2, 9, 7, 64, 3, 2, (1, 0, 0, 1), 1), (6, 1, 5, 5, 20, 2, 2, (1, 1, 0, 0), 1), (7, 2, 6, 11, 3, 3, 1, (0, 1, 1, 0), 0)]


# ---------------------------------------------------------------------------------------------------------------------
# labels, reference, runner
# ---------------------------------------------------------------------------------------------------------------------
def label_of(st, prec):
    """The Profile() label of a planned conv step that runs on the kernel it was planned for."""
    a, t, sk = st["algo"], st["tile"], st["splitk"]
    f16 = prec == "fp16"
    if a in ("igemm_vec", "igemm_scalar"):
        bm, bn, kg, deep = IGEMM_TILES[t]
        return (("conv_igemm_f16_kernel<" if f16 else "conv_igemm_kernel<") + f"{bm}x{bn}" + (f"x{kg}kg" if kg > 1 else "") + (",deep" if deep else "") +
                (",vec" if a == "igemm_vec" else ",scalar") + (f",splitk{sk}" if sk > 1 else "") + ">")
    if a == "naive":
        return "conv_naive_kernel"
    if a == "raster3x3":
        return f"conv3x3_raster_kernel<t{t}" + (f",splitk{sk}" if sk > 1 else "") + ">"
    if a == "wino3x3":
        return ("conv3x3_wino_x6_kernel<t" if t >= 8 else "conv3x3_wino_kernel<t") + f"{t}>"
    if a == "ws1x1":
        return ("conv1x1_ws_f16_kernel<t" if f16 else "conv1x1_ws_f32_kernel<t") + f"{t}>"
    if a == "ws3x3":
        return f"conv3x3_ws_f16_kernel<t{t}>"
    if a == "conv1x1_x6":
        return f"conv1x1_x6_kernel<t{t}>"
    if a == "direct":
        k = "conv1x1_as_kernel<f32,t" if t >= 10 else "conv_win_kernel<f32,t" if t >= 6 else "conv_direct_kernel<f16,t" if f16 else "conv_direct_kernel<f32,t"
        return f"{k}{t}>"
    raise AssertionError(st)


def conv_step(steps):
    (st,) = [s for s in steps if s["name"].split("+")[0] == "conv"]
    return st


@functools.lru_cache(maxsize=None)
def reference(case, prec, nsplit=1, family=""):
    """(ref64, S, half terms, c_emul, {emulation: c}) of a case, all in the graph's output shape [N, 2 Cout, OH, OW]."""
    d = build(case)
    f16 = prec == "fp16"
    cols, wm, b, relu, rounded = G.conv_operands(d, f16)
    ref, S = R.ref64_S(cols, wm, b, relu)
    extra_runs = []
    if d["pre"] and not f16:
        # a loader that rounds s * x before it adds t is as legal as the FMA: its result on the same data is one more order
        p = d["pre_bn"]
        x2 = R.prologue32(G.lifted(d["x"], d["w0"]), *R.bn_affine(p["g"], p["b"], p["m"], p["v"]), fused=False)
        extra_runs.append(R.chain32(R.im2col(x2, d["k"], d["k"], d["stride"], (d["pad"],) * 4, d["dil"]).reshape(cols.shape), wm, b, relu=relu))
    if family in ("wino", "wino_x6"):
        wt = wm.reshape(d["cout"], 3, 3, d["cin"]).transpose(0, 3, 1, 2)
        yw = R.wino32(G.conv_xhat(d), wt, b, relu, x6=(family == "wino_x6"))
        extra_runs.append(yw.transpose(0, 2, 3, 1).reshape(-1, d["cout"]))
    if family == "x6":
        extra_runs.append(R.x6_32(cols, wm, b, relu))
    ce, parts = R.c_emul(cols, wm, b, relu, nsplit=nsplit, seed=d["seed"], extra_runs=extra_runs)
    ref, S = G.two_copies(ref, d), G.two_copies(S, d)
    extra = R.half_terms(ref, S, half_out=True, rounded_operands=rounded) if f16 else 0.0
    return ref, S, extra, ce, parts


def with_env(env, fn):
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k in env:
            os.environ.pop(k, None)


def run_graph(tmp_path, d, env, prec, runs=1):
    """-> (plan steps, outputs of `runs` inferences, {step name: launched kernel})."""
    path = models.write_repo(str(tmp_path), "k", d["model"])
    env = dict(env, **(dict(IE_PRECISION="fp16") if prec == "fp16" else {}))

    def go():
        steps = B.DescribeModel(path, d["ishape"][0])["plan"]["steps"]
        m = B.CreateModel(path, "k")
        try:
            ys = []
            for _ in range(runs):
                r = m.Infer([B.TensorData("x", B.DataTypeFloat32, B.Shape(list(d["ishape"])), d["x"])],
                            [B.OutputConfig("out", Shape=list(d["oshape"]), DataType="FLOAT32")])
                assert r[0].Shape.Dims == list(d["oshape"])
                ys.append(r[0].Data.reshape(d["oshape"]).copy())
            prof = {p["name"]: p["kernel"] for p in B.Profile(m, 1)}
        finally:
            m.Destroy()
        return steps, ys, prof
    return with_env(env, go)


def check_conv(tmp_path, case, env, prec, tag, want_algo=None, want_tile=None, want_splitk=None, nsplit=None, family="", runs=1):
    d = build(case)
    steps, ys, prof = run_graph(tmp_path, d, env, prec, runs)
    st = conv_step(steps)
    if want_algo is not None:
        assert st["algo"] == want_algo, (tag, case, st["algo"], st["tile"])
    if want_tile is not None:
        assert st["tile"] == want_tile, (tag, case, st["algo"], st["tile"])
    if want_splitk is not None:
        assert st["splitk"] == want_splitk, (tag, case, st["splitk"])
    label = prof[st["name"]]
    if want_algo is not None:
        assert label == label_of(st, prec), (tag, case, "launched", label, "planned", label_of(st, prec))
    ns = nsplit if nsplit is not None else st["splitk"]
    ref, S, extra, ce, parts = reference(case, prec, ns, family)
    y = ys[0]
    c, at = R.c_stat(y, ref, S, extra)
    cls = R.position_class((at[0], at[1] % d["cout"], at[2], at[3]), (d["n"], d["cout"], d["oh"], d["ow"]))
    used = float((np.abs(y - ref) / np.maximum(R.MARGIN * ce * R.U * S + extra, 1e-300)).max())
    print(f"{tag} {prec} {label} case {case[0]} K={d['k'] ** 2 * d['cin']}: c {c:.2f} c_emul {ce:.2f} worst {at} ({cls}); largest |err| / bound {used:.2f}")
    assert c <= R.MARGIN * ce, (f"{tag} {prec} {label}: c {c:.2f} > 2 x c_emul {ce:.2f} {parts} at (n, channel, row, col) = {at} ({cls}): "
                                f"got {y[at]!r}, ref64 {ref[at]!r}, S {S[at]:.3e}, case {case}")
    for y2 in ys[1:]:
        np.testing.assert_array_equal(y, y2)
    return c, ce


# ---------------------------------------------------------------------------------------------------------------------
# the operands are exact
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("n,h,w,cin", [(2, 9, 7, 3), (3, 5, 6, 20), (2, 13, 11, 64), (1, 4, 4, 256), (2, 8, 8, 728), (1, 5, 3, 1024)])
def test_lifted_tensor_is_bit_exact(tmp_path, prec, n, h, w, cin):
    """The tensor every case feeds its kernel: the engine's lifting conv equals numpy bit for bit in both precisions."""
    d = G.lift_case(200 + cin, n, h, w, cin)
    _, ys, prof = run_graph(tmp_path, d, {}, prec)
    print(f"lift {prec} cin {cin}: {sorted(prof.values())}")
    np.testing.assert_array_equal(ys[0], G.lifted(d["x"], d["w0"]))


# ---------------------------------------------------------------------------------------------------------------------
# the families
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", range(16))
def test_igemm_vector_loader_fp32(tmp_path, tile):
    for case in IGEMM32:
        check_conv(tmp_path, case, dict(IE_FORCE_ALGO="igemm", IE_FORCE_TILE=str(tile)), "fp32", f"igemm t{tile}", "igemm_vec", tile)


@pytest.mark.parametrize("tile", range(16))
def test_igemm_scalar_loader_fp32(tmp_path, tile):
    """Tiles 7-15 (K groups, deep prefetch) exist for the vector loader only: the planner gives the scalar loader its heuristic tile there."""
    for case in SCALAR32:
        check_conv(tmp_path, case, dict(IE_FORCE_ALGO="scalar", IE_FORCE_TILE=str(tile)), "fp32", f"scalar t{tile}", "igemm_scalar",
                   tile if tile < NUM_IGEMM_BASE_TILES else None)


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("in_launch", ["0", "1"])
@pytest.mark.parametrize("splitk", [2, 3, 7])
def test_igemm_split_k(tmp_path, splitk, in_launch, prec):
    for case in SPLITK:
        check_conv(tmp_path, case, dict(IE_FORCE_ALGO="igemm", IE_FORCE_TILE="4", IE_FORCE_SPLITK=str(splitk), IE_SPLITK_IN_LAUNCH=in_launch), prec,
                   f"igemm splitk{splitk} in-launch {in_launch}", "igemm_vec", 4, splitk, runs=2)


@pytest.mark.parametrize("tile", range(11))
def test_igemm_fp16(tmp_path, tile):
    for case in IGEMM16:
        check_conv(tmp_path, case, dict(IE_FORCE_ALGO="igemm", IE_FORCE_TILE=str(tile)), "fp16", f"igemm t{tile}", "igemm_vec", tile)


@pytest.mark.parametrize("splitk", [1, 2])
@pytest.mark.parametrize("tile", range(8))
def test_raster_3x3(tmp_path, tile, splitk):
    for case in RASTER:
        check_conv(tmp_path, case, dict(IE_FORCE_ALGO="raster", IE_FORCE_TILE=str(tile), IE_FORCE_SPLITK=str(splitk)), "fp32", f"raster t{tile} splitk{splitk}",
                   "raster3x3", tile, splitk)


@pytest.mark.parametrize("tile", range(12))
def test_winograd_3x3(tmp_path, tile):
    env = dict(IE_FORCE_ALGO="wino", IE_FORCE_TILE=str(tile), **(dict(IE_FP32_SPLIT="1") if tile >= 8 else {}))
    for case in WINO:
        check_conv(tmp_path, case, env, "fp32", f"wino t{tile}", "wino3x3", tile, family="wino_x6" if tile >= 8 else "wino")


@pytest.mark.parametrize("tile", range(20))
def test_weights_stationary_1x1_fp32(tmp_path, tile):
    for case in ws32_cases(tile):
        check_conv(tmp_path, case, dict(IE_FORCE_ALGO="ws", IE_FORCE_TILE=str(tile)), "fp32", f"ws t{tile}", "ws1x1", tile)


@pytest.mark.parametrize("tile", range(18))
def test_weights_stationary_1x1_fp16(tmp_path, tile):
    for case in ws16_cases(tile):
        check_conv(tmp_path, case, dict(IE_FORCE_ALGO="ws", IE_FORCE_TILE=str(tile)), "fp16", f"ws t{tile}", "ws1x1", tile)


@pytest.mark.parametrize("tile", range(5))
def test_weights_stationary_3x3_fp16(tmp_path, tile):
    for case in WS16_3X3:
        check_conv(tmp_path, case, dict(IE_FORCE_ALGO="ws", IE_FORCE_TILE=str(tile)), "fp16", f"ws3x3 t{tile}", "ws3x3", tile)


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("tile", range(6))
def test_direct_split_k(tmp_path, tile, prec):
    for case in direct_cases(tile, prec):
        check_conv(tmp_path, case, dict(IE_FORCE_ALGO="direct", IE_FORCE_TILE=str(tile)), prec, f"direct t{tile}", "direct", tile, nsplit=DIRECT_WAVES[tile])


@pytest.mark.parametrize("tile", [6, 7, 8, 9])
def test_direct_window(tmp_path, tile):
    for case in WINDOW:
        check_conv(tmp_path, case, dict(IE_FORCE_ALGO="direct", IE_FORCE_TILE=str(tile)), "fp32", f"window t{tile}", "direct", tile, nsplit=DIRECT_WAVES[tile])


@pytest.mark.parametrize("tile", [10, 11, 12, 13, 14])
def test_activations_stationary_1x1(tmp_path, tile):
    for case in as_cases(tile):
        check_conv(tmp_path, case, dict(IE_FORCE_ALGO="direct", IE_FORCE_TILE=str(tile)), "fp32", f"as t{tile}", "direct", tile)


@pytest.mark.parametrize("tile", [0, 1])
def test_bf16x6_1x1(tmp_path, tile):
    for case in X6:
        check_conv(tmp_path, case, dict(IE_FORCE_ALGO="x6", IE_FORCE_TILE=str(tile), IE_FP32_SPLIT="1"), "fp32", f"x6 t{tile}", "conv1x1_x6", tile, family="x6")


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_naive(tmp_path, prec):
    for case in NAIVE:
        check_conv(tmp_path, case, dict(IE_FORCE_ALGO="naive"), prec, "naive", "naive")


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("env", [dict(), dict(IE_AUTOTUNE="0")], ids=["searched", "planned"])
@pytest.mark.parametrize("i", range(14))
def test_planner_choice_on_random_shapes(tmp_path, i, env, prec):
    """Whatever the search (or, without it, the planner's default) picks for the 14 random shapes of test_random_conv_graphs_vs_oracle."""
    check_conv(tmp_path, random14_case(i), env, prec, f"random {i} {'planned' if env else 'searched'}", nsplit=1)


# ---------------------------------------------------------------------------------------------------------------------
# pools
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("is_max", [True, False], ids=["max", "avg"])
@pytest.mark.parametrize("pool", POOLS, ids=[f"p{p[0]}" for p in POOLS])
def test_pool_maps(tmp_path, pool, is_max, prec):
    """MaxPool of exact inputs is bit-exact (all-negative windows at a padded border included: padding never wins); AveragePool is a k*k-term
    fp32 sum and one scaling: within k*k * u * mean|window|, plus u_h |ref| for a half result."""
    seed, n, h, w, c, k, stride, pads, cip = pool
    d = G.pool_case(300 + seed, n, h, w, c, k, stride, pads, is_max, cip)
    _, ys, prof = run_graph(tmp_path, d, {}, prec)
    assert prof["pool"] == "pool_kernel", prof
    x = G.lifted(d["x"], d["w0"])
    ref, mabs = R.pool_ref(x, k, stride, pads, is_max, cip)
    err = np.abs(ys[0].astype(np.float64) - ref)
    at = tuple(int(v) for v in np.unravel_index(int(np.argmax(err)), err.shape))
    if is_max:
        assert (ref < 0).any()
        print(f"maxpool {prec} {pool}: max err {err.max():.1e}")
        assert err.max() == 0, (pool, prec, at, ys[0][at], ref[at])
    else:
        bound = k * k * R.U * mabs + (R.UH * np.abs(ref) if prec == "fp16" else 0.0)
        worst = float((err / np.maximum(bound, 1e-300)).max())
        print(f"avgpool {prec} {pool}: worst err / bound {worst:.3f} at {at}")
        assert np.all(err <= bound), (pool, prec, at, ys[0][at], ref[at], worst)


# ---------------------------------------------------------------------------------------------------------------------
# two-stage kernels: one launch writes two results
# ---------------------------------------------------------------------------------------------------------------------
# (seed, n, h, w, channels of the block input, dense layers): map widths 4 / 7 / 8 / 14 / 16, pixel counts that leave a ragged last tile
DENSE32 = [(60, 3, 4, 4, 64, 2), (61, 5, 7, 7, 64, 2), (62, 3, 8, 8, 96, 2), (63, 13, 14, 14, 64, 1), (64, 2, 16, 16, 64, 2)]
# fp16 chains: maps of at most 7 raster tiles; a block input of 192 channels and more lets consecutive layers share one launch
DENSE16 = [(70, 3, 4, 4, 64, 3), (71, 5, 7, 7, 192, 3), (72, 2, 8, 8, 96, 2), (73, 3, 14, 14, 224, 2)]


def run_outputs(tmp_path, d, env, prec):
    """-> (plan steps, {output name: array}, Profile() records) of a graph with several outputs."""
    path = models.write_repo(str(tmp_path), "k", d["model"])
    env = dict(env, **(dict(IE_PRECISION="fp16") if prec == "fp16" else {}))

    def go():
        steps = B.DescribeModel(path, d["ishape"][0])["plan"]["steps"]
        m = B.CreateModel(path, "k")
        try:
            r = m.Infer([B.TensorData("x", B.DataTypeFloat32, B.Shape(list(d["ishape"])), d["x"])],
                        [B.OutputConfig(nm, Shape=list(sh), DataType="FLOAT32") for nm, sh in d["outputs"]])
            out = {nm: t.Data.reshape(sh).copy() for (nm, sh), t in zip(d["outputs"], r)}
            prof = B.Profile(m, 1)
        finally:
            m.Destroy()
        return steps, out, prof
    return with_env(env, go)


def stage_check(tag, y, xin, wt, bias, k, relu, pre=None, seed=0):
    """One conv stage (stride 1, 'same' padding) of a multi-stage launch, from the input the GPU itself produced: the stage's own
    per-element bound, so that one stage's error cannot hide in the next one's."""
    xh = R.prologue32(xin, *pre) if pre else np.asarray(xin, np.float32)
    shape = (xin.shape[0], xin.shape[2], xin.shape[3])
    cols = R.im2col(xh, k, k, 1, (k // 2,) * 4).reshape(-1, k * k * xin.shape[1])
    wm = R.wmat(wt)
    runs = []
    if pre:
        x2 = R.prologue32(xin, *pre, fused=False)
        runs.append(R.chain32(R.im2col(x2, k, k, 1, (k // 2,) * 4).reshape(cols.shape), wm, bias, relu=relu))
    ref, S = R.ref64_S(cols, wm, bias, relu)
    ce, parts = R.c_emul(cols, wm, bias, relu, seed=seed, extra_runs=runs)
    ref, S = R.to_nchw(ref, shape), R.to_nchw(S, shape)
    c, at = R.c_stat(y, ref, S)
    cls = R.position_class(at, ref.shape)
    print(f"{tag}: c {c:.2f} c_emul {ce:.2f} worst {at} ({cls})")
    assert c <= R.MARGIN * ce, f"{tag}: c {c:.2f} > 2 x c_emul {ce:.2f} {parts} at (n, channel, row, col) = {at} ({cls}): got {y[at]!r}, ref64 {ref[at]!r}"


def folded_1x1(P):
    """(prologue scale / shift, w', b') of a dense layer's BN-ReLU-1x1-BN(-ReLU)."""
    a, b = P["bn1"], P["bn2"]
    return R.bn_affine(a["g"], a["b"], a["m"], a["v"]), R.fold32(P["w1"], None, *R.bn_affine(b["g"], b["b"], b["m"], b["v"]))


@pytest.mark.parametrize("fuse_tile", ["", "3", "4", "5"])
@pytest.mark.parametrize("dense", DENSE32, ids=[f"d{d[0]}" for d in DENSE32])
def test_fused_dense_layer_stages(tmp_path, dense, fuse_tile):
    """conv_dense_fused_kernel: the 3x3 growth conv of layer L and the 1x1 bottleneck conv of layer L + 1 in one launch.  The concat buffer and
    every bottleneck are graph outputs, so each stage is held to its own bound from the tensor the GPU produced before it."""
    seed, n, h, w, c0, layers = dense
    d = G.dense_case(seed, n, h, w, c0, layers, tail=True, expose=True)
    steps, out, prof = run_outputs(tmp_path, d, dict(IE_AUTOTUNE="0", **(dict(IE_FUSE_PB=fuse_tile) if fuse_tile else {})), "fp32")
    assert [p["name"] for p in prof] == [s["name"] for s in steps]
    tile = int(fuse_tile) if fuse_tile else (1 if n * h * w <= 2048 else 2)
    want = ("conv_dense_fused_ws_kernel<t" if tile >= 4 else "conv_dense_fused_kernel<t") + f"{tile}>"
    fused = [(s, p["kernel"]) for s, p in zip(steps, prof) if s.get("algo") == "dense_fused"]
    assert len(fused) == layers and all(s["tile"] == tile and k == want for s, k in fused), [(s["name"], s["tile"], k) for s, k in fused]
    cat = out["cat"]
    for l in range(1, layers + 1):
        lo = c0 + 32 * (l - 1)
        stage_check(f"fused {want} d{seed} layer {l} 3x3", cat[:, lo:lo + 32], out[f"b{l}"], d["layers"][l - 1]["w3"], None, 3, False, seed=seed)
        pre, (w1, b1) = folded_1x1(d["layers"][l])
        stage_check(f"fused {want} d{seed} layer {l + 1} 1x1", out["bott" if l == layers else f"b{l + 1}"], cat[:, :lo + 32], w1, b1, 1, True, pre=pre, seed=seed)
    np.testing.assert_array_equal(cat[:, :c0], G.lifted(d["x"], d["w0"]))


@pytest.mark.parametrize("dense", DENSE16, ids=[f"d{d[0]}" for d in DENSE16])
def test_dense_block_chain_stages(tmp_path, dense):
    """dense_block_f16_kernel: whole dense layers per launch, the bottleneck tensor kept in LDS as halfs.  Each layer's 32 new channels are
    held to the two-stage bound  2 c u (S2 + |W2| S1)  plus the derived half-rounding terms, from the concat slices the GPU itself wrote."""
    seed, n, h, w, c0, layers = dense
    d = G.dense_case(seed, n, h, w, c0, layers, tail=False, expose=False)
    steps, out, prof = run_outputs(tmp_path, d, dict(IE_AUTOTUNE="0"), "fp16")
    assert [p["name"] for p in prof] == [s["name"] for s in steps]
    chains = [(s, p["kernel"]) for s, p in zip(steps, prof) if s.get("algo") == "dense_block"]
    assert sum(len(s["parts"]) // 2 for s, _ in chains) == layers, [s["name"] for s in steps]
    assert all(k == f"dense_block_f16_kernel<{len(s['parts']) // 2} layers>" for s, k in chains), [k for _, k in chains]
    cat = out["cat"]
    np.testing.assert_array_equal(cat[:, :c0], G.lifted(d["x"], d["w0"]))
    shape = (n, h, w)
    for l in range(1, layers + 1):
        P = d["layers"][l - 1]
        c = c0 + 32 * (l - 1)
        (s1, t1), (w1, b1) = folded_1x1(P)
        xh = R.prologue32(cat[:, :c], R.half_exact(s1), R.half_exact(t1))
        cols1, wm1, wm3 = xh.transpose(0, 2, 3, 1).reshape(-1, c), R.wmat(w1), R.wmat(P["w3"])
        T, S1 = R.ref64_S(cols1, wm1, b1, relu=True)
        T, S1 = R.to_nchw(T, shape), R.to_nchw(S1, shape)
        cols3 = R.im2col(T, 3, 3, 1, (1, 1, 1, 1)).reshape(-1, 9 * 128)
        ref, S2 = R.ref64_S(cols3, wm3)
        ref, S2 = R.to_nchw(ref, shape), R.to_nchw(S2, shape)

        def apply_abs_w3(t):
            return R.to_nchw(R.im2col(np.abs(t), 3, 3, 1, (1, 1, 1, 1)).reshape(-1, 9 * 128) @ np.abs(wm3.astype(np.float64)).T, shape)
        scale = R.two_stage_scale(S1, S2, apply_abs_w3)
        half = R.two_stage_half_terms(S1, T, S2, ref, apply_abs_w3)
        ce = max(R.c_emul(cols1, wm1, b1, True, seed=seed)[0], R.c_emul(cols3.astype(np.float32), wm3, seed=seed)[0])
        y = cat[:, c:c + 32]
        cc, at = R.c_stat(y, ref, scale, half)
        raw = float((np.abs(y - ref) / np.maximum(half, 1e-300)).max())
        print(f"dense block d{seed} layer {l} K1={c}: c beyond the half terms {cc:.2f} c_emul {ce:.2f}; worst |err| / half terms {raw:.3f} at {at}")
        assert cc <= R.MARGIN * ce, f"dense block d{seed} layer {l}: c {cc:.2f} > 2 x c_emul {ce:.2f} at (n, channel, row, col) = {at}: got {y[at]!r}, ref64 {ref[at]!r}"
