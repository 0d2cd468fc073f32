"""CPU: the per-element yardstick of tests/kernel_ref.py tested on itself, so that the bound cannot quietly become meaningless.  For a
handful of conv shapes the bound MARGIN * c_emul * u * S (c_emul from the sequential chain and one random k order of the same data)
must accept every legal evaluation order and must reject each of a list of small wrong things, and the worst element it reports must
be where the fault was injected."""
import functools

import numpy as np
import pytest

import kernel_graphs as G
import kernel_ref as R
from oracle import onnx_oracle as O

f32, f64 = np.float32, np.float64

SHAPES = {
    "1x1_K16": dict(n=2, h=9, w=7, cin=16, cout=32, k=1, stride=1, pad=0),
    "1x1_K144": dict(n=2, h=9, w=7, cin=144, cout=32, k=1, stride=1, pad=0),
    "1x1_K1008": dict(n=2, h=9, w=7, cin=1008, cout=32, k=1, stride=1, pad=0),
    "3x3_C32": dict(n=2, h=8, w=10, cin=32, cout=32, k=3, stride=1, pad=1),
    "3x3_C128": dict(n=2, h=8, w=8, cin=128, cout=32, k=3, stride=1, pad=1),
    "5x5_s2": dict(n=2, h=11, w=13, cin=16, cout=32, k=5, stride=2, pad=2),
}
PADDED = ["3x3_C32", "3x3_C128", "5x5_s2"]          # (a 1x1 conv has no padding to misread)
DEEP = ["1x1_K144", "1x1_K1008", "3x3_C32", "3x3_C128", "5x5_s2"]     # K > 32: an accumulator rounded every 32 terms differs from one rounded at the end


class Case:
    def __init__(self, name, half=False):
        g = SHAPES[name]
        self.g = g
        rs = np.random.RandomState(sum(map(ord, name)))
        K = g["cin"] * g["k"] ** 2
        self.x = np.maximum(rs.randn(g["n"], g["cin"], g["h"], g["w"]), 0).astype(f32)       # post-ReLU-like
        self.w = (rs.randn(g["cout"], g["cin"], g["k"], g["k"]) * np.sqrt(2.0 / K)).astype(f32)    # He-scaled
        self.b = (0.2 * rs.randn(g["cout"])).astype(f32)
        if half:
            self.x, self.w, self.b = R.half_exact(self.x), R.half_exact(self.w), None
        self.cols5 = R.im2col(self.x, g["k"], g["k"], g["stride"], (g["pad"],) * 4)
        self.shape = self.cols5.shape[:3]
        self.cols = self.cols5.reshape(-1, K)
        self.wm = R.wmat(self.w)
        ref, S = R.ref64_S(self.cols, self.wm, self.b)
        self.ref, self.S = R.to_nchw(ref, self.shape), R.to_nchw(S, self.shape)
        self.c_emul, self.cs = R.c_emul(self.cols, self.wm, self.b)
        self.extra = R.half_terms(self.ref, self.S, half_out=True) if half else 0.0
        self.seq = self.nchw(R.chain32(self.cols, self.wm, self.b))

    def nchw(self, ym):
        return R.to_nchw(np.asarray(ym), self.shape)

    def c(self, y):
        return R.c_stat(y, self.ref, self.S, self.extra)

    def ok(self, y):
        return R.within(y, self.ref, self.S, self.c_emul, self.extra)


@functools.lru_cache(maxsize=None)
def case(name, half=False):
    return Case(name, half)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_emulation_statistic_is_small_and_does_not_grow_with_k(name):
    cs = case(name)
    print(f"{name}: K = {cs.wm.shape[1]}, c_emul {cs.c_emul:.2f} {cs.cs}")
    assert 0.5 < cs.c_emul < 8.0, cs.cs           # a handful of u * S whatever K is: rounding walk, not worst case K * u


@pytest.mark.parametrize("nsplit", [1, 3, 8])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_bound_accepts_chains_in_another_order(name, nsplit):
    cs = case(name)
    order = np.random.RandomState(977 + nsplit).permutation(cs.wm.shape[1])
    y = cs.nchw(R.chain32(cs.cols, cs.wm, cs.b, order=order, nsplit=nsplit))
    c, at = cs.c(y)
    print(f"{name} nsplit {nsplit}: c {c:.2f} at {at}, c_emul {cs.c_emul:.2f}")
    assert cs.ok(y), (c, cs.c_emul, at)
    y = cs.nchw(R.chain32(cs.cols, cs.wm, cs.b, nsplit=nsplit))
    assert cs.ok(y), (cs.c(y), cs.c_emul)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_bound_accepts_numpy_float32(name):
    cs = case(name)
    y = cs.nchw(R.numpy32(cs.cols, cs.wm, cs.b))
    assert cs.ok(y), (cs.c(y), cs.c_emul)


@pytest.mark.parametrize("name", ["3x3_C32", "3x3_C128"])
def test_bound_accepts_winograd(name):
    cs = case(name)
    y = R.wino32(cs.x, cs.w, cs.b)
    c, at = cs.c(y)
    print(f"{name} wino32: c {c:.2f} at {at}, c_emul {cs.c_emul:.2f}")
    assert cs.ok(y), (c, cs.c_emul, at)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_bf16x6_family_has_its_own_emulation(name):
    """The six kept products drop terms of the order of one fp32 rounding of each product: legal, and above the plain chain's c at large K.
    The family's bound therefore takes x6_32 into c_emul (not a wider margin); another blocking of the same product must then pass, and
    operands cut to 16 bits (the split without its low terms) must still fail."""
    cs = case(name)
    y6 = R.x6_32(cs.cols, cs.wm, cs.b)
    ce, parts = R.c_emul(cs.cols, cs.wm, cs.b, extra_runs=(y6,))
    y = cs.nchw(R.x6_32(cs.cols, cs.wm, cs.b, kblock=32))
    c, at = cs.c(y)
    print(f"{name} x6_32: c {c:.2f} at {at}, c_emul {ce:.2f} {parts}")
    assert R.within(y, cs.ref, cs.S, ce), (c, ce, at)
    y16 = cs.nchw(R.round_bits(cs.cols, 16) @ R.round_bits(cs.wm, 16).T + cs.b.astype(f64))
    assert not R.within(y16, cs.ref, cs.S, ce), (cs.c(y16), ce)


def test_three_bf16_terms_are_the_fp32_number():
    a = np.random.RandomState(3).randn(4096).astype(f32)
    x0, x1, x2 = R.split3(a)
    assert np.array_equal(x0.astype(f64) + x1.astype(f64) + x2.astype(f64), a.astype(f64))
    for p in (x0, x1, x2):
        assert not np.any(p.view(np.uint32) & np.uint32(0xFFFF))          # each term is a bf16 number


@pytest.mark.parametrize("bits", [16, 11])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_bound_rejects_rounded_operands(name, bits):
    """16 bits: a bf16 split that lost its low terms, a transform kept in bf16x2.  11 bits: a half staging buffer, a wrong kernel pick."""
    cs = case(name)
    y = R.round_bits(cs.cols, bits) @ R.round_bits(cs.wm, bits).T + cs.b.astype(f64)
    c, _ = cs.c(cs.nchw(y))
    print(f"{name} operands at {bits} bits: c {c:.0f} against 2 x c_emul = {2 * cs.c_emul:.1f}")
    assert not cs.ok(cs.nchw(y))
    assert c > (3 if bits == 16 else 100) * R.MARGIN * cs.c_emul          # and not by a whisker


def _mut_drop_chunk(cs):
    n, r = 1, cs.shape[1] // 2
    cols = cs.cols5.copy()
    cols[n, r, :, -1, -16:] = 0                      # the last 16-channel K chunk, on one output row
    return cs.nchw(R.chain32(cols.reshape(cs.cols.shape), cs.wm, cs.b)), lambda at: at[0] == n and at[2] == r


def _mut_skip_tap(cs):
    r = cs.shape[1] - 1
    tap = (cs.g["k"] ** 2) // 2                      # the centre tap: never padding
    cols = cs.cols5.copy()
    cols[:, r, :, tap, :] = 0
    return cs.nchw(R.chain32(cols.reshape(cs.cols.shape), cs.wm, cs.b)), lambda at: at[2] == r


def _mut_left_padding(cs):
    """The taps left of the image read x[row * W - 1], the previous row's last pixel, instead of zero."""
    g = cs.g
    k, pad, st = g["k"], g["pad"], g["stride"]
    cols = cs.cols5.copy()
    for oh in range(cs.shape[1]):
        for i in range(k):
            r = oh * st - pad + i
            if 1 <= r < g["h"]:
                cols[:, oh, 0, i * k + (pad - 1), :] = cs.x[:, :, r - 1, g["w"] - 1]        # column -1 of row r
    return cs.nchw(R.chain32(cols.reshape(cs.cols.shape), cs.wm, cs.b)), lambda at: at[3] == 0


def _mut_tile_doubled(cs):
    y = cs.seq.copy()
    y[0, 5, 2:4, 2:4] *= 2
    return y, lambda at: at[:2] == (0, 5) and at[2] in (2, 3) and at[3] in (2, 3)


def _mut_one_element(cs):
    at0 = (1, 17, cs.shape[1] - 2, 1)
    y = cs.seq.astype(f64)
    y[at0] += 4 * R.MARGIN * cs.c_emul * R.U * cs.S[at0]
    return y, lambda at: at == at0


def _mut_bias_block(cs):
    return cs.nchw(R.chain32(cs.cols, cs.wm, np.roll(cs.b, 16))), lambda at: True       # (every channel carries another block's bias)


MUTATIONS = {"last_k_chunk_dropped_on_one_row": _mut_drop_chunk, "tap_skipped_on_bottom_row": _mut_skip_tap, "tile_2x2_doubled": _mut_tile_doubled,
             "one_element_moved_by_4_bounds": _mut_one_element, "bias_of_the_wrong_channel_block": _mut_bias_block}


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_bound_rejects_and_locates(name, mutation):
    cs = case(name)
    y, where = MUTATIONS[mutation](cs)
    c, at = cs.c(y)
    print(f"{name} {mutation}: c {c:.0f} at {at} ({R.position_class(at, cs.ref.shape)}), 2 x c_emul = {2 * cs.c_emul:.1f}")
    assert not cs.ok(y), (c, cs.c_emul)
    assert where(at), at


@pytest.mark.parametrize("name", PADDED)
def test_bound_rejects_left_padding_that_reads_the_previous_row(name):
    cs = case(name)
    y, where = _mut_left_padding(cs)
    c, at = cs.c(y)
    print(f"{name} left padding: c {c:.0f} at {at}")
    assert not cs.ok(y) and where(at), (c, at)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_fp16_tight_bound_accepts_fp32_accumulation(name):
    """Half-representable operands: exact products, fp32 chain, the result rounded to half once."""
    cs = case(name, True)
    order = np.random.RandomState(5).permutation(cs.wm.shape[1])
    for y in (R.chain32(cs.cols, cs.wm), R.chain32(cs.cols, cs.wm, order=order, nsplit=3)):
        y = cs.nchw(y.astype(np.float16).astype(f32))
        assert cs.ok(y), (cs.c(y), cs.c_emul)


@pytest.mark.parametrize("name", DEEP)
def test_fp16_tight_bound_rejects_a_half_accumulator(name):
    cs = case(name, True)
    a, b = cs.cols.astype(f64), cs.wm.astype(f64)
    acc = np.zeros((a.shape[0], b.shape[0]), f32)
    for k0 in range(0, a.shape[1], 32):
        acc = R._chain(acc, a, b, range(k0, min(k0 + 32, a.shape[1]))).astype(np.float16).astype(f32)
    y = cs.nchw(acc)
    c, at = cs.c(y)
    print(f"{name} half accumulator: c {c:.0f} beyond u_h |ref|, 2 x c_emul = {2 * cs.c_emul:.1f}")
    assert not cs.ok(y)
    assert c > 10 * R.MARGIN * cs.c_emul


@pytest.mark.parametrize("pre,bias,post", [(False, False, 0), (False, True, 1), (True, True, 2), (True, False, 3)])
def test_ref64_agrees_with_the_graph_oracle(pre, bias, post):
    """kernel_ref's ref64 of a single-step graph against oracle.run(float64) of the same ONNX bytes: equal without BatchNorm, and within the
    float32 roundings of x_hat, s and w' (4 u S) with it."""
    d = G.conv_case(11, n=2, h=7, w=9, cin=20, cout=24, k=3, stride=2, pad=1, pre=pre, bias=bias, post=post)
    want = O.run(O.load_model(d["model"]), {"x": d["x"]}, dtype=np.float64)["out"]
    cols, wm, b, relu, _ = G.conv_operands(d)
    ref, S = R.ref64_S(cols, wm, b, relu)
    ref, S = G.two_copies(ref, d), G.two_copies(S, d)
    assert want.shape == ref.shape == tuple(d["oshape"])
    tol = (8 if (pre or post >= 2) else 1e-3) * R.U * S
    assert np.all(np.abs(want - ref) <= tol), float((np.abs(want - ref) / (R.U * S)).max())


def test_lifted_tensor_is_exact_and_has_distinct_channels():
    d = G.lift_case(3, 2, 5, 6, 64)
    y = G.lifted(d["x"], d["w0"])
    want = O.run(O.load_model(d["model"]), {"x": d["x"]}, dtype=np.float64)["out"]
    assert np.array_equal(want, y.astype(f64))
    assert len({tuple(t) for t in d["w0"].reshape(64, 3)}) == 64 and (y < 0).any()


@pytest.mark.parametrize("is_max", [True, False])
def test_pool_reference_agrees_with_the_graph_oracle(is_max):
    for cip, pads in ((0, (0, 0, 0, 0)), (1, (1, 1, 1, 1)), (0, (1, 0, 0, 1))):
        d = G.pool_case(5, 2, 7, 9, 20, 3, 2, pads, is_max, cip)
        want = O.run(O.load_model(d["model"]), {"x": d["x"]}, dtype=np.float64)["out"]
        ref, _ = R.pool_ref(G.lifted(d["x"], d["w0"]), 3, 2, pads, is_max, cip)
        assert want.shape == ref.shape and np.abs(want - ref).max() < 1e-12


def test_position_classes():
    shape = (2, 40, 6, 7)
    assert R.position_class((0, 3, 0, 3), shape) == "image border"
    assert R.position_class((1, 3, 2, 6), shape) == "image border"
    assert R.position_class((0, 33, 2, 2), shape) == "last channel block"
    assert R.position_class((0, 3, 2, 2), shape) == "tile-block border"         # pixel 16
    assert R.position_class((0, 3, 2, 4), shape) == "interior"


# ---------------------------------------------------------------------------------------------------------------------
# channel-local steps (depthwise, grouped): the reference against the graph oracle, and the mutants the per-element check must reject
# ---------------------------------------------------------------------------------------------------------------------
import channel_graphs as CG  # noqa: E402
import ref64  # noqa: E402
import test_channel_maps_gpu as CM  # noqa: E402  (the GPU tables: the mutants use their shapes)
from engine_run import RTOL  # noqa: E402


class ChannelCase:
    """One table entry of tests/test_channel_maps_gpu.py with its operands, yardstick and the plain fp32 chain of its first input.  small_block:
    (first channel, count) of output channels whose folded weights and bias are scaled by 2^-13 -- a block behind a small BatchNorm scale, the
    magnitude at which the old bound (a fraction of max|ref| of the whole output) sees nothing."""
    def __init__(self, case, prec="fp32", run=0, small_block=None):
        self.d = d = CM.build(case)
        self.prec, self.f16 = prec, prec == "fp16"
        self.x = CM.inputs(d)[run]
        dot = self.f16 and d["groups"] != d["c"] and (d["c"] // d["groups"]) % 2 == 0
        self.op = op = CG.channel_operands(d, self.x, self.f16, dot)
        if small_block is not None:
            lo, n = small_block
            op["w"] = op["w"].copy()
            op["w"][lo:lo + n] *= f32(2.0 ** -13)
            if op["bias"] is not None:
                op["bias"] = op["bias"].copy()
                op["bias"][lo:lo + n] *= f32(2.0 ** -13)
        self.geom = (d["groups"], d["stride"], d["pads"])
        self.zref, self.Sz = R.channel_ref64_S(op["xh"], op["w"], *self.geom, op["bias"], op["res"])
        runs = [R.channel_chain32(op["xh2"], op["w"], *self.geom, op["bias"], op["res"])] if op["xh2"] is not None else []
        self.c_emul, self.cs = R.channel_c_emul(op["xh"], op["w"], *self.geom, op["bias"], op["res"], seed=d["seed"], extra_runs=runs, ref_S=(self.zref, self.Sz))
        self.a = R.channel_allowance(self.zref, self.Sz, self.c_emul, op["relu"], op["lo"], op["hi"], op["act"], op["rounded"], op["pre_act"], self.f16, RTOL[prec])
        self.seq = self.finish(R.channel_chain32(op["xh"], op["w"], *self.geom, op["bias"], op["res"]))

    def finish(self, z):
        """the epilogue on a pre-activation result, as the kernel applies it (and the half store of fp16 mode)"""
        op = self.op
        y = R.act64(op["act"][0], R.clamp(np.asarray(z, f64), op["relu"], op["lo"], op["hi"]), *op["act"][1:])
        return y.astype(np.float16).astype(f64) if self.f16 else y.astype(f32).astype(f64)

    def c(self, y):
        return R.c_stat(y, self.a["ref"], self.a["S"], self.a["extra"])

    def ok(self, y):
        return self.c(y)[0] <= R.MARGIN * self.c_emul

    def old_ok(self, y):
        return ref64.rel_err(y, self.a["ref"]) < RTOL[self.prec]


@functools.lru_cache(maxsize=None)
def ccase(case, prec="fp32", run=0, small_block=None):
    return ChannelCase(case, prec, run, small_block)


CHANNEL_SAMPLE = CM.DW_PLAIN + CM.DW_ACT[:4] + CM.DW_EDGE[1:6] + CM.GROUPED + CM.GROUPED_GENERIC[:1]


@pytest.mark.parametrize("case", [CM.DW_PLAIN[0], CM.GROUPED[1], CM.DW_EDGE[3], CM.DW_EDGE[5], CM.DW_ACT[3], CM.GROUPED[4]], ids=lambda c: f"case{c[0]}")
def test_channel_reference_agrees_with_the_graph_oracle(case):
    """The prologue acts on in-range taps only (the ONNX graph pads the prologue's OUTPUT): kernel_ref's reference of a step with a BN + ReLU
    prologue and padding, depthwise and grouped, against tests/ref64.py's float64 walk of the same ONNX bytes, within the float32 roundings of
    x_hat, s and w' (8 u S); asymmetric pads, the prologue bound, a prologue activation and an epilogue activation likewise."""
    cs = ccase(case)
    d = cs.d
    want = ref64.run_f64(d["model"], {"x": cs.x})["out"]
    assert want.shape == tuple(d["oshape"])
    got = CG.tile_copies(d, cs.a["ref"])
    tol = CG.tile_copies(d, 8 * R.U * cs.a["S"] + 1e-6 * np.abs(cs.a["ref"]) * bool(d["act"]))          # (the hard activations' a = fl32(1 / 6) against 1 / 6)
    err = np.abs(CG.copies(d, want) - got)
    assert np.all(err <= tol), float((err / np.maximum(tol, 1e-300)).max())


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("case", CHANNEL_SAMPLE, ids=lambda c: f"case{c[0]}")
def test_channel_bound_accepts_the_kernels_order_and_another(case, prec):
    cs = ccase(case, prec)
    K = cs.op["w"][0].size
    for order in (None, np.random.RandomState(977).permutation(K)):
        op = cs.op
        xs = [op["xh"]] + ([op["xh2"]] if op["xh2"] is not None else [])
        for xh in xs:
            y = cs.finish(R.channel_chain32(xh, op["w"], *cs.geom, op["bias"], op["res"], order=order))
            assert cs.ok(y), (cs.c(y), cs.c_emul)
    print(f"case {case[0]} {prec}: c_emul {cs.c_emul:.2f} {cs.cs}")
    assert 0.4 < cs.c_emul < 8.0, cs.cs


def test_activation_lipschitz_constants_bound_the_difference_quotient():
    rs = np.random.RandomState(4)
    lo = rs.uniform(-8, 8, 4000)
    hi = lo + rs.uniform(0, 3, 4000) * rs.randint(0, 2, 4000)
    for kind, a, b in ((R.ACT_SIGMOID, 0, 0), (R.ACT_HARDSIGMOID, CG.HSIG_A, CG.HSIG_B), (R.ACT_SILU, 0, 0), (R.ACT_HARDSWISH, CG.HSWISH_A, CG.HSWISH_B)):
        L = R.act_lipschitz(kind, lo, hi, a, b)
        for t in np.linspace(0, 1, 33):
            p, q = lo + t * (hi - lo), lo + rs.rand(4000) * (hi - lo)
            assert np.all(np.abs(R.act64(kind, p, a, b) - R.act64(kind, q, a, b)) <= L * np.abs(p - q) * (1 + 1e-9) + 1e-15), kind
    assert abs(float(R.act_lipschitz(R.ACT_SILU, -9.0, 9.0)) - 1.0998) < 1e-4 and float(R.act_lipschitz(R.ACT_HARDSWISH, -9.0, 9.0, CG.HSWISH_A, 0.5)) == pytest.approx(1.5, abs=1e-6)
    assert float(R.act_lipschitz(R.ACT_HARDSIGMOID, 4.0, 5.0, CG.HSIG_A, 0.5)) == 0.0 and float(R.act_lipschitz(R.ACT_SIGMOID, -1.0, 2.0)) == 0.25
    # the sigmoid in float32 (one exp, one divide) meets E = RTOL |f| by orders of magnitude
    x = np.linspace(-8, 8, 4001).astype(f32)
    g = (f32(1) / (f32(1) + np.exp(-x).astype(f32))).astype(f32)
    assert np.all(np.abs(g - R.act64(R.ACT_SIGMOID, x)) <= 8 * R.U * R.act64(R.ACT_SIGMOID, x))


def _mut_prologue_on_padding(cs):
    """the prologue's shift also applied on the padding taps: x_hat = relu(t) there instead of 0"""
    d, op = cs.d, cs.op
    p = d["pre_bn"]
    s, t = R.bn_affine(p["g"], p["b"], p["m"], p["v"])
    pt, pl, pb_, pr = d["pads"]
    src = np.pad(G.lifted(cs.x, d["w0"]), ((0, 0), (0, 0), (pt, pb_), (pl, pr)))
    return cs.finish(R.channel_chain32(R.prologue32(src, s, t), op["w"], d["groups"], d["stride"], (0, 0, 0, 0), op["bias"], op["res"]))


def _mut_half_weights(cs):
    """the centre tap's weights rounded to half (all taps: with 9 terms and no averaging the old bound notices as well)"""
    op = cs.op
    w = op["w"].copy()
    w[:, :, w.shape[2] // 2, w.shape[3] // 2] = R.half_exact(w[:, :, w.shape[2] // 2, w.shape[3] // 2])
    return cs.finish(R.channel_chain32(op["xh"], w, *cs.geom, op["bias"], op["res"]))


def _mut_half_accumulator(cs):
    op = cs.op
    return cs.finish(R.channel_chain32(op["xh"], op["w"], *cs.geom, op["bias"], op["res"], half_acc=True))


def _smallest_S_channel(cs):
    return int(np.argmin(cs.Sz.max(axis=(0, 2, 3))))


def _mut_bias_twice(cs):
    ch = _smallest_S_channel(cs)
    z = R.channel_chain32(cs.op["xh"], cs.op["w"], *cs.geom, cs.op["bias"], cs.op["res"])
    z[:, ch] = (z[:, ch] + cs.op["bias"][ch]).astype(f32)
    return cs.finish(z), ch


def _mut_groups_swapped(cs, block):
    """one output block reads the NEXT group's input channels"""
    d, op = cs.d, cs.op
    lo, n = block
    cpg, opg = d["c"] // d["groups"], d["cout"] // d["groups"]
    g = lo // opg
    xh = op["xh"].copy()
    a, b = g * cpg, ((g + 1) % d["groups"]) * cpg
    xh[:, a:a + cpg], xh[:, b:b + cpg] = op["xh"][:, b:b + cpg], op["xh"][:, a:a + cpg]
    z = R.channel_chain32(op["xh"], op["w"], *cs.geom, op["bias"], op["res"])
    z[:, lo:lo + n] = R.channel_chain32(xh, op["w"], *cs.geom, op["bias"], op["res"])[:, lo:lo + n]
    return cs.finish(z)


@pytest.mark.parametrize("case", [CM.DW_PLAIN[0], CM.GROUPED[1]], ids=lambda c: f"case{c[0]}")
def test_channel_bound_rejects_a_prologue_on_padding_taps(case):
    """(this mutant is wrong by a whole tap at every border: the old global bound rejects it too, so only the new one is asserted)"""
    cs = ccase(case)
    y = _mut_prologue_on_padding(cs)
    c, at = cs.c(y)
    print(f"case {case[0]} prologue on padding: c {c:.0f} at {at}")
    sh = y.shape
    assert not cs.ok(y) and R.position_class(at, sh) == "image border"


@pytest.mark.parametrize("case", [CM.DW_PLAIN[3], CM.DW_EDGE[1], CM.DW_EDGE[2], CM.GROUPED_MORE[0], CM.GROUPED[2], CM.GROUPED[6]], ids=lambda c: f"case{c[0]}")
def test_channel_bound_rejects_half_rounded_weights_in_fp32_mode(case):
    cs = ccase(case)
    y = _mut_half_weights(cs)
    c, at = cs.c(y)
    print(f"case {case[0]} weights rounded to half: c {c:.0f} at {at}, 2 x c_emul {2 * cs.c_emul:.1f}; old bound {ref64.rel_err(y, cs.a['ref']):.1e}")
    assert not cs.ok(y) and c > 10 * R.MARGIN * cs.c_emul
    assert cs.old_ok(y)


@pytest.mark.parametrize("case", [CM.DW_PLAIN[3], CM.DW_EDGE[8], CM.GROUPED[5], CM.GROUPED[7]], ids=lambda c: f"case{c[0]}")
def test_channel_bound_rejects_a_half_accumulator(case):
    """fp16 mode (where a half accumulator is the tempting mistake): the sum rounded to half after every tap, against u_h |ref| for the one
    rounding of the result.  (Grouped cases with half-exact weights: where the v_dot2 path rounds the weights itself it is allowed u_h S.)"""
    cs = ccase(case, "fp16")
    assert cs.op["rounded"] == 0
    y = _mut_half_accumulator(cs)
    c, at = cs.c(y)
    print(f"case {case[0]} half accumulator: c {c:.0f} beyond the half terms at {at}; old bound {ref64.rel_err(y, cs.a['ref']):.1e}")
    assert not cs.ok(y) and c > 10 * R.MARGIN * cs.c_emul
    assert cs.old_ok(y)


@pytest.mark.parametrize("case,block", [(CM.DW_PLAIN[3], (8, 4)), (CM.DW_EDGE[4], (20, 4)), (CM.GROUPED[0], (16, 16)), (CM.GROUPED[5], (16, 16))], ids=lambda c: f"case{c[0]}" if len(c) > 2 else "")
def test_channel_bound_rejects_a_bias_added_twice_on_the_smallest_channel(case, block):
    cs = ccase(case, small_block=block)
    y, ch = _mut_bias_twice(cs)
    assert block[0] <= ch < block[0] + block[1]
    c, at = cs.c(y)
    print(f"case {case[0]} bias twice on channel {ch}: c {c:.0f} at {at}; old bound {ref64.rel_err(y, cs.a['ref']):.1e}")
    assert not cs.ok(y) and at[1] == ch
    assert cs.old_ok(y)


@pytest.mark.parametrize("case,block", [(CM.GROUPED[1], (0, 16)), (CM.GROUPED[2], (16, 16)), (CM.GROUPED[3], (8, 8)), (CM.GROUPED[5], (16, 16)), (CM.GROUPED_MORE[0], (32, 16))],
                         ids=lambda c: f"case{c[0]}" if len(c) > 2 else "")
def test_channel_bound_rejects_swapped_group_inputs(case, block):
    """One output block (a wave's channel block, behind a small BatchNorm scale) multiplies the neighbouring group's input channels"""
    cs = ccase(case, small_block=block)
    y = _mut_groups_swapped(cs, block)
    c, at = cs.c(y)
    print(f"case {case[0]} groups swapped for outputs {block}: c {c:.0f} at {at}; old bound {ref64.rel_err(y, cs.a['ref']):.1e}")
    assert not cs.ok(y) and block[0] <= at[1] < block[0] + block[1]
    assert cs.old_ok(y)


@pytest.mark.parametrize("case", [CM.DW_EDGE[1], CM.DW_EDGE[4], CM.DW_PLAIN[3]], ids=lambda c: f"case{c[0]}")
def test_three_inputs_catch_a_pixel_that_is_never_stored(case):
    """The last pixel of every PX = 4 group is not written: it keeps what the previous request left in the reused buffer.  With ONE input run again
    (what the graph tests do) that value is the correct one and every bound passes; with another input before it the per-element bound of the
    second run rejects it, at such a pixel."""
    a, b = ccase(case, run=0), ccase(case, run=1)
    ow = a.d["ow"]
    last = [x for x in range(ow) if x % 4 == 3 or x == ow - 1]
    stale_same, stale_other = b.seq.copy(), b.seq.copy()
    stale_other[..., last] = a.seq[..., last]
    assert b.ok(stale_same) and b.old_ok(stale_same)
    c, at = b.c(stale_other)
    assert not b.ok(stale_other) and at[3] in last, (c, at)
    refs = [ccase(case, run=r) for r in range(3)]
    assert R.written_check_is_conclusive([(r.a["ref"], r.a["S"], r.a["extra"], r.c_emul) for r in refs])
