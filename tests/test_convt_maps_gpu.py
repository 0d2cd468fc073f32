"""GPU (-m gpu): the transposed-convolution kernels checked per element on the feature map they write, the way tests/test_kernel_maps_gpu.py
checks the conv families.

Each case is a single-step graph with exact operands (tests/convt_graphs.map_case): it forces the tile with IE_FORCE_TILE, asserts through
Profile() that this kernel ran, and holds every element to  |y - ref64| <= 2 * c_emul * u * S  (tests/kernel_ref.py), ref64, S and c_emul
computed on the CPU from the op's im2col form (convt_graphs.convt_im2col: the zero-stuffed input against the flipped weights), plus the derived
half-rounding terms in fp16 mode.  Every case runs three times on one model with three different inputs: an element the kernel never wrote
would hold one and the same value in all three results, so three results that each meet their bound prove that every element of the step is
written wherever two of the references lie further apart than their bounds together -- which is asserted for every element of the cases
without a ReLU (their references have no zeros)."""
import functools
import os

import numpy as np
import pytest

import convt_graphs as TG
import kernel_graphs as G
import kernel_ref as R
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models

pytestmark = pytest.mark.gpu

# (seed, n, h, w, cin, cout, k, stride, bias, post, half_w).  Pixel tails: n * h * w is no multiple of 32 (nor of 64) and a pixel block
# straddles two images; Cout = 40: a full 32-channel block and a tail of 8; 9 taps: two full tap groups and one single tap.  (The seeds are
# data seeds: each no-ReLU case's three references are pairwise distinguishable at every element, see written_check_is_conclusive.)
FAST = [(1, 2, 7, 5, 64, 40, (2, 2), (2, 2), 1, 0, 0), (2, 3, 5, 9, 32, 40, (3, 3), (3, 3), 1, 2, 0), (3, 2, 9, 7, 48, 40, (2, 4), (2, 4), 0, 1, 0),
        (14, 1, 6, 7, 128, 8, (2, 2), (2, 2), 1, 3, 1), (5, 2, 11, 13, 16, 72, (2, 2), (2, 2), 1, 0, 1)]
# the generic kernel: overlapping taps, asymmetric pads, output_padding, odd channel counts
GENERIC = [(6, 2, 7, 5, 24, 40, (3, 3), (2, 2), (1, 1, 1, 1), (1, 1), 1, 0), (7, 2, 5, 6, 6, 5, (4, 3), (2, 3), (0, 2, 3, 1), (1, 2), 1, 2),
           (8, 1, 4, 5, 64, 16, (5, 5), (1, 1), (2, 0, 1, 4), (0, 0), 0, 1), (9, 2, 6, 4, 32, 40, (2, 2), (2, 2), (0, 0, 0, 0), (0, 0), 1, 3)]


@functools.lru_cache(maxsize=None)
def build_fast(case):
    seed, n, h, w, cin, cout, k, s, bias, post, hw = case
    return TG.map_case(seed, n, h, w, cin, cout, k, s, bias=bool(bias), post=post, half_w=bool(hw))


@functools.lru_cache(maxsize=None)
def build_generic(case):
    seed, n, h, w, cin, cout, k, s, pads, op, bias, post = case
    return TG.map_case(seed, n, h, w, cin, cout, k, s, pads, op, bias=bool(bias), post=post)


def inputs(d):
    return [d["x"]] + [G.grid_input(np.random.RandomState(9000 * i + d["seed"]), d["n"], d["h"], d["w"]) for i in (1, 2)]


def reference(d, x, prec, half_weights):
    """(ref64, S, half terms, c_emul) in the graph's output shape [N, 2 Cout, OH, OW]"""
    cols, wm, b, relu, rounded = TG.map_operands(d, x, half_weights)
    ref, S = R.ref64_S(cols, wm, b, relu)
    ce, _ = R.c_emul(cols, wm, b, relu, seed=d["seed"])
    ref, S = G.two_copies(ref, d), G.two_copies(S, d)
    extra = R.half_terms(ref, S, half_out=True, rounded_operands=rounded) if prec == "fp16" else 0.0
    return ref, S, extra, ce


def run_all(tmp_path, d, xs, env, prec):
    path = models.write_repo(str(tmp_path), "t", d["model"])
    env = dict(env, IE_AUTOTUNE="0", **(dict(IE_PRECISION="fp16") if prec == "fp16" else {}))
    os.environ.update(env)
    try:
        steps = B.DescribeModel(path, d["ishape"][0])["plan"]["steps"]
        m = B.CreateModel(path, "t")
        try:
            ys = []
            for x in xs:
                r = m.Infer([B.TensorData("x", B.DataTypeFloat32, B.Shape(list(d["ishape"])), x)],
                            [B.OutputConfig("out", Shape=list(d["oshape"]), DataType="FLOAT32")])
                ys.append(r[0].Data.reshape(d["oshape"]).copy())
            prof = {p["name"]: p["kernel"] for p in B.Profile(m, 1)}
        finally:
            m.Destroy()
    finally:
        for k in env:
            os.environ.pop(k, None)
    (st,) = [s for s in steps if s["name"].split("+")[0] == "conv"]
    return st, ys, prof[st["name"]]


def check(tmp_path, d, tile, prec, want_label):
    xs = inputs(d)
    st, ys, label = run_all(tmp_path, d, xs, dict(IE_FORCE_TILE=str(tile)), prec)
    assert st["algo"] == "transposed" and st["tile"] == tile and label == want_label, (st["algo"], st["tile"], label)
    refs = [reference(d, x, prec, half_weights=(tile > 0 and prec == "fp16")) for x in xs]
    for run, (y, (ref, S, extra, ce)) in enumerate(zip(ys, refs)):
        c, at = R.c_stat(y, ref, S, extra)
        used = float((np.abs(y - ref) / np.maximum(R.MARGIN * ce * R.U * S + extra, 1e-300)).max())
        print(f"{want_label} {prec} case {d['seed']} run {run} k {d['k']} s {d['stride']} Cin {d['cin']}: c {c:.2f} c_emul {ce:.2f} worst {at}; largest |err| / bound {used:.2f}")
        assert c <= R.MARGIN * ce, (f"{want_label} {prec}: c {c:.2f} > 2 x c_emul {ce:.2f} at (n, channel, row, col) = {at}: got {y[at]!r}, ref64 {ref[at]!r}, "
                                    f"S {S[at]:.3e}, case {d['seed']} run {run}")
    if d["post"] in (0, 3) and d["bias"]:
        assert R.written_check_is_conclusive(refs), "two of the three inputs must give distinguishable results at every element"


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("tile", [1, 2])
@pytest.mark.parametrize("case", FAST, ids=lambda c: f"case{c[0]}")
def test_phase_kernel(tmp_path, case, tile, prec):
    d = build_fast(case)
    assert d["cin"] % 16 == 0 and (d["n"] * d["h"] * d["w"]) % 32 != 0
    check(tmp_path, d, tile, prec, f"convt_phase_kernel<{'f16' if prec == 'fp16' else 'f32'},px{32 * tile}>")


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("case", GENERIC + [c[:8] + ((0, 0, 0, 0), (0, 0)) + c[8:10] for c in FAST[:2]], ids=lambda c: f"case{c[0]}")
def test_generic_kernel(tmp_path, case, prec):
    check(tmp_path, build_generic(case), 0, prec, "convt_generic_kernel")
