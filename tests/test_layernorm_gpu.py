"""GPU (-m gpu): the layer-norm kernels on the MI355X against the float64 restatement of the ONNX definition in tests/ref64.py, per
element, with the project's bounds (tests/test_gpu_parity.py): fp32 within 2e-4 of max|ref|, fp16 within 3e-3.

Graph of every case but the last two: fp32 x [N, C, H, W] -> Transpose(0,2,3,1) -> LayerNormalization -> Transpose(0,3,1,2) -> y.  Every case runs
on the planner's default tile and on every eligible one (IE_FORCE_TILE 0 ... 4), and the Profile label must be the kernel the plan's tile names.
N, H, W = 2, 3, 5: 30 pixel rows, a multiple of no tile's rows per workgroup (4 for the generic kernel; 32 / 16 / 8 / 4 for tiles 1-4).
C: 6 generic only; 8 one fp16 vector; 96 a partly idle lane group; 100 fp32-fast but fp16-generic; 768 a full group; 1536 the largest row held in
registers (fp32); 1540 just past it."""

import numpy as np
import pytest

import convnext_graphs as G
import ref64
from engine_run import plan_of, RTOL, run_model
from gpu_ai_inference_server_amd.modelgen import models
from oracle import onnx_oracle as O

pytestmark = pytest.mark.gpu
N, H, W = 2, 3, 5


def _every_tile(path, name, prec, x, oshape, check, expect_fast=None):
    """check(y, tile) on the default tile and on each forced tile the plan accepts; -> the tiles that ran"""
    ran = []
    for forced in (None, 0, 1, 2, 3, 4):
        env = dict(IE_PRECISION=prec, **({} if forced is None else {"IE_FORCE_TILE": str(forced)}))
        (ln,) = [s for s in plan_of(path, x.shape[0], env)["steps"] if s["kind"] == "layer_norm"]
        if forced is not None and ln["tile"] != forced:
            assert ln["tile"] == 0                      # not eligible: the generic kernel, which forced tile 0 runs
            continue
        y, kern = run_model(path, name, env, {"x": x}, "y", oshape, by_step=True)
        kern = dict(kern)
        assert kern["ln"] == G.ln_label(ln["tile"], ln["out"]["f16"]), (forced, ln["tile"], kern["ln"])
        check(y, ln["tile"], forced)
        ran.append(ln["tile"])
    if expect_fast is not None:
        assert sorted(set(ran)) == sorted({0} | set(expect_fast)), ran
    return ran


def _ref_of(mb, x):
    return ref64.run_f64(mb, {"x": x})["y"]


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("c", [6, 8, 96, 100, 768, 1536, 1540])
def test_layer_norm(tmp_path, c, eps, prec):
    mb = G.ln_graph(N, c, H, W, eps=eps)
    path = models.write_repo(str(tmp_path), "ln", mb)
    x = (0.5 + np.random.RandomState(c).randn(N, c, H, W)).astype(np.float32)
    ref = _ref_of(mb, x)

    def check(y, tile, forced):
        err = np.abs(y.astype(np.float64) - ref).max() / np.abs(ref).max()
        print(f"C {c} eps {eps} {prec} forced {forced} tile {tile}: max err / max|ref| {err:.3e}")
        assert err < RTOL[prec], (c, eps, prec, tile, err)

    # fp32 buffers only where the plan is fp32: an fp16 plan's layer norm reads and writes halfs
    _every_tile(path, "ln", prec, x, (N, c, H, W), check, expect_fast=[t for t in (1, 2, 3, 4) if G.ln_tile_fits(c, prec == "fp16", t)])


@pytest.mark.parametrize("c", [6, 96, 768, 1024])
def test_large_mean(tmp_path, c):
    """x = 100 + N(0, 1) in fp32.  The centred two-pass evaluation in fp32 stays within 3.1e-5 of max|ref| (numpy, these shapes); the one-pass
    E[x^2] - mean^2 lands at 2.3e-3 ... 5.8e-2: the 2e-4 bound separates the two by ~7x on either side."""
    mb = G.ln_graph(N, c, H, W, eps=1e-5)
    path = models.write_repo(str(tmp_path), "lnm", mb)
    x = (100.0 + np.random.RandomState(100 + c).randn(N, c, H, W)).astype(np.float32)
    ref = _ref_of(mb, x)

    def check(y, tile, forced):
        err = np.abs(y.astype(np.float64) - ref).max() / np.abs(ref).max()
        print(f"large mean C {c} forced {forced} tile {tile}: max err / max|ref| {err:.3e}")
        assert err < RTOL["fp32"], (c, tile, err)

    _every_tile(path, "lnm", "fp32", x, (N, c, H, W), check)


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("c", [6, 96, 768])
def test_constant_row(tmp_path, c, prec):
    """One pixel row of a constant (1.3) inside a random tensor: its variance is 0, the reference there is beta exactly, the kernel's output is
    finite and within the bound of it.  (eps = 1e-5: the fp32 mean of C equal values is off by a few ulp of 1.3, ~1e-7 each, which
    rsqrt(eps) = 316 turns into ~1e-4 of the output: an order of magnitude inside 2e-4 x max|ref| ~ 7e-4.)"""
    mb = G.ln_graph(N, c, H, W, eps=1e-5)
    path = models.write_repo(str(tmp_path), "lnc", mb)
    x = np.random.RandomState(7 + c).randn(N, c, H, W).astype(np.float32)
    x[1, :, 2, 3] = 1.3
    ref = _ref_of(mb, x)
    beta = O.load_model(mb).inits["ln_B"].astype(np.float64)
    np.testing.assert_allclose(ref[1, :, 2, 3], beta, rtol=0, atol=1e-12)

    def check(y, tile, forced):
        assert np.isfinite(y).all()
        bound = RTOL[prec] * np.abs(ref).max()
        row = np.abs(y[1, :, 2, 3].astype(np.float64) - beta).max()
        print(f"constant row C {c} {prec} forced {forced} tile {tile}: |row - beta| {row:.3e} (bound {bound:.3e}), tensor {np.abs(y - ref).max():.3e}")
        assert row < bound and np.abs(y - ref).max() < bound

    _every_tile(path, "lnc", prec, x, (N, c, H, W), check)


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("c", [6, 8])
def test_layer_norm_into_a_concat(tmp_path, c, prec):
    """The norm's input is channels [0, C) of the concat's pixel rows and its output channels [C, 2C): pitch > c on both sides, c_off > 0 on the output.
    C = 6: the offset is no multiple of the vector width, only the generic kernel may run"""
    mb = G.ln_concat_graph(N, c, H, W)
    path = models.write_repo(str(tmp_path), "lncat", mb)
    x = np.random.RandomState(c).randn(N, 4, H, W).astype(np.float32)
    ref = _ref_of(mb, x)
    plan = plan_of(path, N, dict(IE_PRECISION=prec))
    (ln,) = [s for s in plan["steps"] if s["kind"] == "layer_norm"]
    assert (ln["in"]["c_off"], ln["in"]["pitch"], ln["out"]["c_off"], ln["out"]["pitch"], ln["in"]["buf"]) == (0, 2 * c, c, 2 * c, ln["out"]["buf"])
    assert [s["name"] for s in plan["steps"] if s["kind"] == "copy"] == ["to_output(y)"]

    def check(y, tile, forced):
        err = np.abs(y.astype(np.float64) - ref).max() / np.abs(ref).max()
        print(f"concat C {c} {prec} forced {forced} tile {tile}: max err / max|ref| {err:.3e}")
        assert err < RTOL[prec], (c, prec, tile, err)

    _every_tile(path, "lncat", prec, x, (N, 2 * c, H, W), check, expect_fast=[1, 2, 3, 4] if c == 8 else [])


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_layer_norm_of_pooled_vectors(tmp_path, prec):
    """the [N, C, 1, 1] case (ConvNeXt's head) with N = 3"""
    mb = G.ln_graph(3, 96, 1, 1)
    path = models.write_repo(str(tmp_path), "lnv", mb)
    x = np.random.RandomState(3).randn(3, 96, 1, 1).astype(np.float32)
    ref = _ref_of(mb, x)

    def check(y, tile, forced):
        err = np.abs(y.astype(np.float64) - ref).max() / np.abs(ref).max()
        print(f"[3, 96, 1, 1] {prec} forced {forced} tile {tile}: max err / max|ref| {err:.3e}")
        assert err < RTOL[prec], (prec, tile, err)

    _every_tile(path, "lnv", prec, x, (3, 96, 1, 1), check)
