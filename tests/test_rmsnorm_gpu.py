"""GPU (-m gpu): the RMSNorm kernels on the MI355X against the float64 walk of the graph (tests/ref64.py with the operators tests/llama_graphs.py
registers), per element, with the project's bounds: fp32 within 2e-4 of max|ref|, fp16 within 3e-3.

Graph: fp32 x [N = 2, D, 1, L] -> tokens [N, L, D] -> RMSNorm spelled out (Pow -> ReduceMean -> Add -> Sqrt -> Div -> Mul -> Mul) -> back -> y.  The norm
is the last reader of its input, so its output takes over the input's buffer (out aliases in); test_not_the_last_reader keeps the input alive.
(L, D): (5, 64) one lane group per row with rows to spare in the workgroup; (33, 256) 66 rows: more than one workgroup on tiles 1 - 2 and a multiple of
no tile's rows per workgroup; (7, 50) no multiple of a vector: the generic kernel whatever is forced.
Row (0, 1) of every input is scaled by 1e4 (its largest element stays below 6e4, so the halfs an fp16 plan's norm reads are finite; the fp32 sum of
its squares is ~1e10) and row (1, 2) is all zeros: its result is 0 exactly (0 * rsqrt(eps)), not NaN."""

import numpy as np
import pytest

import convnext_graphs as CG
import llama_graphs as LG
import ref64
from engine_run import plan_of, RTOL, run_model
from gpu_ai_inference_server_amd.modelgen import models

pytestmark = pytest.mark.gpu
N = 2
SHAPES = [(5, 64), (33, 256), (7, 50)]


def _input(l, d):
    x = np.random.RandomState(l * d).randn(N, d, 1, l).astype(np.float32)
    x[0, :, 0, 1] *= np.float32(1e4)
    x[1, :, 0, 2] = 0.0
    assert np.abs(x).max() < 6e4
    return x


def _every_tile(path, name, prec, x, ref, d, step="rms_scale"):
    """the default tile and each forced tile the plan accepts: label, bound, finiteness, the zero row; -> the tiles that ran"""
    l = x.shape[3]
    ran = []
    for forced in (None, 0, 1, 2, 3, 4):
        env = dict(IE_PRECISION=prec, **({} if forced is None else {"IE_FORCE_TILE": str(forced)}))
        (st,) = [s for s in plan_of(path, N, env)["steps"] if s["kind"] == "layer_norm"]
        assert st["rms"] is True and st["bias_off"] == -1
        f16 = prec == "fp16"
        if forced is None:
            assert st["tile"] == CG.ln_default_tile(d, f16)
        elif st["tile"] != forced:
            assert st["tile"] == 0 and not CG.ln_tile_fits(d, f16, forced)      # not eligible: the generic kernel, which forced tile 0 runs
            continue
        y, kern = run_model(path, name, env, {"x": x}, "y", (N, d, 1, l), by_step=True)
        (label,) = [k for s, k in kern if s.endswith(step)]
        assert label == LG.rms_label(st["tile"], f16), (forced, st["tile"], label)
        assert np.isfinite(y).all()
        err = ref64.rel_err(y, ref)
        # the scaled row is max|ref| only through gamma; every row's result is O(1), so the bound holds per element on all of them
        print(f"rmsnorm L {l} D {d} {prec} forced {forced} tile {st['tile']}: max err / max|ref| {err:.3e}")
        assert err < RTOL[prec], (l, d, prec, st["tile"], err)
        assert np.array_equal(y[1, :, 0, 2], np.zeros(d, np.float32))
        ran.append(st["tile"])
    assert sorted(set(ran)) == sorted({0} | {t for t in (1, 2, 3, 4) if CG.ln_tile_fits(d, f16, t)}), ran
    return ran


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("l, d", SHAPES)
def test_rms_norm(tmp_path, l, d, prec):
    mb = LG.rms_graph(N, l, d)
    path = models.write_repo(str(tmp_path), "rms", mb)
    x = _input(l, d)
    ref = ref64.run_f64(mb, {"x": x})["y"]
    assert np.abs(ref[1, :, 0, 2]).max() == 0.0 and 0.5 < np.abs(ref[0, :, 0, 1]).max() < 10.0
    (st,) = [s for s in plan_of(path, N, dict(IE_PRECISION=prec))["steps"] if s["kind"] == "layer_norm"]
    assert st["in"]["buf"] == st["out"]["buf"]                # the last reader of its input: in place
    ran = _every_tile(path, "rms", prec, x, ref, d)
    if d == 50:
        assert set(ran) == {0}


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_not_the_last_reader(tmp_path, prec):
    """y = RMSNorm(x) + x: the norm's input lives on, so the norm writes another buffer (the residual stream of a decoder layer)"""
    l, d = 33, 256
    mb = LG.rms_graph(N, l, d, tail="add")
    path = models.write_repo(str(tmp_path), "rmsa", mb)
    x = _input(l, d)
    x[0, :, 0, 1] = np.random.RandomState(1).randn(d).astype(np.float32)      # (the sum with x would be the scaled row itself)
    ref = ref64.run_f64(mb, {"x": x})["y"]
    env = dict(IE_PRECISION=prec)
    (st,) = [s for s in plan_of(path, N, env)["steps"] if s["kind"] == "layer_norm"]
    assert st["in"]["buf"] != st["out"]["buf"]
    y, kern = run_model(path, "rmsa", env, {"x": x}, "y", (N, d, 1, l))
    assert LG.rms_label(st["tile"], prec == "fp16") in kern
    err = ref64.rel_err(y, ref)
    print(f"rmsnorm + x L {l} D {d} {prec}: max err / max|ref| {err:.3e}")
    assert err < RTOL[prec]


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_gated_unit(tmp_path, prec):
    """Llama's MLP, down(SiLU(gate(x)) * up(x)): the product runs as ONE eltwise step with the SiLU in front of it"""
    l, d, mlp = 33, 64, 96
    mb = LG.swiglu_graph(N, l, d, mlp)
    path = models.write_repo(str(tmp_path), "glu", mb)
    x = np.random.RandomState(5).randn(N, d, 1, l).astype(np.float32)
    ref = ref64.run_f64(mb, {"x": x})["y"]
    env = dict(IE_PRECISION=prec)
    steps = plan_of(path, N, env)["steps"]
    (glu,) = [s for s in steps if s["kind"] == "eltwise"]
    assert glu["mul"] is True and glu["pre_act"][0] == "silu"
    y, kern = run_model(path, "glu", env, {"x": x}, "y", (N, d, 1, l))
    assert kern.count("eltwise_kernel") == 1
    err = ref64.rel_err(y, ref)
    print(f"gated unit L {l} D {d} mlp {mlp} {prec}: max err / max|ref| {err:.3e}")
    assert err < RTOL[prec]
