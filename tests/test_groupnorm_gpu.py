"""GPU (-m gpu): the group-norm kernels on the MI355X against the float64 restatement in tests/ref64.py, per element, with the project's bounds
(tests/test_gpu_parity.py): fp32 within 2e-4 of max|ref|, fp16 within 3e-3.  IE_AUTOTUNE=0 throughout.

Graph of the step cases: fp32 x [N, C, H, W] -> group norm [-> SiLU] -> y.  Every case runs on the planner's default tile and on every forced
tile the plan accepts (IE_FORCE_TILE 0 / 1), the Profile label must be the kernel the plan's tile names, and every output must be finite.
Data (gn_graphs.data; values exact in half precision, so that both precisions read the same numbers): randn; group-distinct (every (image, group)
its own mean in [-8, 8] and scale in [0.25, 4]); mean 100 and std 1.  SiLU on the first two.

Shapes (N, C, H, W, G):
  (2, 32, 1, 1, 32)      one element per group: variance 0, the output is beta
  (2, 32, 5, 7, 8)       an odd pixel count
  (1, 64, 9, 9, 32)      2 channels per group: an fp32 vector spans two groups, an fp16 vector four
  (2, 128, 16, 16, 32)   4 channels per group: an fp16 vector spans two groups
  (1, 512, 8, 8, 32)     16 channels per group: a group is several vectors
  (1, 16, 4, 4, 1)       G = 1
  (2, 16, 6, 6, 16)      G = C, also through InstanceNormalization directly (form c)
  (1, 20, 3, 3, 5)       C is no whole fp16 vector: in fp16 tile 0 only, a forced tile 1 falls back to it (in fp32 20 channels are five vectors)
  (1, 64, 37, 41, 32)    tile 1 cuts the image into 6 (fp32) / 3 (fp16) slabs, the last one ragged"""

import numpy as np
import pytest

import gn_graphs as G
import ref64
from engine_run import infer, plan_of, RTOL, run_model, with_env
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models
from oracle import onnx_oracle as O

pytestmark = pytest.mark.gpu
SHAPES = [(2, 32, 1, 1, 32), (2, 32, 5, 7, 8), (1, 64, 9, 9, 32), (2, 128, 16, 16, 32), (1, 512, 8, 8, 32), (1, 16, 4, 4, 1), (2, 16, 6, 6, 16), (1, 20, 3, 3, 5),
          (1, 64, 37, 41, 32)]


def _every_tile(path, name, prec, batch, xs, refs, oshape, act, what):
    """every input on the default tile and on each forced tile the plan accepts, each output finite and inside the bound; -> {tile: worst error}"""
    worst = {}
    for forced in (None, 0, 1):
        env = dict(IE_PRECISION=prec, **({} if forced is None else {"IE_FORCE_TILE": str(forced)}))
        st = G.gn_step(plan_of(path, batch, env))
        if forced is not None and st["tile"] != forced:
            assert st["tile"] == 0                      # not eligible: the generic kernel, which forced tile 0 runs
            continue
        ys, kern = run_model(path, name, env, [{"x": x} for x in xs], "y", oshape, by_step=True)
        kern = dict(kern)
        assert kern[st["name"]] == G.gn_label(st["tile"], st["out"]["f16"], act), (forced, st["tile"], kern[st["name"]])
        for k, (y, ref) in enumerate(zip(ys, refs)):
            assert np.isfinite(y).all()
            err = ref64.rel_err(y, ref)
            print(f"{what} {prec} act {act} input {k} forced {forced} tile {st['tile']}: max err / max|ref| {err:.3e}")
            worst[st["tile"]] = max(worst.get(st["tile"], 0.0), err)
            assert err < RTOL[prec], (what, prec, act, k, st["tile"], err)
    return worst


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_group_norm(tmp_path, shape, prec):
    n, c, h, w, g = shape
    f16 = prec == "fp16"
    for act in (None, "silu"):
        mb = G.gn_graph(n, c, h, w, g, act=act)
        path = models.write_repo(str(tmp_path), "gn_" + str(act), mb)
        xs = [G.data(kind, n, c, h, w, g) for kind in (("randn", "distinct", "mean100") if act is None else ("randn", "distinct"))]
        refs = [ref64.run_f64(mb, {"x": x})["y"] for x in xs]
        worst = _every_tile(path, "gn_" + str(act), prec, n, xs, refs, shape[:4], act, f"{shape}")
        assert sorted(worst) == ([0, 1] if G.gn_tile_fits(c, g, f16, act) else [0]), worst
        if act is None and h * w == 1:
            # one element per group: whatever the input, the reference is beta (and the bound above held the kernels to it)
            beta = O.load_model(mb).inits["gn_beta"].reshape(1, c, 1, 1).astype(np.float64)
            for ref in refs:
                np.testing.assert_allclose(ref, np.broadcast_to(beta, ref.shape), rtol=0, atol=1e-12)
    if shape == (1, 20, 3, 3, 5) and f16:
        assert G.gn_step(plan_of(path, n, dict(IE_PRECISION=prec, IE_FORCE_TILE="1")))["tile"] == 0


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_instance_norm_on_a_map(tmp_path, prec):
    """form c): InstanceNormalization directly on the map is G = C with its own scale / B"""
    n, c, h, w = 2, 16, 6, 6
    mb = G.gn_graph(n, c, h, w, c, form="instance")
    path = models.write_repo(str(tmp_path), "inst", mb)
    xs = [G.data("randn", n, c, h, w, c), G.data("distinct", n, c, h, w, c)]
    refs = [ref64.run_f64(mb, {"x": x})["y"] for x in xs]
    assert sorted(_every_tile(path, "inst", prec, n, xs, refs, (n, c, h, w), None, "instance norm")) == [0, 1]


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_in_place(tmp_path, prec):
    """the norm's input (a conv's result) dies at the norm: the step's output is the input's buffer, on both tiles"""
    n, c, h, w, g = 2, 32, 9, 11, 8
    mb = G.gn_alias_graph(n, c, h, w, g)
    path = models.write_repo(str(tmp_path), "gna", mb)
    st = G.gn_step(plan_of(path, n, dict(IE_PRECISION=prec)))
    assert st["in"]["buf"] == st["out"]["buf"] and (st["in"]["c_off"], st["in"]["pitch"]) == (st["out"]["c_off"], st["out"]["pitch"]) == (0, c)
    xs = [G.data("distinct", n, c, h, w, g, seed=4)]
    refs = [ref64.run_f64(mb, {"x": x})["y"] for x in xs]
    assert sorted(_every_tile(path, "gna", prec, n, xs, refs, (n, c, h, w), "silu", "in place")) == [0, 1]


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_rank3_flat_form(tmp_path, prec):
    n, c, h, w, g = 2, 32, 5, 7, 8
    mb = G.gn_rank3_graph(n, c, h, w, g)
    path = models.write_repo(str(tmp_path), "gn3", mb)
    xs = [G.data("distinct", n, c, h, w, g, seed=3)]
    refs = [ref64.run_f64(mb, {"x": x})["y"] for x in xs]
    assert sorted(_every_tile(path, "gn3", prec, n, xs, refs, (n, c, h, w), None, "rank 3")) == [0, 1]


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("tile", [0, 1])
def test_runs_and_graph_replay_are_bit_equal(tmp_path, tile, prec):
    """no atomics, fixed combine orders: two runs give the same bits, and the captured graph gives the eager run's"""
    n, c, h, w, g = 1, 64, 37, 41, 32
    path = models.write_repo(str(tmp_path), "gnb", G.gn_graph(n, c, h, w, g, act="silu"))
    x = G.data("distinct", n, c, h, w, g, seed=9)

    def go():
        assert G.gn_step(B.DescribeModel(path, n)["plan"])["tile"] == tile
        m = B.CreateModel(path, "gnb")
        try:
            y1 = infer(m, {"x": x}, "y", (n, c, h, w))
            y2 = infer(m, {"x": x}, "y", (n, c, h, w))
            np.testing.assert_array_equal(y1, y2)
            din, dout = B.Prepare(m, [[n, c, h, w]], 1)
            B.CopyToDevice(m, din[0], x)
            B.RunPrepared(m, 2, True)                                              # graph replay
            y = np.empty((n, c, h, w), np.float32)
            B.CopyToHost(m, y, dout[0])
            np.testing.assert_array_equal(y, y1)
        finally:
            m.Destroy()
    with_env(dict(IE_AUTOTUNE="0", IE_PRECISION=prec, IE_FORCE_TILE=str(tile)), go)


# ---- whole networks --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def decoders(tmp_path_factory):
    """the narrow decoder (base 32, latents 8 x 8, N = 2, samples 64 x 64) in both spellings with a symbolic batch, one input and the float64 outputs;
    computed once, read-only"""
    root = str(tmp_path_factory.mktemp("dec"))
    z = G.half_exact(np.random.RandomState(21).randn(2, 4, 8, 8))
    out = {"z": z}
    for form in ("instancenorm", "op18"):
        mb = G.narrow_decoder("N", gn_form=form)
        out[form] = (models.write_repo(root, "dec_" + form, mb), ref64.run_f64(mb, {"latent_sample": z})["sample"])
    return out


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("form", ["instancenorm", "op18"])
def test_vae_decoder_vs_float64(decoders, form, prec):
    path, ref = decoders[form]
    z = decoders["z"]
    y, kern = run_model(path, "dec_" + form, dict(IE_PRECISION=prec), {"latent_sample": z}, "sample", (2, 3, 64, 64), by_step=True)
    kern = dict(kern)
    assert np.isfinite(y).all()
    err = ref64.rel_err(y, ref)
    labels = list(kern.values())
    print(f"vae_decoder {form} {prec}: max err / max|ref| {err:.3e}; group-norm kernels {sorted(set(k for k in labels if k.startswith('groupnorm')))}")
    assert sum(k.startswith("groupnorm") for k in labels) == 30 and "attention_generic_kernel" in labels
    assert err < RTOL[prec], (form, prec, err)


def test_vae_decoder_symbolic_batch(decoders):
    """one model, ModelInfer at batch 2 and at batch 1: the norm's statistics are per image, so image 0 does not depend on the batch"""
    path, ref = decoders["instancenorm"]
    z = decoders["z"]

    def go():
        m = B.CreateModel(path, "dec_instancenorm")
        try:
            y2 = infer(m, {"latent_sample": z}, "sample", (2, 3, 64, 64))
            y1 = infer(m, {"latent_sample": z[:1]}, "sample", (1, 3, 64, 64))
            return y2, y1
        finally:
            m.Destroy()
    y2, y1 = with_env(dict(IE_AUTOTUNE="0", IE_PRECISION="fp32"), go)
    e2, e1 = ref64.rel_err(y2, ref), ref64.rel_err(y1, ref[:1])
    print(f"vae_decoder symbolic batch: batch 2 {e2:.3e}, batch 1 {e1:.3e}")
    assert e2 < RTOL["fp32"] and e1 < RTOL["fp32"]


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_resnet_gn_vs_float64(tmp_path, prec):
    """53 norms and 54 convs deep, ten logits of max|ref| 2.7.  fp32 holds the project's bound.  In fp16 the number format alone costs this depth about
    the bound: the float64 walk with every value and every weight stored as a half (ref64.run_f64(round_half=True), exact arithmetic) is 2.9e-3 from
    the float64 walk on this input and 1.8e-3 / 3.0e-3 on two other draws.  The engine measured 3.19e-3 on the MI355X with the group norms on the
    planner's tiles, 2.71e-3 with all of them on tile 0 and 3.28e-3 with all on tile 1 (IE_GN_TILE): every variant sits in the walk's
    own spread, so it is the depth and the format, not a kernel.  The fp16 bound here is therefore the larger of 3e-3 and twice that walk's own
    error on the same input (two draws of the same rounding noise differ by up to 2x, as the three inputs show); fp32 keeps 2e-4 (measured 2.1e-6)."""
    mb = models.resnet(2, norm="gn", gn_groups=8, width=16, image=64, classes=10)
    path = models.write_repo(str(tmp_path), "rgn", mb)
    x = G.half_exact(models.synthetic_input((2, 3, 64, 64), stream="rgn"))
    ref = ref64.run_f64(mb, {"data": x})["logits"]
    bound = RTOL[prec]
    if prec == "fp16":
        noise = ref64.rel_err(ref64.run_f64(mb, {"data": x}, round_half=True)["logits"], ref)
        bound = max(bound, 2.0 * noise)
        print(f"resnet gn fp16: the half-storage float64 walk is {noise:.3e} from float64; bound {bound:.3e}")
    for gn_tile in (None, "0", "1"):
        y, kern = run_model(path, "rgn", dict(IE_PRECISION=prec, **({} if gn_tile is None else {"IE_GN_TILE": gn_tile})), {"data": x}, "logits", (2, 10), by_step=True)
        kern = dict(kern)
        err = ref64.rel_err(y, ref)
        labels = [k for k in kern.values() if k.startswith("groupnorm")]
        print(f"resnet gn {prec} IE_GN_TILE {gn_tile}: max err / max|ref| {err:.3e}; {sum(k.startswith('groupnorm_stats') for k in labels)} of {len(labels)} norms on tile 1")
        assert np.isfinite(y).all() and len(labels) == 53
        if gn_tile == "0":
            assert all(k == "groupnorm_generic_kernel" for k in labels)
        assert err < bound, (prec, gn_tile, err, bound)
