"""GPU (-m gpu): the N-split tile of the fused dense-layer kernel (fused tile 6, csrc/kernels_fused.hip): 16-pixel tiles on a two-row grid, row h
recomputes the 3x3 and owns output channels [64h, 64h + 64) of the 1x1; waves 0-3 walk all K chunks in tile 1's order on one accumulator behind a
16-deep weight ring, waves 4-7 leave after the last barrier.

Cases: every DENSE32 case of test_kernel_maps_gpu plus
  * 1 x 3 x 3: M = 9, less than one tile -- every row past M reads and stores behind the buffer ranges;
  * 5 x 7 x 7 from 496 channels, two layers: K = 528 / 560 = 33 / 35 chunks, neither a multiple of the ring depth (16);
  * a block input of 16 channels, the smallest that keeps K >= 48 (K must be a multiple of 16): K = 48 / 80, the ring is never full;
  * 13 x 14 x 14: M = 2548, ragged tiles across images on the two-row grid.
Each stage is held to its own per-element bound by test_kernel_maps_gpu.stage_check.  The order-preserving form sums exactly as tile 1 does, so
every exposed output of the tile-6 run equals the tile-1 run's bit for bit.  The mini DenseNet of test_as_staging_gpu runs whole on tile 6."""
import functools
import tempfile

import numpy as np
import pytest

import kernel_graphs as G
import test_as_staging_gpu as AS
import test_kernel_maps_gpu as KM

pytestmark = pytest.mark.gpu
WANT = "conv_dense_fused_kernel<t6>"
CASES = KM.DENSE32 + [(65, 1, 3, 3, 64, 2), (66, 5, 7, 7, 496, 2), (67, 2, 5, 7, 16, 2), (68, 13, 14, 14, 64, 1)]
IDS = [f"d{d[0]}" for d in CASES]


@functools.lru_cache(maxsize=None)
def fused_run(dense, tile):
    """One run of a case on a forced fused tile, shared by the tests: (graph, plan steps, outputs, Profile() records)."""
    seed, n, h, w, c0, layers = dense
    d = G.dense_case(seed, n, h, w, c0, layers, tail=True, expose=True)
    with tempfile.TemporaryDirectory() as tmp:
        steps, out, prof = KM.run_outputs(tmp, d, dict(IE_AUTOTUNE="0", IE_FUSE_PB=str(tile)), "fp32")
    return d, steps, out, prof


@pytest.mark.parametrize("dense", CASES, ids=IDS)
def test_nsplit_stages(dense):
    seed, n, h, w, c0, layers = dense
    d, steps, out, prof = fused_run(dense, 6)
    assert [p["name"] for p in prof] == [s["name"] for s in steps]
    fused = [(s, p["kernel"]) for s, p in zip(steps, prof) if s.get("algo") == "dense_fused"]
    assert len(fused) == layers and all(s["tile"] == 6 and k == WANT for s, k in fused), [(s["name"], s["tile"], k) for s, k in fused]
    cat = out["cat"]
    for l in range(1, layers + 1):
        lo = c0 + 32 * (l - 1)
        KM.stage_check(f"fused {WANT} d{seed} layer {l} 3x3", cat[:, lo:lo + 32], out[f"b{l}"], d["layers"][l - 1]["w3"], None, 3, False, seed=seed)
        pre, (w1, b1) = KM.folded_1x1(d["layers"][l])
        KM.stage_check(f"fused {WANT} d{seed} layer {l + 1} 1x1", out["bott" if l == layers else f"b{l + 1}"], cat[:, :lo + 32], w1, b1, 1, True, pre=pre, seed=seed)
    np.testing.assert_array_equal(cat[:, :c0], G.lifted(d["x"], d["w0"]))


@pytest.mark.parametrize("dense", CASES, ids=IDS)
def test_nsplit_is_bitwise_tile1(dense):
    _, steps6, out6, _ = fused_run(dense, 6)
    _, steps1, out1, prof1 = fused_run(dense, 1)
    assert all(s["tile"] == 1 for s in steps1 if s.get("algo") == "dense_fused") and any(p["kernel"] == "conv_dense_fused_kernel<t1>" for p in prof1)
    assert sorted(out6) == sorted(out1)
    for name in out6:
        diff = int((out6[name] != out1[name]).sum())
        print(f"d{dense[0]} {name}: {diff} of {out6[name].size} elements differ between tile 6 and tile 1")
        assert np.array_equal(out6[name], out1[name]), (dense, name, diff)


def test_mini_densenet_on_nsplit_tiles(tmp_path):
    steps, prof, err = AS.run_mini(tmp_path, dict(IE_AUTOTUNE="0", IE_FUSE_PB="6"))
    n = sum(p["kernel"] == WANT for p in prof)
    print(f"mini DenseNet fused t6: {n} launches of {WANT}; rel err {err:.2e}")
    assert n >= 2, [(s["name"], p["kernel"]) for s, p in zip(steps, prof)]
    assert err < AS.RTOL, err


def test_nsplit_two_inferences_bit_equal(tmp_path):
    from gpu_ai_inference_server_amd import binding as B
    from gpu_ai_inference_server_amd.modelgen import models
    mb, x, _ = AS.mini_densenet()
    path = models.write_repo(str(tmp_path), "asnet", mb)

    def go():
        m = B.CreateModel(path, "asnet")
        try:
            ys = [m.Infer([B.TensorData("data_0", B.DataTypeFloat32, B.Shape([3, 3, 56, 56]), x)], [B.OutputConfig("fc6_1", Shape=[3, 24, 1, 1], DataType="FLOAT32")])[0].Data.copy()
                  for _ in range(2)]
            prof = B.Profile(m, 1)
        finally:
            m.Destroy()
        return ys, prof
    ys, prof = KM.with_env(dict(IE_AUTOTUNE="0", IE_FUSE_PB="6"), go)
    assert sum(p["kernel"] == WANT for p in prof) >= 2
    assert np.array_equal(ys[0], ys[1])
