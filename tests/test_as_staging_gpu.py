"""GPU (-m gpu): conv1x1_as_kernel's staging loop -- one 4-channel column per thread, 16 / 32 / 64 columns per block, rows walked in passes
(csrc/kernels_direct.hip) -- and its predicate-free epilogue, per element on the map each tile writes.

The single-conv cases are chosen for the mapping: column counts K / 4 that are no power of two and below 64 (12, 36, 56: lanes of the only or
the last column block sit out), a partial last block behind full ones (K = 272: 68 columns), a long K that is no multiple of the ring depth
(1008), fewer pixels than one pixel block (1 x 3 x 3: every row past M reads and stores behind the buffer range), and a ragged last block
that straddles two images (2 x 5 x 7); prologue, bias and ReLU on and off.  Which of 16 / 32 / 64 columns a shape gets is the launcher's
choice (as_col_shift: fewest load groups, then fewest load slots): with 512 / 256 / 128 threads the five tiles take different ones for the
same K.  Bounds and runner are test_kernel_maps_gpu's: |y - ref64| <= 2 * c_emul * u * S per element, the kernel asserted through Profile().

The mini DenseNet's 1x1s read a channel slice of a wider concat buffer (row pitch != K); it runs on each forced tile and on the fused
dense-layer kernel (t1, t2), against the float64 oracle with the bound test_gpu_parity holds this graph to (2e-4 of max|ref|)."""
import functools

import numpy as np
import pytest

import test_kernel_maps_gpu as KM
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models
from oracle import onnx_oracle as O

pytestmark = pytest.mark.gpu
C = KM.C
RTOL = 2e-4          # of max|ref|: test_gpu_parity.RTOL, the bound the existing test holds this graph to


def staging_cases(tile):
    co = KM.AS_COUT[tile]
    return [C(501, 1, 3, 3, 48, co, pre=1, bias=1, post=1),             # M = 9 < 16; 12 columns
            C(502, 2, 5, 7, 144, co),                                   # M = 70: ragged, straddles two images; 36 columns; nothing fused
            C(503, 2, 5, 7, 224, 2 * co, pre=1, post=1),                # 56 columns; two channel blocks
            C(504, 2, 5, 7, 272, co, pre=1, bias=1),                    # 68 columns: a partial last block behind full ones
            C(505, 1, 3, 3, 1008, co, bias=1, post=1),                  # 63 chunks: not a multiple of the ring depth (8 / 16)
            C(506, 2, 5, 7, 1008, co, pre=1, bias=1, post=1)]


@pytest.mark.parametrize("tile", [10, 11, 12, 13, 14])
def test_staging_columns_and_ragged_rows(tmp_path, tile):
    for case in staging_cases(tile):
        KM.check_conv(tmp_path, case, dict(IE_FORCE_ALGO="direct", IE_FORCE_TILE=str(tile)), "fp32", f"as staging t{tile}", "direct", tile, runs=2)


@functools.lru_cache(maxsize=None)
def mini_densenet():
    mb = models.densenet(3, growth=32, blocks=(3, 3), stem=256, image=56, classes=24, seed=87)
    x = models.synthetic_input((3, 3, 56, 56), stream="as")
    ref = O.run(O.load_model(mb), {"data_0": x}, dtype=np.float64)["fc6_1"]
    return mb, x, ref


def run_mini(tmp_path, env):
    mb, x, ref = mini_densenet()
    path = models.write_repo(str(tmp_path), "asnet", mb)

    def go():
        steps = B.DescribeModel(path, 3)["plan"]["steps"]
        m = B.CreateModel(path, "asnet")
        try:
            r = m.Infer([B.TensorData("data_0", B.DataTypeFloat32, B.Shape([3, 3, 56, 56]), x)], [B.OutputConfig("fc6_1", Shape=[3, 24, 1, 1], DataType="FLOAT32")])
            y = r[0].Data.reshape(ref.shape).copy()
            prof = B.Profile(m, 1)
        finally:
            m.Destroy()
        return steps, y, prof
    steps, y, prof = KM.with_env(env, go)
    err = float(np.abs(y.astype(np.float64) - ref).max() / np.abs(ref).max())
    return steps, prof, err


@pytest.mark.parametrize("tile", [10, 11, 13, 14])           # t12 owns 256 output channels per workgroup: the bottlenecks have 128
def test_mini_densenet_sliced_rows(tmp_path, tile):
    steps, prof, err = run_mini(tmp_path, dict(IE_FORCE_ALGO="direct", IE_FORCE_TILE=str(tile)))
    want = f"conv1x1_as_kernel<f32,t{tile}>"
    sliced = [s for s, p in zip(steps, prof) if p["kernel"] == want and s["in"]["pitch"] != s["in"]["c"]]
    print(f"mini DenseNet t{tile}: {sum(p['kernel'] == want for p in prof)} launches of {want}, {len(sliced)} on a slice (pitch != K); rel err {err:.2e}")
    assert sliced, [(s["name"], p["kernel"]) for s, p in zip(steps, prof)]
    assert err < RTOL, (tile, err)


@pytest.mark.parametrize("tile", [1, 2])
def test_mini_densenet_fused_dense_layers(tmp_path, tile):
    steps, prof, err = run_mini(tmp_path, dict(IE_AUTOTUNE="0", IE_FUSE_PB=str(tile)))
    want = f"conv_dense_fused_kernel<t{tile}>"
    n = sum(p["kernel"] == want for p in prof)
    print(f"mini DenseNet fused t{tile}: {n} launches of {want}; rel err {err:.2e}")
    assert n >= 2, [(s["name"], p["kernel"]) for s, p in zip(steps, prof)]
    assert err < RTOL, (tile, err)
