"""GPU (-m gpu): conv1x1_pooled_kernel (csrc/kernels_trans.hip) -- a transition's average pool folded into the staging loop of the 1x1 conv behind
it, optionally with the next block's entry 1x1 chained on the stored tile -- per element and bit for bit against the split launches.

Single transitions (tests/transition_graphs.py: BN -> ReLU -> Conv 1x1 -> AveragePool 2x2 / s2, swapped by the planner), forced with
IE_POOL_CONV=1:<tile> on every tile (0-4 conv1x1_as_kernel's shapes, 5 the 16-channel tile, 6-7 the chain shapes on 16-pixel blocks); Profile() must name the kernel for both steps.  The shapes are chosen for the row -> window mapping:

    N x H x W    out    M    K     what it exercises
    1 x 2 x 2    1 x 1   1    48   fewer pixels than a block; 12 columns
    2 x 6 x 10   3 x 5  30   144   odd output width: a 16-pixel block spans several output rows and both images; ragged last block
    2 x 10 x 14  5 x 7  70   272   68 columns: a partial last column block behind full ones
    3 x 4 x 6    2 x 3  18  1008   63 chunks: not a multiple of either ring depth
    2 x 6 x 10   3 x 5  30    64   no BN and no ReLU in front (pool without prologue)

Every shape runs with BN only and with BN + ReLU, with and without a conv bias, with Cout = the tile's channel count and twice it (two channel
blocks stage the same rows).  Two checks per run:
  * per element against the float64 oracle of the graph as written (oracle/onnx_oracle.py).  Bound = the two derived bounds the suite already
    uses, added: test_kernel_maps_gpu.check_conv's 2 * c_emul * u * S with S = |pooled float64 activations| . |w| (+ |bias|), c_emul the largest
    c of the legal fp32 summation orders on this case's own data; plus test_pool_maps' k * k * u * mean|window| per pooled activation, carried
    through sum |w|.
  * np.array_equal against the same graph with IE_POOL_CONV=0 and the conv forced to conv1x1_as_kernel: the staged rows are bit-equal to the pooled
    tensor and the loop behind them is the as-kernel's, so any difference is a bug.

Chain: mini DenseNets whose transition goes 256 -> 128 (stem 192) and 512 -> 256 (stem 448) on 4 x 4 maps (M = 48), the entry conv reading a slice
of the wider concat buffer; IE_POOL_CONV=2:<chain tile> (0 / 6 hold 128 channels, 2 / 7 hold 256).  Logits within test_gpu_parity.RTOL (2e-4 of max|ref|) of the float64 oracle and
np.array_equal to the IE_POOL_CONV=0 run with the same kernels elsewhere.  A 352 -> 176 transition fits no chain tile: the pair runs without the
chain.  With nothing set the load-time search decides; Profile() keeps one entry per plan step."""
import functools

import numpy as np
import pytest

import kernel_ref as R
import test_kernel_maps_gpu as KM
import transition_graphs as T
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models
from oracle import onnx_oracle as O

pytestmark = pytest.mark.gpu
RTOL = 2e-4          # of max|ref|: test_gpu_parity.RTOL

TILE_COUT = {0: 128, 1: 64, 2: 256, 3: 64, 4: 64, 5: 16, 6: 128, 7: 256}         # channels per workgroup of each conv1x1_pooled_kernel tile
AS_TWIN = {0: 10, 1: 11, 2: 12, 3: 13, 4: 14, 5: 13, 6: 10, 7: 12}       # conv1x1_as_kernel's tile of the same shape (tiles 5-7: of the same channel count; every as tile sums alike)
SHAPES = {"m1": (1, 2, 2, 48), "m30": (2, 6, 10, 144), "m70": (2, 10, 14, 272), "m18": (3, 4, 6, 1008)}
# (bn, relu, bias, Cout multiplier): each shape with BN only and BN + ReLU, with and without a bias, one and two channel blocks
VARIANTS = [(True, False, False, 1), (True, True, True, 1), (True, False, True, 2), (True, True, False, 2)]
NO_BN = (2, 6, 10, 64)


@functools.lru_cache(maxsize=None)
def reference(seed, shape, bn, relu, bias, cout):
    """(case, ref64 of the graph as written, bound) -- computed once per case and shared by the tiles that use the same Cout."""
    n, h, w, k = shape
    d = T.transition_case(seed, n, h, w, k, cout, bn=bn, relu=relu, bias=bias)
    ref = O.run(O.load_model(d["model"]), {"x": d["x"]}, dtype=np.float64)["out"]
    cols32, cols64, mabs64 = T.pooled_operands(d)
    wm, b = R.wmat(d["wt"]), d.get("bvec")
    ref_p, S = R.ref64_S(cols64, wm, b, False)
    assert np.allclose(T.two_copies(ref_p, d), ref, rtol=1e-9, atol=1e-12)       # pool and 1x1 conv commute: the oracle's graph and the pooled form agree
    ce, _ = R.c_emul(cols32, wm, b, False, seed=seed)
    pool_term = (4 * R.U * mabs64) @ np.abs(wm.astype(np.float64)).T
    bound = T.two_copies(R.MARGIN * ce * R.U * S + pool_term, d)
    return d, ref, bound, ce


def run_case(tmp_path, d, env):
    steps, ys, prof = KM.run_graph(tmp_path, d, env, "fp32")
    return steps, ys[0], prof


def check(tmp_path, tile, seed, shape, bn, relu, bias, mult):
    cout = TILE_COUT[tile] * mult
    if tile == 5:
        cout = 48 if mult == 1 else 128                    # 48: a channel count only the 16-channel tile takes (no as-kernel run to compare with)
    d, ref, bound, ce = reference(seed, shape, bn, relu, bias, cout)
    forced = dict(IE_FORCE_ALGO="direct", IE_FORCE_TILE=str(AS_TWIN[tile]))
    steps, y, prof = run_case(tmp_path, d, dict(forced, IE_POOL_CONV=f"1:{tile}"))
    names = [s["name"] for s in steps if s["kind"] == "pool" or s["name"] == "conv"]
    assert len(names) == 2, [s["name"] for s in steps]
    label = f"conv1x1_pooled_kernel<f32,t{tile}>"
    assert [prof[nm] for nm in names] == [label, label], prof
    err = np.abs(y.astype(np.float64) - ref)
    used = float((err / np.maximum(bound, 1e-300)).max())
    at = tuple(int(v) for v in np.unravel_index(int(np.argmax(err / np.maximum(bound, 1e-300))), err.shape))
    print(f"pooled t{tile} {shape} bn={bn} relu={relu} bias={bias} Cout={cout}: c_emul {ce:.2f}, largest |err| / bound {used:.3f} at {at}")
    assert np.all(err <= bound), (tile, shape, bn, relu, bias, cout, at, y[at], ref[at], used)
    if cout % 64 == 0:                                     # (conv1x1_as_kernel takes multiples of 64 channels)
        _, y0, prof0 = run_case(tmp_path, d, dict(forced, IE_POOL_CONV="0"))
        assert prof0[names[0]] == "pool_kernel" and prof0[names[1]] == f"conv1x1_as_kernel<f32,t{AS_TWIN[tile]}>", prof0
        np.testing.assert_array_equal(y, y0)


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("tile", range(8))
def test_pooled_staging_maps(tmp_path, tile, shape):
    for i, (bn, relu, bias, mult) in enumerate(VARIANTS):
        check(tmp_path, tile, 700 + 10 * sorted(SHAPES).index(shape) + i, SHAPES[shape], bn, relu, bias, mult)


@pytest.mark.parametrize("tile", range(8))
def test_pool_without_prologue(tmp_path, tile):
    check(tmp_path, tile, 760, NO_BN, False, False, False, 1)
    check(tmp_path, tile, 761, NO_BN, False, False, True, 2)


def test_forced_tile_that_does_not_fit_runs_split(tmp_path):
    """IE_POOL_CONV=1:2 (256 channels per workgroup) on a 64-channel conv: the launcher declines, the two plain launches run."""
    d, ref, bound, _ = reference(770, SHAPES["m30"], True, True, True, 64)
    steps, y, prof = run_case(tmp_path, d, dict(IE_FORCE_ALGO="direct", IE_FORCE_TILE="13", IE_POOL_CONV="1:2"))
    names = [s["name"] for s in steps if s["kind"] == "pool" or s["name"] == "conv"]
    assert [prof[nm] for nm in names] == ["pool_kernel", "conv1x1_as_kernel<f32,t13>"], prof
    assert np.all(np.abs(y.astype(np.float64) - ref) <= bound)


# ---------------------------------------------------------------------------------------------------------------------
# the chain, on mini DenseNets
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mini(stem, blocks):
    mb = models.densenet(3, growth=32, blocks=blocks, stem=stem, image=32, classes=12)
    x = models.synthetic_input((3, 3, 32, 32), stream="trans")
    ref = O.run(O.load_model(mb), {"data_0": x}, dtype=np.float64)["fc6_1"]
    return mb, x, ref


def run_mini(tmp_path, stem, blocks, env):
    mb, x, ref = mini(stem, blocks)
    path = models.write_repo(str(tmp_path), "trnet", mb)

    def go():
        d = B.DescribeModel(path, 3)
        m = B.CreateModel(path, "trnet")
        try:
            r = m.Infer([B.TensorData("data_0", B.DataTypeFloat32, B.Shape([3, 3, 32, 32]), x)], [B.OutputConfig("fc6_1", Shape=[3, 12, 1, 1], DataType="FLOAT32")])
            y = r[0].Data.reshape(ref.shape).copy()
            prof = B.Profile(m, 1)
        finally:
            m.Destroy()
        return d, y, prof
    d, y, prof = KM.with_env(env, go)
    err = float(np.abs(y.astype(np.float64) - ref).max() / np.abs(ref).max())
    return d, y, prof, err


def transition_of(d):
    (e,) = [e for e in d["paired_launches"] if e["kind"] is not None]
    return e


@pytest.mark.parametrize("stem,tile", [(192, 0), (448, 2), (192, 6), (448, 7)])
def test_chain_on_mini_densenet(tmp_path, stem, tile):
    kernels = dict(IE_FORCE_ALGO="direct", IE_FORCE_TILE="10")      # the same kernels in every run; the 1x1 convs on conv1x1_as_kernel (the chain's summation order)
    d, y, prof, err = run_mini(tmp_path, stem, (2, 2), dict(kernels, IE_POOL_CONV=f"2:{tile}"))
    e = transition_of(d)
    steps = d["plan"]["steps"]
    assert e["kind"] == "pool_conv_chain" and tile in e["chain_tiles"], e
    entry = steps[e["steps"][2]]
    assert entry["in"]["pitch"] > entry["in"]["c"] and entry["out"]["n"] * entry["out"]["h"] * entry["out"]["w"] == 48, entry
    assert len(prof) == len(steps) and [p["name"] for p in prof] == [s["name"] for s in steps] and all(p["ms"] > 0 for p in prof)
    label = f"conv1x1_pooled_kernel<f32,t{tile},chain>"
    assert [prof[i]["kernel"] for i in e["steps"]] == [label] * 3, [prof[i]["kernel"] for i in e["steps"]]
    print(f"chain t{tile} stem {stem}: {steps[e['steps'][1]]['in']['c']} -> {steps[e['steps'][1]]['out']['c']} -> 128, rel err {err:.2e}")
    assert err < RTOL, err
    d0, y0, prof0, _ = run_mini(tmp_path, stem, (2, 2), dict(kernels, IE_POOL_CONV="0"))
    assert [prof0[i]["kernel"] for i in e["steps"]] == ["pool_kernel", "conv1x1_as_kernel<f32,t10>", "conv1x1_as_kernel<f32,t10>"], [prof0[i]["kernel"] for i in e["steps"]]
    assert [p["kernel"] for j, p in enumerate(prof0) if j not in e["steps"]] == [p["kernel"] for j, p in enumerate(prof) if j not in e["steps"]]
    np.testing.assert_array_equal(y, y0)
    # pool + conv without the chain on the same graph: bit-equal too
    d1, y1, prof1, _ = run_mini(tmp_path, stem, (2, 2), dict(kernels, IE_POOL_CONV=f"1:{tile}"))
    assert [prof1[i]["kernel"] for i in e["steps"][:2]] == [f"conv1x1_pooled_kernel<f32,t{tile}>"] * 2 and "pooled" not in prof1[e["steps"][2]]["kernel"]
    np.testing.assert_array_equal(y1, y0)


def test_transition_that_fits_no_chain_tile(tmp_path):
    d, y, prof, err = run_mini(tmp_path, 256, (3, 3), dict(IE_AUTOTUNE="0", IE_POOL_CONV="2"))
    e = transition_of(d)
    conv = d["plan"]["steps"][e["steps"][1]]
    assert (conv["in"]["c"], conv["out"]["c"]) == (352, 176) and e["kind"] == "pool_conv" and e["chain_tiles"] == [], e
    ks = [prof[i]["kernel"] for i in e["steps"]]
    print(f"352 -> 176: {ks}, rel err {err:.2e}")
    assert ks == ["conv1x1_pooled_kernel<f32,t5>"] * 2, ks
    assert err < RTOL, err


def test_searched_choice(tmp_path):
    d, y, prof, err = run_mini(tmp_path, 192, (2, 2), dict(IE_TUNE_CACHE="0"))
    steps = d["plan"]["steps"]
    e = transition_of(d)
    print(f"searched: {[prof[i]['kernel'] for i in e['steps']]}, rel err {err:.2e}")
    assert len(prof) == len(steps) and [p["name"] for p in prof] == [s["name"] for s in steps]
    assert all(p["ms"] > 0 for p in prof), [(p["name"], p["ms"]) for p in prof]
    assert err < RTOL, err
