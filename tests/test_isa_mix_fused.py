"""CPU: the vector-ALU overhead of conv_dense_fused_kernel, read off the compiler's listing (scripts/isa_mix.py; nothing runs on a GPU).

fp32 MFMAs and VALU instructions share the issue slot on this part, so the fused dense-layer kernel pays for its address
arithmetic, predicates and selects in matrix-pipe time.  Two properties are pinned for the build recipe's compiler flags:
  * no instantiation has a quarter-rate integer multiply or a v_rcp* after its entry block (nothing is divided or multiplied per slot, per
    chunk or per pixel block: the host passes reciprocals and slot counts, FusedConsts in csrc/kernels.h);
  * for <2,true,false,false> (fused tile 2 with the BN prologue, the kernel of DenseNet block 3) on the path of a block-3 layer the VALU count
    is at most HALF of what the kernel issued on the same path before.  The bound is the count of instructions the work itself needs, about
    350 of the parent's 900 (16 staged quads x (2 v_pk_fma + 4 v_max), tap zeroing, two reductions, the fresh-channel item, two epilogue quads,
    one add per load slot); it is not the achieved value.

The path: K = 512, Cin3 = 128, W = 14, prologue ReLU, no 3x3 bias or ReLU, 1x1 bias and ReLU, wave 4 (which publishes its partial 3x3 tile and
adds nothing).  The window is 62 rows of 32 columns: 16 rows per slot, three full slots and a partial fourth, four dead; the old channels are 120
columns: 4 rows per slot, 8 full slots, 8 dead; all nine 3x3 chunks are live and the slice (chunks 36 .. 44 of 72) changes tap after its fourth; the 1x1 is 32 chunks = four ring
trips (the ring-trip block counts four times) and no remainder chunk.  Dead slots are left out.  The kernel names the blocks of its slots and
variants with `; ie-mark` comments; the path is the cheapest way from the entry to s_endpgm through those of the live slots, in order, that
enters no other marked block.

PARENT_PATH_VALU was read off the listing of commit 402e7b4 (profiles/isa_r04/isa_mix_conv_dense_fused_kernel.txt, <2,true,false>):
    python scripts/isa_mix.py gpu-ai-inference-server_amd/csrc/kernels_fused.hip --kernel conv_dense_fused_kernelILi2ELb1ELb0E
as the blocks a wave runs at that shape: bb.0 .. bb.16 (entry, the window's offset chain and loads) 197 + bb.17 .. bb.48 (16 old-channel load
slots, the dead ones predicated, not skipped) 155 + bb.49 5 + .LBB8_50 4 + .LBB8_52 2 + .LBB8_145 4 + the four live window stores .LBB8_54 /
_65 / _66 / _67 16 + .LBB8_63 (setup) 138 + nine chunks bb.64 / .LBB8_72 / _117 .. _122 / _80 171 + .LBB8_81 4 + bb.82 3 + staging bb.86 1,
eight live slots bb.87 .. bb.101 112 and their connectors .LBB8_90 .. _98, _102 12 + .LBB8_111 1 + bb.112 (fresh channels) 26 + .LBB8_113 4 +
bb.114 8 + 4 x .LBB8_115 8 + bb.116 2 + epilogue .LBB8_138 2, bb.139 8, .LBB8_141 7, bb.142 8, .LBB8_144 4 = 902
(72 quarter-rate multiplies and 12 v_rcp after the entry block in the whole instantiation)."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import isa_mix  # noqa: E402

pytestmark = pytest.mark.skipif(not (os.path.exists(isa_mix.build_recipe().HIPCC) or shutil.which("hipcc")), reason="needs hipcc")
PARENT_PATH_VALU = 902
FUSED_INSTANCES = 8            # tiles 1 and 2, the two-workgroups-per-CU tile 3 and the N-split tile 6, with and without the prologue
RING_TRIPS = 4                 # K = 512: 32 chunks through a ring of 8


@pytest.fixture(scope="module")
def fused_kernels():
    k = isa_mix.analyze(os.path.join(ROOT, "gpu-ai-inference-server_amd", "csrc", "kernels_fused.hip"))
    return {isa_mix.template_args(s): b for s, b in k.items() if "conv_dense_fused_kernel" in s}


def test_no_slow_integer_ops_after_the_entry_block(fused_kernels):
    assert len(fused_kernels) == FUSED_INSTANCES, sorted(fused_kernels)
    for name, blocks in fused_kernels.items():
        bad = [(b["label"], b["qmul"], b["rcp"]) for b in blocks[1:] if b["qmul"] or b["rcp"]]
        print(f"conv_dense_fused_kernel{name}: entry block {blocks[0]['qmul']} quarter-rate multiplies, {blocks[0]['rcp']} v_rcp; after it {bad}")
        assert not bad, (name, bad)


def test_block3_path_valu_count_tile2_prologue(fused_kernels):
    blocks = fused_kernels["<2,true,false,false>"]
    marked = {}
    for i, b in enumerate(blocks):
        for m in b["marks"]:
            assert m not in marked, f"mark {m!r} names two blocks"
            marked[m] = i
    loop = max(range(len(blocks)), key=lambda i: blocks[i]["mfma"])
    assert blocks[loop]["mfma"] == 64 and blocks[loop]["label"] in blocks[loop]["targets"], blocks[loop]      # one ring trip: 8 chunks x 8 MFMAs, a self loop
    names = [f"fused-win-load u={u}" for u in range(3)] + ["fused-win-load-last u=3"] + [f"fused-old-load u={u}" for u in range(8)]
    names += [f"fused-win-put u={u}" for u in range(3)] + ["fused-win-put-last u=3"]
    names += [f"fused-chunk i={i}" for i in range(4)] + ["fused-tap-switch i=3"] + [f"fused-chunk i={i}" for i in range(4, 9)]      # wave 4: chunks 36 .. 44
    names += ["fused-stage relu=1"] + [f"fused-stage-put relu=1 u={u}" for u in range(8)] + ["fused-stage-end relu=1", "fused-fresh relu3=0 relu=1"]
    through = [marked[n] for n in names] + [loop, marked["fused-finish relu=1 bias=1"]]
    avoid = {i for i, b in enumerate(blocks) if i not in through and b["marks"]}
    once, path = isa_mix.path_cost(blocks, "valu", through, avoid)
    valu = once + (RING_TRIPS - 1) * blocks[loop]["valu"]
    print(f"conv_dense_fused_kernel<2,true,false,false> block-3 path: {valu} VALU (parent {PARENT_PATH_VALU}, bound {PARENT_PATH_VALU / 2:.0f}) over {' '.join(path)}")
    assert valu <= PARENT_PATH_VALU / 2, (valu, path)
