"""CPU: the vector-ALU overhead of conv1x1_as_kernel, read off the compiler's listing (scripts/isa_mix.py; nothing runs on a GPU).

fp32 MFMAs and VALU instructions do not overlap on this part, so what the staging loop, the setup and the epilogue issue on the
vector ALU is paid in matrix-pipe time.  Two properties are pinned for the build recipe's compiler flags:
  * no instantiation has a quarter-rate integer multiply or a v_rcp* after its entry block (no division or multiply per staged item);
  * for <8,1,2,true> (tile t10 with the BN prologue, the kernel of DenseNet blocks 1-2) on the single-pass path -- K = 128: one column block of 32
    columns, two row passes, prologue ReLU, bias and ReLU; entry, staging, barrier, setup, ONE ring trip, epilogue -- the VALU count is at most
    40 % of what the kernel issued on that path before the staging loop kept one column per thread.

PARENT_PATH_VALU was read off the listing of commit 82221fa:
    git show 82221fa:gpu-ai-inference-server_amd/csrc/kernels_direct.hip > kernels_direct.hip      (in a copy of csrc/)
    python scripts/isa_mix.py kernels_direct.hip --kernel conv1x1_as_kernelILi8ELi1ELi2ELb1
as the blocks a workgroup runs at K = 128 (items 0 and 1 of the four-item loop body live, bias and ReLU on, no remainder chunks):
    bb.0 4 + bb.1 10 + .LBB9_3 85 + .LBB9_6 40 + .LBB9_2 4 + .LBB9_9 8 + bb.10 8 + .LBB9_11 3 + .LBB9_22 3 + bb.23 2 + bb.25 8 + .LBB9_26 6
    + bb.27 2 + bb.29 8 + .LBB9_30 6 = 197   (14 quarter-rate multiplies in .LBB9_3, 6 in .LBB9_6, a v_rcp in bb.1).
The new kernel names the blocks of its variants with `; ie-mark` comments; the path is the cheapest way from the entry to s_endpgm through the
marked blocks of that case and the ring-trip loop (the block with the most MFMAs) that enters no other variant and no remainder-chunk block."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import isa_mix  # noqa: E402

pytestmark = pytest.mark.skipif(not (os.path.exists(isa_mix.build_recipe().HIPCC) or shutil.which("hipcc")), reason="needs hipcc")
PARENT_PATH_VALU = 197
AS_INSTANCES = 10              # five tiles, with and without the prologue


@pytest.fixture(scope="module")
def as_kernels():
    k = isa_mix.analyze(os.path.join(ROOT, "gpu-ai-inference-server_amd", "csrc", "kernels_direct.hip"))
    return {isa_mix.template_args(s): b for s, b in k.items() if "conv1x1_as_kernel" in s}


def test_no_slow_integer_ops_after_the_entry_block(as_kernels):
    assert len(as_kernels) == AS_INSTANCES, sorted(as_kernels)
    for name, blocks in as_kernels.items():
        bad = [(b["label"], b["qmul"], b["rcp"]) for b in blocks[1:] if b["qmul"] or b["rcp"]]
        print(f"conv1x1_as_kernel{name}: entry block {blocks[0]['qmul']} quarter-rate multiplies, {blocks[0]['rcp']} v_rcp; after it {bad}")
        assert not bad, (name, bad)


def test_single_pass_valu_count_t10_prologue(as_kernels):
    blocks = as_kernels["<8,1,2,true>"]
    marked = {m: i for i, b in enumerate(blocks) for m in b["marks"]}
    loop = max(range(len(blocks)), key=lambda i: blocks[i]["mfma"])
    assert blocks[loop]["mfma"] == 64 and blocks[loop]["label"] in blocks[loop]["targets"], blocks[loop]      # one ring trip: 8 chunks x 8 MFMAs, a self loop
    through = [marked["as-stage n=2 relu=1"], marked["as-stage-end n=2 relu=1"], loop, marked["as-finish relu=1 bias=1"]]
    avoid = {i for i, b in enumerate(blocks) if i not in through and (b["marks"] or b["mfma"])}
    valu, path = isa_mix.path_cost(blocks, "valu", through, avoid)
    print(f"conv1x1_as_kernel<8,1,2,true> single-pass path: {valu} VALU (parent {PARENT_PATH_VALU}, bound {0.4 * PARENT_PATH_VALU:.1f}) over {' '.join(path)}")
    assert valu <= 0.4 * PARENT_PATH_VALU, (valu, path)
