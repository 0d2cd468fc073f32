"""CPU: the vector-ALU side of conv1x1_pooled_kernel, read off the compiler's listing (scripts/isa_mix.py; nothing runs on a GPU).

The staging loop maps every LDS row to its 2x2 input window: m -> (b, oy, ox) with host-passed reciprocals and 24-bit multiplies.  Pinned for the
build recipe's flags, for every instantiation (eight tiles with and without the pool's prologue, the four chain tiles again with the chain):
  * no quarter-rate integer multiply and no v_rcp* after the entry block (no division by a runtime divisor per staged row);
  * the compiler's resource report shows no scratch: no private segment, no spilled register.
The VALU count of the staging blocks (named with `; ie-mark pooled-stage ...`) is printed per instantiation."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import isa_mix  # noqa: E402

pytestmark = pytest.mark.skipif(not (os.path.exists(isa_mix.build_recipe().HIPCC) or shutil.which("hipcc")), reason="needs hipcc")
INSTANCES = 8 * 2 + 4 * 2


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("isa") / "kernels_trans.s")
    isa_mix.compile_listing(os.path.join(ROOT, "gpu-ai-inference-server_amd", "csrc", "kernels_trans.hip"), out)
    return open(out).read()


@pytest.fixture(scope="module")
def kernels(listing):
    k = {isa_mix.template_args(s): b for s, b in isa_mix.parse(listing).items() if "conv1x1_pooled_kernel" in s}
    assert len(k) == INSTANCES, sorted(k)
    return k


def test_no_slow_integer_ops_after_the_entry_block(kernels):
    for name, blocks in kernels.items():
        bad = [(b["label"], b["qmul"], b["rcp"]) for b in blocks[1:] if b["qmul"] or b["rcp"]]
        print(f"conv1x1_pooled_kernel{name}: entry block {blocks[0]['qmul']} quarter-rate multiplies, {blocks[0]['rcp']} v_rcp; after it {bad}")
        assert not bad, (name, bad)
        assert blocks[0]["rcp"] == 0, name                # the reciprocals come from the host


def test_staging_blocks_valu(kernels):
    for name, blocks in kernels.items():
        rows = {}
        open_mark = None
        for b in blocks:
            for m in b["marks"]:
                if m.startswith("pooled-stage-end"):
                    open_mark = None
                elif m.startswith("pooled-stage"):
                    open_mark = m
            stage = [m for m in b["marks"] if m.startswith("pooled-stage") and not m.startswith("pooled-stage-end")]
            for m in stage or ([open_mark] if open_mark else []):
                rows[m] = rows.get(m, 0) + b["valu"]
        print(f"conv1x1_pooled_kernel{name}: VALU per staging group " + ", ".join(f"[{m}] {v}" for m, v in sorted(rows.items())))
        assert rows, name                                  # the marks are there
        assert all(b["mfma"] == 0 for b in blocks if any(m.startswith("pooled-stage") for m in b["marks"])), name


def test_no_scratch(listing):
    seen = 0
    for meta in re.findall(r"  - \.agpr_count:.*?\.wavefront_size:\s+\d+", listing, re.S):
        name = re.search(r"\.name:\s+(\S+)", meta).group(1)
        if "conv1x1_pooled_kernel" not in name:
            continue
        seen += 1
        priv = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1))
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", meta).group(1))
        sspill = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", meta).group(1))
        vg = int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1))
        print(f"{isa_mix.template_args(name)}: {vg} VGPRs, private segment {priv} B, spills v{spill} s{sspill}")
        assert priv == 0 and spill == 0 and sspill == 0, name
    assert seen == INSTANCES
    assert not re.search(r"conv1x1_pooled_kernel\S*\.uses_flat_scratch,\s*1", listing)
