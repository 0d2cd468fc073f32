"""Instruction mix of every kernel of one .hip file, per basic block:
    python scripts/isa_mix.py gpu-ai-inference-server_amd/csrc/kernels_direct.hip [--kernel conv1x1_as_kernel] [--json] [--totals] [--asm listing.s]

The file is compiled to an AMDGPU listing with build.py's flags (hipcc --offload-arch=gfx950 -mllvm -amdgpu-mfma-vgpr-form=1 -O3
--cuda-device-only -S); --asm reads an existing listing instead.  Nothing runs on a GPU.  Per kernel symbol and basic block (a block
starts at a `.LBB` label or at a `; %bb.N:` fall-through comment; block 0 is the entry block) it prints the counts of
    mfma   v_mfma* / v_smfmac*
    valu   every other v_* (qmul and rcp included)
    qmul   the quarter-rate integer multiplies among them: v_mul_lo_*, v_mul_hi_* (32-bit), v_mad_u64_u32, v_mad_i64_i32
    rcp    v_rcp*
    vld / vst   buffer_ / global_ / flat_ / scratch_ loads and stores (atomics count as stores)
    ds     ds_*
    wait   s_waitcnt*          bar   s_barrier
and the labels the block branches to (a target at or before the block is a loop), plus any `; ie-mark <text>` comment a kernel plants with
an empty asm statement to name the blocks of one of its variants.  Classification is by opcode prefix only: fp32 MFMAs and
VALU instructions do not overlap on this part, so `valu` beside `mfma` is what a block pays on top of its matrix work."""
import argparse
import importlib.util
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("mfma", "valu", "qmul", "rcp", "vld", "vst", "ds", "wait", "bar")
QMUL = ("v_mul_lo_u32", "v_mul_lo_i32", "v_mul_hi_u32", "v_mul_hi_i32", "v_mad_u64_u32", "v_mad_i64_i32")
VMEM = ("buffer_", "global_", "flat_", "scratch_")


def build_recipe():
    spec = importlib.util.spec_from_file_location("ie_build_recipe", os.path.join(ROOT, "gpu-ai-inference-server_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compile_listing(src, out):
    b = build_recipe()
    flags = [f for f in b.COMMON if f not in ("-fPIC", "-Wall", "-Wextra")]
    cmd = [b.HIPCC, "--offload-arch=" + b.ARCH, "-mllvm", "-amdgpu-mfma-vgpr-form=1", *flags, "-w", "--cuda-device-only", "-S", src, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed:\n" + r.stdout + r.stderr)
    return out


def template_args(sym):
    """'<8,1,2,true>' from the integer / bool template literals of a mangled name ('' when there are none or others)."""
    m = re.search(r"I((?:L[a-z]n?\d+E)+)E", sym)
    if not m:
        return ""
    out = []
    for ty, neg, val in re.findall(r"L([a-z])(n?)(\d+)E", m.group(1)):
        out.append(("true" if val == "1" else "false") if ty == "b" else ("-" if neg else "") + val)
    return "<" + ",".join(out) + ">"


def classify(op):
    if op.startswith(("v_mfma", "v_smfmac")):
        return ("mfma",)
    if op.startswith("v_"):
        return ("valu",) + (("qmul",) if op.startswith(QMUL) else ()) + (("rcp",) if op.startswith("v_rcp") else ())
    if op.startswith(VMEM):
        return ("vld",) if "_load" in op else ("vst",)
    if op.startswith("ds_"):
        return ("ds",)
    if op.startswith("s_waitcnt"):
        return ("wait",)
    if op.startswith("s_barrier"):
        return ("bar",)
    return ()


def parse(text):
    """{kernel symbol: [block, ...]}, block = {"label", counts..., "targets": [labels]} in listing order."""
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    out, cur, blocks = {}, None, None
    for line in text.splitlines():
        s = line.strip()
        m = re.match(r"^([A-Za-z_.$][\w.$]*):", line)
        if m and m.group(1) in kernels:
            cur, blocks = m.group(1), []
            out[cur] = blocks
            continue
        if cur is None:
            continue
        if s.startswith(".Lfunc_end") or s.startswith(".section") or s.startswith(".end_amdhsa_kernel"):
            cur = None
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", s) or re.match(r"^; %(bb\.\d+):", s)
        if m:
            blocks.append(dict({k: 0 for k in KEYS}, label=m.group(1), targets=[], marks=[], ends=False))
            continue
        if blocks and s.startswith("; ie-mark "):
            blocks[-1]["marks"].append(s[len("; ie-mark "):].strip())
        if not s or s[0] in ";." or not blocks:
            continue
        op = s.split()[0]
        b = blocks[-1]
        for k in classify(op):
            b[k] += 1
        if op.startswith(("s_cbranch", "s_branch")):
            b["targets"].append(s.split()[1].rstrip(","))
        if op.startswith(("s_branch", "s_endpgm")):
            b["ends"] = True                     # no fall-through into the next block
    return out


def analyze(src=None, asm=None):
    if asm is None:
        with tempfile.TemporaryDirectory() as tmp:
            asm = compile_listing(src, os.path.join(tmp, "listing.s"))
            return parse(open(asm).read())
    return parse(open(asm).read())


def successors(blocks):
    """[[index, ...]] per block: branch targets, then the fall-through block unless the block ends in s_branch / s_endpgm."""
    order = {b["label"]: i for i, b in enumerate(blocks)}
    return [[order[t] for t in b["targets"] if t in order] + ([i + 1] if not b["ends"] and i + 1 < len(blocks) else []) for i, b in enumerate(blocks)]


def back_edges(succ):
    """{(i, j)}: the edges that close a loop (j is on the depth-first stack when i is left through it)."""
    state, back = {}, set()

    def visit(i):
        state[i] = 1
        for j in succ[i]:
            if state.get(j) == 1:
                back.add((i, j))
            elif j not in state:
                visit(j)
        state[i] = 2
    visit(0)
    return back


def path_cost(blocks, key, through=(), avoid=(), pick=min):
    """(sum of `key`, [labels]) of the cheapest (pick=max: costliest) way from block 0 to an s_endpgm that runs every loop body once (no
    loop-closing edge), visits the block indices `through` in that order and none of `avoid`; None when there is no such way.  With the
    blocks of one variant pinned by `through` (ie-mark) the cheapest way is that variant's path without detours the control flow graph allows
    but the program never takes (a flag set in one branch and tested after the join)."""
    succ = successors(blocks)
    back = back_edges(succ)
    ends = {i for i, b in enumerate(blocks) if b["ends"] and not b["targets"]}

    def leg(src, dsts):
        memo = {}

        def best(i):                                           # costliest continuation from i to one of dsts, i included
            if i not in memo:
                memo[i] = None
                if i in dsts:
                    memo[i] = (blocks[i][key], [i])
                else:
                    tails = [t for t in (best(j) for j in succ[i] if (i, j) not in back and j not in avoid) if t]
                    if tails:
                        t = pick(tails, key=lambda t: t[0])
                        memo[i] = (blocks[i][key] + t[0], [i] + t[1])
            return memo[i]
        return best(src)
    total, path, at = 0, [], 0
    for stop in list(through) + [None]:
        r = leg(at, ends if stop is None else {stop})
        if r is None:
            return None
        total += r[0] - (blocks[at][key] if path else 0)
        path += r[1][1:] if path else r[1]
        at = path[-1]
    return total, [blocks[i]["label"] for i in path]


def totals(blocks):
    return {k: sum(b[k] for b in blocks) for k in KEYS}


def render(kernels, out=sys.stdout, totals_only=False):
    if totals_only:                                  # one line per kernel: a listing of every block of a kernel with hundreds of them is long
        out.write(f"  {'kernel (every block once)':48s}" + "".join(f"{k:>6s}" for k in KEYS) + "  blocks\n")
        for sym, blocks in kernels.items():
            t = totals(blocks)
            name = re.sub(r"^_ZN\d+[a-z]+\d+", "", sym).split("I", 1)[0] + template_args(sym)
            out.write(f"  {name:48s}" + "".join(f"{t[k]:6d}" for k in KEYS) + f"  {len(blocks):6d}\n")
        return
    for sym, blocks in kernels.items():
        out.write(f"{sym} {template_args(sym)}\n")
        out.write("  block        " + "".join(f"{k:>6s}" for k in KEYS) + "  -> targets\n")
        order = {b["label"]: i for i, b in enumerate(blocks)}
        for i, b in enumerate(blocks):
            tg = " ".join(t + ("^" if order.get(t, 1 << 30) <= i else "") for t in b["targets"])
            out.write(f"  {b['label']:12s} " + "".join(f"{b[k]:6d}" for k in KEYS) + (f"  -> {tg}" if tg else "") + "".join(f"  [{m}]" for m in b["marks"]) + "\n")
        t = totals(blocks)
        out.write("  total        " + "".join(f"{t[k]:6d}" for k in KEYS) + "   (every block once; ^ = backward branch)\n\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("src", help=".hip file to compile (ignored with --asm)")
    ap.add_argument("--asm", help="read this listing instead of compiling")
    ap.add_argument("--kernel", action="append", default=[], help="only symbols containing this text (repeatable)")
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--totals", action="store_true", help="one line of totals per kernel instead of the block tables")
    a = ap.parse_args()
    k = analyze(a.src, a.asm)
    if a.kernel:
        k = {s: b for s, b in k.items() if any(f in s for f in a.kernel)}
    if a.json:
        json.dump(k, sys.stdout)
    else:
        render(k, totals_only=a.totals)


if __name__ == "__main__":
    main()
