#!/usr/bin/env python3
"""The window-attention step alone at the four Swin-T stage shapes, on both kernels and in both precisions, next to its bandwidth roofline and to
torch's F.scaled_dot_product_attention with a float attn_mask.

    python scripts/window_attention_shapes.py [N32 [N16]]        default: batch 32 in fp32, batch 128 in fp16

The graph is the window region without Linears between the NCHW graph input [N, 3 D, H, W] and output (tests/swin_graphs.py wattn_graph); the
figures are the step's own, from HIP events around its launch (median of 50 passes).  The step is bandwidth-bound (4 L hd = 6272 FLOP per 512 bytes
of fp32 traffic per token and head): its roofline is its bytes at the 3.6 TB/s layernorm_kernel sustains.  torch gets the operands
already partitioned, [N nW, heads, L, hd] each, and bias + mask as one float attn_mask [N nW, heads, L, L] (it moves more bytes than the step:
the mask per window and head); it runs in a process of its own."""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _pkg import load_package  # noqa: E402

load_package()
import numpy as np  # noqa: E402
import swin_graphs as G  # noqa: E402
from gpu_ai_inference_server_amd import binding as B  # noqa: E402
from gpu_ai_inference_server_amd.modelgen import models  # noqa: E402

TORCH_SDPA = """
import json, sys, torch
import torch.nn.functional as F
out = []
for prec, n, hw, heads, hd, L in json.loads(sys.argv[1]):
    dt = torch.float16 if prec == "fp16" else torch.float32
    b = n * (hw // 7) ** 2
    q, k, v = (torch.randn(b, heads, L, hd, device="cuda", dtype=dt) for _ in range(3))
    mask = torch.randn(b, heads, L, L, device="cuda", dtype=dt)
    f = lambda: F.scaled_dot_product_attention(q, k, v, attn_mask=mask)
    for _ in range(5):
        f()
    ts = []
    for _ in range(50):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    out.append(sorted(ts)[len(ts) // 2])
print(json.dumps(out))
"""

ROOF_TBS = 3.6
batches = {"fp32": int(sys.argv[1]) if len(sys.argv) > 1 else 32, "fp16": int(sys.argv[2]) if len(sys.argv) > 2 else 128}
STAGES = [(56, 3, 3), (28, 6, 3), (14, 12, 3), (7, 24, 0)]          # map extent, heads, shift (window 7, hd 32)
os.environ["IE_AUTOTUNE"] = "0"
rows, cases = [], []
with tempfile.TemporaryDirectory() as root:
    for prec in ("fp32", "fp16"):
        n = batches[prec]
        for hw, heads, shift in STAGES:
            path = models.write_repo(root, f"w{n}_{hw}", G.wattn_graph(n, hw, 7, shift, heads, 32))
            x = np.random.RandomState(0).randn(n, 3 * heads * 32, hw, hw).astype(np.float32)
            cases.append([prec, n, hw, heads, 32, 49])
            for tile in (1, 0):
                os.environ.update(IE_PRECISION=prec, IE_FORCE_TILE=str(tile))
                m = B.CreateModel(path, "wattn")
                din, _ = B.Prepare(m, [list(x.shape)], 1)
                B.CopyToDevice(m, din[0], x)
                B.RunPrepared(m, 3, True)
                (p,) = [q for q in B.Profile(m, 50 if tile else 5) if q["kernel"].startswith("window_attention_")]
                rows.append((len(cases) - 1, p["kernel"], p["ms"], p["flops"], p["bytes"]))
                m.Destroy()
child = subprocess.run([sys.executable, "-c", TORCH_SDPA, json.dumps(cases)], capture_output=True, text=True, timeout=600)
tms = json.loads(child.stdout.strip().splitlines()[-1]) if child.returncode == 0 else None
if tms is None:
    print("# torch yardstick failed:", child.stderr.strip().splitlines()[-1:])
print(f"{'prec N,HxW,heads':>22} {'kernel':38} {'us':>9} {'TB/s':>6} {'roof us':>8} {'%roof':>6} {'TF/s':>7} {'torch sdpa us':>13}")
for ci, kern, ms, flops, nbytes in rows:
    prec, n, hw, heads, _, _ = cases[ci]
    roof = nbytes / (ROOF_TBS * 1e9)
    t = tms[ci] * 1e3 if tms else float("nan")
    print(f"{f'{prec} {n},{hw}x{hw},{heads}':>22} {kern:38} {ms * 1e3:9.1f} {nbytes / ms / 1e9:6.2f} {roof * 1e3:8.1f} {roof / ms * 100:5.1f}% {flops / ms / 1e9:7.2f} {t:13.1f}")
