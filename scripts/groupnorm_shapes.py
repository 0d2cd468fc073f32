#!/usr/bin/env python3
"""The group-norm step alone at given shapes, on both tiles and in both precisions, next to torch's F.group_norm on channels_last tensors.

    python scripts/groupnorm_shapes.py [N,C,H,W,G ...]      default: the VAE decoder's maps (base 128, latent 32) at batch 8 (fp32) / 32 (fp16)

The graph is x -> Conv1x1 -> group norm -> SiLU -> Conv1x1 -> y (tests/gn_graphs.py gn_alias_graph: the norm reads and writes activation buffers of
the plan's precision, in place); the figures are the group-norm step's own, from HIP events around its launches (median of 50 passes).  TB/s is
algorithmic: the tensor read once and written once, whatever the kernel re-reads, against the 6.29 TB/s copy rate.  torch runs in a
process of its own."""
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
import gn_graphs as G  # noqa: E402
from gpu_ai_inference_server_amd import binding as B  # noqa: E402
from gpu_ai_inference_server_amd.modelgen import models  # noqa: E402

TORCH_GN = """
import json, sys, torch
import torch.nn.functional as F
out = []
for n, c, h, w, g, half in json.loads(sys.argv[1]):
    dt = torch.float16 if half else torch.float32
    x = torch.randn(n, c, h, w, device="cuda", dtype=dt).contiguous(memory_format=torch.channels_last)
    ga, be = torch.randn(c, device="cuda", dtype=dt), torch.randn(c, device="cuda", dtype=dt)
    f = lambda: F.silu(F.group_norm(x, g, ga, be, 1e-6))
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

DECODER = [(32, 32, 512), (64, 64, 512), (128, 128, 512), (128, 128, 256), (256, 256, 256), (256, 256, 128)]      # (H, W, C) of the decoder's norms
if sys.argv[1:]:
    cases = [tuple(int(v) for v in a.split(",")) + (half,) for a in sys.argv[1:] for half in (0, 1)]
else:
    cases = [(8, c, h, w, 32, 0) for h, w, c in DECODER] + [(32, c, h, w, 32, 1) for h, w, c in DECODER]
os.environ["IE_AUTOTUNE"] = "0"
rows = []
with tempfile.TemporaryDirectory() as root:
    for n, c, h, w, g, half in cases:
        path = models.write_repo(root, f"g{n}_{c}_{h}_{w}_{g}", G.gn_alias_graph(n, c, h, w, g))
        x = np.random.RandomState(0).randn(n, c, h, w).astype(np.float32)
        for tile in (1, 0):
            os.environ.update(IE_PRECISION="fp16" if half else "fp32", IE_FORCE_TILE=str(tile))
            m = B.CreateModel(path, "gn")
            din, _ = B.Prepare(m, [[n, c, h, w]], 1)
            B.CopyToDevice(m, din[0], x)
            B.RunPrepared(m, 3, True)
            (p,) = [q for q in B.Profile(m, 50) if q["kernel"].startswith("groupnorm_")]
            rows.append((n, c, h, w, g, half, p["kernel"], p["ms"]))
            m.Destroy()
child = subprocess.run([sys.executable, "-c", TORCH_GN, json.dumps(cases)], capture_output=True, text=True, timeout=600)
tms = json.loads(child.stdout.strip().splitlines()[-1]) if child.returncode == 0 else None
if tms is None:
    print("# torch yardstick failed:", child.stderr.strip().splitlines()[-1:])
print(f"{'N,C,H,W,G':>20} {'prec':>5} {'kernel':68} {'us':>9} {'TB/s':>6} {'%6.29T':>7} {'torch gn+silu us':>16}")
for n, c, h, w, g, half, kern, ms in rows:
    t = tms[cases.index((n, c, h, w, g, half))] * 1e3 if tms else float("nan")
    tbs = 2.0 * n * c * h * w * (2 if half else 4) / ms / 1e9
    print(f"{f'{n},{c},{h},{w},{g}':>20} {'fp16' if half else 'fp32':>5} {kern:68} {ms * 1e3:9.1f} {tbs:6.2f} {tbs / 6.29 * 100:6.1f}% {t:16.1f}")
