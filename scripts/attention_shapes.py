#!/usr/bin/env python3
"""The attention step alone at given shapes, on both kernels and in both precisions, next to torch's F.scaled_dot_product_attention.

    python scripts/attention_shapes.py [N,H,L,hd ...]        default: 32,12,197,64 32,12,50,64 (ViT-B/16 and ViT-B/32 at batch 32)

The graph is the attention pattern between the NCHW graph input [N, 3 D, 1, L] and output (tests/vit_graphs.py attn_graph); the figures are the
attention step's own, from HIP events around its launch (median of 50 passes).  torch runs in a process of its own."""
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
import vit_graphs as G  # noqa: E402
from gpu_ai_inference_server_amd import binding as B  # noqa: E402
from gpu_ai_inference_server_amd.modelgen import models  # noqa: E402

TORCH_SDPA = """
import json, sys, torch
import torch.nn.functional as F
out = []
for n, h, l, hd in json.loads(sys.argv[1]):
    for dt in (torch.float32, torch.float16):
        q, k, v = (torch.randn(n, h, l, hd, device="cuda", dtype=dt) for _ in range(3))
        f = lambda: F.scaled_dot_product_attention(q, k, v)
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

shapes = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:]] or [(32, 12, 197, 64), (32, 12, 50, 64)]
os.environ["IE_AUTOTUNE"] = "0"
rows = []
with tempfile.TemporaryDirectory() as root:
    for n, h, l, hd in shapes:
        path = models.write_repo(root, f"a{n}_{h}_{l}_{hd}", G.attn_graph(n, l, h, hd))
        x = np.random.RandomState(0).randn(n, 3 * h * hd, 1, l).astype(np.float32)
        for prec in ("fp32", "fp16"):
            for tile in (1, 0):
                os.environ.update(IE_PRECISION=prec, IE_FORCE_TILE=str(tile))
                m = B.CreateModel(path, "attn")
                din, _ = B.Prepare(m, [[n, 3 * h * hd, 1, l]], 1)
                B.CopyToDevice(m, din[0], x)
                B.RunPrepared(m, 5, True)
                (p,) = [q for q in B.Profile(m, 50) if q["kernel"].startswith("attention_")]
                rows.append((n, h, l, hd, prec, p["kernel"], p["ms"], p["flops"]))
                m.Destroy()
child = subprocess.run([sys.executable, "-c", TORCH_SDPA, json.dumps(shapes)], capture_output=True, text=True, timeout=600)
tms = json.loads(child.stdout.strip().splitlines()[-1]) if child.returncode == 0 else None
if tms is None:
    print("# torch yardstick failed:", child.stderr.strip().splitlines()[-1:])
print(f"{'N,H,L,hd':>14} {'prec':>5} {'kernel':30} {'us':>9} {'TF/s':>7} {'torch sdpa us':>13}")
for n, h, l, hd, prec, kern, ms, flops in rows:
    t = tms[2 * shapes.index((n, h, l, hd)) + (prec == "fp16")] * 1e3 if tms else float("nan")
    print(f"{f'{n},{h},{l},{hd}':>14} {prec:>5} {kern:30} {ms * 1e3:9.1f} {flops / ms / 1e9:7.2f} {t:13.1f}")
