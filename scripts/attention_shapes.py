#!/usr/bin/env python3
"""The attention step alone at given shapes, on the generic kernel (tile 0) and on the MFMA kernels of its head dim (tile 1 and tile 3, the chunk kernel,
for hd 32 / 64; tile 2, the streaming kernel for one wide head, for hd 128 / 256 / 512) in both precisions, next to torch's
F.scaled_dot_product_attention on the same shapes.  causal = 1: the causal step (gpt2_graphs.causal_attn_graph) and torch's is_causal.
--causal makes every case causal; --kv-heads K gives every case K grouped K / V heads and --rope the rotary embedding (llama_graphs.gqa_attn_graph: the
kernel reads the raw input as q | k | v of H + 2 K heads; --rope implies --causal); torch's yardstick then runs on K and V expanded to H heads, q and k
taken as rotated beforehand (the rotation is not in its time).

    python scripts/attention_shapes.py [--causal] [--rope] [--kv-heads K] [--tiles T,...] [--no-torch] [N,H,L,hd[,half[,causal]] ...]

default: the VAE decoder's step (base 128, latent 32: fp32 batch 8, fp16 batch 32), latent 64, two multi-head shapes and the crossover grid
L {64, 128, 256} x hd {128, 512} x N {2, 8} (profiles/attn_vit: 32,12,197,64 32,12,50,64, ViT-B/16 and ViT-B/32 at batch 32)

The graph is tests/vit_graphs.py attn_graph (the kernel reads the raw input as q | k | v); the figures are the attention step's own, from HIP events
around its launch (B.Profile: median of 20 passes, of 3 where a pass takes more than 50 ms, one pass where it takes more than a second), IE_AUTOTUNE=0;
--tiles measures those tiles only, --no-torch leaves torch's column empty (nan).  TFLOP/s counts 4 N H L^2 hd, and for a
causal step 2 N H L (L + 1) hd, the work actually needed (the lower triangle); the share is of the MFMA rate, 155 TF in fp32 and 2.5 PF in fp16.  Every measurement is a process of its own under a time limit, torch's too, and the first one
that fails ends the run."""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_TF = {0: 155.0, 1: 2500.0}
STEP_TIMEOUT = 180

TORCH_SDPA = """
import json, sys, torch
import torch.nn.functional as F
out = []
for n, h, l, hd, half, causal, kvh in json.loads(sys.argv[1]):
    dt = torch.float16 if half else torch.float32
    q = torch.randn(n, h, l, hd, device="cuda", dtype=dt)
    k, v = (torch.randn(n, kvh or h, l, hd, device="cuda", dtype=dt).repeat_interleave(h // (kvh or h), dim=1) for _ in range(2))
    f = lambda: F.scaled_dot_product_attention(q, k, v, is_causal=bool(causal))
    for _ in range(3):
        f()
    ts = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    out.append(sorted(ts)[len(ts) // 2])
print(json.dumps(out))
"""


def measure(n, h, l, hd, half, causal=0, kvh=0, rope=0, tiles=None):
    """child: the tiles of one case -> one JSON line [[kernel, ms, passes], ...].  kvh: grouped K / V heads (0: one per head, the q | k | v graphs);
    rope: the rotary embedding (with kvh or rope the graph is llama_graphs.gqa_attn_graph); tiles: those tiles only (None: the head dim's)"""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _pkg import load_package
    load_package()
    import numpy as np
    import gpt2_graphs as GG
    import llama_graphs as LG
    import vit_graphs as G
    from gpu_ai_inference_server_amd import binding as B
    from gpu_ai_inference_server_amd.modelgen import models
    c = (h + 2 * (kvh or h)) * hd                  # channels of a q | k | v row
    out = []
    with tempfile.TemporaryDirectory() as root:
        if kvh or rope:
            mb = LG.gqa_attn_graph(n, l, h, kvh or h, hd, rope="init" if rope else None, causal=bool(causal))
        else:
            mb = GG.causal_attn_graph(n, l, h, hd) if causal else G.attn_graph(n, l, h, hd)
        path = models.write_repo(root, "attn", mb)
        x = np.random.RandomState(0).randn(n, c, 1, l).astype(np.float32)
        for tile in tiles or ((1, 3, 0) if hd in (32, 64) else (2, 0)):
            os.environ.update(IE_AUTOTUNE="0", IE_PRECISION="fp16" if half else "fp32", IE_ATTN_TILE=str(tile))
            m = B.CreateModel(path, "attn")
            try:
                din, _ = B.Prepare(m, [[n, c, 1, l]], 1)
                B.CopyToDevice(m, din[0], x)
                B.RunPrepared(m, 1, True)
                step = lambda prof: [q for q in prof if q["kernel"].startswith("attention_")][0]  # noqa: E731
                first = step(B.Profile(m, 1))
                passes = 1 if first["ms"] > 1000.0 else 3 if first["ms"] > 50.0 else 20
                p = first if passes == 1 else step(B.Profile(m, passes))
                if p["kernel"] not in [o[0] for o in out]:      # (a pinned tile that does not fit the shape is the generic kernel: once)
                    out.append([p["kernel"], p["ms"], passes])
            finally:
                m.Destroy()
    print(json.dumps(out))


def main():
    args = sys.argv[1:]
    rope = int("--rope" in args)
    causal = int("--causal" in args or rope)
    kvh = int(args[args.index("--kv-heads") + 1]) if "--kv-heads" in args else 0
    tiles = [args[args.index("--tiles") + 1]] if "--tiles" in args else []
    no_torch = "--no-torch" in args
    args = [a for i, a in enumerate(args) if a not in ("--rope", "--causal", "--kv-heads", "--tiles", "--no-torch") and (i == 0 or args[i - 1] not in ("--kv-heads", "--tiles"))]
    if args:
        cases = []
        for a in args:
            v = tuple(int(t) for t in a.split(","))
            cases += [v + (0,)] if len(v) == 5 else [v] if len(v) == 6 else [v + (0, 0), v + (1, 0)]
    else:
        cases = [(8, 1, 1024, 512, 0), (32, 1, 1024, 512, 1), (1, 1, 4096, 512, 0), (1, 1, 4096, 512, 1)]
        cases += [(8, 8, 1024, 128, half) for half in (0, 1)] + [(8, 2, 1024, 256, half) for half in (0, 1)]
        cases += [(n, 1, l, hd, half) for half in (0, 1) for hd in (128, 512) for l in (64, 128, 256) for n in (2, 8)]
        cases = [c + (0,) for c in cases]
    cases = [c[:5] + (int(c[5] or causal), kvh, rope) for c in cases]
    if kvh or rope:
        print(f"grouped K / V heads: {kvh or 'one per head'}; rotary embedding: {'yes' if rope else 'no'}", flush=True)
    if no_torch:
        tms = [float("nan")] * len(cases)
    else:
        try:
            child = subprocess.run([sys.executable, "-c", TORCH_SDPA, json.dumps([c[:7] for c in cases])], capture_output=True, text=True, timeout=STEP_TIMEOUT)
        except subprocess.TimeoutExpired:
            sys.exit("torch yardstick ran into its time limit; nothing further is started")
        if child.returncode != 0:
            sys.exit("torch yardstick failed (nothing further is started): " + " | ".join(child.stderr.strip().splitlines()[-3:]))
        tms = json.loads(child.stdout.strip().splitlines()[-1])
    print(f"{'N,H,L,hd':>16} {'prec':>5} {'kernel':44} {'us':>10} {'passes':>6} {'TFLOP/s':>8} {'% MFMA':>7} {'torch sdpa us':>13}", flush=True)
    for case, tms_case in zip(cases, tms):
        n, h, l, hd, half, causal = case[:6]
        try:
            child = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", ",".join(map(str, case))] + tiles, capture_output=True, text=True, timeout=STEP_TIMEOUT)
        except subprocess.TimeoutExpired:
            sys.exit(f"{case}: ran into its time limit; nothing further is started")
        if child.returncode != 0:
            sys.exit(f"{case}: failed with status {child.returncode} (nothing further is started): " + " | ".join(child.stderr.strip().splitlines()[-3:]))
        for kern, ms, passes in json.loads(child.stdout.strip().splitlines()[-1]):
            tf = (2.0 * n * h * l * (l + 1) * hd if causal else 4.0 * n * h * l * l * hd) / ms / 1e9
            print(f"{f'{n},{h},{l},{hd}':>16} {'fp16' if half else 'fp32':>5} {kern:44} {ms * 1e3:10.1f} {passes:6d} {tf:8.2f} {tf / PEAK_TF[half] * 100:6.2f}% {tms_case * 1e3:13.1f}",
                  flush=True)


if __name__ == "__main__":
    if len(sys.argv) in (3, 4) and sys.argv[1] == "--one":      # (the child: N,H,L,hd,half,causal,kv_heads,rope [tiles])
        measure(*(int(t) for t in sys.argv[2].split(",")), tiles=[int(t) for t in sys.argv[3].split(",")] if len(sys.argv) == 4 else None)
    else:
        main()
