#!/usr/bin/env python3
"""Llama at SmolLM-135M's shape (30 x 576, 9 heads of 64 over 3 K / V heads, mlp 1536, vocab 49 152) as a prefill / scoring forward on one MI355X: what
DESIGN 3.30 records.

    python scripts/llama_profile.py [out_dir] [batch]       seq 128 and seq 1 024, fp32 and fp16; writes <out_dir>/llama_135m.txt (default profiles/llama).
                                                            batch (default 8): N L V 4 bytes of logits must stay below 2^31 (N L < 10 922)

* graph-replay time of the whole forward (median of 20 single replays after 3 warm ones) and tokens/s
* the share of the eager forward per step family (HIP events around each launch, B.Profile)
* the attention step with the rotary embedding, against the step of the same graph written without the rope nodes, and against torch's
  F.scaled_dot_product_attention(is_causal=True) on [N, H, L, hd] operands with K and V expanded to H heads, timed in a process of its own.  TFLOP/s of a
  causal step counts 2 N H L (L + 1) hd, the work actually needed
* the RMSNorm step's GB/s (one read and one write of the tokens)
Every measurement is a child process under its own time limit; the first one that fails ends the run."""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB, DIM, HEADS, KV_HEADS, HD = 49152, 576, 9, 3, 64
STEP_TIMEOUT = 600

TORCH_SDPA = """
import json, sys, torch
import torch.nn.functional as F
n, h, hkv, l, hd, prec = json.loads(sys.argv[1])
dt = torch.float16 if prec == "fp16" else torch.float32
q = torch.randn(n, h, l, hd, device="cuda", dtype=dt)
k, v = (torch.randn(n, hkv, l, hd, device="cuda", dtype=dt).repeat_interleave(h // hkv, dim=1) for _ in range(2))
f = lambda: F.scaled_dot_product_attention(q, k, v, is_causal=True)
for _ in range(5):
    f()
ts = []
for _ in range(30):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); f(); e1.record()
    torch.cuda.synchronize()
    ts.append(e0.elapsed_time(e1))
print(json.dumps({"causal": sorted(ts)[len(ts) // 2]}))
"""


def family(k):
    for key, name in (("embed", "embed"), ("attention", "attention"), ("rmsnorm", "rms norm"), ("eltwise", "gated unit (eltwise)"), ("copy", "copy")):
        if k.startswith(key):
            return name
    return "Linears and the head (1x1 convs)"


def measure(path, seq, n, prec):
    """child: one model, one precision -> one JSON line {replay_ms, steps: [[kernel, ms, flops, bytes], ...]}"""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _pkg import load_package
    load_package()
    import numpy as np
    from gpu_ai_inference_server_amd import binding as B
    os.environ.update(IE_PRECISION=prec, IE_AUTOTUNE="0")
    m = B.CreateModel(path, os.path.basename(path))
    try:
        din, _ = B.Prepare(m, [[n, seq]], 1)
        B.CopyToDevice(m, din[0], np.random.RandomState(0).randint(0, VOCAB, size=(n, seq)).astype(np.int64))
        B.RunPrepared(m, 3, True)
        ts = []
        for _ in range(20):
            t0 = time.perf_counter()
            B.RunPrepared(m, 1, True)
            ts.append(time.perf_counter() - t0)
        prof = B.Profile(m, 10)
    finally:
        m.Destroy()
    print(json.dumps({"replay_ms": sorted(ts)[len(ts) // 2] * 1e3, "steps": [[p["kernel"], p["ms"], p["flops"], p.get("bytes", 0)] for p in prof]}))


def child(args, what):
    try:
        r = subprocess.run([sys.executable] + args, capture_output=True, text=True, timeout=STEP_TIMEOUT)
    except subprocess.TimeoutExpired:
        sys.exit(f"{what}: ran into its time limit; nothing further is started")
    if r.returncode != 0 or not r.stdout.strip():
        sys.exit(f"{what}: failed with status {r.returncode} (nothing further is started): " + " | ".join(r.stderr.strip().splitlines()[-3:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _pkg import load_package
    load_package()
    from gpu_ai_inference_server_amd.modelgen import models
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "llama")
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    os.makedirs(out_dir, exist_ok=True)
    lines = []
    with tempfile.TemporaryDirectory() as root:
        for seq in (128, 1024):
            assert n * seq * VOCAB * 4 < 2 ** 31, "the logits must stay below 2^31 bytes"
            paths = {rope: models.write_repo(root, f"llama_135m_{seq}_{rope}", models.llama_135m(n, seq=seq, rope=rope)) for rope in ("slice", "none")}
            for prec in ("fp32", "fp16"):
                us = {}
                for rope, path in paths.items():
                    what = f"llama_135m seq {seq} {prec} batch {n}, {'rotary' if rope != 'none' else 'written without the rope nodes'}"
                    r = child([os.path.abspath(__file__), "--one", path, str(seq), str(n), prec], what)
                    steps = r["steps"]
                    total = sum(s[1] for s in steps)
                    lines.append(f"{what}:")
                    lines.append(f"  graph replay {r['replay_ms']:.3f} ms = {n * seq / r['replay_ms'] * 1e3:.0f} tokens/s; eager sum of steps {total:.3f} ms over {len(steps)} steps")
                    fam = {}
                    for s in steps:
                        e = fam.setdefault(family(s[0]), [0, 0.0])
                        e[0] += 1
                        e[1] += s[1]
                    for k, (cnt, ms) in sorted(fam.items(), key=lambda kv: -kv[1][1]):
                        lines.append(f"    {k:34s} {cnt:3d} steps {ms:9.3f} ms {100 * ms / total:5.1f} %")
                    at = sorted((s for s in steps if s[0].startswith("attention")), key=lambda s: s[1])
                    k, ms, flops = at[len(at) // 2][:3]
                    us[rope] = ms * 1e3
                    lines.append(f"  attention step ({k}): median of the {len(at)} steps {ms * 1e3:.1f} us, {flops / (ms * 1e-3) / 1e12:.2f} TFLOP/s of 2 N H L (L + 1) hd, the work needed")
                    rn = sorted((s for s in steps if s[0].startswith("rmsnorm")), key=lambda s: s[1])
                    k, ms = rn[len(rn) // 2][:2]
                    nbytes = 2 * n * seq * DIM * (2 if prec == "fp16" else 4)
                    lines.append(f"  rms norm step ({k}): median of the {len(rn)} steps {ms * 1e3:.1f} us, {nbytes / (ms * 1e-3) / 1e9:.0f} GB/s of one read and one write of [{n * seq}, {DIM}]")
                sdpa = child(["-c", TORCH_SDPA, json.dumps([n, HEADS, KV_HEADS, seq, HD, prec])], f"torch SDPA (N {n}, H {HEADS}, L {seq}, hd {HD}) {prec}")
                qk_bytes = 2 * n * seq * (HEADS + KV_HEADS) * HD * (2 if prec == "fp16" else 4)
                lines.append(f"attention (N {n}, H {HEADS} / {KV_HEADS}, L {seq}, hd {HD}) {prec}: rotary {us['slice']:.1f} us, without the rope nodes {us['none']:.1f} us "
                             f"(difference {us['slice'] - us['none']:.1f} us; one read and one write of the q and k columns at 6.3 TB/s: {qk_bytes / 6.3e12 * 1e6:.1f} us); "
                             f"torch SDPA is_causal with K / V expanded {sdpa['causal'] * 1e3:.1f} us")
                print("\n".join(lines[-3:]), flush=True)
    text = "\n".join(lines) + "\n"
    open(os.path.join(out_dir, "llama_135m.txt"), "w").write(text)
    print(text)


if __name__ == "__main__":
    if len(sys.argv) == 6 and sys.argv[1] == "--one":
        measure(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5])
    else:
        main()
