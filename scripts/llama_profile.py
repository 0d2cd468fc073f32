#!/usr/bin/env python3
"""Llama at SmolLM-135M's shape (30 x 576, 9 heads of 64 over 3 K / V heads, mlp 1536, vocab 49 152) as a prefill / scoring forward on one MI355X: what
DESIGN 3.30 records; or, as model llama_3b_layers, two layers of Llama-3.2-3B's shape (3072, 24 heads of 128 over 8 K / V heads, mlp 8192) behind a small
vocabulary: what DESIGN 3.31 records.

    python scripts/llama_profile.py [out_dir] [batch] [model]    seq 128 and seq 1 024, fp32 and fp16; writes <out_dir>/<model>.txt (default profiles/llama, llama_135m).
                                                                 batch (default 8): N L V 4 bytes of logits must stay below 2^31 (llama_135m: N L < 10 922)

* graph-replay time of the whole forward (median of 20 single replays after 3 warm ones; where a replay takes more than a second, of 2 after 1) and tokens/s
* the share of the eager forward per step family (HIP events around each launch, B.Profile)
* the attention step with the rotary embedding, against the step of the same graph written without the rope nodes (llama_135m) or the same forward under
  IE_ATTN_TILE=0, the generic kernel (llama_3b_layers: the only route of a head of 128 before tile 2 had a causal and a rotary form), and against torch's
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
MODELS = {"llama_135m": (49152, 576, 9, 3, 64), "llama_3b_layers": (1024, 3072, 24, 8, 128)}      # vocab, dim, heads, K / V heads, head dim
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


def measure(path, seq, n, prec, vocab, attn_tile):
    """child: one model, one precision -> one JSON line {replay_ms, steps: [[kernel, ms, flops, bytes], ...]}.  attn_tile: IE_ATTN_TILE ("": unset)"""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _pkg import load_package
    load_package()
    import numpy as np
    from gpu_ai_inference_server_amd import binding as B
    os.environ.update(IE_PRECISION=prec, IE_AUTOTUNE="0", **({"IE_ATTN_TILE": attn_tile} if attn_tile else {}))
    m = B.CreateModel(path, os.path.basename(path))
    try:
        din, _ = B.Prepare(m, [[n, seq]], 1)
        B.CopyToDevice(m, din[0], np.random.RandomState(0).randint(0, vocab, size=(n, seq)).astype(np.int64))
        t0 = time.perf_counter()
        B.RunPrepared(m, 1, True)
        slow = time.perf_counter() - t0 > 1.0      # (a forward on the generic kernel at seq 1 024 takes seconds: 2 replays and one profile pass)
        if not slow:
            B.RunPrepared(m, 2, True)
        ts = []
        for _ in range(2 if slow else 20):
            t0 = time.perf_counter()
            B.RunPrepared(m, 1, True)
            ts.append(time.perf_counter() - t0)
        prof = B.Profile(m, 1 if slow else 10)
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
    model = sys.argv[3] if len(sys.argv) > 3 else "llama_135m"
    VOCAB, DIM, HEADS, KV_HEADS, HD = MODELS[model]
    # the second forward each rotary one is set against: (what, rope spelling, IE_ATTN_TILE)
    other = ("written without the rope nodes", "none", "") if model == "llama_135m" else ("rotary, IE_ATTN_TILE=0 (the generic kernel)", "slice", "0")
    os.makedirs(out_dir, exist_ok=True)
    lines = []
    with tempfile.TemporaryDirectory() as root:
        for seq in (128, 1024):
            assert n * seq * VOCAB * 4 < 2 ** 31, "the logits must stay below 2^31 bytes"
            paths = {rope: models.write_repo(root, f"{model}_{seq}_{rope}", getattr(models, model)(n, seq=seq, rope=rope)) for rope in {"slice", other[1]}}
            for prec in ("fp32", "fp16"):
                us = {}
                for key, (label, rope, tile) in (("first", ("rotary", "slice", "")), ("other", other)):
                    what = f"{model} seq {seq} {prec} batch {n}, {label}"
                    r = child([os.path.abspath(__file__), "--one", paths[rope], str(seq), str(n), prec, str(VOCAB), tile], what)
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
                    us[key] = ms * 1e3
                    lines.append(f"  attention step ({k}): median of the {len(at)} steps {ms * 1e3:.1f} us, {flops / (ms * 1e-3) / 1e12:.2f} TFLOP/s of 2 N H L (L + 1) hd, the work needed")
                    rn = sorted((s for s in steps if s[0].startswith("rmsnorm")), key=lambda s: s[1])
                    k, ms = rn[len(rn) // 2][:2]
                    nbytes = 2 * n * seq * DIM * (2 if prec == "fp16" else 4)
                    lines.append(f"  rms norm step ({k}): median of the {len(rn)} steps {ms * 1e3:.1f} us, {nbytes / (ms * 1e-3) / 1e9:.0f} GB/s of one read and one write of [{n * seq}, {DIM}]")
                sdpa = child(["-c", TORCH_SDPA, json.dumps([n, HEADS, KV_HEADS, seq, HD, prec])], f"torch SDPA (N {n}, H {HEADS}, L {seq}, hd {HD}) {prec}")
                qk_bytes = 2 * n * seq * (HEADS + KV_HEADS) * HD * (2 if prec == "fp16" else 4)
                if other[1] == "none":             # against the graph without the rope nodes: what the rotation costs
                    versus = (f"(difference {us['first'] - us['other']:.1f} us; one read and one write of the q and k columns at 6.3 TB/s: "
                              f"{qk_bytes / 6.3e12 * 1e6:.1f} us)")
                else:                              # against the generic kernel on the same graph
                    versus = f"({us['other'] / us['first']:.0f} x)"
                lines.append(f"attention (N {n}, H {HEADS} / {KV_HEADS}, L {seq}, hd {HD}) {prec}: rotary {us['first']:.1f} us, {other[0]} {us['other']:.1f} us {versus}; "
                             f"torch SDPA is_causal with K / V expanded {sdpa['causal'] * 1e3:.1f} us")
                print("\n".join(lines[-3:]), flush=True)
    text = "\n".join(lines) + "\n"
    open(os.path.join(out_dir, model + ".txt"), "w").write(text)
    print(text)


if __name__ == "__main__":
    if len(sys.argv) == 8 and sys.argv[1] == "--one":
        measure(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5], int(sys.argv[6]), sys.argv[7])
    else:
        main()
