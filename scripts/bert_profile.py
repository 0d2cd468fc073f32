#!/usr/bin/env python3
"""BERT-base (seq 128) on one MI355X: what DESIGN 3.26 records.

    python scripts/bert_profile.py [out_dir]          fp32 at batch 32 and fp16 at batch 128; writes <out_dir>/bert_base.txt (default profiles/bert)

* graph-replay time of the whole forward (median of 30 single replays after 5 warm ones) and sequences/s
* the share of the eager forward per step family (HIP events around each launch, B.Profile)
* the masked attention step against the unmasked step of the same graph written without a mask, and against torch's
  F.scaled_dot_product_attention with the same additive key mask on [N, H, L, hd] operands, timed in a process of its own
* the embed step: microseconds and algorithmic TB/s, with fresh random ids uploaded before every timed launch.  The whole word table (94 MB) fits the
  256 MB Infinity Cache, so this is a warm-cache rate whatever the ids are; it says nothing about HBM"""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _pkg import load_package  # noqa: E402

load_package()
import numpy as np  # noqa: E402
from gpu_ai_inference_server_amd import binding as B  # noqa: E402
from gpu_ai_inference_server_amd.modelgen import models  # noqa: E402

SEQ, VOCAB, HEADS, HD = 128, 30522, 12, 64

TORCH_SDPA = """
import json, sys, torch
import torch.nn.functional as F
n, h, l, hd, prec = json.loads(sys.argv[1])
dt = torch.float16 if prec == "fp16" else torch.float32
q, k, v = (torch.randn(n, h, l, hd, device="cuda", dtype=dt) for _ in range(3))
keep = torch.arange(l, device="cuda")[None, :] < torch.randint(1, l + 1, (n, 1), device="cuda")
mask = ((~keep).to(dt) * torch.finfo(dt).min)[:, None, None, :]
out = {}
for name, m in (("masked", mask), ("unmasked", None)):
    f = lambda: F.scaled_dot_product_attention(q, k, v, attn_mask=m)
    for _ in range(5):
        f()
    ts = []
    for _ in range(30):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); f(); e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    out[name] = sorted(ts)[len(ts) // 2]
print(json.dumps(out))
"""


def family(p):
    k = p["kernel"]
    for key, name in (("embed", "embed"), ("attention", "attention"), ("layernorm", "layer norm"), ("eltwise", "GELU / tanh (eltwise)"), ("copy", "copy")):
        if k.startswith(key):
            return name
    return "Linears (1x1 convs)"


def feeds(n, rng, mask=True):
    f = {"input_ids": rng.randint(0, VOCAB, size=(n, SEQ)).astype(np.int64)}
    if mask:
        f["attention_mask"] = (np.arange(SEQ)[None, :] < rng.randint(1, SEQ + 1, size=(n, 1))).astype(np.int64)
    f["token_type_ids"] = rng.randint(0, 2, size=(n, SEQ)).astype(np.int64)
    return f


def measure(path, name, n, mask, lines):
    rng = np.random.RandomState(0)
    m = B.CreateModel(path, name)
    try:
        f = feeds(n, rng, mask)
        din, _ = B.Prepare(m, [[n, SEQ]] * len(f), 1)
        for d, a in zip(din, f.values()):
            B.CopyToDevice(m, d, a)
        B.RunPrepared(m, 5, True)
        ts = []
        for _ in range(30):
            t0 = time.perf_counter()
            B.RunPrepared(m, 1, True)
            ts.append(time.perf_counter() - t0)
        replay = sorted(ts)[len(ts) // 2]
        prof = B.Profile(m, 20)
        emb = []
        for _ in range(10):                         # fresh ids before every timed embed launch
            B.CopyToDevice(m, din[0], rng.randint(0, VOCAB, size=(n, SEQ)).astype(np.int64))
            emb.append(B.Profile(m, 1)[0])
    finally:
        m.Destroy()
    total = sum(p["ms"] for p in prof)
    lines.append(f"  graph replay {replay * 1e3:.3f} ms = {n / replay:.0f} sequences/s; eager sum of steps {total:.3f} ms over {len(prof)} steps")
    fam = {}
    for p in prof:
        e = fam.setdefault(family(p), [0, 0.0])
        e[0] += 1
        e[1] += p["ms"]
    for k, (cnt, ms) in sorted(fam.items(), key=lambda kv: -kv[1][1]):
        lines.append(f"    {k:28s} {cnt:3d} steps {ms:8.3f} ms {100 * ms / total:5.1f} %")
    at = [p for p in prof if p["kernel"].startswith("attention")]
    us = sorted(p["ms"] for p in at)[len(at) // 2] * 1e3
    lines.append(f"  attention step ({at[0]['kernel']}): median of the 12 steps {us:.1f} us, {at[0]['flops'] / (us * 1e-6) / 1e12:.1f} TFLOP/s")
    e = sorted(emb, key=lambda p: p["ms"])[len(emb) // 2]
    lines.append(f"  embed step ({e['kernel']}), fresh ids per launch, cache-resident tables: median {e['ms'] * 1e3:.1f} us, {e['bytes'] / 1e6:.1f} MB algorithmic, "
                 f"{e['bytes'] / (e['ms'] * 1e-3) / 1e12:.2f} algorithmic TB/s")
    return us


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bert")
    os.makedirs(out_dir, exist_ok=True)
    lines = []
    with tempfile.TemporaryDirectory() as root:
        paths = {mask: models.write_repo(root, "bert_base_mask" if mask else "bert_base_bare", models.bert_base("N", mask=mask)) for mask in (True, False)}
        for prec, n in (("fp32", 32), ("fp16", 128)):
            os.environ.update(IE_PRECISION=prec, IE_AUTOTUNE="0")
            us = {}
            for mask in (True, False):
                lines.append(f"bert_base seq {SEQ} {prec} batch {n}, {'key mask' if mask else 'written without a mask'}:")
                us[mask] = measure(paths[mask], "bert_base_mask" if mask else "bert_base_bare", n, mask, lines)
            r = subprocess.run([sys.executable, "-c", TORCH_SDPA, json.dumps([n, HEADS, SEQ, HD, prec])], capture_output=True, text=True, timeout=300)
            sdpa = json.loads(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 and r.stdout.strip() else None
            lines.append(f"attention (N {n}, H {HEADS}, L {SEQ}, hd {HD}) {prec}: masked {us[True]:.1f} us, unmasked {us[False]:.1f} us"
                         + (f"; torch SDPA masked {sdpa['masked'] * 1e3:.1f} us, unmasked {sdpa['unmasked'] * 1e3:.1f} us" if sdpa else f"; torch SDPA not measured ({r.stderr.strip()[-200:]})"))
    text = "\n".join(lines) + "\n"
    open(os.path.join(out_dir, "bert_base.txt"), "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
