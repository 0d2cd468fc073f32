#!/usr/bin/env python3
"""An extend step (a past of P rows and Lq >= 2 new tokens) of a Llama-class model on one MI355X: what DESIGN 3.33 records.

    python scripts/extend_profile.py [out_dir]      writes <out_dir>/extend_attention.txt and <out_dir>/llama_135m_extend.txt (default profiles/extend)

* the extend attention step alone (tests/extend_graphs.extend_attn_graph: rope at run-time positions, the chunk mask, every cache row valid) at
  (N, H / Hkv, P, hd) = (8, 9 / 3, 1 023, 64) for Lq = 4, 16, 128, 512 and at (1, 9 / 3, 4 095, 64) for Lq = 8, fp32 and fp16: tile 5 (the kv_append
  launch and attention_extend_kernel) under the planner's split count, a sweep of IE_ATTN_SPLITS, the generic pair (kv_append_kernel,
  attention_extend_generic_kernel), and torch's F.scaled_dot_product_attention with the same boolean mask on the same `present` with K / V expanded
  to H heads, in a process of its own (its time has neither the append nor the rotation in it)
* tile 5 against the generic pair at the fewest query rows g * Lq there are: the table behind kernels.h kAttnExtendMinRows
* llama_135m (modelgen.llama_135m(8, seq=128, past=1023)): graph replay of one step, tokens/s, the share of the step families; the same under IE_ATTN_TILE=0
Step times are HIP events around each launch (B.Profile, median of 20).  Every group of measurements is a child process under its own time limit; the
first one that fails ends the run."""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((8, 9, 3, 1023, 64, 4), (8, 9, 3, 1023, 64, 16), (8, 9, 3, 1023, 64, 128), (8, 9, 3, 1023, 64, 512), (1, 9, 3, 4095, 64, 8))
STEP_TIMEOUT = 600

TORCH_SDPA = """
import json, sys, torch
import torch.nn.functional as F
n, h, hkv, past, lq, hd, prec = json.loads(sys.argv[1])
dt = torch.float16 if prec == "fp16" else torch.float32
q = torch.randn(n, h, lq, hd, device="cuda", dtype=dt)
k, v = (torch.randn(n, hkv, past + lq, hd, device="cuda", dtype=dt).repeat_interleave(h // hkv, dim=1) for _ in range(2))
i, j = torch.arange(lq, device="cuda")[:, None], torch.arange(past + lq, device="cuda")[None, :]
mask = (j <= past + i)[None, None]
f = lambda: F.scaled_dot_product_attention(q, k, v, attn_mask=mask)
for _ in range(5):
    f()
ts = []
for _ in range(30):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); f(); e1.record()
    torch.cuda.synchronize()
    ts.append(e0.elapsed_time(e1))
print(json.dumps({"ms": sorted(ts)[len(ts) // 2]}))
"""


def _setup():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _pkg import load_package
    load_package()


def attention_child(configs):
    """child: [(n, h, hkv, past, hd, lq, prec, env)] -> [{kernel, ms, tile}] of the attention step of each, one model after the other"""
    _setup()
    import extend_graphs as EG
    from engine_run import with_env
    from gpu_ai_inference_server_amd import binding as B
    from gpu_ai_inference_server_amd.modelgen import models
    out = []
    with tempfile.TemporaryDirectory() as root:
        for i, (n, h, hkv, past, hd, lq, prec, env) in enumerate(configs):
            rows, feeds = EG.extend_feeds(n, h, hkv, hd, past, lq, positions=[list(range(past, past + lq))] * n, max_pos=past + lq)
            path = models.write_repo(root, f"a{i}", EG.extend_attn_graph(rows, n, h, hkv, hd, past, lq, max_pos=past + lq))

            def go():
                plan = B.DescribeModel(path, n)["plan"]
                (at,) = [s for s in plan["steps"] if s["kind"] == "attention"]
                m = B.CreateModel(path, f"a{i}")
                try:
                    din, _ = B.Prepare(m, [list(v.shape) for v in feeds.values()], 3)
                    for d, v in zip(din, feeds.values()):
                        B.CopyToDevice(m, d, v)
                    B.RunPrepared(m, 3, True)
                    (p,) = [p for p in B.Profile(m, 20) if "attention_extend" in p["kernel"]]
                    return {"kernel": p["kernel"], "ms": p["ms"], "tile": at["tile"], "splits": at.get("splits", 0)}
                finally:
                    m.Destroy()
            out.append(with_env(dict(IE_PRECISION=prec, IE_AUTOTUNE="0", **env), go))
    print(json.dumps(out))


def model_child(path, n, past, lq, prec, tile, vocab, depth, hkv, hd):
    """child: llama_135m's extend graph -> {replay_ms, steps}"""
    _setup()
    import numpy as np
    from gpu_ai_inference_server_amd import binding as B
    os.environ.update(IE_PRECISION=prec, IE_AUTOTUNE="0", **({"IE_ATTN_TILE": tile} if tile else {}))
    r = np.random.RandomState(0)
    feeds = [r.randint(0, vocab, (n, lq)).astype(np.int64), np.ones((n, past + lq), np.int64), np.tile(np.arange(past, past + lq, dtype=np.int64), (n, 1))]
    feeds += [r.randn(n, hkv, past, hd).astype(np.float32) for _ in range(2 * depth)]
    m = B.CreateModel(path, os.path.basename(path))
    try:
        din, _ = B.Prepare(m, [list(v.shape) for v in feeds], 1 + 2 * depth)
        for d, v in zip(din, feeds):
            B.CopyToDevice(m, d, v)
        B.RunPrepared(m, 3, True)
        ts = []
        for _ in range(20):
            t0 = time.perf_counter()
            B.RunPrepared(m, 1, True)
            ts.append(time.perf_counter() - t0)
        prof = B.Profile(m, 10)
    finally:
        m.Destroy()
    print(json.dumps({"replay_ms": sorted(ts)[len(ts) // 2] * 1e3, "steps": [[p["kernel"], p["ms"]] for p in prof]}))


def child(args, what):
    try:
        r = subprocess.run([sys.executable] + args, capture_output=True, text=True, timeout=STEP_TIMEOUT)
    except subprocess.TimeoutExpired:
        sys.exit(f"{what}: ran into its time limit; nothing further is started")
    if r.returncode != 0 or not r.stdout.strip():
        sys.exit(f"{what}: failed with status {r.returncode} (nothing further is started): " + " | ".join(r.stderr.strip().splitlines()[-3:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def family(k):
    for key, name in (("embed", "embed"), ("kv_append", "attention (append + extend)"), ("attention_extend", "attention (append + extend)"), ("rmsnorm", "rms norm"),
                      ("eltwise", "gated unit (eltwise)"), ("copy", "copy")):
        if k.startswith(key):
            return name
    return "Linears (1x1 convs)"


def main():
    _setup()
    from gpu_ai_inference_server_amd.modelgen import models
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "extend")
    os.makedirs(out_dir, exist_ok=True)
    me = os.path.abspath(__file__)
    lines = []
    sweep = (1, 2, 4, 8, 16, 32)
    for n, h, hkv, past, hd, lq in SHAPES:
        for prec in ("fp32", "fp16"):
            what = f"extend attention (N {n}, H {h} / {hkv}, P {past}, Lq {lq}, hd {hd}) {prec}"
            cfg = [(n, h, hkv, past, hd, lq, prec, {}), (n, h, hkv, past, hd, lq, prec, {"IE_ATTN_TILE": "0"})] + [(n, h, hkv, past, hd, lq, prec, {"IE_ATTN_SPLITS": str(s)}) for s in sweep]
            res = child([me, "--attn", json.dumps(cfg)], what)
            sdpa = child(["-c", TORCH_SDPA, json.dumps([n, h, hkv, past, lq, hd, prec])], f"torch SDPA for {what}")
            d, t0 = res[0], res[1]
            lines.append(f"{what}:")
            lines.append(f"  tile 5, S = {d['splits']} (the planner's): {d['ms'] * 1e3:9.1f} us = {d['ms'] * 1e3 / lq:8.1f} us per new token   [{d['kernel']}]")
            lines.append(f"  tile 0, the generic pair:         {t0['ms'] * 1e3:9.1f} us ({t0['ms'] / d['ms']:.2f} x)   [{t0['kernel']}]")
            lines.append(f"  torch SDPA, boolean mask, K / V expanded, no append, no rotation: {sdpa['ms'] * 1e3:9.1f} us ({sdpa['ms'] / d['ms']:.2f} x)")
            lines.append("  IE_ATTN_SPLITS sweep: " + ", ".join(f"S {r['splits']}: {r['ms'] * 1e3:.1f} us" for r in res[2:]))
            print("\n".join(lines[-5:]), flush=True)
    lines.append("tile 5 (the planner's S) against the generic pair at few query rows g * Lq, (N 8, P 1023, hd 64):")
    for prec in ("fp32", "fp16"):
        small = ((3, 3, 2), (9, 3, 2), (9, 3, 4), (9, 3, 8))       # (H, Hkv, Lq): 2, 6, 12 and 24 rows
        cfg = [(8, h, hkv, 1023, 64, lq, prec, {"IE_ATTN_TILE": t}) for h, hkv, lq in small for t in ("5", "0")]
        res = child([me, "--attn", json.dumps(cfg)], f"threshold sweep {prec}")
        for i, (h, hkv, lq) in enumerate(small):
            a, b = res[2 * i], res[2 * i + 1]
            lines.append(f"  {prec} H {h} / {hkv}, Lq {lq} ({h // hkv * lq:2d} rows): tile 5 (S {a['splits']}) {a['ms'] * 1e3:7.1f} us, generic pair {b['ms'] * 1e3:7.1f} us ({b['ms'] / a['ms']:.2f} x)")
    print("\n".join(lines[-9:]), flush=True)
    open(os.path.join(out_dir, "extend_attention.txt"), "w").write("\n".join(lines) + "\n")

    lines = []
    N, PAST, LQ, VOCAB, DEPTH, HKV, HD = 8, 1023, 128, 49152, 30, 3, 64
    with tempfile.TemporaryDirectory() as root:
        path = models.write_repo(root, "llama_135m_extend", models.llama_135m(N, seq=LQ, past=PAST))
        for prec, tile in (("fp32", ""), ("fp32", "0"), ("fp16", ""), ("fp16", "0")):
            what = f"llama_135m extend step, batch {N}, P {PAST}, Lq {LQ}, {prec}" + (", IE_ATTN_TILE=0" if tile else "")
            r = child([me, "--model", path, str(N), str(PAST), str(LQ), prec, tile, str(VOCAB), str(DEPTH), str(HKV), str(HD)], what)
            steps = r["steps"]
            total = sum(s[1] for s in steps)
            lines.append(f"{what}:")
            lines.append(f"  graph replay {r['replay_ms']:.3f} ms = {N * LQ / r['replay_ms'] * 1e3:.0f} tokens/s; eager sum of steps {total:.3f} ms over {len(steps)} steps")
            fam = {}
            for i, s in enumerate(steps):
                e = fam.setdefault("the vocabulary head" if i == len(steps) - 1 else family(s[0]), [0, 0.0])
                e[0] += 1
                e[1] += s[1]
            for k, (cnt, ms) in sorted(fam.items(), key=lambda kv: -kv[1][1]):
                lines.append(f"    {k:34s} {cnt:3d} steps {ms:9.3f} ms {100 * ms / total:5.1f} %")
            print("\n".join(lines[-8:]), flush=True)
    open(os.path.join(out_dir, "llama_135m_extend.txt"), "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--attn":
        attention_child(json.loads(sys.argv[2]))
    elif len(sys.argv) == 12 and sys.argv[1] == "--model":
        model_child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), sys.argv[6], sys.argv[7], *(int(v) for v in sys.argv[8:12]))
    else:
        main()
