#!/usr/bin/env python3
"""The decode step of a Llama-class model with a KV cache on one MI355X: what DESIGN 3.32 records.

    python scripts/decode_profile.py [out_dir]      writes <out_dir>/decode_attention.txt and <out_dir>/llama_135m_decode.txt (default profiles/decode)

* the decode attention step alone (tests/kv_graphs.decode_attn_graph: rope at run-time positions, key mask, every cache row valid) at (N, H / Hkv, P, hd) =
  (8, 9 / 3, 1 023, 64), (8, 24 / 8, 1 023, 128) and (1, 32 / 8, 4 095, 128), fp32 and fp16: the time of tile 4 under the planner's split count, the
  algorithmic rate (read past K, V + write present K, V) / time against the project's measured copy rate, tile 0's two launches, a sweep of
  IE_ATTN_SPLITS, and torch's F.scaled_dot_product_attention with one query on the same cache with K / V expanded to H heads, in a process of its own
  (its time has no append and no rotation in it)
* tile 4 against the parts over the cache length at the first shape: the table behind kernels.h kAttnDecodeMinKeys
* llama_135m (modelgen.llama_135m(8, seq=1, past=1023)): graph replay of one step, tokens/s, the share of the step families; the same under IE_ATTN_TILE=0
Step times are HIP events around each launch (B.Profile, median of 20).  Every group of measurements is a child process under its own time limit; the
first one that fails ends the run."""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((8, 9, 3, 1023, 64), (8, 24, 8, 1023, 128), (1, 32, 8, 4095, 128))
COPY_RATE = 6.29e12          # bytes/s: the project's measured device copy rate
STEP_TIMEOUT = 900

TORCH_SDPA = """
import json, sys, torch
import torch.nn.functional as F
n, h, hkv, keys, hd, prec = json.loads(sys.argv[1])
dt = torch.float16 if prec == "fp16" else torch.float32
q = torch.randn(n, h, 1, hd, device="cuda", dtype=dt)
k, v = (torch.randn(n, hkv, keys, hd, device="cuda", dtype=dt).repeat_interleave(h // hkv, dim=1) for _ in range(2))
f = lambda: F.scaled_dot_product_attention(q, k, v)
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
    """child: [(n, h, hkv, past, hd, prec, env)] -> [{kernel, ms, splits, tile}] of the attention step of each, one model after the other"""
    _setup()
    import kv_graphs as KG
    from engine_run import with_env
    from gpu_ai_inference_server_amd import binding as B
    from gpu_ai_inference_server_amd.modelgen import models
    out = []
    with tempfile.TemporaryDirectory() as root:
        for i, (n, h, hkv, past, hd, prec, env) in enumerate(configs):
            rows, feeds = KG.decode_feeds(n, h, hkv, hd, past, positions=[past] * n)
            path = models.write_repo(root, f"a{i}", KG.decode_attn_graph(rows, n, h, hkv, hd, past, max_pos=past + 1))

            def go():
                plan = B.DescribeModel(path, n)["plan"]
                (at,) = [s for s in plan["steps"] if s["kind"] == "attention"]
                m = B.CreateModel(path, f"a{i}")
                try:
                    din, _ = B.Prepare(m, [list(v.shape) for v in feeds.values()], 3)
                    for d, v in zip(din, feeds.values()):
                        B.CopyToDevice(m, d, v)
                    B.RunPrepared(m, 3, True)
                    (p,) = [p for p in B.Profile(m, 20) if "attention_decode" in p["kernel"]]
                    return {"kernel": p["kernel"], "ms": p["ms"], "splits": at.get("splits", 0), "tile": at["tile"]}
                finally:
                    m.Destroy()
            out.append(with_env(dict(IE_PRECISION=prec, IE_AUTOTUNE="0", **env), go))
    print(json.dumps(out))


def model_child(path, n, past, prec, tile, vocab, depth, hkv, hd):
    """child: llama_135m's decode graph -> {replay_ms, steps}"""
    _setup()
    import numpy as np
    from gpu_ai_inference_server_amd import binding as B
    os.environ.update(IE_PRECISION=prec, IE_AUTOTUNE="0", **({"IE_ATTN_TILE": tile} if tile else {}))
    r = np.random.RandomState(0)
    feeds = [r.randint(0, vocab, (n, 1)).astype(np.int64), np.ones((n, past + 1), np.int64), np.full((n, 1), past, np.int64)]
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
    for key, name in (("embed", "embed"), ("attention_decode", "attention (append + decode)"), ("kv_append", "attention (append + decode)"), ("rmsnorm", "rms norm"),
                      ("eltwise", "gated unit (eltwise)"), ("copy", "copy")):
        if k.startswith(key):
            return name
    return "Linears (1x1 convs, M = 8 rows)"


def main():
    _setup()
    from gpu_ai_inference_server_amd.modelgen import models
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "decode")
    os.makedirs(out_dir, exist_ok=True)
    me = os.path.abspath(__file__)
    lines = []
    sweep = (1, 2, 4, 8, 16, 32, 64)
    for n, h, hkv, past, hd in SHAPES:
        cache = 4.0 * n * hkv * hd * (2 * past + 2 * (past + 1))       # read past K, V + write present K, V
        for prec in ("fp32", "fp16"):
            cfg = [(n, h, hkv, past, hd, prec, {}), (n, h, hkv, past, hd, prec, {"IE_ATTN_TILE": "0"})] + [(n, h, hkv, past, hd, prec, {"IE_ATTN_SPLITS": str(s)}) for s in sweep]
            what = f"decode attention (N {n}, H {h} / {hkv}, P {past}, hd {hd}) {prec}"
            res = child([me, "--attn", json.dumps(cfg)], what)
            sdpa = child(["-c", TORCH_SDPA, json.dumps([n, h, hkv, past + 1, hd, prec])], f"torch SDPA for {what}")
            d, t0 = res[0], res[1]
            lines.append(f"{what}: cache traffic {cache / 1e6:.2f} MB")
            lines.append(f"  tile 4, S = {d['splits']} (the planner's): {d['ms'] * 1e3:8.1f} us = {cache / (d['ms'] * 1e-3) / 1e12:.2f} TB/s, {100 * cache / (d['ms'] * 1e-3) / COPY_RATE:.0f} % of the copy rate   [{d['kernel']}]")
            lines.append(f"  tile 0, the parts:                  {t0['ms'] * 1e3:8.1f} us ({t0['ms'] / d['ms']:.2f} x)   [{t0['kernel']}]")
            lines.append(f"  torch SDPA, one query, K / V expanded, no append, no rotation: {sdpa['ms'] * 1e3:8.1f} us ({sdpa['ms'] / d['ms']:.2f} x)")
            lines.append("  IE_ATTN_SPLITS sweep: " + ", ".join(f"S {r['splits']}: {r['ms'] * 1e3:.1f} us" for r in res[2:]))
            print("\n".join(lines[-5:]), flush=True)
    n, h, hkv, _, hd = SHAPES[0]
    lines.append(f"tile 4 (the planner's S) against the parts over the cache length, (N {n}, H {h} / {hkv}, hd {hd}):")
    for prec in ("fp32", "fp16"):
        pasts = (1, 15, 31, 63, 127, 255, 511)
        cfg = [(n, h, hkv, p, hd, prec, {"IE_ATTN_TILE": t}) for p in pasts for t in ("4", "0")]
        res = child([me, "--attn", json.dumps(cfg)], f"threshold sweep {prec}")
        for i, p in enumerate(pasts):
            a, b = res[2 * i], res[2 * i + 1]
            lines.append(f"  {prec} P {p:4d}: tile 4 (S {a['splits']}) {a['ms'] * 1e3:7.1f} us, parts {b['ms'] * 1e3:7.1f} us ({b['ms'] / a['ms']:.2f} x)")
    open(os.path.join(out_dir, "decode_attention.txt"), "w").write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)

    lines = []
    N, PAST, VOCAB, DEPTH, HKV, HD = 8, 1023, 49152, 30, 3, 64
    with tempfile.TemporaryDirectory() as root:
        path = models.write_repo(root, "llama_135m_decode", models.llama_135m(N, seq=1, past=PAST))
        for prec in ("fp32", "fp16"):
            for tile in ("", "0"):
                what = f"llama_135m decode step, batch {N}, P {PAST}, {prec}" + (", IE_ATTN_TILE=0" if tile else "")
                r = child([me, "--model", path, str(N), str(PAST), prec, tile, str(VOCAB), str(DEPTH), str(HKV), str(HD)], what)
                steps = r["steps"]
                total = sum(s[1] for s in steps)
                lines.append(f"{what}:")
                lines.append(f"  graph replay {r['replay_ms']:.3f} ms = {N / r['replay_ms'] * 1e3:.0f} tokens/s; eager sum of steps {total:.3f} ms over {len(steps)} steps")
                fam = {}
                for i, s in enumerate(steps):
                    e = fam.setdefault("the vocabulary head" if i == len(steps) - 1 else family(s[0]), [0, 0.0])
                    e[0] += 1
                    e[1] += s[1]
                for k, (cnt, ms) in sorted(fam.items(), key=lambda kv: -kv[1][1]):
                    lines.append(f"    {k:34s} {cnt:3d} steps {ms:9.3f} ms {100 * ms / total:5.1f} %")
                print("\n".join(lines[-8:]), flush=True)
    open(os.path.join(out_dir, "llama_135m_decode.txt"), "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--attn":
        attention_child(json.loads(sys.argv[2]))
    elif len(sys.argv) == 11 and sys.argv[1] == "--model":
        model_child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5], sys.argv[6], *(int(v) for v in sys.argv[7:11]))
    else:
        main()
