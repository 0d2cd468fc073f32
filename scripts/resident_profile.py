#!/usr/bin/env python3
"""A resident KV cache against the client-held cache of the parent commit on one MI355X: what DESIGN 3.34 records.

    python scripts/resident_profile.py [--parent-lib <libinference_engine.so of a build of the parent commit>] [out_dir]     (default profiles/decode_resident)

Both builds run in the same session, each in child processes of its own (the library is chosen through INFERENCE_ENGINE_LIB); without --parent-lib the
parent's columns are left out.
* the decode attention step alone at DESIGN 3.32's three shapes, fp32 and fp16: the parent's tile 4, and the in-place tile 4 with len = P - 1 and len = P / 4
* the extend attention step alone at DESIGN 3.33's Lq = 4 and 128 rows: the parent's tile 5, and the in-place tile 5 with len = P - Lq
* llama_135m, batch 8, P = 1 023, fp32 and fp16: the wall time of a ModelInfer decode call (seconds inside the C call, binding.InferTimed) unbound on the
  parent build (every past tensor up, every present tensor down) and bound; the graph replay of the step (EngineRunPrepared) on both
Step times are HIP events around each launch (B.Profile, median of 20); wall times are medians of 20 with the spread (min .. max) beside them.  Every
group of measurements is a child process under its own time limit; the first one that fails ends the run."""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECODE_SHAPES = ((8, 9, 3, 1023, 64), (8, 24, 8, 1023, 128), (1, 32, 8, 4095, 128))
EXTEND_SHAPES = ((8, 9, 3, 1023, 64, 4), (8, 9, 3, 1023, 64, 128))
STEP_TIMEOUT = 600
LLAMA = dict(n=8, past=1023, vocab=49152, depth=30, hkv=3, hd=64)


def _setup():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _pkg import load_package
    load_package()


def _median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def attention_child(configs):
    """child: [(n, h, hkv, past, hd, lq, prec, len or None)] -> [{kernel, ms, samples}]: the attention step of each, unbound (len None) or bound to a cache whose
    images all hold len rows.  The step is profiled three times over (3 x median of 20): the spread of the three is the session's run-to-run spread"""
    _setup()
    import extend_graphs as EG
    import kv_graphs as KG
    from engine_run import with_env
    from gpu_ai_inference_server_amd import binding as B
    from gpu_ai_inference_server_amd.modelgen import models
    out = []
    with tempfile.TemporaryDirectory() as root:
        for i, (n, h, hkv, past, hd, lq, prec, ln) in enumerate(configs):
            valid = [past if ln is None else ln] * n
            if lq == 1:
                rows, feeds = KG.decode_feeds(n, h, hkv, hd, past, valid=valid, positions=valid)
                mb = KG.decode_attn_graph(rows, n, h, hkv, hd, past, max_pos=past + 1)
            else:
                rows, feeds = EG.extend_feeds(n, h, hkv, hd, past, lq, valid=valid, max_pos=past + lq)
                mb = EG.extend_attn_graph(rows, n, h, hkv, hd, past, lq, max_pos=past + lq)
            path = models.write_repo(root, f"a{i}", mb)

            def go():
                m = B.CreateModel(path, f"a{i}")
                kc = None
                try:
                    if ln is not None:
                        kc = B.KvCache(1, n, hkv, past, hd)
                        kc.bind(m)
                        kc.write(0, 0, feeds["past_key_values.0.key"])
                        kc.write(0, 1, feeds["past_key_values.0.value"])
                        kc.set_lengths(valid)
                    din, _ = B.Prepare(m, [list(v.shape) for v in feeds.values()], 3)
                    for d, (k, v) in zip(din, feeds.items()):
                        if ln is None or not k.startswith("past_key_values."):
                            B.CopyToDevice(m, d, v)
                    B.RunPrepared(m, 3, True)
                    samples = []
                    for _ in range(3):
                        (p,) = [p for p in B.Profile(m, 20) if "attention_decode" in p["kernel"] or "attention_extend" in p["kernel"]]
                        samples.append(p["ms"])
                    return {"kernel": p["kernel"], "ms": sorted(samples)[1], "samples": samples}
                finally:
                    if kc is not None:
                        kc.destroy()
                    m.Destroy()
            out.append(with_env(dict(IE_PRECISION=prec, IE_AUTOTUNE="0"), go))
    print(json.dumps(out))


def model_child(path, prec, bound):
    """child: llama_135m's decode graph -> {infer_ms: (median, min, max), replay_ms: (median, min, max)}; bound: to a cache whose images hold P - 1 rows"""
    _setup()
    import numpy as np
    from engine_run import tensor
    from gpu_ai_inference_server_amd import binding as B
    os.environ.update(IE_PRECISION=prec, IE_AUTOTUNE="0")
    n, past, vocab, depth, hkv, hd = (LLAMA[k] for k in ("n", "past", "vocab", "depth", "hkv", "hd"))
    r = np.random.RandomState(0)
    feeds = {"input_ids": r.randint(0, vocab, (n, 1)).astype(np.int64), "attention_mask": np.ones((n, past + 1), np.int64), "position_ids": np.full((n, 1), past - 1, np.int64)}
    feeds["attention_mask"][:, past - 1] = 0                    # every image holds P - 1 rows, so a bound call has room for its token
    cache = {f"past_key_values.{i}.{w}": r.randn(n, hkv, past, hd).astype(np.float32) for i in range(depth) for w in ("key", "value")}
    m = B.CreateModel(path, os.path.basename(path))
    kc = None
    try:
        outs = [B.OutputConfig("logits", Shape=[n, 1, vocab], DataType="FLOAT32")]
        if bound:
            kc = B.KvCache(depth, n, hkv, past, hd)
            kc.bind(m)
            for i in range(depth):
                kc.write(i, 0, cache[f"past_key_values.{i}.key"])
                kc.write(i, 1, cache[f"past_key_values.{i}.value"])
            ins = [tensor(k, v) for k, v in feeds.items()]
        else:
            ins = [tensor(k, v) for k, v in dict(feeds, **cache).items()]
            outs += [B.OutputConfig(f"present.{i}.{w}", Shape=[n, hkv, past + 1, hd], DataType="FLOAT32") for i in range(depth) for w in ("key", "value")]
        ts = []
        for it in range(22):
            if bound:
                kc.set_lengths([past - 1] * n)
            t = m.InferTimed(ins, outs, 1)[0]
            if it >= 2:
                ts.append(t * 1e3)
        if bound:
            kc.set_lengths([past - 1] * n)
        din, _ = B.Prepare(m, [list(v.shape) for v in dict(feeds, **cache).values()], 1 + 2 * depth)
        for d, (k, v) in zip(din, dict(feeds, **cache).items()):
            if not bound or not k.startswith("past_key_values."):
                B.CopyToDevice(m, d, v)
        B.RunPrepared(m, 3, True)
        rs = []
        for _ in range(20):
            t0 = time.perf_counter()
            B.RunPrepared(m, 1, True)
            rs.append((time.perf_counter() - t0) * 1e3)
        kern = sorted({p["kernel"] for p in B.Profile(m, 1) if "attention" in p["kernel"]})
    finally:
        if kc is not None:
            kc.destroy()
        m.Destroy()
    print(json.dumps({"infer_ms": _median(ts), "replay_ms": _median(rs), "attention": kern}))


def child(args, what, lib=None):
    env = dict(os.environ)
    if lib:
        env["INFERENCE_ENGINE_LIB"] = lib
    try:
        r = subprocess.run([sys.executable] + args, capture_output=True, text=True, timeout=STEP_TIMEOUT, env=env)
    except subprocess.TimeoutExpired:
        sys.exit(f"{what}: ran into its time limit; nothing further is started")
    if r.returncode != 0 or not r.stdout.strip():
        sys.exit(f"{what}: failed with status {r.returncode} (nothing further is started): " + " | ".join(r.stderr.strip().splitlines()[-3:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    _setup()
    from gpu_ai_inference_server_amd.modelgen import models
    args = sys.argv[1:]
    parent = None
    if args and args[0] == "--parent-lib":
        parent, args = os.path.abspath(args[1]), args[2:]
    out_dir = args[0] if args else os.path.join(ROOT, "profiles", "decode_resident")
    os.makedirs(out_dir, exist_ok=True)
    me = os.path.abspath(__file__)
    us = lambda r: f"{r['ms'] * 1e3:8.1f} us (three medians of 20: " + ", ".join(f"{s * 1e3:.1f}" for s in r["samples"]) + ")"      # noqa: E731

    lines = []
    for prec in ("fp32", "fp16"):
        mine = child([me, "--attn", json.dumps([(n, h, hkv, p, hd, 1, prec, ln) for n, h, hkv, p, hd in DECODE_SHAPES for ln in (None, p - 1, p // 4)])], f"decode attention {prec}")
        theirs = child([me, "--attn", json.dumps([(n, h, hkv, p, hd, 1, prec, None) for n, h, hkv, p, hd in DECODE_SHAPES])], f"decode attention {prec}, parent build", parent) if parent else None
        for i, (n, h, hkv, p, hd) in enumerate(DECODE_SHAPES):
            lines.append(f"decode attention (N {n}, H {h} / {hkv}, P {p}, hd {hd}) {prec}:")
            if theirs:
                lines.append(f"  parent build, tile 4 (client-held cache)   {us(theirs[i])}   [{theirs[i]['kernel']}]")
            a, b, c = mine[3 * i:3 * i + 3]
            lines.append(f"  this build, unbound tile 4                 {us(a)}   [{a['kernel']}]")
            lines.append(f"  in place, len = P - 1 = {p - 1:5d}              {us(b)}   [{b['kernel']}]")
            lines.append(f"  in place, len = P / 4 = {p // 4:5d}              {us(c)}")
        print("\n".join(lines[-5 * len(DECODE_SHAPES):]), flush=True)
    for prec in ("fp32", "fp16"):
        mine = child([me, "--attn", json.dumps([(n, h, hkv, p, hd, lq, prec, ln) for n, h, hkv, p, hd, lq in EXTEND_SHAPES for ln in (None, p - lq)])], f"extend attention {prec}")
        theirs = child([me, "--attn", json.dumps([(n, h, hkv, p, hd, lq, prec, None) for n, h, hkv, p, hd, lq in EXTEND_SHAPES])], f"extend attention {prec}, parent build", parent) if parent else None
        for i, (n, h, hkv, p, hd, lq) in enumerate(EXTEND_SHAPES):
            lines.append(f"extend attention (N {n}, H {h} / {hkv}, P {p}, hd {hd}, Lq {lq}) {prec}:")
            if theirs:
                lines.append(f"  parent build, tile 5 (client-held cache)   {us(theirs[i])}   [{theirs[i]['kernel']}]")
            a, b = mine[2 * i:2 * i + 2]
            lines.append(f"  this build, unbound tile 5                 {us(a)}   [{a['kernel']}]")
            lines.append(f"  in place, len = P - Lq = {p - lq:5d}             {us(b)}   [{b['kernel']}]")
        print("\n".join(lines[-4 * len(EXTEND_SHAPES):]), flush=True)
    open(os.path.join(out_dir, "resident_attention.txt"), "w").write("\n".join(lines) + "\n")

    lines = []
    ms = lambda t: f"{t[0]:9.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"      # noqa: E731
    with tempfile.TemporaryDirectory() as root:
        path = models.write_repo(root, "llama_135m_decode", models.llama_135m(LLAMA["n"], seq=1, past=LLAMA["past"]))
        for prec in ("fp32", "fp16"):
            what = f"llama_135m decode step, batch {LLAMA['n']}, P {LLAMA['past']}, {prec}"
            b = child([me, "--model", path, prec, "bound"], what + ", bound")
            u = child([me, "--model", path, prec, "unbound"], what + ", unbound on the parent build", parent) if parent else None
            lines.append(what + ":")
            if u:
                lines.append(f"  parent build, client-held cache:  ModelInfer {ms(u['infer_ms'])}   graph replay {ms(u['replay_ms'])}   {u['attention']}")
            lines.append(f"  bound to a resident cache:        ModelInfer {ms(b['infer_ms'])}   graph replay {ms(b['replay_ms'])}   {b['attention']}")
            print("\n".join(lines[-3:]), flush=True)
    open(os.path.join(out_dir, "llama_135m_resident.txt"), "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--attn":
        attention_child(json.loads(sys.argv[2]))
    elif len(sys.argv) == 5 and sys.argv[1] == "--model":
        model_child(sys.argv[2], sys.argv[3], sys.argv[4] == "bound")
    else:
        main()
