#!/usr/bin/env python3
"""Times of the 4-bit Linear kernels on the decoder Linear shapes of llama_3b_layers and llama_135m, fp16 precision.

    python scripts/qlinear_profile.py [--models 3b,135m] [--rows 1,8,16,64,1024] [--variants tile2,tile1,tile0,twin] [--rounds 5] [--iters 50]
                                      [--out profiles/qlinear/linears.txt]
    python scripts/qlinear_profile.py --forward llama_135m [--batch 8] [--seq 1024] [--rounds 5] [--iters 50] --out profiles/qlinear/prefill.txt

Per (shape, rows) one model of ONE Linear (modelgen.qlinear) per variant is loaded side by side: the MatMulNBits graph pinned to tile 2
(qlinear_gemm_kernel), to tile 1 (qlinear_mfma_kernel) and to tile 0 (qlinear_generic_kernel), and the dense twin, whose fp16 conv step is what the engine
ran before this kernel family.  A round profiles them one after the other (EngineProfile: an eager forward with device events around every launch,
averaged over --iters forwards after one warm-up profile); --rounds rounds alternate them, and the table gives the median and the (min .. max) spread of
each.  GB/s is the plan's algorithmic bytes of the step over the median time, against the 6.29 TB/s copy rate of DESIGN 2; TFLOP/s is 2 M K N over it.
The prefill row counts go to profiles/qlinear/prefill.txt with --variants tile2,tile1,twin: tile 0 takes seconds there.

--forward: one whole int4 prefill three ways -- the planner's default tiles, IE_QLINEAR_TILE=1, the dense twin -- as graph replays, alternating rounds
of --iters replays each, appended to --out with the qlinear (or, for the twin, conv) steps' share of an eager profile.
Needs a GPU; nothing is estimated without one."""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _pkg import load_package  # noqa: E402

load_package()
from gpu_ai_inference_server_amd import binding as B  # noqa: E402
from gpu_ai_inference_server_amd.modelgen import models  # noqa: E402

COPY_RATE = 6.29e12
# (K, N) of the merged qkv, o_proj, gate / up and down_proj
SHAPES = {"3b": ((3072, 5120), (3072, 3072), (3072, 8192), (8192, 3072)), "135m": ((576, 960), (576, 576), (576, 1536), (1536, 576))}


def codes(name, cout, nblk, block):
    """random codes, zero points and scales (the times do not depend on the values; drawing them skips the quantisation of 25 M weights)"""
    r = np.random.RandomState(cout + nblk)
    return (r.randint(0, 16, (cout, nblk, block)).astype(np.uint8), r.randint(0, 16, (cout, nblk)).astype(np.uint8),
            (np.float32(0.01) * np.exp2(r.uniform(0.0, 2.0, (cout, nblk)))).astype(np.float32))


def under(env, fn):
    """fn() with env set: the planner reads its switches whenever it builds a plan, at load and at the first request of a new row count"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def forward(a, emit, root):
    base = dict(IE_PRECISION="fp16", IE_AUTOTUNE="0")
    variants = (("default tiles", {"quant": "int4"}, {}), ("IE_QLINEAR_TILE=1", {"quant": "int4"}, {"IE_QLINEAR_TILE": "1"}), ("dense twin", {"quant": "int4", "q_form": "dense"}, {}))
    paths, loaded, ms, share = {}, {}, {}, {}
    vocab = 49152 if a.forward == "llama_135m" else 1024
    ids = np.random.RandomState(0).randint(0, vocab, size=(a.batch, a.seq)).astype(np.int64)
    for v, kw, env in variants:
        key = tuple(sorted(kw.items()))
        if key not in paths:
            paths[key] = models.write_repo(root, f"{a.forward}_{len(paths)}", getattr(models, a.forward)(a.batch, seq=a.seq, **kw))

        def load():
            m = B.CreateModel(paths[key], v)
            din, _ = B.Prepare(m, [[a.batch, a.seq]], 1)
            B.CopyToDevice(m, din[0], ids)
            B.RunPrepared(m, 3, True)      # warm-up
            return m
        loaded[v] = under(dict(base, **env), load)
    for _ in range(a.rounds):
        for v, _, env in variants:
            def run():
                t0 = time.perf_counter()
                B.RunPrepared(loaded[v], a.iters, True)
                return (time.perf_counter() - t0) * 1e3 / a.iters
            ms.setdefault(v, []).append(under(dict(base, **env), run))
    for v, _, env in variants:
        prof = under(dict(base, **env), lambda: B.Profile(loaded[v], 5))
        lin = [p for p in prof if ("qlinear" in p["kernel"] if v != "dense twin" else p["kernel"].startswith("conv"))]
        share[v] = (len(lin), sum(p["ms"] for p in lin), sum(p["ms"] for p in prof), sorted({p["kernel"].split("<")[0] for p in lin}))
    emit(f"# {a.forward} int4 prefill, batch {a.batch}, sequence {a.seq}, fp16 precision: {a.rounds} alternating rounds of {a.iters} graph replays; ms per replay = median (min .. max)")
    twin = statistics.median(ms["dense twin"])
    for v, _, _ in variants:
        med, (cnt, lin, total, names) = statistics.median(ms[v]), share[v]
        emit(f"{v:18s} {med:9.3f} ({min(ms[v]):.3f} .. {max(ms[v]):.3f}) ms, {med / twin:6.3f} of the twin | eager: {cnt} Linear steps ({', '.join(names)}) {lin:.3f} of {total:.3f} ms = {100 * lin / total:.1f} %")
    for m in loaded.values():
        m.Destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--forward", default="")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seq", type=int, default=1024)
    ap.add_argument("--variants", default="tile2,tile1,tile0,twin")
    ap.add_argument("--models", default="3b,135m")
    ap.add_argument("--rows", default="1,8,16,64,1024")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qlinear", "linears.txt"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    base = dict(IE_PRECISION="fp16", IE_AUTOTUNE="0")
    variants = tuple(v for v in (("tile2", "nbits", {"IE_QLINEAR_TILE": "2"}), ("tile1", "nbits", {"IE_QLINEAR_TILE": "1"}), ("tile0", "nbits", {"IE_QLINEAR_TILE": "0"}),
                                 ("twin", "dense", {})) if v[0] in a.variants.split(","))
    envs = {v: env for v, _, env in variants}
    with open(a.out, "a" if a.forward else "w") as out, tempfile.TemporaryDirectory() as root:
        def emit(line):
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()
        if a.forward:
            return forward(a, emit, root)
        emit(f"# one Linear, fp16 precision, block 32 with zero points; {a.rounds} alternating rounds of {a.iters} timed forwards; ms = median (min .. max); GB/s = algorithmic bytes / median")
        emit("# model  K     N     rows | kernel                                   ms                         GB/s   of 6.29 TB/s | TFLOP/s | ratio to the twin")
        for mname in a.models.split(","):
            for k, n in SHAPES[mname]:
                loaded = {}
                for v, form, env in variants:      # one model per variant with a dynamic row count: a plan instance per row count
                    path = models.write_repo(root, f"{mname}_{k}_{n}_{v}", models.qlinear("rows", k, n, q_form=form, q_codes=codes))
                    loaded[v] = under(dict(base, **env), lambda: B.CreateModel(path, v))
                for rows in (int(r) for r in a.rows.split(",")):
                    ms, info = {}, {}
                    x = np.random.RandomState(1).randn(rows, k).astype(np.float32)

                    def profile(v, iters):
                        return under(dict(base, **envs[v]), lambda: timed(v, iters))

                    def timed(v, iters):
                        # (the request makes the plan instance of this row count the model's current one, which EngineProfile times)
                        loaded[v].Infer([B.TensorData("x", B.DataTypeFloat32, B.Shape([rows, k]), x)], [B.OutputConfig("y", Shape=[rows, n], DataType="FLOAT32")])
                        return max((p for p in B.Profile(loaded[v], iters) if "qlinear" in p["kernel"] or "conv" in p["kernel"]), key=lambda p: p["bytes"])
                    for v, _, _ in variants:
                        profile(v, 3)      # warm-up
                    for _ in range(a.rounds):
                        for v, _, _ in variants:
                            info[v] = profile(v, a.iters)
                            ms.setdefault(v, []).append(info[v]["ms"])
                    twin = statistics.median(ms["twin"]) if "twin" in ms else float("nan")
                    for v, _, _ in variants:
                        med = statistics.median(ms[v])
                        rate = info[v]["bytes"] / (med * 1e-3)
                        emit(f"{mname:5s} {k:5d} {n:5d} {rows:5d} | {info[v]['kernel']:40s} {med:8.4f} ({min(ms[v]):.4f} .. {max(ms[v]):.4f})  {rate / 1e9:8.1f}  {100 * rate / COPY_RATE:5.1f} % | {2e-9 * rows * k * n / med:7.1f} | {med / twin:6.3f}")
                for m in loaded.values():
                    m.Destroy()


if __name__ == "__main__":
    main()
