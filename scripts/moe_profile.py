#!/usr/bin/env python3
"""Times of the mixture-of-experts step alone, fp16 precision, D = 2048, I = 4096, k = 2.

    python scripts/moe_profile.py [--rows 1,8,64] [--experts 8,16] [--variants default,dense] [--rounds 5] [--iters 50] [--out profiles/moe/step.txt]
    python scripts/moe_profile.py --rows 256,1024,4096,8192 --variants tile2,tile1,dense --out profiles/moe/prefill.txt      

One model of ONE node (modelgen.moe, gated silu, normalised) per expert count and the dense fp16 SwiGLU MLP of the same D and I -- what one expert costs
today: three conv steps and the gated eltwise step -- are loaded side by side.  --variants: default = the planner's tile, tile2 / tile1 / tile0 = the
same model loaded once more under that IE_MOE_TILE pin (the planner reads it whenever it builds a plan: at load and at the first request of a row count).  A round profiles them one after the other (EngineProfile: an eager forward
with device events around every step, averaged over --iters forwards after one warm-up profile); --rounds rounds alternate them, and the table gives the
median and the (min .. max) spread of each.  The rate is the bytes of the half weights of the experts the router rows choose over the median time, against the
6.29 TB/s copy rate of DESIGN 2.  The router rows are random permutations, so the tokens of a batch choose different experts.
TFLOP/s is 2 rows k 3 D I over the median (the dense MLP: 2 rows 3 D I).
A layer of Mixtral's own size (D 4096, I 14336, E 8) does not fit protobuf's 2 GB.  Needs a GPU; nothing is estimated without one."""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _pkg import load_package  # noqa: E402

load_package()
from gpu_ai_inference_server_amd import binding as B  # noqa: E402
from gpu_ai_inference_server_amd.modelgen import models  # noqa: E402

COPY_RATE = 6.29e12
D, I, K = 2048, 4096, 2


def dense_mlp() -> bytes:
    """x [rows, D] -> down(SiLU(gate(x)) * up(x)) between Muls by 1: the MLP of a dense Llama layer of this size"""
    gb = models.GraphBuilder("mlp", 12)
    one = gb.init("one", np.array(1.0, np.float32))
    h = gb.simple("Mul", ["x", one])
    y = gb.swiglu(gb.linear(h, D, I, name="gate", bias=False), gb.linear(h, D, I, name="up", bias=False))
    gb.simple("Mul", [gb.linear(y, I, D, name="down", bias=False), one], out="y")
    return gb.finish([("x", ["rows", D])], [("y", ["rows", D])], opset=18)


def under(env, fn):
    """fn() with env set"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1,8,64")
    ap.add_argument("--experts", default="8,16")
    ap.add_argument("--variants", default="default,dense")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moe", "step.txt"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    os.environ.update(IE_PRECISION="fp16", IE_AUTOTUNE="0")
    experts = [int(e) for e in a.experts.split(",")]
    pins = {v: ({} if v == "default" else {"IE_MOE_TILE": v[4:]}) for v in a.variants.split(",") if v != "dense"}

    def label(v, e):
        return f"{'moe' if v == 'default' else v} E={e}"
    with open(a.out, "w") as out, tempfile.TemporaryDirectory() as root:
        def emit(line):
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()
        loaded = {}
        for e in experts:      # (the times do not depend on the values: uniform draws skip the Gaussian transform of 400 M weights)
            r = np.random.RandomState(e)
            w = {k: (r.random_sample(s).astype(np.float32) - np.float32(0.5)) * np.float32(0.05) for k, s in (("fc1", (e, D, I)), ("fc2", (e, I, D)), ("fc3", (e, D, I)))}
            path = models.write_repo(root, f"moe{e}", models.moe("rows", D, I, e, K, weights=w))
            del w
            for v, env in pins.items():
                loaded[label(v, e)] = under(env, lambda: B.CreateModel(path, f"moe{e}"))
        envs = {label(v, e): env for e in experts for v, env in pins.items()}
        if "dense" in a.variants.split(","):
            loaded["dense MLP"] = B.CreateModel(models.write_repo(root, "mlp", dense_mlp()), "mlp")
            envs["dense MLP"] = {}
        emit(f"# the moe step alone, fp16 precision, D {D}, I {I}, k {K}, gated silu; {a.rounds} alternating rounds of {a.iters} timed forwards; ms = median (min .. max)")
        emit("# rows | model      kernel(s)                                   ms                          active GB    GB/s  of 6.29 TB/s | TFLOP/s")
        for rows in (int(v) for v in a.rows.split(",")):
            x = np.random.RandomState(rows).randn(rows, D).astype(np.float32)
            ms, info = {}, {}
            routers = {e: np.stack([np.random.RandomState(t).permutation(e) for t in range(rows)]).astype(np.float32) / 8 for e in experts}

            def timed(name, iters):
                return under(envs[name], lambda: timed_pinned(name, iters))

            def timed_pinned(name, iters):
                # (the request makes the plan instance of this row count the model's current one, which EngineProfile times)
                feeds = [B.TensorData("x", B.DataTypeFloat32, B.Shape([rows, D]), x)]
                if name != "dense MLP":
                    e = int(name.split("=")[1])
                    feeds.append(B.TensorData("router", B.DataTypeFloat32, B.Shape([rows, e]), routers[e]))
                loaded[name].Infer(feeds, [B.OutputConfig("y", Shape=[rows, D], DataType="FLOAT32")])
                prof = B.Profile(loaded[name], iters)
                steps = [p for p in prof if "moe_" in p["kernel"]] if name != "dense MLP" else prof[1:]      # (without the Mul by 1 in front of the MLP; the one behind it folds into down's epilogue)
                return sum(p["ms"] for p in steps), " + ".join(p["kernel"].split("<")[0] for p in steps)
            for name in loaded:
                timed(name, 3)      # warm-up
            for _ in range(a.rounds):
                for name in loaded:
                    info[name] = timed(name, a.iters)
                    ms.setdefault(name, []).append(info[name][0])
            for name in loaded:
                med = statistics.median(ms[name])
                # (the experts these router rows really choose: fewer than min(E, rows * k) where tokens agree)
                active = len(set(np.argsort(-routers[int(name.split("=")[1])], axis=-1, kind="stable")[:, :K].ravel().tolist())) if name != "dense MLP" else 1
                gb = active * 3 * D * I * 2 / 1e9
                tf = 2e-9 * rows * (K if name != "dense MLP" else 1) * 3 * D * I / med
                emit(f"{rows:6d} | {name:10s} {info[name][1]:42s} {med:8.4f} ({min(ms[name]):.4f} .. {max(ms[name]):.4f})  {gb:8.3f}  {gb / (med * 1e-3):7.1f}  {100 * gb * 1e9 / (med * 1e-3) / COPY_RATE:5.1f} % | {tf:7.1f}")
            for v in pins if len(experts) >= 2 else ():
                lo, hi = (label(v, e) for e in (min(experts), max(experts)))
                d = statistics.median(ms[hi]) - statistics.median(ms[lo])
                spread = max(max(ms[n]) - min(ms[n]) for n in (lo, hi))
                emit(f"#      rows {rows}: {hi} - {lo} = {d:+.4f} ms, recorded spread {spread:.4f} ms" + (": within the spread" if d <= spread else ": ABOVE the spread"))
            for e in experts if "tile2" in pins and "tile1" in pins else ():      # (the planner's threshold, DESIGN 3.41: tile 2 below tile 1 by more than both spreads)
                t2, t1 = ms[label("tile2", e)], ms[label("tile1", e)]
                d = statistics.median(t1) - statistics.median(t2)
                spread = max(max(t2) - min(t2), max(t1) - min(t1))
                emit(f"#      rows {rows}, E={e} ({rows * K / e:g} mean rows per expert): tile1 - tile2 = {d:+.4f} ms, larger spread {spread:.4f} ms: tile 2 " + ("wins" if d > spread else "does not win"))
        for m in loaded.values():
            m.Destroy()


if __name__ == "__main__":
    main()
