#!/usr/bin/env python3
"""Per-step timing table of a plan (HIP events around each launch, eager mode).

    python scripts/profile_steps.py [batch] [model]      model: a bench.py model (densenet121, resnet50) or any other modelgen builder
                                                          (mobilenet_v2, mobilenet_v3_large, mobilenet_v3_small, efficientnet_b0), written to
                                                          its own repository under IE_BENCH_MODEL_ROOT

For a graph with depthwise convolutions it also prints the device-resident graph-replay time of the whole forward, the algorithmic GB/s of
every depthwise step against the 6.29 TB/s measured copy rate, and torch's own F.conv2d(groups=C) on channels_last tensors for the same
shapes as a yardstick (IE_PRECISION=fp16: half tensors).  For squeeze-excite steps likewise: their share of the eager forward, their algorithmic
GB/s (the input read twice, the output written once) and torch's mean + two 1x1 convs + sigmoid + mul on channels_last tensors per SE shape.
For grouped convolutions (resnext50_32x4d, regnet_y_400mf, regnet_x_400mf; run with IE_GROUPED_CONV=1): every grouped step's algorithmic GB/s, its roofline
max(bytes / 6.29 TB/s, FLOPs / peak) with peak = 157.3 TF (fp32) or 2.5 PF (fp16), the fraction of that roofline the step reaches, and torch's
F.conv2d(groups=g) on channels_last tensors for the same shape.
For transposed convolutions (unet): the graph-replay time as the median of 50 single replays, the transposed steps' share of the eager forward,
and per step the launched kernel (IE_FORCE_TILE=0 / 1 / 2 picks the generic kernel / the MFMA tiles), its algorithmic TB/s against the copy
rate, its roofline and torch's F.conv_transpose2d on channels_last tensors for the same shape.
For layer-norm steps (convnext_tiny): their share of the eager forward, next to the depthwise, the GELU (eltwise) and the remaining steps' shares, and
per distinct shape the launched kernel and its algorithmic GB/s (one read + one write) against the copy rate.
For attention steps (vit_b_16, vit_tiny_16): the graph-replay time as the median of 50 single replays, the share of the eager forward per step family
(attention, the qkv / proj / MLP convs, layer norms, GELU, token assemble), and per distinct attention shape the launched kernel
(IE_FORCE_TILE=0 picks the generic one), its microseconds, its TFLOP/s against the sustained MFMA rate (129 TF/s fp32) and torch's
F.scaled_dot_product_attention on the same [N, H, L, hd] operands, timed in a process of its own.
For window-attention steps (swin_t): the graph-replay time, the share of the eager forward per step family, and per distinct window-attention and
patch-merge shape the launched kernel with its algorithmic TB/s next to the 3.6 TB/s that layernorm_kernel sustains.
For group-norm steps (vae_decoder, resnet50_gn): their share and the attention steps' share of the eager forward, the time per image, and per distinct
shape the launched kernels and their algorithmic TB/s (one read + one write) against the copy rate."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _pkg import load_package  # noqa: E402

load_package()
import numpy as np  # noqa: E402
from gpu_ai_inference_server_amd import binding as B  # noqa: E402
from gpu_ai_inference_server_amd.modelgen import models  # noqa: E402

sys.path.insert(0, ROOT)
import bench  # noqa: E402

# F.conv2d(groups=C) on channels_last tensors, ms per call (20 timed calls after 5 warm ones) for each [n, c, h, w, k, stride, pad]
TORCH_DW = """
import json, sys, torch
import torch.nn.functional as F
dt = torch.float16 if sys.argv[2] == "fp16" else torch.float32
out = []
for n, c, h, w, k, st, pd in json.loads(sys.argv[1]):
    x = torch.randn(n, c, h, w, device="cuda", dtype=dt).to(memory_format=torch.channels_last)
    wt = torch.randn(c, 1, k, k, device="cuda", dtype=dt)
    b = torch.randn(c, device="cuda", dtype=dt)
    f = lambda: F.conv2d(x, wt, b, stride=st, padding=pd, groups=c)
    for _ in range(5):
        f()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        f()
    e1.record()
    torch.cuda.synchronize()
    out.append(e0.elapsed_time(e1) / 20)
print(json.dumps(out))
"""

# F.conv2d(groups=g) on channels_last tensors, ms per call (20 timed calls after 5 warm ones) for each [n, cin, h, w, cout, g, k, stride, pad]
TORCH_GROUPED = """
import json, sys, torch
import torch.nn.functional as F
dt = torch.float16 if sys.argv[2] == "fp16" else torch.float32
out = []
for n, c, h, w, co, g, k, st, pd in json.loads(sys.argv[1]):
    x = torch.randn(n, c, h, w, device="cuda", dtype=dt).to(memory_format=torch.channels_last)
    wt = torch.randn(co, c // g, k, k, device="cuda", dtype=dt).to(memory_format=torch.channels_last)
    b = torch.randn(co, device="cuda", dtype=dt)
    f = lambda: F.conv2d(x, wt, b, stride=st, padding=pd, groups=g)
    for _ in range(5):
        f()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        f()
    e1.record()
    torch.cuda.synchronize()
    out.append(e0.elapsed_time(e1) / 20)
print(json.dumps(out))
"""

# F.conv_transpose2d on channels_last tensors, ms per call (median of 20 timed calls after 5 warm ones) for each
# [n, cin, h, w, cout, kh, kw, sh, sw, pad_h, pad_w, op_h, op_w]
TORCH_CONVT = """
import json, sys, torch
import torch.nn.functional as F
dt = torch.float16 if sys.argv[2] == "fp16" else torch.float32
out = []
for n, c, h, w, co, kh, kw, sh, sw, ph, pw, oh, ow in json.loads(sys.argv[1]):
    x = torch.randn(n, c, h, w, device="cuda", dtype=dt).to(memory_format=torch.channels_last)
    wt = torch.randn(c, co, kh, kw, device="cuda", dtype=dt).to(memory_format=torch.channels_last)
    b = torch.randn(co, device="cuda", dtype=dt)
    f = lambda: torch.relu_(F.conv_transpose2d(x, wt, b, stride=(sh, sw), padding=(ph, pw), output_padding=(oh, ow)))
    for _ in range(5):
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

# torch's SE: mean over H, W -> 1x1 conv (+bias) -> ReLU -> 1x1 conv (+bias) -> sigmoid -> x * gate, for each [n, c, h, w, mid]
TORCH_SE = """
import json, sys, torch
import torch.nn.functional as F
dt = torch.float16 if sys.argv[2] == "fp16" else torch.float32
out = []
for n, c, h, w, mid in json.loads(sys.argv[1]):
    x = torch.randn(n, c, h, w, device="cuda", dtype=dt).to(memory_format=torch.channels_last)
    w1, b1 = torch.randn(mid, c, 1, 1, device="cuda", dtype=dt), torch.randn(mid, device="cuda", dtype=dt)
    w2, b2 = torch.randn(c, mid, 1, 1, device="cuda", dtype=dt), torch.randn(c, device="cuda", dtype=dt)
    f = lambda: x * torch.sigmoid(F.conv2d(torch.relu(F.conv2d(x.mean((2, 3), keepdim=True), w1, b1)), w2, b2))
    for _ in range(5):
        f()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        f()
    e1.record()
    torch.cuda.synchronize()
    out.append(e0.elapsed_time(e1) / 20)
print(json.dumps(out))
"""
# F.scaled_dot_product_attention, ms per call (median of 20 timed calls after 5 warm ones) for each [n, heads, l, hd]
TORCH_SDPA = """
import json, sys, torch
import torch.nn.functional as F
dt = torch.float16 if sys.argv[2] == "fp16" else torch.float32
out = []
for n, h, l, hd in json.loads(sys.argv[1]):
    q, k, v = (torch.randn(n, h, l, hd, device="cuda", dtype=dt) for _ in range(3))
    f = lambda: F.scaled_dot_product_attention(q, k, v)
    for _ in range(5):
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
BUILDERS = {"mobilenet_v3_large": lambda: models.mobilenet_v3("N", variant="large"), "mobilenet_v3_small": lambda: models.mobilenet_v3("N", variant="small")}

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 32
model_name = sys.argv[2] if len(sys.argv) > 2 else "densenet121"
if model_name in bench.MODELS:
    mdir = bench.model_dir(model_name)
else:
    root = os.environ.get("IE_BENCH_MODEL_ROOT", "/tmp/ie_bench_models")
    mdir = os.path.join(root, model_name, "1")
    if not os.path.exists(os.path.join(mdir, "model.onnx")):
        models.write_repo(root, model_name, BUILDERS[model_name]() if model_name in BUILDERS else getattr(models, model_name)("N"))
plan = B.DescribeModel(mdir, batch)["plan"]
m = B.CreateModel(mdir, os.path.basename(os.path.dirname(mdir)))
ishape = plan["inputs"][0]["dims"]          # [batch, 3, 224, 224] for the classifiers; the VAE decoder reads latents [batch, 4, 32, 32]
din, dout = B.Prepare(m, [ishape], 1)
B.CopyToDevice(m, din[0], models.synthetic_input(tuple(ishape), stream="prof"))
B.RunPrepared(m, 5, True)
# per step the median over the passes (50 for a graph with transposed convs: its table is what DESIGN 3.21 records)
prof = B.Profile(m, 50 if any(s.get("algo") == "transposed" for s in plan["steps"]) else 10)
tot = sum(p["ms"] for p in prof)
print(f"# batch {batch}: eager forward {tot:.3f} ms, {sum(p['flops'] for p in prof)/tot/1e9:.1f} TFLOP/s overall")
print(f"{'idx':>3} {'kernel':34} {'M':>7} {'N':>5} {'K':>5} {'ms':>8} {'TF/s':>7} {'GB/s':>7}  name")
for i, (p, s) in enumerate(zip(prof, plan["steps"])):
    M = s["out"]["n"] * s["out"]["h"] * s["out"]["w"]
    K = s["k"][0] * s["k"][1] * s["in"]["c"]
    print(f"{i:3d} {p['kernel']:34} {M:7d} {s['out']['c']:5d} {K:5d} {p['ms']:8.4f} {p['flops']/p['ms']/1e9:7.2f} {p['bytes']/p['ms']/1e6:7.0f}  {p['name'][:40]}")

dws = [(p, s) for p, s in zip(prof, plan["steps"]) if s.get("algo") == "depthwise"]
ses = [(p, s) for p, s in zip(prof, plan["steps"]) if s["kind"] == "squeeze_excite"]
grs = [(p, s) for p, s in zip(prof, plan["steps"]) if s.get("algo") == "grouped"]
cts = [(p, s) for p, s in zip(prof, plan["steps"]) if s.get("algo") == "transposed"]
if cts:
    import time
    B.RunPrepared(m, 10, True)
    ts = []
    for _ in range(50):
        t0 = time.perf_counter()
        B.RunPrepared(m, 1, True)
        ts.append((time.perf_counter() - t0) * 1e3)
    ms = sorted(ts)[len(ts) // 2]
    print(json.dumps({"model": model_name, "batch": batch, "precision": plan["precision"], "replay_ms_per_step_median50": round(ms, 4),
                      "images_per_s": round(batch / ms * 1e3, 1), "force_tile": os.environ.get("IE_FORCE_TILE")}))
    peak_tf = 2500.0 if plan["precision"] == "fp16" else 157.3
    c_ms = sum(p["ms"] for p, _ in cts)
    print(f"# {len(cts)} transposed steps: {c_ms:.4f} ms, {c_ms / tot * 100:.1f}% of the eager forward; roofline peak {peak_tf} TF/s, 6.29 TB/s")
    # (torch takes symmetric pads only: a step with asymmetric pads is timed with its top / left pads)
    shapes = [[s["in"]["n"], s["in"]["c"], s["in"]["h"], s["in"]["w"], s["out"]["c"], *s["k"], *s["stride"], s["pads"][0], s["pads"][1], *s["output_padding"]]
              for _, s in cts]
    tms = [float("nan")] * len(cts)
    if not os.environ.get("PROFILE_NO_TORCH"):            # (set it for the forced-tile passes of one session: torch's time does not depend on our tile)
        child = subprocess.run([sys.executable, "-c", TORCH_CONVT, json.dumps(shapes), plan["precision"]], capture_output=True, text=True, timeout=300)
        if child.returncode == 0:
            tms = json.loads(child.stdout.strip().splitlines()[-1])
        else:
            print("# torch yardstick failed:", child.stderr.strip().splitlines()[-1:])
    print(f"{'transposed step':16} {'kernel':30} {'HxWxCin->Cout':>20} {'k/s':>5} {'ms':>8} {'TB/s':>6} {'%6.29T':>7} {'roof ms':>8} {'%roof':>6} {'torch ms':>9}")
    for (p, s), t in zip(cts, tms):
        tbs = p["bytes"] / p["ms"] / 1e9
        roof = max(p["bytes"] / 6.29e9, p["flops"] / (peak_tf * 1e9))
        shape = f"{s['in']['h']}x{s['in']['w']}x{s['in']['c']}->{s['out']['c']}"
        ks = f"{s['k'][0]}/{s['stride'][0]}"
        print(f"{p['name'][:16]:16} {p['kernel'][:30]:30} {shape:>20} {ks:>5} {p['ms']:8.4f} {tbs:6.2f} {tbs / 6.29 * 100:6.1f}% {roof:8.4f} {roof / p['ms'] * 100:5.1f}% {t:9.4f}")
lns = [(p, s) for p, s in zip(prof, plan["steps"]) if s["kind"] == "layer_norm"]
if lns:
    share = lambda ps: sum(p["ms"] for p, _ in ps)  # noqa: E731
    elt = [(p, s) for p, s in zip(prof, plan["steps"]) if s["kind"] == "eltwise"]
    print(f"# {len(lns)} layer-norm steps: {share(lns):.4f} ms, {share(lns) / tot * 100:.1f}% of the eager forward; {len(dws)} depthwise steps: {share(dws):.4f} ms, "
          f"{share(dws) / tot * 100:.1f}%; {len(elt)} eltwise steps: {share(elt):.4f} ms, {share(elt) / tot * 100:.1f}%; the other steps: "
          f"{tot - share(lns) - share(dws) - share(elt):.4f} ms")
    print(f"{'layer-norm shape':>16} {'steps':>5} {'kernel':28} {'ms (median)':>11} {'GB/s':>7} {'%6.29T':>7}")
    seen = {}
    for p, s in lns:
        seen.setdefault((s["in"]["h"], s["in"]["w"], s["in"]["c"], p["kernel"]), []).append(p)
    for (h, w, c, kern), ps in seen.items():
        ms = sorted(q["ms"] for q in ps)[len(ps) // 2]
        gbs = ps[0]["bytes"] / ms / 1e6
        print(f"{f'{h}x{w}x{c}':>16} {len(ps):5d} {kern:28} {ms:11.4f} {gbs:7.0f} {gbs / 6290 * 100:6.1f}%")
ats = [(p, s) for p, s in zip(prof, plan["steps"]) if s["kind"] == "attention"]
if ats:
    import time
    B.RunPrepared(m, 10, True)
    ts = []
    for _ in range(50):
        t0 = time.perf_counter()
        B.RunPrepared(m, 1, True)
        ts.append((time.perf_counter() - t0) * 1e3)
    ms = sorted(ts)[len(ts) // 2]
    print(json.dumps({"model": model_name, "batch": batch, "precision": plan["precision"], "replay_ms_per_step_median50": round(ms, 4),
                      "images_per_s": round(batch / ms * 1e3, 1), "force_tile": os.environ.get("IE_FORCE_TILE")}))
    # a layer's convs by position: the one in front of the attention step is qkv, the three behind it proj, fc1 and fc2; the first conv of the
    # graph is the patch embedding, the last the head
    kinds = [s["kind"] for s in plan["steps"]]
    convs = [i for i, k in enumerate(kinds) if k == "conv"]
    role = {convs[0]: "conv patch", convs[-1]: "conv head"}
    for i, k in enumerate(kinds):
        if k == "attention":
            role[max(c for c in convs if c < i)] = "conv qkv"
            for c, tag in zip([c for c in convs if c > i][:3], ("conv proj", "conv fc1", "conv fc2")):
                role[c] = tag
    fam = {}
    for i, (p, s) in enumerate(zip(prof, plan["steps"])):
        fam.setdefault(role.get(i, "conv other") if s["kind"] == "conv" else s["kind"], []).append(p["ms"])
    print(f"{'family':16} {'steps':>5} {'ms':>9} {'share':>7}")
    for key, v in sorted(fam.items(), key=lambda kv: -sum(kv[1])):
        print(f"{key:16} {len(v):5d} {sum(v):9.4f} {sum(v) / tot * 100:6.1f}%")
    mfma_tf = 129.0 if plan["precision"] == "fp32" else 2500.0          # fp32: the measured sustained rate; fp16: the roofline peak used above
    seen = {}
    for p, s in ats:
        seen.setdefault((s["in"]["n"], s["heads"], s["in"]["w"], s["head_dim"], p["kernel"]), []).append(p)
    tms = [float("nan")] * len(seen)
    if not os.environ.get("PROFILE_NO_TORCH"):
        child = subprocess.run([sys.executable, "-c", TORCH_SDPA, json.dumps([list(k[:4]) for k in seen]), plan["precision"]], capture_output=True, text=True, timeout=300)
        if child.returncode == 0:
            tms = json.loads(child.stdout.strip().splitlines()[-1])
        else:
            print("# torch yardstick failed:", child.stderr.strip().splitlines()[-1:])
    print(f"{'attention N,H,L,hd':>20} {'steps':>5} {'kernel':30} {'us (median)':>11} {'TF/s':>7} {'%' + str(mfma_tf) + 'T':>8} {'torch sdpa us':>13}")
    for ((n, h, l, hd, kern), ps), t in zip(seen.items(), tms):
        ms = sorted(q["ms"] for q in ps)[len(ps) // 2]
        tf = ps[0]["flops"] / ms / 1e9
        print(f"{f'{n},{h},{l},{hd}':>20} {len(ps):5d} {kern:30} {ms * 1e3:11.1f} {tf:7.2f} {tf / mfma_tf * 100:7.1f}% {t * 1e3:13.1f}")
wts = [(p, s) for p, s in zip(prof, plan["steps"]) if s["kind"] == "window_attention"]
if wts:
    import time
    B.RunPrepared(m, 10, True)
    ts = []
    for _ in range(50):
        t0 = time.perf_counter()
        B.RunPrepared(m, 1, True)
        ts.append((time.perf_counter() - t0) * 1e3)
    ms = sorted(ts)[len(ts) // 2]
    print(json.dumps({"model": model_name, "batch": batch, "precision": plan["precision"], "replay_ms_per_step_median50": round(ms, 4),
                      "images_per_s": round(batch / ms * 1e3, 1), "force_tile": os.environ.get("IE_FORCE_TILE")}))
    # a block's convs by position: the one in front of the window_attention step is qkv, the three behind it proj, fc1 and fc2; the conv behind a
    # patch_merge (and its layer norm) is the reduction; the first conv of the graph is the patch embedding, the last the head
    kinds = [s["kind"] for s in plan["steps"]]
    convs = [i for i, k in enumerate(kinds) if k == "conv"]
    role = {convs[0]: "conv patch", convs[-1]: "conv head"}
    for i, k in enumerate(kinds):
        if k == "window_attention":
            role[max(c for c in convs if c < i)] = "conv qkv"
            for c, tag in zip([c for c in convs if c > i][:3], ("conv proj", "conv fc1", "conv fc2")):
                role[c] = tag
        if k == "patch_merge":
            role[min(c for c in convs if c > i)] = "conv reduction"
    fam = {}
    for i, (p, s) in enumerate(zip(prof, plan["steps"])):
        fam.setdefault(role.get(i, "conv other") if s["kind"] == "conv" else s["kind"], []).append(p["ms"])
    print(f"{'family':16} {'steps':>5} {'ms':>9} {'share':>7}")
    for key, v in sorted(fam.items(), key=lambda kv: -sum(kv[1])):
        print(f"{key:16} {len(v):5d} {sum(v):9.4f} {sum(v) / tot * 100:6.1f}%")
    # the step is bandwidth-bound: its roofline is its bytes at the rate layernorm_kernel sustains (3.6 TB/s)
    seen = {}
    for p, s in wts + [(p, s) for p, s in zip(prof, plan["steps"]) if s["kind"] == "patch_merge"]:
        key = (s["kind"], s["in"]["n"], s["in"]["h"], s["in"]["w"], s.get("heads", 0), tuple(s.get("shift", ())), p["kernel"])
        seen.setdefault(key, []).append(p)
    print(f"{'step N,HxW,heads,shift':>44} {'steps':>5} {'kernel':40} {'us (median)':>11} {'TB/s':>6} {'%3.6T':>6}")
    for (kind, n, h, w, heads, shift, kern), ps in seen.items():
        ms = sorted(q["ms"] for q in ps)[len(ps) // 2]
        tbs = ps[0]["bytes"] / ms / 1e9
        print(f"{f'{kind} {n},{h}x{w},{heads},{list(shift)}':>44} {len(ps):5d} {kern:40} {ms * 1e3:11.1f} {tbs:6.2f} {tbs / 3.6 * 100:5.1f}%")
gns = [(p, s) for p, s in zip(prof, plan["steps"]) if s["kind"] == "group_norm"]
if gns:
    share = lambda ps: sum(p["ms"] for p, _ in ps)  # noqa: E731
    ats = [(p, s) for p, s in zip(prof, plan["steps"]) if s["kind"] == "attention"]
    print(f"# {len(gns)} group-norm steps: {share(gns):.4f} ms, {share(gns) / tot * 100:.1f}% of the eager forward ({tot / batch:.4f} ms per image); "
          f"{len(ats)} attention steps ({', '.join(sorted(set(p['kernel'] for p, _ in ats))) or '-'}): {share(ats):.4f} ms, {share(ats) / tot * 100:.1f}%")
    print(f"{'group-norm shape':>18} {'steps':>5} {'kernel':68} {'ms (median)':>11} {'TB/s':>6} {'%6.29T':>7}")
    seen = {}
    for p, s in gns:
        seen.setdefault((s["in"]["h"], s["in"]["w"], s["in"]["c"], p["kernel"]), []).append((p, s))
    for (h, w, c, kern), ps in seen.items():
        ms = sorted(q["ms"] for q, _ in ps)[len(ps) // 2]
        s0 = ps[0][1]
        tbs = 2.0 * s0["in"]["n"] * h * w * c * (2 if s0["in"]["f16"] else 4) / ms / 1e9       # algorithmic: one read, one write
        print(f"{f'{h}x{w}x{c}':>18} {len(ps):5d} {kern:68} {ms:11.4f} {tbs:6.2f} {tbs / 6.29 * 100:6.1f}%")
if dws or ses or grs:
    import time
    B.RunPrepared(m, 10, True)
    t0 = time.perf_counter()
    reps = 50
    B.RunPrepared(m, reps, True)
    ms = (time.perf_counter() - t0) * 1e3 / reps
    print(json.dumps({"model": model_name, "batch": batch, "precision": plan["precision"], "replay_ms_per_step": round(ms, 4),
                      "images_per_s": round(batch / ms * 1e3, 1)}))
    # torch's yardstick runs in a child process of its own (a fresh HIP context, no state shared with the engine's)
    shapes = [[s["in"]["n"], s["in"]["c"], s["in"]["h"], s["in"]["w"], s["k"][0], s["stride"][0], s["pads"][0]] for _, s in dws]
    child = subprocess.run([sys.executable, "-c", TORCH_DW, json.dumps(shapes), plan["precision"]], capture_output=True, text=True, timeout=300)
    tms = json.loads(child.stdout.strip().splitlines()[-1]) if child.returncode == 0 else [float("nan")] * len(dws)
    if child.returncode != 0:
        print("# torch yardstick failed:", child.stderr.strip().splitlines()[-1:])
    print(f"{'depthwise step':40} {'HxWxC':>14} {'s':>2} {'ms':>8} {'GB/s':>7} {'%6.29T':>7} {'torch ms':>9}")
    for (p, s), t in zip(dws, tms):
        gbs = p["bytes"] / p["ms"] / 1e6
        shape = f"{s['in']['h']}x{s['in']['w']}x{s['in']['c']}"
        print(f"{p['name'][:40]:40} {shape:>14} {s['stride'][0]:2d} {p['ms']:8.4f} {gbs:7.0f} {gbs / 6290 * 100:6.1f}% {t:9.4f}")
if grs:
    peak_tf = 2500.0 if plan["precision"] == "fp16" else 157.3
    g_ms = sum(p["ms"] for p, _ in grs)
    print(f"# {len(grs)} grouped steps: {g_ms:.4f} ms, {g_ms / tot * 100:.1f}% of the eager forward; roofline peak {peak_tf} TF/s, 6.29 TB/s")
    shapes = [[s["in"]["n"], s["in"]["c"], s["in"]["h"], s["in"]["w"], s["out"]["c"], s["group"], s["k"][0], s["stride"][0], s["pads"][0]] for _, s in grs]
    child = subprocess.run([sys.executable, "-c", TORCH_GROUPED, json.dumps(shapes), plan["precision"]], capture_output=True, text=True, timeout=300)
    tms = json.loads(child.stdout.strip().splitlines()[-1]) if child.returncode == 0 else [float("nan")] * len(grs)
    if child.returncode != 0:
        print("# torch yardstick failed:", child.stderr.strip().splitlines()[-1:])
    print(f"{'grouped step':24} {'kernel':36} {'HxWxC/g':>14} {'s':>2} {'ms':>8} {'GB/s':>7} {'roof ms':>8} {'%roof':>6} {'torch ms':>9}")
    for (p, s), t in zip(grs, tms):
        gbs = p["bytes"] / p["ms"] / 1e6
        roof = max(p["bytes"] / 6.29e9, p["flops"] / (peak_tf * 1e9))
        shape = f"{s['in']['h']}x{s['in']['w']}x{s['in']['c']}/{s['group']}"
        print(f"{p['name'][:24]:24} {p['kernel'][:36]:36} {shape:>14} {s['stride'][0]:2d} {p['ms']:8.4f} {gbs:7.0f} {roof:8.4f} {roof / p['ms'] * 100:5.1f}% {t:9.4f}")
if ses:
    se_ms = sum(p["ms"] for p, _ in ses)
    print(f"# {len(ses)} squeeze-excite steps: {se_ms:.4f} ms, {se_ms / tot * 100:.1f}% of the eager forward")
    shapes = [[s["in"]["n"], s["in"]["c"], s["in"]["h"], s["in"]["w"], s["se"]["mid"]] for _, s in ses]
    child = subprocess.run([sys.executable, "-c", TORCH_SE, json.dumps(shapes), plan["precision"]], capture_output=True, text=True, timeout=300)
    tms = json.loads(child.stdout.strip().splitlines()[-1]) if child.returncode == 0 else [float("nan")] * len(ses)
    if child.returncode != 0:
        print("# torch yardstick failed:", child.stderr.strip().splitlines()[-1:])
    print(f"{'squeeze-excite step':40} {'HxWxC/mid':>16} {'chunks':>6} {'ms':>8} {'GB/s':>7} {'%6.29T':>7} {'torch ms':>9}")
    for (p, s), t in zip(ses, tms):
        gbs = p["bytes"] / p["ms"] / 1e6
        shape = f"{s['in']['h']}x{s['in']['w']}x{s['in']['c']}/{s['se']['mid']}"
        print(f"{p['name'][:40]:40} {shape:>16} {s['se']['chunks']:6d} {p['ms']:8.4f} {gbs:7.0f} {gbs / 6290 * 100:6.1f}% {t:9.4f}")
m.Destroy()
