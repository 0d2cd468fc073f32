#!/usr/bin/env python3
"""Headline benchmark: images/sec of DenseNet-121 fp32, batch 32 per GPU, device-resident inputs (+ p50 latency with --full).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

One "step" = one forward pass of the hot path (the captured hipGraph of the fused DenseNet-121 plan) over one batch of
synthetic 3x224x224 images that already sit in the engine's HBM input buffer.  Weak scaling: every rank owns an
independent shard of `--batch` images (no data-path collective); the only RCCL traffic is the load-time weight
broadcast from rank 0.  Rank 0 prints ONE JSON line.  A plain run only loads, warms up, times the K steps and prints it;
--dump-outputs DIR also saves the output of the last timed step (DIR/<output name>.npy, float32; the inputs are seeded,
so two builds can be compared output for output).  --full extends the line with

  roofline      the kernel family with the largest share of the forward's time (kernel name up to '<'): algorithmic FLOPs and
                bytes per launch / average launch duration, measured with HIP events on the model's stream in an instrumented
                eager pass of the same forward (EngineProfile), against the dense MFMA peak of the dtype and 8 TB/s HBM
  cpu_baseline  the oracle (numpy restatement of the ONNX ops, oracle/onnx_oracle.py) timed on this host on a bounded
                sample of the same workload; kind "port" — it is NOT ONNX Runtime (absent from the image)
  p50_ms, modelinfer_*   per-call latency of the device-resident step and of the full ModelInfer C-ABI call
                (host buffers, PCIe-inclusive; never used for `value`)
  secondary     the other BASELINE configurations that fit one GPU (headline runs at N=1 only)
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_FP32_MFMA_TFLOPS = 157.3      # MI355X_MICROARCH.md: dense fp32 matrix peak
SUSTAINED_FP32_MFMA_TFLOPS = 129.0  # what a chip full of v_mfma_f32_32x32x2_f32 sustains (65.5 cycles per issue at 1.97 GHz: profiles/r02/probe_mfma_rate.txt)
PEAK_FP16_MFMA_TFLOPS = 2500.0     # MI355X_MICROARCH.md: dense fp16/bf16 matrix peak (no sparsity)
PEAK_HBM_GBS = 8000.0


MODELS = {   # name -> (builder, input name, output name, classes, published architecture name)
    "densenet121": ("densenet121", "data_0", "fc6_1", "DenseNet-121"),
    "resnet50": ("resnet50", "data", "logits", "ResNet-50"),
}


def model_dir(model: str = "densenet121") -> str:
    from gpu_ai_inference_server_amd.modelgen import models
    root = os.environ.get("IE_BENCH_MODEL_ROOT", "/tmp/ie_bench_models")
    name = "densenet_onnx" if model == "densenet121" else model
    path = os.path.join(root, name, "1", "model.onnx")
    if not os.path.exists(path):
        models.write_repo(root, name, getattr(models, MODELS[model][0])("N"))
    return os.path.join(root, name, "1")


def host_cpu_share() -> int:
    """CPUs this process may actually use: cgroup quota, else scheduler affinity, else cpu_count."""
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            return max(1, int(int(quota) / int(period)))
    except Exception:  # noqa: BLE001
        pass
    try:
        return max(1, len(os.sched_getaffinity(0)))
    except Exception:  # noqa: BLE001
        return os.cpu_count() or 1


def cpu_baseline(sample_images: int, model: str = "densenet121", backend: str = "auto") -> dict:
    """Oracle (CPU restatement of the ONNX graph) on `sample_images` images of the same synthetic workload.

    backend "torch": the oracle's graph walk with torch-CPU (oneDNN) primitives - the closest optimised stand-in for the absent
    ONNX Runtime CPU provider; "numpy": the plain numpy im2col + BLAS oracle; "auto": torch when importable.
    """
    from gpu_ai_inference_server_amd.modelgen import models
    from oracle import onnx_oracle as O
    m = O.load_model(getattr(models, MODELS[model][0])(sample_images))
    x = models.synthetic_input((sample_images, 3, 224, 224), stream="bench")
    iname = MODELS[model][1]
    use_torch = False
    if backend in ("auto", "torch"):
        try:
            import torch  # noqa: F401
            use_torch = True
        except Exception:  # noqa: BLE001
            if backend == "torch":
                raise
    cores = host_cpu_share()
    if use_torch:
        import torch
        torch.set_num_threads(cores)                 # more threads than the CPU share only thrash (128 visible, 16 usable on the box)
        O.run_torch_cpu(m, {iname: x[:1]})           # warm up thread pool / primitive caches
        reps, t0 = 0, time.perf_counter()
        while reps < 16 and (reps == 0 or time.perf_counter() - t0 < 10.0):      # about 10 s of CPU work
            O.run_torch_cpu(m, {iname: x})
            reps += 1
        dt = (time.perf_counter() - t0) / reps
        how = f"oracle graph walk with torch-CPU (oneDNN) primitives, {reps} forwards of {sample_images}, {dt * reps:.1f} s"
    else:
        if sample_images > 8:                        # ~0.5 s per image: keep the numpy sample small
            sample_images = 8
            m = O.load_model(getattr(models, MODELS[model][0])(sample_images))
            x = x[:8]
        try:
            from threadpoolctl import threadpool_info
            cores = max([p.get("num_threads", 1) for p in threadpool_info()] or [1])
        except Exception:  # noqa: BLE001
            pass
        O.run(m, {iname: x[:1]})                     # warm BLAS threads / page in
        t0 = time.perf_counter()
        O.run(m, {iname: x})
        dt = time.perf_counter() - t0
        how = f"numpy im2col + BLAS oracle, one forward, {dt:.1f} s"
    return {"value": round(sample_images / dt, 3), "unit": "images/sec", "cores": int(cores), "kind": "port",
            "sample": f"batches of {sample_images} images of the same synthetic {MODELS[model][3]} fp32 workload ({how}); "
                      f"stand-in for the absent ONNX Runtime CPU EP"}


DTYPES = {"f32": ("fp32", "fp32", PEAK_FP32_MFMA_TFLOPS), "f16": ("fp16", "fp16 (half activations/weights, fp32 accumulate)", PEAK_FP16_MFMA_TFLOPS),
          "f8": ("fp8", "fp8 (OCP e4m3 activations/weights with calibrated scales, fp32 accumulate)", 5000.0),   # dense MFMA peak per dtype (no sparsity)
          # opt-in IE_FP32_SPLIT=1: fp32 tensors and weights; the 128-channel 1x1 convs form every fp32 product from exactly split bf16 pieces
          # (six bf16 MFMAs, fp32 accumulate: kernels_x6.hip); same parity bound as fp32, reported apart from the fp32 headline
          "f32x6": ("fp32", "fp32 with bf16x6 1x1 convs (fp32 products from exactly split bf16 operands on the bf16 matrix pipe, fp32 accumulate)", PEAK_FP32_MFMA_TFLOPS)}
BASELINE_CONFIG = {("densenet121", "f32"): "BASELINE configs[1]", ("densenet121", "f16"): "BASELINE configs[2]", ("resnet50", "f8"): "BASELINE configs[4]"}


DUMP_BYTES = 64 << 20      # --dump-outputs writes at most this much in all (the first rows of a larger output)


def dump_output(dump_dir, name, y, world):
    os.makedirs(dump_dir, exist_ok=True)
    rows = DUMP_BYTES // world // y[0].nbytes
    np.save(os.path.join(dump_dir, name + ".npy"), y[:rows])


def measure(B, models, sharding, *, model_name, dtype, Bsz, steps, warmup, rank, world, local_rank, dist, hostpath, full=True,
            want_detail=True, dump_dir=None):
    """Load `model_name` in precision `dtype`, put a synthetic batch into HBM, time K graph replays; returns the JSON-line dict on rank 0.
    `full`: also the p50 latency, roofline and (with `hostpath`) ModelInfer figures; `dump_dir`: save the last timed step's output there."""
    _, in_name, out_name, arch = MODELS[model_name]
    if rank == 0:
        model_dir(model_name)                        # rank 0 writes the synthetic model file once; the others wait for it
    if dist is not None:
        dist.barrier()
    mdir = model_dir(model_name)
    os.environ["IE_PRECISION"] = DTYPES[dtype][0]
    if dtype == "f32x6":
        os.environ["IE_FP32_SPLIT"] = "1"
    else:
        os.environ.pop("IE_FP32_SPLIT", None)
    model = B.CreateModel(mdir, os.path.basename(os.path.dirname(mdir)), device_id=local_rank)
    try:
        din, dout = B.Prepare(model, [[Bsz, 3, 224, 224]], 1)
        x = models.synthetic_input((Bsz, 3, 224, 224), stream=f"bench/rank{rank}")
        B.CopyToDevice(model, din[0], x)                 # inputs resident in HBM before any timing

        if dist is not None:                             # load-time weight exchange: one RCCL broadcast over xGMI
            import torch
            blob = B.GetWeightBlob(model)
            sharding.broadcast_weights(dist, blob, src=0)
            torch.cuda.synchronize()
            B.WeightsUpdated(model)                      # re-derives the half / fragment-major / e4m3 mirrors from the broadcast blob

        def barrier():
            B.Synchronize(model)
            if dist is not None:
                import torch
                torch.cuda.synchronize()
                dist.barrier()

        B.RunPrepared(model, warmup, True)
        barrier()
        t0 = time.perf_counter()
        B.RunPrepared(model, steps, True)           # EXACTLY K steps, back-to-back graph replays, then sync
        barrier()
        elapsed = time.perf_counter() - t0
        if dist is not None:
            import torch
            t = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed = float(t.item())

        y = np.empty((Bsz, 1000), np.float32)
        B.CopyToHost(model, y, dout[0])                  # the output of the last timed step
        assert np.isfinite(y).all()
        if dump_dir is not None:
            dump_output(dump_dir, out_name if world == 1 else f"{out_name}_rank{rank}", y, world)

        if full:      # per-call latency of the device-resident step (sync after every step)
            lat = []
            for _ in range(min(steps, 50)):
                t1 = time.perf_counter()
                B.RunPrepared(model, 1, True)
                lat.append((time.perf_counter() - t1) * 1e3)
            p50 = float(np.percentile(lat, 50))
        if rank != 0:
            return None
        total_images = Bsz * world * steps
        cfg_name = BASELINE_CONFIG.get((model_name, dtype), "additional configuration")
        result = {
            "metric": f"images/sec, {arch} {'fp32 (bf16x6 1x1 convs)' if dtype == 'f32x6' else DTYPES[dtype][0]}, batch {Bsz} per GPU, device-resident inputs"
                      + (" (+ p50 step latency)" if full else ""),
            "value": round(total_images / elapsed, 2), "unit": "images/sec", "n_gpus": world, "steps": steps,
            "warmup": warmup, "ms_per_step": round(elapsed / steps * 1e3, 4), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": dtype, "data": "synthetic",
            "config": {"workload": f"{arch} {DTYPES[dtype][1]} batch={Bsz} per GPU, synthetic 3x224x224 inputs ({cfg_name}); "
                                   "synthetic ONNX graph + seeded random weights (reference model file is not in the mount)",
                       "global_batch": Bsz * world, "per_gpu_batch": Bsz, "parallelism": f"dp{world} (independent batch shards)",
                       "scaling_note": "weak scaling: every rank runs the SAME per-GPU batch, so N ranks are expected at ~N x this value (no data-path "
                                       "collective); a FIXED global batch of 32 cut over 8 GPUs (4 images each, ~1.0 ms per step against 2.2 ms for 32) "
                                       "would scale ~2.2x, not 8x: DESIGN.md section 6"},
        }
        if not full:
            return result
        result["p50_ms"] = round(p50, 4)
        # ---- roofline of the dominant kernel family, HIP events on the model's stream --------------------------
        prof = B.Profile(model, 9)
        fam = {}
        for p in prof:
            k = p["kernel"].split("<")[0]
            f = fam.setdefault(k, {"ms": 0.0, "flops": 0.0, "bytes": 0.0, "launches": 0})
            f["ms"] += p["ms"]; f["flops"] += p["flops"]; f["bytes"] += p["bytes"]; f["launches"] += 1
        dom = max(fam, key=lambda k: fam[k]["ms"])
        d = fam[dom]
        achieved = d["flops"] / (d["ms"] * 1e-3) / 1e12
        traffic, traffic_src = None, None
        try:      # HBM bytes per launch from the committed PMC pass of the same command (rocprofv3 cannot run inside bench.py)
            tf = {("densenet121", "f32"): "traffic.json", ("densenet121", "f16"): "traffic_f16_b128.json", ("resnet50", "f8"): "traffic_resnet50_f8_b256.json", ("densenet121", "f32x6"): "traffic_f32x6_b32.json"}.get((model_name, dtype))
            rounds = sorted(r_ for r_ in os.listdir(os.path.join(ROOT, "profiles")) if tf and os.path.exists(os.path.join(ROOT, "profiles", r_, tf)))
            if rounds:
                traffic_src = os.path.join("profiles", rounds[-1], tf)
                traffic = json.load(open(os.path.join(ROOT, traffic_src))).get(dom, {}).get("hbm_bytes_per_launch")
        except Exception:  # noqa: BLE001
            pass
        mfma_peak = DTYPES[dtype][2]
        achieved_gbs = d["bytes"] / (d["ms"] * 1e-3) / 1e9
        frac_mfma, frac_hbm = achieved / mfma_peak, achieved_gbs / PEAK_HBM_GBS
        common = {"kernel": dom, "traffic": traffic, "traffic_unit": "HBM bytes per launch", "traffic_source": traffic_src,
                  "algorithmic_bytes_per_launch": round(d["bytes"] / d["launches"], 1), "launches_per_step": d["launches"],
                  "flops_per_launch": round(d["flops"] / d["launches"], 1), "avg_launch_ms": round(d["ms"] / d["launches"], 6),
                  "achieved_tflops": round(achieved, 3), "achieved_gbs": round(achieved_gbs, 1),
                  "frac_of_mfma_peak": round(frac_mfma, 4), "frac_of_hbm_peak": round(frac_hbm, 4)}
        if dtype in ("f32", "f32x6"):
            common["sustained_peak_tflops"] = SUSTAINED_FP32_MFMA_TFLOPS      # `peak` stays the guide's 157.3; this is the measured ceiling
            common["frac_of_sustained_peak"] = round(achieved / SUSTAINED_FP32_MFMA_TFLOPS, 4)
        if frac_mfma >= frac_hbm:      # the ceiling this kernel family is closer to is the one that bounds it
            result["roofline"] = {"bound": "mfma", "achieved": round(achieved, 3), "peak": mfma_peak, "unit": "TFLOP/s", "frac": round(frac_mfma, 4)}
        else:
            result["roofline"] = {"bound": "hbm", "achieved": round(achieved_gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(frac_hbm, 4)}
        result["roofline"].update(common)
        if want_detail:
            result["roofline"]["note"] = (
                "algorithmic FLOPs (2*M*N*K) and bytes (operands once + result once) summed over the family's launches of one forward / sum "
                "of their HIP-event durations in an eager instrumented pass on the model's stream; traffic = (2*FETCH_SIZE + WRITE_SIZE) "
                "from a separate rocprofv3 --pmc pass (gfx950 FETCH_SIZE correction), family average per launch")
        # the tight per-layer bound  sum_l max(bytes_l / HBM peak, flops_l / MFMA peak of the dtype)
        tight_ms = sum(max(p["bytes"] / (PEAK_HBM_GBS * 1e9), p["flops"] / (mfma_peak * 1e12)) for p in prof) * 1e3
        result["roofline_model"] = {"tight_bound_ms_per_step": round(tight_ms, 4), "frac_of_tight_bound": round(tight_ms / (elapsed / steps * 1e3), 4),
                                    "flops_per_step": sum(p["flops"] for p in prof), "algorithmic_bytes_per_step": sum(p["bytes"] for p in prof)}
        result["kernel_families_ms"] = {k: round(v["ms"], 4) for k, v in sorted(fam.items(), key=lambda kv: -kv[1]["ms"])}
        result["eager_forward_ms"] = round(sum(p["ms"] for p in prof), 4)
        # ---- full C-ABI call with host buffers (PCIe-inclusive; reported, never `value`) -----------------------
        if hostpath:
            # Two clocks per payload type.  modelinfer_*: time INSIDE the ModelInfer C call with buffers marshalled as the Go binding
            # has them at the call (fresh C.malloc'ed pageable memory, inference_binding.go:590-651) - what the engine answers for.
            # binding_*: the whole (*Model).Infer mirror including the binding's own malloc + copy in / copy out, which the build
            # leaves unchanged.
            outs = [B.OutputConfig(out_name, [Bsz, 1000, 1, 1] if model_name == "densenet121" else [Bsz, 1000])]
            xb = np.clip(x * 255.0, 0, 255).astype(np.uint8)
            for tag, ins in (("", [B.TensorData(in_name, B.DataTypeFloat32, B.Shape([Bsz, 3, 224, 224]), x)]),
                             ("_uint8", [B.TensorData(in_name, B.DataTypeUint8, B.Shape([Bsz, 3, 224, 224]), xb)])):
                model.InferTimed(ins, outs, 3)
                before = B.RuntimeInfo(model)
                tl = model.InferTimed(ins, outs, 15)
                after = B.RuntimeInfo(model)
                p50c = float(np.percentile(tl, 50))
                result[f"modelinfer{tag}_p50_ms"] = round(p50c * 1e3, 3)
                result[f"modelinfer{tag}_images_per_s"] = round(Bsz / p50c, 1)
                nfw = max(1, after["forwards"] - before["forwards"])
                result[f"modelinfer{tag}_device_ms"] = round((after["device_ms_total"] - before["device_ms_total"]) / nfw, 3)
                if want_detail:
                    hl = []
                    for _ in range(8):
                        t1 = time.perf_counter()
                        model.Infer(ins, outs)
                        hl.append(time.perf_counter() - t1)
                    result[f"binding{tag}_p50_ms"] = round(float(np.percentile(hl, 50)) * 1e3, 3)
            info = B.RuntimeInfo(model)
            result["modelinfer_pipeline"] = {"chunks": info["last_chunks"], "head_steps": info["last_head_steps"]}
            # co-headline: what the unchanged Go server sees through the C ABI (host buffers, PCIe-inclusive) beside the device-resident `value`
            result["metric"] += (f"; through ModelInfer with host FLOAT32 payloads {result['modelinfer_images_per_s']:.0f} images/sec "
                                 f"(p50 {result['modelinfer_p50_ms']:.3f} ms), UINT8 payloads {result['modelinfer_uint8_images_per_s']:.0f} images/sec")
        return result
    finally:
        model.Destroy()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=None, help="images per GPU per step (default 32; 128 for f16, 256 for f8)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need: p50 step latency, roofline (an instrumented eager pass), "
                         "the ModelInfer host path, the secondary configurations and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the output of the last timed step as DIR/<output name>.npy (float32)")
    ap.add_argument("--cpu-sample", type=int, default=32, help="images for the CPU baseline (0 = skip; --full)")
    ap.add_argument("--cpu-backend", choices=["auto", "torch", "numpy"], default="auto")
    ap.add_argument("--dtype", choices=["f32", "f16", "f8", "f32x6"], default="f32",
                    help="f32 = the headline (BASELINE configs[1]); f16 = the fp16 precision mode (configs[2-3]); f8 = the fp8 mode (configs[4], --model resnet50)")
    ap.add_argument("--model", choices=sorted(MODELS), default="densenet121",
                    help="densenet121 = the headline workload; resnet50 = the second model family (BASELINE configs[4]'s architecture)")
    ap.add_argument("--no-hostpath", action="store_true", help="skip the ModelInfer (PCIe-inclusive) measurement (--full)")
    ap.add_argument("--no-secondary", action="store_true", help="headline only: skip the fp16 B=128 and ResNet-50 fp8 B=256 lines (--full)")
    args = ap.parse_args()
    if args.batch is None:
        args.batch = {"f32": 32, "f16": 128, "f8": 256, "f32x6": 32}[args.dtype]

    from _pkg import load_package
    load_package()
    from gpu_ai_inference_server_amd import binding as B
    from gpu_ai_inference_server_amd import sharding
    from gpu_ai_inference_server_amd.modelgen import models

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    if world > 1 or "RANK" in os.environ:      # launched by torch.distributed.run: exercise the RCCL path even at N=1
        import torch
        import torch.distributed as dist_mod
        torch.cuda.set_device(local_rank)
        dist_mod.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        dist = dist_mod
    if args.gpus != world and rank == 0 and world > 1:
        print(f"warning: --gpus {args.gpus} != WORLD_SIZE {world}", file=sys.stderr)

    if not B.IsCUDAAvailable():
        raise SystemExit("bench.py needs a HIP device (the engine has no CPU fallback)")

    common = dict(rank=rank, world=world, local_rank=local_rank, dist=dist)
    result = measure(B, models, sharding, model_name=args.model, dtype=args.dtype, Bsz=args.batch, steps=args.steps, warmup=args.warmup,
                     hostpath=not args.no_hostpath, full=args.full, dump_dir=args.dump_outputs, **common)
    # The other BASELINE configurations that fit one GPU ride on the same line (a few hundred ms each), so they are driver-run
    # numbers too: DenseNet-121 fp16 B=128 (configs[2]) and ResNet-50 fp8 B=256 (configs[4]).  Only behind the default headline.
    headline = args.model == "densenet121" and args.dtype == "f32"
    if args.full and headline and not args.no_secondary and world == 1:
        secondary = []
        for mname, dt, bsz in (("densenet121", "f16", 128), ("resnet50", "f8", 256), ("densenet121", "f32x6", 32)):
            r = measure(B, models, sharding, model_name=mname, dtype=dt, Bsz=bsz, steps=max(5, args.steps // 2), warmup=max(2, args.warmup // 2),
                        hostpath=not args.no_hostpath, want_detail=False, **common)
            if r is not None:
                secondary.append({k: r[k] for k in ("metric", "value", "unit", "ms_per_step", "steps", "warmup", "dtype", "config", "p50_ms", "roofline",
                                                      "roofline_model", "kernel_families_ms") if k in r} |
                                 {k: v for k, v in r.items() if k.startswith("modelinfer")})
        if result is not None:
            result["secondary"] = secondary
    if args.full and rank == 0:
        if args.cpu_sample > 0 and world == 1:       # reported on rank 0 at N=1 only (the other ranks would idle behind it)
            # the numpy oracle needs ~0.5 s per image: keep its sample small
            nimg = args.cpu_sample if args.cpu_backend != "numpy" else min(args.cpu_sample, 8)
            result["cpu_baseline"] = cpu_baseline(nimg, args.model, args.cpu_backend)
        else:
            result["cpu_baseline"] = None
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps(result))


if __name__ == "__main__":
    main()
