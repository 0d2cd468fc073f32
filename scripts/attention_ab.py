#!/usr/bin/env python3
"""The attention kernels of this build against a build of the parent commit on one MI355X: byte-equal outputs, and the time of the attention step.

    python scripts/attention_ab.py --parent-lib <libinference_engine.so of the parent commit> [--equal | --times] [--times-name NAME] [out_dir]     (default profiles/attention_shared)

Both builds run in the same session, each in child processes of its own (the library is chosen through INFERENCE_ENGINE_LIB), one GPU process at a time.
* --equal: seeded inputs through the attention subgraphs of the test helpers (tests/*_graphs.py), every kernel form at the small shapes around its tile
  edges, fp32 and fp16.  Per case the SHA-256 of every output tensor (`out`, `present.*`, for bound runs the cache read back) must be the same under
  both libraries -> ab_equal.txt, one line per case with the kernel that ran.  A bound extend step with more new tokens than the cache has rows
  (Lq 33 or 65 at P 31 or 32) cannot exist (the capacity of a bound cache is the graph's P), so those shapes run unbound only.
* --times: the attention step alone (HIP events around the launch, B.Profile: median of 20 after a warm-up) at the shapes the project records
  (profiles/attn_vit, bert, gpt2, llama, attn_swin), three parent children and three of this build, alternating.  Per shape the
  medians of three and the spreads (max - min) -> ab_times.txt (--times-name NAME: NAME in its place, for the record of a state that is not the
  committed one); this build's median may exceed the parent's by no more than the parent's own spread.
Neither flag: both.  Every child runs under its own time limit; the first one that fails ends the run.  Exit status 1: a case differs or a shape is slower."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 900
PRECS = ("fp32", "fp16")
GROUPS = {1: (4, 4), 2: (4, 2), 4: (4, 1), 8: (8, 1)}      # G -> (heads, K / V heads)


def _setup():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _pkg import load_package
    load_package()


def equal_cases(family):
    """the cases of a family as tuples; the first element names the runner"""
    cs = []
    if family == "tile1":
        cs += [("plain", l, hd) for l in (17, 33) for hd in (32, 64)]
        cs += [("masked", 33, hd, c) for hd in (32, 64) for c in ("min", -10000.0)]
        cs += [("gpt2", l, hd, 1) for l in (33, 129) for hd in (32, 64)]
        cs += [("gqa", l, kvh, hd, rope, 1) for l in (33, 129) for kvh in (4, 2) for hd in (32, 64) for rope in (None, "init")]
    elif family == "tile3":
        cs += [("gqa", l, kvh, hd, "init", 3) for l in (257, 289) for kvh in (4, 2) for hd in (32, 64)]
    elif family == "window":
        cs += [("window", (14, 14), (7, 7), sh, 2, 32) for sh in ((0, 0), (3, 3))]
    elif family in ("decode", "decode_inplace"):
        for hd in (32, 64, 128):
            for g in (1, 2, 4, 8):
                for past in (15, 16, 17, 257):
                    for tile, splits in ((0, 1), (4, 1), (4, 3)):
                        if family == "decode":
                            cs.append(("decode", g, hd, past, tile, splits, None))
                        else:
                            cs += [("decode", g, hd, past, tile, splits, ln) for ln in (0, past // 4, past - 1)]
    elif family in ("extend", "extend_inplace"):
        for hd in (32, 64):
            for lq in (2, 33, 65):
                for past in (31, 32, 257):
                    for tile, splits in ((0, 1), (5, 1), (5, 3)):
                        if family == "extend":
                            cs.append(("extend", hd, lq, past, tile, splits, None))
                        elif past >= lq:
                            cs += [("extend", hd, lq, past, tile, splits, ln) for ln in (0, past // 4, past - lq)]
    return cs


FAMILIES = ("tile1", "tile3", "window", "decode", "extend", "decode_inplace", "extend_inplace")


def _sha(x):
    import numpy as np
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()[:16]


def _attn_label(kern):
    return " | ".join(k for k in kern if "attention" in k or "kv_append" in k)


def run_case(root, case, prec, i):
    """one case under the loaded library -> (the attention kernel that ran, {output: sha})"""
    import numpy as np
    import bert_graphs as BG
    import extend_graphs as EG
    import gpt2_graphs as GG
    import kv_graphs as KG
    import llama_graphs as LG
    import resident_graphs as RG
    import swin_graphs as SG
    import vit_graphs as VG
    from engine_run import run_model
    from gpu_ai_inference_server_amd import binding as B
    from gpu_ai_inference_server_amd.modelgen import models
    kind, name, N = case[0], f"m{i}", 2
    env = dict(IE_PRECISION=prec)
    if kind in ("plain", "masked", "gpt2", "gqa", "window"):
        if kind == "plain":
            _, l, hd = case
            h, mb, feeds, env["IE_FORCE_TILE"] = 3, VG.attn_graph(N, l, 3, hd), [{"x": np.array(VG.make_input(N, l, 3, hd, "randn"))}], "1"
        elif kind == "masked":      # the eight mask rows of the tests over four requests; the last request's first image is fully masked
            _, l, hd, c = case
            h, mb, env["IE_FORCE_TILE"] = 3, BG.masked_attn_graph(N, l, 3, hd, mask_value=c), "1"
            masks, idx = BG.mask_requests(N, l)
            feeds = [{"x": np.array(BG.masked_input(N, l, h, hd, "randn", tuple(r))), "attention_mask": np.array(mk)} for mk, r in zip(masks, idx)]
        elif kind == "gpt2":
            _, l, hd, tile = case
            h, mb, feeds, env["IE_ATTN_TILE"] = 4, GG.causal_attn_graph(N, l, 4, hd, mask="where_const"), [{"x": np.array(VG.make_input(N, l, 4, hd, "randn"))}], str(tile)
        elif kind == "gqa":
            _, l, kvh, hd, rope, tile = case
            h, mb, feeds, env["IE_ATTN_TILE"] = 4, LG.gqa_attn_graph(N, l, 4, kvh, hd, rope=rope, causal=True), [{"x": LG.gqa_input(N, l, 4, kvh, hd)}], str(tile)
        else:
            _, hw, win, sh, h, hd = case
            x = np.array(VG.make_input(N, hw[0] * hw[1], h, hd, "randn")).reshape(N, 3 * h * hd, hw[0], hw[1])
            mb, feeds, env["IE_FORCE_TILE"] = SG.wattn_graph(N, hw, win, sh, h, hd), [{"x": x}], "1"
        oshape = (N, h * hd, hw[0], hw[1]) if kind == "window" else (N, h * hd, 1, l)
        ys, kern = run_model(models.write_repo(root, name, mb), name, env, feeds, "y", oshape)
        return _attn_label(kern), {f"y{k}": _sha(y) for k, y in enumerate(ys)}
    N = 3      # image 0 appends every token; image 1 none (in place: c = 0); image 2 holds 3 rows at most and appends a ragged chunk
    if kind == "decode":
        _, g, hd, past, tile, splits, ln = case
        (h, kvh), lq = GROUPS[g], 1
        lens = [past, past, min(3, past)] if ln is None else [ln, ln, min(3, ln)]
        rows, feeds = KG.decode_feeds(N, h, kvh, hd, past, valid=lens, positions=lens)
        if ln is not None:
            feeds["attention_mask"][1, past] = 0
        mb = KG.decode_attn_graph(rows, N, h, kvh, hd, past, max_pos=past + 8)
    else:
        _, hd, lq, past, tile, splits, ln = case
        h, kvh = 4, 2
        lens = [past, past, min(3, past)] if ln is None else [ln, ln, min(3, ln)]
        new = [lq, 0 if ln is not None else lq, max(1, lq - 1)]
        rows, feeds = EG.extend_feeds(N, h, kvh, hd, past, lq, valid=lens, chunk_valid=new, max_pos=past + lq + 8)
        mb = EG.extend_attn_graph(rows, N, h, kvh, hd, past, lq, max_pos=past + lq + 8)
    env.update(IE_ATTN_TILE=str(tile), IE_ATTN_SPLITS=str(splits))
    path = models.write_repo(root, name, mb)
    if ln is None:
        outs = {"out": (N, lq, h * hd), "present.0.key": (N, kvh, past + lq, hd), "present.0.value": (N, kvh, past + lq, hd)}
        ys, _, kern = GG.run_outputs(path, name, env, feeds, outs)
        return _attn_label(kern), {k: _sha(v) for k, v in ys.items()}
    with RG.session(env, {name: path}, (1, N, kvh, past, hd)) as (ms, kc):
        RG.fill(kc, feeds, lens)
        y = RG.request(ms[name], RG.unbound(feeds), {"out": (N, lq, h * hd)})["out"]
        sha = {"out": _sha(y), "cache.key": _sha(kc.read(0, 0)), "cache.value": _sha(kc.read(0, 1)), "lengths": ",".join(map(str, kc.lengths()))}
        kern = [p["kernel"] for p in B.Profile(ms[name], 1)]
    return _attn_label(kern), sha


def equal_child(family, prec):
    _setup()
    out = {}
    with tempfile.TemporaryDirectory() as root:
        for i, case in enumerate(equal_cases(family)):
            kern, sha = run_case(root, case, prec, i)
            out[json.dumps(case)] = {"kernel": kern, "sha": sha}
            if i % 50 == 49:
                print(f"  {family} {prec}: {i + 1} cases", file=sys.stderr, flush=True)      # (a sign of life: the parent passes stderr through)
    print(json.dumps(out))


# (what, n, heads, kv heads, L or P, hd, Lq, tile or None for the default, in-place length or None): the recorded shapes
TIME_SHAPES = [("vit", 32, 12, 12, 197, 64, 0, None, None), ("vit", 32, 12, 12, 50, 64, 0, None, None), ("bert masked", 32, 12, 12, 128, 64, 0, None, None),
               ("gpt2 causal", 8, 12, 12, 1024, 64, 0, 3, None), ("llama rope", 8, 9, 3, 128, 64, 0, None, None), ("llama rope", 8, 9, 3, 1024, 64, 0, 3, None),
               ("swin 56x56", 32, 3, 3, 56, 32, 0, None, None), ("swin 14x14", 32, 12, 12, 14, 32, 0, None, None),
               ("decode", 8, 9, 3, 1023, 64, 1, None, None), ("decode", 8, 24, 8, 1023, 128, 1, None, None), ("decode", 1, 32, 8, 4095, 128, 1, None, None),
               ("decode in place", 8, 9, 3, 1023, 64, 1, None, 1022), ("decode in place", 8, 24, 8, 1023, 128, 1, None, 1022),
               ("extend", 8, 9, 3, 1023, 64, 4, None, None), ("extend", 8, 9, 3, 1023, 64, 128, None, None),
               ("extend in place", 8, 9, 3, 1023, 64, 4, None, 1019), ("extend in place", 8, 9, 3, 1023, 64, 128, None, 895)]


def time_child():
    """every TIME_SHAPES row at fp32 and fp16 -> {id: {kernel, us}}: the attention step's median of 20 launches behind three warm-up runs"""
    _setup()
    import numpy as np
    import bert_graphs as BG
    import extend_graphs as EG
    import gpt2_graphs as GG
    import kv_graphs as KG
    import llama_graphs as LG
    import swin_graphs as SG
    import vit_graphs as VG
    from engine_run import with_env
    from gpu_ai_inference_server_amd import binding as B
    from gpu_ai_inference_server_amd.modelgen import models
    out = {}
    with tempfile.TemporaryDirectory() as root:
        for i, (what, n, h, kvh, l, hd, lq, tile, ln) in enumerate(TIME_SHAPES):
            r = np.random.RandomState(i)
            if what == "vit":
                mb, feeds = VG.attn_graph(n, l, h, hd), {"x": r.randn(n, 3 * h * hd, 1, l).astype(np.float32)}
            elif what == "bert masked":
                mb, feeds = BG.masked_attn_graph(n, l, h, hd, mask_value="min"), {"x": r.randn(n, 3 * h * hd, 1, l).astype(np.float32), "attention_mask": (r.rand(n, l) < 0.8).astype(np.int64)}
            elif what == "gpt2 causal":
                mb, feeds = GG.causal_attn_graph(n, l, h, hd, mask="where_const"), {"x": r.randn(n, 3 * h * hd, 1, l).astype(np.float32)}
            elif what == "llama rope":
                mb, feeds = LG.gqa_attn_graph(n, l, h, kvh, hd, rope="init", causal=True), {"x": LG.gqa_input(n, l, h, kvh, hd)}
            elif what.startswith("swin"):
                mb, feeds = SG.wattn_graph(n, (l, l), (7, 7), (3, 3), h, hd), {"x": r.randn(n, 3 * h * hd, l, l).astype(np.float32)}
            else:
                valid = [l if ln is None else ln] * n
                if lq == 1:
                    rows, feeds = KG.decode_feeds(n, h, kvh, hd, l, valid=valid, positions=valid)
                    mb = KG.decode_attn_graph(rows, n, h, kvh, hd, l, max_pos=l + 1)
                else:
                    rows, feeds = EG.extend_feeds(n, h, kvh, hd, l, lq, valid=valid, max_pos=l + lq)
                    mb = EG.extend_attn_graph(rows, n, h, kvh, hd, l, lq, max_pos=l + lq)
            path = models.write_repo(root, f"t{i}", mb)
            for prec in PRECS:
                def go():
                    m = B.CreateModel(path, f"t{i}")
                    kc = None
                    try:
                        if ln is not None:
                            kc = B.KvCache(1, n, kvh, l, hd)
                            kc.bind(m)
                            kc.write(0, 0, feeds["past_key_values.0.key"])
                            kc.write(0, 1, feeds["past_key_values.0.value"])
                            kc.set_lengths([ln] * n)
                        din, _ = B.Prepare(m, [list(v.shape) for v in feeds.values()], 3 if lq else 1)
                        for d, (k, v) in zip(din, feeds.items()):
                            if ln is None or not k.startswith("past_key_values."):
                                B.CopyToDevice(m, d, v)
                        B.RunPrepared(m, 3, True)
                        ps = [p for p in B.Profile(m, 20) if "attention" in p["kernel"]]
                        if len(ps) != 1:
                            sys.exit(f"{what} N {n} H {h} / {kvh} L {l} hd {hd} Lq {lq} {prec}: {len(ps)} attention steps in the profile, one expected: {[p['kernel'] for p in ps]}")
                        return {"kernel": ps[0]["kernel"], "us": ps[0]["ms"] * 1e3}
                    finally:
                        if kc is not None:
                            kc.destroy()
                        m.Destroy()
                env = dict(IE_PRECISION=prec, IE_AUTOTUNE="0", **({} if tile is None else {"IE_ATTN_TILE": str(tile)}))
                out[f"{what} (N {n}, H {h} / {kvh}, {'P' if lq else 'L'} {l}, hd {hd}" + (f", Lq {lq}" if lq > 1 else "") + (f", len {ln}" if ln is not None else "") + f") {prec}"] = with_env(env, go)
    print(json.dumps(out))


def child(args, what, lib=None):
    env = dict(os.environ)
    if lib:
        env["INFERENCE_ENGINE_LIB"] = lib
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE, text=True, timeout=CHILD_TIMEOUT, env=env)
    except subprocess.TimeoutExpired:
        sys.exit(f"{what}: ran into its time limit; nothing further is started")
    if r.returncode != 0 or not r.stdout.strip():
        sys.exit(f"{what}: failed with status {r.returncode}; nothing further is started")
    return json.loads(r.stdout.strip().splitlines()[-1])


def equal(parent, out_dir):
    lines, bad = [], 0
    for family in FAMILIES:
        for prec in PRECS:
            theirs = child(["--equal-child", family, prec], f"{family} {prec}, parent build", parent)
            mine = child(["--equal-child", family, prec], f"{family} {prec}, this build")
            for case in sorted(set(theirs) ^ set(mine)):      # a case only one build has a result for
                bad += 1
                lines.append(f"DIFFER {family} {prec} {case}: a result under {'the parent build' if case in theirs else 'this build'} only")
            for case, a in theirs.items():
                if case not in mine:
                    continue
                b = mine[case]
                same = a["sha"] == b["sha"] and a["kernel"] == b["kernel"]
                bad += not same
                diff = "" if same else "   parent " + json.dumps(a) + "   this " + json.dumps(b)
                lines.append(f"{'equal ' if same else 'DIFFER'} {family} {prec} {case} ({len(a['sha'])} tensors) [{b['kernel']}]{diff}")
            print(f"{family} {prec}: {len(theirs)} cases, {sum(l.startswith('DIFFER') and f' {family} {prec} ' in l for l in lines)} differ", flush=True)
    lines.append(f"{len(lines)} cases, {bad} differ")
    open(os.path.join(out_dir, "ab_equal.txt"), "w").write("\n".join(lines) + "\n")
    print(lines[-1], flush=True)
    return bad


def times(parent, out_dir, name="ab_times.txt"):
    runs = {"parent": [], "this": []}
    for rep in range(3):
        runs["parent"].append(child(["--time-child"], f"timing, parent build, run {rep}", parent))
        runs["this"].append(child(["--time-child"], f"timing, this build, run {rep}"))
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    lines, bad = ["us of the attention step, median of 20 launches per run, three runs per build alternating: median (max - min); margin = the parent's max - min"], 0
    for k in runs["parent"][0]:
        p, t = [r[k]["us"] for r in runs["parent"]], [r[k]["us"] for r in runs["this"]]
        slow = med(t) - med(p) > max(p) - min(p)
        bad += slow
        lines.append(f"{k:70s} parent {med(p):9.1f} ({max(p) - min(p):6.1f})   this {med(t):9.1f} ({max(t) - min(t):6.1f})   {'OUTSIDE' if slow else 'within '}   [{runs['this'][0][k]['kernel']}]")
    lines.append(f"{len(lines) - 1} shapes, {bad} outside the parent's spread")
    open(os.path.join(out_dir, name), "w").write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)
    return bad


def main():
    args = sys.argv[1:]
    if len(args) < 2 or args[0] != "--parent-lib":
        sys.exit(__doc__)
    parent, args = os.path.abspath(args[1]), args[2:]
    name = "ab_times.txt"
    if "--times-name" in args:
        k = args.index("--times-name")
        name, args = args[k + 1], args[:k] + args[k + 2:]
    which = [a for a in args if a in ("--equal", "--times")] or ["--equal", "--times"]
    rest = [a for a in args if a not in ("--equal", "--times")]
    out_dir = rest[0] if rest else os.path.join(ROOT, "profiles", "attention_shared")
    os.makedirs(out_dir, exist_ok=True)
    bad = (equal(parent, out_dir) if "--equal" in which else 0) + (times(parent, out_dir, name) if "--times" in which else 0)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--equal-child":
        equal_child(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 2 and sys.argv[1] == "--time-child":
        time_child()
    else:
        main()
