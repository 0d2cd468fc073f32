"""CPU: com.microsoft MatMulNBits through the ONNX reader and the planner: the qlinear steps of one Linear and of an int4 Llama (prefill, decode, extend),
the merged qkv step, the folded residual, the packed byte count, the tile switch, and every refusal by node and rule."""
import numpy as np
import pytest

from engine_run import describe
from gpu_ai_inference_server_amd.modelgen import models
from gpu_ai_inference_server_amd.modelgen import onnx_pb as pb

N = 2


def _plan(tmp_path, monkeypatch, mb, batch=N, prec="fp32", **env):
    return describe(models.write_repo(str(tmp_path), "g", mb), batch, monkeypatch, prec, **env)


@pytest.mark.parametrize("prec", ("fp32", "fp16"))
@pytest.mark.parametrize("block,zero,res", ((32, True, True), (64, False, False), (128, True, False)))
def test_one_linear(tmp_path, monkeypatch, engine_lib, prec, block, zero, res):
    k, n = 384, 80
    st = [s for s in _plan(tmp_path, monkeypatch, models.qlinear(8, k, n, q_block=block, q_zero=zero, residual=res), 8, prec)["steps"] if s["kind"] == "qlinear"]
    assert len(st) == 1
    q = st[0]
    assert (q["in"]["c"], q["out"]["c"], q["block_size"], q["residual"], "in2" in q) == (k, n, block, res, res)
    assert q["packed_bytes"] == n * k // 2 + 4 * n * (k // block) + (n * ((k // block + 1) // 2) if zero else 0)
    assert (q["zero_points_off"] >= 0) == zero and q["tile"] == (1 if prec == "fp16" else 0)      # the MFMA kernel by default where it is eligible
    assert q["bytes"] == q["packed_bytes"] + (2 if prec == "fp16" else 4) * 8 * (k + n * (2 if res else 1))


@pytest.mark.parametrize("kw", (dict(seq=8, present=True), dict(seq=1, past=12), dict(seq=4, past=12)), ids=("prefill", "decode", "extend"))
def test_int4_llama(tmp_path, monkeypatch, engine_lib, kw):
    depth = 2
    p = _plan(tmp_path, monkeypatch, models.llama_tiny(N, quant="int4", **kw), prec="fp16")
    twin = _plan(tmp_path, monkeypatch, models.llama_tiny(N, quant="int4", q_form="dense", **kw), prec="fp16")
    ql = [s for s in p["steps"] if s["kind"] == "qlinear"]
    # per layer: the merged qkv (q 128 | k 64 | v 64 columns), o_proj and down_proj with the residual folded, gate and up; the head stays a conv
    assert [(s["in"]["c"], s["out"]["c"], s["residual"]) for s in ql] == depth * [(128, 256, False), (128, 128, True), (128, 256, False), (128, 256, False), (256, 128, True)]
    assert all(s["tile"] == 1 and s["block_size"] == 32 and s["zero_points_off"] >= 0 for s in ql)
    assert [s["kind"] for s in p["steps"]] == [("qlinear" if s["kind"] == "conv" and i < len(twin["steps"]) - 1 else s["kind"]) for i, s in enumerate(twin["steps"])]
    pinned = _plan(tmp_path, monkeypatch, models.llama_tiny(N, quant="int4", **kw), prec="fp16", IE_QLINEAR_TILE="0")
    assert {s["tile"] for s in pinned["steps"] if s["kind"] == "qlinear"} == {0}
    assert [s.get("tile") for s in pinned["steps"] if s["kind"] != "qlinear"] == [s.get("tile") for s in p["steps"] if s["kind"] != "qlinear"]


def _node(edit=None, drop=(), extra=(), attrs=None, scales=np.float32, k=64, n=16):
    """x [N, k] -> MatMulNBits -> y with every operand present; `edit` / `drop` / `extra` / `attrs` spoil one thing"""
    gb = models.GraphBuilder("bad", 3)
    nblk = k // 32
    ops = {"B": np.zeros((n, nblk, 16), np.uint8), "scales": np.ones(n * nblk, scales), "zero_points": np.zeros((n, (nblk + 1) // 2), np.uint8),
           "g_idx": None, "bias": np.zeros(n, np.float32)}
    ops.update(edit or {})
    ins = ["x"] + [gb.init(name, a) if a is not None and name not in drop else "" for name, a in ops.items()]
    at = dict({"K": k, "N": n, "bits": 4, "block_size": 32}, **(attrs or {}))
    gb.nodes.append(pb.node("MatMulNBits", ins, ["y"], "mm4", [pb.attr_int(a, v) for a, v in at.items()], domain="com.microsoft"))
    for name, a in extra:
        gb.init(name, a)
    return gb.finish([("x", [N, k])], [("y", [N, n])], opset=18)


@pytest.mark.parametrize("mb,why", (
    (_node(attrs={"bits": 8}), "mm4: bits = 8 is not supported"),
    (_node(attrs={"block_size": 16}), "mm4: block_size = 16 is not supported"),
    (_node(attrs={"K": 80}, k=80), "mm4: K = 80 is not a positive multiple of block_size"),
    (_node(scales=np.float16), "mm4: scales must be a float32 initializer"),
    (_node(edit={"zero_points": np.zeros((16, 1), np.float32)}), "mm4: zero_points must be a packed UINT8 initializer"),
    (_node(edit={"g_idx": np.zeros(64, np.int32)}), "mm4: g_idx is not supported"),
    (_node(edit={"bias": np.zeros(3, np.float32)}), "mm4: bias must be a [N] float initializer"),
    (_node(edit={"B": np.zeros((16, 2, 8), np.uint8)}), "mm4: B must be a UINT8 initializer"),
    (_node(extra=(("stray", np.zeros(4, np.uint8)),)), "initializer stray: unsupported data type 2"),
), ids=lambda v: v.split(":")[1].strip()[:24] if isinstance(v, str) else "")
def test_refusals(tmp_path, monkeypatch, engine_lib, mb, why):
    with pytest.raises(RuntimeError) as e:
        _plan(tmp_path, monkeypatch, mb)
    assert why in str(e.value), str(e.value)
    assert _plan(tmp_path, monkeypatch, _node())["steps"][0]["kind"] == "qlinear"      # (the unspoiled node loads)


def test_qkv_must_agree_and_fp8_refuses(tmp_path, monkeypatch, engine_lib):
    """q / k / v Linears of different block size or zero-point presence are refused by name; fp8 refuses the graph as it refuses Llama"""
    def mixed(**k_proj):
        gb_linear = models.GraphBuilder.linear

        def linear(self, x, cin, cout, name=None, **kw):
            return gb_linear(self, x, cin, cout, name=name, **dict(kw, **(k_proj if name and name.endswith("_k_proj") else {})))
        monkeypatch.setattr(models.GraphBuilder, "linear", linear)
        try:
            return models.llama_tiny(N, quant="int4")
        finally:
            monkeypatch.setattr(models.GraphBuilder, "linear", gb_linear)
    for mb, why in ((mixed(q_block=64), "has block_size 64, the q Linear"), (mixed(q_zero=False), "has no zero points, the q Linear")):
        with pytest.raises(RuntimeError) as e:
            _plan(tmp_path, monkeypatch, mb)
        assert why in str(e.value) and "the k Linear matmulnbits_" in str(e.value), str(e.value)
    with pytest.raises(RuntimeError):
        _plan(tmp_path, monkeypatch, models.llama_tiny(N, quant="int4"), prec="fp8")
