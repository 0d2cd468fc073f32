"""GPU (-m gpu): whole BERT encoders (modelgen.models.bert) on the MI355X against the float64 walk of tests/ref64.py, with the project's bounds
(tests/test_gpu_parity.py): fp32 within 2e-4 of max|ref|, fp16 within 3e-3, for `logits` and `pooler_output`.

The narrow net: dim 64, 2 heads of 32, 2 layers, seq 40, vocab 50; batch 3 with lengths 40 / 17 / 1.  Graph replay is bit-equal to the eager run;
bert_tiny (dim 128, 2 heads of 64, seq 128, vocab 30522) runs once in fp32; with dynamic batching three concurrent callers of 1 / 2 / 3 rows each get
their own rows -- the batcher's padding rows are id 0 with mask 0, fully masked images that must not disturb them."""
import threading

import numpy as np
import pytest

import bert_graphs as G
import ref64
from engine_run import RTOL, with_env
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models

pytestmark = pytest.mark.gpu
SEQ, VOCAB, DIM = 40, 50, 64
NAMES = ("input_ids", "attention_mask", "token_type_ids")


def make_feeds(n, seq, vocab, lengths, seed=7):
    st = np.random.RandomState(seed)
    ids = st.randint(0, vocab, size=(n, seq)).astype(np.int64)
    tt = (st.rand(n, seq) < 0.5).astype(np.int64)
    mask = np.zeros((n, seq), np.int64)
    for i, ln in enumerate(lengths):
        mask[i, :ln] = 1
    return {"input_ids": ids, "attention_mask": mask, "token_type_ids": tt}


@pytest.fixture(scope="module")
def narrow(tmp_path_factory):
    """the narrow net with a symbolic batch, six rows of feeds (lengths 40 / 17 / 1 first) and their float64 outputs; computed once, read-only"""
    root = str(tmp_path_factory.mktemp("bert"))
    path = models.write_repo(root, "bert", G.narrow_bert("N"))
    feeds = make_feeds(6, SEQ, VOCAB, (40, 17, 1, 33, 8, 40))
    ref = ref64.run_f64(G.narrow_bert(6), feeds)
    for a in list(feeds.values()) + list(ref.values()):
        a.setflags(write=False)
    return path, feeds, ref


def _infer(m, feeds, lo, hi, classes=2, dim=DIM):
    n = hi - lo
    ins = [B.TensorData(k, B.DataTypeInt64, B.Shape([n, feeds[k].shape[1]]), feeds[k][lo:hi]) for k in NAMES]
    r = m.Infer(ins, [B.OutputConfig("logits", Shape=[n, classes], DataType="FLOAT32"), B.OutputConfig("pooler_output", Shape=[n, dim], DataType="FLOAT32")])
    return {"logits": r[0].Data.reshape(n, classes).copy(), "pooler_output": r[1].Data.reshape(n, dim).copy()}


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_narrow_net(narrow, prec):
    path, feeds, ref = narrow

    def go():
        m = B.CreateModel(path, "bert")
        try:
            y = _infer(m, feeds, 0, 3)
            kern = [p["kernel"] for p in B.Profile(m, 1)]
        finally:
            m.Destroy()
        t = "f16" if prec == "fp16" else "f32"
        assert kern[0] == G.embed_label(G.embed_default_tile(DIM, prec == "fp16"), prec == "fp16") and kern.count(f"attention_mfma_kernel<{t},32,mask>") == 2, kern
        for k in ("logits", "pooler_output"):
            assert np.isfinite(y[k]).all()
            err = ref64.rel_err(y[k], ref[k][:3])
            print(f"narrow BERT {prec} {k}: max err / max|ref| {err:.3e}")
            assert err < RTOL[prec], (k, err)
    with_env(dict(IE_AUTOTUNE="0", IE_PRECISION=prec), go)


def test_replay_is_bit_equal(narrow):
    path, feeds, ref = narrow

    def go():
        m = B.CreateModel(path, "bert")
        try:
            y_host = _infer(m, feeds, 0, 3)
            din, dout = B.Prepare(m, [[3, SEQ]] * 3, 2)
            for d, k in zip(din, NAMES):
                B.CopyToDevice(m, d, feeds[k][:3])
            B.RunPrepared(m, 2, True)                                              # graph replay
            y, p = np.empty((3, 2), np.float32), np.empty((3, DIM), np.float32)
            B.CopyToHost(m, y, dout[0])
            B.CopyToHost(m, p, dout[1])
            np.testing.assert_array_equal(y, y_host["logits"])
            np.testing.assert_array_equal(p, y_host["pooler_output"])
        finally:
            m.Destroy()
    with_env(dict(IE_AUTOTUNE="0", IE_PRECISION="fp32"), go)


def test_bert_tiny(tmp_path):
    mb = models.bert_tiny(2, pooler_output=True)
    path = models.write_repo(str(tmp_path), "tiny", mb)
    feeds = make_feeds(2, 128, 30522, (128, 45), seed=9)
    ref = ref64.run_f64(mb, feeds)

    def go():
        m = B.CreateModel(path, "tiny")
        try:
            y = _infer(m, feeds, 0, 2, dim=128)
            kern = [p["kernel"] for p in B.Profile(m, 1)]
        finally:
            m.Destroy()
        assert kern.count("attention_mfma_kernel<f32,64,mask>") == 2 and kern[0].startswith("embed_ln_kernel<f32,"), kern
        for k in ("logits", "pooler_output"):
            err = ref64.rel_err(y[k], ref[k])
            print(f"bert_tiny fp32 {k}: max err / max|ref| {err:.3e}")
            assert err < RTOL["fp32"], (k, err)
    with_env(dict(IE_AUTOTUNE="0", IE_PRECISION="fp32"), go)


def test_three_concurrent_callers(narrow):
    """1 + 2 + 3 rows coalesce into buckets of up to 8; the padding rows are fully masked images"""
    path, feeds, ref = narrow

    def go():
        m = B.CreateModel(path, "bert")
        try:
            assert B.BatcherStats(m)["max_batch"] == 8
            spans, out, errs = [(0, 1), (1, 3), (3, 6)], {}, []

            def call(lo, hi):
                try:
                    out[lo] = _infer(m, feeds, lo, hi)
                except Exception as e:  # noqa: BLE001
                    errs.append(e)

            before = B.BatcherStats(m)
            ts = [threading.Thread(target=call, args=s) for s in spans]
            [t.start() for t in ts]
            [t.join() for t in ts]
            assert not errs, errs
            assert B.BatcherStats(m)["coalesced_requests"] - before["coalesced_requests"] == 3
            for lo, hi in spans:
                for k in ("logits", "pooler_output"):
                    assert np.isfinite(out[lo][k]).all()
                    assert ref64.rel_err(out[lo][k], ref[k][lo:hi]) < RTOL["fp32"], (lo, hi, k)
        finally:
            m.Destroy()
    with_env(dict(IE_AUTOTUNE="0", IE_PRECISION="fp32", IE_DYNAMIC_BATCH="8", IE_BATCH_WINDOW_US="200000"), go)
