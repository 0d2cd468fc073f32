"""GPU (-m gpu): INT64 graph inputs through the C ABI -- payload types, sizes, the request batcher, the row-slice sharder, the device-resident entry
points -- on the embed graph of tests/bert_graphs.py (ids -> embedding sum -> LayerNormalization -> y [N, D, 1, L]) against the float64 walk of
tests/ref64.py, fp32 within 2e-4 of max|ref| (tests/test_gpu_parity.py)."""
import threading

import numpy as np
import pytest

import bert_graphs as G
import ref64
from engine_run import with_env
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models

pytestmark = pytest.mark.gpu
RTOL = 2e-4
L, V, D = 6, 23, 16


@pytest.fixture(scope="module")
def net(tmp_path_factory):
    """the graph with a symbolic batch, 8 rows of ids and the float64 result for them (computed once, shared, read-only)"""
    mb = G.embed_graph("N", L, V, D)
    path = models.write_repo(str(tmp_path_factory.mktemp("int64")), "embed", mb)
    st = np.random.RandomState(3)
    ids = st.randint(-V, V, size=(8, L)).astype(np.int64)
    tt = st.randint(0, 2, size=(8, L)).astype(np.int64)
    ref = ref64.run_f64(G.embed_graph(8, L, V, D), {"input_ids": ids, "token_type_ids": tt})["y"]
    for a in (ids, tt, ref):
        a.setflags(write=False)
    return path, ids, tt, ref


def _tensors(ids, tt, kinds=(B.DataTypeInt64, B.DataTypeInt64)):
    return [B.TensorData("input_ids", kinds[0], B.Shape(list(ids.shape)), ids), B.TensorData("token_type_ids", kinds[1], B.Shape(list(tt.shape)), tt)]


def _infer(m, ids, tt, **kw):
    n = ids.shape[0]
    r = m.Infer(_tensors(ids, tt, **kw), [B.OutputConfig("y", Shape=[n, D, 1, L], DataType="FLOAT32")])
    assert list(r[0].Shape.Dims) == [n, D, 1, L]
    return r[0].Data.reshape(n, D, 1, L)


def test_payload_types_and_sizes(net, tmp_path):
    path, ids, tt, ref = net

    def go():
        m = B.CreateModel(path, "embed")
        try:
            for kind in (B.DataTypeFloat32, B.DataTypeUint8):
                with pytest.raises(RuntimeError, match="Unsupported data type for input: input_ids"):
                    _infer(m, ids[:2], tt[:2], kinds=(kind, B.DataTypeInt64))
                with pytest.raises(RuntimeError, match="Unsupported data type for input: token_type_ids"):
                    _infer(m, ids[:2], tt[:2], kinds=(B.DataTypeInt64, kind))
            short = [B.TensorData("input_ids", B.DataTypeInt64, B.Shape([2, L]), ids[:1]), B.TensorData("token_type_ids", B.DataTypeInt64, B.Shape([2, L]), tt[:2])]
            with pytest.raises(RuntimeError, match=r"Invalid data size for input: input_ids Got: %d bytes Expected: %d bytes" % (L * 8, 2 * L * 8)):
                m.Infer(short, [B.OutputConfig("y", Shape=[2, D, 1, L], DataType="FLOAT32")])
            assert ref64.rel_err(_infer(m, ids[:2], tt[:2]), ref[:2]) < RTOL
        finally:
            m.Destroy()
        # INT64 for a float input: the same text
        fpath = models.write_repo(str(tmp_path), "test_model", models.test_model())
        f = B.CreateModel(fpath, "test_model")
        try:
            x = np.ones((1, 3), np.int64)
            with pytest.raises(RuntimeError, match="Unsupported data type for input: input"):
                f.Infer([B.TensorData("input", B.DataTypeInt64, B.Shape([1, 3]), x)], [B.OutputConfig("output", [1, 2])])
        finally:
            f.Destroy()
    with_env(dict(IE_AUTOTUNE="0", IE_PRECISION="fp32"), go)


def test_replay_is_bit_equal_and_device_resident_ids_are_clamped(net):
    """the captured graph replays to the eager run's bytes; ids written straight into the device buffer (no host check) are wrapped and clamped
    into the table: V + 100 reads row V - 1, -V - 5 reads row 0"""
    path, ids, tt, ref = net

    def go():
        m = B.CreateModel(path, "embed")
        try:
            y_host = _infer(m, ids[:4], tt[:4])
            din, dout = B.Prepare(m, [[4, L], [4, L]], 1)
            B.CopyToDevice(m, din[0], ids[:4])
            B.CopyToDevice(m, din[1], tt[:4])
            B.RunPrepared(m, 2, True)                                              # graph replay
            y = np.empty((4, D, 1, L), np.float32)
            B.CopyToHost(m, y, dout[0])
            np.testing.assert_array_equal(y, y_host)
            assert ref64.rel_err(y, ref[:4]) < RTOL
            wild, tame = ids[:4].copy(), ids[:4].copy()
            wild[0, 0], tame[0, 0] = V + 100, V - 1
            wild[3, L - 1], tame[3, L - 1] = -V - 5, 0
            B.CopyToDevice(m, din[0], wild)
            B.RunPrepared(m, 1, True)
            B.CopyToHost(m, y, dout[0])
            np.testing.assert_array_equal(y, _infer(m, tame, tt[:4]))
        finally:
            m.Destroy()
    with_env(dict(IE_AUTOTUNE="0", IE_PRECISION="fp32"), go)


def test_batcher_coalesces_integer_rows(net):
    """three concurrent callers of 1 / 2 / 3 rows share device batches (8-byte rows, zero-filled padding) and each gets its own rows"""
    path, ids, tt, ref = net

    def go():
        m = B.CreateModel(path, "embed")
        try:
            assert B.BatcherStats(m)["max_batch"] == 8
            _infer(m, ids, tt)                                       # rows == max_batch bypasses the batcher; warms the B = 8 plan
            spans, out, errs = [(0, 1), (1, 3), (3, 6)], {}, []

            def call(lo, hi):
                try:
                    out[lo] = _infer(m, ids[lo:hi], tt[lo:hi])
                except Exception as e:  # noqa: BLE001
                    errs.append(e)

            before = B.BatcherStats(m)
            ts = [threading.Thread(target=call, args=s) for s in spans]
            [t.start() for t in ts]
            [t.join() for t in ts]
            assert not errs, errs
            assert B.BatcherStats(m)["coalesced_requests"] - before["coalesced_requests"] == 3
            for lo, hi in spans:
                assert ref64.rel_err(out[lo], ref[lo:hi]) < RTOL, (lo, hi)
        finally:
            m.Destroy()
    with_env(dict(IE_AUTOTUNE="0", IE_PRECISION="fp32", IE_DYNAMIC_BATCH="8", IE_BATCH_WINDOW_US="200000"), go)


def test_sharder_slices_integer_rows(net):
    """the row-slice sharder cuts a request of 8 rows over three replicas (all on device 0): per-input row bytes are 8 L, not 4 L"""
    path, ids, tt, ref = net

    def go():
        m = B.CreateModel(path, "embed")
        try:
            assert B.ShardStats(m) == (3, 0)
            y = _infer(m, ids, tt)
            assert B.ShardStats(m) == (3, 1)
            assert ref64.rel_err(y, ref) < RTOL
        finally:
            m.Destroy()
    with_env(dict(IE_AUTOTUNE="0", IE_PRECISION="fp32", IE_SHARD_DEVICES="0,0,0"), go)
