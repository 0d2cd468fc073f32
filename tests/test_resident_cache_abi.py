"""CPU: the resident KV cache calls of include/inference_engine_ext.h are exported, refuse a NULL handle with a message without touching a device, and
leave the plans of the graphs they bind to what a build of the parent commit gave (tests/golden/resident_parent_plans.json: the digests of
test_plan_digests.digest for the narrow decode graph and the narrow extend graph, fp32 and fp16): binding is a run-time matter, not a graph form."""
import ctypes as C
import itertools
import json
import os
import subprocess

import numpy as np
import pytest

import kv_graphs as KG
import test_plan_digests as TPD
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models

SYMBOLS = ["EngineKvCacheCreate", "EngineKvCacheDestroy", "EngineKvCacheBind", "EngineKvCacheGetLengths", "EngineKvCacheSetLengths", "EngineKvCacheRead",
           "EngineKvCacheWrite"]


def test_the_cache_calls_are_exported(engine_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", engine_lib], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert not set(SYMBOLS) - exported, set(SYMBOLS) - exported
    assert B.KV_CACHE_SYMBOLS == SYMBOLS and set(SYMBOLS) <= set(B.EXT_SYMBOLS)
    B._kv_lib()                                                         # ctypes binds all of them


def test_a_null_handle_is_refused_with_a_message(engine_lib):
    L = B._kv_lib()
    buf = np.zeros(4, np.float32)
    lens = (C.c_int64 * 2)(0, 0)
    calls = {
        "Bind": lambda e: L.EngineKvCacheBind(None, None, e),
        "GetLengths": lambda e: L.EngineKvCacheGetLengths(None, lens, e),
        "SetLengths": lambda e: L.EngineKvCacheSetLengths(None, lens, e),
        "Read": lambda e: L.EngineKvCacheRead(None, 0, 0, buf.ctypes.data, buf.nbytes, e),
        "Write": lambda e: L.EngineKvCacheWrite(None, 0, 0, buf.ctypes.data, buf.nbytes, e),
    }
    for name, call in calls.items():
        err = C.c_void_p()
        assert not call(C.byref(err)), name
        msg = B._take_error(err)
        assert msg == ("Invalid model handle" if name == "Bind" else "Invalid KV cache handle"), (name, msg)
        assert not call(None), name                                     # the error pointer may be NULL
    L.EngineKvCacheDestroy(None)
    assert not buf.any() and list(lens) == [0, 0]
    # no geometry, no cache: refused before any device is asked for
    err = C.c_void_p()
    assert not L.EngineKvCacheCreate(0, 0, 2, 2, 12, 32, C.byref(err))
    assert "must be positive" in B._take_error(err)
    if not B.IsCUDAAvailable():
        with pytest.raises(RuntimeError, match="no HIP device 0"):
            B.KvCache(2, 2, 2, 12, 32)


def test_the_plans_of_the_graphs_that_bind_are_the_parents(tmp_path, engine_lib):
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resident_parent_plans.json")) as f:
        parent = json.load(f)
    cases = {"narrow_decode": lambda: KG.narrow(seq=1, past=KG.NARROW_P), "narrow_extend": lambda: KG.narrow(seq=4, past=KG.NARROW_P)}
    assert sorted(parent) == sorted(f"{n}/{p}" for n, p in itertools.product(cases, ("fp32", "fp16")))
    for name, mk in cases.items():
        path = models.write_repo(str(tmp_path), name, mk())
        for prec in ("fp32", "fp16"):
            d = TPD.digest(path, KG.NARROW_N, {"IE_PRECISION": prec})
            assert " ".join(d[k] for k in ("plan", "weights") if k in d) == parent[f"{name}/{prec}"], (name, prec)
