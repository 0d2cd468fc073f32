"""CPU: the typed creation call of the resident KV cache (include/inference_engine_ext.h EngineKvCacheCreateTyped) is exported, refuses an
unknown dtype by name before any device is asked for, and B.KvCache passes its dtype through."""
import ctypes as C
import subprocess

import pytest

from gpu_ai_inference_server_amd import binding as B


def test_the_typed_call_is_exported(engine_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", engine_lib], capture_output=True, text=True, check=True).stdout
    assert "EngineKvCacheCreateTyped" in {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert "EngineKvCacheCreateTyped" in B.EXT_SYMBOLS and "EngineKvCacheCreateTyped" not in B.KV_CACHE_SYMBOLS


@pytest.mark.parametrize("dtype", (b"f8", b"fp16", b"", None))
def test_an_unknown_dtype_is_refused_by_name(engine_lib, dtype):
    """device 99 does not exist on any machine: the dtype is refused first, so the message is the dtype's"""
    create = B._kv_lib().EngineKvCacheCreateTyped
    err = C.c_void_p()
    assert not create(99, 1, 2, 2, 12, 32, dtype, C.byref(err))
    msg = B._take_error(err)
    assert msg == 'EngineKvCacheCreateTyped: unknown dtype "%s" (a resident cache stores "f32" or "f16")' % (dtype or b"").decode(), msg
    assert not create(99, 1, 2, 2, 12, 32, dtype, None)                          # the error pointer may be NULL


@pytest.mark.parametrize("dtype", ("f32", "f16"))
def test_a_known_dtype_reaches_the_geometry_and_device_checks(engine_lib, dtype):
    err = C.c_void_p()
    assert not B._kv_lib().EngineKvCacheCreateTyped(0, 0, 2, 2, 12, 32, dtype.encode(), C.byref(err))
    assert B._take_error(err).startswith("EngineKvCacheCreateTyped: layers, batch, kv_heads, capacity and head_dim must be positive")
    with pytest.raises(RuntimeError, match="EngineKvCacheCreateTyped: no HIP device 99"):
        B.KvCache(1, 2, 2, 12, 32, 99, dtype)


def test_kvcache_passes_its_dtype_through(engine_lib):
    with pytest.raises(RuntimeError, match='unknown dtype "bf16"'):
        B.KvCache(1, 2, 2, 12, 32, 99, "bf16")
    with pytest.raises(RuntimeError, match='unknown dtype "f64"'):
        B.KvCache(1, 2, 2, 12, 32, dtype="f64")
