"""Helpers of the resident KV cache tests (tests/test_resident_cache_abi.py, tests/test_resident_cache_gpu.py): a session that holds models bound to one
B.KvCache under an environment, requests on a bound model, the cache image a test writes (rows at or beyond an image's length are NaN, so any read
beyond `len` poisons what it feeds) and the float64 reference on the equivalent right-padded client-held cache, mirrors of the in-place kernel labels."""
from __future__ import annotations

import contextlib
import os

import numpy as np

import extend_graphs as EG  # noqa: F401  (registers Where in ref64.OPS)
import kv_graphs as KG
from engine_run import tensor
from gpu_ai_inference_server_amd import binding as B


def bits(x: np.ndarray) -> np.ndarray:
    """float32 values as their bit patterns: NaN rows compare equal bit for bit"""
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def nan_beyond(cache: np.ndarray, lens) -> np.ndarray:
    """a copy of [N, Hkv, P, hd] whose rows at or beyond lens[n] are NaN"""
    out = np.array(cache, np.float32, copy=True)
    for n, ln in enumerate(lens):
        out[n, :, ln:] = np.nan
    return out


def decode_label(tile: int, f16: bool, hd: int, splits: int = 1) -> str:
    """launch.cpp kernel_label of a decode attention step bound to a cache"""
    t = "f16" if f16 else "f32"
    if tile == KG.DECODE_TILE:
        return "attention_decode_kernel<%s,%d,inplace>" % (t, hd) + (" + attention_decode_combine_kernel" if splits > 1 else "")
    return "kv_append_rows_kernel + attention_inplace_generic_kernel<%s>" % t


def extend_label(tile: int, f16: bool, hd: int, splits: int = 1) -> str:
    """launch.cpp kernel_label of an extend step bound to a cache"""
    t = "f16" if f16 else "f32"
    if tile == EG.EXTEND_TILE:
        return "kv_append_rows_kernel + attention_extend_kernel<%s,%d,inplace>" % (t, hd) + (" + attention_extend_combine_kernel" if splits > 1 else "")
    return "kv_append_rows_kernel + attention_inplace_generic_kernel<%s>" % t


def request(m, feeds: dict, outs: dict) -> dict:
    """one request on a B.Model for the outputs {name: shape}, in the graph's output order -> {name: array}"""
    r = m.Infer([tensor(k, v) for k, v in feeds.items()], [B.OutputConfig(k, Shape=list(s), DataType="FLOAT32") for k, s in outs.items()])
    return {t.Name: t.Data.reshape(outs[t.Name]).copy() for t in r}


def unbound(feeds: dict) -> dict:
    """the feeds of a bound model: those of the graph without the cache"""
    return {k: v for k, v in feeds.items() if not k.startswith("past_key_values.")}


@contextlib.contextmanager
def session(env: dict, models_: dict, cache_dims=None, **create):
    """models_ {name: path} created under IE_AUTOTUNE=0 plus env (the variables stay set inside), and a B.KvCache(*cache_dims) every one of them is bound
    to (cache_dims None: no cache, nothing bound).  Yields ({name: model}, cache); everything is destroyed on the way out, the cache first"""
    full = dict(IE_AUTOTUNE="0", **env)
    old = {k: os.environ.get(k) for k in full}      # (engine_run.with_env scopes one call; a context manager keeps the variables for its whole body)
    os.environ.update(full)
    ms, kc = {}, None
    try:
        for name, path in models_.items():
            ms[name] = B.CreateModel(path, name, **create)
        if cache_dims is not None:
            kc = B.KvCache(*cache_dims)
            for m in ms.values():
                kc.bind(m)
        yield ms, kc
    finally:
        if kc is not None:
            kc.destroy()
        for m in ms.values():
            m.Destroy()
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def fill(kc, feeds: dict, lens, layers: int = 1) -> dict:
    """write the past_key_values.* of feeds into the cache with NaN beyond every image's length, set the lengths; -> {(layer, which): what was written}"""
    written = {}
    for layer in range(layers):
        for which, w in enumerate(("key", "value")):
            x = nan_beyond(feeds[f"past_key_values.{layer}.{w}"], lens)
            kc.write(layer, which, x)
            written[(layer, which)] = x
    kc.set_lengths(lens)
    return written

