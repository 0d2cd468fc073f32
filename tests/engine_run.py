"""The one way the tests run the engine: an environment scope, single-input inference on a loaded model, a whole model run that reports the
launched kernels, and the plan of a model under a precision.  RTOL is the bound of tests/test_gpu_parity.py per precision, of max|ref|."""
from __future__ import annotations

import os

import numpy as np

from gpu_ai_inference_server_amd import binding as B

RTOL = {"fp32": 2e-4, "fp16": 3e-3}


def with_env(env, fn):
    """fn() with the variables of env set; the previous values (unset ones included) are back afterwards"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def tensor(name, x):
    """a request tensor: INT64 for an int64 array, else FLOAT32"""
    return B.TensorData(name, B.DataTypeInt64 if x.dtype == np.int64 else B.DataTypeFloat32, B.Shape(list(x.shape)), x)


def infer(m, feeds, oname, oshape):
    """one request on a B.Model: feeds {input name: array} -> the fp32 output oname, reshaped (a copy)"""
    r = m.Infer([tensor(k, v) for k, v in feeds.items()], [B.OutputConfig(oname, Shape=list(oshape), DataType="FLOAT32")])
    return r[0].Data.reshape(oshape).copy()


def run_model(path, name, env, feeds, oname, oshape, *, by_step=False):
    """A model of its own under IE_AUTOTUNE=0 plus env: create, infer, B.Profile(m, 1), destroy.
    feeds: {input name: array} -> (output, kernels); a list of them (several requests on the one model) -> ([output per request], kernels).
    kernels: the launched kernel of every step in plan order; by_step: (step name, kernel) pairs instead (dict() of them looks up by step)"""
    def go():
        m = B.CreateModel(path, name)
        try:
            ys = [infer(m, f, oname, oshape) for f in (feeds if isinstance(feeds, list) else [feeds])]
            prof = B.Profile(m, 1)
            kern = [(p["name"], p["kernel"]) if by_step else p["kernel"] for p in prof]
            return (ys if isinstance(feeds, list) else ys[0]), kern
        finally:
            m.Destroy()
    return with_env(dict(IE_AUTOTUNE="0", **env), go)


def describe_model(path, batch, monkeypatch, prec="fp32", **env):
    """B.DescribeModel(path, batch) under IE_PRECISION=prec with no forced tile / algorithm / split-K, plus env (plan tests: the fixture undoes it)"""
    monkeypatch.setenv("IE_PRECISION", prec)
    for k in ("IE_FORCE_TILE", "IE_FORCE_ALGO", "IE_FORCE_SPLITK"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return B.DescribeModel(path, batch)


def describe(path, batch, monkeypatch, prec="fp32", **env):
    """the plan of describe_model()"""
    return describe_model(path, batch, monkeypatch, prec, **env)["plan"]


def plan_of(path, batch, env):
    """the plan of a model under env, without a fixture (GPU tests)"""
    return with_env(env, lambda: B.DescribeModel(path, batch)["plan"])
