"""CPU: every entry of the case tables of tests/test_kernel_maps_gpu.py plans onto the kernel family, tile and split-K it names (the
planner's eligibility predicates decide; no GPU is needed to see that), and the table of random shapes is the one
test_gpu_parity._random_conv_graph draws."""
import os

import numpy as np
import pytest

import kernel_graphs as G
import test_kernel_maps_gpu as M
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models


def planned(tmp_path, case, env, prec):
    d = M.build(case)
    path = models.write_repo(str(tmp_path), "k", d["model"])
    env = dict(env, **(dict(IE_PRECISION="fp16") if prec == "fp16" else {}))
    st = M.conv_step(M.with_env(env, lambda: B.DescribeModel(path, d["ishape"][0])["plan"]["steps"]))
    return st["algo"], st["tile"], st["splitk"]


def forced(algo, tile, **more):
    return dict(IE_FORCE_ALGO=algo, IE_FORCE_TILE=str(tile), **more)


def test_igemm_tables(tmp_path):
    for t in range(16):
        for case in M.IGEMM32:
            assert planned(tmp_path, case, forced("igemm", t), "fp32")[:2] == ("igemm_vec", t), (t, case)
        for case in M.SCALAR32:
            a, pt, _ = planned(tmp_path, case, forced("scalar", t), "fp32")
            assert a == "igemm_scalar" and (pt == t if t < M.NUM_IGEMM_BASE_TILES else pt < M.NUM_IGEMM_BASE_TILES), (t, case, a, pt)
    for t in range(11):
        for case in M.IGEMM16:
            assert planned(tmp_path, case, forced("igemm", t), "fp16")[:2] == ("igemm_vec", t), (t, case)
    for sk in (2, 3, 7):
        for prec in ("fp32", "fp16"):
            for case in M.SPLITK:
                assert planned(tmp_path, case, forced("igemm", 4, IE_FORCE_SPLITK=str(sk)), prec) == ("igemm_vec", 4, sk), (sk, prec, case)


def test_3x3_tables(tmp_path):
    for t in range(8):
        for sk in (1, 2):
            for case in M.RASTER:
                assert planned(tmp_path, case, forced("raster", t, IE_FORCE_SPLITK=str(sk)), "fp32") == ("raster3x3", t, sk), (t, case)
    for t in range(12):
        for case in M.WINO:
            assert planned(tmp_path, case, forced("wino", t, IE_FP32_SPLIT="1"), "fp32")[:2] == ("wino3x3", t), (t, case)
    for t in range(5):
        for case in M.WS16_3X3:
            assert planned(tmp_path, case, forced("ws", t), "fp16")[:2] == ("ws3x3", t), (t, case)


def test_1x1_tables(tmp_path):
    for t in range(20):
        for case in M.ws32_cases(t):
            assert planned(tmp_path, case, forced("ws", t), "fp32")[:2] == ("ws1x1", t), (t, case)
    for t in range(18):
        for case in M.ws16_cases(t):
            assert planned(tmp_path, case, forced("ws", t), "fp16")[:2] == ("ws1x1", t), (t, case)
    for t in (10, 11, 12, 13, 14):
        for case in M.as_cases(t):
            assert planned(tmp_path, case, forced("direct", t), "fp32")[:2] == ("direct", t), (t, case)
    for t in (0, 1):
        for case in M.X6:
            assert planned(tmp_path, case, forced("x6", t, IE_FP32_SPLIT="1"), "fp32")[:2] == ("conv1x1_x6", t), (t, case)


def test_direct_tables(tmp_path):
    for prec in ("fp32", "fp16"):
        for t in range(6):
            for case in M.direct_cases(t, prec):
                assert planned(tmp_path, case, forced("direct", t), prec)[:2] == ("direct", t), (t, prec, case)
    for t in (6, 7, 8, 9):
        for case in M.WINDOW:
            assert planned(tmp_path, case, forced("direct", t), "fp32")[:2] == ("direct", t), (t, case)
    for prec in ("fp32", "fp16"):
        for case in M.NAIVE:
            assert planned(tmp_path, case, dict(IE_FORCE_ALGO="naive"), prec)[0] == "naive"


def test_random_shapes_are_the_parity_tests(tmp_path):
    import test_gpu_parity as T
    rs = np.random.RandomState(1000)
    for i in range(14):
        _, ishape, _, d = T._random_conv_graph(rs, i)
        rs.rand(*ishape)
        assert M.RANDOM14[i] == (ishape[0], d["k"], d["stride"], d["pad"], d["cin"], d["cout"], d["h"], d["w"], int(d["pre"]), d["post"], int(d["bias"]))
        for prec in ("fp32", "fp16"):
            planned(tmp_path, M.random14_case(i), {}, prec)          # plans, whatever the choice


def test_two_stage_tables(tmp_path):
    for seed, n, h, w, c0, layers in M.DENSE32:
        d = G.dense_case(seed, n, h, w, c0, layers, tail=True, expose=True)
        path = models.write_repo(str(tmp_path), "k", d["model"])
        for pb_, tile in (("", 1 if n * h * w <= 2048 else 2), ("3", 3), ("4", 4), ("5", 5)):
            env = dict(IE_AUTOTUNE="0", **(dict(IE_FUSE_PB=pb_) if pb_ else {}))
            steps = M.with_env(env, lambda: B.DescribeModel(path, n)["plan"]["steps"])
            assert [s["tile"] for s in steps if s.get("algo") == "dense_fused"] == [tile] * layers, (seed, pb_)
    assert {1, 2} == {1 if n * h * w <= 2048 else 2 for _, n, h, w, _, _ in M.DENSE32}          # both pixel-tile sizes of the default variant
    chained = 0
    for seed, n, h, w, c0, layers in M.DENSE16:
        d = G.dense_case(seed, n, h, w, c0, layers, tail=False, expose=False)
        path = models.write_repo(str(tmp_path), "k", d["model"])
        steps = M.with_env(dict(IE_AUTOTUNE="0", IE_PRECISION="fp16"), lambda: B.DescribeModel(path, n)["plan"]["steps"])
        per = [len(s["parts"]) // 2 for s in steps if s.get("algo") == "dense_block" and s["tile"] != 0]
        assert sum(per) == layers, (seed, per)
        chained += max(per) > 1
    assert chained >= 2          # launches that walk several layers, not only single-layer ones
