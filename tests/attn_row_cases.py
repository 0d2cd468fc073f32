"""The data of the per-row attention tests (tests/test_attn_ref.py on the CPU, tests/test_attn_rows_gpu.py on the GPU): for one attention step the
graph, the feeds of both data kinds and the attn_ref.Step of each, so that the CPU test holds the yardstick to itself on the very data the GPU test
runs.  N = 2, H = 4.

Data kinds.  "even": N(0, 1) rows and cache, a flat softmax.  "peaked": the q columns times attn_ref.Q_GAIN (scores of about +-10) and the cached
keys of every (image, K / V head) sorted by one query's score, ascending or descending (attn_ref.peaked).  Both kinds of a cache step run on ONE
model: the `rows` initializer holds the flat rows and behind them their peaked copies, and the ids pick one or the other.

The cos / sin tables of the cache steps have independent random values in both halves of a row (llama_graphs.random_tables), the positions differ
per image and run backwards inside a chunk, as in tests/test_extend_gpu.py.  A causal prefill takes true rope tables (peaked_prefill must undo
the rotation)."""
from __future__ import annotations

import functools

import numpy as np

import attn_ref as AR
import extend_graphs as EG
import kv_graphs as KG
import llama_graphs as LG
from gpu_ai_inference_server_amd.modelgen import models

N, H = 2, 4
ROWS = 7
MAX_POS = 64
KINDS = ("even", "peaked")


class Case:
    """mb: the graph; feeds[kind]; tok[kind]: the token rows [N, Lq, C] float32 the ids pick; lens[kind], new[kind]; step(kind, prec) -> attn_ref.Step
    from the operands the kernel is given under that precision; ref() and yard() -> its reference and c_emul, computed once"""

    def __init__(self, form, mb, h, kvh, hd, past, lq, tables):
        self.form, self.mb, self.h, self.kvh, self.hd, self.past, self.lq, self.tables = form, mb, h, kvh, hd, past, lq, tables
        self.feeds, self.tok, self.lens, self.new, self.pos = {}, {}, {}, {}, {}
        self._steps, self._yard = {}, {}

    def step(self, kind, prec="fp32"):
        key = (kind, prec)
        if key not in self._steps:
            tok = self.tok[kind] if prec == "fp32" else AR.half_exact(self.tok[kind])
            if self.form == "prefill":
                self._steps[key] = AR.prefill_step(tok, self.h, self.kvh, self.hd, self.tables)
            else:
                f = self.feeds[kind]
                self._steps[key] = AR.inplace_step(tok, self.h, self.kvh, self.hd, f["past_key_values.0.key"], f["past_key_values.0.value"], self.lens[kind], self.new[kind],
                                                   tables=self.tables, pos=self.pos[kind])
        return self._steps[key]

    def ref(self, kind, prec="fp32"):
        """attn_ref.reference of the step under prec, computed once"""
        key = (kind, prec)
        if key not in self._yard:
            self._yard[key] = AR.reference(self.step(kind, prec))
        return self._yard[key]

    def yard(self, kind, prec="fp32", splits=1, slots=0):
        """(reference of the step under prec, c_emul of the fp32 step at `splits` (slots: tile 4's key slots), {emulation: c}).  c_emul is the fp32
        data's in both precisions: in fp16 mode the term it scales is four orders of magnitude below the half terms"""
        ce = ("c", kind, splits, slots)
        if ce not in self._yard:
            st = self.step(kind)
            self._yard[ce] = AR.c_emul(st, self.ref(kind), AR.own_key_valid(st), splits=splits, slots=slots)
        return (self.ref(kind, prec),) + self._yard[ce]


def _seed(*v):
    return int(sum((i + 1) * 7919 * int(x) for i, x in enumerate(v)) % (2 ** 31 - 1))


@functools.lru_cache(maxsize=None)
def cache_case(kvh, hd, past, lq, lens_even, lens_peaked, new=None):
    """A decode (lq = 1) or extend step over a cache of `past` rows.  lens_*: the valid cache rows per image of each data kind; new: the valid new
    tokens per image (None: all lq).  The same Case serves the graph with a client-held cache (feeds as they are: rows at or beyond len are
    garbage behind a zero mask column) and the model bound to a resident cache (resident_graphs.fill writes NaN there)"""
    seed = _seed(kvh, hd, past, lq, *lens_even, *lens_peaked, *(new or ()))
    table = AR.token_table(H, kvh, hd, seed, ROWS)
    tables = LG.random_tables(MAX_POS, hd)
    if lq == 1:
        mb = KG.decode_attn_graph(table, N, H, kvh, hd, past, tables=tables, max_pos=MAX_POS)
    else:
        mb = EG.extend_attn_graph(table, N, H, kvh, hd, past, lq, tables=tables, max_pos=MAX_POS)
    c = Case("cache", mb, H, kvh, hd, past, lq, tables)
    r = np.random.RandomState(seed + 1)
    ids = r.randint(0, ROWS, (N, lq)).astype(np.int64)
    ck, cv = r.randn(N, kvh, past, hd).astype(np.float32), r.randn(N, kvh, past, hd).astype(np.float32)
    new = tuple(new) if new is not None else (lq,) * N
    for kind, lens in zip(KINDS, (lens_even, lens_peaked)):
        kid = ids + (ROWS if kind == "peaked" else 0)
        pos = np.array([[(ln + lq - 1 - l) % MAX_POS for l in range(lq)] for ln in lens], np.int64)
        assert lq < 2 or pos[0, 0] != pos[0, 1] - 1
        c.tok[kind], c.lens[kind], c.new[kind], c.pos[kind] = table[kid], tuple(lens), new, pos
        k2, v2 = ck, cv
        if kind == "peaked":
            k2, v2 = AR.peaked(AR.cache_step(table[kid], H, kvh, hd, ck, cv, tables=tables, pos=pos), lens, ck, cv)
        c.feeds[kind] = {"input_ids": kid, "attention_mask": AR.resident_mask(lens, new, past, lq), "position_ids": pos,
                         "past_key_values.0.key": k2, "past_key_values.0.value": v2}
    return c


@functools.lru_cache(maxsize=None)
def prefill_case(kvh, hd, l):
    """llama_graphs.gqa_attn_graph, causal with rope: x [N, C, 1, L]"""
    tables = models.rope_tables(l, hd)
    mb = LG.gqa_attn_graph(N, l, H, kvh, hd, rope="init")
    c = Case("prefill", mb, H, kvh, hd, 0, l, tables)
    x = LG.gqa_input(N, l, H, kvh, hd)
    tok = np.ascontiguousarray(x[:, :, 0, :].transpose(0, 2, 1))
    for kind in KINDS:
        t = tok if kind == "even" else AR.peaked_prefill(tok, H, kvh, hd, tables)
        c.tok[kind] = t
        c.feeds[kind] = {"x": np.ascontiguousarray(t.transpose(0, 2, 1)[:, :, None, :])}
    return c


def out_rows(y, case):
    """an `out` [N, Lq, D] (a prefill's y [N, D, 1, L]) as [N, Lq, H, hd]"""
    y = np.asarray(y)
    if case.form == "prefill":
        y = y[:, :, 0, :].transpose(0, 2, 1)
    return y.reshape(N, case.lq, case.h, case.hd)


# ---- the cases of tests/test_attn_rows_gpu.py (the CPU test takes its data from the same lists) ----------------------------------------------------
def lens_pair(past):
    """(even lengths, peaked lengths) of a case that exists today: the peaked data keep today's (3, P)"""
    return tuple(AR.even_lengths(past)), (min(3, past), past)


DECODE = [(kvh, hd, KG.key_tile(hd) + d) for hd in (32, 64, 128) for kvh in (4, 1) for d in (-1, 1)]
EXTEND = [(hd, p, lq) for hd in (32, 64) for p, lq in ((33, 5), (255, 5), (257, 5), (40, 65))]
PREFILL = [(1, 2, 64, 40), (1, 2, 32, 129), (3, 2, 64, LG.KC + 8), (2, 2, 128, 40)]      # (tile, kvh, hd, L)
