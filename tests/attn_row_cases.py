"""The data of the per-row attention tests (tests/test_attn_ref.py on the CPU, tests/test_attn_rows_gpu.py on the GPU): for one attention step the
graph, the feeds of both data kinds and the attn_ref.Step of each, so that the CPU test holds the yardstick to itself on the very data the GPU test
runs.  N = 2, H = 4 (the G = 8 cases of the half tile 4: H = 8).

Data kinds.  "even": N(0, 1) rows and cache, a flat softmax.  "peaked": the q columns times attn_ref.Q_GAIN (scores of about +-10) and the cached
keys of every (image, K / V head) sorted by one query's score, ascending or descending (attn_ref.peaked).  Both kinds of a cache step run on ONE
model: the `rows` initializer holds the flat rows and behind them their peaked copies, and the ids pick one or the other.

The cos / sin tables of the cache steps have independent random values in both halves of a row (llama_graphs.random_tables), the positions differ
per image and run backwards inside a chunk, as in tests/test_extend_gpu.py.  A causal prefill takes true rope tables (peaked_prefill must undo
the rotation).

A case over a HALF resident cache (cache_case(..., half=True)) rounds the drawn cache to half before attn_ref.peaked sorts it: what
resident_graphs.fill writes is then exact, and the Step, the reference and the kernel see the same numbers.  The numbers it was rounded from are kept
(Case.raw, under the same permutation) for the CPU test of the roundings a half-cache entry does not list."""
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
    from the operands the kernel is given under that precision; ref() and yard() -> its reference and c_emul, computed once.  half: the cache of the
    feeds holds halves; raw[kind] = (k, v): the numbers it was rounded from"""

    def __init__(self, form, mb, h, kvh, hd, past, lq, tables, half=False):
        self.form, self.mb, self.h, self.kvh, self.hd, self.past, self.lq, self.tables, self.half = form, mb, h, kvh, hd, past, lq, tables, half
        self.feeds, self.tok, self.lens, self.new, self.pos, self.raw = {}, {}, {}, {}, {}, {}
        self._steps, self._yard = {}, {}

    def step(self, kind, prec="fp32", raw=""):
        """raw = "k" or "v" (a half-cache case): that cache operand as the numbers it was rounded from"""
        key = (kind, prec, raw)
        if key not in self._steps:
            tok = self.tok[kind] if prec == "fp32" else AR.half_exact(self.tok[kind])
            if self.form == "prefill":
                self._steps[key] = AR.prefill_step(tok, self.h, self.kvh, self.hd, self.tables)
            else:
                f = self.feeds[kind]
                ck = self.raw[kind][0] if raw == "k" else f["past_key_values.0.key"]
                cv = self.raw[kind][1] if raw == "v" else f["past_key_values.0.value"]
                self._steps[key] = AR.inplace_step(tok, self.h, self.kvh, self.hd, ck, cv, self.lens[kind], self.new[kind], tables=self.tables, pos=self.pos[kind])
        return self._steps[key]

    def resident(self, kind):
        """(lens, new): what attn_ref.kernel_keys takes for the key order of a kernel bound to the cache"""
        return self.lens[kind], self.new[kind]

    def ref(self, kind, prec="fp32"):
        """attn_ref.reference of the step under prec, computed once"""
        key = (kind, prec)
        if key not in self._yard:
            self._yard[key] = AR.reference(self.step(kind, prec))
        return self._yard[key]

    def yard(self, kind, prec="fp32", splits=1, slots=0, waves=0, hmerge=False, bound=False):
        """(reference of the step under prec, c_emul of the fp32 step at `splits` (slots: tile 4's key slots; waves: tile 6's key waves; hmerge: the
        half tile 4's butterfly; bound: the keys in the order of a kernel bound to the cache), {emulation: c}).  c_emul is the fp32 data's in both
        precisions: in fp16 mode the term it scales is four orders of magnitude below the half terms"""
        ce = ("c", kind, splits, slots, waves, hmerge, bound)
        if ce not in self._yard:
            st = self.step(kind)
            self._yard[ce] = AR.c_emul(st, self.ref(kind), AR.own_key_valid(st), splits=splits, slots=slots, waves=waves, hmerge=hmerge,
                                       resident=self.resident(kind) if bound else None)
        return (self.ref(kind, prec),) + self._yard[ce]


def _seed(*v):
    return int(sum((i + 1) * 7919 * int(x) for i, x in enumerate(v)) % (2 ** 31 - 1))


@functools.lru_cache(maxsize=None)
def cache_case(kvh, hd, past, lq, lens_even, lens_peaked, new=None, heads=H, half=False, rope=True):
    """A decode (lq = 1) or extend step over a cache of `past` rows.  lens_*: the valid cache rows per image of each data kind; new: the valid new
    tokens per image (None: all lq).  The same Case serves the graph with a client-held cache (feeds as they are: rows at or beyond len are
    garbage behind a zero mask column) and the model bound to a resident cache (resident_graphs.fill writes NaN there).  heads: the query heads;
    half: the cache holds halves, rounded before the peaked data are sorted; rope False: no rotation (the graph has no position_ids): the "rope" terms
    of attn_ref.HALF_TERMS are then absent, and the entry is held to what is left"""
    seed = _seed(kvh, hd, past, lq, *lens_even, *lens_peaked, *(new or ()))
    H = heads                                      # (the seed does not take the head count or the cache type: the existing cases keep their draws)
    table = AR.token_table(H, kvh, hd, seed, ROWS)
    tables = LG.random_tables(MAX_POS, hd) if rope else None
    how = {} if rope else {"rope": None}
    if lq == 1:
        mb = KG.decode_attn_graph(table, N, H, kvh, hd, past, tables=tables, max_pos=MAX_POS, **how)
    else:
        mb = EG.extend_attn_graph(table, N, H, kvh, hd, past, lq, tables=tables, max_pos=MAX_POS, **how)
    c = Case("cache", mb, H, kvh, hd, past, lq, tables, half)
    r = np.random.RandomState(seed + 1)
    ids = r.randint(0, ROWS, (N, lq)).astype(np.int64)
    ck, cv = r.randn(N, kvh, past, hd).astype(np.float32), r.randn(N, kvh, past, hd).astype(np.float32)
    rk, rv = ck, cv
    if half:
        ck, cv = AR.half_exact(ck), AR.half_exact(cv)
    new = tuple(new) if new is not None else (lq,) * N
    for kind, lens in zip(KINDS, (lens_even, lens_peaked)):
        kid = ids + (ROWS if kind == "peaked" else 0)
        pos = np.array([[(ln + lq - 1 - l) % MAX_POS for l in range(lq)] for ln in lens], np.int64)
        assert lq < 2 or pos[0, 0] != pos[0, 1] - 1
        c.tok[kind], c.lens[kind], c.new[kind], c.pos[kind] = table[kid], tuple(lens), new, pos
        k2, v2, c.raw[kind] = ck, cv, (rk, rv)
        if kind == "peaked":
            k2, v2, *raw = AR.peaked(AR.cache_step(table[kid], H, kvh, hd, ck, cv, tables=tables, pos=pos), lens, ck, cv, (rk, rv))
            c.raw[kind] = tuple(raw)
        c.feeds[kind] = {"input_ids": kid, "attention_mask": AR.resident_mask(lens, new, past, lq), "position_ids": pos,
                         "past_key_values.0.key": k2, "past_key_values.0.value": v2}
        if not rope:
            del c.feeds[kind]["position_ids"]
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


def wide_key_waves(rows):
    """kernels.h ExtendWideKeyWaves: tile 6's key waves for R = g Lq query rows"""
    return 4 if rows <= 32 else (2 if rows <= 64 else 1)


def half_key_tile(hd):
    """kernels.h DecodeKeyTileHalf: the keys of the half tile 4 per iteration"""
    return AR.HALF_TILE_ELEMS // hd


# ---- the cases of tests/test_attn_rows_gpu.py (the CPU test takes its data from the same lists) ----------------------------------------------------
def lens_pair(past):
    """(even lengths, peaked lengths) of a case that exists today: the peaked data keep today's (3, P)"""
    return tuple(AR.even_lengths(past)), (min(3, past), past)


DECODE = [(kvh, hd, KG.key_tile(hd) + d) for hd in (32, 64, 128) for kvh in (4, 1) for d in (-1, 1)]
EXTEND = [(hd, p, lq) for hd in (32, 64) for p, lq in ((33, 5), (255, 5), (257, 5), (40, 65))]
EXTEND_WIDE = [(33, 5), (127, 5), (129, 5), (40, 17), (40, 65)]      # (P, Lq) at hd 128, kvh 2: R = 10 (KW 4), the 128-key chunk -+ 1, R = 34 (KW 2), R = 130 (KW 1)
DECODE_HALF = [(kvh, hd, half_key_tile(hd) + d) for hd in (32, 64, 128) for kvh in (4, 1) for d in (-1, 1)]      # (kvh, hd, P): the half key tile -+ 1
# tile 6 bound to a cache, (cache rows, Lq, lens, new, splits): three splits round the 128-key chunk, two row blocks, a ragged c
WIDE_BOUND = ([(300, 8, lens, None, 3) for lens in ((3, 292), (127, 128), (129, 290))] + [(110, 65, (3, 40), None, s) for s in (1, 3)]
              + [(40, 5, lens, (0, 5), 1) for lens in ((7, 30), (0, 30))])


def wide_case(past, lq, lens=None, new=None, half=False, rope=True):
    """tile 6's data: hd 128, kvh 2; lens None: the pair of a client-held cache"""
    return cache_case(2, 128, past, lq, *(lens_pair(past) if lens is None else (lens, lens)), new=new, half=half, rope=rope)


def decode_half_case(kvh, hd, past, heads=H, rope=True):
    """a decode step over a half cache of P + 1 rows, so that the image that holds P rows can append"""
    return cache_case(kvh, hd, past + 1, 1, *lens_pair(past), heads=heads, half=True, rope=rope)


# half-cache cases WITHOUT a rotation, (tile, cache_case arguments, splits): the entries "0h", "4h", "5h", "6h" reduced to their unconditional terms
NO_ROPE_HALF = [(0, (4, 64, 34, 1, (28, 33), (28, 33)), 1), (4, (4, 64, 34, 1, (28, 33), (28, 33)), 1), (4, (1, 32, 66, 1, (60, 65), (60, 65)), 1),
                (5, (2, 64, 300, 8, (255, 256), (255, 256)), 3), (6, (2, 128, 300, 8, (129, 290), (129, 290)), 3)]


def no_rope_half_case(args):
    return cache_case(*args, half=True, rope=False)


PREFILL = [(1, 2, 64, 40), (1, 2, 32, 129), (3, 2, 64, LG.KC + 8), (2, 2, 128, 40)]      # (tile, kvh, hd, L)
