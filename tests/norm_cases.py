"""Data and case tables of the per-element normalisation tests: tests/test_norm_ref.py and tests/test_norm_rows_plan.py (CPU) and
tests/test_norm_rows_gpu.py (GPU) read the same literal tables, draw the same inputs and compute the same yardstick (tests/norm_ref.py).

Every case is one model and three requests on it.  Inputs are half-exact (an fp32 and an fp16 plan read the same numbers); gamma, beta and the
embedding tables are the fp32 initializers of the graph.  Data kinds:
  randn      mean 0.5, std 1
  mean100    mean 100, std 1
  distinct   group norm only, gn_graphs.data: every (image, group) its own mean in [-8, 8] and scale in [0.25, 4]
  near_eps   every row / (image, group) its own std of 0.3, 1 or 3 times sqrt(eps), mean 0 (RMSNorm: that rms); run with eps 1e-5 and 1e-6.  Magnitudes
             below the smallest normal half, 2^-14, are raised to it.  Embed: the word rows have those stds, type and position rows a tenth of the smallest
  edges      randn with one constant row (1.3), one row of zeros (RMSNorm: the result is exactly 0) and one row scaled so that its largest |x| is 5.9e4
A yardstick entry ("yard") is dict(ref, B, extra, ce, cs, bound): hold y to |y - ref| <= bound = MARGIN ce u B + extra, element by element."""
from __future__ import annotations

import functools
from types import SimpleNamespace as NS

import numpy as np

import bert_graphs as BG
import convnext_graphs as CG
import gn_graphs as GG
import gpt2_graphs as G2
import llama_graphs as LG
import norm_ref as NR
from engine_run import RTOL
from gpu_ai_inference_server_amd.modelgen import models
from gpu_ai_inference_server_amd.modelgen import onnx_pb as pb
from oracle import onnx_oracle as O

f32, f64 = np.float32, np.float64
PRECS = ("fp32", "fp16")
DRAWS = 3
MIN_HALF = 2.0 ** -14
NEAR_STDS = (0.3, 1.0, 3.0)
# (kind, eps) of the row kernels' cases; eps of the kinds that do not probe it is the graphs' usual 1e-5
ROW_DATA = (("randn", 1e-5), ("mean100", 1e-5), ("near_eps", 1e-5), ("near_eps", 1e-6), ("edges", 1e-5))
GN_DATA = (("randn", 1e-5), ("mean100", 1e-5), ("distinct", 1e-5), ("near_eps", 1e-5), ("near_eps", 1e-6), ("edges", 1e-5))
EMBED_DATA = (("randn", 1e-12), ("mean100", 1e-12), ("near_eps", 1e-5), ("near_eps", 1e-6))

# ---- the tables ------------------------------------------------------------------------------------------------------------------------------
N, H, W = 2, 3, 5                        # 30 pixel rows: a multiple of no tile's rows per workgroup
# layer norm: C -> the tiles a forced IE_FORCE_TILE lands on, (fp32, fp16).  6: generic only; 8: one half vector; 96: a partly idle lane group; 100: whole
# fp32 vectors, no whole half vector; 768: a full group; 1536: the largest row held in registers (fp32); 1540: past it
LN_TILES = {6: ((0,), (0,)), 8: ((0, 1, 2, 3, 4), (0, 1, 2, 3, 4)), 96: ((0, 1, 2, 3, 4), (0, 1, 2, 3, 4)), 100: ((0, 1, 2, 3, 4), (0,)),
            768: ((0, 3, 4), (0, 2, 3, 4)), 1536: ((0, 4), (0, 3, 4)), 1540: ((0,), (0,))}
# RMSNorm: (L, D) -> tiles (fp32, fp16); the norm runs in place, and out of place with tail "add"
RMS_TILES = {(5, 64): ((0, 1, 2, 3, 4), (0, 1, 2, 3, 4)), (33, 256): ((0, 2, 3, 4), (0, 1, 2, 3, 4)), (7, 50): ((0,), (0,))}
RMS_ADD = (33, 256)
LN_CONCAT_TILES = {6: ((0,), (0,)), 8: ((0, 1, 2, 3, 4), (0, 1, 2, 3, 4))}
# group norm (N, C, H, W, G) -> may tile 1 run (fp32, fp16).  The first nine are test_groupnorm_gpu.SHAPES.  (1, 512, 3, 3, 512): G = C > kGnBlock, in fp32
# CPV = 1 and NG = 4, 512 columns: two trips of the column, group and g0 loops, P = 1.  (1, 1024, 17, 17, 8): 289 pixels in 19 slabs of 16 (fp32) / 10 slabs of
# 32 (fp16), the last slab ONE pixel in both, P = 16: more slabs than P in fp32, fewer in fp16
GN_TILE1 = {(2, 32, 1, 1, 32): (True, True), (2, 32, 5, 7, 8): (True, True), (1, 64, 9, 9, 32): (True, True), (2, 128, 16, 16, 32): (True, True),
            (1, 512, 8, 8, 32): (True, True), (1, 16, 4, 4, 1): (True, True), (2, 16, 6, 6, 16): (True, True), (1, 20, 3, 3, 5): (True, False),
            (1, 64, 37, 41, 32): (True, True), (1, 512, 3, 3, 512): (True, True), (1, 1024, 17, 17, 8): (True, True)}
GN_SLABS = {(1, 64, 37, 41, 32): ((256, 6), (512, 3)), (1, 512, 3, 3, 512): ((32, 1), (64, 1)), (1, 1024, 17, 17, 8): ((16, 19), (32, 10))}   # (pixels per slab, slabs)
GN_ACTS = (None, "silu")


def gn_in_place(shape, act):
    """what the planner does with gn_graphs.gn_graph: behind a SiLU the norm overwrites the staging copy of x, its last reader; without one it writes another
    buffer; an [N, C, 1, 1] input needs no staging copy, and the graph input itself is never overwritten"""
    return act is not None and shape[2] * shape[3] > 1


GN_INPLACE = (2, 32, 9, 11, 8)


def gn_out_f16(shape, prec):
    """an [N, C, 1, 1] input needs no staging copy and no output copy: the plan is the norm alone, from the fp32 graph input to the fp32 graph output in
    either precision"""
    return prec == "fp16" and shape[2] * shape[3] > 1

# embed (N, L, V, D) -> tiles (fp32, fp16): test_embed_gpu.SHAPES
EMBED_TILES = {(2, 5, 37, 8): ((0, 1, 2, 3, 4), (0, 1, 2, 3, 4)), (2, 5, 37, 20): ((0, 1, 2, 3, 4), (0,)), (1, 3, 5, 7): ((0,), (0,)),
               (2, 4, 11, 768): ((0, 3, 4), (0, 2, 3, 4)), (1, 3, 5, 3080): ((0,), (0,))}
# the sum-only form (gpt2_graphs.embed_sum_graph), (L, V, D, pos) -> tiles
SUM_TILES = {(5, 37, 64, "gather"): ((0, 1, 2, 3, 4), (0, 1, 2, 3, 4)), (7, 37, 50, "gather"): ((0,), (0,))}


def tiles_of(table, key, prec):
    return table[key][PRECS.index(prec)]


# ---- data ------------------------------------------------------------------------------------------------------------------------------------
def to_rows(x):
    """[N, C, H, W] -> [N * H * W, C]: the pixel / token rows a row kernel walks"""
    n, c, h, w = x.shape
    return np.ascontiguousarray(x.transpose(0, 2, 3, 1).reshape(n * h * w, c))


def from_rows(r, n, h, w):
    return np.ascontiguousarray(r.reshape(n, h, w, -1).transpose(0, 3, 1, 2))


def _normal_halfs(x):
    """half-exact, magnitudes below 2^-14 raised to it"""
    x = NR.half_exact(x)
    x = np.where(np.abs(x) < MIN_HALF, np.where(x < 0, -MIN_HALF, MIN_HALF), x).astype(f32)
    assert np.abs(x[x != 0]).min() >= MIN_HALF
    return x


def rows_data(kind, rows, c, eps, draw):
    """[rows, c] float32, half-exact"""
    st = np.random.RandomState(1000 * draw + 7 * c + rows + 13 * len(kind))
    x = st.randn(rows, c)
    if kind == "randn":
        return NR.half_exact(x + 0.5)
    if kind == "mean100":
        return NR.half_exact(x + 100.0)
    if kind == "near_eps":
        s = np.array(NEAR_STDS)[(np.arange(rows) + draw) % 3] * np.sqrt(eps)
        return _normal_halfs(x * s[:, None])
    if kind == "edges":
        x = NR.half_exact(x + 0.5)
        if rows > 3:                                                                 # (a group norm of one or two groups keeps its randn rows)
            x[1] = NR.half_exact(1.3)
            x[2] = 0.0
            x[3] = NR.half_exact(x[3] * (5.9e4 / np.abs(x[3]).max()))
        assert np.abs(x).max() < 6e4
        return x
    raise ValueError(kind)


def gn_data(kind, shape, eps, draw):
    """[N, C, H, W] float32, half-exact; the rows of rows_data are the (image, group)s"""
    n, c, h, w, g = shape
    if kind == "distinct":
        return GG.data("distinct", n, c, h, w, g, seed=draw + 1)
    return rows_data(kind, n * g, (c // g) * h * w, eps, draw).reshape(n, c, h, w)


# ---- graphs of this module's own ---------------------------------------------------------------------------------------------------------------
def _replace_inits(gb, first, arrays):
    """the initializers gb.inits[first:] in order <- arrays {name: float32 array} (the graph builders draw their own; these cases need chosen ones)"""
    for k, (name, a) in enumerate(arrays.items()):
        gb.inits[first + k] = pb.tensor(name, np.ascontiguousarray(a, f32))


def _checked(mb, arrays):
    inits = O.load_model(mb).inits
    for name, a in arrays.items():
        assert np.array_equal(np.asarray(inits[name]).reshape(a.shape), a), name
    return mb


def gn_inplace_graph(n, c, h, w, groups, act="silu"):
    """gn_graphs.gn_alias_graph (x -> Conv1x1 "pre" -> group norm -> act -> Conv1x1 "post" -> y: the norm's input dies at the norm, so the step writes in
    place) with both convolutions the identity and no bias, exact in both precisions on half-exact data: x is the norm's input and y its result"""
    gb = models.GraphBuilder("gna", 33)
    eye = {"_w": np.eye(c, dtype=f32).reshape(c, c, 1, 1), "_b": np.zeros(c, f32)}
    k = len(gb.inits)
    a = gb.conv("x", c, c, 1, bias=True, name="pre")
    _replace_inits(gb, k, {"pre" + s: v for s, v in eye.items()})
    y = gb.group_norm(a, c, groups, back="shape", name="gn")
    if act == "silu":
        y = gb.silu(y)
    k = len(gb.inits)
    gb.conv(y, c, c, 1, bias=True, name="post", out="y")
    _replace_inits(gb, k, {"post" + s: v for s, v in eye.items()})
    return _checked(gb.finish([("x", [n, c, h, w])], [("y", [n, c, h, w])], opset=17), {"pre_w": eye["_w"], "post_b": eye["_b"]})


def ln_concat_exact(n, c, h, w, eps=1e-6):
    """convnext_graphs.ln_concat_graph (a = Conv1x1(x [n, 4, h, w]), y = Concat(a, layer norm of a)) with weights in {-1, -1/2, 0, 1/2, 1} and a bias in
    eighths: on inputs in sixteenths of [-4, 4] every product and every partial sum is a multiple of 1/32 below 32, exact in half in any order.
    -> (model, wm [c, 4], bias [c])"""
    st = np.random.RandomState(c)
    wm = (st.randint(-2, 3, size=(c, 4)) / 2.0).astype(f32)
    wm[np.arange(c), np.arange(c) % 4] = 1.0                                    # no all-zero filter: every channel of a varies
    bias = (st.randint(-8, 9, size=c) / 8.0).astype(f32)
    gb = models.GraphBuilder("lncat", 9)
    a = gb.conv("x", 4, c, 1, bias=True, name="pre")
    _replace_inits(gb, 0, {"pre_w": wm.reshape(c, 4, 1, 1), "pre_b": bias})
    b = gb.transpose(gb.layernorm(gb.transpose(a, (0, 2, 3, 1)), c, eps=eps, name="ln"), (0, 3, 1, 2))
    gb.nodes.append(pb.node("Concat", [a, b], ["y"], "cat", [pb.attr_int("axis", 1)]))
    return _checked(gb.finish([("x", [n, 4, h, w])], [("y", [n, 2 * c, h, w])], opset=17), {"pre_w": wm.reshape(c, 4, 1, 1), "pre_b": bias}), wm, bias


def embed_tables(v, d, types, max_pos, kind, eps):
    """word [v, d], type [types, d], position [max_pos, d] float32.  randn / mean100: the three rows of a token sum to mean 0.5 / 100 and std 1"""
    st = np.random.RandomState(v + 3 * d)
    w, t, p = st.randn(v, d), st.randn(types, d), st.randn(max_pos, d)
    if kind == "near_eps":
        s = np.array(NEAR_STDS)[np.arange(v) % 3] * np.sqrt(eps)
        w, t, p = w * s[:, None], t * (0.03 * np.sqrt(eps)), p * (0.03 * np.sqrt(eps))
    else:
        m = {"randn": 0.5, "mean100": 100.0}[kind] / 3.0
        w, t, p = (m + a / np.sqrt(3.0) for a in (w, t, p))
    return w.astype(f32), t.astype(f32), p.astype(f32)


def embed_graph(n, l, v, d, kind, eps, types=2):
    """bert_graphs.embed_graph with chosen tables and eps -> (model, word, type, position rows [l, d])"""
    word, typ, pos = embed_tables(v, d, types, l + 3, kind, eps)
    gb = models.GraphBuilder("embed", 11)
    t = models.bert_embeddings(gb, l, v, d, types=types, max_pos=l + 3, pos="const", eps=eps)
    arrays = {"word_embeddings": word, "token_type_embeddings": typ, "position_rows": pos[:l].reshape(1, l, d)}
    _replace_inits(gb, 0, arrays)
    gb.simple("Reshape", [gb.transpose(t, (0, 2, 1)), gb.init("back_shape", np.array([0, d, 1, l], np.int64))], out="y")
    mb = gb.finish([("input_ids", [n, l], pb.INT64), ("token_type_ids", [n, l], pb.INT64)], [("y", [n, d, 1, l])], opset=17)
    return _checked(mb, arrays), word, typ, pos[:l]


def embed_ids(n, l, v, draw, types=2):
    """draw 0: bert_graphs.make_ids (0, V - 1, -1, -V and a repeat); then other draws, a negative id in each"""
    if draw == 0:
        return BG.make_ids(n, l, v, types)
    st = np.random.RandomState(100 * l + v + draw)
    ids = st.randint(0, v, size=(n, l)).astype(np.int64)
    ids.ravel()[draw] -= v
    return ids, ((np.arange(n * l).reshape(n, l) + draw) % types).astype(np.int64)


# ---- cases: model, inputs, operands and yardstick --------------------------------------------------------------------------------------------------
def _yard(ref, B, ce, cs, extra):
    return dict(ref=ref, B=B, extra=extra, ce=ce, cs=cs, bound=NR.MARGIN * ce * NR.U * B + extra)


def _rows_yard(x32, ref, B, gamma, beta, eps, rms, prec, seed):
    f16 = prec == "fp16"
    ce, cs = NR.rows_c_emul(x32, ref, B, gamma, beta, eps, rms, f16, seed)
    return _yard(ref, B, ce, cs, NR.half_extra(ref, f16))


@functools.lru_cache(maxsize=None)
def ln_case(c, kind, eps):
    mb = CG.ln_graph(N, c, H, W, eps=eps)
    ini = O.load_model(mb).inits
    rows = [rows_data(kind, N * H * W, c, eps, d) for d in range(DRAWS)]
    return NS(mb=mb, name="ln", gamma=ini["ln_scale"], beta=ini["ln_B"], rows=rows, feeds=[{"x": from_rows(r, N, H, W)} for r in rows], oshape=(N, c, H, W),
              eps=eps, rms=False, c=c)


@functools.lru_cache(maxsize=None)
def ln_yard(c, kind, eps, draw, prec):
    k = ln_case(c, kind, eps)
    return _rows_yard(k.rows[draw], *NR.rows_ref(k.rows[draw], k.gamma, k.beta, eps), k.gamma, k.beta, eps, False, prec, draw)


@functools.lru_cache(maxsize=None)
def rms_case(l, d, kind, eps, tail=None):
    mb = LG.rms_graph(N, l, d, eps=eps, tail=tail)
    rows = [rows_data(kind, N * l, d, eps, dr) for dr in range(DRAWS)]
    return NS(mb=mb, name="rms", gamma=O.load_model(mb).inits["rms_weight"], beta=None, rows=rows, feeds=[{"x": from_rows(r, N, 1, l)} for r in rows],
              oshape=(N, d, 1, l), eps=eps, rms=True, c=d)


@functools.lru_cache(maxsize=None)
def rms_yard(l, d, kind, eps, draw, prec, tail=None):
    """tail "add": y = RMSNorm(x) + x, an eltwise step behind the norm: its own rounding is relative to |y| (B grows by |y|, the emulations add x in
    fp32), and an fp16 plan stores the norm's result and the sum as halfs"""
    k = rms_case(l, d, kind, eps, tail)
    x = k.rows[draw]
    ref, B = NR.rows_ref(x, k.gamma, None, eps, rms=True)
    if tail is None:
        return _rows_yard(x, ref, B, k.gamma, None, eps, True, prec, draw)
    f16 = prec == "fp16"
    y = ref + x.astype(f64)
    ce, cs = NR.rows_c_emul(x, y, B + np.abs(y), k.gamma, None, eps, True, f16, draw, post=lambda z: (z + x).astype(f32))
    return _yard(y, B + np.abs(y), ce, cs, NR.UH * (np.abs(ref) + np.abs(y)) if f16 else 0.0)


def quantised_input(n, h, w, draw):
    """[n, 4, h, w]: sixteenths in [-4, 4]"""
    return (np.random.RandomState(40 + draw).randint(-64, 65, size=(n, 4, h, w)) / 16.0).astype(f32)


@functools.lru_cache(maxsize=None)
def ln_concat_case(c):
    mb, wm, bias = ln_concat_exact(N, c, H, W)
    ini = O.load_model(mb).inits
    xs = [quantised_input(N, H, W, d) for d in range(DRAWS)]
    rows = [(to_rows(x).astype(f64) @ wm.astype(f64).T + bias.astype(f64)).astype(f32) for x in xs]
    for r in rows:
        assert np.array_equal(NR.half_exact(r), r)
    return NS(mb=mb, name="lncat", gamma=ini["ln_scale"], beta=ini["ln_B"], rows=rows, feeds=[{"x": x} for x in xs], oshape=(N, 2 * c, H, W), eps=1e-6, rms=False, c=c)


@functools.lru_cache(maxsize=None)
def ln_concat_yard(c, draw, prec):
    k = ln_concat_case(c)
    return _rows_yard(k.rows[draw], *NR.rows_ref(k.rows[draw], k.gamma, k.beta, k.eps), k.gamma, k.beta, k.eps, False, prec, draw)


@functools.lru_cache(maxsize=None)
def gn_case(shape, kind, eps, act, inplace=False):
    n, c, h, w, g = shape
    mb = gn_inplace_graph(n, c, h, w, g, act) if inplace else GG.gn_graph(n, c, h, w, g, act=act, eps=eps)
    ini = O.load_model(mb).inits
    xs = [gn_data(kind, shape, eps, d) for d in range(DRAWS)]
    return NS(mb=mb, name="gn", gamma=ini["gn_gamma"].reshape(-1), beta=ini["gn_beta"].reshape(-1), xs=xs, feeds=[{"x": x} for x in xs], oshape=shape[:4], eps=eps,
              act=act)


@functools.lru_cache(maxsize=None)
def gn_pre(shape, kind, eps, draw, prec, inplace=False):
    """(ref_z, B, c_emul, {name: c}) of the value before the activation: the same for every act, gamma and beta being drawn from the same streams"""
    n, c, h, w, g = shape
    k = gn_case(shape, kind, eps, None, inplace)
    f16 = prec == "fp16"
    ref, B = NR.gn_ref(k.xs[draw], k.gamma, k.beta, eps, g)
    px = GG.gn_slabs(n, h * w, c, f16)[0] if GG.gn_tile_fits(c, g, f16) else None
    return (ref, B) + NR.gn_c_emul(k.xs[draw], ref, B, k.gamma, k.beta, eps, g, f16, px)


def gn_yard(shape, kind, eps, draw, prec, act, inplace=False):
    ref, B, ce, cs = gn_pre(shape, kind, eps, draw, prec, inplace)
    a = NR.gn_allowance(ref, B, ce, act, prec == "fp16", RTOL[prec])
    return _yard(a["ref"], a["S"], ce, cs, a["extra"])


@functools.lru_cache(maxsize=None)
def embed_case(shape, kind, eps):
    n, l, v, d = shape
    mb, word, typ, pos = embed_graph(n, l, v, d, kind, eps)
    ini = O.load_model(mb).inits
    ids = [embed_ids(n, l, v, dr) for dr in range(DRAWS)]
    return NS(mb=mb, name="embed", gamma=ini["emb_ln_scale"], beta=ini["emb_ln_B"], word=word, typ=typ, pos=pos, ids=ids,
              feeds=[BG.embed_feeds(i, t, 2) for i, t in ids], oshape=(n, d, 1, l), eps=eps, c=d)


def _gathered(k, draw, n, l):
    ids, tt = k.ids[draw]
    return k.word[ids.ravel() % k.word.shape[0]], k.typ[tt.ravel()], np.tile(k.pos, (n, 1))


@functools.lru_cache(maxsize=None)
def embed_yard(shape, kind, eps, draw, prec):
    n, l, v, d = shape
    k = embed_case(shape, kind, eps)
    x, X, x32 = NR.embed_rows(*_gathered(k, draw, n, l))
    ref, B = NR.rows_ref(x, k.gamma, k.beta, eps, X=X)
    return _rows_yard(x32, ref, B, k.gamma, k.beta, eps, False, prec, draw)


@functools.lru_cache(maxsize=None)
def sum_case(l, v, d, pos):
    mb = G2.embed_sum_graph(N, l, v, d, pos=pos)
    ini = O.load_model(mb).inits
    p = ini["wpe"][:l] if pos == "gather" else ini["position_rows"].reshape(l, d)
    ids = [G2.gpt2_ids(N, l, v)] + [np.random.RandomState(l + v + dr).randint(0, v, size=(N, l)).astype(np.int64) for dr in (1, 2)]
    return NS(mb=mb, name="esum", word=ini["wte"], pos=p, ids=ids, feeds=[{"input_ids": i} for i in ids], oshape=(N, l, d), c=d)


@functools.lru_cache(maxsize=None)
def sum_yard(l, v, d, pos, draw, prec):
    """B = |word| + |pos|; the one emulation is the fp32 sum itself"""
    k = sum_case(l, v, d, pos)
    x, X, x32 = NR.embed_rows(k.word[k.ids[draw].ravel()], None, np.tile(k.pos, (N, 1)))
    c = NR.c_stat(x32, x, X)
    return _yard(x, X, c, {"sum": c}, NR.half_extra(x, prec == "fp16"))


# ---- what the plan and the GPU test ask of a plan ------------------------------------------------------------------------------------------------
def step_of(plan, kind):
    """the one step of that kind (an embed_sum graph has a layer norm behind the embed step: the first of the kind)"""
    return [s for s in plan["steps"] if s["kind"] == kind][0]


def force(tile, var="IE_FORCE_TILE"):
    return {var: str(tile)}


def in_place(st):
    return st["in"]["buf"] == st["out"]["buf"] and (st["in"]["c_off"], st["in"]["pitch"]) == (st["out"]["c_off"], st["out"]["pitch"])


def conclusive(yards, vector, nchw=False):
    """norm_ref.written_check on the three yards of a case -> (share of inconclusive elements, vectors without a conclusive element)"""
    t = (lambda a: a.transpose(0, 2, 3, 1)) if nchw else (lambda a: a)
    return NR.written_check([(t(y["ref"]), t(y["bound"])) for y in yards], vector)
