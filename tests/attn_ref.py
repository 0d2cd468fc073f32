"""Per-element reference and error bound for ONE attention step (numpy only; test infrastructure, in the style of tests/kernel_ref.py).

A step is described by the operands its kernel is given (Step): the q | k | v token rows as float32 numbers (fp16 mode: as the halves the step
receives), the cache rows, the cos / sin table rows of every query and of every new key, the key mask's bias (1 - mask) * constant and, for every
query row, the set J of keys it may see.  Four builders make a Step: prefill_step (causal), cache_step (a decode step, and an extend step with its
past P and the chunk index) and inplace_step (a resident cache with its (len, c) per image).

reference() gives, per output element (n, i, h, e), in float64:

    q', k'    rotated: x' = x cos + rotate_half(x) sin  (a cache row is stored rotated: its cos is 1 and its sin 0)
    s_j       = scale * q' . k'_j + bias_j,   p = softmax of s over J,   ref_e = sum_j p_j v_je
              (a bias of finfo.min absorbs the score in float64 as it does in the graph: a row whose visible keys are all masked is the uniform
              average of their V rows, and next to one unmasked key a masked one weighs exp(-3.4e38) = 0; the graph's own sum also runs over
              the chunk's future keys, which only shows in a row without any unmasked key, and no client reads such a row)
    Sv_e      = sum_j p_j |v_je|
    A_j       = scale * sum_e |q'|_e |k'_j|_e + |s_j - max_J s|,   |x'|_e = |x_e| |cos_e| + |x_partner| |sin_e|
    D_e       = sum_j p_j A_j |v_je - ref_e|
    B_e       = Sv_e + D_e                   the scale every fp32 rounding of the step is proportional to
    E_e       = sum_j p_j |v_je - ref_e|     (<= 2 Sv_e) what a relative error of the exponential is proportional to
    Dqk_e     = sum_j p_j (scale * sum_e |q'|_e |k'_j|_e) |v_je - ref_e|      what a relative error of q or of k is proportional to

Why B: a relative error d_j of p_j moves ref_e by sum_j p_j d_j (v_je - ref_e) (the common factor of numerator and denominator cancels, which is
also why the rescaling factors alpha of an online softmax and the weights of a split combine cancel: they multiply both).  d_j is the score's error,
and the score's error is the dot product's and the rotation's roundings (u times the first term of A_j) plus the fp32 product (s_j - m) * log2 e in
front of the hardware exp2 (u times the second term).  The accumulation of P V adds u * Sv.

    c(y) = max_e |y_e - ref_e| / (u B_e),  u = 2^-24.

Admissible error in fp32, element by element:

    |y - ref| <= MARGIN * c_emul * u * B + EXP_ULP * 2u * E

c_emul comes from the emulations below on the test's own data (c_emul()): an fp32 FMA chain over the head dim for the scores, the online softmax
in key tiles of 32 with exp2(float32(x * log2 e)), an fp32 FMA chain for P V; the same with a seeded random order of the head dim and of the key
tiles; for split kernels the records (m, l, o) of consecutive runs of key tiles, combined in split order.  MARGIN = 2 as in kernel_ref and for the
same reason: the emulation fixes one summation order and the kernel uses another, both are samples of one rounding walk and the statistic is a
maximum.  The emulations round exp2 correctly; the hardware instruction does not.  EXP_ULP = 1: the CDNA3 / CDNA4 instruction set reference gives
V_EXP_F32 an accuracy of 1 ULP (= 2u relative); every p_j carries one such error, hence the term 2u E.  It is read off the manual, not fitted.

fp16 mode (u_h = 2^-11) adds derived terms per kernel, HALF_TERMS below, read off the kernels' text:

    out   u_h |ref|   the output is a half tensor
    v, p  u_h Sv      each, for a V or a P that the kernel rounds to half
    q, k  u_h Dqk     each, for a q or a k that the kernel rounds itself (a rotated one, or an fp32 cache row staged as half)

An operand that arrives as an exact half adds nothing (in fp16 mode the token rows are halves already: the reference is computed from them).

Appended rows (appended_check): a v row and an unrotated k row are float32(operand) bit for bit.  A rotated k element is
fl(x cos + fl(+-x_p sin)): the product carries (1 + d1), the FMA (1 + d2), |d| <= u, so the error is at most
u |x_p sin| + u |x cos + x_p sin| (1 + u) <= 2u (|x||cos| + |x_p||sin|) (1 + u): the coefficient is 2u.

Two data builders (token_table, peaked) give the tests a softmax that is not flat, and even_lengths the lengths of the "even" data.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
UH = 2.0 ** -11
MARGIN = 2.0
EXP_ULP = 1.0                       # V_EXP_F32: 1 ULP (instruction set reference); 1 ULP = 2u
TILE = 32                           # keys per tile of the emulated online softmax
FLT_MAX = float(np.finfo(np.float32).max)
LOG2E = np.float32(1.4426950408889634)

f32, f64 = np.float32, np.float64

# Which operands a kernel rounds to half in fp16 mode, from its text (csrc/kernels_decode.hip, kernels_attn.hip, attn_mfma.h).  "rope": only when
# the step rotates (without a rotation the half operand passes as it is).
#   tile 0   attend_wave / attention_generic_kernel: operands are converted to float, all arithmetic fp32, the result is stored as T
#   tile 4   attention_decode_kernel: q rotated and kept in fp32 registers, the cache read as fp32, the result stored as T (the combine likewise)
#   tile 5   attention_extend_kernel: q rotated in fp32 and rounded to half (q8), K and V of the fp32 cache rounded where they enter LDS, the
#            probabilities rounded in front of the PV MFMA (pb), the result stored as T
#   tiles 1, 2, 3   rope_rot rounds the rotated q and k once; V is the half input as it is; the probabilities are rounded (pb); the result is T
HALF_TERMS = {
    0: dict(out=True, q=False, k=False, v=False, p=False),
    4: dict(out=True, q=False, k=False, v=False, p=False),
    5: dict(out=True, q="rope", k=True, v=True, p=True),
    1: dict(out=True, q="rope", k="rope", v=False, p=True),
    2: dict(out=True, q="rope", k="rope", v=False, p=True),
    3: dict(out=True, q="rope", k="rope", v=False, p=True),
}


def half_exact(a):
    return np.asarray(a, f32).astype(np.float16).astype(f32)


# ---------------------------------------------------------------------------------------------------------------------
# the operands of a step
# ---------------------------------------------------------------------------------------------------------------------
class Step:
    """q [N, Lq, H, hd]; k, v [N, Hkv, Lk, hd] (cache rows first, then the new tokens' rows, k UNROTATED); qcos / qsin [N, Lq, hd] and kcos / ksin
    [N, Lk, hd] or None; bias [N, Lk] float64; vis [N, Lq, Lk] bool; scale (a float32 number); past = the index of the first new key.
    All floating-point operands are float64 arrays that hold float32 (or half) numbers."""

    def __init__(self, q, k, v, vis, bias=None, scale=None, qcos=None, qsin=None, kcos=None, ksin=None, past=0):
        self.q, self.k, self.v = (np.asarray(t, f64) for t in (q, k, v))
        self.vis = np.asarray(vis, bool)
        n, lq, h, hd = self.q.shape
        lk = self.k.shape[2]
        self.bias = np.zeros((n, lk), f64) if bias is None else np.asarray(bias, f64)
        self.scale = float(f32(1.0 / np.sqrt(hd))) if scale is None else float(f32(scale))
        self.rope = qcos is not None
        one, zero = np.ones((n, 1, hd), f64), np.zeros((n, 1, hd), f64)
        self.qcos, self.qsin = (np.asarray(qcos, f64), np.asarray(qsin, f64)) if self.rope else (one.repeat(lq, 1), zero.repeat(lq, 1))
        self.kcos, self.ksin = (np.asarray(kcos, f64), np.asarray(ksin, f64)) if self.rope else (one.repeat(lk, 1), zero.repeat(lk, 1))
        self.past = past
        self.N, self.Lq, self.H, self.hd, self.Hkv, self.Lk = n, lq, h, hd, self.k.shape[1], lk
        assert self.vis.shape == (n, lq, lk) and self.bias.shape == (n, lk) and self.v.shape == self.k.shape
        assert self.qcos.shape == (n, lq, hd) and self.kcos.shape == (n, lk, hd)


def split_rows(tok, heads, kv_heads, hd):
    """token rows [N, L, (H + 2 Hkv) hd] -> q [N, L, H, hd], k [N, Hkv, L, hd], v [N, Hkv, L, hd]"""
    tok = np.asarray(tok, f64)
    n, l, _ = tok.shape
    d, dkv = heads * hd, kv_heads * hd
    q = tok[..., :d].reshape(n, l, heads, hd)
    k = tok[..., d:d + dkv].reshape(n, l, kv_heads, hd).transpose(0, 2, 1, 3)
    v = tok[..., d + dkv:].reshape(n, l, kv_heads, hd).transpose(0, 2, 1, 3)
    return q, k, v


def _table_rows(tables, pos):
    return tuple(np.asarray(t, f64)[np.asarray(pos)] for t in tables)


def prefill_step(tok, heads, kv_heads, hd, tables=None):
    """causal prefill: token i sees the keys <= i; tables (cos, sin) [>= L, hd]: token i is rotated at row i"""
    q, k, v = split_rows(tok, heads, kv_heads, hd)
    n, l = q.shape[:2]
    vis = np.broadcast_to(np.tril(np.ones((l, l), bool)), (n, l, l))
    rows = {}
    if tables is not None:
        c, s = _table_rows(tables, np.tile(np.arange(l), (n, 1)))
        rows = dict(qcos=c, qsin=s, kcos=c, ksin=s)
    return Step(q, k, v, vis, **rows)


def cache_step(tok, heads, kv_heads, hd, cache_k, cache_v, mask=None, mask_value=float(np.finfo(np.float32).min), tables=None, pos=None):
    """a decode step (Lq = 1) or an extend step over a past of P rows: token i sees the keys <= P + i (the chunk index), the key mask [N, P + Lq] puts
    (1 - mask) * mask_value on a key's scores; pos [N, Lq]: the table row of every new token (q and its own k)"""
    q, k, v = split_rows(tok, heads, kv_heads, hd)
    n, lq = q.shape[:2]
    p = np.asarray(cache_k).shape[2]
    kk = np.concatenate([np.asarray(cache_k, f64), k], axis=2)
    vv = np.concatenate([np.asarray(cache_v, f64), v], axis=2)
    vis = np.broadcast_to(np.arange(p + lq)[None, :] <= p + np.arange(lq)[:, None], (n, lq, p + lq))
    bias = None if mask is None else (1.0 - np.asarray(mask, f64)) * float(f32(mask_value))
    rows = {}
    if tables is not None:
        c, s = _table_rows(tables, pos)
        one, zero = np.ones((n, p, hd), f64), np.zeros((n, p, hd), f64)
        rows = dict(qcos=c, qsin=s, kcos=np.concatenate([one, c], 1), ksin=np.concatenate([zero, s], 1))
    return Step(q, kk, vv, vis, bias, past=p, **rows)


def resident_mask(lens, new, capacity, lq):
    """the attention_mask [N, capacity + lq] of a step bound to a resident cache: ones below len and over the first c new tokens"""
    m = np.zeros((len(lens), capacity + lq), np.int64)
    for i, (ln, c) in enumerate(zip(lens, new)):
        m[i, :ln] = 1
        m[i, capacity:capacity + c] = 1
    return m


def inplace_step(tok, heads, kv_heads, hd, cache_k, cache_v, lens, new, **kw):
    """a step bound to a resident cache of `capacity` rows whose image n holds lens[n] rows and appends new[n] tokens: the equivalent right-padded
    cache_step.  Rows at or beyond len (NaN in the tests' cache) are zeros here: their mask column is 0, so their weight is exactly 0"""
    ck, cv = np.array(cache_k, f64), np.array(cache_v, f64)
    for n, ln in enumerate(lens):
        ck[n, :, ln:] = 0.0
        cv[n, :, ln:] = 0.0
    lq = np.asarray(tok).shape[1]
    return cache_step(tok, heads, kv_heads, hd, ck, cv, mask=resident_mask(lens, new, ck.shape[2], lq), **kw)


def own_key_valid(step):
    """[N, Lq] bool: the queries whose own key carries no bias (the rows a client reads)"""
    return step.bias[:, step.past + np.arange(step.Lq)] == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# reference and statistic
# ---------------------------------------------------------------------------------------------------------------------
def _partner(x):
    hh = x.shape[-1] // 2
    return np.concatenate([x[..., hh:], x[..., :hh]], axis=-1)


def rotate64(x, cos, sin):
    """x cos + rotate_half(x) sin on the last axis, and the magnitude |x||cos| + |x_p||sin|"""
    hh = x.shape[-1] // 2
    xp = _partner(x)
    sg = np.concatenate([-np.ones(hh), np.ones(hh)])
    return x * cos + sg * xp * sin, np.abs(x) * np.abs(cos) + np.abs(xp) * np.abs(sin)


def reference(step):
    """dict(ref, Sv, D, B, E, Dqk), each [N, Lq, H, hd] float64 (the module's docstring defines them)"""
    s_ = step
    g = s_.H // s_.Hkv
    out = {k: np.zeros((s_.N, s_.Lq, s_.H, s_.hd), f64) for k in ("ref", "Sv", "D", "E", "Dqk")}
    for n in range(s_.N):
        for h in range(s_.H):
            kvh = h // g
            q, qa = rotate64(s_.q[n, :, h], s_.qcos[n], s_.qsin[n])                 # [Lq, hd]
            k, ka = rotate64(s_.k[n, kvh], s_.kcos[n], s_.ksin[n])                  # [Lk, hd]
            v = s_.v[n, kvh]
            vis = s_.vis[n]
            s = np.where(vis, s_.scale * (q @ k.T) + s_.bias[n][None, :], -np.inf)
            m = s.max(-1, keepdims=True)
            p = np.exp(s - m)
            p /= p.sum(-1, keepdims=True)
            ref = p @ v
            with np.errstate(invalid="ignore"):
                dist = np.where(vis, np.abs(s - m), 0.0)                             # |s_j - max|; (p = 0 where it is huge)
            qk = s_.scale * (qa @ ka.T)
            dev = np.abs(v[None, :, :] - ref[:, None, :])                            # [Lq, Lk, hd]
            pa = np.where(p > 0, p * (qk + dist), 0.0)
            out["ref"][n, :, h] = ref
            out["Sv"][n, :, h] = p @ np.abs(v)
            out["D"][n, :, h] = np.einsum("ij,ije->ie", pa, dev)
            out["E"][n, :, h] = np.einsum("ij,ije->ie", p, dev)
            out["Dqk"][n, :, h] = np.einsum("ij,ije->ie", p * qk, dev)
    out["B"] = out["Sv"] + out["D"]
    return out


def exp_term(r):
    return EXP_ULP * 2.0 * U * r["E"]


def half_allowance(r, tile, rope):
    """fp16 mode's additive allowance of the kernel `tile` (HALF_TERMS) per element"""
    t = {k: (rope if v == "rope" else bool(v)) for k, v in HALF_TERMS[tile].items()}
    return UH * (t["out"] * np.abs(r["ref"]) + (t["v"] + t["p"]) * r["Sv"] + (t["q"] + t["k"]) * r["Dqk"])


def excess(y, r, extra=0.0):
    """|y - ref| less the additive allowance, in units of u B, per element"""
    err = np.maximum(np.abs(np.asarray(y, f64) - r["ref"]) - extra, 0.0)
    B = r["B"]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(B > 0, err / (U * np.where(B > 0, B, 1.0)), np.where(err > 0, np.inf, 0.0))


def c_stat(y, r, rows=None, extra=0.0):
    """max over the elements of the query rows `rows` ([N, Lq] bool, None: all) of excess()"""
    x = excess(y, r, extra)
    if rows is not None:
        x = x[np.asarray(rows, bool)]
    return float(x.max()) if x.size else 0.0


def bound(r, ce, extra=0.0):
    """the admissible |y - ref| per element: MARGIN c_emul u B + the exponential's term + extra (fp16: half_allowance)"""
    return MARGIN * ce * U * r["B"] + exp_term(r) + extra


def worst_ratio(y, r, ce, rows=None, extra=0.0):
    """max |y - ref| / bound over the rows: <= 1 passes"""
    b = bound(r, ce, extra)
    err = np.abs(np.asarray(y, f64) - r["ref"])
    with np.errstate(divide="ignore", invalid="ignore"):
        x = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))
    if rows is not None:
        x = x[np.asarray(rows, bool)]
    return float(x.max()) if x.size else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# emulations of what the hardware does
# ---------------------------------------------------------------------------------------------------------------------
def _r32(x):
    with np.errstate(over="ignore"):               # (finfo.min * log2 e rounds to -inf and is clamped, as in the kernels)
        return np.asarray(x, f64).astype(f32).astype(f64)


def _h16(x):
    return np.asarray(x, f64).astype(np.float16).astype(f64)


def rotate32(x, cos, sin):
    """the kernels' rotation: fmaf(x, cos, (+-x_p) * sin), the product rounded to float32, then one FMA (double holds x cos exactly)"""
    hh = x.shape[-1] // 2
    sg = np.concatenate([-np.ones(hh), np.ones(hh)])
    return _r32(x * cos + _r32(sg * _partner(x) * sin))


def _exp2_32(x):
    with np.errstate(under="ignore"):
        return _r32(np.exp2(_r32(x)))


def _online(x, v, tiles, hd, p_half=False, drop_alpha=None):
    """the online softmax of the rows x [R, Lk] (units of log2, hidden keys -inf) over the key tiles `tiles` = [(name, key indices)] -> the record
    (m, l, o): the running maximum from -FLT_MAX, per tile alpha = exp2(m - m'), the tile's probabilities summed one by one, l = fma(l, alpha, sum),
    o *= alpha, then one FMA per key"""
    rows = x.shape[0]
    m, l, o = np.full((rows, 1), -FLT_MAX), np.zeros((rows, 1)), np.zeros((rows, hd))
    for t, keys in tiles:
        xt = x[:, keys]
        mn = np.maximum(m, xt.max(-1, keepdims=True))
        alpha = _exp2_32(m - mn)
        p = _exp2_32(xt - mn)
        ps = np.zeros_like(l)
        for j in range(p.shape[1]):
            ps = _r32(ps + p[:, j:j + 1])
        l = _r32(l * alpha + ps)
        if drop_alpha is not None and drop_alpha == t:
            o[:, :hd // 2] = _r32(o[:, :hd // 2] * alpha)
        else:
            o = _r32(o * alpha)
        if p_half:
            p = _h16(p)
        for j, key in enumerate(keys):
            o = _r32(o + p[:, j:j + 1] * v[key][None, :])
        m = mn
    return m, l, o


def _merge(recs):
    """records (m, l, o) added in their order with the weights exp2(m - M), one FMA each: a workgroup's key slots, a row's splits"""
    M = np.max([r[0] for r in recs], axis=0)
    L, O = np.zeros_like(M), np.zeros_like(recs[0][2])
    for m, l, o in recs:
        w = _exp2_32(m - M)
        L = _r32(L + l * w)
        O = _r32(O + o * w)
    return M, L, O


def emulate(step, *, hd_order=None, tile_seed=None, splits=1, slots=0, half=(), mutant=None, drop_alpha=None):
    """One legal fp32 evaluation of the step -> [N, Lq, H, hd] (float64 array of float32 numbers, of halves with "out" in `half`).
    hd_order: a permutation of the head dim for the score chain; tile_seed: a seeded random order of every split's key tiles; splits: the key tiles
    in `splits` consecutive runs, each with its own (m, l, o) record, combined in split order.
    slots = NS > 0: tile 4's partition instead of key tiles of 32.  A split's keys are dealt to NS key slots (key j of the split to slot j mod NS, the
    splits cut at multiples of NS), every slot runs its own online softmax key by key, and the slots' records are merged in slot order before the
    splits are.  What this form adds is the ORDER: the record that holds the largest score may come first, and every later record is then added to
    sums that already have their full size.
    half / mutant: operands rounded to half on the way ("q" and "k" after the rotation, "v", "p" in front of P V, "out"): `half` is an fp16 kernel's
    legal form, `mutant` the same switches as a precision mistake of an fp32 kernel.  drop_alpha = t: the rescale of key tile t left out of the
    second half of the head dim (a mutant)."""
    s_ = step
    rnd = set(half) | set(mutant or ())
    g = s_.H // s_.Hkv
    hd = s_.hd
    order = np.arange(hd) if hd_order is None else np.asarray(hd_order)
    sl2 = float(f32(f32(s_.scale) * LOG2E))
    width = slots or TILE
    ntiles = -(-s_.Lk // width)
    per = -(-ntiles // splits)
    out = np.zeros((s_.N, s_.Lq, s_.H, hd), f64)
    rs = np.random.RandomState(tile_seed) if tile_seed is not None else None
    for n in range(s_.N):
        bias2 = np.maximum(_r32(_r32(s_.bias[n]) * float(LOG2E)), -FLT_MAX)
        for kvh in range(s_.Hkv):
            k = rotate32(s_.k[n, kvh], s_.kcos[n], s_.ksin[n])
            v = s_.v[n, kvh]
            if "k" in rnd:
                k = _h16(k)
            if "v" in rnd:
                v = _h16(v)
            q = np.stack([rotate32(s_.q[n, :, kvh * g + r], s_.qcos[n], s_.qsin[n]) for r in range(g)], 1).reshape(s_.Lq * g, hd)      # row = i g + r
            if "q" in rnd:
                q = _h16(q)
            vis = np.repeat(s_.vis[n], g, axis=0)                                      # [R, Lk]
            acc = np.zeros((q.shape[0], s_.Lk), f64)
            for e in order:
                acc = _r32(acc + q[:, e:e + 1] * k[None, :, e])
            x = np.maximum(_r32(acc * sl2 + bias2[None, :]), -FLT_MAX)
            x = np.where(vis, x, -np.inf)
            recs = []
            for sp in range(splits):
                k0, k1 = sp * per * width, min(s_.Lk, (sp + 1) * per * width)
                if slots:
                    dealt = [[(j, [j]) for j in range(k0 + t, k1, slots)] for t in range(slots)]
                    recs.append(_merge([_online(x, v, d, hd, "p" in rnd) for d in dealt]))
                    continue
                tiles = [(t, list(range(t * TILE, min(k1, (t + 1) * TILE)))) for t in range(k0 // TILE, -(-max(k1, k0) // TILE))]
                if rs is not None:
                    rs.shuffle(tiles)
                recs.append(_online(x, v, tiles, hd, "p" in rnd, drop_alpha))
            _, l, o = recs[0] if splits == 1 else _merge(recs)
            y = _r32(o / l)
            if "out" in rnd:
                y = _h16(y)
            out[n, :, kvh * g:(kvh + 1) * g] = y.reshape(s_.Lq, g, hd)
    return out


def c_emul(step, r=None, rows=None, splits=1, slots=0, seed=0):
    """The largest c over the legal orders of this step's own data: the sequential chains, one seeded random order of the head dim and of the key
    tiles, (splits > 1) the records of `splits` runs of key tiles combined in split order, sequential and in the random order, and (slots > 0, tile
    4) the key-slot partition at the step's splits.  -> (c_emul, {name: c})"""
    r = r if r is not None else reference(step)
    perm = np.random.RandomState(seed).permutation(step.hd)
    runs = {"seq": emulate(step), "perm": emulate(step, hd_order=perm, tile_seed=seed)}
    if splits > 1:
        runs[f"split{splits}"] = emulate(step, splits=splits)
        runs[f"split{splits} perm"] = emulate(step, hd_order=perm, tile_seed=seed, splits=splits)
    if slots:
        runs[f"slots{slots}"] = emulate(step, splits=splits, slots=slots)
        runs[f"slots{slots} perm"] = emulate(step, hd_order=perm, splits=splits, slots=slots)
    cs = {k: c_stat(v, r, rows) for k, v in runs.items()}
    return max(cs.values()), cs


MUTANTS = {"K half": dict(mutant=("k",)), "V half": dict(mutant=("v",)), "P half": dict(mutant=("p",)), "q half": dict(mutant=("q",))}


# ---------------------------------------------------------------------------------------------------------------------
# appended rows
# ---------------------------------------------------------------------------------------------------------------------
def appended_check(step, got_k, got_v, image, count):
    """The first `count` new rows of image `image` as a kernel wrote them (got_k, got_v [Hkv, count, hd] float32) against the rule: v and an
    unrotated k bit for bit float32(operand); a rotated k element within 2u (|x||cos| + |x_p||sin|) (1 + u) of float64.
    -> (ok, the worst rotated error in units of u * magnitude)"""
    n, p = image, step.past
    k, v = step.k[n, :, p:p + count], step.v[n, :, p:p + count]
    ok = np.array_equal(np.asarray(got_v, f32), v.astype(f32))
    if not step.rope:
        return ok and np.array_equal(np.asarray(got_k, f32), k.astype(f32)), 0.0
    ref, mag = rotate64(k, step.kcos[n, p:p + count][None], step.ksin[n, p:p + count][None])
    err = np.abs(np.asarray(got_k, f64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(mag > 0, err / (U * np.where(mag > 0, mag, 1.0)), np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max()) if ratio.size else 0.0
    return ok and worst <= 2.0 * (1.0 + U), worst


# ---------------------------------------------------------------------------------------------------------------------
# data builders
# ---------------------------------------------------------------------------------------------------------------------
Q_GAIN = 3.5        # N(0, 1) q and k of any head dim have scores of spread 1 after the scale; the largest of some hundred is near 2.9: +-10


def token_table(heads, kv_heads, hd, seed, rows=7, q_gain=Q_GAIN):
    """[2 rows, (H + 2 Hkv) hd] float32: `rows` N(0, 1) q | k | v rows (every head another draw), then the same rows with their q columns times
    q_gain: ids < rows pick the flat data, ids >= rows the peaked"""
    t = np.random.RandomState(seed).randn(rows, (heads + 2 * kv_heads) * hd).astype(f32)
    hot = t.copy()
    hot[:, :heads * hd] *= f32(q_gain)
    return np.concatenate([t, hot], 0)


def even_lengths(past, n=2):
    """lengths of the same order for every image: P - 5 (at least 1), P, ... alternating"""
    return [max(1, past - 5) if i % 2 == 0 else past for i in range(n)]


def peaked(step, lens, cache_k, cache_v):
    """Copies of the cache [N, Hkv, P, hd] whose rows below lens[n] are permuted, K and V together, so that the scores of ONE query (the last new
    token of the K / V head's first query head) ascend over the cached keys of (image, K / V head) where n + kvh is odd and descend where it is even:
    with ascending scores the running maximum moves in every key tile and the largest score sits in the last split.  `step`: the Step of the
    unpermuted data (its q is the one the kernel gets: build it from the peaked token rows)"""
    ck, cv = np.array(cache_k, copy=True), np.array(cache_v, copy=True)
    g = step.H // step.Hkv
    for n in range(step.N):
        q, _ = rotate64(step.q[n, -1], step.qcos[n, -1], step.qsin[n, -1])            # [H, hd]
        for kvh in range(step.Hkv):
            ln = lens[n]
            s = np.asarray(cache_k[n, kvh, :ln], f64) @ q[kvh * g]
            o = np.argsort(s if (n + kvh) % 2 else -s, kind="stable")
            ck[n, kvh, :ln] = np.asarray(cache_k)[n, kvh, :ln][o]
            cv[n, kvh, :ln] = np.asarray(cache_v)[n, kvh, :ln][o]
    return ck, cv


def peaked_prefill(tok, heads, kv_heads, hd, tables=None, q_gain=Q_GAIN):
    """Token rows [N, L, C] float32 of a causal prefill with a peaked softmax: q times q_gain, and the k rows of every K / V head replaced so that the
    ROTATED keys are a permutation of the rotated keys of the input, ascending ((n + kvh) odd) or descending in the score of the last token's query of
    the head's first query head.  The rotation is undone at the key's new position, which needs true rope tables (cos^2 + sin^2 = 1, both halves of a
    row alike); the result is rounded to float32, so the order holds up to that rounding"""
    tok = np.array(tok, f32, copy=True)
    n, l, _ = tok.shape
    d, dkv, g = heads * hd, kv_heads * hd, heads // kv_heads
    tok[..., :d] *= f32(q_gain)
    st = prefill_step(tok, heads, kv_heads, hd, tables)
    hh = hd // 2
    sg = np.concatenate([-np.ones(hh), np.ones(hh)])
    for i in range(n):
        q, _ = rotate64(st.q[i, -1], st.qcos[i, -1], st.qsin[i, -1])
        for kvh in range(kv_heads):
            kr, _ = rotate64(st.k[i, kvh], st.kcos[i], st.ksin[i])                    # [L, hd]
            s = kr @ q[kvh * g]
            kr = kr[np.argsort(s if (i + kvh) % 2 else -s, kind="stable")]
            back = kr * st.kcos[i] - sg * _partner(kr) * st.ksin[i]                   # the inverse rotation
            tok[i, :, d + kvh * hd:d + (kvh + 1) * hd] = back.astype(f32)
    return tok
