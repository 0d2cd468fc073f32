"""Per-element reference and error bound for ONE normalisation step (numpy only; test infrastructure): layernorm_kernel / rmsnorm_kernel and their
generic forms, groupnorm_generic_kernel, groupnorm_stats_kernel + groupnorm_apply_kernel, embed_ln_kernel and embed_sum_kernel.

The yardstick.  From the operands the kernel is handed (x as the half-exact numbers both precisions read; gamma, beta and the embedding tables as
float32) the float64 value `ref` and a scale `B` per output element.  With mu the mean and r = 1 / sqrt(var + eps) of a row (layer norm, embed) or
of an (image, group) (group norm), all in float64,

    y = (x - mu) r gamma + beta          B = |gamma| r (|x - mu| + A) + |beta|          A = mean |x| over the row / the (image, group)

Derivation, every fp32 rounding of the chain in turn (u = 2^-24):
  * the mean is a sum of C terms: whatever the order, its error is a multiple of u sum |x| / C = u A.  It shifts every centred value by the same
    amount, which r gamma carries to the output: |gamma| r A.  This is all that is left where |mu| >> std (x - mu is then exact by Sterbenz).
  * x - mu, (x - mu) r and the final FMA each round a value of size |gamma| r |x - mu| (+ |beta| for the FMA): |gamma| r |x - mu| + |beta|.
  * r: the centred squares are positive, so their sum, the division by C, + eps, the square root and the reciprocal are each RELATIVE errors of
    some u; the error of the mean enters the variance in second order only.  A relative error of r is one of |gamma| r |x - mu| again.
RMSNorm has no centring and no mean: y = x r gamma and every rounding, the mean of the squares' included, is relative to |gamma| r |x|, so
B = |gamma| r |x|; a row of zeros has B = 0 and its result must be 0 exactly.
The embed step builds x = word + type + pos in fp32 first: two roundings relative to X = |word| + |type| + |pos|, which |x| may be far below.  X
takes the place of |x| in A and of |x - mu| elementwise (|x - mu| <= X + A always): B = |gamma| r (X + A) + |beta|, A = mean X.  The sum-only
form has B = X.

    c(y) = |y - ref| / (u B)

The admissible error is  MARGIN c_emul u B  plus the half terms, MARGIN = kernel_ref.MARGIN = 2, and c_emul the largest c of the emulations below on
the case's OWN data, each a legal sample of a kernel's rounding walk in fp32 arithmetic:
  (a) rows_lanes     layernorm_kernel / rmsnorm_kernel / embed_ln_kernel as written: per-lane chains over the 16-byte vectors l, l + LANES, ...,
                     the xor tree of group_sum, the centred second pass with its `has` guard, multiply by 1 / C
  (b) rows_perm      the same chains and tree with the channels dealt to them in a seeded random order
  (c) rows_lanes(lanes=64, V=1, div=True)   the generic row kernels' stride-64 chains;  gn_generic  groupnorm_generic_kernel's stride-kGnBlock
                     chains with block_sum (xor tree per wave, then the wave sums in wave order)
  (d) gn_tile1       groupnorm_stats_kernel + groupnorm_apply_kernel restated: per vector the sub-group's own mean and M2, the running Chan merge with
                     f = 1 / (seen + 1), the LDS merges in row and then in channel order, one record per (slab, group), the P-way combine in slab order
  (a) and (d) also run with the sums a * b + c of the kernels' text (q / C + eps; m2b + d d n f) as ONE fma each: the compiler may contract them
Half terms (u_h = 2^-11): u_h |ref| where the step stores halfs; nothing for the inputs, which are half-exact.  Behind a fused activation (group
norm) the allowance is kernel_ref.channel_allowance's, with B as its S.

The emulations take `mutant=` names; tests/test_norm_ref.py shows that each mutant exceeds the bound on the case built for it."""
import numpy as np

import kernel_ref as KR
from kernel_ref import MARGIN, U, UH, f32, f64

GN_BLOCK = 256                           # kernels.h kGnBlock
PERMS = 3                                # random orders per form in c_emul: the maximum over a row of a few elements is a noisy statistic
ACT_CODES = {None: 0, "sigmoid": 1, "silu": 3, "relu": 5}


def half_exact(a):
    return np.asarray(a, f32).astype(np.float16).astype(f32)


def _h16(a):
    return np.asarray(a, f32).astype(np.float16).astype(f32)


def store(z, f16):
    """the store of a step's fp32 result: a half in an fp16 plan"""
    return _h16(z) if f16 else np.asarray(z, f32)


# ---------------------------------------------------------------------------------------------------------------------------------------
# reference and scale
# ---------------------------------------------------------------------------------------------------------------------------------------
def rows_ref(x, gamma, beta, eps, rms=False, X=None):
    """x [R, C] -> (ref, B) float64.  eps: the float32 number the kernel holds.  X [R, C]: the embed step's |word| + |type| + |pos| (x is then the
    exact float64 sum)"""
    x = np.asarray(x, f64)
    g = np.abs(np.asarray(gamma, f64))[None]
    e = float(f32(eps))
    if rms:
        r = 1.0 / np.sqrt((x * x).mean(1, keepdims=True) + e)
        return x * r * np.asarray(gamma, f64)[None], g * r * np.abs(x)
    b = np.zeros(x.shape[1]) if beta is None else np.asarray(beta, f64)
    mu = x.mean(1, keepdims=True)
    r = 1.0 / np.sqrt(((x - mu) ** 2).mean(1, keepdims=True) + e)
    ref = (x - mu) * r * np.asarray(gamma, f64)[None] + b[None]
    mag = np.abs(x - mu) if X is None else np.asarray(X, f64)
    A = (np.abs(x) if X is None else np.asarray(X, f64)).mean(1, keepdims=True)
    return ref, g * r * (mag + A) + np.abs(b)[None]


def gn_ref(x, gamma, beta, eps, groups):
    """x [N, C, H, W] -> (ref_z, B) float64 of the value BEFORE the activation"""
    x = np.asarray(x, f64)
    n, c, h, w = x.shape
    xg = x.reshape(n, groups, -1)
    mu = xg.mean(2, keepdims=True)
    r = 1.0 / np.sqrt(((xg - mu) ** 2).mean(2, keepdims=True) + float(f32(eps)))
    A = np.abs(xg).mean(2, keepdims=True)
    g4, b4 = np.asarray(gamma, f64).reshape(1, c, 1, 1), np.asarray(beta, f64).reshape(1, c, 1, 1)
    ref = ((xg - mu) * r).reshape(x.shape) * g4 + b4
    return ref, np.abs(g4) * (r * (np.abs(xg - mu) + A)).reshape(x.shape) + np.abs(b4)


def embed_rows(word, typ, pos):
    """the gathered table rows [R, D] (typ / pos may be None) -> (x float64 exact sum, X = the sum of magnitudes, x32 = the kernel's fp32 sum)"""
    parts = [np.asarray(p, f32) for p in (word, typ, pos) if p is not None]
    x32 = parts[0]
    for p in parts[1:]:
        x32 = (x32 + p).astype(f32)
    return sum(p.astype(f64) for p in parts), sum(np.abs(p.astype(f64)) for p in parts), x32


def excess(y, ref, B, extra=0.0):
    """kernel_ref.excess with a NaN counted as inf"""
    r = KR.excess(y, ref, B, extra)
    return np.where(np.isnan(r), np.inf, r)


def c_stat(y, ref, B, extra=0.0):
    return float(excess(y, ref, B, extra).max())


def half_extra(ref, f16):
    return UH * np.abs(ref) if f16 else 0.0


def rows_class(idx, C, V, lanes, rows_per_wg):
    """where the element (row, channel) of a row kernel's output sits"""
    row, ch = idx
    cvn = -(-C // V)
    cv = ch // V
    if cv in (0, cvn - 1):
        return "first vector of the row" if cv == 0 else "last vector of the row"
    if lanes and cv >= (cvn - 1) // lanes * lanes:
        return "last lane group"
    if row % rows_per_wg == rows_per_wg - 1:
        return "last row of a workgroup"
    return "interior"


def gn_class(idx, shape, slab_px):
    """where the element (n, c, y, x) of a group-norm map sits"""
    _, _, H, W = shape
    p = idx[2] * W + idx[3]
    if slab_px and H * W % slab_px and p >= H * W // slab_px * slab_px:
        return "ragged slab"
    return "first pixel of a slab" if slab_px and p % slab_px == 0 else "interior"


def worst_ratio(y, ref, B, c_emul, extra=0.0, classify=None):
    """-> (the worst |y - ref| less `extra`, as a share of MARGIN c_emul u B; its c; its index in ref's shape; its position class)"""
    r = excess(y, ref, B, extra)
    i = int(np.argmax(r))
    idx = tuple(int(v) for v in np.unravel_index(i, r.shape))
    c = float(r.ravel()[i])
    share = c / (MARGIN * c_emul) if c_emul > 0 else (np.inf if c > 0 else 0.0)      # (c_emul 0: the emulations are exact, and so must the kernel be)
    return share, c, idx, (classify(idx) if classify else "")


def describe(kernel, tile, prec, w, c_emul):
    """the failure message: kernel, tile, precision, c and c_emul, the worst element and its class"""
    return f"{kernel} tile {tile} {prec}: c {w[1]:.2f} against c_emul {c_emul:.2f} ({w[0]:.2f} of the bound) at {w[2]} ({w[3]})"


# ---------------------------------------------------------------------------------------------------------------------------------------
# emulations of the row kernels; all return the fp32 result BEFORE a half store
# ---------------------------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """one fp32 FMA of float32 operands (the product is exact in double)"""
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def _tree(v):
    """group_sum: v [R, L] -> [R], the xor tree m = L / 2 ... 1 (every lane ends with the same bits)"""
    L = v.shape[-1]
    idx = np.arange(L)
    m = L // 2
    while m >= 1:
        v = (v + v[..., idx ^ m]).astype(f32)
        m //= 2
    return v[..., 0]


def _finish_rows(xc, x, rstd, gamma, beta, rms, mutant):
    g = np.asarray(gamma, f32)
    if mutant == "gamma_half":
        g = _h16(g)
    if mutant == "rstd":
        rstd = (rstd * f32(1 + 2.0 ** -12)).astype(f32)
    if rms:
        return ((x * rstd[:, None]).astype(f32) * g[None]).astype(f32)
    b = np.zeros_like(g) if beta is None else np.asarray(beta, f32)
    return _fma((xc * rstd[:, None]).astype(f32), g[None], b[None])


def _rstd(q, C, eps, div, mutant, mean=None, contract=False):
    """contract: q * (1 / C) + eps as ONE fma, which the compiler may make of the kernel's expression"""
    n = f32(C - 1 if mutant == "c_minus_1" else C)
    e = f32(1e-6) if mutant == "eps" else f32(eps)
    var = (q / n).astype(f32) if div or mutant == "c_minus_1" else (q * (f32(1) / n)).astype(f32)
    if mutant == "one_pass":
        var = (var - (mean * mean).astype(f32)).astype(f32)
    ve = _fma(q, np.full_like(q, f32(1) / n), np.full_like(q, e)) if contract and not div and mutant is None else (var + e).astype(f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (f32(1) / np.sqrt(ve)).astype(f32)


def rows_lanes(x, gamma, beta, eps, lanes, V, rms=False, div=False, mutant=None, contract=False):
    """(a) / (c): lane l of a group of `lanes` holds the V-channel vectors l, l + lanes, ... of its row.  lanes = 64, V = 1, div: the generic kernels
    (any C; the mean is a division by C).  mutants: mean_drop_last / sq_drop_last (the row's last vector missing from the first / second sum),
    c_minus_1, rstd, one_pass, gamma_half, eps, no_has (a zero-filled absent vector counted as -mean)"""
    x = np.asarray(x, f32)
    R, C = x.shape
    cvn = -(-C // V)
    NV = -(-cvn // lanes)
    xp = np.zeros((R, NV * lanes * V), f32)
    xp[:, :C] = x
    xp = xp.reshape(R, NV, lanes, V)
    has = (np.arange(NV)[:, None] * lanes + np.arange(lanes)[None] < cvn)[None, :, :, None]
    keep = lambda name: (np.arange(NV)[:, None] * lanes + np.arange(lanes)[None] != cvn - 1) if mutant == name else np.ones((NV, lanes), bool)  # noqa: E731
    inv = f32(1) / f32(C)

    def chain(vals, square, kp):
        s = np.zeros((R, lanes), f32)
        for j in range(NV):
            for v in range(V):
                t = _fma(vals[:, j, :, v], vals[:, j, :, v], s) if square else (s + vals[:, j, :, v]).astype(f32)
                s = np.where(kp[j][None], t, s)
        return _tree(s)

    if rms:
        return _finish_rows(None, x, _rstd(chain(xp, True, keep("sq_drop_last")), C, eps, div, mutant, None, contract), gamma, beta, True, mutant)
    tot = chain(xp, False, keep("mean_drop_last"))
    mean = (tot / f32(C)).astype(f32) if div else (tot * inv).astype(f32)
    cen = (xp - mean[:, None, None, None]).astype(f32)
    xc = cen if mutant == "no_has" else np.where(has, cen, f32(0))
    q = chain(xp if mutant == "one_pass" else xc, True, keep("sq_drop_last"))
    rstd = _rstd(q, C, eps, div, mutant, mean, contract)
    return _finish_rows(xc.reshape(R, -1)[:, :C], x, rstd, gamma, beta, False, mutant)


def rows_perm(x, gamma, beta, eps, lanes, V, rms=False, div=False, seed=0):
    """(b): the same lane chains and tree over the channels in a seeded random order (which channel a lane adds when is the kernel's choice)"""
    C = np.asarray(x).shape[1]
    order = np.random.RandomState(seed).permutation(C)
    y = rows_lanes(np.asarray(x, f32)[:, order], np.asarray(gamma)[order], None if beta is None else np.asarray(beta)[order], eps, lanes, V, rms, div)
    out = np.empty_like(y)
    out[:, order] = y
    return out


def rows_c_emul(x32, ref, B, gamma, beta, eps, rms=False, f16=False, seed=0, post=None):
    """c_emul of a row step on its own data: (a) on every lane group that holds the row (V of the step's element type), (b) PERMS times each, (c).
    post: what a step behind the norm does to each emulated result before it is measured.  -> (c_emul, {name: c})"""
    C = x32.shape[1]
    V = 8 if f16 else 4
    runs = {"generic": rows_lanes(x32, gamma, beta, eps, 64, 1, rms, div=True)}
    forms = [("generic", 64, 1, True)] + ([(f"lanes{l}", l, V, False) for l in (8, 16, 32, 64) if C // V <= 6 * l] if C % V == 0 else [])
    for name, lanes, v, div in forms:
        if not div:
            runs[name] = rows_lanes(x32, gamma, beta, eps, lanes, v, rms)
            runs[name + " fma"] = rows_lanes(x32, gamma, beta, eps, lanes, v, rms, contract=True)
        for k in range(PERMS):
            runs[f"{name} perm{k}"] = rows_perm(x32, gamma, beta, eps, lanes, v, rms, div, PERMS * seed + k)
    cs = {k: c_stat(post(v) if post else v, ref, B) for k, v in runs.items()}
    return max(cs.values()), cs


# ---------------------------------------------------------------------------------------------------------------------------------------
# emulations of the group-norm kernels; both return the fp32 value BEFORE the activation
# ---------------------------------------------------------------------------------------------------------------------------------------
def _block_sum(v):
    """v [M, GN_BLOCK] -> [M]: the xor tree inside each wave of 64, then the wave sums added in wave order from 0"""
    w = _tree(v.reshape(v.shape[0], GN_BLOCK // 64, 64))
    s = np.zeros(v.shape[0], f32)
    for k in range(GN_BLOCK // 64):
        s = (s + w[:, k]).astype(f32)
    return s


def gn_generic(x, gamma, beta, eps, groups):
    """(c): one workgroup per (image, group); thread t walks the elements t, t + 256, ... in (pixel, channel of the group) order"""
    x = np.asarray(x, f32)
    n, c, h, w = x.shape
    cpg = c // groups
    E = h * w * cpg
    xe = x.reshape(n, groups, cpg, h * w).transpose(0, 1, 3, 2).reshape(n * groups, E)
    it = -(-E // GN_BLOCK)
    xp = np.zeros((n * groups, it * GN_BLOCK), f32)
    xp[:, :E] = xe
    valid = (np.arange(it * GN_BLOCK) < E).reshape(it, GN_BLOCK)
    xp = xp.reshape(-1, it, GN_BLOCK)
    s = np.zeros((n * groups, GN_BLOCK), f32)
    for i in range(it):
        s = (s + xp[:, i]).astype(f32)
    mean = (_block_sum(s) / f32(E)).astype(f32)
    q = np.zeros_like(s)
    for i in range(it):
        d = (xp[:, i] - mean[:, None]).astype(f32)
        q = np.where(valid[i][None], _fma(d, d, q), q)
    rstd = (f32(1) / np.sqrt(((_block_sum(q) / f32(E)).astype(f32) + f32(eps)).astype(f32))).astype(f32)
    d = (xe - mean[:, None]).astype(f32).reshape(n, groups, h * w, cpg).transpose(0, 1, 3, 2).reshape(x.shape)
    a = (np.asarray(gamma, f32).reshape(1, groups, cpg) * rstd.reshape(n, groups, 1)).astype(f32).reshape(n, c, 1, 1)
    return _fma(d, a, np.asarray(beta, f32).reshape(1, c, 1, 1))


def _madd(a, b, c, contract):
    """a * b + c: one fma where the compiler contracts the expression, else two roundings"""
    a, b, c = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32))
    return _fma(a, b, c) if contract else ((a * b).astype(f32) + c).astype(f32)


def _chan(n, mean, m2, nb, mb, m2b, contract=False):
    """kernels_gn.hip chan() on float32 arrays"""
    tot = (n + nb).astype(f32)
    d = (mb - mean).astype(f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        f = (nb / tot).astype(f32)
    m2 = (m2 + _madd(((d * d).astype(f32) * n).astype(f32), f, m2b, contract)).astype(f32)
    return tot, _fma(d, f, mean), m2


def gn_tile1(x, gamma, beta, eps, groups, f16, slab_px, mutant=None, contract=False):
    """(d): groupnorm_stats_kernel<T, CPV> and groupnorm_apply_kernel restated.  slab_px: gn_graphs.gn_slabs' pixels per slab.  mutants:
    last_pixel (the last pixel of the last slab missing from the statistics), ragged_count (the ragged slab counted as slab_px pixels),
    skip_slab (the second slab's record left out of the combine), group_wrap (groups from 256 on given group g - 256's statistics)"""
    x = np.asarray(x, f32)
    N, C, H, W = x.shape
    V = 8 if f16 else 4
    hw, cvn, cpg = H * W, C // V, C // groups
    R = GN_BLOCK // cvn
    CPV = min(cpg, V)
    NG = V // CPV
    vpg = cpg // V if cpg > V else 1
    slabs = -(-hw // slab_px)
    P = 1
    while P < 16 and 2 * P * groups <= GN_BLOCK:
        P *= 2
    z = lambda *s: np.zeros(s, f32)  # noqa: E731
    out = np.empty_like(x)
    for img in range(N):
        xi = x[img].reshape(C, hw).T                                       # [hw, C]
        recs = []
        for s in range(slabs):
            p0, p1 = s * slab_px, min((s + 1) * slab_px, hw)
            if mutant == "last_pixel" and s == slabs - 1:
                p1 -= 1
            npx = p1 - p0
            mean, m2 = z(R, cvn, NG), z(R, cvn, NG)
            for it in range(-(-npx // R)):
                rows = min(R, npx - it * R)
                xv = np.zeros((R, cvn, NG, CPV), f32)
                xv[:rows] = xi[p0 + it * R:p0 + it * R + rows].reshape(rows, cvn, NG, CPV)
                f = f32(1) / f32(it + 1)
                cm = z(R, cvn, NG)
                for i in range(CPV):
                    cm = (cm + xv[..., i]).astype(f32)
                cm = (cm * (f32(1) / f32(CPV))).astype(f32)
                cq = z(R, cvn, NG)
                for i in range(CPV):
                    d = (xv[..., i] - cm).astype(f32)
                    cq = _fma(d, d, cq)
                d = (cm - mean).astype(f32)
                nm = _fma(d, f, mean)
                nq = (m2 + _madd(((d * d).astype(f32) * f32(it * CPV)).astype(f32), f, cq, contract)).astype(f32)
                live = (np.arange(R) < rows)[:, None, None]
                mean, m2 = np.where(live, nm, mean), np.where(live, nq, m2)
            cnt_px = slab_px if mutant == "ragged_count" else npx
            n_, mu, q = z(cvn, NG), z(cvn, NG), z(cvn, NG)
            for rr in range(R):                                            # the threads of one column, in row order
                cnt = (cnt_px - rr + R - 1) // R if cnt_px > rr else 0
                if cnt == 0:
                    break
                n_, mu, q = _chan(n_, mu, q, f32(cnt * CPV), mean[rr], m2[rr], contract)
            cm_, cq_ = mu.reshape(groups, vpg), q.reshape(groups, vpg)     # the columns of one group, in channel order
            n_, mu, q = z(groups), z(groups), z(groups)
            for k in range(vpg):
                n_, mu, q = _chan(n_, mu, q, f32(cnt_px * CPV), cm_[:, k], cq_[:, k], contract)
            recs.append((n_, mu, q))
        run = -(-slabs // P)
        parts = []
        for part in range(P):                                              # P threads per group, each a contiguous run of slabs
            n_, mu, q = z(groups), z(groups), z(groups)
            for s in range(part * run, min(slabs, (part + 1) * run)):
                if mutant == "skip_slab" and s == 1:
                    continue
                n_, mu, q = _chan(n_, mu, q, *recs[s], contract)
            parts.append((n_, mu, q))
        n_, mu, q = z(groups), z(groups), z(groups)
        for pn, pm, pq in parts:
            if pn[0] > 0:
                n_, mu, q = _chan(n_, mu, q, pn, pm, pq, contract)
        rstd = (f32(1) / np.sqrt(((q / n_).astype(f32) + f32(eps)).astype(f32))).astype(f32)
        if mutant == "group_wrap":
            g = np.arange(groups)
            mu, rstd = mu[np.where(g >= 256, g - 256, g)], rstd[np.where(g >= 256, g - 256, g)]
        gi = np.arange(C) // cpg
        av = (np.asarray(gamma, f32) * rstd[gi]).astype(f32)
        out[img] = _fma((xi - mu[gi][None]).astype(f32), av[None], np.asarray(beta, f32)[None]).T.reshape(C, H, W)
    return out


def gn_finish(z, act, f16):
    """the activation as ApplyAct computes it in fp32 (the exponential rounded correctly), then the half store of an fp16 plan"""
    z = np.asarray(z, f32)
    code = ACT_CODES[act]
    if code:
        z = KR.act64(code, z).astype(f32)
    return _h16(z) if f16 else z


def gn_c_emul(x, ref, B, gamma, beta, eps, groups, f16, slab_px=None):
    """c_emul of a group-norm step on its own data: (c) always, (d) where tile 1 may run (slab_px given) -> (c_emul, {name: c})"""
    runs = {"generic": gn_generic(x, gamma, beta, eps, groups)}
    if slab_px:
        runs["tile1"] = gn_tile1(x, gamma, beta, eps, groups, f16, slab_px)
        runs["tile1 fma"] = gn_tile1(x, gamma, beta, eps, groups, f16, slab_px, contract=True)
    cs = {k: c_stat(v, ref, B) for k, v in runs.items()}
    return max(cs.values()), cs


def gn_allowance(ref_z, B, c_emul, act, f16, rtol):
    """kernel_ref.channel_allowance with B as its S -> dict(ref, S, extra, ...): hold y to excess(y, ref, S, extra) <= MARGIN c_emul"""
    return KR.channel_allowance(ref_z, B, c_emul, relu=act == "relu", act=(ACT_CODES[act] if act in ("silu", "sigmoid") else 0, 0.0, 0.0), f16=f16, rtol=rtol)


# ---------------------------------------------------------------------------------------------------------------------------------------
# is every element written?
# ---------------------------------------------------------------------------------------------------------------------------------------
def written_check(refs, vector):
    """refs: (ref, bound) of three requests on one model, bound = MARGIN c_emul u B + extra per element, the channel axis LAST.  An element the kernel
    never wrote holds one value in all three results; where two references lie further apart than their bounds together no value meets all three.
    -> (the share of elements where no pair is that far apart, the number of `vector`-channel runs without one conclusive element)"""
    apart = np.zeros(refs[0][0].shape, bool)
    for i in range(3):
        for j in range(i + 1, 3):
            apart |= np.abs(refs[i][0] - refs[j][0]) > refs[i][1] + refs[j][1]
    return float(1.0 - apart.mean()), _dead_vectors(apart, vector)


def _dead_vectors(ok, vector):
    C = ok.shape[-1]
    pad = -C % vector                                                             # (the last run is shorter where C is no multiple)
    ok = np.concatenate([ok.reshape(-1, C), np.zeros((ok.size // C, pad), bool)], axis=1)
    return int((~ok.reshape(ok.shape[0], -1, vector).any(axis=2)).sum())


def stale_input_check(x, ref, bound, vector):
    """in place: the stale value of an element is the request's own x -> the number of `vector`-channel runs where no element has |x - ref| above
    its bound (channel axis last)"""
    return _dead_vectors(np.abs(np.asarray(x, f64) - ref) > bound, vector)
