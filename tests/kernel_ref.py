"""Per-element reference and error bound for ONE convolution / pooling step (numpy only; test infrastructure).

For a step  y = epilogue(conv(prologue(x), w') + b)  the yardstick is, per output element,

    ref64 = the float64 value from the operands the kernel is given (x_hat = prologue(x) and the folded w', b as float32 numbers),
    S     = sum |w'| |x_hat| + |b|        the scale every rounding of the chain is proportional to,
    c(y)  = max |y - ref64| / (u * S),    u = 2^-24.

The admissible error is not a constant: a test computes c_emul on the CPU from the emulations below on its own data (a k-ordered fp32
FMA chain as the MFMA pipe runs it, the same chain in a seeded random k order, the family's own partition / Winograd / bf16x6 form)
and allows  |y - ref64| <= MARGIN * c_emul * u * S  element by element.  MARGIN = 2: the emulation fixes one summation order and the
kernel uses another (K across waves, slabs, fragments); each order is one sample of the same rounding walk and the statistic is a
maximum over 1e4 .. 1e5 elements.  Operands rounded to 16 bits land at c = 24 .. 311, to half's 11 bits at 800 .. 9300, against
c_emul = 3 .. 4.3 (tests/test_kernel_ref.py holds the yardstick to that).

fp16 mode adds two derived terms (u_h = 2^-11): u_h |ref64| when the step writes a half tensor, and u_h * S per operand that the step
rounds to half itself (a prologue result, a BN-folded weight); operands that are exactly representable in half add nothing.

Convolution operands are handled in im2col form: cols [M, K] with M = (n, oh, ow) and K = (tap, channel), wm [Cout, K].

Channel-local steps (depthwise and grouped convolutions, channel_*) are walked tap by tap on NCHW tensors instead, with a residual in S
(S = sum |w'| |x_hat| + |b| + |res|) and the fused activations' allowance in channel_allowance.
"""
import numpy as np

U = 2.0 ** -24
UH = 2.0 ** -11
MARGIN = 2.0

f32, f64 = np.float32, np.float64


# ---------------------------------------------------------------------------------------------------------------------
# operands, as the planner and the loaders make them
# ---------------------------------------------------------------------------------------------------------------------
def bn_affine(g, b, m, v, eps=1e-5):
    """BatchNormalization as the planner stores it: s = g / sqrt(v + eps) in double, rounded once; t = b - m * s likewise."""
    s = np.asarray(g, f64) / np.sqrt(np.asarray(v, f64) + float(f32(eps)))
    return s.astype(f32), (np.asarray(b, f64) - np.asarray(m, f64) * s).astype(f32)


def prologue32(x, s, t, fused=True):
    """relu(s * x + t) per channel of an NCHW float32 tensor: one rounding (FMA, the default contraction) or two."""
    x = np.asarray(x, f32)
    s4, t4 = s.reshape(1, -1, 1, 1), t.reshape(1, -1, 1, 1)
    if fused:
        r = (s4.astype(f64) * x.astype(f64) + t4.astype(f64)).astype(f32)     # the product is exact in double
    else:
        r = (s4 * x).astype(f32) + t4
    return np.maximum(r, f32(0)).astype(f32)


def fold32(w, bias, s, t):
    """A BatchNorm behind the conv folded into its weights and bias, in float32 as the planner does it."""
    w = (np.asarray(w, f32) * s.reshape(-1, 1, 1, 1)).astype(f32)
    b0 = np.zeros(w.shape[0], f32) if bias is None else np.asarray(bias, f32)
    return w, ((b0 * s).astype(f32) + t).astype(f32)


def round_bits(a, bits):
    """Round to a `bits`-bit significand (11 = half's, 16 = what a truncated bf16 split keeps), exponent range untouched."""
    a = np.asarray(a, f64)
    m, e = np.frexp(a)
    return np.ldexp(np.round(m * 2.0 ** bits) / 2.0 ** bits, e)


def half_exact(a):
    return np.asarray(a, f32).astype(np.float16).astype(f32)


def im2col(x, kh, kw, stride=1, pads=(0, 0, 0, 0), dil=1):
    """NCHW -> [N, OH, OW, kh*kw, C] (zero padding; pads = top, left, bottom, right)."""
    n, c, h, w = x.shape
    pt, pl, pb, pr = pads
    xp = np.zeros((n, c, h + pt + pb, w + pl + pr), x.dtype)
    xp[:, :, pt:pt + h, pl:pl + w] = x
    oh = (h + pt + pb - dil * (kh - 1) - 1) // stride + 1
    ow = (w + pl + pr - dil * (kw - 1) - 1) // stride + 1
    cols = np.empty((n, oh, ow, kh * kw, c), x.dtype)
    for i in range(kh):
        for j in range(kw):
            cols[:, :, :, i * kw + j, :] = xp[:, :, i * dil:i * dil + (oh - 1) * stride + 1:stride,
                                              j * dil:j * dil + (ow - 1) * stride + 1:stride].transpose(0, 2, 3, 1)
    return cols


def wmat(w):
    """[Cout, Cin, kh, kw] -> [Cout, K] in the (tap, channel) order of im2col."""
    return np.ascontiguousarray(np.asarray(w).transpose(0, 2, 3, 1).reshape(w.shape[0], -1))


def to_nchw(ym, shape):
    """[M, Cout] -> [N, Cout, OH, OW] for shape = (N, OH, OW)."""
    n, oh, ow = shape
    return np.ascontiguousarray(ym.reshape(n, oh, ow, -1).transpose(0, 3, 1, 2))


# ---------------------------------------------------------------------------------------------------------------------
# reference and statistic
# ---------------------------------------------------------------------------------------------------------------------
def ref64_S(cols, wm, bias=None, relu=False):
    """(ref64, S), each [M, Cout] float64."""
    a = np.asarray(cols, f64).reshape(-1, wm.shape[1])
    b = np.asarray(wm, f64)
    ref = a @ b.T
    S = np.abs(a) @ np.abs(b).T
    if bias is not None:
        ref = ref + np.asarray(bias, f64)
        S = S + np.abs(np.asarray(bias, f64))
    if relu:
        ref = np.maximum(ref, 0.0)
    return ref, S


def excess(y, ref, S, extra=0.0):
    """|y - ref| less the additive allowance `extra`, in units of u * S.  An element with S == 0 has nothing to round: any error is inf."""
    err = np.maximum(np.abs(np.asarray(y, f64) - ref) - extra, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(S > 0, err / (U * np.where(S > 0, S, 1.0)), np.where(err > 0, np.inf, 0.0))


def c_stat(y, ref, S, extra=0.0):
    """(c, index of the worst element) -- index unravelled in the shape of ref."""
    r = excess(y, ref, S, extra)
    i = int(np.argmax(r))
    return float(r.ravel()[i]), tuple(int(v) for v in np.unravel_index(i, r.shape))


def half_terms(ref, S, half_out=False, rounded_operands=0):
    """fp16 mode's additive allowance: u_h |ref| for a half result, u_h S per operand the step itself rounds to half."""
    return (UH * np.abs(ref) if half_out else 0.0) + rounded_operands * UH * S


def within(y, ref, S, c_emul, extra=0.0, margin=MARGIN):
    return bool(np.all(excess(y, ref, S, extra) <= margin * c_emul))


def position_class(idx, shape, block=16, cblock=16):
    """Where a worst element (n, channel, row, col) of an [N, C, H, W] map sits."""
    n, ch, r, c = idx
    _, C, H, W = shape
    if r in (0, H - 1) or c in (0, W - 1):
        return "image border"
    if ch >= (C - 1) // cblock * cblock and C % cblock:
        return "last channel block"
    p = (n * H + r) * W + c
    if p % block in (0, block - 1):
        return "tile-block border"
    return "interior"


# ---------------------------------------------------------------------------------------------------------------------
# emulations of what the hardware does
# ---------------------------------------------------------------------------------------------------------------------
def _chain(acc, a, b, ks):
    """acc[M, Cout] (float32) += sum over k in ks of a[:, k] b[:, k], one fp32 FMA per k (double product and add, one rounding)."""
    for k in ks:
        acc = (acc.astype(f64) + a[:, k:k + 1] * b[None, :, k]).astype(f32)
    return acc


def chain32(cols, wm, bias=None, order=None, nsplit=1, relu=False):
    """k-ordered fp32 FMA chain; `order` = a permutation of K (None: 0..K-1); `nsplit` partial chains over consecutive pieces of the
    order, added in order (split-K slabs, K over the waves of a workgroup); bias and ReLU in float32 at the end."""
    a = np.asarray(cols, f32).reshape(-1, wm.shape[1]).astype(f64)
    b = np.asarray(wm, f32).astype(f64)
    K = b.shape[1]
    order = np.arange(K) if order is None else np.asarray(order)
    total = None
    for piece in np.array_split(order, nsplit):
        part = _chain(np.zeros((a.shape[0], b.shape[0]), f32), a, b, piece)
        total = part if total is None else (total + part).astype(f32)
    if bias is not None:
        total = (total + np.asarray(bias, f32)).astype(f32)
    return np.maximum(total, f32(0)) if relu else total


def numpy32(cols, wm, bias=None, relu=False):
    a = np.asarray(cols, f32).reshape(-1, wm.shape[1])
    y = a @ np.asarray(wm, f32).T
    if bias is not None:
        y = y + np.asarray(bias, f32)
    return np.maximum(y, f32(0)) if relu else y


_BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], f64)
_G = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], f64)
_AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], f64)


def _pass32(m, t, axis):
    """One 1-D transform pass along `axis`, rounded to float32 (the entries of B and A are 0 / +-1: each output is a short sum)."""
    return np.moveaxis(np.tensordot(m, np.moveaxis(t.astype(f64), axis, 0), axes=(1, 0)), 0, axis).astype(f32)


def wino32(x, w, bias=None, relu=False, x6=False):
    """Textbook Winograd F(2x2, 3x3) for a 3x3 / stride 1 / pad 1 conv on even H, W: U = G g G^T rounded to float32 once, V = B^T d B
    rounded after each 1-D pass, the channel sum an fp32 chain in the Winograd domain (x6: the bf16x6 product of x6_32 instead),
    A^T m A rounded per pass.  Returns NCHW."""
    x = np.asarray(x, f32)
    n, c, h, wd = x.shape
    cout = w.shape[0]
    assert w.shape[2:] == (3, 3) and h % 2 == 0 and wd % 2 == 0
    Uw = np.einsum("ij,ocjk,lk->ocil", _G, np.asarray(w, f64), _G).astype(f32)           # [Cout, Cin, 4, 4]
    xp = np.zeros((n, c, h + 2, wd + 2), f32)
    xp[:, :, 1:-1, 1:-1] = x
    th, tw = h // 2, wd // 2
    d = np.empty((n, th, tw, c, 4, 4), f32)
    for i in range(4):
        for j in range(4):
            d[..., i, j] = xp[:, :, i:i + 2 * th:2, j:j + 2 * tw:2].transpose(0, 2, 3, 1)
    V = _pass32(_BT, _pass32(_BT, d, 4), 5)                                              # rows, then columns
    Vm = V.reshape(-1, c, 16)
    Um = Uw.reshape(cout, c, 16)
    gemm = x6_32 if x6 else chain32                                                      # 16 independent [tiles, C] x [C, Cout] products
    acc = np.stack([gemm(np.ascontiguousarray(Vm[:, :, p]), np.ascontiguousarray(Um[:, :, p])) for p in range(16)], axis=2)
    m = acc.reshape(n, th, tw, cout, 4, 4)
    Y = _pass32(_AT, _pass32(_AT, m, 4), 5)                                              # [n, th, tw, cout, 2, 2]
    y = Y.transpose(0, 3, 1, 4, 2, 5).reshape(n, cout, h, wd)
    if bias is not None:
        y = (y + np.asarray(bias, f32).reshape(1, -1, 1, 1)).astype(f32)
    return np.maximum(y, f32(0)) if relu else y


def _trunc16(a):
    return (np.asarray(a, f32).view(np.uint32) & np.uint32(0xFFFF0000)).view(f32)


def split3(a):
    """An fp32 number as three bf16 numbers: x0 = trunc16(x), x1 = trunc16(x - x0), x2 = x - x0 - x1."""
    a = np.asarray(a, f32)
    x0 = _trunc16(a)
    x1 = _trunc16((a - x0).astype(f32))
    return x0, x1, ((a - x0).astype(f32) - x1).astype(f32)


def x6_32(cols, wm, bias=None, relu=False, kblock=16):
    """The bf16x6 product: three bf16 terms per operand, the six products with i + j <= 2 kept, each exact in fp32, accumulated in fp32
    per 16-deep K block smallest terms first."""
    a = [p.astype(f64) for p in split3(np.asarray(cols, f32).reshape(-1, wm.shape[1]))]
    b = [p.astype(f64) for p in split3(wm)]
    K = wm.shape[1]
    acc = np.zeros((a[0].shape[0], wm.shape[0]), f32)
    for k0 in range(0, K, kblock):
        ks = range(k0, min(K, k0 + kblock))
        for i, j in ((0, 2), (1, 1), (2, 0), (0, 1), (1, 0), (0, 0)):
            acc = _chain(acc, a[i], b[j], ks)
    if bias is not None:
        acc = (acc + np.asarray(bias, f32)).astype(f32)
    return np.maximum(acc, f32(0)) if relu else acc


def c_emul(cols, wm, bias=None, relu=False, nsplit=1, seed=0, extra_runs=()):
    """The largest c over the legal orders of this case's own data: the sequential chain, one seeded random k order, the family's
    partition (nsplit > 1), and any further emulation results in `extra_runs` ([M, Cout] arrays: wino32, x6_32, a two-rounding
    prologue ...).  Returns (c_emul, {name: c})."""
    ref, S = ref64_S(cols, wm, bias, relu)
    K = wm.shape[1]
    runs = {"seq": chain32(cols, wm, bias, relu=relu),
            "perm": chain32(cols, wm, bias, order=np.random.RandomState(seed).permutation(K), relu=relu)}
    if nsplit > 1:
        runs[f"split{nsplit}"] = chain32(cols, wm, bias, nsplit=nsplit, relu=relu)
    for i, y in enumerate(extra_runs):
        runs[f"extra{i}"] = y
    cs = {k: c_stat(v, ref, S)[0] for k, v in runs.items()}
    return max(cs.values()), cs


# ---------------------------------------------------------------------------------------------------------------------
# channel-local steps: depthwise (groups == C) and grouped convolutions
# ---------------------------------------------------------------------------------------------------------------------
def channel_out_hw(h, w, kh, kw, stride, pads):
    pt, pl, pb, pr = pads
    return (h + pt + pb - kh) // stride + 1, (w + pl + pr - kw) // stride + 1


def _taps(xh, kh, kw, stride, pads):
    """(tap index, [N, G * cpg, OH, OW] window of the zero-padded input) per filter tap, row-major: no [M, K] matrix is built."""
    n, c, h, w = xh.shape
    pt, pl, pb, pr = pads
    oh, ow = channel_out_hw(h, w, kh, kw, stride, pads)
    xp = np.zeros((n, c, h + pt + pb, w + pl + pr), xh.dtype)
    xp[:, :, pt:pt + h, pl:pl + w] = xh
    for i in range(kh):
        for j in range(kw):
            yield i * kw + j, xp[:, :, i:i + (oh - 1) * stride + 1:stride, j:j + (ow - 1) * stride + 1:stride]


def _grouped_w(w, groups):
    """[Cout, cpg, kh, kw] -> [taps, cpg, G, opg, 1, 1] float64"""
    cout, cpg, kh, kw = w.shape
    return np.asarray(w, f64).reshape(groups, cout // groups, cpg, kh * kw).transpose(3, 2, 0, 1)[..., None, None]


def channel_ref64_S(xh, w, groups, stride=1, pads=(0, 0, 0, 0), bias=None, res=None):
    """(ref64, S) of a channel-local conv step BEFORE any activation, each [N, Cout, OH, OW] float64.  xh: the input after the prologue, NCHW
    (float32, or float64 where a prologue activation makes the reference's x_hat a real number); w [Cout, Cin / groups, kh, kw]; output
    channel o reads the input channels of group o // (Cout / groups); pads = (top, left, bottom, right), padding taps contribute 0;
    S = sum |w| |x_hat| + |bias| + |res|.  ReLU and Clip are 1-Lipschitz: a bound on this value holds for the clamped one (clamp)."""
    cout, cpg, kh, kw = w.shape
    n = xh.shape[0]
    wg = _grouped_w(w, groups)
    ref = S = 0.0
    for t, win in _taps(np.asarray(xh), kh, kw, stride, pads):
        xg = win.astype(f64).reshape(n, groups, cpg, *win.shape[2:])
        for c in range(cpg):
            p = xg[:, :, c, None] * wg[t, c][None]                       # [N, G, opg, OH, OW]
            ref = ref + p
            S = S + np.abs(p)
    ref, S = ref.reshape(n, cout, *ref.shape[3:]), S.reshape(n, cout, *S.shape[3:])
    if bias is not None:
        b = np.asarray(bias, f64).reshape(1, -1, 1, 1)
        ref, S = ref + b, S + np.abs(b)
    if res is not None:
        ref, S = ref + np.asarray(res, f64), S + np.abs(np.asarray(res, f64))
    return ref, S


def channel_chain32(xh, w, groups, stride=1, pads=(0, 0, 0, 0), bias=None, res=None, order=None, half_acc=False):
    """Both kernels' order: the fp32 FMA chain from 0 over taps, then the group's channels (`order`: a permutation of the taps * cpg terms
    instead), then + bias, then + res, each rounded to float32.  half_acc (a mutant): the accumulator rounded to half after every tap."""
    cout, cpg, kh, kw = w.shape
    n = xh.shape[0]
    wg = _grouped_w(np.asarray(w, f32), groups)
    wins = [win.astype(f32).reshape(n, groups, cpg, *win.shape[2:]) for _, win in _taps(np.asarray(xh, f32), kh, kw, stride, pads)]
    terms = [(t, c) for t in range(kh * kw) for c in range(cpg)]
    acc = np.zeros((n, groups, cout // groups) + wins[0].shape[3:], f32)
    for i, k in enumerate(range(len(terms)) if order is None else order):
        t, c = terms[k]
        acc = (acc.astype(f64) + wins[t][:, :, c, None].astype(f64) * wg[t, c][None]).astype(f32)
        if half_acc and (i + 1) % cpg == 0:
            acc = acc.astype(np.float16).astype(f32)
    acc = acc.reshape(n, cout, *acc.shape[3:])
    if bias is not None:
        acc = (acc + np.asarray(bias, f32).reshape(1, -1, 1, 1)).astype(f32)
    if res is not None:
        acc = (acc + np.asarray(res, f32)).astype(f32)
    return acc


def channel_c_emul(xh, w, groups, stride=1, pads=(0, 0, 0, 0), bias=None, res=None, seed=0, extra_runs=(), ref_S=None):
    """c_emul of a channel-local step on its own data: the kernels' tap-then-channel chain, one seeded random order of the same terms, and
    any further legal results in `extra_runs` (the two-rounding prologue's).  Returns (c_emul, {name: c})."""
    ref, S = ref_S if ref_S is not None else channel_ref64_S(xh, w, groups, stride, pads, bias, res)
    K = w.shape[1] * w.shape[2] * w.shape[3]
    runs = {"seq": channel_chain32(xh, w, groups, stride, pads, bias, res),
            "perm": channel_chain32(xh, w, groups, stride, pads, bias, res, order=np.random.RandomState(seed).permutation(K))}
    for i, y in enumerate(extra_runs):
        runs[f"extra{i}"] = y
    cs = {k: c_stat(v, ref, S)[0] for k, v in runs.items()}
    return max(cs.values()), cs


def clamp(z, relu=False, lo=None, hi=None):
    """The epilogue's ReLU and Clip bounds (None: open), in the argument's precision."""
    if relu:
        z = np.maximum(z, 0)
    if lo is not None:
        z = np.maximum(z, lo)
    if hi is not None:
        z = np.minimum(z, hi)
    return z


# fused activations: the codes 1-4 of kernels.h's ApplyActBasic
ACT_SIGMOID, ACT_HARDSIGMOID, ACT_SILU, ACT_HARDSWISH = 1, 2, 3, 4
_SILU_KNEE = 2.399357280515468          # |x| where silu'' = 0: silu' is largest (1.0998) at +knee and smallest (-0.0998) at -knee


def _sig(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, f64)))


def act64(kind, x, a=0.0, b=0.0):
    """The activation in float64 (a, b: the hard forms' slope and offset, as the float32 numbers the kernel holds)."""
    x = np.asarray(x, f64)
    if kind == 0:
        return x
    g = np.clip(float(a) * x + float(b), 0.0, 1.0) if kind in (ACT_HARDSIGMOID, ACT_HARDSWISH) else _sig(x)
    return x * g if kind in (ACT_SILU, ACT_HARDSWISH) else g


def _act_d(kind, x, a, b):
    """|f'| at x from the closed forms (one-sided limits at the kinks of the hard forms are covered by act_lipschitz)"""
    s = _sig(x)
    if kind == ACT_SIGMOID:
        return s * (1 - s)
    if kind == ACT_SILU:
        return np.abs(s * (1 + x * (1 - s)))
    lin = (a * x + b > 0) & (a * x + b < 1)
    if kind == ACT_HARDSIGMOID:
        return np.where(lin, abs(a), 0.0)
    return np.abs(np.where(lin, 2 * a * x + b, np.where(a * x + b >= 1, 1.0, 0.0)))


def act_lipschitz(kind, lo, hi, a=0.0, b=0.0):
    """max |f'| on [lo, hi], element by element: |f'| at the end points and at every point of the interval where it can peak (0 for the
    sigmoid, +-knee for SiLU, both sides of the two kinks of the hard forms)."""
    lo, hi = np.asarray(lo, f64), np.asarray(hi, f64)
    if kind == 0:
        return np.ones_like(lo)
    a, b = float(a), float(b)
    L = np.maximum(_act_d(kind, lo, a, b), _act_d(kind, hi, a, b))
    pts = {ACT_SIGMOID: [0.0], ACT_SILU: [-_SILU_KNEE, _SILU_KNEE]}.get(kind)
    if pts is None:
        k0, k1 = sorted((-b / a, (1 - b) / a))
        eps = 1e-9 * max(1.0, abs(k0), abs(k1))
        pts = [k0 - eps, k0 + eps, k1 - eps, k1 + eps]
    for p in pts:
        L = np.where((lo <= p) & (p <= hi), np.maximum(L, _act_d(kind, np.full_like(lo, p), a, b)), L)
    return L


def channel_allowance(ref_z, S, c_emul, relu=False, lo=None, hi=None, act=(0, 0.0, 0.0), rounded=0, pre_act=False, f16=False, rtol=0.0):
    """The per-element yardstick of a channel-local step behind its epilogue -> dict(ref, S, extra, L_rest): a result y is held to
    c_stat(y, ref, S, extra) <= MARGIN * c_emul, that is  |y - ref| <= MARGIN * c_emul * u * S + extra.

    z, the value before the epilogue, is bound by  delta = MARGIN c_emul u S_z + rest,  rest = u_h S_z per operand the kernel rounds to half
    (fp16 mode) + rtol S_z where a prologue activation gives every tap's x_hat that relative error.  ReLU and Clip are 1-Lipschitz, so delta
    carries through them.  Behind a fused activation f (codes 1-4):  |y - f(ref_z)| <= L delta + E,  L = max |f'| on [ref_z - delta,
    ref_z + delta] from the closed forms and E = rtol |f(ref_z)|.  E is the project's own relative figure (engine_run.RTOL) applied per
    element, not a new number: generous for one exp and one divide, to be tightened from the ratios the GPU tests print.  A half result
    adds u_h |ref|.  Returned S is L S_z, extra the rest; L_rest = L * rest and half = the half result's term (for the printed ratios)."""
    S = np.asarray(S, f64)
    rest = (rounded * UH * S if f16 else 0.0) + (rtol * S if pre_act else 0.0)
    zc = clamp(np.asarray(ref_z, f64), relu, lo, hi)
    kind, a, b = act
    if kind:
        delta = MARGIN * c_emul * U * S + rest
        L = act_lipschitz(kind, zc - delta, zc + delta, a, b)
        ref = act64(kind, zc, a, b)
        E = rtol * np.abs(ref)
    else:
        L, ref, E = np.ones_like(S), zc, 0.0
    half = UH * np.abs(ref) if f16 else np.zeros_like(S)
    return dict(ref=ref, S=L * S, extra=L * rest + E + half, L_rest=L * rest, half=half)


def written_check_is_conclusive(refs, vector=1):
    """refs: (ref64, S, additive allowance, c_emul) of three runs of one model on three inputs.  An element the kernel never wrote holds one and
    the same value in all three results: where two of the references lie further apart than their bounds together no single value meets all
    three bounds, so three results within their bounds prove the element is written.  True when that holds at EVERY element (and no
    reference is zero, which a cleared buffer would meet).  vector > 1: at one element at least of every run of `vector` consecutive channels
    -- the unit a kernel that stores whole channel vectors writes or skips (fp16 maps of millions of elements: three half-precision bounds
    overlap at a few elements per million by chance)."""
    bounds = [MARGIN * ce * U * S + extra for _, S, extra, ce in refs]
    apart = np.zeros(refs[0][0].shape, bool)
    for i in range(3):
        for j in range(i + 1, 3):
            apart |= np.abs(refs[i][0] - refs[j][0]) > bounds[i] + bounds[j]
    if vector > 1:
        n, c = apart.shape[:2]
        assert c % vector == 0
        apart = apart.reshape(n, c // vector, vector, *apart.shape[2:]).any(axis=2)
    return bool(np.all(apart)) and all(bool(np.all(r[0] != 0)) for r in refs)


# ---------------------------------------------------------------------------------------------------------------------
# two-stage kernels whose intermediate is not visible (fp16: a bottleneck tensor T = relu(conv1(x_hat) + b1) kept in LDS as halfs)
# ---------------------------------------------------------------------------------------------------------------------
def two_stage_scale(S1, S2, apply_abs_w2):
    """S2 + |W2| applied to S1: the scale of the fp32 roundings of both accumulations, per element of the second stage's output.
    `apply_abs_w2(t)` runs the second conv with |w2| on an NCHW tensor t and returns the result in the output's layout."""
    return S2 + apply_abs_w2(S1)


def two_stage_half_terms(S1, T_ref, S2, ref, apply_abs_w2, rounded1=2):
    """What half rounding may add, worst case, to an element of the second stage: the first stage rounds `rounded1` operands (x_hat, w1')
    to half, (1 + u_h)^rounded1 - 1 of S1; T is stored as half, u_h |T|; both pass through |w2|, itself rounded to half, u_h S2; and the
    result is a half, u_h |ref|.  Second-order products are kept, so the term is rigorous."""
    e1 = ((1 + UH) ** rounded1 - 1) * S1
    eT = e1 * (1 + UH) + UH * np.abs(T_ref)
    return apply_abs_w2(eT) * (1 + UH) + UH * S2 + UH * np.abs(ref)


# ---------------------------------------------------------------------------------------------------------------------
# pooling
# ---------------------------------------------------------------------------------------------------------------------
def pool_ref(x, k, stride, pads, is_max, count_include_pad=0):
    """(ref64, mean |window| per output element) of MaxPool / AveragePool on NCHW; pads = top, left, bottom, right."""
    x = np.asarray(x, f64)
    n, c, h, w = x.shape
    pt, pl, pb, pr = pads
    oh = (h + pt + pb - k) // stride + 1
    ow = (w + pl + pr - k) // stride + 1
    ref = np.empty((n, c, oh, ow), f64)
    mabs = np.empty((n, c, oh, ow), f64)
    for i in range(oh):
        for j in range(ow):
            r0, c0 = i * stride - pt, j * stride - pl
            win = x[:, :, max(r0, 0):min(r0 + k, h), max(c0, 0):min(c0 + k, w)]
            cnt = k * k if count_include_pad else win.shape[2] * win.shape[3]
            ref[:, :, i, j] = win.max(axis=(2, 3)) if is_max else win.sum(axis=(2, 3)) / cnt
            mabs[:, :, i, j] = np.abs(win).sum(axis=(2, 3)) / cnt
    return ref, mabs
