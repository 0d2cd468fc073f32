"""CPU: the yardstick of tests/norm_ref.py held to account on the data of tests/norm_cases.py, before any kernel is measured with it.

  * every honest emulation, with the step's own store (a half in fp16 mode, the fused activation of a group norm), stays within MARGIN c_emul of the
    bound on every data kind, and c_emul itself stays below CEILING: a restatement that went wrong in one of the ways below would not
  * every mutant of the restatement exceeds the bound on the case built for it, by the factor printed next to its value on the old measure
    (max |y - ref| / max |ref| against engine_run.RTOL); the mutants that the old measure lets pass are asserted to pass it: the gap, recorded
  * three requests on one model: an element that kept an earlier request's value fails a bound wherever two references are further apart than
    their bounds together, which is the case at all but 0.5% of the elements and in every 16-byte vector; in place the stale value is the request's
    own x, and every vector has an element where x is outside the bound"""
import numpy as np
import pytest

import gn_graphs as GG
import norm_cases as NC
import norm_ref as NR
from engine_run import RTOL

f32, f64 = np.float32, np.float64
# c_emul of an honest restatement: about 3 u B by the count of the roundings in norm_ref's derivation (x - mu, the product with r, the FMA, and r's own
# handful of relative errors), plus the mean's sqrt(chain length) walk.  Twice that is no honest form's; the mildest mutant below sits at 79
CEILING = 6.0


def _within(y, yard):
    return NR.c_stat(y, yard["ref"], yard["B"], yard["extra"]) / (NR.MARGIN * yard["ce"]) if yard["ce"] > 0 else float(np.any(np.abs(y - yard["ref"]) > yard["extra"]))


def _row_forms(x32, gamma, beta, eps, rms, f16):
    C, V = x32.shape[1], 8 if f16 else 4
    forms = {"generic": dict(lanes=64, V=1, div=True)}
    if C % V == 0:
        forms.update({f"lanes{l}": dict(lanes=l, V=V) for l in (8, 16, 32, 64) if C // V <= 6 * l})
    out = {}
    for name, kw in forms.items():
        out[name] = NR.rows_lanes(x32, gamma, beta, eps, rms=rms, **kw)
        out[name + " perm"] = NR.rows_perm(x32, gamma, beta, eps, kw["lanes"], kw["V"], rms, kw.get("div", False), seed=5)
    return out


# ---- honest forms ----------------------------------------------------------------------------------------------------------------------------
def _rows_honest(what, x32, gamma, beta, eps, rms, yard, prec):
    shares = {n: _within(NR.store(z, prec == "fp16"), yard) for n, z in _row_forms(x32, gamma, beta, eps, rms, prec == "fp16").items()}
    print(f"NORM_REF {what} {prec}: c_emul {yard['ce']:.2f}, the forms at {min(shares.values()):.2f} .. {max(shares.values()):.2f} of the bound")
    assert yard["ce"] <= CEILING and max(shares.values()) <= 1.0, (what, prec, yard["cs"], shares)
    return yard["ce"]


@pytest.mark.parametrize("prec", NC.PRECS)
def test_honest_row_forms(prec):
    """(a), (b), (c) on every layer-norm, RMSNorm and embed case of the tables, first draw"""
    ces = []
    for c in NC.LN_TILES:
        for kind, eps in NC.ROW_DATA:
            k = NC.ln_case(c, kind, eps)
            ces.append(_rows_honest(f"layer norm C {c} {kind} eps {eps}", k.rows[0], k.gamma, k.beta, eps, False, NC.ln_yard(c, kind, eps, 0, prec), prec))
    for l, d in NC.RMS_TILES:
        for kind, eps in NC.ROW_DATA:
            k = NC.rms_case(l, d, kind, eps)
            ces.append(_rows_honest(f"RMSNorm L {l} D {d} {kind} eps {eps}", k.rows[0], k.gamma, None, eps, True, NC.rms_yard(l, d, kind, eps, 0, prec), prec))
            if kind == "edges":
                z = NR.rows_lanes(k.rows[0], k.gamma, None, eps, 64, 1, True, div=True)
                assert np.array_equal(z[2], np.zeros(d, f32)) and np.all(NC.rms_yard(l, d, kind, eps, 0, prec)["bound"][2] == 0)        # the row of zeros: 0 exactly
    for shape in NC.EMBED_TILES:
        for kind, eps in NC.EMBED_DATA:
            k = NC.embed_case(shape, kind, eps)
            _, _, x32 = NR.embed_rows(*NC._gathered(k, 0, shape[0], shape[1]))
            ces.append(_rows_honest(f"embed {shape} {kind} eps {eps}", x32, k.gamma, k.beta, eps, False, NC.embed_yard(shape, kind, eps, 0, prec), prec))
    for c in NC.LN_CONCAT_TILES:
        k = NC.ln_concat_case(c)
        ces.append(_rows_honest(f"layer norm into a concat C {c}", k.rows[0], k.gamma, k.beta, k.eps, False, NC.ln_concat_yard(c, 0, prec), prec))
    print(f"NORM_REF rows {prec}: c_emul {min(ces):.2f} .. {max(ces):.2f} over {len(ces)} cases")


@pytest.mark.parametrize("prec", NC.PRECS)
def test_honest_group_norm_forms(prec):
    """(c) and (d) on every group-norm shape, data kind and activation, first draw"""
    f16 = prec == "fp16"
    ces = []
    for shape in NC.GN_TILE1:
        n, c, h, w, g = shape
        for kind, eps in NC.GN_DATA:
            k = NC.gn_case(shape, kind, eps, None)
            forms = {"generic": NR.gn_generic(k.xs[0], k.gamma, k.beta, eps, g)}
            if NC.tiles_of(NC.GN_TILE1, shape, prec):
                forms["tile1"] = NR.gn_tile1(k.xs[0], k.gamma, k.beta, eps, g, f16, GG.gn_slabs(n, h * w, c, f16)[0])
            for act in NC.GN_ACTS:
                yard = NC.gn_yard(shape, kind, eps, 0, prec, act)
                shares = {name: _within(NR.gn_finish(z, act, f16), yard) for name, z in forms.items()}
                assert yard["ce"] <= CEILING and max(shares.values()) <= 1.0, (shape, kind, eps, act, yard["cs"], shares)
            print(f"NORM_REF group norm {shape} {kind} eps {eps} {prec}: c_emul {yard['ce']:.2f} {({k_: round(v, 2) for k_, v in yard['cs'].items()})}")
            ces.append(yard["ce"])
    print(f"NORM_REF group norm {prec}: c_emul {min(ces):.2f} .. {max(ces):.2f} over {len(ces)} cases")


# ---- mutants -----------------------------------------------------------------------------------------------------------------------------------
def _measure(y, yard):
    """(factor over the new bound, the old measure)"""
    return _within(y, yard), float(np.nanmax(np.abs(y.astype(f64) - yard["ref"])) / np.abs(yard["ref"]).max())


def _row_mutant(name, c, kind, eps, prec, lanes, mutant, designed=True):
    f16 = prec == "fp16"
    k, yard = NC.ln_case(c, kind, eps), NC.ln_yard(c, kind, eps, 0, prec)
    y = NR.store(NR.rows_lanes(k.rows[0], k.gamma, k.beta, eps, lanes, 8 if f16 else 4, mutant=mutant), f16)
    factor, old = _measure(y, yard)
    honest, _ = _measure(NR.store(NR.rows_lanes(k.rows[0], k.gamma, k.beta, eps, lanes, 8 if f16 else 4), f16), yard)
    print(f"NORM_REF mutant | {name} | C {c} {kind} {prec} | {factor:.3g} times the bound (honest {honest:.2f}) | old measure {old:.2e} of max|ref|, {old / RTOL[prec]:.2f} of RTOL")
    assert honest <= 1.0 and (factor > 1.0 or not designed), (name, c, factor, honest)
    return old


@pytest.mark.parametrize("c", (768, 1536))
def test_mutants_the_old_measure_lets_pass(c):
    """fp16 mode, randn + 0.5, 30 rows: a lost vector, an approximate rsqrt and a variance over C - 1 are under the old RTOL and far over the new bound"""
    for name, mutant in (("last 16-byte vector missing from the mean", "mean_drop_last"), ("rstd * (1 + 2^-12)", "rstd"), ("variance over C - 1", "c_minus_1")):
        assert _row_mutant(name, c, "randn", 1e-5, "fp16", 64, mutant) < RTOL["fp16"]


def test_row_mutants():
    for c in (768, 1536):
        for prec in NC.PRECS:
            _row_mutant("last vector missing from the squares", c, "randn", 1e-5, prec, 64, "sq_drop_last")
            _row_mutant("gamma rounded to half", c, "randn", 1e-5, prec, 64, "gamma_half")
        for name, mutant in (("last 16-byte vector missing from the mean", "mean_drop_last"), ("rstd * (1 + 2^-12)", "rstd"), ("variance over C - 1", "c_minus_1")):
            _row_mutant(name, c, "randn", 1e-5, "fp32", 64, mutant)
        _row_mutant("one-pass E[x^2] - mean^2", c, "mean100", 1e-5, "fp32", 64, "one_pass")
    for c in (96, 768):
        for prec in NC.PRECS:
            # rows whose std is near sqrt(eps) see which eps was used; the rows of variance 1 of the old tests do not (5e-6 of max|ref|)
            _row_mutant("eps 1e-6 used where 1e-5 was given", c, "near_eps", 1e-5, prec, 64, "eps")
            old = _row_mutant("eps 1e-6 used where 1e-5 was given", c, "randn", 1e-5, prec, 64, "eps", designed=False)
            assert old < RTOL[prec]
    _row_mutant("a zero-filled absent vector counted as -mean", 96, "randn", 1e-5, "fp32", 64, "no_has")
    _row_mutant("a zero-filled absent vector counted as -mean", 96, "randn", 1e-5, "fp16", 64, "no_has")
    # RMSNorm: the last vector missing from the squares
    for prec in NC.PRECS:
        f16 = prec == "fp16"
        k, yard = NC.rms_case(33, 256, "randn", 1e-5), NC.rms_yard(33, 256, "randn", 1e-5, 0, prec)
        factor, old = _measure(NR.store(NR.rows_lanes(k.rows[0], k.gamma, None, 1e-5, 32, 8 if f16 else 4, rms=True, mutant="sq_drop_last"), f16), yard)
        print(f"NORM_REF mutant | RMSNorm, last vector missing from the squares | D 256 randn {prec} | {factor:.3g} times the bound | old measure {old:.2e}")
        assert factor > 1.0


def _gn_mutant(name, shape, kind, prec, mutant):
    n, c, h, w, g = shape
    f16 = prec == "fp16"
    k, yard = NC.gn_case(shape, kind, 1e-5, None), NC.gn_yard(shape, kind, 1e-5, 0, prec, None)
    px = GG.gn_slabs(n, h * w, c, f16)[0]
    factor, old = _measure(NR.gn_finish(NR.gn_tile1(k.xs[0], k.gamma, k.beta, 1e-5, g, f16, px, mutant=mutant), None, f16), yard)
    honest, _ = _measure(NR.gn_finish(NR.gn_tile1(k.xs[0], k.gamma, k.beta, 1e-5, g, f16, px), None, f16), yard)
    print(f"NORM_REF mutant | group norm tile 1, {name} | {shape} {kind} {prec} | {factor:.3g} times the bound (honest {honest:.2f}) | old measure {old:.2e} of max|ref|, {old / RTOL[prec]:.2f} of RTOL")
    assert honest <= 1.0 < factor, (name, shape, factor, honest)
    return old


def test_group_norm_mutants():
    ragged = (1, 64, 37, 41, 32)
    for prec in NC.PRECS:
        old = _gn_mutant("the last pixel of the last slab missing", ragged, "randn", prec, "last_pixel")
        if prec == "fp16":
            assert old < RTOL[prec]                          # a lost pixel passes the old fp16 bound
        _gn_mutant("the ragged slab counted as slab_px pixels", ragged, "randn", prec, "ragged_count")
        _gn_mutant("one slab's record left out of the combine", ragged, "randn", prec, "skip_slab")
        _gn_mutant("the one-pixel last slab missing", (1, 1024, 17, 17, 8), "randn", prec, "last_pixel")
        _gn_mutant("groups from 256 on given group g - 256's statistics", (1, 512, 3, 3, 512), "distinct", prec, "group_wrap")


# ---- is every element written? -------------------------------------------------------------------------------------------------------------------
def _written(what, yards, vector, honest0=None):
    share, dead = NR.written_check([(y["ref"], y["bound"]) for y in yards], vector)
    print(f"NORM_REF written | {what}: {100 * share:.3f}% of the elements inconclusive, {dead} vectors of {vector} without a conclusive element")
    assert share <= 0.005 and dead == 0, (what, share, dead)
    if honest0 is not None:                                  # a value inside request 0's bound, left in place, fails request 1's or request 2's
        apart = np.zeros(yards[0]["ref"].shape, bool)
        for i in range(3):
            for j in range(i + 1, 3):
                apart |= np.abs(yards[i]["ref"] - yards[j]["ref"]) > yards[i]["bound"] + yards[j]["bound"]
        fails = (np.abs(honest0 - yards[1]["ref"]) > yards[1]["bound"]) | (np.abs(honest0 - yards[2]["ref"]) > yards[2]["bound"])
        assert np.all(fails[apart]), what


@pytest.mark.parametrize("prec", NC.PRECS)
def test_written_check_is_conclusive(prec):
    f16 = prec == "fp16"
    V = 8 if f16 else 4
    for c in (8, 96, 768, 1536):
        k = NC.ln_case(c, "randn", 1e-5)
        y0 = NR.store(NR.rows_lanes(k.rows[0], k.gamma, k.beta, 1e-5, 64, V), f16).astype(f64)
        _written(f"layer norm C {c} {prec}", [NC.ln_yard(c, "randn", 1e-5, d, prec) for d in range(3)], V, y0)
    for l, d in NC.RMS_TILES:
        k = NC.rms_case(l, d, "randn", 1e-5)
        yards = [NC.rms_yard(l, d, "randn", 1e-5, dr, prec) for dr in range(3)]
        _written(f"RMSNorm L {l} D {d} {prec}", yards, V)
        dead = [NR.stale_input_check(k.rows[dr], yards[dr]["ref"], yards[dr]["bound"], V) for dr in range(3)]      # in place: the stale value is x
        assert dead == [0, 0, 0], (l, d, dead)
    for shape in NC.EMBED_TILES:
        _written(f"embed {shape} {prec}", [NC.embed_yard(shape, "randn", 1e-12, d, prec) for d in range(3)], V)
    for shape in NC.GN_TILE1:
        if shape[2] * shape[3] > 1:                          # (one element per group: the result is beta whatever the input)
            yards = [NC.gn_yard(shape, "randn", 1e-5, d, prec, None) for d in range(3)]
            _written(f"group norm {shape} {prec}", [dict(ref=y["ref"].transpose(0, 2, 3, 1), bound=y["bound"].transpose(0, 2, 3, 1)) for y in yards], V)
    k = NC.gn_case(NC.GN_INPLACE, "randn", 1e-5, "silu", True)
    for d in range(3):
        y = NC.gn_yard(NC.GN_INPLACE, "randn", 1e-5, d, prec, "silu", True)
        assert NR.stale_input_check(k.xs[d].transpose(0, 2, 3, 1), y["ref"].transpose(0, 2, 3, 1), y["bound"].transpose(0, 2, 3, 1), V) == 0
