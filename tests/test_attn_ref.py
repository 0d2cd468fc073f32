"""CPU: the attention yardstick of tests/attn_ref.py held to itself, on the data of tests/test_attn_rows_gpu.py (tests/attn_row_cases.py).

  * attn_ref.reference agrees with the float64 walk of the same graph on the same feeds (tests/ref64.py) to 1e-12: decode, extend, causal prefill;
  * c_emul of every emulation stays below CEILING;
  * the precision mistakes an fp32 kernel can make (K, V, P, or the rotated q rounded to half; one key tile's alpha left out of the second half of
    the head dim) exceed the fp32 bound by at least 10 times (65 .. 2530 times, the alpha 3.8e5 times and more), and the K-half mutant's value under
    the old measure (max err / max|ref| against engine_run.RTOL = 2e-4) is printed on the P = 300 case: 1.93e-4 on the feeds of
    test_extend_gpu.py::test_long_cache_and_splits, which the old bound lets through, 2.2e-4 and 3.8e-4 on this file's even and peaked data;
  * tile 4's key-slot order is a legal sample the key-tile forms do not bound (found on the MI355X), so c_emul of a tile 4 case includes it;
  * the fp16 term table (attn_ref.HALF_TERMS) admits the half-operand emulation of every kernel it describes."""
import numpy as np
import pytest

import attn_ref as AR
import attn_row_cases as RC
import ref64
from engine_run import RTOL

# Measured here over the cases below: the flat data give c_emul 0.35 .. 2.3, the peaked data 1.2 .. 10.2 (extend P 40 Lq 64; prefill L 129: 9.4).  With a peaked softmax one key
# holds p = 0.99, B is little more than |ref|, and what is left is the walk of the L - 1 small terms added to it one by one, each rounding up to u |ref|:
# about 0.3 sqrt(L) u in the root mean square, and the statistic is a maximum over 1e4 elements.
CEILING = 12.0

def _p300():
    return RC.cache_case(2, 64, 300, 8, *RC.lens_pair(300))


def _decode200():
    return RC.cache_case(2, 64, 200, 1, *RC.lens_pair(200))


CASES = {
    "decode P 17": lambda: RC.cache_case(4, 64, 17, 1, *RC.lens_pair(17)),
    "decode hd 128 P 9": lambda: RC.cache_case(1, 128, 9, 1, *RC.lens_pair(9)),
    "decode P 200": _decode200,
    "extend P 33 Lq 5": lambda: RC.cache_case(2, 32, 33, 5, *RC.lens_pair(33)),
    "extend P 40 Lq 65": lambda: RC.cache_case(2, 64, 40, 65, *RC.lens_pair(40)),
    "extend P 300 Lq 8": _p300,
    "extend P 40 Lq 64": lambda: RC.cache_case(2, 64, 40, 64, *RC.lens_pair(40)),
    "extend ragged c (0, 5)": lambda: RC.cache_case(2, 64, 40, 5, (7, 30), (0, 30), new=(0, 5)),
    "prefill L 40": lambda: RC.prefill_case(2, 64, 40),
    "prefill L 129": lambda: RC.prefill_case(2, 32, 129),
}
SPLITS = {"decode P 200": 3, "extend P 300 Lq 8": 3, "extend P 40 Lq 65": 3, "extend P 40 Lq 64": 3}
SLOTS = {"decode P 17": 16, "decode hd 128 P 9": 8, "decode P 200": 16}      # tile 4's key slots (kv_graphs.key_tile) of the decode cases


@pytest.mark.parametrize("kind", RC.KINDS)
@pytest.mark.parametrize("name", ["decode P 17", "extend P 33 Lq 5", "extend ragged c (0, 5)", "extend P 300 Lq 8", "prefill L 40"])
def test_reference_is_the_float64_walk(name, kind):
    case = CASES[name]()
    want = RC.out_rows(ref64.run_f64(case.mb, case.feeds[kind])["y" if case.form == "prefill" else "out"], case)
    got = case.ref(kind)["ref"]
    # every row that sees one unmasked key (the rest: c = 0 over an empty cache; there the walk averages over the chunk's future keys too, whose
    # finfo.min is as good as a masked key's, the kernels over the visible ones, and no client reads the row)
    st = case.step(kind)
    some = (st.vis & (st.bias == 0.0)[:, None, :]).any(-1)
    assert some[AR.own_key_valid(st)].all() and some.sum() >= some.size // 2
    err = float(np.abs(got - want)[some].max() / np.abs(want).max())
    print(f"{name} {kind}: attn_ref.reference against ref64.run_f64: {err:.2e}")
    assert err < 1e-12
    if case.form == "cache":                       # the appended rows of the walk meet the rule of appended_check (its own float32 rounding aside)
        st = case.step(kind)
        walk = ref64.run_f64(case.mb, case.feeds[kind])
        for n in range(RC.N):
            c = case.new[kind][n]
            ok, worst = AR.appended_check(st, walk["present.0.key"][n, :, case.past:case.past + c].astype(np.float32),
                                          walk["present.0.value"][n, :, case.past:case.past + c].astype(np.float32), n, c)
            assert ok and worst <= 1.0, (name, kind, n, worst)


@pytest.mark.parametrize("kind", RC.KINDS)
@pytest.mark.parametrize("name", list(CASES))
def test_c_emul_stays_below_the_ceiling(name, kind):
    case = CASES[name]()
    _, ce, parts = case.yard(kind, splits=SPLITS.get(name, 1), slots=SLOTS.get(name, 0))
    print(f"{name} {kind}: c_emul {ce:.2f} " + " ".join(f"{k} {v:.2f}" for k, v in parts.items()))
    assert 0 < ce < CEILING, (name, kind, parts)


def test_the_key_slot_form_is_a_sample_the_key_tile_form_does_not_bound():
    """Why c_emul of a tile 4 case includes the key-slot form: hd 128, P = 9 (one key beyond the key tile of 8), peaked.  The cached keys of image 1
    ascend, so the largest score is key 8, the second key of slot 0, and the merge adds the seven other slots to sums that already have their
    full size, l just above 1 where a rounding is a whole u: c = 3.9 against 1.6 of the key-tile forms, more than MARGIN apart"""
    case = CASES["decode hd 128 P 9"]()
    parts = case.yard("peaked", slots=8)[2]
    print(" ".join(f"{k} {v:.2f}" for k, v in parts.items()))
    assert parts["slots8"] > AR.MARGIN * max(parts["seq"], parts["perm"])


def _old_measure(y, r, rows):
    return float(np.abs(y - r["ref"])[rows].max() / np.abs(r["ref"]).max())


@pytest.mark.parametrize("kind", RC.KINDS)
@pytest.mark.parametrize("name", ["extend P 300 Lq 8", "decode P 200", "prefill L 129"])
def test_half_mutants_miss_the_fp32_bound_tenfold(name, kind):
    case = CASES[name]()
    st = case.step(kind)
    r, ce, _ = case.yard(kind, splits=SPLITS.get(name, 1))
    rows = AR.own_key_valid(st)
    for mname, kw in AR.MUTANTS.items():
        y = AR.emulate(st, **kw)
        ratio, old = AR.worst_ratio(y, r, ce, rows), _old_measure(y, r, rows)
        print(f"{name} {kind}: mutant {mname}: misses the bound {ratio:.0f} times (c = {AR.c_stat(y, r, rows):.0f}, c_emul {ce:.2f}); "
              f"old measure {old:.2e} of RTOL {RTOL['fp32']:.0e}")
        assert ratio >= 10.0, (name, kind, mname, ratio)


def test_k_half_under_the_old_measure_on_todays_p300_data():
    """tests/test_extend_gpu.py::test_long_cache_and_splits' own feeds (image 0 valid in 3 cache rows, image 1 in 300): the K-half mutant under the old
    measure, max err over the compared rows / max|ref|, next to RTOL, and against the derived bound.  Printed, not asserted: a record of what the old
    bound does with it"""
    import extend_graphs as EG
    h, kvh, hd, past, lq = 4, 2, 64, 300, 8
    rows, feeds = EG.extend_feeds(2, h, kvh, hd, past, lq, valid=(3, None), max_pos=64)
    st = AR.cache_step(rows[feeds["input_ids"]], h, kvh, hd, feeds["past_key_values.0.key"], feeds["past_key_values.0.value"], mask=feeds["attention_mask"],
                       tables=EG.KG.LG.random_tables(64, hd), pos=feeds["position_ids"])
    r = AR.reference(st)
    own = AR.own_key_valid(st)
    ce, _ = AR.c_emul(st, r, own)
    y = AR.emulate(st, mutant=("k",))
    per_image = [float(np.abs(y - r["ref"])[n].max() / np.abs(r["ref"][n]).max()) for n in range(2)]
    old, ratio = _old_measure(y, r, own), AR.worst_ratio(y, r, ce, own)
    print(f"today's P = 300 data: max|ref| per image {[round(float(np.abs(r['ref'][n]).max()), 2) for n in range(2)]}; K half: old measure {old:.2e} of RTOL "
          f"{RTOL['fp32']:.0e} (per image, of its own max|ref|: {per_image[0]:.2e}, {per_image[1]:.2e}); misses the derived bound {ratio:.0f} times")
    assert ratio >= 10.0


@pytest.mark.parametrize("name", ["extend P 300 Lq 8", "decode P 200", "prefill L 129"])
def test_a_missing_alpha_misses_the_fp32_bound_tenfold(name):
    """one key tile's alpha left out of the second half of the head dim, on the peaked data (ascending scores: the maximum moves in every tile); the
    tile is the last one that holds cached keys of the long image"""
    case = CASES[name]()
    st = case.step("peaked")
    r, ce, _ = case.yard("peaked", splits=SPLITS.get(name, 1))
    rows = AR.own_key_valid(st)
    t = (max(case.lens["peaked"]) - 1) // AR.TILE if case.form == "cache" else (case.lq - 1) // AR.TILE
    y = AR.emulate(st, drop_alpha=t)
    ratio, old = AR.worst_ratio(y, r, ce, rows), _old_measure(y, r, rows)
    print(f"{name} peaked: alpha of key tile {t} left out of the second half of hd: misses the bound {ratio:.0f} times; old measure {old:.2e}")
    assert ratio >= 10.0
    first = AR.worst_ratio(y[..., :case.hd // 2], {k: v[..., :case.hd // 2] for k, v in r.items()}, ce, rows)
    assert first <= 1.0, "the first half of the head dim is untouched"


HALF_FORMS = {0: ("out",), 4: ("out",), 5: ("q", "k", "v", "p", "out"), 1: ("q", "k", "p", "out"), 2: ("q", "k", "p", "out"), 3: ("q", "k", "p", "out")}


@pytest.mark.parametrize("kind", RC.KINDS)
@pytest.mark.parametrize("tile, name", [(0, "decode P 200"), (4, "decode P 200"), (0, "extend P 300 Lq 8"), (5, "extend P 300 Lq 8"), (5, "extend P 40 Lq 65"),
                                        (1, "prefill L 129"), (3, "prefill L 129"), (2, "prefill L 40")])
def test_half_terms_admit_the_half_operand_emulation(tile, name, kind):
    """the kernel's fp16 form as HALF_TERMS describes it (the token rows arrive as halves), emulated, within the fp32 bound plus the table's terms"""
    case = CASES[name]()
    assert all(bool(v) == (k in HALF_FORMS[tile]) for k, v in AR.HALF_TERMS[tile].items())
    st = case.step(kind, "fp16")
    slots = SLOTS[name] if tile == 4 else 0
    r, ce, _ = case.yard(kind, "fp16", splits=SPLITS.get(name, 1), slots=slots)
    rows = AR.own_key_valid(st)
    y = AR.emulate(st, half=HALF_FORMS[tile], slots=slots)
    extra = AR.half_allowance(r, tile, st.rope)
    ratio = AR.worst_ratio(y, r, ce, rows, extra)
    print(f"{name} {kind} tile {tile}: half-operand emulation at {ratio:.3f} of the bound (without the terms: {AR.worst_ratio(y, r, ce, rows):.0f})")
    assert ratio <= 1.0
    assert AR.worst_ratio(y, r, ce, rows) > 10.0, "without its terms the fp16 form is a mutant"
