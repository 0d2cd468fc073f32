"""GPU (-m gpu): the normalisation kernels held element by element to the derived bound of tests/norm_ref.py,

    |y - ref| <= MARGIN c_emul u B (+ u_h |ref| where the step stores halfs; behind a fused SiLU kernel_ref.channel_allowance's terms),

on the literal tables and data of tests/norm_cases.py: layernorm_kernel / rmsnorm_kernel on tiles 1-4 and their generic forms, groupnorm_generic_kernel,
groupnorm_stats_kernel + groupnorm_apply_kernel, embed_ln_kernel and embed_sum_kernel with their generic forms, in both precisions.  Per case ONE model
(IE_AUTOTUNE=0, the tile forced) answers three requests; the Profile label is the kernel the table names, every output is finite and every element of
every output is within its bound.  c = max |y - ref| / (u B) (fp16: of what is left beyond the half terms) is printed per request next to c_emul.
Where the three references are distinguishable (every kind but "edges", whose constant and zero rows give beta in every request) the case is also
asserted conclusive: an element that kept an earlier request's value would fail one of its three bounds.  tests/test_norm_rows_plan.py checks on the
CPU that every table entry plans onto the kernel, tile, slab count and aliasing it names."""
import numpy as np
import pytest

import bert_graphs as BG
import convnext_graphs as CG
import gn_graphs as GG
import gpt2_graphs as G2
import llama_graphs as LG
import norm_cases as NC
import norm_ref as NR
from engine_run import plan_of, run_model, tensor, with_env
from gpu_ai_inference_server_amd import binding as B
from gpu_ai_inference_server_amd.modelgen import models

pytestmark = pytest.mark.gpu
DATA_IDS = lambda d: f"{d[0]}-{d[1]:g}"  # noqa: E731


def _hold(what, kernel, tile, prec, ys, yards, classify, vector, written=True):
    """every output finite and within its bound, element by element; the three requests distinguishable"""
    for d, (y, yd) in enumerate(zip(ys, yards)):
        assert np.isfinite(y).all(), (what, kernel, d, "the output is not finite")
        w = NR.worst_ratio(y, yd["ref"], yd["B"], yd["ce"], yd["extra"], classify)
        print(f"NORM_ROWS | {kernel} | tile {tile} | {prec} | {what} | draw {d} | c {w[1]:.2f} | c_emul {yd['ce']:.2f} | of the bound {w[0]:.3f}")
        assert w[0] <= 1.0, (what, d, NR.describe(kernel, tile, prec, w, yd["ce"]))
    if written:
        share, dead = NC.conclusive(yards, vector, nchw=yards[0]["ref"].ndim == 4)
        assert share <= 0.005 and dead == 0, (what, share, dead)


def _rows_class(c, tile, f16):
    lanes = CG.LANES[tile] or 64
    return lambda idx: NR.rows_class(idx, c, (8 if f16 else 4) if tile else 1, lanes, 256 // lanes)


def _row_tiles(tmp_path, case, tiles, prec, kind_step, label_of, yards, what, written, out_rows=NC.to_rows, check_plan=None, run=None):
    """the case on each tile of its table entry: plan, label, bound"""
    f16 = prec == "fp16"
    path = models.write_repo(str(tmp_path), case.name, case.mb)
    for tile in tiles:
        env = dict(IE_PRECISION=prec, **NC.force(tile))
        st = NC.step_of(plan_of(path, case.oshape[0], env), kind_step)
        assert st["tile"] == tile and st["out"]["f16"] is f16, (what, tile, st)
        if check_plan:
            check_plan(st)
        ys, kern = (run or run_model)(path, case.name, env, case.feeds, "y", case.oshape, by_step=True)
        assert dict(kern)[st["name"]] == label_of(tile, f16), (what, tile, kern)
        _hold(what, label_of(tile, f16), tile, prec, [out_rows(y) for y in ys], yards, _rows_class(case.c, tile, f16), 8 if f16 else 4, written)
        yield tile, ys


# ---- layer norm ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", NC.PRECS)
@pytest.mark.parametrize("kind, eps", NC.ROW_DATA, ids=map(DATA_IDS, NC.ROW_DATA))
@pytest.mark.parametrize("c", list(NC.LN_TILES))
def test_layer_norm(tmp_path, c, kind, eps, prec):
    case = NC.ln_case(c, kind, eps)
    yards = [NC.ln_yard(c, kind, eps, d, prec) for d in range(NC.DRAWS)]
    ran = [t for t, _ in _row_tiles(tmp_path, case, NC.tiles_of(NC.LN_TILES, c, prec), prec, "layer_norm", CG.ln_label, yards, f"layer norm C {c} {kind} eps {eps:g}", kind != "edges")]
    assert ran == list(NC.tiles_of(NC.LN_TILES, c, prec))


@pytest.mark.parametrize("prec", NC.PRECS)
@pytest.mark.parametrize("c", list(NC.LN_CONCAT_TILES))
def test_layer_norm_into_a_concat(tmp_path, c, prec):
    """pitch 2 C on both sides, channel offset C on the output; the conv in front is exact, so channels [0, C) of y are the norm's input bit for bit"""
    case = NC.ln_concat_case(c)
    yards = [NC.ln_concat_yard(c, d, prec) for d in range(NC.DRAWS)]

    def plan(st):
        assert (st["in"]["c_off"], st["in"]["pitch"], st["out"]["c_off"], st["out"]["pitch"]) == (0, 2 * c, c, 2 * c) and st["in"]["buf"] == st["out"]["buf"], st
    for _, ys in _row_tiles(tmp_path, case, NC.tiles_of(NC.LN_CONCAT_TILES, c, prec), prec, "layer_norm", CG.ln_label, yards, f"layer norm into a concat C {c}", True,
                            out_rows=lambda y: NC.to_rows(y)[:, c:], check_plan=plan):
        for y, rows in zip(ys, case.rows):
            assert np.array_equal(NC.to_rows(y)[:, :c], rows)


# ---- RMSNorm ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", NC.PRECS)
@pytest.mark.parametrize("kind, eps", NC.ROW_DATA, ids=map(DATA_IDS, NC.ROW_DATA))
@pytest.mark.parametrize("l, d", list(NC.RMS_TILES))
def test_rms_norm(tmp_path, l, d, kind, eps, prec):
    """in place: the norm is the last reader of its input.  The row of zeros of "edges" comes back as zeros exactly"""
    case = NC.rms_case(l, d, kind, eps)
    yards = [NC.rms_yard(l, d, kind, eps, dr, prec) for dr in range(NC.DRAWS)]
    if kind == "randn":          # in place the stale value is the request's own x: every vector has an element where x is outside the bound
        assert [NR.stale_input_check(case.rows[dr], yards[dr]["ref"], yards[dr]["bound"], 8 if prec == "fp16" else 4) for dr in range(NC.DRAWS)] == [0] * NC.DRAWS

    def plan(st):
        assert st["rms"] is True and NC.in_place(st), st
    for _, ys in _row_tiles(tmp_path, case, NC.tiles_of(NC.RMS_TILES, (l, d), prec), prec, "layer_norm", LG.rms_label, yards, f"RMSNorm L {l} D {d} {kind} eps {eps:g}", kind != "edges",
                            check_plan=plan):
        if kind == "edges":
            for y in ys:
                assert np.array_equal(NC.to_rows(y)[2], np.zeros(d, np.float32))


@pytest.mark.parametrize("prec", NC.PRECS)
@pytest.mark.parametrize("kind, eps", (("randn", 1e-5), ("near_eps", 1e-5)), ids=("randn", "near_eps"))
def test_rms_norm_not_the_last_reader(tmp_path, kind, eps, prec):
    """y = RMSNorm(x) + x: the norm writes another buffer, an eltwise step adds x (its rounding is in the yardstick)"""
    l, d = NC.RMS_ADD
    case = NC.rms_case(l, d, kind, eps, "add")
    yards = [NC.rms_yard(l, d, kind, eps, dr, prec, "add") for dr in range(NC.DRAWS)]

    def plan(st):
        assert st["rms"] is True and st["in"]["buf"] != st["out"]["buf"], st
    list(_row_tiles(tmp_path, case, NC.tiles_of(NC.RMS_TILES, (l, d), prec), prec, "layer_norm", LG.rms_label, yards, f"RMSNorm + x L {l} D {d} {kind}", True, check_plan=plan))


# ---- group norm ------------------------------------------------------------------------------------------------------------------------------
def _gn_tiles(tmp_path, shape, kind, eps, prec, act, inplace=False):
    n, c, h, w, g = shape
    f16 = NC.gn_out_f16(shape, prec)
    case = NC.gn_case(shape, kind, eps, act, inplace)
    yards = [NC.gn_yard(shape, kind, eps, d, "fp16" if f16 else "fp32", act, inplace) for d in range(NC.DRAWS)]
    path = models.write_repo(str(tmp_path), f"gn_{act}", case.mb)
    fits = (True, True) if inplace else NC.GN_TILE1[shape]
    for tile in (0, 1) if fits[prec == "fp16"] else (0,):
        env = dict(IE_PRECISION=prec, **NC.force(tile, "IE_GN_TILE" if inplace else "IE_FORCE_TILE"))
        plan = plan_of(path, n, env)
        st = NC.step_of(plan, "group_norm")
        assert st["tile"] == tile and st["out"]["f16"] is f16 and NC.in_place(st) == (inplace or NC.gn_in_place(shape, act)), (shape, tile, st)
        px, slabs = GG.gn_slabs(n, h * w, c, f16) if tile else (0, 0)
        if tile and shape in NC.GN_SLABS:
            assert (px, slabs) == NC.GN_SLABS[shape][f16] and plan["workspace_floats"] >= 3 * n * slabs * g
        ys, kern = run_model(path, f"gn_{act}", env, case.feeds, "y", case.oshape, by_step=True)
        label = GG.gn_label(tile, f16, act)
        assert dict(kern)[st["name"]] == label, (shape, tile, kern)
        what = f"group norm{' in place behind a conv' if inplace else ''} {shape} act {act} {kind} eps {eps:g}"
        _hold(what, label, tile, prec, ys, yards, lambda idx: NR.gn_class(idx, shape[:4], px), 8 if f16 else 4, written=kind != "edges" and h * w > 1 and act is None)
        if h * w == 1 and act is None and not f16:          # one element per group: beta, whatever the input (the bound there is 0: exactly)
            for y in ys:
                assert np.array_equal(y, np.broadcast_to(case.beta.reshape(1, c, 1, 1), y.shape))
    return case, yards


@pytest.mark.parametrize("prec", NC.PRECS)
@pytest.mark.parametrize("kind, eps", NC.GN_DATA, ids=map(DATA_IDS, NC.GN_DATA))
@pytest.mark.parametrize("shape", list(NC.GN_TILE1), ids=lambda s: "x".join(map(str, s)))
def test_group_norm(tmp_path, shape, kind, eps, prec):
    """both tiles where the plan accepts a forced tile 1, act none (out of place) and SiLU (in place: the staging copy of x dies at the norm)"""
    for act in NC.GN_ACTS:
        _gn_tiles(tmp_path, shape, kind, eps, prec, act)


@pytest.mark.parametrize("prec", NC.PRECS)
@pytest.mark.parametrize("kind", ("randn", "distinct"))
def test_group_norm_in_place_behind_a_conv(tmp_path, kind, prec):
    """gn_alias_graph's shape with identity convolutions: the norm overwrites a conv's result.  The stale value of an element is x itself"""
    for act in NC.GN_ACTS:
        case, yards = _gn_tiles(tmp_path, NC.GN_INPLACE, kind, 1e-5, prec, act, inplace=True)
        t = lambda a: a.transpose(0, 2, 3, 1)  # noqa: E731
        assert [NR.stale_input_check(t(x), t(y["ref"]), t(y["bound"]), 8 if prec == "fp16" else 4) for x, y in zip(case.xs, yards)] == [0] * NC.DRAWS


# ---- embed -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", NC.PRECS)
@pytest.mark.parametrize("kind, eps", NC.EMBED_DATA, ids=map(DATA_IDS, NC.EMBED_DATA))
@pytest.mark.parametrize("shape", list(NC.EMBED_TILES), ids=lambda s: "x".join(map(str, s)))
def test_embed(tmp_path, shape, kind, eps, prec):
    case = NC.embed_case(shape, kind, eps)
    yards = [NC.embed_yard(shape, kind, eps, d, prec) for d in range(NC.DRAWS)]

    def plan(st):
        assert st["ln"] is True, st
    list(_row_tiles(tmp_path, case, NC.tiles_of(NC.EMBED_TILES, shape, prec), prec, "embed", BG.embed_label, yards, f"embed {shape} {kind} eps {eps:g}", True, check_plan=plan))


@pytest.mark.parametrize("prec", NC.PRECS)
@pytest.mark.parametrize("l, v, d, pos", list(NC.SUM_TILES), ids=lambda s: str(s))
def test_embed_sum(tmp_path, l, v, d, pos, prec):
    """the sum-only form: `sum` is the step's own result, a token output [N, L, D]"""
    case = NC.sum_case(l, v, d, pos)
    yards = [NC.sum_yard(l, v, d, pos, dr, prec) for dr in range(NC.DRAWS)]

    def plan(st):
        assert st["ln"] is False, st

    def run(path, name, env, feeds, oname, oshape, by_step):
        """engine_run.run_model for the graph's two outputs at once; -> the `sum`s"""
        def go():
            m = B.CreateModel(path, name)
            try:
                outs = [B.OutputConfig("sum", Shape=[NC.N, l, d], DataType="FLOAT32"), B.OutputConfig("y", Shape=[NC.N, d, 1, l], DataType="FLOAT32")]
                ys = [{t.Name: t.Data.copy() for t in m.Infer([tensor(k, a) for k, a in f.items()], outs)}["sum"].reshape(NC.N, l, d) for f in feeds]
                return ys, [(p["name"], p["kernel"]) for p in B.Profile(m, 1)]
            finally:
                m.Destroy()
        return with_env(dict(IE_AUTOTUNE="0", **env), go)
    list(_row_tiles(tmp_path, case, NC.tiles_of(NC.SUM_TILES, (l, v, d, pos), prec), prec, "embed", G2.embed_sum_label, yards, f"embed sum L {l} D {d}", True,
                    out_rows=lambda y: y.reshape(-1, d), check_plan=plan, run=run))
