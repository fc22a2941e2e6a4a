"""The line path between the stage-0 tensors and the line filter, one launcher at a time on hand-built input (tests/line_mid_ref.py; the properties of every case are
proved in tests/test_line_mid_ref_cpu.py): the junction-to-line match in both forms, the kept list and the unique pairs through wireframe_kernel's short AND long path, the
junctions' tap rows and projections from both sources, and stage 1 in its four forms with more line tiles than workgroups.  airfe_debug_line_mid stages the tensors into the
context's own buffers and runs the launchers production runs (include/airfe_debug.h); every output buffer is 0xFF bytes when the launches start.

Index work (match, kept list, pairs, tap rows, lines_adjusted) is compared for equality, whole buffers, poison included.  Projections and scores are compared with float64;
the gate is the float32 restatement's own error against float64 on the same case, times 4: a different summation order of the same float32 products stays inside it, a wrong
tap or a stale tile header moves an unsaturated score by orders of magnitude more.

Measured on an MI355X (LAB_NOTES.md section 14; every run records them through diag(...)): scores at 0.20 - 0.43 of the gate in every form — 2.1e-6 of 4.9e-6 on the
one-line case, 1.51e-5 of 7.1e-5 on the 18597 lines of the full-size case —, projections 1.6e-7 of 6.4e-7 (s1_junc_proj, either source) and 6.7e-8 of 4.0e-7
(s1h_junc_proj), split against f32 form at most 1.2e-6 of the project's 5e-6."""
import os

import numpy as np
import pytest

import line_mid_ref as R
from airslam_amd import api, weights
from conftest import GOLDEN
from gpu_common import diag

pytestmark = pytest.mark.gpu
F = np.float32
FORMS = {0: "chw", 1: "head_rows", 2: "tap_rows", 3: "tap_rows_split"}
_CTX, _RUNS, _ERR = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for c in _CTX.values():
        c.close()
    _CTX.clear()
    _RUNS.clear()


def _ctx():
    if "pl" not in _CTX:
        _CTX["pl"] = api.Context(superpoint=weights.synthetic_plnet_s0(1234), plnet_s1=os.path.join(GOLDEN, "plnet_s1.airfe"), max_batch=2, enc_chunk=2, check_launches=1)
    return _CTX["pl"]


def _call(case, j2l, form, wgs):
    B = len(case["juncs"])
    thin, aux, loi = R.stage_tensors(B)
    return _ctx().debug_line_mid(case["juncs"], case["lines_pred"], thin, aux, loi, case.get("iskeep"), case.get("idx_min"), case.get("idx_max"), j2l=j2l, s1_form=form, wgs=wgs)


def _run(kind, name, j2l, form, wgs=0):
    key = (kind, name, j2l, form, wgs)
    if key not in _RUNS:
        _RUNS[key] = _call(R.j2l_case(name) if kind == "j2l" else R.host_case(name), j2l, form, wgs)
    return _RUNS[key]


def _poison(a):
    return np.ascontiguousarray(a).view(np.int32) == -1


def _check_dedup(r, b, juncs, lines_pred, keep, pairs, rep, what):
    """image b of a run against the reference lists: counts, keep, pairs, rep, head4, prop4, the clean table, and the poison behind every list"""
    m1, m2 = len(keep), len(pairs)
    print(f"{what}[{b}]: M1 = {r['counts'][b, 0]} (reference {m1}), M2 = {r['counts'][b, 1]} (reference {m2}), table entries left behind: {r['table_dirty'][b]}")
    assert tuple(r["counts"][b]) == (m1, m2)
    np.testing.assert_array_equal(r["keep"][b, :m1], keep)
    np.testing.assert_array_equal(r["pairs"][b, :m2], pairs)
    np.testing.assert_array_equal(r["rep"][b, :m2], rep)
    assert _poison(r["keep"][b, m1:]).all() and _poison(r["pairs"][b, m2:]).all() and _poison(r["rep"][b, m2:]).all(), "an entry behind the lists was written"
    np.testing.assert_array_equal(r["head4"][b, :m2], np.concatenate([juncs[pairs[:, 0]], juncs[pairs[:, 1]]], 1).reshape(m2, 4))
    np.testing.assert_array_equal(r["prop4"][b, :m2], lines_pred[keep[rep]].reshape(m2, 4))
    assert _poison(r["head4"][b, m2:]).all() and _poison(r["prop4"][b, m2:]).all()
    assert r["table_dirty"][b] == 0, "wireframe_kernel must leave its pair table clean"


# ---------------------------------------------------------------------------------------------------------------- the junction-to-line match
@pytest.mark.parametrize("name", list(R.J2L_CASES))
def test_j2l_brute_force_and_cell_search(name):
    case = R.j2l_case(name)
    full, fast = _run("j2l", name, 1, 2), _run("j2l", name, 2, 2)
    for b, im in enumerate(case["images"]):
        keep, lo, hi, _, _ = im["ref"]
        kept = keep > 0
        print(f"{name}[{b}]: kept {int((full['iskeep'][b] > 0).sum())} (brute force) / {int((fast['iskeep'][b] > 0).sum())} (cell search) / {int(kept.sum())} (reference); "
              f"cell search idx differs from the full match on {int(((fast['idx_min'][b] != lo) | (fast['idx_max'][b] != hi)).sum())} proposals that are not kept")
        np.testing.assert_array_equal(full["iskeep"][b], keep)
        np.testing.assert_array_equal(full["idx_min"][b], lo)
        np.testing.assert_array_equal(full["idx_max"][b], hi)
        np.testing.assert_array_equal(fast["iskeep"][b], keep)
        np.testing.assert_array_equal(fast["idx_min"][b][kept], lo[kept])
        np.testing.assert_array_equal(fast["idx_max"][b][kept], hi[kept])
        for p, k, a, c in im["claims"]["expect"]:            # the hand-built rows by name (the reference holds the same: tests/test_line_mid_ref_cpu.py)
            assert (full["iskeep"][b, p], full["idx_min"][b, p], full["idx_max"][b, p]) == (k, a, c), (p, case["lines_pred"][b, p])
            assert fast["iskeep"][b, p] == k and (not k or (fast["idx_min"][b, p], fast["idx_max"][b, p]) == (a, c)), (p, case["lines_pred"][b, p])
        k_ref, pairs, rep = R.dedup_ref(keep, lo, hi)
        for r, what in ((full, f"{name} brute force, counted = false"), (fast, f"{name} cell search, counted = true")):
            _check_dedup(r, b, case["juncs"][b], case["lines_pred"][b], k_ref, pairs, rep, what)
    for k in ("counts", "keep", "pairs", "rep", "head4", "prop4", "lines_adjusted", "scores_line"):      # counted = true gives the bytes of counted = false
        np.testing.assert_array_equal(full[k].view(np.int32), fast[k].view(np.int32), err_msg=k)


# ---------------------------------------------------------------------------------------------------------------- kept list and unique pairs
@pytest.mark.parametrize("name", list(R.DEDUP_CASES))
def test_dedup_short_and_long_path(name):
    case, ref = R.host_case(name), R.host_ref(name)
    r = _run("host", name, 0, 2)
    again = _call(case, 0, 2, 0)                               # the same context, the table as the first call left it
    for b, x in enumerate(ref):
        for run, what in ((r, name), (again, name + " again")):
            _check_dedup(run, b, case["juncs"][b], case["lines_pred"][b], x["keep"], x["pairs"], x["rep"], what)
        np.testing.assert_array_equal(r["iskeep"][b], case["iskeep"][b])      # (host indices: staged, not recomputed)
    for k in r:
        np.testing.assert_array_equal(r[k].view(np.int32), again[k].view(np.int32), err_msg=k)


def test_long_path_then_short_path_on_one_table():
    """a long-path call (24000 kept), then short-path calls whose pairs the long one also held: a table entry left behind would hide their first proposals"""
    for name in ("m1_24000", "m1_8192", "m1_8193", "m1_1", "m1_24000"):
        case, ref = R.host_case(name), R.host_ref(name)
        r = _call(case, 0, 2, 0)
        _check_dedup(r, 0, case["juncs"][0], case["lines_pred"][0], ref[0]["keep"], ref[0]["pairs"], ref[0]["rep"], name + " in sequence")


# ---------------------------------------------------------------------------------------------------------------- tap rows and projections
@pytest.mark.parametrize("form", [1, 2, 3], ids=[FORMS[f] for f in (1, 2, 3)])
def test_tap_rows_and_projections(form):
    name = "m2_33" if form == 1 else "b2_unequal"
    case, ref = R.host_case(name), R.host_ref(name)
    r = _run("host", name, 0, form)
    worst = {}
    for b, x in enumerate(ref):
        if form >= 2:
            np.testing.assert_array_equal(r["ridx"][b], R.tap_rows(case["juncs"][b]) + b * R.NPX)
        else:
            assert _poison(r["ridx"]).all()
        err = float(np.abs(r["proj"][b].astype(np.float64) - x["proj64"]).max())
        gate = 4 * x["proj32_err"]
        worst[f"image{b}"] = [err, gate]
        print(f"projections, {FORMS[form]}[{b}]: max |device - float64| = {err:.3e}, gate 4 x {x['proj32_err']:.3e} = {gate:.3e}")
        assert np.isfinite(r["proj"][b]).all() and err <= gate
    _ERR[f"proj/{FORMS[form]}"] = [worst[k] for k in sorted(worst)]
    diag("line_mid_pin_projections", **{k: v for k, v in sorted(_ERR.items()) if k.startswith("proj/")})      # [error, gate] per image


def test_projection_sources_agree():
    """head rows (pitch 160) and gathered tap rows feed the same kernel the same values: the same bytes"""
    a, b = _run("host", "m2_33", 0, 1), _run("host", "m2_33", 0, 2)
    np.testing.assert_array_equal(a["proj"], b["proj"])
    np.testing.assert_array_equal(a["scores_line"].view(np.int32), b["scores_line"].view(np.int32))


# ---------------------------------------------------------------------------------------------------------------- stage 1
def _check_stage1(name, form, wgs):
    case, ref = R.host_case(name), R.host_ref(name)
    r = _run("host", name, 0, form, wgs)
    base = _run("host", name, 0, form, 0)
    for b, x in enumerate(ref):
        m2 = len(x["pairs"])
        assert r["counts"][b, 1] == m2
        np.testing.assert_array_equal(r["lines_adjusted"][b, :m2], x["la"])
        assert _poison(r["scores_line"][b, m2:]).all(), "a score slot at or beyond M2 was written"
        if form != 3:                                          # (form 3 reads lines_adjusted where launch_wireframe left it: head4, checked with the pairs)
            assert _poison(r["lines_adjusted"][b, m2:]).all()
        if m2:
            sc = r["scores_line"][b, :m2]
            err = float(np.abs(sc.astype(np.float64) - x["scores64"]).max())
            gate = 4 * x["e32"]
            print(f"{name}[{b}] {FORMS[form]} wgs {wgs}: M2 = {m2}, max |device - float64| = {err:.3e}, gate 4 x {x['e32']:.3e} = {gate:.3e}, "
                  f"|float32 restatement - device| = {float(np.abs(sc - x['scores32']).max()):.3e}")
            _ERR[f"score/{name}[{b}]/{FORMS[form]}/wgs{wgs}"] = [err, gate]
            assert np.isfinite(sc).all() and err <= gate
    for k in ("lines_adjusted", "scores_line", "proj", "pairs", "rep", "keep", "counts"):      # any grid gives the default grid's bytes
        np.testing.assert_array_equal(r[k].view(np.int32), base[k].view(np.int32), err_msg=f"{k}: wgs = {wgs} against the default grid")
    diag("line_mid_pin_scores", **{k: v for k, v in sorted(_ERR.items()) if k.startswith("score/")})      # [error, gate] per image, form and grid


@pytest.mark.parametrize("wgs", (0,) + R.STAGE1_WGS)
@pytest.mark.parametrize("form", list(FORMS), ids=list(FORMS.values()))
@pytest.mark.parametrize("name", list(R.STAGE1_CASES))
def test_stage1_tiles(name, form, wgs):
    if form <= 1 and len(R.STAGE1_CASES[name]) > 1:
        with pytest.raises(api.AirfeError, match="one image"):
            _call(R.host_case(name), 0, form, wgs)
        return
    _check_stage1(name, form, wgs)


@pytest.mark.parametrize("form", list(FORMS), ids=list(FORMS.values()))
def test_stage1_full_size_at_the_default_grid(form):
    """18597 unique lines through 512 workgroups of 32: 70 workgroups take a second tile; the dedup's long path feeds it"""
    assert len(R.host_ref(R.FULL_CASE)[0]["pairs"]) > 512 * 32
    _check_stage1(R.FULL_CASE, form, 0)


@pytest.mark.parametrize("name", ["m2_33", "m2_100", "b2_unequal", R.FULL_CASE])
def test_split_form_agrees_with_the_f32_form(name):
    """plnet_s1h_kernel against plnet_s1_kernel<true> on the same tap rows: the project's 5e-6 (tests/test_gpu_stage1_split.py)"""
    a, b = _run("host", name, 0, 2), _run("host", name, 0, 3)
    worst = 0.0
    for i, x in enumerate(R.host_ref(name)):
        m2 = len(x["pairs"])
        worst = max(worst, float(np.abs(a["scores_line"][i, :m2] - b["scores_line"][i, :m2]).max()))
        np.testing.assert_array_equal(a["lines_adjusted"][i, :m2], b["lines_adjusted"][i, :m2])
    _ERR[f"split/{name}"] = worst
    diag("line_mid_pin_split_vs_f32", **{k: v for k, v in sorted(_ERR.items()) if k.startswith("split/")})
    print(f"{name}: max |split - f32| score = {worst:.3e}")
    assert worst <= 5e-6


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_context_usable():
    ctx = _ctx()
    one = R.host_case("m2_33")
    thin, aux, loi = R.stage_tensors(1)
    args = (one["juncs"], one["lines_pred"], thin, aux, loi)
    idx = (one["iskeep"], one["idx_min"], one["idx_max"])
    z = lambda *s: np.zeros(s, F)
    with pytest.raises(api.AirfeError, match="arena"):
        ctx.debug_line_mid(z(3, 300, 2), z(3, R.NP, 4), z(3, 4, 128, 128), z(3, 4, 128, 128), z(3, R.NPX, 128), j2l=1)      # (max_batch = 2)
    with pytest.raises(api.AirfeError, match="j2l = 0 needs"):
        ctx.debug_line_mid(*args, j2l=0)
    for wgs in (-1, 513):
        with pytest.raises(api.AirfeError, match="wgs"):
            ctx.debug_line_mid(*args, *idx, wgs=wgs)
    with pytest.raises(api.AirfeError, match="s1_form"):
        ctx.debug_line_mid(*args, *idx, s1_form=4)
    bad = one["juncs"].copy()
    bad[0, 5, 0] = np.nan
    with pytest.raises(api.AirfeError, match="finite"):
        ctx.debug_line_mid(bad, *args[1:], *idx)
    r = ctx.debug_line_mid(*args, *idx, s1_form=2)
    np.testing.assert_array_equal(r["scores_line"].view(np.int32), _run("host", "m2_33", 0, 2)["scores_line"].view(np.int32))
