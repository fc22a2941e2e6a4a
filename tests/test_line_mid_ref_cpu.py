"""The references and cases of tests/line_mid_ref.py, proved without a device: every property a case claims follows from the references alone, the float64 match equals the
float32 contract (oracle.ref_nets.j2l_match) on every j2l case, the float64 stage 1 agrees with the float32 restatement of plnet_s1.onnx, and the planted defects the GPU
tests must catch (no tie rule, <= at the threshold, a stale tile header, a long path that forgets its table) move the expected outputs of at least one case."""
import numpy as np
import pytest

import line_mid_ref as R
from oracle import ref_nets

F = np.float32
CELL = 4


def _cell(v):
    return np.minimum(31, np.maximum(0, (np.asarray(v, np.float64) / CELL).astype(np.int64)))


# ---------------------------------------------------------------------------------------------------------------- j2l
@pytest.mark.parametrize("name", list(R.J2L_IMAGES))
def test_j2l_image_is_exact_and_busy(name):
    im = R.j2l_image(name)
    keep, lo, hi, c1, c2 = im["ref"]
    for a in (im["juncs"], im["lines_pred"]):
        assert a.dtype == F and (a >= 0).all() and (a <= 128).all() and (a * 8 == np.round(a * 8)).all(), "multiples of 1/8 in [0, 128]"
    k32, lo32, hi32 = ref_nets.j2l_match(im["lines_pred"], im["juncs"], R.THR)          # float32, operation by operation: the same decisions everywhere
    np.testing.assert_array_equal(keep, k32)
    np.testing.assert_array_equal(lo, lo32)
    np.testing.assert_array_equal(hi, hi32)
    print(f"{name}: {int(keep.sum())} of {R.NP} proposals kept, {len(im['claims']['expect'])} hand-built")
    assert keep.sum() >= 2000
    for p, k, a, b in im["claims"]["expect"]:
        assert (keep[p], lo[p], hi[p]) == (k, a, b), (name, p, im["lines_pred"][p])
    # the defects the device tests must see: `<=` at the threshold changes a decision, and so does a search confined to the end point's OWN cell
    at_thr = (c1 == R.THR) | (c2 == R.THR)
    if name in ("threshold", "padding"):
        assert (at_thr & (lo < hi) & (c1 <= R.THR) & (c2 <= R.THR)).any(), "a proposal that `<=` would keep"


def test_tie_cases_put_the_lower_index_in_the_later_cell():
    im = R.j2l_image("ties")
    j = im["juncs"]
    raster = lambda p: int(_cell(p[1]) * 32 + _cell(p[0]))
    d2 = lambda p, q: float((p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2)
    for e, low, high in (((21, 21), 3, 10), ((60, 60), 2, 41)):
        assert d2(e, j[low]) == d2(e, j[high]) == 4.0 and raster(j[low]) > raster(j[high]), "equidistant, the lower index later in the cell walk"
        others = np.delete(np.arange(300), [low, high])
        assert ((j[others] - np.array(e, F)) ** 2).sum(1).min() > 4.0
    assert (j[7] == j[50]).all() and (j[7] == j[200]).all()
    # a walk in cell order that keeps the FIRST minimum it meets (no tie rule) answers 10 and 41: the expected rows differ
    exp = {p: (a, b) for p, k, a, b in im["claims"]["expect"] if k}
    assert any(3 in v for v in exp.values()) and any(2 in v for v in exp.values()) and any(7 in v for v in exp.values())
    swapped = [p for p in exp if im["lines_pred"][p][0] == 100]                          # the partner first: i1 > i2 for partner 120, i1 < i2 for partner 0
    assert len(swapped) >= 4


def test_padding_case():
    im = R.j2l_image("padding")
    j = im["juncs"]
    assert (j[37:] == 0).all() and (np.abs(j[:37]).max(1) >= 10).all() and len({tuple(p) for p in j[:37].tolist()}) == 37
    keep, lo, hi, _, _ = im["ref"]
    both = [(p, k) for p, k, a, b in im["claims"]["expect"] if a == b == 37]
    assert len(both) >= 5 and all(k == 0 for _, k in both)
    assert (hi[keep > 0] <= 37).all(), "no kept proposal names a padding row behind the first"
    assert ((hi == 37) & (keep > 0)).sum() > 100


def test_threshold_offsets():
    below, at, above = R.below_threshold_offsets()
    s = lambda o: o[0] ** 2 + o[1] ** 2
    assert s(at) == 640 and s(below) < 640 < s(above)
    sums = {a * a + b * b for a in range(40) for b in range(40)}
    assert not any(s(below) < v < 640 or 640 < v < s(above) for v in sums), "the nearest representable squared distances on either side of 10"
    assert 639 not in sums
    im = R.j2l_image("threshold")
    kept = {k for _, k, _, _ in im["claims"]["expect"]}
    assert kept == {0, 1}
    _, _, _, c1, c2 = im["ref"]
    got = {float(min(c1[p], c2[p]) + max(c1[p], c2[p])) for p, _, _, _ in im["claims"]["expect"]}
    assert got == {s(below) / 64, 10.0, s(above) / 64}


def test_cell_border_and_one_cell_cases():
    im = R.j2l_image("cell_borders")
    j = im["juncs"]
    assert (j % 4 == 0).all() and (j == 128).any() and len({tuple(p) for p in j.tolist()}) == 300
    l = im["lines_pred"]
    keep = im["ref"][0] > 0
    ends = np.concatenate([l[keep, :2], l[keep, 2:]])
    cells = _cell(ends)
    assert (cells == 0).any() and (cells == 31).any() and (ends % 4 == 0).all(1).sum() > 100, "kept end points in cells 0 and 31 and on multiples of 4"
    assert any(tuple(l[p][:2]) == (22.0, 22.0) for p, _, _, _ in im["claims"]["expect"]) and any(tuple(l[p][:2]) == (127.0, 64.0) for p, _, _, _ in im["claims"]["expect"])
    one = R.j2l_image("one_cell")
    c = _cell(one["juncs"])
    assert (c[:, 0] == 10).all() and (c[:, 1] == 12).all() and len({tuple(p) for p in one["juncs"].tolist()}) == 300


def test_two_image_case_holds_different_images():
    c = R.j2l_case("two_images")
    assert c["juncs"].shape == (2, 300, 2) and not np.array_equal(c["juncs"][0], c["juncs"][1]) and not np.array_equal(c["lines_pred"][0], c["lines_pred"][1])


# ---------------------------------------------------------------------------------------------------------------- dedup
def _counts(name):
    return [(len(r["keep"]), len(r["pairs"])) for r in R.host_ref(name)]


def test_dedup_cases_reach_what_they_claim():
    assert _counts("m1_0") == [(0, 0)] and _counts("m1_1") == [(1, 1)]
    assert _counts("m1_8192")[0][0] == R.SHORT_MAX and _counts("m1_8193")[0][0] == R.SHORT_MAX + 1
    m1, m2 = _counts("m1_24000")[0]
    print(f"m1_24000: M1 = {m1}, M2 = {m2}")
    assert m1 == 24000 and 18000 < m2 < 19200 and m2 > 16384, "more unique lines than one pass of the default grid (512 workgroups of 32 lines)"
    assert _counts("one_pair") == [(20000, 1)]
    m1, m2 = _counts("dup6")[0]
    assert m1 == 20000 and 3000 < m2 <= 3333
    eq = R.host_ref("equal_ends")[0]
    assert len(eq["keep"]) == 9000 and (eq["pairs"][:, 0] == eq["pairs"][:, 1]).all()
    un = R.host_ref("m1_24000")[0]
    assert (un["pairs"][:, 0] == un["pairs"][:, 1]).any() and (un["pairs"][:, 0] >= un["pairs"][:, 1]).all()
    (q, _), (r, _) = _counts("bunched")
    kq, kr = R.host_ref("bunched")[0]["keep"], R.host_ref("bunched")[1]["keep"]
    assert q == R.WF_RUN // 4 and (kq // R.WF_RUN == 5).all() and ((kq % R.WF_RUN) // (R.WF_RUN // 4) == 2).all(), "one wave's quarter of one wf_emit run"
    assert r == R.WF_RUN and (kr // R.WF_RUN == 47).all()
    assert _counts("long_and_empty")[0][0] == 20000 and _counts("long_and_empty")[1] == (0, 0)


@pytest.mark.parametrize("name", list(R.DEDUP_CASES) + list(R.STAGE1_CASES))
def test_host_index_cases_are_well_formed(name):
    c = R.host_case(name)
    for b, r in enumerate(R.host_ref(name)):
        k = c["iskeep"][b]
        assert (k < 0).sum() > 1000, "negative values elsewhere"
        if len(r["keep"]) > 1:
            assert len(np.unique(k[k > 0])) > 1 and not (k[k > 0] == 1).all(), "kept = any positive value, not only 1"
        assert (c["idx_min"][b] <= c["idx_max"][b]).all() and c["idx_min"][b].min() >= 0 and c["idx_max"][b].max() < 300
        # rep is the FIRST proposal of its pair, pairs are in first-seen order
        a, bb = c["idx_min"][b][r["keep"]].astype(int), c["idx_max"][b][r["keep"]].astype(int)
        code = a * 300 + bb
        first = {}
        for pos, v in enumerate(code.tolist()):
            first.setdefault(v, pos)
        assert list(first.values()) == r["rep"].tolist()
        assert [(v % 300, v // 300) for v in first] == [tuple(p) for p in r["pairs"].tolist()]


def test_long_path_defects_move_the_expected_outputs():
    """what mutation 1 of the pull request does to wireframe_kernel's long path, on the reference: a first-proposal test against k + 1 finds no pair at all, and a table that
    is not cleaned after m1_24000 changes the NEXT call's pairs"""
    a = R.host_ref("m1_24000")[0]
    b = R.host_ref("dup6")[0]
    assert len(a["keep"]) > R.SHORT_MAX and len(b["keep"]) > R.SHORT_MAX
    # the stale table holds, per pair of the first call, its first position: a pair of the second call whose first position is LATER than that would not be found first
    stale = {tuple(p): int(k) for p, k in zip(a["pairs"].tolist(), a["rep"].tolist())}
    lost = sum(1 for p, k in zip(b["pairs"].tolist(), b["rep"].tolist()) if stale.get(tuple(p), 1 << 30) < k)
    assert lost > 100


# ---------------------------------------------------------------------------------------------------------------- stage 1
def test_stage1_junctions_and_proposals():
    for b in range(2):
        j, l = R.s1_juncs(b), R.s1_lines(b)
        assert (j[:12] < 0.5).any() and (j[:12] > 127.5).any() and (j[280:] == 0).all()
        assert ((j[:12] % 1) == 0.5).any(), "exactly on x.5: bilinear weights 0 and 1"
        assert not (j == 127.5).any()
        rows = R.tap_rows(j)
        assert rows.min() >= 0 and rows.max() < R.NPX and (rows[280:] == [0, 128, 1, 129]).all()
        assert (rows[1] == R.NPX - 1).all(), "(127.75, 127.9): all four taps clamp to the last pixel"
        assert ((l == 0) | (l == 128)).all(1).sum() >= 300, "proposals that join map corners"


@pytest.mark.parametrize("name", list(R.STAGE1_CASES) + list(R.DEDUP_CASES))
def test_stage1_reference_agrees_with_the_float32_restatement(name):
    """float64 against oracle.ref_nets.plnet_s1_forward (float32, the restatement pinned to the real graph): e32 is the gate's unit on the device (4 e32 per case)"""
    want = dict(R.STAGE1_CASES).get(name)
    for b, r in enumerate(R.host_ref(name)):
        sc = r["scores64"]
        if want is not None:
            assert len(sc) == want[b][0]
        if not len(sc):
            continue
        mid = float(((sc > 0.05) & (sc < 0.95)).mean())
        print(f"{name}[{b}]: M2 = {len(sc)}, e32 = {r['e32']:.3e}, projection float32 error {r['proj32_err']:.3e}, scores in (0.05, 0.95): {mid:.2f}, above 0.75: "
              f"{float((sc > 0.75).mean()):.2f}, distance from the sampler's discontinuity {r['margin']:.2e}")
        assert mid >= 0.5, "saturated scores hide errors"
        assert r["margin"] > 1e-4, "a sample point within rounding of x = 127.5 is decided by the last bit"
        assert 0 < r["e32"] < 5e-5 and 0 < r["proj32_err"] < 1e-6
        np.testing.assert_array_equal(r["la"][:, :2], R.s1_juncs(b)[r["pairs"][:, 0]])
    if name == "m2_31":
        r = R.host_ref(name)[0]
        used = set(r["pairs"].reshape(-1).tolist())
        assert {0, 1, 2, 3, 4, 5, 6, 7, 280, 299} <= used, "the special junctions are line ends"
        assert ((r["li"] == 0) | (r["li"] == 128)).all(1).any(), "a first proposal that joins map corners"


def test_a_stale_tile_header_moves_the_scores():
    """mutation 2 (the next tile's header fetched from the current tile): tile 1 of m2_100 at one workgroup would be scored with tile 0's lines — far outside the gate"""
    r = R.host_ref("m2_100")[0]
    sc = r["scores64"]
    assert np.abs(sc[32:64] - sc[0:32]).max() > 0.1 and np.abs(sc[32:64] - sc[0:32]).max() > 1000 * 4 * r["e32"]
    assert not np.array_equal(r["la"][32:64], r["la"][0:32])


def test_a_wrong_tap_clamp_moves_projections_and_scores():
    """mutation 5 (x1 clamped to W - 2): a junction whose x1 tap is column 127 reads column 126 instead — the tap rows differ, and so does the projection"""
    j = R.s1_juncs(0)
    rows = R.tap_rows(j)
    assert (rows[:, 2] % 128 == 127).any()
