"""The hand-built junction-tail inputs (tests/junction_tail_cases.py) hold what they claim, by the exact reference alone (tests/detector_tail_ref.py): every case the
GPU test (tests/test_gpu_junction_tail.py) relies on is shown to occur here first."""
import numpy as np
import pytest

import detector_tail_ref as R
import junction_tail_cases as J

F = np.float32


def _pixels(rows):
    """the endpoint pixels (x, y) of lines with score >= 0.5, as the filter takes them"""
    out = []
    for r in rows:
        if r[4] < F(0.5):
            continue
        p = (r[:4].astype(F) * F(4)).astype(F)
        q = [int(np.float64(v) + 0.1) for v in p]
        out += [(q[0], q[1]), (q[2], q[3])]
    return out


@pytest.mark.parametrize("border", [4, 0])
def test_special_lines_hold_the_cases(border):
    s = J.special_lines(border)
    nms = R.simple_nms(J.heat_map(), 4)
    lines, junc = J.reference(s, border, nms)
    jset = {(int(x), int(y)) for _, x, y in junc}
    pix = _pixels(s)
    # two lines sharing an endpoint pixel: one junction
    assert pix.count((200, 200)) == 2 and (200, 200) in jset and len(junc) == len(jset)
    # endpoints on and beside the border lines: border and R - border are out, border + 1 and R - border - 1 are in
    for v, inside in ((border, False), (border + 1, True), (512 - border - 1, True), (512 - border, False)):
        assert (v, 120) in pix and (240, v) in pix
        assert ((v, 120) in jset) == inside and ((240, v) in jset) == inside
    # endpoints outside [0, 512) on every side: no junction, and the line's other endpoint still counts
    assert any(x < 0 for x, _ in pix) and any(y < 0 for _, y in pix) and any(x >= 512 for x, _ in pix) and any(y >= 512 for _, y in pix)
    assert all(0 < x < 512 and 0 < y < 512 for x, y in jset) and (280, 164) in jset and (288, 176) in jset
    # score exactly 0.5 (its endpoints count) and the float just below (they do not)
    sc = s[:, 4]
    at, below = s[sc == F(0.5)][0], s[sc == np.nextafter(F(0.5), F(0))][0]
    assert (int(at[0] * 4), int(at[1] * 4)) in jset and (int(below[0] * 4), int(below[1] * 4)) not in jset
    # lines that pass 0.5 and fail line_thr or the length test: not among the lines, their endpoints among the junctions
    weak = s[(sc >= F(0.5)) & (sc < R.LINE_THR)]
    assert len(weak) > 10 and len(lines) < (sc >= F(0.5)).sum()
    short = s[6]
    assert short[4] >= R.LINE_THR and (40, 40) in jset and not any(abs(l[0] - 40 * float(J.WS)) < 1e-9 and abs(l[2] - 88 * float(J.WS)) < 1e-9 and l[3] < 54 * float(J.HS)
                                                                   for l in lines)
    # junctions whose keep bit is 0 (score 0) and 1 (their score)
    assert (junc[:, 0] == 0).sum() >= 10 and (junc[:, 0] > 0).sum() >= 10
    # every run of lines fits the list tests' buffers
    for run in J.runs(border):
        assert len(J.reference(run, border, nms)[1]) < 64


@pytest.mark.parametrize("border", [4, 0])
def test_overflow_image_exceeds_every_capacity(border):
    nms = R.simple_nms(J.heat_map(), 4)
    assert len(J.reference(J.overflow_image(border), border, nms)[1]) > 64


def test_empty_image():
    lines, junc = J.reference(np.zeros((0, 5), F), 4, R.simple_nms(J.heat_map(), 4))
    assert lines.shape == (0, 4) and junc.shape == (0, 3)


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 23, 24, 63, 64])
def test_counted_images_have_their_count(n):
    rows = J.counted_image(n, 40 + n)
    lines, junc = J.reference(rows, 0, R.simple_nms(J.heat_map(), 4))
    assert len(junc) == n and len(lines) == 0
    if n >= 6:                                  # the corner pixels: a tap index of each is clipped to the descriptor map's edge, low side (floor(ix) = -1 -> 0: x < 3.5,
        kinds = set()                           # from ix = 63 (2 x - 7) / 1015) or high side (64 -> 63: two taps share a cell)
        for x, y in J.CORNERS:
            low, high = x < 3.5 or y < 3.5, len(set(R.desc_cells(x, y))) < 4
            assert (low or high) and (F(x), F(y)) in {(a, b) for _, a, b in junc}
            kinds |= {("low", low), ("high", high)}
        assert ("low", True) in kinds and ("high", True) in kinds
