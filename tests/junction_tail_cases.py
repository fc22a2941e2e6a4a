"""Hand-built inputs for the junction tail of the batched line path (tests/test_junction_tail_ref_cpu.py, tests/test_gpu_junction_tail.py): the special lines of
detector_tail_ref.line_post — plus endpoints outside the map on either side — cut into five runs short enough that every junction of a run fits a 64-row buffer, and
lines that give an image an exact number of junctions.  numpy only; the exact reference is detector_tail_ref's line_filter + junction_detector."""
import numpy as np

import detector_tail_ref as R

F = np.float32
H, W = 480, 752
WS, HS = F(W) / F(512), F(H) / F(512)


def special_lines(border):
    """[n, 5] (x1, y1, x2, y2, score): line_post's special lines and four more with an endpoint left of, above, right of and below the map"""
    lp = R.line_post(border, (1024,))
    n = lp["n_special"]
    rows = np.concatenate([lp["la"][0, :n], lp["sc"][0, :n, None]], 1)
    out = np.array([(-1.0, 40.0, 70.0, 41.0, 0.6), (40.0, -0.5, 71.0, 42.0, 0.6), (130.0, 43.0, 72.0, 44.0, 0.6), (45.0, 129.0, 73.0, 46.0, 0.6)], F)
    return np.concatenate([rows, out]).astype(F)


def runs(border):
    """the special lines in five runs"""
    return np.array_split(special_lines(border), 5)


def list_batch(border, B):
    """the images of the list test's batch of B: three runs (B = 3); the overflow image, a run, an image without lines, the last run (B = 4)"""
    r = runs(border)
    return r[:3] if B == 3 else [overflow_image(border), r[3], np.zeros((0, 5), F), r[4]]


def pack(images):
    """list of [m2_b, 5] line arrays -> la [B, ld, 4], sc [B, ld], m2 [B]"""
    ld = max(max(len(i) for i in images), 1)
    la, sc = np.zeros((len(images), ld, 4), F), np.zeros((len(images), ld), F)
    for b, rows in enumerate(images):
        la[b, :len(rows)], sc[b, :len(rows)] = rows[:, :4], rows[:, 4]
    return la, sc, np.array([len(i) for i in images], np.int32)


def overflow_image(border):
    """line_post's 1023-line image: hundreds of distinct endpoint pixels, more than any capacity used here"""
    lp = R.line_post(border, (1023,))
    return np.concatenate([lp["la"][0], lp["sc"][0, :, None]], 1).astype(F)


def heat_map():
    return R.nms_spacing()["maps"][0]


def reference(rows, border, nms):
    """(lines float64 [L, 4], junction rows [J, 3] = score, x, y unscaled) of one image's lines"""
    lines, jmap = R.line_filter(rows[:, :4], rows[:, 4], border, R.LINE_THR, R.LEN_THR, WS, HS)
    return lines, R.junction_detector(jmap, nms, border)


CORNERS = [(1, 1), (511, 1), (1, 511), (511, 511), (3, 3), (508, 2)]      # (x, y) whose bilinear taps clip at the descriptor map's edge (border 0)


def counted_image(n, seed):
    """n lines with ONE junction each (the other endpoint lies right of the map): n distinct pixels, the corner pixels first, score 0.6 (kept by neither line test)"""
    rng = np.random.default_rng(seed)
    pix = list(CORNERS[:n])
    seen = set(pix)
    while len(pix) < n:
        p = (int(rng.integers(1, 512)), int(rng.integers(1, 512)))
        if p not in seen:
            seen.add(p)
            pix.append(p)
    return np.array([(x / 4, y / 4, 130.0, 64.0, 0.6) for x, y in pix], F).reshape(-1, 5)
