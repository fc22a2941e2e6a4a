"""Plain references and hand-built cases for the line path between the stage-0 tensors and the line filter (airfe_debug_line_mid, include/airfe_debug.h):
the junction-to-line match (s0_j2l_kernel / s0_j2l_grid_kernel), the kept list and the unique pairs (wf_count / wf_emit / wireframe_kernel), the junctions' tap rows and
projections (s1_junc_rows / s1_junc_proj / s1h_junc_proj) and stage 1 (plnet_s1_kernel<false|true>, plnet_s1h_kernel).  numpy / torch-CPU only, no device code.

  j2l_f64        float64 squared distances, first minimum, lo < hi, both < thr
  dedup_ref      oracle.ref_post.wireframe_matcher + rep = position in keep of every unique pair's first proposal
  tap_rows       the four rows a junction's bilinear sample reads, in bil_eval's order i00, i10, i01, i11
  stage1_f64     oracle.ref_nets.plnet_s1_forward restated in float64 (+ the junction projections W0[:, 0:128] . loi(j), W0[:, 128:256] . loi(j))

The case builders live here so that tests/test_line_mid_ref_cpu.py (which proves every claimed property from the references alone) and tests/test_gpu_line_mid_pin.py see the
same bytes.  A case is a dict of [B, ...] arrays: juncs [B, 300, 2], lines_pred [B, 49152, 4], and either nothing more (the j2l cases: the device matches) or iskeep / idx_min /
idx_max [B, 49152] (the dedup and stage-1 cases: host indices).  thin / aux / loi of image b are seeded by b alone (stage_inputs) and shared by every case.

Every j2l coordinate is a multiple of 1/8 in [0, 128]: differences, squares and their sums are exact in float32 (at most 2 * 1024^2 / 64 needs 21 bits), so float32 and
float64 take the same decisions and "exact" needs no rounding argument."""
from __future__ import annotations

import functools
import os

import numpy as np
import torch

from conftest import GOLDEN
from oracle import ref_post

F = np.float32
NP, JN, FH, NPX = 3 * 128 * 128, 300, 128, 128 * 128
LINE_CAP = 45056
THR = 10.0
WF_RUN = NP // 48                     # proposals per wf_emit workgroup (48 runs of 1024; a wave owns a quarter: 256)
SHORT_MAX = 16 * 8 * 64               # kept proposals wireframe_kernel's short path holds in registers: 8192


@functools.lru_cache(maxsize=None)
def s1_weights():
    from airslam_amd import weights
    return weights.load_pack(os.path.join(GOLDEN, "plnet_s1.airfe"))


# ================================================================================================================ references
def j2l_f64(lines: np.ndarray, juncs: np.ndarray, thr: float = THR):
    """-> iskeep, idx_min, idx_max [n] float32 and the two nearest squared distances [n] float64"""
    l, j = lines.astype(np.float64), juncs.astype(np.float64)
    n = l.shape[0]
    i1, i2 = np.zeros(n, np.int64), np.zeros(n, np.int64)
    c1, c2 = np.zeros(n), np.zeros(n)
    for s in range(0, n, 8192):
        e = slice(s, s + 8192)
        d1 = (l[e, None, 0] - j[None, :, 0]) ** 2 + (l[e, None, 1] - j[None, :, 1]) ** 2
        d2 = (l[e, None, 2] - j[None, :, 0]) ** 2 + (l[e, None, 3] - j[None, :, 1]) ** 2
        i1[e], i2[e] = d1.argmin(1), d2.argmin(1)                       # (argmin: the first minimum)
        c1[e], c2[e] = d1.min(1), d2.min(1)
    lo, hi = np.minimum(i1, i2), np.maximum(i1, i2)
    keep = (lo < hi) & (c1 < thr) & (c2 < thr)
    return keep.astype(F), lo.astype(F), hi.astype(F), c1, c2


def dedup_ref(iskeep, idx_min, idx_max):
    """-> keep [M1], pairs [M2, 2] as (max, min), rep [M2]: position in keep of the first proposal of every unique pair (first-seen order)"""
    keep, inverse, pairs = ref_post.wireframe_matcher(iskeep, idx_min, idx_max)
    rep = np.zeros(len(pairs), np.int64)
    rep[inverse[::-1]] = np.arange(len(inverse))[::-1]                  # the first k with inverse[k] == u
    return keep, pairs, rep


def _taps(x, y, size=FH):
    """bil_setup in the dtype of x / y: tap coordinates x0, y0, x1, y1 (as floats) and the shifted point"""
    px, py = x - 0.5, y - 0.5
    x0, y0 = np.clip(np.floor(px), 0, size - 1), np.clip(np.floor(py), 0, size - 1)
    x1, y1 = np.clip(x0 + 1, 0, size - 1), np.clip(y0 + 1, 0, size - 1)
    return px, py, x0, y0, x1, y1


def tap_rows(juncs: np.ndarray) -> np.ndarray:
    """[300, 4] rows of the image's [128*128] pixel list in bil_eval's order i00, i10, i01, i11 (x - 0.5 is exact in float32 for every x < 2^22, so is the floor)"""
    _, _, x0, y0, x1, y1 = _taps(juncs[:, 0].astype(np.float64), juncs[:, 1].astype(np.float64))
    x0, y0, x1, y1 = (v.astype(np.int64) for v in (x0, y0, x1, y1))
    return np.stack([y0 * FH + x0, y1 * FH + x0, y0 * FH + x1, y1 * FH + x1], 1)


def _bil64(fm, x, y):
    """fm [P, C] pixel-major float64, x / y [n] float64 -> [n, C]; plnet_s1_forward's bil, term for term"""
    px, py, x0, y0, x1, y1 = _taps(x, y)
    i = lambda yy, xx: yy.astype(np.int64) * FH + xx.astype(np.int64)
    return (fm[i(y0, x0)] * ((y1 - py) * (x1 - px))[:, None] + fm[i(y1, x0)] * ((py - y0) * (x1 - px))[:, None]
            + fm[i(y0, x1)] * ((y1 - py) * (px - x0))[:, None] + fm[i(y1, x1)] * ((py - y0) * (px - x0))[:, None])


def stage1_f64(juncs, lines_pred, pairs, keep, rep, loi, thin, aux):
    """oracle.ref_nets.plnet_s1_forward in float64.  loi [16384, 128] pixel-major, thin / aux [4, 128, 128].
    -> lines_adjusted [M2, 4] float32 (a gather: exact), scores [M2] float64, proj [300, 256] float64, margin = the smallest distance of a sample coordinate from 127.5,
    the sampler's one discontinuity (inf without lines)"""
    w = {k: v.astype(np.float64) for k, v in s1_weights().items()}
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    m2 = len(pairs)
    la32 = np.concatenate([juncs[pairs[:, 0]], juncs[pairs[:, 1]]], 1).astype(F).reshape(m2, 4)
    li32 = lines_pred[np.asarray(keep, np.int64)[np.asarray(rep, np.int64)]].reshape(m2, 4)
    la, li = la32.astype(np.float64), li32.astype(np.float64)
    loi64 = loi.astype(np.float64)
    jf = _bil64(loi64, juncs[:, 0].astype(np.float64), juncs[:, 1].astype(np.float64))              # [300, 128]
    W0 = w["fc2.0.weight"]
    proj = np.concatenate([jf @ W0[:, 0:128].T, jf @ W0[:, 128:256].T], 1)
    t = torch.linspace(0, 1, 32)[1:-1].numpy().astype(np.float64)                                 # (the graph's constants are float32)

    margin = [np.inf, float(np.abs(juncs.astype(np.float64) - 127.5).min())]

    def along(fm, ln):
        px = ln[:, None, 0] * t[None] + ln[:, None, 2] * (1 - t)[None]
        py = ln[:, None, 1] * t[None] + ln[:, None, 3] * (1 - t)[None]
        if m2:
            margin.append(float(min(np.abs(px - 127.5).min(), np.abs(py - 127.5).min())))
        s = _bil64(fm.reshape(4, NPX).T.astype(np.float64), px.reshape(-1), py.reshape(-1))         # [M2 * 30, 4]
        return s.reshape(m2, 30, 4).transpose(0, 2, 1).reshape(m2, 120)                            # channel-major: c * 30 + j
    p_thin, p_aux = along(thin, la), along(aux, li)
    x = np.concatenate([jf[pairs[:, 0]], jf[pairs[:, 1]], p_thin, p_aux], 1)
    lin = lambda name, v: v @ w[name + ".weight"].T + w[name + ".bias"]
    relu = lambda v: np.maximum(v, 0)
    h = lin("fc2.4", relu(lin("fc2.2", relu(lin("fc2.0", x)))))
    h = h + relu(lin("fc2_res.0", np.concatenate([p_thin, p_aux], 1)))
    z = lin("fc2_head", h)
    z = z - z.max(1, keepdims=True)
    e = np.exp(z)
    return la32, e[:, 1] / e.sum(1), proj, min(margin)


def proj_f32(juncs, loi):
    """the junction projections float32 operation by operation in numpy (bilinear sample as plnet_s1_forward's bil, then a float32 matmul): the float32 restatement whose
    own error against float64 gates the device's"""
    x, y = juncs[:, 0].astype(F), juncs[:, 1].astype(F)
    px, py, x0, y0, x1, y1 = _taps(x, y)
    i = lambda yy, xx: yy.astype(np.int64) * FH + xx.astype(np.int64)
    jf = (loi[i(y0, x0)] * ((y1 - py) * (x1 - px))[:, None] + loi[i(y1, x0)] * ((py - y0) * (x1 - px))[:, None]
          + loi[i(y0, x1)] * ((y1 - py) * (px - x0))[:, None] + loi[i(y1, x1)] * ((py - y0) * (px - x0))[:, None]).astype(F)
    W0 = s1_weights()["fc2.0.weight"]
    return np.concatenate([jf @ W0[:, 0:128].T, jf @ W0[:, 128:256].T], 1).astype(F)


# ================================================================================================================ shared stage-1 tensors
AMPLITUDE = 0.2          # seeded normal; with the real weights most scores stay unsaturated (0.05 saturates 99 % of them and would hide errors)


@functools.lru_cache(maxsize=None)
def stage_inputs(b: int):
    """thin, aux [4, 128, 128], loi [16384, 128] of image slot b"""
    rng = np.random.default_rng(7000 + b)
    n = lambda *s: (rng.standard_normal(s) * AMPLITUDE).astype(F)
    return n(4, FH, FH), n(4, FH, FH), n(NPX, 128)


def eighths(rng, lo, hi, shape):
    """multiples of 1/8 in [lo, hi]"""
    return (rng.integers(int(lo * 8), int(hi * 8) + 1, shape).astype(F) / F(8)).astype(F)


# ================================================================================================================ j2l cases
def below_threshold_offsets():
    """(a, b) in eighths with a^2 + b^2 the largest sum of two squares below 10 * 64 (639 = 9 * 71 is none: 71 = 3 mod 4), and the smallest above it"""
    sums = {}
    for a in range(0, 26):
        for b in range(a, 26):
            sums.setdefault(a * a + b * b, (a, b))
    lo = max(s for s in sums if s < 640)
    hi = min(s for s in sums if s > 640)
    return sums[lo], sums[640], sums[hi]


def _fill(rng, juncs, lines, start, near=0.6):
    """filler proposals from `start` on: both ends near a random junction (offsets on the eighth grid in [-4, 4]) or anywhere on the map"""
    n = NP - start
    ja, jb = rng.integers(0, JN, n), rng.integers(0, JN, n)
    e = np.concatenate([juncs[ja] + eighths(rng, -4, 4, (n, 2)), juncs[jb] + eighths(rng, -4, 4, (n, 2))], 1)
    far = rng.random(n) > near
    e[far] = eighths(rng, 0, FH, (int(far.sum()), 4))
    lines[start:] = np.clip(e, 0, FH).astype(F)


def _scatter_juncs(rng, n, avoid, lo=0, hi=FH, margin=8.0):
    """n distinct eighth-grid junctions, none within `margin` (in x and in y) of a point of `avoid`"""
    out, seen = [], set()
    while len(out) < n:
        p = eighths(rng, lo, hi, (2,))
        if tuple(p) in seen or any(abs(p[0] - a[0]) < margin and abs(p[1] - a[1]) < margin for a in avoid):
            continue
        seen.add(tuple(p))
        out.append(p)
    return np.array(out, F)


def _image_ties(seed):
    """exact ties.  A: junctions 10 at (19, 21) [cell 4, 5] and 3 at (23, 21) [cell 5, 5] around the end point (21, 21): both at squared distance 4, the LOWER index in
    the LATER cell of the raster walk.  B: the same across two cell rows, 41 at (60, 58) [cell 15, 14] and 2 at (60, 62) [cell 15, 15] around (60, 60).  C: junctions 7, 50
    and 200 all at (30.5, 40.25).  Partners: junction 120 at (100, 20) (above every tied index) and junction 0 at (100, 100) (below)."""
    rng = np.random.default_rng(seed)
    spots = [(21, 21), (60, 60), (30.5, 40.25), (100, 20), (100, 100)]
    juncs = _scatter_juncs(rng, JN, spots)
    put = {10: (19, 21), 3: (23, 21), 41: (60, 58), 2: (60, 62), 7: (30.5, 40.25), 50: (30.5, 40.25), 200: (30.5, 40.25), 120: (100, 20), 0: (100, 100)}
    for k, p in put.items():
        juncs[k] = p
    ends = {"A": ((21, 21), 3), "B": ((60, 60), 2), "C": ((30.5, 40.25), 7), "C_near": ((31.5, 41.25), 7)}
    lines = np.zeros((NP, 4), F)
    expect = []                                            # (proposal, iskeep, idx_min, idx_max)
    k = 0
    for name, (e, win) in ends.items():
        for partner, pj in (((100, 20), 120), ((100, 100), 0)):
            for swap in (0, 1):
                lines[k] = (*e, *partner) if not swap else (*partner, *e)
                expect.append((k, 1, min(win, pj), max(win, pj)))
                k += 1
        lines[k] = (*e, *e)                                # i1 == i2: not kept
        expect.append((k, 0, win, win))
        k += 1
    lines[k] = (21, 21, 60, 60); expect.append((k, 1, 2, 3)); k += 1          # two tied ends in one proposal, i1 > i2
    lines[k] = (60, 60, 30.5, 40.25); expect.append((k, 1, 2, 7)); k += 1
    _fill(rng, juncs, lines, k)
    return juncs, lines, dict(expect=expect)


def _image_padding(seed):
    """37 real junctions and 263 rows of (0, 0) — what the line branch emits when jloc has fewer than 300 positive maxima.  End points near the origin: the nearest is
    row 37, the FIRST padding row; both ends there: not kept."""
    rng = np.random.default_rng(seed)
    juncs = np.zeros((JN, 2), F)
    juncs[:37] = _scatter_juncs(rng, 37, [(0, 0)], margin=10.0)
    lines = np.zeros((NP, 4), F)
    expect = []
    k = 0
    for e in ((0, 0), (0.5, 0.5), (1, 1), (2, 1), (0, 3), (3.125, 0), (1.75, 2.625)):
        for pj in (0, 5, 36):
            for swap in (0, 1):
                lines[k] = (*e, *juncs[pj]) if not swap else (*juncs[pj], *e)
                expect.append((k, 1, pj, 37))
                k += 1
        lines[k] = (*e, 1, 0.5)                            # both ends pick row 37
        expect.append((k, 0, 37, 37))
        k += 1
    lines[k] = (1, 3, *juncs[4]); expect.append((k, 0, 4, 37)); k += 1        # squared distance exactly 10 to the padding rows
    # filler: around the 38 distinct positions only (rows 0 .. 37)
    n = NP - k
    ja, jb = rng.integers(0, 38, n), rng.integers(0, 38, n)
    e = np.concatenate([juncs[ja] + eighths(rng, -4, 4, (n, 2)), juncs[jb] + eighths(rng, -4, 4, (n, 2))], 1)
    lines[k:] = np.clip(e, 0, FH).astype(F)
    return juncs, lines, dict(expect=expect)


def _image_threshold(seed):
    """squared distance exactly 10 (offsets 1, 3) is not kept; the largest eighth-grid value below 10 is kept, the smallest above is not — on either end, in every
    quadrant.  Junction 20 at (40, 40) stands alone; partner junction 150 at (90, 90)."""
    rng = np.random.default_rng(seed)
    juncs = _scatter_juncs(rng, JN, [(40, 40), (90, 90)], margin=10.0)
    juncs[20], juncs[150] = (40, 40), (90, 90)
    below, at, above = below_threshold_offsets()
    lines = np.zeros((NP, 4), F)
    expect = []
    k = 0
    for (a, b), kept in ((below, 1), (at, 0), (above, 0)):
        for dx, dy in ((a, b), (b, a), (-a, b), (a, -b), (-b, -a)):
            e = (40 + dx / 8, 40 + dy / 8)
            for swap in (0, 1):
                lines[k] = (*e, 90, 90) if not swap else (90, 90, *e)
                expect.append((k, kept, 20, 150))
                k += 1
    _fill(rng, juncs, lines, k)
    return juncs, lines, dict(expect=expect, offsets=(below, at, above))


def _image_cell_borders(seed):
    """every junction on a multiple of 4 (a cell's first row / column), 128.0 included (the clamp to cell 31); end points on multiples of 4, in the diagonal
    neighbour cell (offsets 2, 2), at 127.0 beside a junction at 128.0, and in cells 0 and 31 (the 3 x 3 block clipped at the map's edge)."""
    rng = np.random.default_rng(seed)
    grid = [(x, y) for y in range(0, 129, 4) for x in range(0, 129, 4)]
    must = [(0, 0), (128, 0), (0, 128), (128, 128), (128, 64), (64, 128), (24, 24), (40, 60), (0, 64)]
    # (the other three corners around the diagonal end points stay empty: the neighbour cell's junction is the only nearest)
    empty = [(20, 20), (24, 20), (20, 24), (44, 64), (44, 60), (40, 64), (36, 56), (36, 60), (40, 56), (124, 60), (124, 64), (128, 60)]
    rest = [g for g in grid if g not in must and g not in empty]
    pick = rng.permutation(len(rest))[:JN - len(must)]
    pts = must + [rest[i] for i in pick]
    order = rng.permutation(JN)
    juncs = np.array(pts, F)[order]
    at = {tuple(p): int(i) for i, p in enumerate(juncs.tolist())}
    partner = juncs[150]
    lines = np.zeros((NP, 4), F)
    expect = []
    k = 0
    specials = [((22, 22), (24, 24)), ((127, 64), (128, 64)), ((64, 127), (64, 128)), ((128, 128), (128, 128)), ((127, 127), (128, 128)), ((1, 1), (0, 0)),
                ((127.5, 0.5), (128, 0)), ((0.5, 127.5), (0, 128)), ((40, 60), (40, 60)), ((42, 62), (40, 60)), ((38, 58), (40, 60)), ((1, 65), (0, 64)), ((126, 62), (128, 64))]
    for e, j in specials:
        if tuple(map(float, j)) == tuple(partner.tolist()):
            continue
        for swap in (0, 1):
            lines[k] = (*e, *partner) if not swap else (*partner, *e)
            expect.append((k, 1, min(at[tuple(map(float, j))], 150), max(at[tuple(map(float, j))], 150)))
            k += 1
    # filler: end points on the eighth grid everywhere, a third of them on multiples of 4 themselves, a band along all four edges
    n = NP - k
    e = eighths(rng, 0, FH, (n, 4))
    on4 = rng.random(n) < 0.33
    e[on4] = (rng.integers(0, 33, (int(on4.sum()), 4)) * 4).astype(F)
    edge = rng.random(n) < 0.1
    e[edge, 0] = np.where(rng.random(int(edge.sum())) < 0.5, eighths(rng, 0, 3, int(edge.sum())), eighths(rng, 125, 128, int(edge.sum())))
    edge2 = rng.random(n) < 0.1
    e[edge2, 3] = np.where(rng.random(int(edge2.sum())) < 0.5, eighths(rng, 0, 3, int(edge2.sum())), eighths(rng, 125, 128, int(edge2.sum())))
    lines[k:] = e
    return juncs, lines, dict(expect=expect)


def _image_one_cell(seed):
    """all 300 junctions inside the 4 x 4 cell (10, 12): x in [40, 44), y in [48, 52)"""
    rng = np.random.default_rng(seed)
    pos = rng.permutation(32 * 32)[:JN]
    juncs = np.stack([F(40) + (pos % 32).astype(F) / F(8), F(48) + (pos // 32).astype(F) / F(8)], 1).astype(F)
    lines = np.zeros((NP, 4), F)
    n = NP
    ja, jb = rng.integers(0, JN, n), rng.integers(0, JN, n)
    lines[:] = np.clip(np.concatenate([juncs[ja] + eighths(rng, -4, 4, (n, 2)), juncs[jb] + eighths(rng, -4, 4, (n, 2))], 1), 0, FH)
    return juncs, lines, dict(expect=[])


J2L_IMAGES = {"ties": (_image_ties, 501), "padding": (_image_padding, 502), "threshold": (_image_threshold, 503), "cell_borders": (_image_cell_borders, 504),
              "one_cell": (_image_one_cell, 505)}
# case -> its images (two images in one call: stage_stride addressing, different content per grid row)
J2L_CASES = {"ties": ("ties",), "padding": ("padding",), "threshold": ("threshold",), "cell_borders": ("cell_borders",), "one_cell": ("one_cell",),
             "two_images": ("cell_borders", "padding")}


@functools.lru_cache(maxsize=None)
def j2l_image(name):
    fn, seed = J2L_IMAGES[name]
    juncs, lines, claims = fn(seed)
    ref = j2l_f64(lines, juncs)
    return dict(juncs=juncs, lines_pred=lines, claims=claims, ref=ref)


def j2l_case(name):
    imgs = [j2l_image(n) for n in J2L_CASES[name]]
    return dict(juncs=np.stack([i["juncs"] for i in imgs]), lines_pred=np.stack([i["lines_pred"] for i in imgs]), images=imgs)


# ================================================================================================================ stage-1 junctions and proposals
@functools.lru_cache(maxsize=None)
def s1_juncs(b: int):
    """300 junctions of image slot b: rows 0 .. 11 hold both tap clamps (below 0.5, above 127.5), exact x.5 coordinates (bilinear weights 0 and 1) and the map's corners; rows
    280 .. 299 are (0, 0) padding; the rest anywhere in [0, 128).  No coordinate is 127.5: there the graph's sampler is DISCONTINUOUS (x0 = x1 = 127 from px = 127 on: the
    weights cancel, the value drops from f[127] to 0), so a sample point within rounding of it is decided by the last bit — stage1_f64 reports every case's distance from it"""
    rng = np.random.default_rng(7100 + b)
    j = (rng.random((JN, 2), dtype=F) * F(FH)).astype(F)
    j[:12] = [(0.25, 0.3), (127.75, 127.9), (0.1, 64.3), (64.7, 127.6), (10.5, 20.5), (0.5, 0.5), (126.5, 0.5), (33.5, 77.25), (0, 0.4), (128, 128), (127.75, 3.2), (5.5, 0)]
    j[280:] = 0
    return j


@functools.lru_cache(maxsize=None)
def s1_lines(b: int):
    """49152 proposals of image slot b (what the aux samples are taken along): uniform in [0, 128), every 97th one joins two of the map's corners or edges"""
    rng = np.random.default_rng(7200 + b)
    l = (rng.random((NP, 4), dtype=F) * F(FH)).astype(F)
    corners = np.array([(0, 0, 128, 128), (128, 0, 0, 128), (0, 0, 0, 128), (128, 128, 0.2, 0.1), (127.9, 0.3, 64, 64), (0, 128, 128, 128)], F)
    idx = np.arange(0, NP, 97)
    l[idx] = corners[np.arange(len(idx)) % len(corners)]
    return l


def _indices_from_pairs(rng, where, a, b, scale=True):
    """iskeep / idx_min / idx_max [49152]: proposals `where` kept (any positive value, not only 1) with the junction pairs (a, b); negative and zero values and arbitrary
    in-range indices everywhere else"""
    iskeep = np.zeros(NP, F)
    other = np.setdiff1d(np.arange(NP), where)
    neg = other[rng.random(len(other)) < 0.3]
    iskeep[neg] = -(rng.random(len(neg), dtype=F) + F(0.001))
    iskeep[where] = (rng.random(len(where), dtype=F) * F(3) + F(0.001)).astype(F) if scale else F(1)
    x, y = rng.integers(0, JN, NP), rng.integers(0, JN, NP)
    imin, imax = np.minimum(x, y).astype(F), np.maximum(x, y).astype(F)
    imin[where], imax[where] = np.minimum(a, b), np.maximum(a, b)
    return iskeep, imin, imax


def _dedup_image(kind: str, seed: int):
    rng = np.random.default_rng(seed)
    pick = lambda n: np.sort(rng.choice(NP, n, replace=False))
    if kind == "m1_0":
        where = np.zeros(0, np.int64); a = b = np.zeros(0, np.int64)
    elif kind.startswith("uniform_"):                  # uniform pairs over all 300 junctions, a == b included
        where = pick(int(kind.split("_")[1]))
        a, b = rng.integers(0, JN, len(where)), rng.integers(0, JN, len(where))
    elif kind == "one_pair_20000":
        where = pick(20000)
        a, b = np.full(20000, 17), np.full(20000, 230)
    elif kind == "dup6_20000":
        where = pick(20000)
        pa, pb = rng.integers(0, JN, 20000 // 6), rng.integers(0, JN, 20000 // 6)
        u = rng.integers(0, len(pa), 20000)
        a, b = pa[u], pb[u]
    elif kind == "equal_ends":                         # every kept proposal has a == b
        where = pick(9000)
        a = b = rng.integers(0, JN, 9000)
    elif kind == "one_wave_quarter":                   # all kept proposals inside quarter 2 of wf_emit's run 5
        where = np.arange(5 * WF_RUN + 2 * (WF_RUN // 4), 5 * WF_RUN + 3 * (WF_RUN // 4))
        a, b = rng.integers(0, JN, len(where)), rng.integers(0, JN, len(where))
    elif kind == "last_run":                           # the whole of the last run, and nothing else
        where = np.arange(47 * WF_RUN, NP)
        a, b = rng.integers(0, JN, len(where)), rng.integers(0, JN, len(where))
    else:
        raise KeyError(kind)
    return _indices_from_pairs(rng, where, a, b)


# case -> (kind, seed) per image
DEDUP_CASES = {
    "m1_0": (("m1_0", 601),),
    "m1_1": (("uniform_1", 602),),
    "m1_8192": (("uniform_8192", 603),),                # the short path's last value
    "m1_8193": (("uniform_8193", 604),),                # the long path's first
    "m1_24000": (("uniform_24000", 605),),              # about 18600 unique pairs: the full-size stage-1 case
    "one_pair": (("one_pair_20000", 606),),
    "dup6": (("dup6_20000", 607),),
    "equal_ends": (("equal_ends", 608),),
    "bunched": (("one_wave_quarter", 609), ("last_run", 610)),
    "long_and_empty": (("dup6_20000", 611), ("m1_0", 612)),
}


def _stage1_image(m2: int, seed: int):
    """m2 unique pairs, each proposed two or three times, the duplicates shuffled among the first proposals; the first pairs join the special junctions of s1_juncs"""
    rng = np.random.default_rng(seed)
    special = [(2, 3), (0, 1), (4, 280), (5, 6), (7, 299), (8, 9), (10, 11), (281, 282), (9, 9)]
    pairs = set()
    out = []
    for p in special[:m2]:
        out.append(p); pairs.add((min(p), max(p)))
    while len(out) < m2:
        x, y = (int(v) for v in rng.integers(0, JN, 2))
        if (min(x, y), max(x, y)) not in pairs:
            pairs.add((min(x, y), max(x, y))); out.append((x, y))
    out = np.array(out, np.int64).reshape(m2, 2)
    reps = rng.integers(2, 4, m2)
    u = np.repeat(np.arange(m2), reps)
    u = u[rng.permutation(len(u))]
    # the kept list opens with the corner proposals of s1_lines (every 97th), so that some pairs' FIRST proposal — the one the aux samples follow — joins map corners
    nc = min(6, len(u))
    where = np.concatenate([np.arange(nc) * 97, np.sort(rng.choice(np.arange(600, NP), len(u) - nc, replace=False))]).astype(np.int64)
    return _indices_from_pairs(rng, where, out[u, 0], out[u, 1])


# case -> (m2, seed) per image (host indices; thin / aux / loi = stage_inputs(b), juncs = s1_juncs(b), lines_pred = s1_lines(b))
STAGE1_CASES = {"m2_0": ((0, 800),), "m2_1": ((1, 801),), "m2_31": ((31, 831),), "m2_32": ((32, 832),), "m2_33": ((33, 833),), "m2_100": ((100, 900),),
                "b2_unequal": ((70, 870), (33, 843))}
STAGE1_WGS = (1, 2)                  # with 1 and 2 workgroups per image: second, third and ragged last tiles, and (m2 <= 32, wgs = 2) a workgroup without any tile
FULL_CASE = "m1_24000"               # at the default grid (512 workgroups, B = 1): a second tile for some workgroups, the dedup's long path in front


@functools.lru_cache(maxsize=None)
def host_case(name: str):
    """a dedup or stage-1 case: dict juncs [B, 300, 2], lines_pred [B, 49152, 4], iskeep / idx_min / idx_max [B, 49152]"""
    if name in DEDUP_CASES:
        imgs = [_dedup_image(kind, seed) for kind, seed in DEDUP_CASES[name]]
    else:
        imgs = [_stage1_image(m2, seed) for m2, seed in STAGE1_CASES[name]]
    B = len(imgs)
    return dict(juncs=np.stack([s1_juncs(b) for b in range(B)]), lines_pred=np.stack([s1_lines(b) for b in range(B)]),
                iskeep=np.stack([i[0] for i in imgs]), idx_min=np.stack([i[1] for i in imgs]), idx_max=np.stack([i[2] for i in imgs]))


def stage_tensors(B: int):
    """thin, aux [B, 4, 128, 128], loi [B, 16384, 128]"""
    t = [stage_inputs(b) for b in range(B)]
    return np.stack([x[0] for x in t]), np.stack([x[1] for x in t]), np.stack([x[2] for x in t])


@functools.lru_cache(maxsize=None)
def host_ref(name: str):
    """per image of a host-index case: dict keep, pairs, rep, la (lines_adjusted float32), li (the first proposals), scores64, proj64, margin, scores32, e32, proj32_err"""
    from oracle import ref_nets
    c = host_case(name)
    out = []
    for b in range(len(c["juncs"])):
        thin, aux, loi = stage_inputs(b)
        keep, pairs, rep = dedup_ref(c["iskeep"][b], c["idx_min"][b], c["idx_max"][b])
        la, sc64, proj64, margin = stage1_f64(c["juncs"][b], c["lines_pred"][b], pairs, keep, rep, loi, thin, aux)
        r = dict(keep=keep, pairs=pairs, rep=rep, la=la, li=c["lines_pred"][b][keep[rep]].reshape(-1, 4), scores64=sc64, proj64=proj64, margin=margin)
        if len(pairs):
            _, inverse, _ = ref_post.wireframe_matcher(c["iskeep"][b], c["idx_min"][b], c["idx_max"][b])
            la32, sc32 = ref_nets.plnet_s1_forward(s1_weights(), c["juncs"][b], c["lines_pred"][b], pairs, inverse, keep,
                                                   np.ascontiguousarray(loi.T).reshape(128, FH, FH), thin, aux)
            assert np.array_equal(la32, la)
            r["scores32"] = sc32
            r["e32"] = float(np.abs(sc32.astype(np.float64) - sc64).max())
        else:
            r["scores32"], r["e32"] = np.zeros(0, F), 0.0
        r["proj32_err"] = float(np.abs(proj_f32(c["juncs"][b], loi).astype(np.float64) - proj64).max())
        out.append(r)
    return out
