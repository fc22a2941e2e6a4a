"""Exact references and hand-built cases for the index work behind the networks: point NMS, candidate compaction, top-K, descriptor sampling, the line filter, the
junction scan and the junction top-300 (tests/test_detector_tail_ref_cpu.py, tests/test_gpu_detector_tail_pin.py).  numpy only, nothing imported from the library or
from oracle/: the rules are comparisons and integer work, so these references are exact, and the CPU test holds them equal to oracle/ref_post.py where that has a
counterpart.  The score maps of real images are smooth soft-max outputs: no exact ties, plateaus, exact zeros, scores equal to the threshold or peaks on a border
line — the inputs the kernels treat specially, which the case builders below put there on purpose.  Every builder returns its inputs and a dict of the properties
it claims; the CPU test checks each claim, so a case cannot silently stop probing what it says it probes."""
import numpy as np

F = np.float32
R = 512
THR = F(0.004)                 # cfg.keypoint_threshold's default as the float the kernels compare with


# ------------------------------------------------------------------ references
def max_pool_brute(x, radius):
    """the (2 radius + 1)^2 maximum around every pixel, -inf outside the map: by definition, over all window offsets"""
    h, w = x.shape
    k = 2 * radius + 1
    p = np.full((h + 2 * radius, w + 2 * radius), -np.inf, x.dtype)
    p[radius:radius + h, radius:radius + w] = x
    out = np.full((h, w), -np.inf, x.dtype)
    for dy in range(k):                                   # every one of the k * k window offsets, none of them combined with another
        for dx in range(k):
            np.maximum(out, p[dy:dy + h, dx:dx + w], out=out)
    return out


def nms_keep(scores, radius):
    """SuperPoint simple_nms' final max_mask (bool): the pixels whose score survives"""
    if radius <= 0:
        return np.ones(scores.shape, bool)
    keep = scores == max_pool_brute(scores, radius)
    for _ in range(2):
        supp = max_pool_brute(keep.astype(scores.dtype), radius) > 0
        ss = np.where(supp, F(0), scores)
        keep = keep | ((ss == max_pool_brute(ss, radius)) & ~supp)
    return keep


def simple_nms(scores, radius):
    return np.where(nms_keep(scores, radius), scores, F(0)).astype(F)


def pack_plane(keep):
    """bool [512, 512] -> the keep plane of kernels.h: word [band][lane], byte r = row 8 band + r, bit j = column 8 lane + j"""
    k = keep.reshape(64, 8, 64, 8).transpose(0, 2, 1, 3).reshape(64, 64, 64).astype(np.uint64)      # [band][lane][8 r + j]
    return (k << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)


def candidates(nms_map, thr, border):
    """raster indices of detect_point's candidates: !(score < thr) inside the border box, upper bound INCLUSIVE"""
    h, w = nms_map.shape
    idx = np.nonzero(~(nms_map.reshape(-1) < F(thr)))[0]
    y, x = idx // w, idx % w
    return idx[~((x < border) | (x > w - border) | (y < border) | (y > h - border))]


def detect_point(nms_map, thr, border, top_k):
    """-> (score, x, y) float32: more than top_k candidates: score descending, raster ascending on ties; else raster order"""
    idx = candidates(nms_map, thr, border)
    s = nms_map.reshape(-1)[idx]
    if idx.size > top_k:
        order = np.lexsort((idx, -s.astype(np.float64)))[:top_k]
        idx, s = idx[order], s[order]
    w = nms_map.shape[1]
    return s.astype(F), (idx % w).astype(F), (idx // w).astype(F)


def select_key(score, idx):
    """the 50-bit candidate key of kernels_sel.hip: valid bit | score bits << 18 | inverted raster index (descending key = the tie rule)"""
    return (1 << 49) | ((int(np.asarray(score, F).view(np.uint32)) & 0x7FFFFFFF) << 18) | (0x3FFFF - int(idx))


def cut_digit(nms_map, thr, border, top_k):
    """the radix digit (0 .. 4: key bits 38-48, 27-37, 16-26, 5-15, 0-4) that holds the first key bit in which rank top_k and rank top_k + 1 differ"""
    idx = candidates(nms_map, thr, border)
    keys = sorted((select_key(nms_map.reshape(-1)[i], i) for i in idx), reverse=True)
    assert len(keys) > top_k
    bit = (keys[top_k - 1] ^ keys[top_k]).bit_length() - 1
    return [d for d, lo in enumerate((38, 27, 16, 5, 0)) if bit >= lo][0]


def _desc_geometry(xs, ys, h, w, dt, s=8):
    sx = dt(F(2.0 / (w * s - s // 2 - 0.5))); bx = dt(F((1 - s) / (w * s - s // 2 - 0.5) - 1))
    sy = dt(F(2.0 / (h * s - s // 2 - 0.5))); by = dt(F((1 - s) / (h * s - s // 2 - 0.5) - 1))
    kx = ((xs.astype(dt) * sx + bx).astype(dt) + dt(1)) * dt(0.5)
    ky = ((ys.astype(dt) * sy + by).astype(dt) + dt(1)) * dt(0.5)
    ix, iy = (kx.astype(dt) * dt(w - 1)).astype(dt), (ky.astype(dt) * dt(h - 1)).astype(dt)
    clip = lambda v, mx: np.clip(v, 0, mx - 1)
    x0, y0 = clip(np.floor(ix).astype(np.int64), w), clip(np.floor(iy).astype(np.int64), h)
    x1, y1 = clip(x0 + 1, w), clip(y0 + 1, h)
    wts = [(x1 - ix) * (y1 - iy), (ix - x0) * (y1 - iy), (x1 - ix) * (iy - y0), (ix - x0) * (iy - y0)]          # nw, ne, sw, se
    return [(y0, x0), (y0, x1), (y1, x0), (y1, x1)], [np.asarray(v, dt) for v in wts]


def desc_cells(x, y, h=64, w=64):
    """the four cells (row, column) a keypoint at pixel (x, y) samples"""
    taps, _ = _desc_geometry(np.array([x], F), np.array([y], F), h, w, F)
    return [(int(t[0][0]), int(t[1][0])) for t in taps]


def extract_descriptors_f64(desc_hwc, xs, ys):
    """extract_descriptors (src/plnet.cpp:369-417) in float64 on the normalised map [h, w, 256] (the grid coefficients stay the reference's floats) -> [N, 256]"""
    h, w, _ = desc_hwc.shape
    taps, wts = _desc_geometry(xs, ys, h, w, np.float64)
    d = desc_hwc.astype(np.float64)
    v = sum(d[t[0], t[1]] * wt[:, None] for t, wt in zip(taps, wts))
    nrm = np.sqrt((v * v).sum(-1, keepdims=True))
    return np.where(nrm > 0, v / np.where(nrm > 0, nrm, 1.0), v)


def line_filter(la, sc, border, line_thr, len_thr, w_scale, h_scale):
    """process_output's line loop (src/plnet.cpp:519-558) + the rescale (:577-582), with the index guard line_filter_kernel has: an endpoint outside the 512 x 512 map
    marks nothing (the C++ writes out of bounds there).  la [m2, 4] in 128-space, sc [m2] -> (lines float64 [L, 4] in image pixels, junction map uint8 [512, 512])."""
    jmap = np.zeros((R, R), np.uint8)
    border = max(border, 0)
    thr2 = F(F(len_thr) * F(len_thr))
    ws, hs = float(F(w_scale)), float(F(h_scale))
    out = []
    for i in range(len(sc)):
        if sc[i] < F(0.5):
            continue
        p = (la[i].astype(F) * F(4)).astype(F)
        q = [int(np.float64(v) + 0.1) for v in p]
        for xi, yi in ((q[0], q[1]), (q[2], q[3])):
            if 0 <= xi < R and 0 <= yi < R:
                jmap[yi, xi] = border < xi < R - border and border < yi < R - border
        if sc[i] < F(line_thr):
            continue
        dx, dy = F(p[2] - p[0]), F(p[3] - p[1])
        if F(F(dx * dx) + F(dy * dy)) < thr2:
            continue
        out.append((float(p[0]) * ws, float(p[1]) * hs, float(p[2]) * ws, float(p[3]) * hs))
    return np.array(out, np.float64).reshape(-1, 4), jmap


def junction_detector(jmap, score_map, border):
    """junction_detector's scan (src/plnet.cpp:425-448): raster order over [border, 512 - border) — upper bound EXCLUSIVE — -> rows (score, x, y), unscaled"""
    border = max(border, 0)
    m = np.zeros_like(jmap)
    m[border:R - border, border:R - border] = jmap[border:R - border, border:R - border]
    ys, xs = np.nonzero(m)
    return np.stack([score_map[ys, xs].astype(F), xs.astype(F), ys.astype(F)], 1).reshape(-1, 3)


# ------------------------------------------------------------------ score-map cases
def _blank():
    return np.zeros((R, R), F)


def _survivors(heat, radius=4):
    """positive pixels that survive simple_nms, as a set of (y, x)"""
    ys, xs = np.nonzero(nms_keep(heat, radius) & (heat > 0))
    return set(zip(ys.tolist(), xs.tolist()))


def block_census(keep):
    """survivors per lane block (the 8 x 8 block one lane of nms512_kernel owns) [64, 64]"""
    return keep.reshape(64, 8, 64, 8).sum((1, 3))


def nms_spacing():
    """pairs of peaks 4 px apart (the lower one dies) and 5 px apart (both live), horizontal / vertical / diagonal, across a lane boundary (column 159 | 160), across a
    band boundary (row 255 | 256), inside lane 0 and lane 63, inside band 0 and band 63; equal peaks 3 px apart (both live); the four corner pixels"""
    h = _blank()
    live, dead = set(), set()
    dirs = {"h": (0, 1), "v": (1, 0), "d": (1, 1)}
    k = 0
    for site in ("lane_edge", "lane0", "lane63", "band_edge", "band0", "band63"):
        for dn, (dy, dx) in dirs.items():
            for dist in (4, 5):
                t = 40 + 24 * (k % 6)                                   # the free coordinate: pairs of one site 24 px apart
                k += 1
                if site == "lane_edge":
                    y0, x0 = t, (160 - 3 if dx else 160)               # x0 .. x0 + dist crosses 159 | 160 (a vertical pair stands in column 160)
                elif site == "lane0":
                    y0, x0 = t, 1
                elif site == "lane63":
                    y0, x0 = t, 505
                elif site == "band_edge":
                    y0, x0 = (256 - 3 if dy else 256), t
                elif site == "band0":
                    y0, x0 = 1, t
                else:
                    y0, x0 = 505, t
                y1, x1 = y0 + dist * dy, x0 + dist * dx
                h[y0, x0], h[y1, x1] = F(0.625), F(0.5)
                live.add((y0, x0))
                (dead if dist == 4 else live).add((y1, x1))
    h[300, 300] = h[300, 303] = F(0.375)
    live |= {(300, 300), (300, 303)}
    for c in ((0, 0), (0, 511), (511, 0), (511, 511)):
        h[c] = F(0.75)
        live.add(c)
    return dict(name="nms_spacing", maps=[h], claims=dict(live=live, dead=dead))


def nms_chains():
    """seven peaks of strictly decreasing score 3 px and 4 px apart, in a row across a lane boundary and in a column across a band boundary: peaks 1, 3, 5 live, peak 7
    does not (it would take a third suppression round; the reference has two)"""
    h = _blank()
    live, dead = set(), set()
    sc = [F(0.875 - 0.0625 * i) for i in range(7)]
    for step, off in ((3, 0), (4, 60)):
        for i in range(7):
            row, col = (100 + off, 160 - 3 * step + 1 + step * i), (256 - 3 * step + 1 + step * i, 300 + off)      # peak 4 just across column 159 | 160, row 255 | 256
            for p in (row, col):
                h[p] = sc[i]
                (live if i in (0, 2, 4) else dead).add(p)
    return dict(name="nms_chains", maps=[h], claims=dict(live=live, dead=dead))


def nms_plateaus():
    """an 8 x 8 block of one value aligned to a lane's block (64 survivors, 16 rounds in one lane), the same shifted by (4, 4) (four lanes, two bands), a 3 x 20 bar;
    the background is exact zero, which survives wherever no positive pixel lies within 4 px (full 16 rounds in those lanes)"""
    h = _blank()
    h[80:88, 160:168] = F(0.5)
    h[204:212, 300:308] = F(0.5)
    h[400:403, 100:120] = F(0.25)
    return dict(name="nms_plateaus", maps=[h], claims=dict(positive_survivors=64 + 64 + 60, full_blocks=1, zero_blocks_full=True))


def nms_few_values():
    """16 score levels drawn uniformly: thousands of exact ties, up to 12 survivors in one lane block (three rounds and more), the top-K cut decided by the raster index"""
    maps = [(np.random.default_rng(s).integers(0, 16, (R, R)) / 32).astype(F) for s in (0, 1, 2)]
    return dict(name="nms_few_values", maps=maps, claims=dict(positive_survivors_seed0=16664, max_per_block_seed0=12))


def threshold_and_border(border):
    """isolated peaks with score exactly thr (kept), one ulp below (dropped) and above; peaks at x or y = border - 1 (dropped), border, 512 - border (kept: inclusive),
    512 - border + 1 (dropped), 0 and 511"""
    h = _blank()
    below, above = np.nextafter(THR, F(0)), np.nextafter(THR, F(1))
    h[100, 100], h[100, 120], h[100, 140] = THR, below, above
    kept, dropped = {(100, 100), (100, 140)}, {(100, 120)}
    edge = sorted({v for v in (border - 1, border, R - border, R - border + 1, 0, R - 1) if 0 <= v < R})
    for i, v in enumerate(edge):
        for p in ((200 + 12 * i, v), (v, 200 + 12 * i)):
            h[p] = F(0.5)
            (kept if border <= v <= R - border else dropped).add(p)
    return dict(name=f"threshold_and_border_{border}", maps=[h], claims=dict(kept=kept, dropped=dropped, border=border))


def _lattice(n, rng=None, pitch=10, first=10):
    """n distinct sites on a lattice of isolated positions (>= 9 px apart, inside the border box), in raster order or shuffled"""
    per = (R - 2 * first) // pitch + 1
    idx = np.arange(per * per) if rng is None else rng.permutation(per * per)
    return [(first + pitch * int(i // per), first + pitch * int(i % per)) for i in idx[:n]]


def _bits(u):
    return np.array([u], np.uint32).view(F)[0]


def topk_cut(K=37):
    """isolated peaks around the top-K cut of max_keypoints = K; claims: candidate count, and where one is named the radix digit that decides the cut"""
    rng = np.random.default_rng(7)
    maps, claims = [], []

    def case(peaks, **cl):
        h = _blank()
        for p, v in peaks:
            h[p] = v
        maps.append(h)
        claims.append(dict(count=len(peaks), **cl))

    distinct = lambda n, base=0.25: (F(base) + rng.permutation(n).astype(F) / F(1024)).astype(F)      # n distinct scores in an order unrelated to the raster
    case([])                                                                                    # count 0
    case(list(zip(_lattice(K), distinct(K))), raster_differs=True)                              # count K: raster order, not score order
    case(list(zip(_lattice(K + 1, rng), distinct(K + 1))))                                      # count K + 1
    case([(p, F(0.5)) for p in _lattice(3 * K, rng)])                                           # 3K peaks of one score
    case(list(zip(_lattice(K + 15, rng), np.concatenate([distinct(K - 5, 0.5), np.full(20, F(0.375), F)]))), tied_at_cut=20)
    case([(p, _bits(0x3E800000 + int(rng.integers(0, 2)))) for p in _lattice(2 * K, rng)], digit=None, mantissa_bit0=True)
    # one sub-case per radix digit: K - 1 higher peaks, the two contenders of rank K and K + 1, ten lower peaks
    contenders = {0: ((F(0.5), (250, 250)), (F(0.25), (250, 270))),
                  1: ((_bits(0x3F000000 | 1 << 12), (250, 250)), (F(0.5), (250, 270))),
                  2: ((_bits(0x3F000000 | 1 << 3), (250, 250)), (F(0.5), (250, 270))),
                  3: ((F(0.5), (260, 250)), (F(0.5), (270, 250))),                              # one score, rows 260 and 270: the raster indices differ from bit 12 down
                  4: ((F(0.5), (250, 265)), (F(0.5), (250, 274)))}                              # one score, one row, columns inside one aligned run of 32
    for d, (a, b) in contenders.items():
        others = [p for p in _lattice(K + 40, rng) if abs(p[0] - 260) > 30][:K + 9]
        hi, lo = list(zip(others[:K - 1], distinct(K - 1, 0.75))), list(zip(others[K - 1:], distinct(10, 0.125)))
        case(hi + [(a[1], a[0]), (b[1], b[0])] + lo, digit=d)
    # the early exit with more than one key in the bucket: exactly K keys share the top digit
    sites = _lattice(K + 12, rng)
    case([(p, F(0.5) + F(i) / F(4096)) for i, p in enumerate(sites[:K])] + [(p, F(0.0625)) for p in sites[K:]], digit=0, early_exit=True)
    return dict(name="topk_cut", maps=maps, claims=claims)


def topk_1024():
    """more than 1024 candidates with max_keypoints = 1024: 1500 isolated peaks on 8 score levels"""
    rng = np.random.default_rng(11)
    h = _blank()
    for p in _lattice(1500, rng):
        h[p] = F(0.25) + F(rng.integers(0, 8)) / F(64)
    return dict(name="topk_1024", maps=[h], claims=dict(count=1500))


def descriptors():
    """isolated peaks at random pixels (every sub-cell position of the 8-px descriptor grid), among them the outermost cells"""
    rng = np.random.default_rng(3)
    h = _blank()
    sites = _lattice(300, rng, pitch=9, first=4)
    for y, x in sites:
        h[min(y + int(rng.integers(0, 5)), R - 1), min(x + int(rng.integers(0, 5)), R - 1)] = F(0.1) + F(rng.integers(0, 4096)) / F(8192)
    return dict(name="descriptors", maps=[h], claims=dict(min_keypoints=250))


ACT_SCALE = 0.9      # convDa's output on the synthetic detector: the fp32 oracle (oracle/ref_nets.superpoint_heads, weights.synthetic_superpoint(1234), synth.gabor_image(480, 752, 0))
#                      gives post-ReLU activations with half the entries zero, rms 0.64 and maximum 4.2 — a rectified normal of standard deviation 0.9


def activations(i):
    """convDa-like activations [64, 64, 256] of image slot i"""
    return np.maximum(np.random.default_rng(100 + i).normal(0.0, ACT_SCALE, (64, 64, 256)), 0).astype(F)


def zero_descriptor():
    """one keypoint whose four cells hold zero activations (with convDb's bias zero: an all-zero descriptor, not NaN) beside ordinary ones"""
    h = _blank()
    pts = [(100, 100), (100, 200), (300, 133)]
    for i, p in enumerate(pts):
        h[p] = F(0.5) - F(i) / F(16)
    act = activations(0)
    for cy, cx in desc_cells(100, 100):
        act[cy, cx] = 0
    return dict(name="zero_descriptor", maps=[h], act=act, claims=dict(zero_keypoint=(100, 100)))


# ------------------------------------------------------------------ line / junction cases
LINE_THR, LEN_THR = F(0.75), F(50.0)


def _one_ulp_short():
    """an endpoint y2 (128-space) with fl(48^2 + (4 y2 - 40)^2) == 2500 - 1 ulp: the length test's threshold missed by the smallest amount"""
    want = np.nextafter(F(2500), F(0))
    y2 = F(13.5)
    for _ in range(64):
        y2 = np.nextafter(y2, F(0))
        dy = F(F(y2 * F(4)) - F(40))
        if F(F(F(48) * F(48)) + F(dy * dy)) == want:
            return y2
    raise AssertionError("no endpoint gives the squared length one ulp below the threshold")


def line_post(border, m2s=(0, 1, 1023, 1024), seed=5):
    """per image: the special lines first (scores 0.5 / one ulp below / line_thr / one ulp below; squared length exactly thr^2 and one ulp below; endpoints whose pixel lands
    on border, border + 1, R - border - 1, R - border, 0 and 512; two lines sharing an endpoint pixel; endpoints on the first / last pixels of scan spans and scan threads;
    endpoints on the peaks of nms_spacing, live and suppressed), then random lines up to m2.  -> la [B, ld, 4], sc [B, ld], m2 [B], heat [B, 512, 512]"""
    nxt = lambda v: np.nextafter(F(v), F(0))
    sp = nms_spacing()
    heat = sp["maps"][0]
    spec = []
    for s in (F(0.5), nxt(0.5), LINE_THR, nxt(LINE_THR), F(0.9)):                             # score thresholds, long lines
        spec.append((20.0, 20.0 + len(spec), 90.0, 25.0 + len(spec), s))
    spec.append((10.0, 10.0, 22.0, 13.5, F(0.9)))                                              # dx = 48, dy = 14 in 512-space: l2 = 2500 exactly (kept)
    spec.append((10.0, 10.0, 22.0, float(_one_ulp_short()), F(0.9)))                           # l2 one ulp below (dropped)
    for v in (border / 4, (border + 1) / 4, (R - border - 1) / 4, (R - border) / 4, 0.0, 128.0):      # endpoint pixels on and beside the border lines, 0 and 512
        spec.append((v, 30.0, 60.0, v, F(0.6)))
    spec.append((50.0, 50.0, 100.0, 100.0, F(0.9)))
    spec.append((50.0, 50.0, 50.25, 110.0, F(0.9)))                                            # shares the pixel (200, 200); its other end is one pixel from nothing
    for s in (0, 1, 31, 63):                                                                   # scan spans: pixels [4096 s, 4096 (s + 1)) = rows 8 s .. 8 s + 7
        spec.append((0.25, 2.0 * s, 127.75, 2.0 * s + 1.75, F(0.6)))                           # (x = 1, first row of the span) .. (x = 511, last row): the last pixel of the span
        spec.append((3.75, 2.0 * s, 4.0, 2.0 * s + 1.75, F(0.6)))                              # x = 15 | 16: the last pixel of one scan thread, the first of the next
    for (y, x) in sorted(sp["claims"]["dead"]) + sorted(sp["claims"]["live"]):                 # junctions on NMS peaks: suppressed ones score 0, live ones their score
        spec.append((x / 4, y / 4, 64.0, 64.0, F(0.6)))
    spec = np.array(spec, F)
    rng = np.random.default_rng(seed)
    ld = max(max(m2s), 1)
    la, sc = np.zeros((len(m2s), ld, 4), F), np.zeros((len(m2s), ld), F)
    for b, m2 in enumerate(m2s):
        rl = np.concatenate([(rng.integers(0, 513, (ld, 4)) / 4).astype(F), rng.choice([0.3, 0.5, 0.6, 0.75, 0.9], (ld, 1)).astype(F)], 1)
        rows = np.concatenate([spec, rl])[:ld] if m2 >= len(spec) else rl
        la[b], sc[b] = rows[:, :4], rows[:, 4]
    return dict(name=f"line_post_{border}", la=la, sc=sc, m2=np.array(m2s, np.int32), heat=np.stack([heat] * len(m2s)), n_special=len(spec), claims=dict(border=border))


def scan_maps(border, seed=13):
    """junction maps [2, 512, 512] for the scan alone: 1 % random pixels plus, in the first, the complete rows and columns border - 1, border, 512 - border - 1, 512 - border,
    0 and 511 — pixels the line filter never marks: the scan's own bounds (lower inclusive, upper EXCLUSIVE), and the first and last pixel of every one of its 64 spans;
    in both, the peaks of nms_spacing's score map"""
    rng = np.random.default_rng(seed)
    m = (rng.random((2, R, R)) < 0.01).astype(np.uint8)
    for v in {max(border - 1, 0), border, R - border - 1, min(R - border, R - 1), 0, R - 1}:
        m[0, v, :] = 1
        m[0, :, v] = 3                                       # any non-zero byte counts
    cl = nms_spacing()["claims"]
    for y, x in cl["live"] | cl["dead"]:                      # junctions on the peaks of nms_spacing's map: their score, or 0 where the NMS suppressed them
        m[:, y, x] = 1
    return m


# ------------------------------------------------------------------ junction top-300 cases
def junctions_topk_cases():
    """jloc / joff maps [n, 128, 128] / [n, 2, 128, 128] with the claimed number of positive 3x3 maxima each"""
    rng = np.random.default_rng(9)
    jl, counts = [], []
    sites = [(2 + 3 * int(i // 42), 2 + 3 * int(i % 42)) for i in rng.permutation(42 * 42)]      # isolated: 3 px apart
    a = np.zeros((128, 128), F)                       # more than 300 isolated maxima, distinct scores
    for k, p in enumerate(sites[:500]):
        a[p] = F(0.1) + F(k) / F(1024)
    jl.append(a); counts.append(500)
    jl.append(np.full((128, 128), F(0.25), F)); counts.append(128 * 128)      # flat: all tied, the first 300 in raster order
    a = np.zeros((128, 128), F)                       # a plateau straddling the cut: 290 higher maxima, then a 6 x 6 block of one value
    for k, p in enumerate([s for s in sites if s[0] > 12 or s[1] > 12][:290]):
        a[p] = F(0.5) + F(k) / F(1024)
    a[2:8, 2:8] = F(0.25)
    jl.append(a); counts.append(290 + 36)
    a = np.zeros((128, 128), F)                       # 40 isolated maxima, distinct scores, raster order != score order
    for k, p in enumerate(sites[:40]):
        a[p] = F(0.1) + F(k) / F(1024)
    jl.append(a); counts.append(40)
    jloc = np.stack(jl)
    joff = rng.choice(np.array([-0.5, 0.5, 0.25, -0.4999999, 0.3333333, 1e-8], F), (len(jl), 2, 128, 128)).astype(F)      # +-0.5, and sums with the pixel coordinate that round
    return dict(name="junctions_topk", jloc=jloc, joff=joff, claims=dict(counts=counts))


DETECTOR_CASES = {"nms_spacing": nms_spacing, "nms_chains": nms_chains, "nms_plateaus": nms_plateaus, "nms_few_values": nms_few_values,
                  "threshold_and_border_4": lambda: threshold_and_border(4), "threshold_and_border_0": lambda: threshold_and_border(0), "topk_cut": topk_cut,
                  "topk_1024": topk_1024, "descriptors": descriptors, "zero_descriptor": zero_descriptor}
NMS_CASES = ("nms_spacing", "nms_chains", "nms_plateaus", "nms_few_values")
# the detector settings a case runs with (everything else: the library's defaults — threshold 0.004, remove_borders 4, max_keypoints 400, nms_radius 4)
CASE_CFG = {"threshold_and_border_0": dict(remove_borders=0), "topk_cut": dict(max_keypoints=37), "topk_1024": dict(max_keypoints=1024)}
_CASES = {}


def case(name):
    """a built case, built once and shared (treat as read-only)"""
    if name not in _CASES:
        _CASES[name] = DETECTOR_CASES[name]()
    return _CASES[name]


_REF = {}


def detector_ref(name, i, radius=4):
    """the exact result for map i of a case at its settings: dict keep (bool), nms (float32), cand_cnt, score / x / y (unscaled), built once and shared"""
    key = (name, i, radius)
    if key not in _REF:
        cfg = dict(dict(remove_borders=4, max_keypoints=400), **CASE_CFG.get(name, {}))
        heat = case(name)["maps"][i]
        keep = nms_keep(heat, radius)
        nms = np.where(keep, heat, F(0)).astype(F)
        s, x, y = detect_point(nms, THR, cfg["remove_borders"], cfg["max_keypoints"])
        _REF[key] = dict(keep=keep, nms=nms, cand_cnt=int(candidates(nms, THR, cfg["remove_borders"]).size), score=s, x=x, y=y, cfg=cfg)
    return _REF[key]
