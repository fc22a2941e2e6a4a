"""The references and cases of tests/detector_tail_ref.py, checked without a GPU: the brute-force restatements equal oracle/ref_post.py (written separately, the NMS
separable there and by definition here), and every property a case builder claims holds — so a case cannot silently stop probing what it says it probes."""
import numpy as np
import pytest

import detector_tail_ref as R
from oracle import ref_nets, ref_post

F = np.float32
MAPS = [(name, i) for name in R.DETECTOR_CASES for i in range(len(R.case(name)["maps"]))]


@pytest.mark.parametrize("name,i", MAPS, ids=[f"{n}-{i}" for n, i in MAPS])
def test_references_equal_the_oracle(name, i):
    heat = R.case(name)["maps"][i]
    assert heat.dtype == F and np.isfinite(heat).all() and heat.min() >= 0 and heat.max() <= 1
    ref = R.detector_ref(name, i)
    cfg = ref["cfg"]
    np.testing.assert_array_equal(ref["nms"], ref_post.simple_nms(heat, 4))
    s, x, y = ref_post.detect_point(ref["nms"], R.THR, cfg["remove_borders"], cfg["max_keypoints"])
    for got, want in ((ref["score"], s), (ref["x"], x), (ref["y"], y)):
        np.testing.assert_array_equal(got, want)
    assert ref["cand_cnt"] >= len(s) == min(ref["cand_cnt"], cfg["max_keypoints"])
    if name in R.NMS_CASES:
        np.testing.assert_array_equal(R.simple_nms(heat, 2), ref_post.simple_nms(heat, 2))


def test_keep_plane_layout():
    keep = np.zeros((512, 512), bool)
    keep[8 * 5 + 3, 8 * 9 + 6] = keep[0, 0] = keep[511, 511] = True
    plane = R.pack_plane(keep)
    assert plane[5, 9] == np.uint64(1) << np.uint64(8 * 3 + 6) and plane[0, 0] == 1 and plane[63, 63] == np.uint64(1) << np.uint64(63)
    assert np.count_nonzero(plane) == 3


def test_nms_spacing_and_chain_claims():
    for name in ("nms_spacing", "nms_chains"):
        c = R.case(name)
        heat, cl = c["maps"][0], c["claims"]
        assert R._survivors(heat) == cl["live"] and not (cl["live"] & cl["dead"])
        assert all(heat[p] > 0 for p in cl["dead"]) and len(cl["dead"]) >= 16
    sp = R.case("nms_spacing")["claims"]
    cols, rows = {x for _, x in sp["live"] | sp["dead"]}, {y for y, _ in sp["live"] | sp["dead"]}
    assert {159 - 2, 161} <= cols and {256 - 3, 257} <= rows                    # a pair across column 159 | 160 and one across row 255 | 256
    assert min(cols) < 8 and max(cols) >= 504 and min(rows) < 8 and max(rows) >= 504      # lane 0 / 63, band 0 / 63
    ch = R.case("nms_chains")
    for p in ch["claims"]["dead"]:                                               # the seventh peaks are isolated from every LIVE peak: only the missing third round kills them
        if ch["maps"][0][p] == F(0.875 - 0.0625 * 6):
            assert min(max(abs(p[0] - q[0]), abs(p[1] - q[1])) for q in ch["claims"]["live"]) > 4


def test_plateau_and_tie_claims():
    c = R.case("nms_plateaus")
    heat, keep = c["maps"][0], R.detector_ref("nms_plateaus", 0)["keep"]
    pos = R.block_census(keep & (heat > 0))
    assert int(pos.sum()) == c["claims"]["positive_survivors"] and int((pos == 64).sum()) == 1 and int((pos == 16).sum()) == 4
    assert R.block_census(keep)[0, 0] == 64 and (R.block_census(keep) == 64).sum() > 3000           # exact-zero background: all 64 pixels of a lane block survive
    assert not keep[76:80, 160:168].any()                                                           # ... but not within 4 px of a positive pixel
    c = R.case("nms_few_values")
    r0 = R.detector_ref("nms_few_values", 0)
    pos = R.block_census(r0["keep"] & (c["maps"][0] > 0))
    assert int(pos.sum()) == c["claims"]["positive_survivors_seed0"] and int(pos.max()) == c["claims"]["max_per_block_seed0"] > 8
    assert len(np.unique(r0["score"])) == 1 and r0["cand_cnt"] > 10000                              # the top-400 cut falls inside one score level: the raster index decides


@pytest.mark.parametrize("border", [4, 0])
def test_threshold_and_border_claims(border):
    name = f"threshold_and_border_{border}"
    cl, ref = R.case(name)["claims"], R.detector_ref(name, 0)
    got = set(zip(ref["y"].astype(int).tolist(), ref["x"].astype(int).tolist()))
    assert got == cl["kept"] and not (got & cl["dropped"]) and ref["cfg"]["remove_borders"] == border
    assert R.THR in ref["score"] and np.nextafter(R.THR, F(0)) not in ref["score"]
    if border == 0:
        assert {0, 511} <= set(ref["x"].astype(int).tolist()) and {0, 511} <= set(ref["y"].astype(int).tolist())      # keypoints whose descriptor taps clip


def test_topk_cut_claims():
    c = R.case("topk_cut")
    K = 37
    digits = set()
    for i, cl in enumerate(c["claims"]):
        ref = R.detector_ref("topk_cut", i)
        assert ref["cand_cnt"] == cl["count"] and ref["cfg"]["max_keypoints"] == K
        if cl.get("raster_differs"):
            assert cl["count"] == K and (np.diff(ref["score"]) > 0).any() and (np.diff(ref["y"] * 512 + ref["x"]) > 0).all()
        if cl.get("tied_at_cut"):
            assert 0 < int((ref["score"] == ref["score"][-1]).sum()) < cl["tied_at_cut"]
        if cl.get("mantissa_bit0"):
            assert len(set(ref["nms"][ref["nms"] > 0].view(np.uint32).tolist())) == 2 and np.ptp(ref["nms"][ref["nms"] > 0].view(np.uint32)) == 1
        if cl.get("digit") is not None:
            assert R.cut_digit(ref["nms"], R.THR, 4, K) == cl["digit"]
            digits.add(cl["digit"])
        if cl.get("early_exit"):
            top = {R.select_key(s, 0) >> 38 for s in ref["score"]}
            assert len(top) == 1 and int((ref["nms"] >= ref["score"].min()).sum()) == K                  # K keys in the cut's bucket, every one selected
    assert digits == {0, 1, 2, 3, 4}
    counts = [cl["count"] for cl in c["claims"]]
    assert 0 in counts and K in counts and K + 1 in counts and 3 * K in counts
    assert R.detector_ref("topk_1024", 0)["cand_cnt"] == 1500 and len(R.detector_ref("topk_1024", 0)["score"]) == 1024


def test_descriptor_case_claims():
    ref = R.detector_ref("descriptors", 0)
    assert len(ref["score"]) >= R.case("descriptors")["claims"]["min_keypoints"]
    assert len({(int(x) % 8, int(y) % 8) for x, y in zip(ref["x"], ref["y"])}) >= 60               # the sub-cell positions of the descriptor grid
    z = R.case("zero_descriptor")
    y, x = z["claims"]["zero_keypoint"]
    cells = R.desc_cells(x, y)
    assert len(set(cells)) == 4 and all((z["act"][c] == 0).all() for c in cells) and (z["act"] != 0).any()
    a = R.activations(0)
    assert 0.55 < np.sqrt((a * a).mean()) < 0.72 and 0.45 < (a > 0).mean() < 0.55                   # the magnitude ACT_SCALE is documented with


def test_descriptor_restatements_agree():
    rng = np.random.default_rng(0)
    d = rng.normal(size=(64, 64, 256)).astype(F)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    xs, ys = rng.integers(0, 512, 200).astype(F), rng.integers(0, 512, 200).astype(F)
    xs[:4], ys[:4] = [0, 511, 0, 511], [0, 0, 511, 511]
    a = ref_post.extract_descriptors(np.ascontiguousarray(d.transpose(2, 0, 1)), xs, ys)
    b = R.extract_descriptors_f64(d, xs, ys)
    # At coordinate 511 the grid coordinate is 63 to within rounding and all four taps clip to one row / column: the weights cancel.  In float32 they are exactly zero
    # (a zero descriptor, kept zero by the normalisation rule); in float64 they are +-1e-6 and the normalisation blows the difference up.  No number to compare there.
    edge = (xs == 511) | (ys == 511)
    assert edge.sum() >= 3 and (a[edge] == 0).all()
    assert np.abs(a - b)[~edge].max() < 2e-6


@pytest.mark.parametrize("border", [4, 0])
def test_line_filter_and_junction_detector_equal_the_oracle(border):
    lp = R.line_post(border)
    ws, hs = F(752 / 512), F(480 / 512)
    n_marked = []
    for b, m2 in enumerate(lp["m2"]):
        la, sc = lp["la"][b, :m2], lp["sc"][b, :m2]
        lines, jmap = R.line_filter(la, sc, border, R.LINE_THR, R.LEN_THR, ws, hs)
        inside = ((la * 4 + 0.1).astype(int) < 512).all(1) | (sc < 0.5)          # the C++ (and its restatement) index out of bounds at pixel 512
        ol, oj = ref_post.line_filter(la[inside], sc[inside], border, R.LINE_THR, R.LEN_THR)
        gl, gj = R.line_filter(la[inside], sc[inside], border, R.LINE_THR, R.LEN_THR, ws, hs)
        np.testing.assert_array_equal(gl, ref_post.rescale_lines(ol, ws, hs))
        np.testing.assert_array_equal(gj.astype(bool), oj)
        nms = R.simple_nms(lp["heat"][b], 4) if b == 0 else nms
        got = R.junction_detector(gj, nms, border)
        want = ref_post.junction_detector(nms, np.zeros((256, 64, 64), F), oj, border)
        np.testing.assert_array_equal(got, want[:, :3])
        n_marked.append(int(jmap.sum()))
        if m2 >= lp["n_special"]:
            assert (~inside).sum() >= 1 and len(lines) > 100
            j = R.junction_detector(jmap, nms, border)
            assert (j[:, 0] == 0).any() and (j[:, 0] > 0).any()                   # junctions on suppressed and on live peaks
            xs, ys = set(j[:, 1].astype(int).tolist()), set(j[:, 2].astype(int).tolist())
            assert (border + 1 in xs) and (512 - border - 1 in xs) and border not in xs and 512 - border not in xs
            if border == 0:
                assert {(511., 8. * s + 7) for s in (0, 1, 31, 63)} <= {(r[1], r[2]) for r in j.tolist()}      # the last pixel of scan spans 0, 1, 31, 63
    assert n_marked[0] == 0 and n_marked[-1] > 500


@pytest.mark.parametrize("border", [4, 0])
def test_scan_maps_probe_the_scan_bounds(border):
    m = R.scan_maps(border)
    nms = R.simple_nms(R.case("nms_spacing")["maps"][0], 4)
    for b in range(2):
        got = R.junction_detector(m[b], nms, border)
        want = ref_post.junction_detector(nms, np.zeros((256, 64, 64), F), m[b].astype(bool), border)
        np.testing.assert_array_equal(got, want[:, :3])
    j = R.junction_detector(m[0], nms, border)
    xs, ys = set(j[:, 1].astype(int).tolist()), set(j[:, 2].astype(int).tolist())
    assert min(xs) == min(ys) == border and max(xs) == max(ys) == 512 - border - 1 and m[0, 512 - border - 1 + (border > 0), :].all()
    assert len(j) > 4000 and (j[:, 0] > 0).any()
    if border == 0:                                           # the first and the last pixel of every scan span (rows 8 s .. 8 s + 7) are junctions
        px = set((j[:, 2] * 512 + j[:, 1]).astype(int).tolist())
        assert all(4096 * s in px and 4096 * s + 4095 in px for s in range(64))


def test_line_length_threshold_cases():
    y2 = R._one_ulp_short()
    la = np.array([[10, 10, 22, 13.5], [10, 10, 22, y2]], F)
    lines, _ = R.line_filter(la, np.array([0.9, 0.9], F), 4, R.LINE_THR, R.LEN_THR, 1, 1)
    assert len(lines) == 1 and lines[0, 3] == 54.0


def test_junction_topk_claims():
    c = R.junctions_topk_cases()
    for b, n in enumerate(c["claims"]["counts"]):
        a = c["jloc"][b]
        p = np.pad(a, 1, constant_values=-np.inf)
        mx = np.max([p[dy:dy + 128, dx:dx + 128] for dy in range(3) for dx in range(3)], 0)
        assert int(((a == mx) & (a > 0)).sum()) == n
    assert sorted(c["claims"]["counts"])[0] < 300 < sorted(c["claims"]["counts"])[1]
    j = ref_nets.junctions_topk(c["jloc"][3], c["joff"][3])
    assert (j[40:] == 0).all() and (j[:40] != 0).any(1).all()
    ys, xs = np.nonzero(c["jloc"][3])                                              # raster order
    assert (np.diff(c["jloc"][3][ys, xs]) > 0).any()                               # ... is not score order
