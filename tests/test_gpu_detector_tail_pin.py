"""The index work behind the networks — point NMS, candidate compaction, top-K, descriptor sampling, the line filter, the junction scan and the junction top-300 —
on hand-built maps (tests/detector_tail_ref.py): exact ties, plateaus, exact zeros, scores equal to the threshold, peaks on the border lines, cuts decided in every
digit of the radix select.  The hooks stage the maps into the context's own buffers and run the launchers production runs (include/airfe_debug.h).  Scores,
positions, counts, keep planes, lines and junction rows are integer and comparison work: the gate is equality with the exact reference, whole buffers, sentinel
rows included.  Every form of the detector tail must also give the bytes of the one-image form, descriptors included."""
import os

import numpy as np
import pytest

import detector_tail_ref as R
from airslam_amd import api, weights
from conftest import GOLDEN
from gpu_common import diag
from oracle import ref_nets, ref_post

pytestmark = pytest.mark.gpu
F = np.float32
SENTINEL = 7.0
H, W = 480, 752                                   # the image size keypoints and lines are scaled to
WS, HS = F(W) / F(512), F(H) / F(512)
FUSED = {"gemmr_min_m": 256}                      # the streaming gather GEMM with the sampling in it from 256 rows on (default at these sizes: the tiled kernel + sample_desc)
# form -> (B, Bs, tuning): one image (dense NMS'd map, dense descriptor head, sample_desc(compact = 0)); three images (no dense map, gather head); the same with the
# sampling inside the streaming gather GEMM; four images to two destinations as a stereo call
FORMS = {"b1": (1, 0, None), "b3": (3, 0, None), "b3_fused": (3, 0, FUSED), "b4_stereo": (4, 2, None)}
_CTX, _RUNS, _F64 = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for c in _CTX.values():
        c.close()
    _CTX.clear()
    _RUNS.clear()


def _ctx(kind="sp", tuning=None, **cfg):
    key = (kind, tuple(sorted((tuning or {}).items())), tuple(sorted(cfg.items())))
    if key not in _CTX:
        kw = dict(max_batch=4, enc_chunk=4, check_launches=1, tuning=tuning, **cfg)
        if kind == "pl":
            _CTX[key] = api.Context(superpoint=weights.synthetic_plnet_s0(1234), plnet_s1=os.path.join(GOLDEN, "plnet_s1.airfe"), **kw)
        else:
            sp = dict(weights.synthetic_superpoint(1234))
            if kind == "sp_zero_bias":
                sp["convDb.bias"] = np.zeros_like(sp["convDb.bias"])
            _CTX[key] = api.Context(superpoint=sp, **kw)
    return _CTX[key]


def _run(name, form, radius=4):
    """every map of a case through one form -> per map: dict feat [cap, 259], n, cand_cnt, keep, nms_map, desc (the device's dense normalised head map of that image)"""
    key = (name, form, radius)
    if key in _RUNS:
        return _RUNS[key]
    case = R.case(name)
    B, Bs, tuning = FORMS[form]
    cfg = dict(R.CASE_CFG.get(name, {}))
    if radius != 4:
        cfg["nms_radius"] = radius
    ctx = _ctx("sp_zero_bias" if name == "zero_descriptor" else "sp", tuning, **cfg)
    K = ctx.max_keypoints
    cap = min(K + 4, 1024)                         # rows K .. cap - 1 are never filled
    maps = case["maps"]
    act = lambda i: case["act"] if "act" in case else R.activations(i % 4)
    out = {}
    for g in range((len(maps) + B - 1) // B):
        ids = [(g * B + j) % len(maps) for j in range(B)]
        r = ctx.debug_detector_tail(np.stack([maps[i] for i in ids]), np.stack([act(i) for i in ids]), cap, Bs=Bs, h=H, w=W, sentinel=SENTINEL)
        _, _, desc = ctx.detector_maps(B)
        for j, i in enumerate(ids):
            slot = dict(feat=r["feat"][j], n=int(r["n"][j]), cand_cnt=int(r["cand_cnt"][j]), keep=None if r["keep"] is None else r["keep"][j],
                        nms_map=None if r["nms_map"] is None else r["nms_map"][j], desc=desc[j])
            if i in out:                           # a map that fills a batch up a second time: the same bytes whatever slot it sits in
                np.testing.assert_array_equal(slot["feat"], out[i]["feat"])
            out.setdefault(i, slot)
    _RUNS[key] = out
    return out


def _check_against_reference(name, form, radius=4):
    got = _run(name, form, radius)
    one = _run(name, "b1", radius)
    B = FORMS[form][0]
    worst32 = worst64 = 0.0
    for i, g in sorted(got.items()):
        ref = R.detector_ref(name, i, radius)
        n, feat = len(ref["score"]), g["feat"]
        print(f"{name}[{i}] {form} r{radius}: n = {g['n']} (reference {n}), candidates {g['cand_cnt']} (reference {ref['cand_cnt']})")
        assert g["n"] == n and g["cand_cnt"] == ref["cand_cnt"]
        np.testing.assert_array_equal(feat[:n, 0], ref["score"])
        np.testing.assert_array_equal(feat[:n, 1], (ref["x"] * WS).astype(F))
        np.testing.assert_array_equal(feat[:n, 2], (ref["y"] * HS).astype(F))
        assert (feat[n:] == SENTINEL).all(), "a row k >= n was written"
        if radius == 4:
            np.testing.assert_array_equal(g["keep"], R.pack_plane(ref["keep"]))
        assert (g["nms_map"] is not None) == (radius > 0 and (B <= 2 or radius != 4)), "the dense NMS'd map is written by the one- and two-image forms only"
        if g["nms_map"] is not None:
            np.testing.assert_array_equal(g["nms_map"], ref["nms"])
        # descriptors: the reference's sampling, float32 operation for operation, on the device's own dense head map (the head GEMM is pinned elsewhere)
        assert np.isfinite(feat[:n]).all()
        if n:
            want = ref_post.extract_descriptors(np.ascontiguousarray(g["desc"].transpose(2, 0, 1)), ref["x"], ref["y"])
            worst32 = max(worst32, float(np.abs(feat[:n, 3:] - want).max()))
            np.testing.assert_allclose(feat[:n, 3:], want, atol=2e-6, rtol=0)
            inner = (ref["x"] < 511) & (ref["y"] < 511)        # (at 511 the bilinear weights cancel: zero in float32, noise in float64 — tests/test_detector_tail_ref_cpu.py)
            if inner.any():
                worst64 = max(worst64, float(np.abs(feat[:n, 3:][inner] - R.extract_descriptors_f64(g["desc"], ref["x"][inner], ref["y"][inner])).max()))
        np.testing.assert_array_equal(feat, one[i]["feat"])    # the bytes of the one-image form, descriptors and sentinel rows included
    _F64[f"{name}/{form}/r{radius}"] = dict(max_abs_vs_float32_restatement=worst32, max_abs_vs_float64_restatement=worst64)
    diag("detector_tail_pin_descriptors", **{k: str(v) for k, v in sorted(_F64.items())})


CASES4 = [n for n in R.DETECTOR_CASES]


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", CASES4)
def test_detector_tail_case(name, form):
    _check_against_reference(name, form)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("radius", [2, 0])
@pytest.mark.parametrize("name", R.NMS_CASES)
def test_nms_cases_at_other_radii(name, radius, form):
    """radius 2: the multi-pass NMS kernels + launch_candidates; radius 0: launch_candidates on the raw map"""
    _check_against_reference(name, form, radius)


def test_case_activity_on_the_device():
    """the device saw what the cases claim: more than four survivors per lane block, full blocks, a cut inside one score level"""
    keep = _run("nms_plateaus", "b1")[0]["keep"]
    bits = np.array([bin(int(w)).count("1") for w in keep.reshape(-1)]).reshape(64, 64)
    assert (bits == 64).sum() > 3000 and bits[10, 20] == 64
    few = _run("nms_few_values", "b3")[0]
    assert few["cand_cnt"] > 10000 and few["n"] == 400 and len(np.unique(few["feat"][:400, 0])) == 1


def test_zero_descriptor_stays_zero():
    z = R.case("zero_descriptor")
    y, x = z["claims"]["zero_keypoint"]
    for form in FORMS:
        r = _run("zero_descriptor", form)[0]            # (the call did not raise: the activation-range flag stayed down)
        feat = r["feat"][:r["n"]]
        row = feat[(feat[:, 1] == F(x) * WS) & (feat[:, 2] == F(y) * HS)]
        assert row.shape[0] == 1 and (row[0, 3:] == 0).all() and np.isfinite(feat).all()
        others = feat[(feat[:, 1] != F(x) * WS)]
        assert len(others) == 2 and np.allclose(np.linalg.norm(others[:, 3:], axis=1), 1, atol=1e-5)


# ---------------------------------------------------------------------------------------------------------------- line filter + junction scan
def _line_reference(lp, border, b, nms):
    m2 = lp["m2"][b]
    lines, jmap = R.line_filter(lp["la"][b, :m2], lp["sc"][b, :m2], border, R.LINE_THR, R.LEN_THR, WS, HS)
    return lines, R.junction_detector(jmap, nms, border)


@pytest.mark.parametrize("from_plane", [False, True], ids=["dense_map", "keep_plane"])
@pytest.mark.parametrize("border", [4, 0])
@pytest.mark.parametrize("m2s", [(0, 1, 1023, 1024), (1025,)], ids=["m2_0_1_1023_1024", "m2_1025"])
def test_line_filter_and_junction_scan(m2s, border, from_plane):
    ctx = _ctx("pl", remove_borders=border)
    lp = R.line_post(border, m2s)
    nms = R.simple_nms(lp["heat"][0], 4)                # (one score map for every image of the case)
    capL, capJ = 1100, 2200
    r = ctx.debug_line_post(lp["la"], lp["sc"], lp["m2"], lp["heat"], capL, capJ, from_plane=from_plane, h=H, w=W, sentinel=SENTINEL)
    small = ctx.debug_line_post(lp["la"], lp["sc"], lp["m2"], lp["heat"], 16, 8, from_plane=from_plane, h=H, w=W, sentinel=SENTINEL)
    for b in range(len(m2s)):
        lines, junc = _line_reference(lp, border, b, nms)
        nl, nj = len(lines), len(junc)
        print(f"m2 = {m2s[b]}: lines {r['nlines'][b]} / found {r['nfound'][b]} (reference {nl}), junctions {r['njunc'][b]} / found {r['jfound'][b]} (reference {nj}), "
              f"with score 0: {int((junc[:, 0] == 0).sum())}")
        assert nl < capL and nj < capJ
        assert r["nlines"][b] == r["nfound"][b] == nl and r["njunc"][b] == r["jfound"][b] == nj
        np.testing.assert_array_equal(r["lines"][b, :nl], lines)
        assert (r["lines"][b, nl:] == SENTINEL).all()
        np.testing.assert_array_equal(r["junc"][b, :nj, :3], junc)
        assert (r["junc"][b, :, 3:] == SENTINEL).all() and (r["junc"][b, nj:] == SENTINEL).all()
        # capacities below the counts: the first rows in index / raster order, the true counts reported
        assert small["nfound"][b] == nl and small["nlines"][b] == min(nl, 16) and small["jfound"][b] == nj and small["njunc"][b] == min(nj, 8)
        np.testing.assert_array_equal(small["lines"][b, :min(nl, 16)], lines[:16])
        np.testing.assert_array_equal(small["junc"][b, :min(nj, 8), :3], junc[:8])
        assert (small["lines"][b, min(nl, 16):] == SENTINEL).all() and (small["junc"][b, min(nj, 8):] == SENTINEL).all() and (small["junc"][b, :, 3:] == SENTINEL).all()
        if m2s[b] >= 1023:
            assert nl > 16 and nj > 8 and (junc[:, 0] == 0).any() and (junc[:, 0] > 0).any()


@pytest.mark.parametrize("from_plane", [False, True], ids=["dense_map", "keep_plane"])
@pytest.mark.parametrize("border", [4, 0])
def test_junction_scan_bounds_on_a_given_map(border, from_plane):
    """the scan alone on junction maps that hold what the filter never marks: whole rows and columns on and beside the border lines (upper bound exclusive), the first
    and last pixel of all 64 spans, 1 % random pixels; capacity above and below the count"""
    ctx = _ctx("pl", remove_borders=border)
    lp = R.line_post(border, (1, 1))
    jm = R.scan_maps(border)
    nms = R.simple_nms(lp["heat"][0], 4)
    for capJ in (12000, 100):
        r = ctx.debug_line_post(lp["la"], lp["sc"], lp["m2"], lp["heat"], 16, capJ, from_plane=from_plane, h=H, w=W, sentinel=SENTINEL, jmap=jm)
        for b in range(2):
            junc = R.junction_detector(jm[b], nms, border)
            k = min(len(junc), capJ)
            print(f"map {b}, capacity {capJ}: junctions {r['njunc'][b]} / found {r['jfound'][b]} (reference {len(junc)})")
            assert r["njunc"][b] == k and r["jfound"][b] == len(junc) and (b == 1 or len(junc) > 4000)
            np.testing.assert_array_equal(r["junc"][b, :k, :3], junc[:k])
            assert (r["junc"][b, k:] == SENTINEL).all() and (r["junc"][b, :, 3:] == SENTINEL).all()


# ---------------------------------------------------------------------------------------------------------------- junction top-300
@pytest.mark.parametrize("batched", [True, False], ids=["B4", "B1"])
def test_junction_top300(batched):
    """get_junctions against the contract (oracle/ref_nets.junctions_topk): score order whatever the number of maxima — more than 300, a flat map (16384 tied), a plateau
    across the cut, and 40 maxima (fewer than 300: detect_point's raster rule must NOT apply here)"""
    ctx = _ctx("pl", remove_borders=4)
    c = R.junctions_topk_cases()
    n = len(c["jloc"])
    got = ctx.debug_junctions_topk(c["jloc"], c["joff"]) if batched else np.concatenate([ctx.debug_junctions_topk(c["jloc"][b:b + 1], c["joff"][b:b + 1]) for b in range(n)])
    for b in range(n):
        want = ref_nets.junctions_topk(c["jloc"][b], c["joff"][b])
        print(f"junction map {b}: {c['claims']['counts'][b]} maxima, rows equal to the contract: {int((got[b] == want).all(1).sum())} / 300")
        np.testing.assert_array_equal(got[b], want)
