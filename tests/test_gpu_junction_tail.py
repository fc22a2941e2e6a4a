"""The junction tail of the batched line path in its fused form — the junction list built inside the line filter from a bitmap in LDS, the descriptors from the
sampling gather GEMM at the junctions' tap rows (airfe_debug_junction_tail, include/airfe_debug.h) — on hand-built lines (tests/junction_tail_cases.py, whose claims
tests/test_junction_tail_ref_cpu.py checks).  Lines, counts, scores and positions are comparison and integer work: whole buffers equal the exact reference
(tests/detector_tail_ref.py), sentinel rows included, and the byte-map form (airfe_debug_line_post, one image at a time, either score source).  Descriptor rows are the
bytes of the one-image form (dense head + sample_desc) and lie within the bound tests/test_gpu_detector_tail_pin.py holds descriptors to (2e-6 absolute against the
reference's sampling restated in float32 on the device's own dense head map; the same against the float64 restatement, away from the pixels 511 where the float64 weights
do not cancel)."""
import os

import numpy as np
import pytest

import detector_tail_ref as R
import junction_tail_cases as J
from airslam_amd import api, weights
from conftest import GOLDEN
from gpu_common import diag
from oracle import ref_post

pytestmark = pytest.mark.gpu
F = np.float32
SENTINEL = 7.0
H, W, WS, HS = J.H, J.W, J.WS, J.HS
FUSED = {"gemmr_min_m": 256}                       # the streaming forms from 256 rows on
WRAP = {"gemmr_min_m": 256, "gemmr_wgs": 2}        # ... on two workgroups: 16 tiles each at capJ = 64 and four images, twice round the 7-slot ring
_CTX, _ACT, _NMS = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for c in _CTX.values():
        c.close()
    _CTX.clear()


def _ctx(border, tuning=None):
    key = (border, tuple(sorted((tuning or {}).items())))
    if key not in _CTX:
        _CTX[key] = api.Context(superpoint=weights.synthetic_plnet_s0(1234), plnet_s1=os.path.join(GOLDEN, "plnet_s1.airfe"), max_batch=4, enc_chunk=4,
                                check_launches=1, tuning=tuning, remove_borders=border)
    return _CTX[key]


def _act(B):
    if B not in _ACT:
        _ACT[B] = np.stack([R.activations(i) for i in range(B)])
    return _ACT[B]


def _nms():
    if "m" not in _NMS:
        _NMS["m"] = R.simple_nms(J.heat_map(), 4)
    return _NMS["m"]


def _check_rows(out, b, lines, junc, capL, capJ):
    """image b of a hook result against the exact reference: counts, lines, score / x / y of the junction rows, sentinels"""
    nl, nj = len(lines), len(junc)
    kl, kj = min(nl, capL), min(nj, capJ)
    assert out["nlines"][b] == kl and out["nfound"][b] == nl
    np.testing.assert_array_equal(out["lines"][b, :kl], lines[:kl])
    assert (out["lines"][b, kl:] == SENTINEL).all()
    if b < len(out["njunc"]):
        assert out["njunc"][b] == kj and out["jfound"][b] == nj
        np.testing.assert_array_equal(out["junc"][b, :kj, 0], junc[:kj, 0])
        np.testing.assert_array_equal(out["junc"][b, :kj, 1], (junc[:kj, 1] * WS).astype(F))
        np.testing.assert_array_equal(out["junc"][b, :kj, 2], (junc[:kj, 2] * HS).astype(F))
        assert (out["junc"][b, kj:] == SENTINEL).all(), "a row k >= n was written"
        assert np.isfinite(out["junc"][b, :kj]).all()


@pytest.mark.parametrize("border", [4, 0])
@pytest.mark.parametrize("B,nj", [(3, 2), (3, 3), (4, 3), (4, 4)])
def test_junction_list_in_the_line_filter(B, nj, border):
    ctx = _ctx(border, FUSED)
    images = J.list_batch(border, B)
    la, sc, m2 = J.pack(images)
    heat = np.stack([J.heat_map()] * B)
    capL, capJ = 32, 64
    out = ctx.debug_junction_tail(la, sc, m2, heat, _act(B), capL, capJ, nj=nj, h=H, w=W, sentinel=SENTINEL)
    assert out["fused"], "the fused form did not run"
    for b in range(B):
        lines, junc = J.reference(images[b], border, _nms())
        print(f"B = {B}, nj = {nj}, border {border}, image {b}: m2 = {m2[b]}, lines {out['nlines'][b]} / {out['nfound'][b]} (reference {len(lines)}), junctions "
              f"{out['njunc'][b] if b < nj else '-'} / {out['jfound'][b] if b < nj else '-'} (reference {len(junc)}), with score 0: {int((junc[:, 0] == 0).sum())}")
        _check_rows(out, b, lines, junc, capL, capJ)
        if b >= nj:
            continue
        # the byte-map form, one image at a time, from the dense NMS'd map and from the keep plane: the same lines, counts, scores and (unscaled) positions
        for from_plane in (False, True):
            one = ctx.debug_line_post(la[b:b + 1], sc[b:b + 1], m2[b:b + 1], heat[:1], capL, capJ, from_plane=from_plane, h=H, w=W, sentinel=SENTINEL)
            np.testing.assert_array_equal(out["lines"][b], one["lines"][0])
            assert (out["nlines"][b], out["nfound"][b], out["njunc"][b], out["jfound"][b]) == (one["nlines"][0], one["nfound"][0], one["njunc"][0], one["jfound"][0])
            k = int(one["njunc"][0])
            np.testing.assert_array_equal(out["junc"][b, :k, 0], one["junc"][0, :k, 0])
            np.testing.assert_array_equal(out["junc"][b, :k, 1], (one["junc"][0, :k, 1] * WS).astype(F))
            np.testing.assert_array_equal(out["junc"][b, :k, 2], (one["junc"][0, :k, 2] * HS).astype(F))
            np.testing.assert_array_equal(out["junc"][b, k:], one["junc"][0, k:])
    if B == 4:
        assert out["jfound"][0] > capJ and out["njunc"][0] == capJ and (nj < 3 or out["jfound"][2] == 0)


COUNTS = {24: [(9, 0, 24, 7), (1, 23, 8, 0), (8, 0, 24)], 64: [(9, 0, 64, 7), (1, 63, 8, 0), (8, 0, 64)]}


@pytest.mark.parametrize("tuning", [FUSED, WRAP], ids=["wgs_default", "wgs_2"])
@pytest.mark.parametrize("capJ", [24, 64])
def test_junction_descriptors_from_the_gather_gemm(capJ, tuning):
    """junction counts 0, 1, 7, 8, 9, capJ - 1, capJ: tile edges, a dead image inside the live prefix, a full image; corner pixels whose taps clip (border 0)"""
    ctx = _ctx(0, tuning)
    worst32 = worst64 = 0.0
    for bi, counts in enumerate(COUNTS[capJ]):
        B = len(counts)
        images = [J.counted_image(n, 100 * capJ + 10 * bi + b) for b, n in enumerate(counts)]
        la, sc, m2 = J.pack(images)
        heat, act = np.stack([J.heat_map()] * B), _act(B)
        out = ctx.debug_junction_tail(la, sc, m2, heat, act, 8, capJ, h=H, w=W, sentinel=SENTINEL)
        assert out["fused"], "the fused form did not run"
        _, _, desc = ctx.detector_maps(B)                      # the device's dense normalised head map of these activations
        for b, n in enumerate(counts):
            lines, junc = J.reference(images[b], 0, _nms())
            assert len(junc) == n
            _check_rows(out, b, lines, junc, 8, capJ)
            # the one-image form: dense NMS'd map, byte maps and scan, dense head, sample_desc — the same bytes, sentinel rows included
            one = ctx.debug_junction_tail(la[b:b + 1], sc[b:b + 1], m2[b:b + 1], heat[:1], act[b:b + 1], 8, capJ, h=H, w=W, sentinel=SENTINEL)
            assert not one["fused"]
            np.testing.assert_array_equal(out["junc"][b], one["junc"][0])
            if n == 0:
                continue
            got = out["junc"][b, :n, 3:]
            want = ref_post.extract_descriptors(np.ascontiguousarray(desc[b].transpose(2, 0, 1)), junc[:, 1], junc[:, 2])
            d32 = float(np.abs(got - want).max())
            inner = (junc[:, 1] < 511) & (junc[:, 2] < 511)
            d64 = float(np.abs(got[inner] - R.extract_descriptors_f64(desc[b], junc[inner, 1], junc[inner, 2])).max()) if inner.any() else 0.0
            worst32, worst64 = max(worst32, d32), max(worst64, d64)
            print(f"capJ {capJ}, batch {counts}, image {b}: {n} junctions, max |d| vs float32 restatement {d32:.3g}, vs float64 {d64:.3g}")
            np.testing.assert_allclose(got, want, atol=2e-6, rtol=0)
            assert d64 <= 2e-6
    diag("junction_tail_descriptors", **{f"capJ{capJ}/{'wgs2' if 'gemmr_wgs' in tuning else 'wgs'}": str(dict(max_abs_vs_float32_restatement=worst32,
                                                                                                               max_abs_vs_float64_restatement=worst64))})


def test_unfused_forms_give_the_same_bytes():
    """the same batch with the streaming form out of reach (default gemmr_min_m): byte maps, scan, the junction images' dense head, sample_desc — the fused form's bytes"""
    counts = COUNTS[24][0]
    images = [J.counted_image(n, 900 + b) for b, n in enumerate(counts)]
    la, sc, m2 = J.pack(images)
    heat, act = np.stack([J.heat_map()] * 4), _act(4)
    a = _ctx(0, FUSED).debug_junction_tail(la, sc, m2, heat, act, 8, 24, nj=3, h=H, w=W, sentinel=SENTINEL)
    b = _ctx(0, None).debug_junction_tail(la, sc, m2, heat, act, 8, 24, nj=3, h=H, w=W, sentinel=SENTINEL)
    assert a["fused"] and not b["fused"]
    for k in ("lines", "nlines", "nfound", "junc", "njunc", "jfound"):
        np.testing.assert_array_equal(a[k], b[k])
