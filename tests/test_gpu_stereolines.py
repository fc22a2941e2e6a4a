"""Stereo line triangulation on the GPU (include/airfe.h "Stereo lines"): airfe_stereo_lines_batch_dev through the C ABI against the host entry
(airfe_stereo_lines) and the Python restatement (tests/stereoline_ref.py), byte for byte, on hand-built and seeded input; the composite
airfe_stereo_line_landmarks_batch_dev against the same chain through the existing entries; the argument checks."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import stereoline_ref as sr
from airslam_amd import api, synth, weights
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
KEYS = ("lines_right_sel", "right_valid", "status", "endpoints", "plucker", "count")
_C = {}


def _ctx():
    if "plain" not in _C:
        _C["plain"] = api.Context(lightglue=weights.synthetic_lightglue(1234, n_layers=2), max_batch=1, max_keypoints=256)
    return _C["plain"]


def _outputs(B, cap, dev):
    """sentinel-filled output buffers: what the entry does not write shows"""
    return dict(lines_right_sel=torch.full((B, cap, 4), -7.0, dtype=torch.float64, device=dev), right_valid=torch.full((B, cap), 77, dtype=torch.uint8, device=dev),
                status=torch.full((B, cap), -7, dtype=torch.int32, device=dev), endpoints=torch.full((B, cap, 6), -7.0, dtype=torch.float64, device=dev),
                plucker=torch.full((B, cap, 6), -7.0, dtype=torch.float64, device=dev), count=torch.full((B, 3), -7, dtype=torch.int32, device=dev))


def _args(o):
    return [o[k] for k in KEYS]


def _expected(per_frame, B, cap):
    """per-frame results (nl rows each) laid into sentinel-filled host buffers of the device shapes"""
    want = dict(lines_right_sel=np.full((B, cap, 4), -7.0), right_valid=np.full((B, cap), 77, np.uint8), status=np.full((B, cap), -7, np.int32),
                endpoints=np.full((B, cap, 6), -7.0), plucker=np.full((B, cap, 6), -7.0), count=np.zeros((B, 3), np.int32))
    for b, f in enumerate(per_frame):
        n = len(f["status"])
        for k in KEYS[:5]:
            want[k][b, :n] = f[k]
        want["count"][b] = f["count"]
    return want


def _same(got, want):
    return [k for k in KEYS if got[k].cpu().numpy().tobytes() != np.ascontiguousarray(want[k]).tobytes()]


def test_hand_built_frames_equal_the_host_entry_and_the_restatement():
    ctx, dev = _ctx(), torch.device("cuda")
    frames = sr.hand_frames(8)
    B, cap = 3, 8
    t = lambda key, dt: torch.from_numpy(np.stack([np.asarray(f[key]) for f in frames]).astype(dt)).to(dev)
    left, right, matches, Twc = t("left", np.float64), t("right", np.float64), t("matches", np.int32), t("Twc", np.float64)
    nl = torch.tensor([f["nl"] for f in frames], dtype=torch.int32, device=dev)
    nr = torch.tensor([f["nr"] for f in frames], dtype=torch.int32, device=dev)
    assert nl.tolist() == [8, 6, 0] and nr.tolist()[1] == 1
    ref = [sr.frame(sr.CAM, f["left"], f["nl"], f["right"], f["nr"], f["matches"], f["Twc"]) for f in frames]
    host = [ctx.stereo_lines(sr.CAM, f["left"][:f["nl"]], f["right"][:f["nr"]], f["matches"][:f["nl"]], f["Twc"]) for f in frames]
    for b, f in enumerate(frames):
        assert ref[b]["status"].tolist() == f["status"]
        for k in KEYS:
            assert np.ascontiguousarray(host[b][k]).tobytes() == np.ascontiguousarray(ref[b][k]).tobytes(), (b, k)      # the host entry == the restatement
    want = _expected(ref, B, cap)
    runs = []
    for _ in range(2):
        out = _outputs(B, cap, dev)
        ctx.stereo_lines_batch_dev(sr.CAM, left, nl, right, nr, matches, Twc, *_args(out))
        ctx.sync()
        assert _same(out, want) == []                               # ... == the device, and the sentinel behind every frame's lines is untouched
        runs.append({k: out[k].cpu().numpy().tobytes() for k in KEYS})
    assert runs[0] == runs[1]
    assert want["count"].tolist() == [[7, 4, 3], [0, 0, 0], [0, 0, 0]]


@pytest.mark.parametrize("with_pose", [True, False], ids=["Twc", "NULL"])
def test_seeded_pairs_equal_the_restatement(with_pose):
    ctx, dev = _ctx(), torch.device("cuda")
    s = sr.seeded_pairs()
    B, cap = sr.SEED_B, sr.SEED_CAP
    # left and right lines as the two halves of ONE [2B][capL][4] buffer, counts likewise: the layout airfe_stereo_plnet_batch_dev writes
    lines = torch.from_numpy(np.concatenate([s["left"], s["right"]])).to(dev)
    nlines = torch.from_numpy(np.concatenate([s["nl"], s["nr"]])).to(dev)
    matches = torch.from_numpy(s["matches"]).to(dev)
    Twc = torch.from_numpy(s["Twc"]).to(dev) if with_pose else None
    out = _outputs(B, cap, dev)
    ctx.stereo_lines_batch_dev(sr.CAM, lines[:B], nlines[:B], lines[B:], nlines[B:], matches, Twc, *_args(out))
    ctx.sync()
    ref = sr.seeded_reference(with_pose)
    want = _expected(ref, B, cap)
    assert _same(out, want) == []
    counts = np.bincount(out["status"].cpu().numpy().reshape(-1), minlength=6)
    assert (counts >= 100).all() and counts[0] >= 1024, counts      # (what tests/test_stereoline_cpu.py asserts of the restatement alone)


def test_composite_equals_the_chain_by_hand():
    """B = 3 synthetic stereo pairs through the PLNet stereo step; then the composite against assign x 2 + match (with the band) through the existing entries
    and Context.stereo_lines per frame on the downloaded lists."""
    B, H, W, K, CL, CJ, CE = 3, 480, 752, 400, 512, 1024, 8192
    cam = (2.0, 60.0, 3.0, 47.90639384423901, 458.654, 457.296, 367.215, 248.375)
    ctx = api.Context(superpoint=weights.synthetic_plnet_s0(1234), lightglue=weights.synthetic_lightglue(1234), plnet_s1=os.path.join(GOLDEN, "plnet_s1.airfe"),
                      max_batch=B, enc_chunk=min(2 * B, 16), max_keypoints=K, image_width=W, image_height=H)
    dev = torch.device("cuda")
    ls, rs = synth.stereo_batch(B, H, W, 31)
    L, R = torch.from_numpy(ls).to(dev), torch.from_numpy(rs).to(dev)
    fl = torch.zeros((B, K, 259), device=dev); fr = torch.zeros((B, K, 259), device=dev)
    nl = torch.zeros((B,), dtype=torch.int32, device=dev); nr = torch.zeros((B,), dtype=torch.int32, device=dev)
    idx = torch.zeros((B, K, 2), dtype=torch.int32, device=dev); sc = torch.zeros((B, K), device=dev)
    nm = torch.zeros((B,), dtype=torch.int32, device=dev)
    lines = torch.zeros((2 * B, CL, 4), dtype=torch.float64, device=dev); nlines = torch.zeros((2 * B,), dtype=torch.int32, device=dev)
    junc = torch.zeros((B, CJ, 259), device=dev); njunc = torch.zeros((B,), dtype=torch.int32, device=dev)
    ctx.stereo_plnet_batch_dev(L, R, fl, fr, nl, nr, lines, nlines, junc, njunc, idx, sc, nm)
    ctx.sync()
    rng = np.random.RandomState(7)
    Twc_h = np.stack([sr._pose(rng) for _ in range(B)])
    Twc = torch.from_numpy(Twc_h).to(dev)

    def relation():
        return (torch.zeros((B, CL + 1), dtype=torch.int32, device=dev), torch.full((B, CE), -7, dtype=torch.int32, device=dev),
                torch.full((B, CE), -7.0, dtype=torch.float64, device=dev), torch.zeros((B,), dtype=torch.int32, device=dev))

    # the chain by hand
    hl, hr = relation(), relation()
    hlm = torch.full((B, CL), -9, dtype=torch.int32, device=dev)
    ctx.assign_points_to_lines_batch_dev(lines[:B], nlines[:B], fl, nl, *hl)
    ctx.assign_points_to_lines_batch_dev(lines[B:], nlines[B:], fr, nr, *hr)
    ctx.match_lines_batch_dev(hl[0], hl[1], nlines[:B], nl, hr[0], hr[1], nlines[B:], nr, idx, nm, hlm, stereo_filter=cam[:3], feat0_t=fl, feat1_t=fr)
    ctx.sync()
    lines_h, nlines_h, hlm_h = lines.cpu().numpy(), nlines.cpu().numpy(), hlm.cpu().numpy()
    per_frame = [ctx.stereo_lines(cam, lines_h[b, :nlines_h[b]], lines_h[B + b, :nlines_h[B + b]], hlm_h[b, :nlines_h[b]], Twc_h[b]) for b in range(B)]
    want = _expected(per_frame, B, CL)
    # the composite, into buffers of its own
    cl, cr = relation(), relation()
    clm = torch.full((B, CL), -9, dtype=torch.int32, device=dev)
    out = _outputs(B, CL, dev)
    ctx.stereo_line_landmarks_batch_dev(cam, lines[:B], nlines[:B], lines[B:], nlines[B:], fl, nl, fr, nr, idx, nm, Twc, cl, cr, clm, *_args(out))
    ctx.sync()
    for got, hand in zip(cl + cr + (clm,), hl + hr + (hlm,)):
        assert torch.equal(got, hand)                               # the relations and the line matches: whole buffers
    assert _same(out, want) == []
    total = want["count"].sum(0)
    print("stereo lines of the synthetic pairs: left lines %d, valid right %d, triangulated %d, map lines %d" % (int(nlines_h[:B].sum()), *total.tolist()))
    for b in range(B):                                              # and the restatement agrees with the host entry on this input too
        ref = sr.frame(cam, lines_h[b], int(nlines_h[b]), lines_h[B + b], int(nlines_h[B + b]), hlm_h[b], Twc_h[b])
        for k in KEYS:
            assert np.ascontiguousarray(per_frame[b][k]).tobytes() == np.ascontiguousarray(ref[k]).tobytes(), (b, k)
    ctx.close()


def test_bad_arguments_are_refused_with_a_message():
    """negative capL, a batch below 1 or above the launch's 65535 frames (max_batch does not apply: the entries use nothing sized by it), NULL outputs"""
    ctx, dev = _ctx(), torch.device("cuda")
    B, cap = 2, 8
    lines = torch.zeros((2 * B, cap, 4), dtype=torch.float64, device=dev)
    n = torch.zeros((2 * B,), dtype=torch.int32, device=dev)
    lm = torch.full((B, cap), -1, dtype=torch.int32, device=dev)
    out = _outputs(B, cap, dev)
    cam = (C.c_double * 8)(*sr.CAM)
    camp = C.cast(cam, C.c_void_p)
    p = lambda t: t.data_ptr()
    outs = [p(o) for o in _args(out)]
    torch.cuda.synchronize()

    def batch(capL=cap, nb=B, o=outs, cam_=camp):
        return ctx._l.airfe_stereo_lines_batch_dev(ctx._h, cam_, p(lines[:B]), p(n[:B]), p(lines[B:]), p(n[B:]), capL, p(lm), None, nb, *o, None)

    def err():
        return (ctx._l.airfe_last_error(ctx._h) or b"").decode()

    assert batch(capL=-1) != 0 and "stereo_lines_batch_dev: bad argument" in err()
    assert batch(nb=0) != 0 and "stereo_lines_batch_dev: bad argument" in err()
    assert batch(nb=65536) != 0 and "stereo_lines_batch_dev: bad argument" in err()
    assert batch(cam_=None) != 0 and "stereo_lines_batch_dev: bad argument" in err()
    for k in range(6):
        assert batch(o=outs[:k] + [None] + outs[k + 1:]) != 0 and "stereo_lines_batch_dev: null output" in err()
    feat = torch.zeros((B, 16, 259), device=dev)
    npts = torch.zeros((B,), dtype=torch.int32, device=dev)
    idx = torch.zeros((B, 16, 2), dtype=torch.int32, device=dev)
    rel = [torch.zeros((B, cap + 1), dtype=torch.int32, device=dev), torch.zeros((B, 32), dtype=torch.int32, device=dev),
           torch.zeros((B, 32), dtype=torch.float64, device=dev), torch.zeros((B,), dtype=torch.int32, device=dev)]
    relp = [p(r) for r in rel]
    torch.cuda.synchronize()

    def composite(capL=cap, nb=B, o=outs, lm_=p(lm), capE=32):
        return ctx._l.airfe_stereo_line_landmarks_batch_dev(ctx._h, camp, p(lines[:B]), p(n[:B]), p(lines[B:]), p(n[B:]), capL, p(feat), p(npts), p(feat), p(npts),
                                                            16, p(idx), p(npts), 16, None, nb, *relp, *relp, capE, lm_, *o, None)

    assert composite(capL=-1) != 0 and "stereo_line_landmarks_batch_dev: bad argument" in err()
    assert composite(nb=0) != 0 and "stereo_line_landmarks_batch_dev: bad argument" in err()
    assert composite(nb=65536) != 0 and "stereo_line_landmarks_batch_dev: bad argument" in err()
    assert composite(capE=0) != 0 and "stereo_line_landmarks_batch_dev: bad argument" in err()
    assert composite(lm_=None) != 0 and "stereo_line_landmarks_batch_dev: null output" in err()
    assert composite(o=outs[:5] + [None]) != 0 and "stereo_line_landmarks_batch_dev: null output" in err()
    one = np.zeros((1, 4))
    with pytest.raises(api.AirfeError, match="stereo_lines: bad argument"):
        ctx._chk(ctx._l.airfe_stereo_lines(ctx._h, camp, one.ctypes.data, -1, one.ctypes.data, 1, None, None, None, None, None, None, None, None), "airfe_stereo_lines")
    with pytest.raises(api.AirfeError, match="stereo_lines: bad argument"):
        ctx._chk(ctx._l.airfe_stereo_lines(ctx._h, camp, one.ctypes.data, 1, one.ctypes.data, 1, None, None, None, None, None, None, None, None), "airfe_stereo_lines")
    # nothing was written by a refused call, and the context still works: empty frames give zero counts and touch nothing else
    assert all((o == s).all() for o, s in zip(_args(out), (-7.0, 77, -7, -7.0, -7.0, -7)))
    assert batch() == 0 and composite() == 0
    ctx.sync()
    assert not out["count"].any() and (out["status"] == -7).all() and (out["endpoints"] == -7.0).all()
