"""The detector's tail behind the encoder at batch sizes that take the sparse descriptor path (B > 2): NMS -> top-K (+ the gather rows) -> descriptor head with the
sampling in its epilogue, each stage ONE launch over both stereo sides.  The gate is byte equality — whole buffers, unused rows included — with the same images run
one per call: a one-image call takes the dense NMS'd map, the dense descriptor head, sample_desc(compact = 0) and one-destination launches, the forms the batched
ones are derived from.  The feature buffers start from a sentinel, so a write to a row k >= n[b] shows."""
import os

import numpy as np
import pytest

from airslam_amd import api, synth, weights
from conftest import GOLDEN
from hostile import hostile_detector

pytestmark = pytest.mark.gpu
SENTINEL = 7.0
FUSED = {"gemmr_min_m": 256}          # the streaming gather GEMM (with the sampling in it) from 256 rows on; default: the tiled kernel + sample_desc(compact = 1) at these sizes


def _ctx(tuning=None, **kw):
    return api.Context(superpoint=weights.synthetic_superpoint(1234), lightglue=weights.synthetic_lightglue(1234, n_layers=2), max_batch=8, enc_chunk=4,
                       check_launches=1, tuning=tuning, **kw)


def _one_per_call(torch, ctx, imgs, cap):
    """every image through a batch-1 call of its own -> feat [B][cap][259] (sentinel where nothing is written), n [B]"""
    feats, ns = [], []
    for img in imgs:
        f = torch.full((1, cap, 259), SENTINEL, device="cuda")
        n = torch.zeros((1,), dtype=torch.int32, device="cuda")
        ctx.detect_batch_dev(torch.from_numpy(img[None]).cuda(), f, n)
        ctx.sync()
        feats.append(f.cpu().numpy()[0]); ns.append(int(n.cpu().numpy()[0]))
    return np.stack(feats), np.array(ns, np.int32)


@pytest.fixture(scope="module")
def straddle_ref():
    """3 stereo pairs, 37 keypoints in rows of capacity 41, one image per call"""
    import torch
    ls, rs = synth.stereo_batch(3, 480, 752, 500)
    ctx = _ctx(max_keypoints=37)
    ref = _one_per_call(torch, ctx, list(ls) + list(rs), 41)
    ctx.close()
    return ls, rs, ref


@pytest.mark.parametrize("tuning", [FUSED, None], ids=["fused_gather", "tiled_fallback"])
def test_tiles_that_straddle_images_and_both_destinations(straddle_ref, tuning):
    """capacity 41 > max_keypoints 37: slots 37 .. 40 of every image are never filled; 8 keypoints per 32-row tile and 41 per image, so tiles straddle images and the
    left / right boundary (slot 123 = tile 15, slot 3); M = 6 * 41 * 4 = 984 rows pads to 1024: the last tile is padding only."""
    import torch
    ls, rs, (rfeat, rn) = straddle_ref
    B, cap = 3, 41
    ctx = _ctx(tuning, max_keypoints=37)
    fL, fR = torch.full((B, cap, 259), SENTINEL, device="cuda"), torch.full((B, cap, 259), SENTINEL, device="cuda")
    nL, nR = torch.zeros((B,), dtype=torch.int32, device="cuda"), torch.zeros((B,), dtype=torch.int32, device="cuda")
    idx, sc, nm = torch.zeros((B, cap, 2), dtype=torch.int32, device="cuda"), torch.zeros((B, cap), device="cuda"), torch.zeros((B,), dtype=torch.int32, device="cuda")
    ctx.stereo_batch_dev(torch.from_numpy(ls).cuda(), torch.from_numpy(rs).cuda(), fL, fR, nL, nR, idx, sc, nm)
    ctx.sync()
    got_n = np.concatenate([nL.cpu().numpy(), nR.cpu().numpy()])
    got = np.concatenate([fL.cpu().numpy(), fR.cpu().numpy()])
    ctx.close()
    print("keypoints per image:", got_n.tolist())
    assert rn.max() == 37, "top-K must cut at least one image for the test to mean what it says"
    np.testing.assert_array_equal(got_n, rn)
    np.testing.assert_array_equal(got, rfeat)                       # whole buffers: the sentinel rows 37 .. 40 (and k >= n) included
    assert (rfeat[:, 37:] == SENTINEL).all()


def test_ring_wrap_with_eight_workgroups():
    """8 images x 400 slots = 400 tiles over 8 persistent workgroups: each streams 50 tiles through its seven-slot ring and reuses the staging tile 50 times"""
    import torch
    imgs = np.stack([synth.gabor_image(480, 752, 40 + 3 * i) for i in range(8)])
    ctx = _ctx(dict(FUSED, gemmr_wgs=8))
    f = torch.full((8, 400, 259), SENTINEL, device="cuda")
    n = torch.zeros((8,), dtype=torch.int32, device="cuda")
    ctx.detect_batch_dev(torch.from_numpy(imgs).cuda(), f, n)
    ctx.sync()
    ctx.close()
    ref = _ctx()
    rfeat, rn = _one_per_call(torch, ref, imgs, 400)
    ref.close()
    print("keypoints per image:", rn.tolist())
    assert rn.min() > 100
    np.testing.assert_array_equal(n.cpu().numpy(), rn)
    np.testing.assert_array_equal(f.cpu().numpy(), rfeat)


def test_junction_scores_come_from_the_nms_bit_plane():
    """B = 5 > 2: no dense NMS'd map is written; a junction's score (column 0 of its row) is the raw score under the final keep mask.  Equal to the one-image
    calls (which read the dense map), and the inspection hook still rebuilds the map the one-image call holds."""
    import torch
    B, J, capJ = 5, 3, 1024
    imgs = np.stack([synth.gabor_image(480, 752, 8 + 3 * i) for i in range(B)])
    ctx = api.Context(superpoint=weights.synthetic_plnet_s0(1234), plnet_s1=os.path.join(GOLDEN, "plnet_s1.airfe"), max_batch=8, enc_chunk=4, check_launches=1)
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device="cuda")
    feat, n, lines, nlines = z(B, 400, 259), z(B, dt=torch.int32), z(B, 2048, 4, dt=torch.float64), z(B, dt=torch.int32)
    junc, njunc = z(J, capJ, 259), z(J, dt=torch.int32)
    ctx.detect_plnet_batch_dev(torch.from_numpy(imgs).cuda(), feat, n, lines, nlines, junc, njunc)
    ctx.sync()
    _, nms_batch, _ = ctx.detector_maps(B)
    nj, junc = njunc.cpu().numpy(), junc.cpu().numpy()
    kept = []
    for b in range(B):
        _, _, rj = ctx.detect_plnet(imgs[b], None, want_junctions=b < J)
        _, nms_one, _ = ctx.detector_maps(1)
        np.testing.assert_array_equal(nms_batch[b], nms_one[0])
        if b < J:
            assert nj[b] == rj.shape[0] and nj[b] >= 50
            np.testing.assert_array_equal(junc[b, :nj[b], 0], rj[:, 0])
            kept.append((int(nj[b]), int((rj[:, 0] != 0).sum())))
    ctx.close()
    print("junctions (all, with a non-zero score):", kept)


def test_non_finite_descriptors_fail_the_batched_call_like_the_single_one():
    """a pack whose 2-byte activations overflow: the 6-image call through the fused kernel fails with the "activation range" error of the one-image call, and names
    the same causes as the unfused form (tiled GEMM + sample_desc) does on the same batch"""
    import torch
    imgs = np.stack([synth.gabor_image(480, 752, 7 + i) for i in range(6)])
    errs = {}
    for name, tuning in (("fused", FUSED), ("unfused", None)):
        ctx = api.Context(superpoint=hostile_detector(), max_batch=8, enc_chunk=4, precision=1, check_launches=1, tuning=tuning)
        for batch in (imgs[:1], imgs):
            f = torch.zeros((len(batch), 400, 259), device="cuda")
            n = torch.zeros((len(batch),), dtype=torch.int32, device="cuda")
            ctx.detect_batch_dev(torch.from_numpy(batch).cuda(), f, n)
            with pytest.raises(api.AirfeError, match="left the fp16 range") as e:
                ctx.sync()
            errs[name, len(batch)] = str(e.value)[:160]
            print(name, len(batch), "images:", errs[name, len(batch)], "| keypoints:", n.cpu().numpy().tolist())
            ctx.sync()                                              # reported once, cleared
        ctx.close()
    assert errs["fused", 6] == errs["unfused", 6]
    assert errs["fused", 1] == errs["unfused", 1]
