"""F-matrix RANSAC on the device (kernels_fransac.hip; contract: include/airfe.h "F-matrix RANSAC") against the numpy restatement (tests/fransac_ref.py),
the one-call entry against the batch entry, the host entries with outlier rejection on, the reference's own MatchingPoints(..., true) on the device's
scores (its cv::findFundamentalMat is the project's C++ stand-in: what that pins is the reference's glue, not OpenCV), and the sequence drivers."""

import numpy as np
import pytest

import fransac_ref as fr
from airslam_amd import api, seq, synth, weights
from gpu_common import diag
from oracle import ref_lib

pytestmark = pytest.mark.gpu
live = pytest.mark.skipif(not fr.oracle_has_stand_in(),
                          reason="oracle/_ref/libairslam_ref.so did not travel to this machine or predates the cv::findFundamentalMat stand-in")
W, H = 752, 480
_C = {}


def _ctx(kind="lg"):
    if kind not in _C:
        if kind == "lg":
            _C[kind] = api.Context(lightglue=weights.synthetic_lightglue(1234), max_batch=1, max_keypoints=1024)
        elif kind == "sg":
            _C[kind] = api.Context(superglue=weights.synthetic_superglue(1234), matcher=1, max_batch=1, max_keypoints=1024)
        elif kind == "sp":
            _C[kind] = api.Context(superpoint=weights.synthetic_superpoint(1234), max_batch=2, enc_chunk=2)
        elif kind == "track":
            _C[kind] = api.Context(superpoint=weights.synthetic_superpoint(1234), lightglue=weights.synthetic_lightglue(1234), max_batch=2, enc_chunk=2,
                                   max_keypoints=400, image_width=W, image_height=H)
    return _C[kind]


def _case(m, k):
    """planted list k of length m: (f0, f1, idx, score) with idx = (i, i) in a shuffled order"""
    ratio = (1.0, 0.9, 0.6, 0.3)[k % 4]
    if m == 0:
        return np.zeros((1, 259), np.float32), np.zeros((1, 259), np.float32), np.zeros((0, 2), np.int32), np.zeros(0, np.float32)
    _, _, _, xyf = fr.planted(m, ratio, seed=1000 * m + k)
    f0, f1 = fr.features_for(xyf, seed=k)
    rng = np.random.default_rng(k)
    idx = np.stack([np.arange(m), rng.permutation(m)], 1).astype(np.int32)
    f1 = f1[np.argsort(idx[:, 1])]                               # row idx[i, 1] of f1 is the partner of row i of f0
    score = rng.random(m, dtype=np.float32)
    return f0, f1, idx, score


def _batch(cases, cap=1024, mcap=1024):
    import torch
    B = len(cases)
    f0 = torch.zeros((B, cap, 259), dtype=torch.float32); f1 = torch.zeros_like(f0)
    idx = torch.zeros((B, mcap, 2), dtype=torch.int32); sc = torch.zeros((B, mcap)); nm = torch.zeros(B, dtype=torch.int32)
    for b, (a0, a1, i, s) in enumerate(cases):
        f0[b, :len(a0)] = torch.from_numpy(a0); f1[b, :len(a1)] = torch.from_numpy(a1)
        idx[b, :len(i)] = torch.from_numpy(i); sc[b, :len(s)] = torch.from_numpy(s); nm[b] = len(i)
    d = [x.cuda() for x in (f0, f1, idx, sc, nm)]
    F = torch.zeros((B, 9), dtype=torch.float64, device="cuda")
    _ctx().fundamental_ransac_batch_dev(*d, F_t=F)
    torch.cuda.synchronize()
    out = []
    for b in range(B):
        n = int(d[4][b])
        out.append((d[2][b, :n].cpu().numpy(), d[3][b, :n].cpu().numpy(), F[b].cpu().numpy()))
    return out


def _oracle(case):
    f0, f1, idx, score = case
    r = fr.fransac(fr.points(f0, f1, idx)) if len(idx) else dict(mask=np.zeros(0, bool), F=np.zeros(9), sel=-2, err=None)
    return r


def _check(case, got, near):
    f0, f1, idx, score = case
    r = _oracle(case)
    gi, gs, gF = got
    keep = r["mask"]
    if r["err"] is not None:                                     # matches whose oracle error sits within 1e-9 of the threshold may go either way
        near[0] += int((np.abs(r["err"].astype(np.float64) - 400.0) <= 4e-7).sum())
    np.testing.assert_array_equal(gi, idx[keep])
    np.testing.assert_array_equal(gs, score[keep])
    np.testing.assert_allclose(gF, r["F"], rtol=1e-7, atol=1e-12)   # same selected sample and model (a different one differs at O(1))


@pytest.mark.parametrize("B", [1, 7, 64])
def test_batch_kernel_equals_the_numpy_restatement(B):
    sizes = [0, 7, 8, 9, 14, 15, 16, 400, 1024]
    cases = [_case(sizes[b % len(sizes)], b) for b in range(B)]
    got = _batch(cases)
    near = [0]
    for c, g in zip(cases, got):
        _check(c, g, near)
    diag(f"fransac_vs_numpy_B{B}", pairs=B, near_threshold=near[0])


def test_a_pair_gives_the_same_bytes_alone_and_anywhere_in_a_batch():
    cases = [_case([400, 1024, 15, 60][b % 4], 50 + b) for b in range(64)]
    full = _batch(cases)
    again = _batch(cases)
    for b in (0, 17, 63):
        alone = _batch([cases[b]])[0]
        for x, y, z in zip(alone, full[b], again[b]):
            assert x.tobytes() == y.tobytes() == z.tobytes()


def test_host_entry_equals_the_batch_entry_and_keeps_short_lists():
    ctx = _ctx()
    for m, k in ((400, 1), (1024, 2), (12, 3), (30, 2)):
        c = _case(m, k)
        gi, gs = ctx.fundamental_ransac(*c)
        bi, bs, _ = _batch([c])[0]
        assert gi.tobytes() == bi.tobytes() and gs.tobytes() == bs.tobytes()
    c = _case(8, 0)
    gi, gs = ctx.fundamental_ransac(*c)
    assert gi.tobytes() == c[2].tobytes() and gs.tobytes() == c[3].tobytes()


def test_track_frame_with_rejection_equals_track_frame_then_host_ransac():
    ctx = _ctx("track")
    left0, _ = synth.stereo_pair(H, W, 3)
    left1, _ = synth.stereo_pair(H, W, 4)
    ref = ctx.detect_points(left0)
    f_off, i_off, s_off = ctx.track_frame(left1, ref_feat=ref)
    f_on, i_on, s_on = ctx.track_frame(left1, ref_feat=None, outlier_rejection=True)
    f_off2, i_off2, s_off2 = ctx.track_frame(left1, ref_feat=None)
    assert f_on.tobytes() == f_off.tobytes() and i_off2.tobytes() == i_off.tobytes() and s_off2.tobytes() == s_off.tobytes()
    hi, hs = ctx.fundamental_ransac(ref, f_off, i_off, s_off)
    diag("fransac_track_frame", matches=len(i_off), kept=len(i_on))
    assert len(i_off) >= 9 and hi.tobytes() == i_on.tobytes() and hs.tobytes() == s_on.tobytes()


@live
@pytest.mark.parametrize("matcher,seed", [(0, 4), (1, 4)])
def test_matching_points_with_rejection_equals_the_reference(tmp_path, matcher, seed):
    """the reference's MatchingPoints(f0, f1, matches, true) on the device's own scores == api.PointMatcher.MatchingPoints(..., outlier_rejection=True)"""
    sp = _ctx("sp")
    left, right = synth.stereo_pair(H, W, seed)
    f0, f1 = sp.detect_points(left), sp.detect_points(right)
    ctx = _ctx("sg" if matcher else "lg")
    pm = api.PointMatcher(ctx, W, H, matcher)
    cnt0, m0 = pm.MatchingPoints(np.asfortranarray(f0.T), np.asfortranarray(f1.T))
    cnt, matches = pm.MatchingPoints(np.asfortranarray(f0.T), np.asfortranarray(f1.T), outlier_rejection=True)
    n0 = api.PointMatcher.NormalizeKeypoints(np.asfortranarray(f0.T), W, H, 0.7 if matcher else 0.5)
    n1 = api.PointMatcher.NormalizeKeypoints(np.asfortranarray(f1.T), W, H, 0.7 if matcher else 0.5)
    if matcher:
        scores = ctx.superglue_scores(np.ascontiguousarray(n0.T), np.ascontiguousarray(n1.T))
    else:
        scores = ctx.lightglue_scores(np.ascontiguousarray(n0[1:].T), np.ascontiguousarray(n1[1:].T))
    ref_lib.set_engines({"superglue" if matcher else "lightglue": lambda ins: dict(scores=scores)})
    rpm = ref_lib.PointMatcher(str(tmp_path / "m"), matcher, W, H)
    rcnt0, q0, t0, _ = rpm.matching_points(f0, f1, False)
    rcnt, q, t, d = rpm.matching_points(f0, f1, True)
    rpm.close()
    diag(f"fransac_refpin_{matcher}_{seed}", before=cnt0, dev=cnt, ref=int(rcnt))
    assert rcnt0 == cnt0 and cnt0 >= 50 and rcnt == cnt
    np.testing.assert_array_equal(q, np.array([m[0] for m in matches], np.int32))
    np.testing.assert_array_equal(t, np.array([m[1] for m in matches], np.int32))
    np.testing.assert_allclose(d, np.array([m[2] for m in matches], np.float32), atol=2e-7, rtol=0)
    keep = fr.fransac(fr.points(f0, f1, np.stack([q0, t0], 1)))["mask"]                 # == "matcher list -> numpy RANSAC"
    np.testing.assert_array_equal(q, q0[keep])


def test_sequence_drivers_with_rejection_agree():
    """native driver == BatchedSequences == SequenceFrontEnd, byte for byte per frame, 3 sequences x 40 frames with scene cuts, rejection on"""
    import torch
    from test_gpu_seq import POLICY, _contexts, _frames, _summary
    S, N = 3, 40
    cfg = seq.KeyframeConfig(**POLICY)
    seqs = [_frames(N, 30 + s, 13) for s in range(S)]
    single, single_off = [], []
    kf, nf = _contexts(2)
    for s in range(S):
        fe = seq.SequenceFrontEnd(kf, nf, cfg, outlier_rejection=True)
        single.append([fe.step(l, r) for l, r in seqs[s]])
        fe = seq.SequenceFrontEnd(kf, nf, cfg)
        single_off.append([fe.step(l, r) for l, r in seqs[s]])
    kf.close(); nf.close()
    bad = {}
    for which in ("batched", "native"):
        kfb, nfb = _contexts(S)
        drv = (seq.BatchedSequences if which == "batched" else seq.NativeSequences)(kfb, nfb, S, cfg, outlier_rejection=True)
        for t in range(N):
            L = torch.from_numpy(np.stack([seqs[s][t][0] for s in range(S)])).cuda()
            R = torch.from_numpy(np.stack([seqs[s][t][1] for s in range(S)])).cuda()
            for s, r in enumerate(drv.step(L, R)):
                d = r.same_as(single[s][t])
                if d:
                    bad[(which, s, t)] = d
        if which == "native":
            drv.close()
        kfb.close(); nfb.close()
    on, off = [_summary(x) for x in single], [_summary(x) for x in single_off]
    diag("fransac_seq_on_vs_off", keyframes_on=sum(m["keyframes"] for m in on), keyframes_off=sum(m["keyframes"] for m in off),
         promoted_on=sum(m["promoted"] for m in on), promoted_off=sum(m["promoted"] for m in off),
         temporal_mean_on=float(np.mean([m["temporal_matches_mean"] for m in on])), temporal_mean_off=float(np.mean([m["temporal_matches_mean"] for m in off])))
    assert not bad, f"{len(bad)} results differ: {dict(list(bad.items())[:5])}"
