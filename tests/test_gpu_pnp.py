"""PnP RANSAC and stereo points on the device (kernels_pnp.hip; contract: include/airfe.h "PnP RANSAC", "Stereo points"): the one-call entry against
the host core (pnp_core.h compiled for the host), the batch entry against the one-call entry at every batch size and position, the stereo points
against tests/pnp_ref.py, the tracking composite on planted rows and on the matcher's own output."""
import ctypes as C

import numpy as np
import pytest

import pnp_ref as pr
from test_pnp_cpu import core, run_core  # noqa: F401  (the host core fixture)
from airslam_amd import _lib, api, synth, weights
from gpu_common import diag

pytestmark = pytest.mark.gpu
K = np.array(pr.K_EUROC)
CAM = np.array(pr.CAM_EUROC)
_C = {}


def _ctx(kind="plain"):
    if kind not in _C:
        if kind == "plain":
            _C[kind] = api.Context(lightglue=weights.synthetic_lightglue(1234), max_batch=1, max_keypoints=1024)
        else:
            _C[kind] = api.Context(superpoint=weights.synthetic_superpoint(1234), lightglue=weights.synthetic_lightglue(1234), max_batch=2, enc_chunk=2,
                                   max_keypoints=400, image_width=pr.W, image_height=pr.H)
    return _C[kind]


def _problem(n, k):
    if n == 0:
        return np.zeros((0, 3), np.float32), np.zeros((0, 2), np.float32)
    obj, img, _, _, _ = pr.planted(n, (1.0, 0.9, 0.6, 0.3)[k % 4], seed=7000 + 13 * n + k)
    return obj, img


def _batch(probs, ncap=1024):
    import torch
    B = len(probs)
    obj = torch.zeros((B, ncap, 3)); img = torch.zeros((B, ncap, 2)); n = torch.zeros(B, dtype=torch.int32)
    for b, (o, i) in enumerate(probs):
        obj[b, :len(o)] = torch.from_numpy(o); img[b, :len(i)] = torch.from_numpy(i); n[b] = len(o)
    obj, img, n = obj.cuda(), img.cuda(), n.cuda()
    Twc = torch.full((B, 16), 7.0, dtype=torch.float64, device="cuda"); Rt = torch.full((B, 12), 7.0, dtype=torch.float64, device="cuda")
    mask = torch.full((B, ncap), 9, dtype=torch.uint8, device="cuda"); cnt = torch.full((B,), -5, dtype=torch.int32, device="cuda")
    _ctx().pnp_ransac_batch_dev(obj, img, n, K, Twc, mask, cnt, Rt_t=Rt)
    torch.cuda.synchronize()
    out = []
    for b, (o, _) in enumerate(probs):
        m = mask[b].cpu().numpy()
        assert not m[len(o):].any()
        out.append(dict(Twc=Twc[b].cpu().numpy().reshape(4, 4), Rt=Rt[b].cpu().numpy(), inlier=m[:len(o)], count=int(cnt[b])))
    return out


def _same(a, b):
    assert a["count"] == b["count"]
    assert np.asarray(a["inlier"], np.uint8).tobytes() == np.asarray(b["inlier"], np.uint8).tobytes()
    assert np.asarray(a["Rt"], np.float64).tobytes() == np.asarray(b["Rt"], np.float64).tobytes()
    assert np.asarray(a["Twc"], np.float64).tobytes() == np.asarray(b["Twc"], np.float64).tobytes()


def test_one_call_entry_equals_the_host_core(core):  # noqa: F811
    ctx = _ctx()
    for n, k in ((0, 0), (7, 1), (8, 0), (12, 1), (30, 2), (100, 3), (300, 1), (1024, 2), (1000, 3)):
        obj, img = _problem(n, k)
        got = ctx.pnp_ransac(obj.astype(np.float64), img.astype(np.float64), K)
        want = run_core(core, obj, img)
        _same(got, want)
    obj, img, _, _, _ = pr.planted(120, 0.9, seed=21, planar=True)
    _same(ctx.pnp_ransac(obj, img, K), run_core(core, obj, img))
    obj, img = _problem(300, 2)
    ref = pr.pnp_ransac(obj, img)
    _same(ctx.pnp_ransac(obj, img, K), ref)


@pytest.mark.parametrize("B", [1, 7, 64])
def test_batch_entry_equals_the_one_call_entry(B):
    rng = np.random.default_rng(B)
    sizes = [0, 5, 8, 9, 1024] + rng.integers(0, 1025, max(B - 5, 0)).tolist()
    probs = [_problem(int(sizes[b % len(sizes)]), b) for b in range(B)]
    got = _batch(probs)
    ctx = _ctx()
    for (o, i), g in zip(probs, got):
        _same(g, ctx.pnp_ransac(o, i, K))
    diag(f"pnp_batch_B{B}", problems=B, models=sum(g["count"] > 0 for g in got))


def test_a_problem_gives_the_same_bytes_alone_and_anywhere_in_a_batch():
    probs = [_problem([300, 1024, 8, 60][b % 4], 50 + b) for b in range(64)]
    full, again = _batch(probs), _batch(probs)
    rev = _batch(probs[::-1])
    for b in (0, 17, 63):
        alone = _batch([probs[b]])[0]
        _same(alone, full[b]); _same(alone, again[b]); _same(alone, rev[63 - b])


def _stereo_case(n, seed):
    fL, fR, idx, X = pr.stereo_rows(n, seed)
    idx = np.concatenate([idx, idx[:10][:, ::-1], idx[5:9]])
    idx[-4:, 1] = idx[:4, 1]
    return fL, fR, np.ascontiguousarray(idx[:1024], np.int32), X


def test_stereo_points_equal_the_restatement_and_the_seq_count():
    import torch
    ctx = _ctx()
    cases = [_stereo_case(n, s) for n, s in ((300, 1), (1000, 2), (10, 3), (600, 4))]
    lib = _lib.lib()
    p = _lib.SeqPolicy()
    lib.airfe_seq_default_policy(C.byref(p))
    differ = 0
    for fL, fR, idx, _ in cases:
        ref = pr.stereo_points(fL, fR, idx)
        got = ctx.stereo_points(CAM, fL, fR, idx)
        for k in ("u_right", "depth", "xyz"):
            assert got[k].tobytes() == ref[k].tobytes(), k
        assert got["good"] == ref["good"] == lib.airfe_seq_good_stereo_points(C.byref(p), fL.ctypes.data, fR.ctypes.data, idx.ctypes.data, len(idx))
        s = ref["depth"] > 0
        differ += int((ref["xyz"][s, 2] != ref["depth"][s]).sum())
    assert differ > 0                       # the float-parallax depth and the double-difference point are told apart
    B, cap, mcap = len(cases), 1024, 1024
    fl = torch.zeros((B, cap, 259)); fr = torch.zeros((B, cap, 259)); ti = torch.zeros((B, mcap, 2), dtype=torch.int32)
    nl = torch.zeros(B, dtype=torch.int32); nr = torch.zeros(B, dtype=torch.int32); nm = torch.zeros(B, dtype=torch.int32)
    for b, (fL, fR, idx, _) in enumerate(cases):
        fl[b, :len(fL)] = torch.from_numpy(fL); fr[b, :len(fR)] = torch.from_numpy(fR); ti[b, :len(idx)] = torch.from_numpy(idx)
        nl[b], nr[b], nm[b] = len(fL), len(fR), len(idx)
    d = [x.cuda() for x in (fl, nl, fr, nr, ti, nm)]
    u = torch.zeros((B, cap), dtype=torch.float64, device="cuda"); dp = torch.zeros_like(u)
    xyz = torch.zeros((B, cap, 3), dtype=torch.float64, device="cuda"); good = torch.zeros(B, dtype=torch.int32, device="cuda")
    ctx.stereo_points_batch_dev(CAM, *d, u, dp, xyz, good)
    torch.cuda.synchronize()
    for b, (fL, fR, idx, _) in enumerate(cases):
        ref = pr.stereo_points(fL, fR, idx)
        n = len(fL)
        assert u[b, :n].cpu().numpy().tobytes() == ref["u_right"].tobytes()
        assert dp[b, :n].cpu().numpy().tobytes() == ref["depth"].tobytes()
        assert xyz[b, :n].cpu().numpy().tobytes() == ref["xyz"].tobytes()
        assert int(good[b]) == ref["good"]
        assert (u[b, n:] == -1).all() and torch.isnan(xyz[b, n:]).all()


def _composite(ctx, xyz_list, feat_list, tidx_list, capK=1024, cap=1024, mcap=1024):
    import torch
    B = len(xyz_list)
    xyz = torch.full((B, capK, 3), float("nan"), dtype=torch.float64); feat = torch.zeros((B, cap, 259))
    ti = torch.zeros((B, mcap, 2), dtype=torch.int32); nt = torch.zeros(B, dtype=torch.int32)
    for b in range(B):
        xyz[b, :len(xyz_list[b])] = torch.from_numpy(xyz_list[b]); feat[b, :len(feat_list[b])] = torch.from_numpy(feat_list[b])
        ti[b, :len(tidx_list[b])] = torch.from_numpy(tidx_list[b]); nt[b] = len(tidx_list[b])
    xyz, feat, ti, nt = xyz.cuda(), feat.cuda(), ti.cuda(), nt.cuda()
    Twc = torch.zeros((B, 16), dtype=torch.float64, device="cuda"); Rt = torch.zeros((B, 12), dtype=torch.float64, device="cuda")
    mask = torch.full((B, mcap), 9, dtype=torch.uint8, device="cuda"); cnt = torch.zeros(B, dtype=torch.int32, device="cuda")
    ctx.track_pose_batch_dev(K, xyz, feat, ti, nt, Twc, mask, cnt, Rt_t=Rt)
    torch.cuda.synchronize()
    return [dict(Twc=Twc[b].cpu().numpy().reshape(4, 4), Rt=Rt[b].cpu().numpy(), inlier=mask[b, :len(tidx_list[b])].cpu().numpy(), count=int(cnt[b]),
                 tail=mask[b, len(tidx_list[b]):].cpu().numpy()) for b in range(B)]


def _step_by_step(ctx, xyz, feat, tidx):
    ok = np.array([0 <= r < len(xyz) and not np.isnan(xyz[r, 0]) for r in tidx[:, 0]], bool)
    sel = np.nonzero(ok)[0]
    r = ctx.pnp_ransac(xyz[tidx[sel, 0]].astype(np.float32), feat[tidx[sel, 1], 1:3], K)
    m = np.zeros(len(tidx), np.uint8)
    m[sel] = r["inlier"]
    return dict(Twc=r["Twc"], Rt=r["Rt"], inlier=m, count=r["count"])


def test_composite_recovers_planted_motion():
    ctx = _ctx()
    xyzs, feats, tidxs, truths = [], [], [], []
    for b, n in enumerate((300, 100, 1000)):
        obj, img, R, t, truth = pr.planted(n, 0.8, seed=900 + b)
        xyz = obj.astype(np.float64)
        xyz[::7] = np.nan                                         # keyframe points that do not exist: skipped, mask 0
        rng = np.random.default_rng(b)
        perm = rng.permutation(n)
        feat = np.zeros((n, 259), np.float32)
        feat[perm, 1:3] = img                                     # current row perm[i] sees keyframe point i
        tidx = np.stack([np.arange(n), perm], 1).astype(np.int32)
        xyzs.append(xyz); feats.append(feat); tidxs.append(tidx); truths.append((R, t, truth))
    got = _composite(ctx, xyzs, feats, tidxs)
    for b, g in enumerate(got):
        R, t, truth = truths[b]
        rot, tr = pr.pose_errors(g["Rt"], R, t)
        kept = g["inlier"].astype(bool)
        assert not kept[::7].any() and not (kept & ~truth).any() and not g["tail"].any()
        has = ~np.isnan(xyzs[b][:, 0])
        assert (kept & truth & has).sum() >= 0.99 * (truth & has).sum()
        assert rot <= 0.1 and tr <= 0.01 * np.linalg.norm(t) + 1e-3, (rot, tr)            # the CPU suite's gates for n >= 100
        _same(g, _step_by_step(ctx, xyzs[b], feats[b], tidxs[b]))


def test_composite_on_matcher_output_equals_the_steps():
    """a synthetic stereo keyframe and a tracked frame through the existing entries, then stereo points + the composite == stereo_points + gather +
    pnp_ransac one step at a time"""
    import torch
    ctx = _ctx("track")
    left0, right0 = synth.stereo_pair(pr.H, pr.W, 3)
    left1, _ = synth.stereo_pair(pr.H, pr.W, 4)
    fL, fR = ctx.detect_points(left0), ctx.detect_points(right0)
    _, matches = api.PointMatcher(ctx, pr.W, pr.H, 0).MatchingPoints(np.asfortranarray(fL.T), np.asfortranarray(fR.T))
    sidx = np.ascontiguousarray(np.array([(m[0], m[1]) for m in matches], np.int32).reshape(-1, 2))
    feat1, tidx, _ = ctx.track_frame(left1, ref_feat=fL)
    sp = ctx.stereo_points(CAM, fL, fR, sidx)
    cap = 1024
    fl = torch.zeros((1, cap, 259)); fr = torch.zeros((1, cap, 259)); ti = torch.zeros((1, cap, 2), dtype=torch.int32)
    fl[0, :len(fL)] = torch.from_numpy(fL); fr[0, :len(fR)] = torch.from_numpy(fR); ti[0, :len(sidx)] = torch.from_numpy(sidx)
    d = [x.cuda() for x in (fl, torch.tensor([len(fL)], dtype=torch.int32), fr, torch.tensor([len(fR)], dtype=torch.int32), ti,
                            torch.tensor([len(sidx)], dtype=torch.int32))]
    u = torch.zeros((1, cap), dtype=torch.float64, device="cuda"); dp = torch.zeros_like(u)
    xyz = torch.zeros((1, cap, 3), dtype=torch.float64, device="cuda"); good = torch.zeros(1, dtype=torch.int32, device="cuda")
    ctx.stereo_points_batch_dev(CAM, *d, u, dp, xyz, good)
    torch.cuda.synchronize()
    assert xyz[0, :len(fL)].cpu().numpy().tobytes() == sp["xyz"].tobytes() and int(good[0]) == sp["good"]
    got = _composite(ctx, [xyz[0, :len(fL)].cpu().numpy()], [feat1], [tidx])[0]
    want = _step_by_step(ctx, sp["xyz"], feat1, tidx)
    diag("pnp_matcher_composite", stereo=len(sidx), good=sp["good"], temporal=len(tidx), count=got["count"])
    assert len(tidx) >= 8 and sp["good"] > 0
    _same(got, want)
