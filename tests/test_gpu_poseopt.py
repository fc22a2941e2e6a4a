"""Pose-only frame optimisation on the device (kernels_poseopt.hip; contract: include/airfe.h "Frame optimisation"): the one-call entry against the host
core (poseopt_core.h compiled for the host), the batch entry against the one-call entry at every batch size and position, the tracking composite
against its steps one at a time, on planted rows and on the matcher's own output."""
import numpy as np
import pytest

import pnp_ref as pr
import poseopt_ref as po
from test_poseopt_cpu import core, run_core  # noqa: F401  (the host core fixture)
from test_gpu_pnp import CAM as STEREO_CAM, _ctx
from airslam_amd import api, synth
from gpu_common import diag

pytestmark = pytest.mark.gpu
CAM = np.array(po.CAM_EUROC)
THR = np.array(po.THR_EUROC)
K = np.array(pr.K_EUROC)


def _problem(n, k):
    """(X, obs, Twc0): mixed inlier ratios, mono / half-stereo, identity and perturbed start poses"""
    if n == 0:
        return np.zeros((0, 3)), np.zeros((0, 3)), np.eye(4)
    X, obs, _, _, _ = po.planted_constraints(n, (1.0, 0.8, 0.5)[k % 3], seed=9000 + 13 * n + k, stereo=bool(k & 1))
    T0 = np.eye(4)
    if k % 4 >= 2:
        T0[:3, :3] = pr.rotation((0.3, -1.0, 0.5), 1.0 + k % 5)
        T0[:3, 3] = (0.02 * (k % 7), -0.05, 0.03)
    return X, obs, T0


def _batch(probs, ncap=1024):
    import torch
    B = len(probs)
    X = torch.zeros((B, ncap, 3), dtype=torch.float64); obs = torch.zeros((B, ncap, 3), dtype=torch.float64)
    n = torch.zeros(B, dtype=torch.int32); T0 = torch.zeros((B, 16), dtype=torch.float64)
    for b, (x, o, t0) in enumerate(probs):
        X[b, :len(x)] = torch.from_numpy(x); obs[b, :len(o)] = torch.from_numpy(o); n[b] = len(x); T0[b] = torch.from_numpy(t0.reshape(16))
    X, obs, n, T0 = X.cuda(), obs.cuda(), n.cuda(), T0.cuda()
    Twc = torch.full((B, 16), 7.0, dtype=torch.float64, device="cuda"); Rt = torch.full((B, 12), 7.0, dtype=torch.float64, device="cuda")
    mask = torch.full((B, ncap), 9, dtype=torch.uint8, device="cuda"); num = torch.full((B,), -5, dtype=torch.int32, device="cuda")
    _ctx().frame_optimize_batch_dev(X, obs, n, T0, CAM, THR, Twc, mask, num, Rt_t=Rt)
    torch.cuda.synchronize()
    out = []
    for b, (x, _, _) in enumerate(probs):
        m = mask[b].cpu().numpy()
        assert not m[len(x):].any()                              # (and no junk left: every slot was written)
        out.append(dict(Twc=Twc[b].cpu().numpy().reshape(4, 4), Rt=Rt[b].cpu().numpy(), inlier=m[:len(x)], num_inliers=int(num[b])))
    return out


def _same(a, b):
    assert a["num_inliers"] == b["num_inliers"]
    assert np.asarray(a["inlier"], np.uint8).tobytes() == np.asarray(b["inlier"], np.uint8).tobytes()
    assert np.asarray(a["Rt"], np.float64).tobytes() == np.asarray(b["Rt"], np.float64).tobytes()
    assert np.asarray(a["Twc"], np.float64).tobytes() == np.asarray(b["Twc"], np.float64).tobytes()


def test_one_call_entry_equals_the_host_core(core):  # noqa: F811
    ctx = _ctx()
    k = 0
    for n in (0, 10, 30, 100, 300, 1000, 1024):
        for ratio in (1.0, 0.8, 0.5):
            for stereo in (False, True):
                if n == 0:
                    X, obs = np.zeros((0, 3)), np.zeros((0, 3))
                else:
                    X, obs, _, _, _ = po.planted_constraints(n, ratio, seed=17 * n + int(10 * ratio), stereo=stereo)
                _same(ctx.frame_optimize(X, obs, CAM, THR, np.eye(4)), run_core(core, X, obs))
                k += 1
    # an extrinsic and a start pose that is not the identity; the Python restatement
    X, obs, T0 = _problem(200, 3)
    Tcb = np.concatenate([pr.rotation((0.2, -1.0, 0.4), 7.0).reshape(9), [0.05, -0.02, 0.1]])
    got = ctx.frame_optimize(X, obs, CAM, THR, T0, Tcb=Tcb)
    _same(got, run_core(core, X, obs, Twc0=T0, Tcb=Tcb))
    _same(got, po.frame_optimize(X, obs, Twc0=T0.reshape(16), Tcb=Tcb))
    # a start pose with NaN: the start pose comes back
    Tn = np.eye(4)
    Tn[1, 3] = np.nan
    got = ctx.frame_optimize(X, obs, CAM, THR, Tn)
    _same(got, run_core(core, X, obs, Twc0=Tn))
    assert got["num_inliers"] == 0 and got["Twc"].tobytes() == Tn.tobytes()
    diag("poseopt_one_call", problems=k + 2)


@pytest.mark.parametrize("B", [1, 7, 64])
def test_batch_entry_equals_the_one_call_entry(B):
    rng = np.random.default_rng(B)
    sizes = [0, 5, 10, 9, 1024] + rng.integers(0, 1025, max(B - 5, 0)).tolist()
    probs = [_problem(int(sizes[b % len(sizes)]), b) for b in range(B)]
    got = _batch(probs)
    ctx = _ctx()
    for (x, o, t0), g in zip(probs, got):
        _same(g, ctx.frame_optimize(x, o, CAM, THR, t0))
    diag(f"poseopt_batch_B{B}", problems=B, inliers=sum(g["num_inliers"] for g in got))


def test_a_problem_gives_the_same_bytes_alone_and_anywhere_in_a_batch():
    probs = [_problem([300, 1024, 10, 60][b % 4], 50 + b) for b in range(64)]
    full, again = _batch(probs), _batch(probs)
    rev = _batch(probs[::-1])
    for b in (0, 17, 63):
        alone = _batch([probs[b]])[0]
        _same(alone, full[b]); _same(alone, again[b]); _same(alone, rev[63 - b])


# ---- the composite -----------------------------------------------------------------------------------------------------------------------------------
def _composite(ctx, xyz_list, feat_list, tidx_list, lost, u_right_list=None, last_list=None, capK=1024, cap=1024, mcap=1024):
    import torch
    B = len(xyz_list)
    xyz = torch.full((B, capK, 3), float("nan"), dtype=torch.float64); feat = torch.zeros((B, cap, 259))
    ti = torch.zeros((B, mcap, 2), dtype=torch.int32); nt = torch.zeros(B, dtype=torch.int32)
    ur = None if u_right_list is None else torch.full((B, cap), -1.0, dtype=torch.float64)
    last = None if last_list is None else torch.zeros((B, 16), dtype=torch.float64)
    for b in range(B):
        xyz[b, :len(xyz_list[b])] = torch.from_numpy(xyz_list[b]); feat[b, :len(feat_list[b])] = torch.from_numpy(feat_list[b])
        ti[b, :len(tidx_list[b])] = torch.from_numpy(tidx_list[b]); nt[b] = len(tidx_list[b])
        if ur is not None:
            ur[b, :len(u_right_list[b])] = torch.from_numpy(u_right_list[b])
        if last is not None:
            last[b] = torch.from_numpy(last_list[b].reshape(16))
    xyz, feat, ti, nt = xyz.cuda(), feat.cuda(), ti.cuda(), nt.cuda()
    ur = None if ur is None else ur.cuda()
    last = None if last is None else last.cuda()
    Twc = torch.full((B, 16), 7.0, dtype=torch.float64, device="cuda"); Rt = torch.full((B, 12), 7.0, dtype=torch.float64, device="cuda")
    mask = torch.full((B, mcap), 9, dtype=torch.uint8, device="cuda"); num = torch.full((B,), -5, dtype=torch.int32, device="cuda")
    ok = torch.full((B,), -5, dtype=torch.int32, device="cuda"); pc = torch.full((B,), -5, dtype=torch.int32, device="cuda")
    ctx.track_pose_opt_batch_dev(CAM, THR, lost, xyz, feat, ti, nt, Twc, mask, num, ok, u_right_t=ur, Twc_last_t=last, Rt_t=Rt, pnp_count_t=pc)
    torch.cuda.synchronize()
    return [dict(Twc=Twc[b].cpu().numpy().reshape(4, 4), Rt=Rt[b].cpu().numpy(), inlier=mask[b, :len(tidx_list[b])].cpu().numpy(),
                 num_inliers=int(num[b]), ok=int(ok[b]), pnp_count=int(pc[b]), tail=mask[b, len(tidx_list[b]):].cpu().numpy()) for b in range(B)]


def _step_by_step(ctx, xyz, feat, tidx, lost, u_right=None, last=None):
    """PnP entry -> fallback -> gather -> airfe_frame_optimize, one step at a time"""
    has = np.array([0 <= r < len(xyz) and not np.isnan(xyz[r, 0]) for r in tidx[:, 0]], bool)
    sel = np.nonzero(has)[0]
    pnp = ctx.pnp_ransac(xyz[tidx[sel, 0]].astype(np.float32), feat[tidx[sel, 1], 1:3], K)
    last = np.eye(4) if last is None else last
    fell_back = po.use_last(pnp["Twc"], pnp["count"], last, lost)
    seed = last if fell_back else pnp["Twc"]
    obs = np.stack([feat[tidx[sel, 1], 1].astype(np.float64), feat[tidx[sel, 1], 2].astype(np.float64),
                    np.full(len(sel), -1.0) if u_right is None else u_right[tidx[sel, 1]]], 1).reshape(-1, 3)
    r = ctx.frame_optimize(xyz[tidx[sel, 0]], obs, CAM, THR, seed)
    ok = r["num_inliers"] > lost
    m = np.zeros(len(tidx), np.uint8)
    m[sel] = r["inlier"]
    if ok:
        Twc, Rt = r["Twc"], r["Rt"]
    else:                                                        # the seed stays; its Rcw, tcw come from an empty problem at the seed
        e = ctx.frame_optimize(np.zeros((0, 3)), np.zeros((0, 3)), CAM, THR, seed)
        Twc, Rt = e["Twc"], e["Rt"]
    return dict(Twc=Twc, Rt=Rt, inlier=m, num_inliers=r["num_inliers"], ok=int(ok), pnp_count=pnp["count"], fell_back=fell_back, pnp=pnp, sel=sel)


def _same_composite(g, w):
    _same(g, w)
    assert g["ok"] == w["ok"] and g["pnp_count"] == w["pnp_count"] and not g["tail"].any()


def _planted_rows(n, ratio, seed, missing=7):
    obj, img, R, t, truth = pr.planted(n, ratio, seed)
    xyz = obj.astype(np.float64)
    xyz[::missing] = np.nan                                      # keyframe points that do not exist: skipped, mask 0
    perm = np.random.default_rng(seed).permutation(n)
    feat = np.zeros((n, 259), np.float32)
    feat[perm, 1:3] = img                                         # current row perm[i] sees keyframe point i
    tidx = np.stack([np.arange(n), perm], 1).astype(np.int32)
    return xyz, feat, tidx, R, t, truth


def _sq_reprojection(Rt, xyz, feat, tidx, sel, keep):
    """the summed squared reprojection error at the pose Rt (Rcw, tcw) over the constraints `keep` of the gathered list `sel`, summed by the contract's
    own rule (64 partials in lane order: tests/poseopt_ref.py).  The PnP pose and the optimised pose minimise the same sum, so the two values agree
    to about one part in 1e15 and only ONE fixed summation can compare them: with numpy's pairwise sum, or in 80-bit arithmetic, the sign of the
    difference is rounding noise (-5e-15 ... +3e-14 on these three problems).  In the contract's arithmetic the comparison is exact: Levenberg-Marquardt
    takes a trial only when this very sum decreases, and 0.5 px of noise keeps every planted inlier in the quadratic part of the Huber kernel."""
    obs = np.stack([feat[tidx[sel, 1], 1], feat[tidx[sel, 1], 2], np.full(len(sel), -1.0)], 1).astype(np.float64)
    P = po._Problem(xyz[tidx[sel, 0]], obs, po.CAM_EUROC, None, po.THR_EUROC)
    chi2 = P.errors(list(Rt))[3]
    assert (chi2[keep] <= po.THR_EUROC[0]).all()
    return P.chi(list(Rt), ~keep)


def test_composite_equals_the_steps_and_recovers_planted_motion():
    ctx = _ctx()
    cases = [_planted_rows(n, 0.8, 900 + b) for b, n in enumerate((300, 100, 1000))]
    lost = 50
    got = _composite(ctx, [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], lost)
    for b, g in enumerate(got):
        xyz, feat, tidx, R, t, truth = cases[b]
        w = _step_by_step(ctx, xyz, feat, tidx, lost)
        _same_composite(g, w)
        assert not w["fell_back"] and g["ok"] == 1 and g["pnp_count"] >= lost
        rot, tr = pr.pose_errors(g["Rt"], R, t)
        kept = g["inlier"].astype(bool)
        has = ~np.isnan(xyz[:, 0])
        assert not kept[~has].any() and not (kept & ~truth).any()
        assert (kept & truth & has).sum() >= 0.99 * (truth & has).sum()
        assert g["num_inliers"] == kept.sum()
        assert rot <= 0.1 and tr <= 0.01 * np.linalg.norm(t) + 1e-3, (rot, tr)            # the CPU suite's gates for n >= 100
        # not worse than the PnP pose it started from, in summed squared reprojection error over the planted inliers
        keep = (truth & has)[tidx[w["sel"], 0]]
        start = po.frame_optimize(np.zeros((0, 3)), np.zeros((0, 3)), Twc0=w["pnp"]["Twc"].reshape(16))["Rt"]     # Rcw, tcw of the seed, as the optimiser forms them
        e_opt, e_pnp = _sq_reprojection(g["Rt"], xyz, feat, tidx, w["sel"], keep), _sq_reprojection(start, xyz, feat, tidx, w["sel"], keep)
        diag(f"poseopt_composite_{b}", rot_deg=rot, tr_m=tr, sq_err_opt=e_opt, sq_err_pnp=e_pnp, num_inliers=g["num_inliers"])
        assert e_opt <= e_pnp, (e_opt, e_pnp)


def test_composite_forced_into_the_fallback_equals_the_steps():
    """few correspondences and lost_num_match above the PnP count: the seed is the last tracked pose (here: a pose near the truth, and the identity)"""
    ctx = _ctx()
    cases = [_planted_rows(40, 0.9, 950 + b, missing=5) for b in range(3)]
    lasts = []
    for xyz, feat, tidx, R, t, truth in cases:
        T = np.eye(4)
        Rwc = (pr.rotation((0.1, 0.9, -0.3), 0.7) @ R).T
        T[:3, :3], T[:3, 3] = Rwc, -Rwc @ t + 0.01
        lasts.append(T)
    lasts[2] = np.eye(4)
    for lost, last_list in ((1000, lasts), (33, None)):
        got = _composite(ctx, [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], lost, last_list=last_list)
        for b, g in enumerate(got):
            xyz, feat, tidx, R, t, truth = cases[b]
            w = _step_by_step(ctx, xyz, feat, tidx, lost, last=None if last_list is None else last_list[b])
            _same_composite(g, w)
            if lost == 1000:
                assert w["fell_back"] and g["ok"] == 0                 # 32 constraints can never give more than 1000 inliers: the seed stays
                assert g["Twc"].tobytes() == last_list[b].tobytes()
            assert not g["inlier"][::5].any()


def test_composite_on_matcher_output_equals_the_steps():
    """a synthetic stereo keyframe and a tracked frame through the existing entries; the composite with the current frame as a keyframe (d_u_right from
    stereo_points_batch_dev on the current frame's own stereo list) and as a normal frame (all mono)"""
    import torch
    ctx = _ctx("track")
    left0, right0 = synth.stereo_pair(pr.H, pr.W, 3)
    left1, right1 = synth.stereo_pair(pr.H, pr.W, 4)
    fL, fR = ctx.detect_points(left0), ctx.detect_points(right0)
    pm = api.PointMatcher(ctx, pr.W, pr.H, 0)
    _, matches = pm.MatchingPoints(np.asfortranarray(fL.T), np.asfortranarray(fR.T))
    sidx = np.ascontiguousarray(np.array([(m[0], m[1]) for m in matches], np.int32).reshape(-1, 2))
    feat1, tidx, _ = ctx.track_frame(left1, ref_feat=fL)
    fR1 = ctx.detect_points(right1)
    _, matches1 = pm.MatchingPoints(np.asfortranarray(feat1.T), np.asfortranarray(fR1.T))
    sidx1 = np.ascontiguousarray(np.array([(m[0], m[1]) for m in matches1], np.int32).reshape(-1, 2))
    sp = ctx.stereo_points(STEREO_CAM, fL, fR, sidx)
    cap = 1024

    def dev_stereo(a, b, idx):
        fl = torch.zeros((1, cap, 259)); fr = torch.zeros((1, cap, 259)); ti = torch.zeros((1, cap, 2), dtype=torch.int32)
        fl[0, :len(a)] = torch.from_numpy(a); fr[0, :len(b)] = torch.from_numpy(b); ti[0, :len(idx)] = torch.from_numpy(idx)
        d = [x.cuda() for x in (fl, torch.tensor([len(a)], dtype=torch.int32), fr, torch.tensor([len(b)], dtype=torch.int32), ti,
                                torch.tensor([len(idx)], dtype=torch.int32))]
        u = torch.zeros((1, cap), dtype=torch.float64, device="cuda"); dp = torch.zeros_like(u)
        xyz = torch.zeros((1, cap, 3), dtype=torch.float64, device="cuda"); good = torch.zeros(1, dtype=torch.int32, device="cuda")
        ctx.stereo_points_batch_dev(STEREO_CAM, *d, u, dp, xyz, good)
        torch.cuda.synchronize()
        return u[0, :len(a)].cpu().numpy(), xyz[0, :len(a)].cpu().numpy()

    _, xyz0 = dev_stereo(fL, fR, sidx)
    u1, _ = dev_stereo(feat1, fR1, sidx1)
    assert xyz0.tobytes() == sp["xyz"].tobytes() and len(tidx) >= 8 and sp["good"] > 0
    for lost in (0, 50):
        for ur in (u1, None):
            got = _composite(ctx, [xyz0], [feat1], [tidx], lost, u_right_list=None if ur is None else [ur])[0]
            want = _step_by_step(ctx, sp["xyz"], feat1, tidx, lost, u_right=ur)
            diag("poseopt_matcher_composite", temporal=len(tidx), constraints=len(want["sel"]), stereo=0 if ur is None else int((ur[tidx[want["sel"], 1]] > 0).sum()),
                 pnp_count=got["pnp_count"], num_inliers=got["num_inliers"], ok=got["ok"], lost=lost)
            _same_composite(got, want)
