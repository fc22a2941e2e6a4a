"""Relocalisation to the pose on the device (include/airfe.h "Map state in the database", "Grouping", "Relocalisation composite"): the grouping kernel
against tests/bowgroup_ref.py on the cases tests/test_bowgroup_cpu.py pins the host core to (so kernel == host core == restatement, bit for bit); the map
tables' round trips and refusals; the composite against the steps done by hand through the existing entries, byte for byte; every stage's failure."""
import numpy as np
import pytest

import bowgroup_cases as bc
import bowgroup_ref as gr
import pnp_ref as pr
import poseopt_ref as po
from airslam_amd import weights
from planted import features, planted_pair

pytestmark = pytest.mark.gpu
CAP = 400
PLANTED = (380, 360)         # keypoints of query 0 and of every revisit: about half of the smaller count come back as matches
CAM = np.array(po.CAM_EUROC)
THR = np.array(po.THR_EUROC)
MIN_INLIER = 20
_S = {}


def _ctx():
    """one context for the file: LightGlue for the composite (16 pairs), the 10^4-word vocabulary"""
    if "ctx" not in _S:
        from airslam_amd import api
        c = api.Context(lightglue=weights.synthetic_lightglue(1234), max_batch=16, max_keypoints=CAP)
        c.bow_load(weights.synthetic_vocabulary(1234, k=10, L=4))
        _S["ctx"] = c
    return _S["ctx"]


def _empty_db(N, cap, edges):
    """N frames without words or features (the grouping reads neither) + the map tables"""
    import torch
    from airslam_amd import api
    db = api.BowDatabase(_ctx(), N, cap, keep_features=True)
    db.add_batch_dev(torch.zeros((N, cap), dtype=torch.int32, device="cuda"), torch.zeros((N, cap), dtype=torch.float64, device="cuda"),
                     torch.zeros(N, dtype=torch.int32, device="cuda"), torch.zeros((N, cap, 259), dtype=torch.float32, device="cuda"),
                     torch.zeros(N, dtype=torch.int32, device="cuda"))
    db.attach_map(edges)
    return db


def _group_dev(db, mode, K, lists, ccap, extra=None, qpos=None, max_dist=None, ncand=None):
    """lists: per query [(frame, score)] -> per query dict(frames, scores, ngroups, status) of one group_dev call"""
    import torch
    Q = len(lists)
    cf, sc = np.full((Q, ccap), -7, np.int32), np.full((Q, ccap), np.nan)
    nc = np.array([len(l) for l in lists] if ncand is None else ncand, np.int32)
    for q, l in enumerate(lists):
        cf[q, :len(l)], sc[q, :len(l)] = [f for f, _ in l], [s for _, s in l]
    gf = torch.full((Q, K), -9, dtype=torch.int32, device="cuda")
    gs = torch.full((Q, K), float("nan"), dtype=torch.float64, device="cuda")
    ng = torch.full((Q,), -9, dtype=torch.int32, device="cuda")
    st = torch.full((Q,), -9, dtype=torch.int32, device="cuda")
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    db.group_dev(mode, up(cf), up(sc), up(nc), gf, gs, ng, st, extra_t=up(extra), qpos_t=up(qpos), max_dist_t=up(max_dist))
    torch.cuda.synchronize()
    gf, gs, ng, st = gf.cpu().numpy(), gs.cpu().numpy(), ng.cpu().numpy(), st.cpu().numpy()
    return [dict(frames=gf[q].tolist(), scores=gs[q].tolist(), ngroups=int(ng[q]), status=int(st[q])) for q in range(Q)]


def _same(a, b):
    return (a["status"] == b["status"] and a["ngroups"] == b["ngroups"] and list(a["frames"]) == list(b["frames"]) and
            np.array(a["scores"], np.float64).tobytes() == np.array(b["scores"], np.float64).tobytes())


def test_grouping_kernel_equals_the_restatement_bit_for_bit():
    """every shared case as query 0 of a call of Q = 1 and of Q = 5; the other four queries of the batch are the same list cut in half, emptied, without its
    last entry, and with its scores reversed — each against the restatement"""
    NMAX = 300
    db = _empty_db(NMAX, 8, 8192)
    cases = bc.all_cases()
    assert any(len(c["cands"]) == 130 and c["N"] == 200 for c in cases)
    for c in cases:
        db.set_covisibility(c["row_ptr"], c["nbr"], c["weight"])
        pos = np.zeros((NMAX, 3))
        pos[:c["N"]] = c["positions"]
        db.set_positions(0, pos)
        l0 = c["cands"]
        rev = [(f, s) for (f, _), (_, s) in zip(l0, l0[::-1])]
        lists = [l0, l0[:len(l0) // 2], [], l0[:-1], rev]
        ncand = [c["ncand"]] + [len(l) for l in lists[1:]]
        extra = None
        if c["extra"] is not None:
            extra = np.zeros((5, NMAX))
            extra[:, :c["N"]] = c["extra"]
        loop = c["mode"] == gr.LOOP
        qpos = np.tile(c["qpos"], (5, 1)) if loop else None
        md = np.full(5, c["max_dist"]) if loop else None
        want = [bc.reference(dict(c, cands=l, ncand=n)) for l, n in zip(lists, ncand)]
        got5 = _group_dev(db, c["mode"], c["K"], lists, c["ccap"], extra, qpos, md, ncand)
        got1 = _group_dev(db, c["mode"], c["K"], lists[:1], c["ccap"], None if extra is None else extra[:1], None if qpos is None else qpos[:1],
                          None if md is None else md[:1], ncand[:1])
        for q in range(5):
            assert _same(got5[q], want[q]), (c["name"], q, got5[q], want[q])
        assert _same(got1[0], got5[0]), c["name"]                       # the same bytes alone and inside the batch
    db.close()


def test_map_tables_round_trip_and_refusals():
    import torch
    from airslam_amd import api
    db = _empty_db(6, 8, 32)
    assert np.isnan(db.get_points(0, 6)).all()                          # initialised to NaN: no map point anywhere
    rng = np.random.default_rng(3)
    xyz = rng.normal(size=(2, 8, 3))
    xyz[0, 3] = np.nan
    db.set_points(2, xyz)
    db.set_points_dev(4, torch.from_numpy(xyz[::-1].copy()).cuda())
    torch.cuda.synchronize()
    back = db.get_points(0, 6)
    assert back[2:4].tobytes() == xyz.tobytes() and back[4:6].tobytes() == xyz[::-1].tobytes() and np.isnan(back[:2]).all()
    row_ptr, nbr, weight = bc.csr(4, {0: [(0, 12), (2, 3)], 2: [(0, 3), (2, 40), (5, 11)]})
    db.set_covisibility(row_ptr, nbr, weight)
    r, n, w = db.get_covisibility(32)
    assert r.tolist() == row_ptr.tolist() + [len(nbr)] * 2 and n.tolist() == nbr.tolist() and w.tolist() == weight.tolist()
    for bad in ([0, 2, 1], [2, 2, 0]):                                  # descending, and a repeated neighbour: refused, nothing changed
        with pytest.raises(api.AirfeError):
            db.set_covisibility(np.array([0, 3], np.int32), np.array(bad, np.int32), np.array([11, 12, 13], np.int32))
    with pytest.raises(api.AirfeError):                                 # more entries than max_edges
        db.set_covisibility(np.array([0, 33], np.int32), np.arange(33, dtype=np.int32), np.ones(33, np.int32))
    with pytest.raises(api.AirfeError):                                 # frames beyond max_frames
        db.set_points(5, xyz)
    r, n, w = db.get_covisibility(32)
    assert r.tolist() == row_ptr.tolist() + [len(nbr)] * 2 and n.tolist() == nbr.tolist() and w.tolist() == weight.tolist()
    assert db.get_points(0, 6).tobytes() == back.tobytes()
    db.close()
    # without attach_map the grouping and the composite are return codes
    plain = api.BowDatabase(_ctx(), 4, CAP, keep_features=True)
    out = _reloc_buffers(1)
    with pytest.raises(api.AirfeError):
        plain.relocalize_batch_dev(torch.zeros((1, CAP, 259), dtype=torch.float32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"), CAM, THR,
                                   MIN_INLIER, *[out[k] for k in ("ok", "stage", "Twc", "best", "num", "mask", "idx", "score", "nmatch")])
    with pytest.raises(api.AirfeError):
        _group_dev(plain, gr.RELOC, 3, [[(0, 0.5)]], 4)
    with pytest.raises(api.AirfeError):                                 # needs keep_features
        api.BowDatabase(_ctx(), 4, CAP).attach_map(8)
    plain.close()


# ---- the composite ---------------------------------------------------------------------------------------------------------------------------------
def _scene():
    """Q = 4 queries against N = 12 stored frames; stored frame 2 q + 1 is query q's revisit (tests/planted.py: rows 0 .. k - 1 correspond).  The revisit's
    planted rows carry X = Twc_true . backproject(the QUERY row's pixel, depth ~ U(2, 10)) for a planted motion (Xc = R X + t); 20 % of them an unrelated
    point (one that projects 60-200 px away, at another depth), 10 % NaN; its other rows NaN.  Every other frame: points in front of no particular camera."""
    if "scene" in _S:
        return _S["scene"]
    Q, N = 4, 12
    fx, fy, cx, cy = CAM[:4]
    qf, dbf = np.zeros((Q, CAP, 259), np.float32), np.zeros((N, CAP, 259), np.float32)
    qn, dn = np.zeros(Q, np.int32), np.zeros(N, np.int32)
    rng = np.random.default_rng(2024)
    xyz = np.full((N, CAP, 3), np.nan)
    for f in range(N):
        k = 300 + 5 * f
        dbf[f, :k], dn[f] = features(k, 900 + f), k
        xyz[f, :k] = rng.uniform(-5, 5, (k, 3)) + (0, 0, 8)
    motions, kinds = [], []
    for q in range(Q):
        a, b = planted_pair(PLANTED[0] - 20 * q, PLANTED[1], 70 + 10 * q)
        qf[q, :len(a)], qn[q] = a, len(a)
        f = 2 * q + 1
        dbf[f], dn[f] = 0, len(b)
        dbf[f, :len(b)] = b
        k = min(len(a), len(b)) // 2
        R, t = pr.planted_motion(rng)
        z = rng.uniform(2.0, 10.0, k)
        u, v = a[:k, 1].astype(np.float64), a[:k, 2].astype(np.float64)
        kind = rng.choice(3, k, p=(0.7, 0.2, 0.1))                      # 0 true, 1 unrelated, 2 none
        d = rng.normal(size=(k, 2))
        d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(60.0, 200.0, (k, 1)) * (kind == 1)[:, None]
        z = np.where(kind == 1, rng.uniform(2.0, 10.0, k), z)
        Xc = np.stack([(u + d[:, 0] - cx) / fx * z, (v + d[:, 1] - cy) / fy * z, z], 1)
        X = (Xc - t) @ R                                                # Xw = R^T (Xc - t)
        X[kind == 2] = np.nan
        xyz[f] = np.nan
        xyz[f, :k] = X
        motions.append((R, t))
        kinds.append(kind)
    _S["scene"] = dict(Q=Q, N=N, qf=qf, qn=qn, dbf=dbf, dn=dn, xyz=xyz, motions=motions, kinds=kinds)
    return _S["scene"]


def _scene_db():
    """the scene's frames through bow_vector_batch_dev into a database with its map points and a covisibility that links each revisit to its neighbours"""
    import torch
    from airslam_amd import api
    s = _scene()
    ctx, N = _ctx(), s["N"]
    ft, nt = torch.from_numpy(s["dbf"]).cuda(), torch.from_numpy(s["dn"]).cuda()
    ids = torch.zeros((N, CAP), dtype=torch.int32, device="cuda")
    vals = torch.zeros((N, CAP), dtype=torch.float64, device="cuda")
    nw = torch.zeros((N,), dtype=torch.int32, device="cuda")
    ctx.bow_vector_batch_dev(ft, nt, ids, vals, nw)
    db = api.BowDatabase(ctx, N, CAP, keep_features=True)
    db.add_batch_dev(ids, vals, nw, ft, nt)
    db.attach_map(64)
    db.set_points(0, s["xyz"])
    rows = {f: [(f, 30)] + [(g, 15) for g in (f - 1, f + 1) if 0 <= g < N] for f in range(N)}
    db.set_covisibility(*bc.csr(N, rows))
    torch.cuda.synchronize()
    return db


def _reloc_buffers(Q):
    import torch
    t = lambda shape, dt, fill: torch.full(shape, fill, dtype=dt, device="cuda")  # noqa: E731
    return dict(ok=t((Q,), torch.int32, -9), stage=t((Q,), torch.int32, -9), Twc=t((Q, 16), torch.float64, float("nan")), best=t((Q,), torch.int32, -9),
                num=t((Q,), torch.int32, -9), mask=t((Q, CAP), torch.uint8, 7), idx=t((Q, CAP, 2), torch.int32, -9), score=t((Q, CAP), torch.float32, float("nan")),
                nmatch=t((Q,), torch.int32, -9), pnp_count=t((Q,), torch.int32, -9))


def _composite(db, qf, qn, refine, min_inlier=MIN_INLIER, extra=None):
    import torch
    Q = qf.shape[0]
    o = _reloc_buffers(Q)
    db.relocalize_batch_dev(torch.from_numpy(qf).cuda(), torch.from_numpy(qn).cuda(), CAM, THR, min_inlier, o["ok"], o["stage"], o["Twc"], o["best"], o["num"],
                            o["mask"], o["idx"], o["score"], o["nmatch"], pnp_count_t=o["pnp_count"], extra_t=None if extra is None else torch.from_numpy(extra).cuda(),
                            pose_refinement=refine)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def _by_hand(db, qf, qn, xyz, refine, min_inlier=MIN_INLIER, extra=None):
    """the same chain through the existing entries + group_dev, with a numpy gather"""
    import torch
    ctx, Q, N = _ctx(), qf.shape[0], db.size
    i32 = lambda shape, fill=0: torch.full(shape, fill, dtype=torch.int32, device="cuda")  # noqa: E731
    f64 = lambda shape: torch.zeros(shape, dtype=torch.float64, device="cuda")  # noqa: E731
    qt, qnt = torch.from_numpy(qf).cuda(), torch.from_numpy(qn).cuda()
    ids, vals, nw = i32((Q, CAP)), f64((Q, CAP)), i32((Q,))
    ctx.bow_vector_batch_dev(qt, qnt, ids, vals, nw)
    cf, cs, sc, nc, ms = i32((Q, N)), i32((Q, N)), f64((Q, N)), i32((Q,)), i32((Q,))
    db.query_batch_dev(ids, vals, nw, cf, cs, sc, nc, ms, ratio=0.3)
    gf, gs, ng, gst = i32((Q, 3)), f64((Q, 3)), i32((Q,)), i32((Q,))
    db.group_dev(gr.RELOC, cf, sc, nc, gf, gs, ng, gst, extra_t=None if extra is None else torch.from_numpy(extra).cuda())
    best, idx, msc, nm = i32((Q,)), i32((Q, CAP, 2), -9), torch.full((Q, CAP), float("nan"), dtype=torch.float32, device="cuda"), i32((Q,))
    db.match_candidates_batch_dev(qt, qnt, gf, best, idx, msc, nm, None, outlier_rejection=True)
    torch.cuda.synchronize()
    h = dict(best=best.cpu().numpy(), idx=idx.cpu().numpy(), score=msc.cpu().numpy(), nmatch=nm.cpu().numpy(), ncand=nc.cpu().numpy(),
             groups=gf.cpu().numpy(), gstatus=gst.cpu().numpy(), ngroups=ng.cpu().numpy())
    obj, img = np.zeros((Q, CAP, 3), np.float32), np.zeros((Q, CAP, 2), np.float32)
    X, obs = np.zeros((Q, CAP, 3)), np.zeros((Q, CAP, 3))
    n, pre, maps = np.zeros(Q, np.int32), np.zeros(Q, np.int32), []
    for q in range(Q):
        m, b = int(h["nmatch"][q]), int(h["best"][q])
        pre[q] = 1 if h["ncand"][q] <= 0 else 2 if (h["gstatus"][q] != 0 or h["ngroups"][q] <= 0) else 3 if (b < 0 or m < min_inlier) else 0
        keep = []
        if not pre[q]:
            li = h["idx"][q, :m]
            keep = [j for j in range(m) if not np.isnan(xyz[b, li[j, 1], 0])]
            k = len(keep)
            P = xyz[b, li[keep, 1]]
            uv = qf[q, li[keep, 0], 1:3]
            obj[q, :k], img[q, :k], X[q, :k] = P.astype(np.float32), uv, P
            obs[q, :k, :2], obs[q, :k, 2] = uv.astype(np.float64), -1.0
            n[q] = k
            if refine and k < min_inlier:
                pre[q] = 4
        maps.append(keep)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    Twc, inl, cnt = f64((Q, 16)), torch.zeros((Q, CAP), dtype=torch.uint8, device="cuda"), i32((Q,))
    ctx.pnp_ransac_batch_dev(up(obj), up(img), up(n), CAM[:4], Twc, inl, cnt)
    torch.cuda.synchronize()
    h["pnp_count"] = cnt.cpu().numpy()
    num = h["pnp_count"].copy()
    if refine:
        n_opt = np.where(pre == 0, n, 0).astype(np.int32)
        T2, inl2, num2 = f64((Q, 16)), torch.zeros((Q, CAP), dtype=torch.uint8, device="cuda"), i32((Q,))
        ctx.frame_optimize_batch_dev(up(X), up(obs), up(n_opt), Twc, CAM, THR, T2, inl2, num2)
        torch.cuda.synchronize()
        Twc, inl, num = T2, inl2, num2.cpu().numpy()
        n = n_opt
    flags = inl.cpu().numpy()
    mask = np.zeros((Q, CAP), np.uint8)
    for q in range(Q):
        for i, j in enumerate(maps[q][:n[q]]):
            mask[q, j] = flags[q, i]
    stage = np.where(pre != 0, pre, np.where(num < min_inlier, 5, 0)).astype(np.int32)
    h.update(Twc=Twc.cpu().numpy(), mask=mask, num=num.astype(np.int32), stage=stage, ok=(stage == 0).astype(np.int32))
    return h


def _assert_equal(got, want, Q, who):
    for k in ("ok", "stage", "best", "nmatch", "num", "pnp_count"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{who}: {k}")
    for q in range(Q):
        m = int(want["nmatch"][q])
        assert got["idx"][q, :m].tobytes() == want["idx"][q, :m].tobytes() and got["score"][q, :m].tobytes() == want["score"][q, :m].tobytes(), (who, q)
        assert (got["idx"][q, m:] == -9).all(), (who, q)
        assert got["mask"][q].tobytes() == want["mask"][q].tobytes(), (who, q)
        assert got["Twc"][q].tobytes() == want["Twc"][q].tobytes(), (who, q, got["Twc"][q], want["Twc"][q])


def _key(o, q):
    m = int(o["nmatch"][q])
    return tuple(o[k][q].tobytes() for k in ("ok", "stage", "best", "nmatch", "num", "pnp_count", "mask", "Twc")) + (o["idx"][q, :m].tobytes(), o["score"][q, :m].tobytes())


@pytest.mark.parametrize("refine", [True, False])
def test_composite_equals_the_steps_done_by_hand(refine):
    s = _scene()
    db = _scene_db()
    Q = s["Q"]
    got = _composite(db, s["qf"], s["qn"], refine)
    want = _by_hand(db, s["qf"], s["qn"], s["xyz"], refine)
    _assert_equal(got, want, Q, f"refine={refine}")
    assert got["best"].tolist() == [1, 3, 5, 7] and got["stage"].tolist() == [0] * 4 and got["ok"].tolist() == [1] * 4
    for q in range(Q):
        R, t = s["motions"][q]
        T = got["Twc"][q].reshape(4, 4)
        Rcw = T[:3, :3].T
        rot, tr = pr.pose_errors(np.concatenate([Rcw.reshape(9), -Rcw @ T[:3, 3]]), R, t)
        print(f"refine={refine} q={q}: nmatch {got['nmatch'][q]} pnp {got['pnp_count'][q]} num {got['num'][q]} rot {rot:.3g} deg, trans {tr:.3g} m")
        assert rot <= 0.1 and tr <= 0.01 * np.linalg.norm(t) + 1e-3, (q, rot, tr)      # the gate of test_pnp_cpu.py::test_planted_motion_is_recovered, n >= 100
        m = int(got["nmatch"][q])
        assert m >= 100 and got["num"][q] >= MIN_INLIER
        li, k = got["idx"][q, :m], len(s["kinds"][q])
        planted = (li[:, 0] == li[:, 1]) & (li[:, 1] < k)
        unrelated = np.array([li[j, 1] < k and s["kinds"][q][li[j, 1]] == 1 for j in range(m)])
        assert unrelated.sum() >= 10 and not (got["mask"][q, :m].astype(bool) & unrelated).any()          # no unrelated-point row is an inlier
        assert (got["mask"][q, :m].astype(bool) & planted).sum() >= MIN_INLIER
    # a query's bytes are the same alone and in the batch of 4
    for q in (0, 3):
        one = _composite(db, s["qf"][q:q + 1], s["qn"][q:q + 1], refine)
        assert _key(one, 0) == _key(got, q), q
    db.close()


def test_composite_with_lists_longer_than_one_round_of_the_gather(monkeypatch):
    """The scene at capacity 640 with 620 .. 560 x 600 keypoints: the winners' lists hold close to 300 entries, so reloc_gather_kernel walks them in two rounds
    of 256 with a running base and its last round ends inside a wave.  (Three rounds would need more than 512 entries: the planted recipe gives at most half of
    max_keypoints <= 1024.)"""
    import sys
    me = sys.modules[__name__]
    monkeypatch.setattr(me, "CAP", 640)
    monkeypatch.setattr(me, "PLANTED", (620, 600))
    monkeypatch.setattr(me, "_S", {})
    s = _scene()
    db = _scene_db()
    got = _composite(db, s["qf"], s["qn"], True)
    _assert_equal(got, _by_hand(db, s["qf"], s["qn"], s["xyz"], True), s["Q"], "long lists")
    print("nmatch", got["nmatch"].tolist(), "pnp", got["pnp_count"].tolist())
    assert (got["nmatch"] > 256).all() and (got["nmatch"] % 64 != 0).all() and got["stage"].tolist() == [0] * 4 and (got["pnp_count"] > 128).all()
    db.close()


def test_every_stage_fails_where_it_should():
    """One query of each kind.  Stage 2 (best_group_score < 0) cannot be reached through the query: L1 scores are never negative, so a candidate list always
    stores a group; it is covered through group_dev alone (the shared case "negative" and the empty lists of the grouping test: status 1)."""
    s = _scene()
    db = _scene_db()
    Q, eye = s["Q"], np.eye(4).reshape(16)
    xyz = s["xyz"].copy()
    rng = np.random.default_rng(5)
    xyz[5] = np.nan                                                     # query 2's revisit: no map point at any row -> stage 4 (with refinement)
    xyz[7, :s["dn"][7]] = rng.uniform(-5, 5, (s["dn"][7], 3)) + (0, 0, 8)        # query 3's revisit: every point unrelated -> stage 5
    db.set_points(0, xyz)
    qf, qn = s["qf"].copy(), s["qn"].copy()
    qn[1] = 0                                                           # query 1: no feature, no shared word -> stage 1
    for refine in (True, False):
        got = _composite(db, qf, qn, refine)
        want = _by_hand(db, qf, qn, xyz, refine)
        _assert_equal(got, want, Q, f"stages, refine={refine}")
        assert got["stage"].tolist() == ([0, 1, 4, 5] if refine else [0, 1, 5, 5]), got["stage"]
        assert got["ok"].tolist() == [1, 0, 0, 0]
        assert got["Twc"][1].tobytes() == eye.tobytes() and got["best"][1] == -1 and got["num"][1] == 0 and got["nmatch"][1] == 0
        assert got["Twc"][2].tobytes() == eye.tobytes() and got["best"][2] == 5 and got["num"][2] == 0 and got["pnp_count"][2] == 0      # PnP without a model: identity
        assert got["best"][3] == 7 and got["num"][3] < MIN_INLIER
        assert not got["mask"][1].any() and not got["mask"][2].any()
    # stage 3: the winner's list is shorter than min_inlier (every list is: the matcher's lists hold at most CAP entries)
    got = _composite(db, qf, qn, True, min_inlier=CAP + 1)
    want = _by_hand(db, qf, qn, xyz, True, min_inlier=CAP + 1)
    _assert_equal(got, want, Q, "stage 3")
    assert got["stage"].tolist() == [3, 1, 3, 3] and all(got["Twc"][q].tobytes() == eye.tobytes() for q in range(Q))
    assert got["best"].tolist() == [1, -1, 5, 7] and not got["mask"].any() and not got["num"].any()
    # stage 2 through the grouping alone
    g = _group_dev(db, gr.RELOC, 3, [[(2, -2.0), (5, -3.0)]], 4)
    assert g[0]["status"] == gr.NO_GROUP and g[0]["frames"] == [-1, -1, -1] and g[0]["ngroups"] == 0
    db.close()
