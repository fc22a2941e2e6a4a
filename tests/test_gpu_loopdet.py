"""Batched loop detection on the device (include/airfe.h "Map state for loop detection", "Stored queries against their predecessors", "Loop detection
composite"): the stored query against tests/loopdet_ref.py AND against a second database grown one frame at a time through the entries that existed
before, byte for byte; the new tables' round trips and refusals; the composite against the steps done by hand through the existing entries, byte for byte,
and against the planted relative motion; every stage's failure."""
import numpy as np
import pytest

import bowdb_ref as br
import bowgroup_cases as bc
import bowgroup_ref as gr
import loopdet_ref as lr
import pnp_ref as pr
import poseopt_ref as po
from airslam_amd import weights
from planted import features, planted_pair

pytestmark = pytest.mark.gpu
CAP = 400
PLANTED = (380, 360)         # keypoints of query 0 and of every revisit: about half of the smaller count come back as matches
CAM = np.array(po.CAM_EUROC)
THR = np.array(po.THR_EUROC)
K = 5
_S = {}


def _ctx():
    """one context for the file: LightGlue for the composite (Q K = 20 pairs), the 10^4-word vocabulary"""
    if "ctx" not in _S:
        from airslam_amd import api
        c = api.Context(lightglue=weights.synthetic_lightglue(1234), max_batch=20, max_keypoints=CAP)
        c.bow_load(weights.synthetic_vocabulary(1234, k=10, L=4))
        _S["ctx"] = c
    return _S["ctx"]


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- the stored query -------------------------------------------------------------------------------------------------------------------------------
VCAP = 64


def _hand_vectors():
    """N = 70 frames of 25 .. 64 words out of 260 (ids spread over the vocabulary's 10^4): any two share a dozen, so the thresholds and the lists are busy.
    Frame 40's exact duplicate is stored later, as frame 66; frame 33 is empty; frame 69 repeats frame 2.  Covisibility: six neighbours per row at any
    weight, below and above the row's own index, on both sides of frame 32 and of frame 64."""
    if "vec" not in _S:
        rng = np.random.default_rng(70)
        N = 70
        vecs = []
        for f in range(N):
            w = sorted(int(x) * 37 + 5 for x in rng.choice(260, size=int(rng.integers(25, VCAP + 1)), replace=False))
            vecs.append(br.frame_to_bow(w, rng.uniform(0.1, 1.0, len(w))))
        vecs[66] = (vecs[40][0].copy(), vecs[40][1].copy())
        vecs[69] = (vecs[2][0].copy(), vecs[2][1].copy())
        vecs[33] = (np.zeros(0, np.uint32), np.zeros(0))
        rows = {f: sorted((int(g), int(rng.integers(1, 40))) for g in rng.choice(N, size=6, replace=False)) for f in range(N)}
        rows[68] = [(g, 3) for g in (1, 30, 31, 32, 33, 63, 64, 65, 68, 69)]
        _S["vec"] = (vecs, bc.csr(N, rows))
    return _S["vec"]


def _pack(vecs):
    ids, vals, nw = np.zeros((len(vecs), VCAP), np.uint32), np.zeros((len(vecs), VCAP)), np.zeros(len(vecs), np.int32)
    for f, (i, v) in enumerate(vecs):
        ids[f, :len(i)], vals[f, :len(i)], nw[f] = i, v, len(i)
    return ids.view(np.int32), vals, nw


def _vector_db(vecs, csr, count):
    """a database of the first `count` vectors (no feature rows are read by the query) with the covisibility attached"""
    import torch
    from airslam_amd import api
    N = len(vecs)
    db = api.BowDatabase(_ctx(), N, VCAP, keep_features=True)
    db.attach_map(max(len(csr[1]), 1))
    db.set_covisibility(*csr)
    ids, vals, nw = _pack(vecs)
    if count:
        db.add_batch_dev(_up(ids[:count]), _up(vals[:count]), _up(nw[:count]), torch.zeros((count, VCAP, 259), dtype=torch.float32, device="cuda"),
                         torch.zeros(count, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    return db


def _out(Q, ccap, N):
    import torch
    t = lambda shape, dt, fill: torch.full(shape, fill, dtype=dt, device="cuda")  # noqa: E731
    return dict(frame=t((Q, ccap), torch.int32, -7), sharing=t((Q, ccap), torch.int32, -7), score=t((Q, ccap), torch.float64, float("nan")),
                ncand=t((Q,), torch.int32, -1), max_sharing=t((Q,), torch.int32, -1), dense=t((Q, max(N, 1)), torch.int32, -1))


def _stored(db, qframes, ccap, excl, ratio=0.5):
    import torch
    o = _out(len(qframes), ccap, db.size)
    qt = _up(np.asarray(qframes, np.int32))                          # (kept alive until the stream is synchronised)
    db.query_stored_batch_dev(qt, o["frame"], o["sharing"], o["score"], o["ncand"], o["max_sharing"], ratio=ratio,
                              exclude_covisible=excl, sharing_t=o["dense"])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def _key(g, q, ccap):
    k = min(int(g["ncand"][q]), ccap)
    return (int(g["ncand"][q]), int(g["max_sharing"][q]), g["frame"][q, :k].tobytes(), g["sharing"][q, :k].tobytes(), g["score"][q, :k].tobytes(),
            g["frame"][q, k:].tobytes(), g["dense"][q].tobytes())


def _want_key(w, ccap, N):
    k = min(len(w["cands"]), ccap)
    c = w["cands"][:k]
    return (len(w["cands"]), w["max_sharing"], np.array([x[0] for x in c], np.int32).tobytes(), np.array([x[1] for x in c], np.int32).tobytes(),
            np.array([x[2] for x in c], np.float64).tobytes(), np.full(ccap - k, -7, np.int32).tobytes(), np.array(w["dense"], np.int32).tobytes())


def test_stored_query_equals_incremental_growth():
    import torch
    vecs, csr = _hand_vectors()
    N = len(vecs)
    covis = lr.covisible_sets(csr[0], csr[1], N)
    db = _vector_db(vecs, csr, N)
    ids, vals, nw = _pack(vecs)
    for excl in (False, True):
        want = lr.stored_queries(vecs, range(N), 0.5, 8, covis if excl else None)
        got = _stored(db, list(range(N)), N, excl)
        for f in range(N):
            assert _key(got, f, N) == _want_key(want[f], N, N), (excl, f)
        # a second database grown through the entries that existed before: query_batch_dev with Q = 1 on the frames so far, a host-built exclusion row, add
        grown = _vector_db(vecs, csr, 0)
        words = (N + 31) // 32
        for f in range(N):
            o = _out(1, N, N)
            bits = np.zeros((1, words), np.uint32)
            for g in (covis[f] if excl else ()):
                bits[0, g >> 5] |= np.uint32(1) << np.uint32(g & 31)
            dense = torch.zeros((1, max(f, 1)), dtype=torch.int32, device="cuda")
            grown.query_batch_dev(_up(ids[f:f + 1]), _up(vals[f:f + 1]), _up(nw[f:f + 1]), o["frame"], o["sharing"], o["score"], o["ncand"], o["max_sharing"],
                                  ratio=0.5, exclude_t=_up(bits.view(np.int32)) if excl else None, sharing_t=dense)
            torch.cuda.synchronize()
            h = {k: v.cpu().numpy() for k, v in o.items()}
            h["dense"] = np.zeros((1, N), np.int32)
            h["dense"][0, :f] = dense.cpu().numpy()[0, :f]
            assert _key(h, 0, N) == _key(got, f, N), (excl, f)
            grown.add_batch_dev(_up(ids[f:f + 1]), _up(vals[f:f + 1]), _up(nw[f:f + 1]), torch.zeros((1, VCAP, 259), dtype=torch.float32, device="cuda"),
                                torch.zeros(1, dtype=torch.int32, device="cuda"))
        grown.close()
    want = lr.stored_queries(vecs, range(N), 0.5, 8, covis)
    got = _stored(db, list(range(N)), N, True)
    assert max(len(w["cands"]) for w in want) > 20 and want[66]["dense"][40] == len(vecs[40][0]) and want[40]["dense"][66] == 0
    assert sum(len(w["cands"]) < len(p["cands"]) for w, p in zip(want, lr.stored_queries(vecs, range(N), 0.5, 8, None))) >= 10      # the exclusion bites
    # ccap below the count: the full count is reported, the first ccap entries written
    small = _stored(db, list(range(N)), 3, True)
    assert (small["ncand"] > 3).sum() >= 20
    for f in range(N):
        assert _key(small, f, 3) == _want_key(want[f], 3, N), f
    # any order, repeats, indices outside the database; the same bytes alone and inside the batch
    order = [69, 5, 5, -1, 40, 70, 66, 0, 33, 1000, 64, 63, 32, 31, 68, 5]
    mixed = _stored(db, order, N, True)
    none = (0, 0, b"", b"", b"", np.full(N, -7, np.int32).tobytes(), np.zeros(N, np.int32).tobytes())
    for q, f in enumerate(order):
        assert _key(mixed, q, N) == (_key(got, f, N) if 0 <= f < N else none), (q, f)
    for q in (0, 4, 9, 14):
        assert _key(_stored(db, order[q:q + 1], N, True), 0, N) == _key(mixed, q, N), q
    # the other ratio
    r3 = _stored(db, list(range(N)), N, False, ratio=0.3)
    w3 = lr.stored_queries(vecs, range(N), 0.3, 8, None)
    for f in range(N):
        assert _key(r3, f, N) == _want_key(w3[f], N, N), f
    db.close()


def test_stored_query_over_more_frames_than_one_round_of_the_prefix_walk():
    """514 stored frames of 16 .. 20 words out of 24 (any two share about 13, so most of a prefix passes the threshold): the select kernel walks the prefix
    0 .. fq - 1 in rounds of 256 with a running base.  fq = 257 and 513 end one frame into a wave, 256 and 512 on a round's border; 300 inside the second."""
    rng = np.random.default_rng(514)
    N = 514
    vecs = []
    for f in range(N):
        w = sorted(int(x) * 37 + 5 for x in rng.choice(24, size=int(rng.integers(16, 21)), replace=False))
        vecs.append(br.frame_to_bow(w, rng.uniform(0.1, 1.0, len(w))))
    csr = bc.csr(N, {f: sorted((int(g), int(rng.integers(1, 40))) for g in rng.choice(N, size=6, replace=False)) for f in range(N)})
    covis = lr.covisible_sets(csr[0], csr[1], N)
    db = _vector_db(vecs, csr, N)
    qf = [256, 257, 300, 512, 513]
    for excl in (False, True):
        want = lr.stored_queries(vecs, qf, 0.5, 8, covis if excl else None)
        got = _stored(db, qf, N, excl)
        for q in range(len(qf)):
            assert _key(got, q, N) == _want_key(want[q], N, N), (excl, qf[q])
        assert len(want[1]["cands"]) > 128 and len(want[4]["cands"]) > 256          # the kept entries of a later round land behind a base above a round
    small = _stored(db, qf, 200, True)                                              # ccap inside the first round: the later rounds write nothing
    for q in range(len(qf)):
        assert _key(small, q, 200) == _want_key(want[q], 200, N), qf[q]
    db.close()


# ---- the tables -------------------------------------------------------------------------------------------------------------------------------------
def _loop_buffers(Q):
    import torch
    t = lambda shape, dt, fill: torch.full(shape, fill, dtype=dt, device="cuda")  # noqa: E731
    return dict(ok=t((Q,), torch.int32, -9), stage=t((Q,), torch.int32, -9), loop=t((Q,), torch.int32, -9), Twq=t((Q, 16), torch.float64, float("nan")),
                Rlq=t((Q, 9), torch.float64, float("nan")), tlq=t((Q, 3), torch.float64, float("nan")), num=t((Q,), torch.int32, -9),
                mask=t((Q, CAP), torch.uint8, 7), idx=t((Q, CAP, 2), torch.int32, -9), score=t((Q, CAP), torch.float32, float("nan")),
                nmatch=t((Q,), torch.int32, -9), ncons=t((Q,), torch.int32, -9))


def _composite(db, qframes, **kw):
    import torch
    o = _loop_buffers(len(qframes))
    qt = _up(np.asarray(qframes, np.int32))
    db.loop_detect_batch_dev(qt, CAM, THR, o["ok"], o["stage"], o["loop"], o["Twq"], o["Rlq"], o["tlq"], o["num"], o["mask"],
                             o["idx"], o["score"], o["nmatch"], ncons_t=o["ncons"], K=K, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def test_pose_and_u_right_tables_round_trip_and_refusals():
    import torch
    from airslam_amd import api
    vecs, csr = _hand_vectors()
    db = _vector_db(vecs[:6], bc.csr(6, {}), 6)
    eye = np.eye(4).reshape(16)
    assert db.get_poses(0, 6).tobytes() == np.tile(eye, (6, 1)).tobytes()          # initialised to the identity
    assert (db.get_u_right(0, 6) == -1.0).all()                                    # ... and to "no right image"
    with pytest.raises(api.AirfeError):                                            # the composite without poses
        _composite(db, [3])
    rng = np.random.default_rng(4)
    T = rng.normal(size=(2, 16))
    db.set_poses(3, T)
    back = db.get_poses(0, 6)
    assert back[3:5].tobytes() == T.tobytes() and back[:3].tobytes() == np.tile(eye, (3, 1)).tobytes() and back[5].tobytes() == eye.tobytes()
    # the translation columns became the positions the loop form of the grouping reads: a deputy at distance 0 of the query's position stays
    cf, sc, nc = _up(np.array([[3]], np.int32)), _up(np.array([[0.5]])), _up(np.array([1], np.int32))
    gf, gs = torch.zeros((1, K), dtype=torch.int32, device="cuda"), torch.zeros((1, K), dtype=torch.float64, device="cuda")
    ng, st = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    for qpos, left in ((T[0, [3, 7, 11]], 1), (T[0, [3, 7, 11]] + (0.0, 2.0, 0.0), 0)):
        db.group_dev(gr.LOOP, cf, sc, nc, gf, gs, ng, st, qpos_t=_up(qpos.reshape(1, 3)), max_dist_t=_up(np.array([1.0])))
        torch.cuda.synchronize()
        assert int(ng[0]) == left and int(st[0]) == gr.OK
    u = rng.uniform(-5, 700, (2, VCAP))
    db.set_u_right(1, u)
    db.set_u_right_dev(4, _up(u[::-1].copy()))
    torch.cuda.synchronize()
    ub = db.get_u_right(0, 6)
    assert ub[1:3].tobytes() == u.tobytes() and ub[4:6].tobytes() == u[::-1].tobytes() and (ub[[0, 3]] == -1.0).all()
    for call in (lambda: db.set_poses(5, T), lambda: db.set_u_right(5, u), lambda: db.set_u_right_dev(5, _up(u)), lambda: db.get_poses(5, 2),
                 lambda: db.get_u_right(-1, 2)):                                   # frames beyond max_frames: refused, nothing changed
        with pytest.raises(api.AirfeError):
            call()
    assert db.get_poses(0, 6).tobytes() == back.tobytes() and db.get_u_right(0, 6).tobytes() == ub.tobytes()
    db.close()
    # without attach_map: the tables, the covisible form of the stored query and the composite are return codes; the plain stored query is not
    plain = api.BowDatabase(_ctx(), 4, VCAP, keep_features=True)
    for call in (lambda: plain.set_poses(0, T), lambda: plain.get_poses(0, 1), lambda: plain.set_u_right(0, u), lambda: plain.get_u_right(0, 1),
                 lambda: _stored(plain, [0], 4, True), lambda: _composite(plain, [0])):
        with pytest.raises(api.AirfeError):
            call()
    assert _stored(plain, [0], 4, False)["ncand"].tolist() == [0]
    plain.close()


# ---- the composite ----------------------------------------------------------------------------------------------------------------------------------
def _T(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def _scene(share=0.7):
    """The scene recipe of tests/test_gpu_reloc.py with 12 stored frames + one: frames 0 .. 7 lie 25 m apart along x; frames 8 .. 11 are the queries and
    revisit frames 1, 3, 5, 7 (tests/planted.py: rows 0 .. k - 1 correspond) from a planted relative motion (up to 10 degrees, 0.2 - 0.5 m).  The loop
    frame's planted rows carry the WORLD point of the query row's pixel at a depth ~ U(2, 10) under the query's TRUE pose: `share` of them; 20 % an
    unrelated point (one that projects 60-200 px away, at another depth), the rest NaN; its other rows NaN.  Every third planted query row carries the exact
    u_right of its depth.  The stored query poses are the true ones perturbed by up to 5 degrees and 0.3 m.  Frame 6 is a copy of frame 7's rows and is
    made covisible with frame 11 (at weight 2): a candidate the filter must drop.  Frame 12 is an exact duplicate of query 9, stored after it."""
    key = ("scene", share)
    if key in _S:
        return _S[key]
    Q, N = 4, 13
    fx, fy, cx, cy, bf = CAM
    dbf, dn = np.zeros((N, CAP, 259), np.float32), np.zeros(N, np.int32)
    rng = np.random.default_rng(2025)
    xyz, ur = np.full((N, CAP, 3), np.nan), np.full((N, CAP), -1.0)
    poses = np.zeros((N, 4, 4))
    for f in range(8):
        k = 300 + 5 * f
        dbf[f, :k], dn[f] = features(k, 900 + f), k
        xyz[f, :k] = rng.uniform(-5, 5, (k, 3)) + (25.0 * f, 0, 8)
        poses[f] = _T(pr.rotation(rng.normal(size=3), rng.uniform(0.0, 20.0)), (25.0 * f, rng.uniform(-1, 1), rng.uniform(-1, 1)))
    rel, kinds = [], []
    for j in range(Q):
        a, b = planted_pair(PLANTED[0] - 20 * j, PLANTED[1], 70 + 10 * j)
        fq, f = 8 + j, 2 * j + 1
        dbf[fq, :len(a)], dn[fq] = a, len(a)
        dbf[f], dn[f] = 0, len(b)
        dbf[f, :len(b)] = b
        k = min(len(a), len(b)) // 2
        Rlq, tlq = pr.planted_motion(rng)
        Twq = poses[f] @ _T(Rlq, tlq)
        z0 = rng.uniform(2.0, 10.0, k)
        u, v = a[:k, 1].astype(np.float64), a[:k, 2].astype(np.float64)
        kind = rng.choice(3, k, p=(share, 0.2, 0.8 - share))                       # 0 true, 1 unrelated, 2 none
        d = rng.normal(size=(k, 2))
        d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(60.0, 200.0, (k, 1)) * (kind == 1)[:, None]
        z = np.where(kind == 1, rng.uniform(2.0, 10.0, k), z0)
        Xc = np.stack([(u + d[:, 0] - cx) / fx * z, (v + d[:, 1] - cy) / fy * z, z], 1)
        X = Xc @ Twq[:3, :3].T + Twq[:3, 3]
        X[kind == 2] = np.nan
        xyz[f] = np.nan
        xyz[f, :k] = X
        third = np.arange(0, k, 3)
        ur[fq, third] = u[third] - bf / z0[third]                                  # the query's own stereo measurement of the row's depth
        dR, dt = pr.planted_motion(rng, max_deg=5.0, max_t=0.3)
        poses[fq] = _T(Twq[:3, :3] @ dR, Twq[:3, 3] + dt)
        rel.append((Rlq, tlq))
        kinds.append(kind)
    dbf[6], dn[6] = dbf[7], dn[7]
    dbf[12], dn[12] = dbf[9], dn[9]
    poses[12] = _T(np.eye(3), (200.0, 0.0, 0.0))
    rows = {f: [(f, 30)] + [(g, 15) for g in (f - 1, f + 1) if 0 <= g < N] for f in range(N)}
    rows[11].append((6, 2))
    _S[key] = dict(Q=Q, N=N, dbf=dbf, dn=dn, xyz=xyz, ur=ur, poses=poses.reshape(N, 16), rel=rel, kinds=kinds, csr=bc.csr(N, rows), qframes=[8, 9, 10, 11])
    return _S[key]


def _scene_db(s):
    """the scene's frames through bow_vector_batch_dev into a database with every map table"""
    import torch
    from airslam_amd import api
    ctx, N = _ctx(), s["N"]
    ft, nt = _up(s["dbf"]), _up(s["dn"])
    ids = torch.zeros((N, CAP), dtype=torch.int32, device="cuda")
    vals = torch.zeros((N, CAP), dtype=torch.float64, device="cuda")
    nw = torch.zeros((N,), dtype=torch.int32, device="cuda")
    ctx.bow_vector_batch_dev(ft, nt, ids, vals, nw)
    db = api.BowDatabase(ctx, N, CAP, keep_features=True)
    db.add_batch_dev(ids, vals, nw, ft, nt)
    db.attach_map(64)
    db.set_points(0, s["xyz"])
    db.set_covisibility(*s["csr"])
    db.set_poses(0, s["poses"])
    db.set_u_right(0, s["ur"])
    torch.cuda.synchronize()
    return db


def _by_hand(db, s, qframes, xyz=None, distance_rate=0.03, min_matches=50, min_points=50, min_inliers=50):
    """the same chain through the entries one at a time, with its host round trips: query_stored_batch_dev, the odometry on the host, group_dev,
    match_candidates_batch_dev on the stored rows, a numpy gather, frame_optimize_batch_dev, loopdet_ref's stages and relative pose"""
    import torch
    ctx, Q, N = _ctx(), len(qframes), db.size
    xyz = s["xyz"] if xyz is None else xyz
    i32 = lambda shape, fill=0: torch.full(shape, fill, dtype=torch.int32, device="cuda")  # noqa: E731
    f64 = lambda shape: torch.zeros(shape, dtype=torch.float64, device="cuda")  # noqa: E731
    cf, cs, sc, nc, ms = i32((Q, N)), i32((Q, N)), f64((Q, N)), i32((Q,)), i32((Q,))
    qt = _up(np.asarray(qframes, np.int32))
    db.query_stored_batch_dev(qt, cf, cs, sc, nc, ms, ratio=0.5, exclude_covisible=True)
    pos = s["poses"].reshape(-1, 4, 4)[:, :3, 3]
    odom = lr.odometry(pos)
    qpos = np.array([pos[f] for f in qframes])
    md = np.array([odom[f] * distance_rate for f in qframes])
    gf, gs, ng, gst = i32((Q, K)), f64((Q, K)), i32((Q,)), i32((Q,))
    db.group_dev(gr.LOOP, cf, sc, nc, gf, gs, ng, gst, qpos_t=_up(qpos), max_dist_t=_up(md))
    best, idx, msc, nm = i32((Q,)), i32((Q, CAP, 2), -9), torch.full((Q, CAP), float("nan"), dtype=torch.float32, device="cuda"), i32((Q,))
    db.match_candidates_batch_dev(_up(s["dbf"][qframes]), _up(s["dn"][qframes]), gf, best, idx, msc, nm, None, outlier_rejection=True)
    torch.cuda.synchronize()
    h = dict(loop=best.cpu().numpy(), idx=idx.cpu().numpy(), score=msc.cpu().numpy(), nmatch=nm.cpu().numpy(), ncand=nc.cpu().numpy(), groups=gf.cpu().numpy(),
             gstatus=gst.cpu().numpy(), ngroups=ng.cpu().numpy())
    X, obs = np.zeros((Q, CAP, 3)), np.zeros((Q, CAP, 3))
    ncons, n_opt, before, maps = np.zeros(Q, np.int32), np.zeros(Q, np.int32), np.zeros(Q, np.int32), []
    for q, fq in enumerate(qframes):
        m, b = int(h["nmatch"][q]), int(h["loop"][q])
        before[q] = lr.stage_before(int(h["ncand"][q]), int(h["gstatus"][q]), int(h["ngroups"][q]), b, N, m, min_matches)
        entries = []
        if not before[q]:
            Xq, oq, entries = lr.constraints(h["idx"][q, :m], xyz[b], s["dbf"][fq], s["ur"][fq])
            ncons[q] = len(entries)
            X[q, :len(entries)], obs[q, :len(entries)] = Xq, oq
            n_opt[q] = len(entries) if len(entries) >= min_points else 0
        maps.append(entries)
    T2, inl, num = f64((Q, 16)), torch.zeros((Q, CAP), dtype=torch.uint8, device="cuda"), i32((Q,))
    ctx.frame_optimize_batch_dev(_up(X), _up(obs), _up(n_opt), _up(s["poses"][qframes]), CAM, THR, T2, inl, num)
    torch.cuda.synchronize()
    Twq, flags, num = T2.cpu().numpy(), inl.cpu().numpy(), num.cpu().numpy()
    mask = np.zeros((Q, CAP), np.uint8)
    Rlq, tlq = np.tile(np.array(lr.IDENTITY9), (Q, 1)), np.zeros((Q, 3))
    stage = np.zeros(Q, np.int32)
    for q in range(Q):
        for i, j in enumerate(maps[q][:n_opt[q]]):
            mask[q, j] = flags[q, i]
        stage[q] = lr.stage(int(before[q]), int(ncons[q]), int(num[q]), min_points, min_inliers)
        if stage[q] in (0, 5):
            Rlq[q], tlq[q] = lr.relative_pose(s["poses"][h["loop"][q]], Twq[q])
    h.update(Twq=Twq, mask=mask, num=num.astype(np.int32), stage=stage, ok=(stage == 0).astype(np.int32), Rlq=Rlq, tlq=tlq, ncons=ncons)
    return h


def _assert_equal(got, want, Q, who):
    for k in ("ok", "stage", "loop", "nmatch", "num", "ncons"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{who}: {k}")
    for q in range(Q):
        m = int(want["nmatch"][q])
        assert got["idx"][q, :m].tobytes() == want["idx"][q, :m].tobytes() and got["score"][q, :m].tobytes() == want["score"][q, :m].tobytes(), (who, q)
        assert (got["idx"][q, m:] == -9).all(), (who, q)
        assert got["mask"][q].tobytes() == want["mask"][q].tobytes(), (who, q)
        for k in ("Twq", "Rlq", "tlq"):
            assert got[k][q].tobytes() == want[k][q].tobytes(), (who, q, k, got[k][q], want[k][q])


def _qkey(o, q):
    m = int(o["nmatch"][q])
    return tuple(o[k][q].tobytes() for k in ("ok", "stage", "loop", "nmatch", "num", "ncons", "mask", "Twq", "Rlq", "tlq")) + (
        o["idx"][q, :m].tobytes(), o["score"][q, :m].tobytes())


def test_composite_equals_the_steps_done_by_hand():
    s = _scene()
    db = _scene_db(s)
    Q, qf = s["Q"], s["qframes"]
    # the scene holds what it was built for: frame 6 is a candidate of frame 11 until the covisibility drops it; frame 12 (the later duplicate of frame 9)
    # does not exist for frame 9, which the existing filter on the full database cannot say
    free, excl = _stored(db, qf, s["N"], False), _stored(db, qf, s["N"], True)
    c_free, c_excl = free["frame"][3, :free["ncand"][3]].tolist(), excl["frame"][3, :excl["ncand"][3]].tolist()
    assert 6 in c_free and 7 in c_free and 6 not in c_excl and 7 in c_excl
    assert excl["dense"][1, 12] == 0 and excl["max_sharing"][1] < _stored(db, [12], s["N"], False)["max_sharing"][0]
    got = _composite(db, qf)
    want = _by_hand(db, s, qf)
    _assert_equal(got, want, Q, "composite")
    assert got["loop"].tolist() == [1, 3, 5, 7] and got["stage"].tolist() == [0] * 4 and got["ok"].tolist() == [1] * 4
    for q in range(Q):
        R, t = s["rel"][q]
        rot, tr = pr.pose_errors(np.concatenate([got["Rlq"][q], got["tlq"][q]]), R, t)
        m = int(got["nmatch"][q])
        print(f"q={q}: nmatch {m} ncons {got['ncons'][q]} num {got['num'][q]} rot {rot:.3g} deg, trans {tr:.3g} m of {np.linalg.norm(t):.3g}")
        assert rot <= 0.1 and tr <= 0.01 * np.linalg.norm(t) + 1e-3, (q, rot, tr)          # the gate of tests/test_gpu_reloc.py
        assert m > 50 and got["ncons"][q] >= 50 and got["num"][q] >= 50
        li, k = got["idx"][q, :m], len(s["kinds"][q])
        unrelated = np.array([li[j, 1] < k and s["kinds"][q][li[j, 1]] == 1 for j in range(m)])
        assert unrelated.sum() >= 10 and not (got["mask"][q, :m].astype(bool) & unrelated).any()              # no unrelated-point row is an inlier
        stereo = np.array([s["ur"][qf[q], li[j, 0]] > 0 for j in range(m)])
        assert (got["mask"][q, :m].astype(bool) & stereo).sum() >= 10                                         # stereo constraints took part
        w = lr.relative_pose(s["poses"][got["loop"][q]], got["Twq"][q])
        assert got["Rlq"][q].tobytes() == np.array(w[0]).tobytes() and got["tlq"][q].tobytes() == np.array(w[1]).tobytes()
    # a query's bytes are the same alone and in the batch of 4
    for q in (0, 3):
        one = _composite(db, qf[q:q + 1])
        assert _qkey(one, 0) == _qkey(got, q), q
    db.close()


def test_composite_with_lists_longer_than_one_round_of_the_gather(monkeypatch):
    """The scene at capacity 640 with 620 .. 560 x 600 keypoints: the loop frames' lists hold close to 300 entries, so loopdet_gather_kernel walks them in two
    rounds of 256 with a running base and its last round ends inside a wave.  (Three rounds would need more than 512 entries: the planted recipe gives at most
    half of max_keypoints <= 1024.)"""
    import sys
    me = sys.modules[__name__]
    monkeypatch.setattr(me, "CAP", 640)
    monkeypatch.setattr(me, "PLANTED", (620, 600))
    monkeypatch.setattr(me, "_S", {})
    s = _scene()
    db = _scene_db(s)
    got = _composite(db, s["qframes"])
    _assert_equal(got, _by_hand(db, s, s["qframes"]), s["Q"], "long lists")
    print("nmatch", got["nmatch"].tolist(), "ncons", got["ncons"].tolist())
    assert (got["nmatch"] > 256).all() and (got["nmatch"] % 64 != 0).all() and got["stage"].tolist() == [0] * 4 and (got["ncons"] > 128).all()
    db.close()


def test_every_stage():
    """One query of each kind.  Stage 1: frame 0, which has no predecessor.  Stage 2: max_dist excludes every deputy (a distance_rate of
    1e-7).  Stage 3: more matches demanded than a list can hold.  Stage 4: the loop frame has no map point.  Stage 5: every point of the loop frame is
    unrelated."""
    import torch
    s = _scene()
    db = _scene_db(s)
    Q, qf, N = s["Q"], s["qframes"], s["N"]
    eye9 = np.array(lr.IDENTITY9)
    xyz = s["xyz"].copy()
    rng = np.random.default_rng(5)
    xyz[5] = np.nan                                                     # query 2's loop frame: no map point at any row -> stage 4
    xyz[7, :s["dn"][7]] = rng.uniform(-5, 5, (s["dn"][7], 3)) + (0, 0, 8)        # query 3's loop frame: every point unrelated -> stage 5
    db.set_points(0, xyz)
    # query 1 is frame 0: no predecessor, so no candidate -> stage 1
    frames = [8, 0, 10, 11]
    got = _composite(db, frames)
    want = _by_hand(db, s, frames, xyz)
    _assert_equal(got, want, Q, "stages")
    assert got["stage"].tolist() == [0, 1, 4, 5] and got["ok"].tolist() == [1, 0, 0, 0], got["stage"]
    assert got["loop"].tolist() == [1, -1, 5, 7] and got["num"][1] == 0 and got["num"][2] == 0 and got["num"][3] < 50 and got["nmatch"][1] == 0
    assert got["ncons"].tolist()[1:3] == [0, 0]
    for q in (1, 2):                                                    # stages 1 - 4: the stored pose, identity, zero, no flag
        assert got["Twq"][q].tobytes() == s["poses"][frames[q]].tobytes() and got["Rlq"][q].tobytes() == eye9.tobytes() and not got["tlq"][q].any()
        assert not got["mask"][q].any()
    w = lr.relative_pose(s["poses"][7], got["Twq"][3])                  # stage 5: the optimised pose and its relative pose are reported
    assert got["Rlq"][3].tobytes() == np.array(w[0]).tobytes() and got["tlq"][3].tobytes() == np.array(w[1]).tobytes() and got["tlq"][3].any()
    # stage 3: the winner's list is not longer than min_matches (no list is: the matcher's lists hold at most CAP entries)
    got = _composite(db, qf, min_matches=CAP)
    want = _by_hand(db, s, qf, xyz, min_matches=CAP)
    _assert_equal(got, want, Q, "stage 3")
    assert got["stage"].tolist() == [3] * 4 and got["loop"].tolist() == [1, 3, 5, 7] and not got["mask"].any() and not got["num"].any()
    assert all(got["Twq"][q].tobytes() == s["poses"][qf[q]].tobytes() and got["Rlq"][q].tobytes() == eye9.tobytes() for q in range(Q))
    # stage 2: every deputy lies farther than max_dist
    got = _composite(db, qf, distance_rate=1e-7)
    want = _by_hand(db, s, qf, xyz, distance_rate=1e-7)
    _assert_equal(got, want, Q, "stage 2")
    assert got["stage"].tolist() == [2] * 4 and got["loop"].tolist() == [-1] * 4 and not got["nmatch"].any() and (want["ncand"] > 0).all()
    assert all(got["Twq"][q].tobytes() == s["poses"][qf[q]].tobytes() for q in range(Q)) and not got["tlq"].any()
    # the capacity errors are return codes
    from airslam_amd import api
    for kw in (dict(K=0), dict(K=6)):
        with pytest.raises(api.AirfeError):
            o = _loop_buffers(1)
            qt = _up(np.array([8], np.int32))
            db.loop_detect_batch_dev(qt, CAM, THR, o["ok"], o["stage"], o["loop"], o["Twq"], o["Rlq"], o["tlq"], o["num"], o["mask"],
                                     o["idx"], o["score"], o["nmatch"], **kw)
    with pytest.raises(api.AirfeError):                                 # Q K = 25 pairs above max_batch = 20
        _composite(db, [8, 9, 10, 11, 8])
    torch.cuda.synchronize()
    db.close()
