"""The map-point merge on the device (include/airfe.h "Map-point merge"): airfe_bowdb_merge_points[_dev] and airfe_bowdb_loop_merge_batch_dev against the
host statement merge_build_host / merge_pairs_host (airslam_amd/csrc/merge_core.h, compiled here with the host compiler), byte for byte — device outputs,
id table and point table — on the hand cases and seeded tables of tests/merge_ref.py (the "loop detection outputs" are hand-built tensors); order
independence, repetition, hostile padding; loop_close_dev against tests/covis_ref.py and a planted point; one composite run behind loop_detect_batch_dev on
the scene of tests/test_gpu_loopdet.py; every refusal."""
import numpy as np
import pytest

import covis_ref as cr
import merge_ref as mr
import test_gpu_loopdet as T

pytestmark = pytest.mark.gpu
HAND = mr.hand_cases()


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    return mr.host_lib(tmp_path_factory.mktemp("merge_core"))


def _feat(xy):
    f = np.zeros(xy.shape[:2] + (259,), np.float32)
    f[..., 1:3] = xy
    return f


def _load(db, case):
    """the case's id table (through the _dev setter, which copies blindly) and point table, every frame of them"""
    import torch
    db.set_point_ids_dev(0, T._up(np.ascontiguousarray(case["ids"], np.int32)))
    db.set_points(0, case["xyz"])
    torch.cuda.synchronize()


def _db(case, merge=True, max_edges=mr.F_ * mr.F_):
    import torch
    from airslam_amd import api
    frames, cap = case["ids"].shape
    size = case["size"]
    db = api.BowDatabase(T._ctx(), frames, cap, keep_features=True)
    z = lambda dt: torch.zeros((size, cap), dtype=dt, device="cuda")  # noqa: E731
    db.add_batch_dev(z(torch.int32), z(torch.float64), torch.zeros(size, dtype=torch.int32, device="cuda"), T._up(_feat(case["xy"][:size])),
                     T._up(np.asarray(case["n"][:size], np.int32)))
    db.attach_map(max_edges)
    db.attach_point_ids(case["P"])
    if merge:
        db.attach_merge()
    _load(db, case)
    return db


def _loop_tensors(L):
    return [T._up(np.ascontiguousarray(L[k])) for k in ("qframe", "stage", "loop", "Rlq", "tlq", "mask", "idx", "nmatch")]


def _tables(db):
    return db.get_point_ids(0, db.max_frames), db.get_points(0, db.max_frames)


def _run(db, case, cam=None, map_none=False):
    """one device call on the tables the database holds -> (ids, xyz, map, info) as the device holds them afterwards"""
    import torch
    mp = torch.full((case["P"],), -7, dtype=torch.int32, device="cuda")
    info = torch.full((8,), -7, dtype=torch.int32, device="cuda")
    if case.get("loop") is not None:
        db.loop_merge_batch_dev(case["loop"]["cam"] if cam is None else cam, *_loop_tensors(case["loop"]), None if map_none else mp, info)
    else:
        db.merge_points_dev(T._up(case["pairs"]) if len(case["pairs"]) else None, None if map_none else mp, info)
    torch.cuda.synchronize()
    return _tables(db) + (mp.cpu().numpy(), info.cpu().numpy().tolist())


@pytest.mark.parametrize("case", HAND, ids=lambda c: c["name"])
def test_hand_cases(core, case):
    want = mr.run_host(core, case)
    db = _db(case)
    got = _run(db, case)
    assert mr.same(got, want), (case["name"], got[3], want[3], np.argwhere(got[0] != want[0])[:8].tolist())
    if case["name"] in ("no_queries", "no_live_entry", "no_pairs"):  # no live entry: the tables' bytes are unchanged and the map is the identity
        assert got[0].tobytes() == case["ids"].tobytes() and got[1].tobytes() == case["xyz"].tobytes() and (got[2] == np.arange(case["P"])).all()
    if case.get("loop") is None:                                     # the host form: the same from host buffers, then a synchronisation
        _load(db, case)
        mp, info = db.merge_points(case["pairs"], case["P"])
        assert mr.same(_tables(db) + (mp, info.tolist()), want), case["name"]
    db.close()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_seeded_tables_order_repetition_and_padding(core, seed):
    case = mr.seeded_case(seed)
    want = mr.run_host(core, case)
    assert want[3][0] > 50 and want[3][3] > 5 and want[3][4] > 10
    db = _db(case)
    got = _run(db, case)
    assert mr.same(got, want), (got[3], want[3])
    for k in range(2):                                               # the query list and every list permuted; the call repeated on restored tables
        _load(db, case)
        assert mr.same(_run(db, mr.permuted(case, 11 * seed + k)), want), k
    _load(db, case)
    assert mr.same(_run(db, case), want)
    db.close()
    p = mr.poisoned(case)                                            # rows beyond n[f] and frames beyond size hold anything, and keep it
    db = _db(p)
    gp = _run(db, p)
    assert mr.same(gp, mr.run_host(core, p))
    live = np.zeros(case["ids"].shape, bool)
    for f in range(case["size"]):
        live[f, :min(max(int(case["n"][f]), 0), mr.CAP)] = True
    assert gp[3] == want[3] and np.array_equal(gp[2], want[2]) and np.array_equal(gp[0][live], want[0][live]) and gp[1][live].tobytes() == want[1][live].tobytes()
    assert np.array_equal(gp[0][~live], p["ids"][~live]) and gp[1][~live].tobytes() == p["xyz"][~live].tobytes()
    db.close()


def _project(Twc, X):
    fx, fy, cx, cy = mr.CAM
    Xc = Twc[:3, :3].T @ (X - Twc[:3, 3])
    return np.float32(fx * Xc[0] / Xc[2] + cx), np.float32(fy * Xc[1] / Xc[2] + cy)


def test_loop_close_dev(core):
    """Merge, re-triangulate, rebuild covisibility on one stream.  Points 300 (frame 50 alone) and 301 (frame 20 alone) have one observer each and no
    position; the loop joins them, and two observers suffice.  Point 310 (frames 21, 22, with a position) is joined by 311 of frame 50."""
    import torch
    s = mr.Scene(40)
    poses = np.tile(np.eye(4), (mr.F_, 1, 1))
    for f in range(mr.F_):
        poses[f, :3, 3] = (0.1 * f, 0.02 * (f % 5), 0.0)
    X = np.array([3.5, 0.5, 6.0])
    s.put(50, 3, 300, tri=False).put(20, 7, 301, tri=False)
    s.xy[50, 3], s.xy[20, 7] = _project(poses[50], X), _project(poses[20], X)
    s.put(21, 1, 310).put(22, 2, 310).put(50, 4, 311).put(20, 8, 310, tri=False).put(51, 0, 310).put(50, 9, 320).put(23, 9, 320).put(20, 0, 321)
    t = np.array((0.3, 0.05, -0.1))
    if not mr.epipolar_er(mr.CAM, mr.I3, t, s.xy[50, 3], s.xy[20, 7]) < 9.0:      # the gate is signed: one of the two directions passes
        t = -t
    s.aim(50, 4, 20, 8, 3.0, t=t)
    assert mr.epipolar_er(mr.CAM, mr.I3, t, s.xy[50, 3], s.xy[20, 7]) < 9.0 and mr.epipolar_er(mr.CAM, mr.I3, t, s.xy[50, 4], s.xy[20, 8]) < 9.0
    s.query(50, 20, [(3, 7, 0), (4, 8, 0)], t=t)
    case = s.case("loop_close")
    want = mr.run_host(core, case)
    assert want[3] == [2, 0, 0, 0, 2, 2, 2, 0] and want[2][301] == 300 and want[2][311] == 310
    db = _db(case)
    db.set_poses(0, poses.reshape(mr.F_, 16))
    db.attach_triangulation()
    P = case["P"]
    i32 = lambda k, v=-7: torch.full((k,), v, dtype=torch.int32, device="cuda")  # noqa: E731
    mp, minfo, status, nobs, tinfo, written, cinfo = i32(P), i32(8), i32(P), i32(P), i32(4), i32(1), i32(4)
    xyz_t = torch.full((P, 3), float("nan"), dtype=torch.float64, device="cuda")
    db.loop_close_dev(mr.CAM, *_loop_tensors(case["loop"]), mp, minfo, xyz_t, status, nobs, tinfo, written, cinfo)
    torch.cuda.synchronize()
    ids, xyz = _tables(db)
    assert np.array_equal(ids, want[0]) and np.array_equal(mp.cpu().numpy(), want[2]) and minfo.cpu().numpy().tolist() == want[3]
    assert ids[20, 7] == 300 and ids[50, 3] == 300 and ids[50, 4] == 310
    had = ~np.isnan(want[1][..., 0])
    assert xyz[had].tobytes() == want[1][had].tobytes()              # only_missing: a stored position stays
    assert np.abs(xyz[20, 7] - X).max() < 1e-3 and xyz[50, 3].tobytes() == xyz[20, 7].tobytes()      # the float32 keypoints' triangulation of X
    assert status.cpu().numpy()[300] == 0 and nobs.cpu().numpy()[300] == 2 and nobs.cpu().numpy()[310] == 5
    ref = cr.build(ids, case["n"], case["size"], mr.F_, P)
    got = db.get_covisibility(ref[3][1]) + (cinfo.cpu().numpy().tolist(),)
    assert all(np.array_equal(g, w) for g, w in zip(got[:3], ref[:3])) and got[3] == ref[3]
    row = {int(g): int(w) for g, w in zip(got[1][got[0][50]:got[0][51]], got[2][got[0][50]:got[0][51]])}
    assert row == {20: 2, 21: 1, 22: 1, 23: 1, 50: 3, 51: 1}, row    # frame 50 sees 300, 310, 320
    db.close()


def test_behind_loop_detection_on_its_scene(core):
    """loop_detect_batch_dev on the scene of tests/test_gpu_loopdet.py, then loop_merge_batch_dev on its outputs in place: equal to merge_build_host on the
    read-back outputs.  Ids: one per stored position; every fourth NaN row of a loop frame an id without a position (the epipolar gate); the query
    frames' even rows an id of their own (pairs), the odd ones none (adoption)."""
    import torch
    s = T._scene()
    db = T._scene_db(s)
    N, P = s["N"], 8192
    ids = np.full((N, T.CAP), -1, np.int32)
    nxt = 0
    for f in range(N):
        for i in range(int(s["dn"][f])):
            if not np.isnan(s["xyz"][f, i, 0]) or (f in (1, 3, 5, 7) and i % 4 == 0) or (f >= 8 and i % 2 == 0):
                ids[f, i], nxt = nxt, nxt + 1
    assert nxt < P
    db.attach_point_ids(P)
    db.set_point_ids(0, ids)
    db.attach_merge()
    o = T._loop_buffers(s["Q"])
    qt = T._up(np.asarray(s["qframes"], np.int32))
    db.loop_detect_batch_dev(qt, T.CAM, T.THR, o["ok"], o["stage"], o["loop"], o["Twq"], o["Rlq"], o["tlq"], o["num"], o["mask"], o["idx"], o["score"],
                             o["nmatch"], ncons_t=o["ncons"], K=T.K)
    mp = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    info = torch.full((8,), -7, dtype=torch.int32, device="cuda")
    db.loop_merge_batch_dev(T.CAM[:4], qt, o["stage"], o["loop"], o["Rlq"], o["tlq"], o["mask"], o["idx"], o["nmatch"], mp, info)
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in o.items()}
    assert h["stage"].tolist() == [0] * 4
    L = dict(qframe=np.asarray(s["qframes"], np.int32), stage=h["stage"], loop=h["loop"], Rlq=h["Rlq"], tlq=h["tlq"], mask=h["mask"], idx=h["idx"],
             nmatch=h["nmatch"], mcap=T.CAP, cam=tuple(T.CAM[:4]))
    case = dict(name="scene", ids=ids, xyz=s["xyz"], xy=s["dbf"][..., 1:3], n=s["dn"], size=N, P=P, loop=L, pairs=None)
    want = mr.run_host(core, case)
    got = _tables(db) + (mp.cpu().numpy(), info.cpu().numpy().tolist())
    print("scene:", got[3])
    assert mr.same(got, want), (got[3], want[3])
    assert got[3][0] > 100 and got[3][1] > 10 and got[3][3] > 20 and got[3][4] > 20 and got[3][6] > 20      # the scene exercises pairs, outliers and adoption
    db.close()


def test_refusals(core):
    import torch
    from airslam_amd import api
    case = [c for c in HAND if c["name"] == "adoption"][0]
    pairs = dict(case, loop=None, pairs=np.array([[200, 202]], np.int32))
    db = _db(case, merge=False)
    before = _tables(db)

    def refused(fn, *a, **k):
        with pytest.raises(api.AirfeError):
            fn(*a, **k)
        now = _tables(db)
        assert now[0].tobytes() == before[0].tobytes() and now[1].tobytes() == before[1].tobytes()

    refused(_run, db, case)                                          # nothing attached
    refused(_run, db, pairs)
    refused(db.merge_points, pairs["pairs"], case["P"])
    db.attach_merge()
    refused(db.attach_merge)                                         # a second attach
    refused(_run, db, case, cam=(0.0, 457.0, 367.0, 248.0))          # fx or fy zero or non-finite
    refused(_run, db, case, cam=(458.0, float("nan"), 367.0, 248.0))
    refused(_run, db, case, cam=(float("inf"), 457.0, 367.0, 248.0))
    refused(_run, db, case, map_none=True)                           # a NULL argument
    refused(_run, db, pairs, map_none=True)
    L = case["loop"]
    lt = _loop_tensors(L)
    mp, info = torch.zeros(case["P"], dtype=torch.int32, device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda")
    refused(db.loop_merge_batch_dev, None, *lt, mp, info)
    refused(db.loop_merge_batch_dev, mr.CAM, lt[0], None, *lt[2:], mp, info)
    refused(db.loop_merge_batch_dev, mr.CAM, *lt, mp, None)
    wide = torch.full((1, 1025, 2), -1, dtype=torch.int32, device="cuda")
    refused(db.loop_merge_batch_dev, mr.CAM, *lt[:6], wide, lt[7], mp, info)      # mcap > 1024
    many = torch.zeros(4097, dtype=torch.int32, device="cuda")
    refused(db.loop_merge_batch_dev, mr.CAM, many, many, many, *lt[3:], mp, info)      # Q > 4096
    assert mr.same(_run(db, case), mr.run_host(core, case))          # and the database still works
    db.close()
    # more than 4096 frames in the database
    big = dict(ids=np.full((4097, 8), -1, np.int32), xyz=np.full((4097, 8, 3), np.nan), xy=np.zeros((4097, 8, 2), np.float32), n=np.full(4097, 8, np.int32),
               size=4097, P=16, loop=None, pairs=np.array([[1, 2]], np.int32))
    big["ids"][5, 0], big["ids"][6, 0] = 1, 2
    db = _db(big, max_edges=1)
    before = _tables(db)
    refused(_run, db, big)
    refused(_run, db, dict(case, ids=big["ids"], P=16))
    db.close()
