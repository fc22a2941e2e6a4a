"""Map-point triangulation on the device (include/airfe.h "Map-point triangulation"): airfe_bowdb_triangulate_points[_dev] and airfe_bowdb_fill_points_dev
against tests/triangulate_ref.py byte for byte on EVERY point — hand cases, a seeded table, segment lengths 1 .. 300, min_observers, status 2 and 3
between good points, hostile padding, repeatability beside the covisibility build, the point table's fill, a planted scene end to end, the refusals."""
import numpy as np
import pytest

import covis_ref as cr
import test_gpu_loopdet as T
import triangulate_ref as tr

pytestmark = pytest.mark.gpu
_S = {}


def _db(xy, n, pose, ids, size, max_points, max_edges=1, attach_ids=True, attach_tri=True):
    """a database of `size` frames without words whose rows hold xy at columns 1 and 2, with the poses and ids of EVERY frame of the tables (the ones past
    `size` included: the _dev setter copies blindly)"""
    import torch
    from airslam_amd import api
    ids = np.ascontiguousarray(ids, np.int32)
    frames, cap = ids.shape
    db = api.BowDatabase(T._ctx(), frames, cap, keep_features=True)
    if size:
        db.add_batch_dev(torch.zeros((size, cap), dtype=torch.int32, device="cuda"), torch.zeros((size, cap), dtype=torch.float64, device="cuda"),
                         torch.zeros(size, dtype=torch.int32, device="cuda"), T._up(tr.feat_rows(np.asarray(xy, np.float32)[:size])), T._up(np.asarray(n[:size], np.int32)))
    db.attach_map(max(max_edges, 1))
    db.set_poses(0, np.ascontiguousarray(pose, np.float64))
    if attach_ids:
        db.attach_point_ids(max_points)
        db.set_point_ids_dev(0, T._up(ids))
        if attach_tri:
            db.attach_triangulation()
    torch.cuda.synchronize()
    return db


def _out(P):
    import torch
    return (torch.full((P, 3), 7.0, dtype=torch.float64, device="cuda"), torch.full((P,), -7, dtype=torch.int32, device="cuda"),
            torch.full((P,), -7, dtype=torch.int32, device="cuda"), torch.full((4,), -7, dtype=torch.int32, device="cuda"))


def _run(db, P, min_observers=2, cam=tr.CAM):
    """one device call -> (xyz, status, nobs, info) as numpy"""
    import torch
    xyz, status, nobs, info = _out(P)
    db.triangulate_points_dev(cam, xyz, status, nobs, info, min_observers=min_observers)
    torch.cuda.synchronize()
    return xyz.cpu().numpy(), status.cpu().numpy(), nobs.cpu().numpy(), info.cpu().numpy().tolist()


def _seeded():
    """the seeded table and its restatement at (size, min_observers), computed once"""
    if "table" not in _S:
        _S["table"] = tr.seeded_table()
    return _S["table"]


def _want(size, mo):
    key = ("want", size, mo)
    if key not in _S:
        xy, n, pose, ids, _ = _seeded()
        _S[key] = tr.build(xy, n, pose, ids, size, 300, min_observers=mo)
    return _S[key]


# ---- hand cases: one frame per observer, the case's id at row 0 of its frames; good points between the bad ones --------------------------------------------
def _hand_table(with_bad=True):
    cases = tr.hand_cases()
    good = [c for c in cases if c[0] == "three_spread"][0]
    order = []
    for c in cases:
        order.append(c)
        if c[2] in (2, 3):
            order.append(good)                                      # ... so that every bad point sits between good ones
    frames = sum(len(c[1]) for c in order) + 2
    cap = 4
    xy, pose = np.zeros((frames, cap, 2), np.float32), np.tile(np.eye(4).reshape(16), (frames, 1))
    ids, n = np.full((frames, cap), -1, np.int32), np.full(frames, cap, np.int32)
    f = 0
    for m, (name, observers, want) in enumerate(order):
        for x, y, Tm in observers:
            xy[f, 0], pose[f] = (x, y), Tm
            ids[f, 0] = m if with_bad or want not in (2, 3) else -1
            f += 1
    return xy, n, pose, ids, order


def test_hand_cases_and_bad_points_between_good_ones():
    xy, n, pose, ids, order = _hand_table()
    frames, P = ids.shape[0], len(order) + 3
    db = _db(xy, n, pose, ids, frames, P)
    got = _run(db, P)
    assert tr.same(got, tr.build(xy, n, pose, ids, frames, P))
    for m, (name, observers, want) in enumerate(order):             # ... and per case what the case says, from the observers directly
        x, st, _ = tr.point(tr.CAM, observers)
        assert st == want == got[1][m] and got[2][m] == len(observers), (name, got[1][m])
        assert np.array_equal(got[0][m].view(np.uint64), np.array(x, np.float64).view(np.uint64)), name
    assert got[3] == [sum(c[2] == 0 for c in order), sum(c[2] != -1 for c in order), sum(c[2] == 2 for c in order), sum(c[2] == 3 for c in order)]
    assert got[3][2] == 3 and got[3][3] == 3
    db.close()
    # the same table without the bad points: every other point keeps its bytes
    xy, n, pose, cids, _ = _hand_table(with_bad=False)
    db = _db(xy, n, pose, cids, frames, P)
    clean = _run(db, P)
    db.close()
    keep = np.array([c[2] not in (2, 3) for c in order] + [True] * 3)
    assert (clean[1][~keep] == -1).all() and clean[3][2:] == [0, 0]
    assert tr.same((got[0][keep], got[1][keep], got[2][keep], []), (clean[0][keep], clean[1][keep], clean[2][keep], []))


@pytest.mark.parametrize("size,mo", [(40, 2), (40, 3), (35, 2)])
def test_seeded_table(size, mo):
    xy, n, pose, ids, _ = _seeded()
    want = _want(size, mo)
    db = _db(xy, n, pose, ids, size, 300)
    got = _run(db, 300, mo)
    assert tr.same(got, want), (got[3], want[3])
    hx, hs, hn, ok = db.triangulate_points(tr.CAM, 300, min_observers=mo)      # the host form: the same bytes, then a synchronisation
    assert tr.same((hx, hs, hn, []), want[:3] + ([],)) and ok == want[3][0]
    if mo == 3:
        two = _want(size, 2)
        assert (want[1][two[2] == 2] == 1).all() and (two[1][two[2] == 2] != 1).all() and (two[2] == 2).sum() > 5      # min_observers decides these
    db.close()


@pytest.mark.parametrize("L", [1, 2, 3, 63, 64, 65, 130, 300])
def test_segment_lengths(L):
    """one point seen by L frames among ordinary ones (cap 8): around a wave, past a workgroup of the sort, longer than any typical segment"""
    frames, cap, P = L + 3, 8, 40
    rng = np.random.default_rng(100 + L)
    X = tr.cloud(P, rng)
    pose = np.stack([tr.pose_on_path(f, frames) for f in range(frames)])
    ids = rng.integers(-1, P, size=(frames, cap)).astype(np.int32)
    ids[ids == 5] = 6
    ids[:L, rng.integers(0, cap)] = 5
    n = np.array([(8, 7, 8, 5)[f % 4] for f in range(frames)], np.int32)
    for f in range(L):                                              # ... inside the count wherever it sits
        i = int(np.flatnonzero(ids[f] == 5)[0])
        if i >= n[f]:
            ids[f, 0], ids[f, i] = 5, ids[f, 0]
    xy = np.zeros((frames, cap, 2), np.float32)
    for f in range(frames):
        for i in range(cap):
            u, v, _ = tr.project(tr.CAM, pose[f], X[max(int(ids[f, i]), 0)])
            xy[f, i] = (u + rng.normal(0, 0.3), v + rng.normal(0, 0.3))
    want = tr.build(xy, n, pose, ids, frames, P)
    assert want[2][5] == L and want[1][5] == (1 if L == 1 else 0)
    db = _db(xy, n, pose, ids, frames, P)
    got = _run(db, P)
    assert tr.same(got, want), (L, got[3], want[3])
    db.close()


def test_hostile_padding():
    xy, n, pose, ids, _ = _seeded()
    frames, P, size = ids.shape[0], 300, 35
    want = _want(size, 2)
    nxy, nids, npose = xy.copy(), ids.copy(), pose.copy()
    for f in range(frames):
        nids[f, n[f]:] = np.array([2 ** 31 - 1, -2 ** 31, 5, P - 1, P, 17], np.int64).astype(np.int32)[(np.arange(ids.shape[1] - n[f]) + f) % 6]
        nxy[f, n[f]:] = np.nan
    nids[size:] = np.array([7, 2 ** 31 - 1, -2 ** 31, 0], np.int64).astype(np.int32)[np.arange(ids.shape[1]) % 4]
    npose[size:] = np.nan
    assert tr.same(tr.build(nxy, n, npose, nids, size, P), want)
    db = _db(nxy, n, npose, nids, size, P)
    assert tr.same(_run(db, P), want)
    db.close()
    clean = ids.copy()
    for f in range(frames):
        clean[f, n[f]:] = -1
    clean[size:] = -1
    db = _db(xy, n, pose, clean, size, P)
    assert tr.same(_run(db, P), want)
    db.close()


def test_repeatability_beside_the_covisibility_build():
    import torch
    xy, n, pose, ids, _ = _seeded()
    frames, P, size = ids.shape[0], 300, 40
    want = _want(size, 2)
    cov = cr.build(ids, n, size, frames, P)
    E = cov[3][1]
    db = _db(xy, n, pose, ids, size, P, max_edges=E)

    def covis():
        info = torch.full((4,), -7, dtype=torch.int32, device="cuda")
        db.build_covisibility_dev(info)
        torch.cuda.synchronize()
        row_ptr, nbr, weight = db.get_covisibility(E)
        got = (row_ptr, nbr, weight, info.cpu().numpy().tolist())
        assert all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(got[:3], cov[:3])) and got[3] == list(cov[3])

    covis()
    first = _run(db, P)
    second = _run(db, P)
    covis()
    third = _run(db, P)
    covis()
    for got in (first, second, third):
        assert tr.same(got, want)
    db.close()


def _points_table(frames, cap, n, size, seed=21):
    """a point table that is partly NaN, with sentinels in rows past n[f] and frames past size"""
    rng = np.random.default_rng(seed)
    pts = rng.normal(0, 5, size=(frames, cap, 3))
    pts[rng.random((frames, cap)) < 0.5] = np.nan
    for f in range(frames):
        pts[f, n[f]:] = -1234.5
    pts[size:] = -4321.5
    return pts


@pytest.mark.parametrize("only_missing", [0, 1])
def test_fill_points(only_missing):
    import torch
    xy, n, pose, ids, _ = _seeded()
    frames, P, size = ids.shape[0], 300, 35
    want = _want(size, 2)
    pts = _points_table(frames, ids.shape[1], n, size)
    db = _db(xy, n, pose, ids, size, P)
    db.set_points(0, pts)
    xyz, status, nobs, info = _out(P)
    written = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    db.triangulate_points_dev(tr.CAM, xyz, status, nobs, info)
    torch.cuda.synchronize()
    assert np.array_equal(db.get_points(0, frames).view(np.uint64), pts.view(np.uint64))        # the triangulation alone leaves the table alone
    db.fill_points_dev(xyz, status, written, only_missing=bool(only_missing))
    torch.cuda.synchronize()
    ref, count = tr.fill(pts, n, ids, size, P, want[0], want[1], bool(only_missing))
    got = db.get_points(0, frames)
    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64))
    assert int(written.item()) == count and count > 200
    other = tr.fill(pts, n, ids, size, P, want[0], want[1], not only_missing)[1]
    assert (count < other) == bool(only_missing)                    # the flag decides something on this table
    for f in range(frames):                                         # sentinels: rows past n[f], frames past size
        assert (got[f, (n[f] if f < size else 0):] == (-1234.5 if f < size else -4321.5)).all()
    db.close()


def test_end_to_end_planted_scene():
    import torch
    xy, n, pose, ids, X = tr.planted_scene()
    frames, cap = ids.shape
    P, mo = len(X), 3
    db = _db(xy, n, pose, ids, frames, P)                           # the point table: NaN everywhere, as attach_map leaves it
    assert np.isnan(db.get_points(0, frames)).all()
    xyz, status, nobs, info = _out(P)
    written = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    db.retriangulate_dev(tr.CAM, xyz, status, nobs, info, written, min_observers=mo, only_missing=True)
    torch.cuda.synchronize()
    status, nobs = status.cpu().numpy(), nobs.cpu().numpy()
    count = np.bincount(ids[ids >= 0], minlength=P)
    assert np.array_equal(nobs, count) and list(nobs[:6]) == [0, 1, 2, 3, 4, 5]
    assert np.array_equal(status == 0, nobs >= mo) and (status[(nobs > 0) & (nobs < mo)] == 1).all() and (status[nobs == 0] == -1).all()
    pts = db.get_points(0, frames)
    filled, worst = 0, 0.0
    for f in range(frames):
        for i in range(cap):
            m = int(ids[f, i])
            if m < 0 or nobs[m] < mo:
                assert np.isnan(pts[f, i]).all()
                continue
            u, v, depth = tr.project(tr.CAM, pose[f], pts[f, i])
            worst = max(worst, abs(u - float(xy[f, i, 0])), abs(v - float(xy[f, i, 1])))
            filled += 1
            assert depth > 0
    print(f"planted scene: {filled} filled rows, largest reprojection error {worst:.3e} px")
    assert filled == int(written.item()) == int(count[count >= mo].sum()) and filled > 400
    assert worst < 1e-3
    db.close()


def test_refusals_change_nothing():
    import torch
    from airslam_amd import api
    xy, n, pose, ids, _ = _seeded()
    frames, P = ids.shape[0], 300
    pts = _points_table(frames, ids.shape[1], n, frames)
    written = torch.full((1,), -7, dtype=torch.int32, device="cuda")

    def untouched(db, out):
        torch.cuda.synchronize()
        assert (out[0] == 7.0).all() and all((t == -7).all() for t in out[1:]) and int(written.item()) == -7
        assert np.array_equal(db.get_points(0, frames).view(np.uint64), pts.view(np.uint64))

    # no id table: nothing to attach to
    db = _db(xy, n, pose, ids, frames, P, attach_ids=False)
    db.set_points(0, pts)
    with pytest.raises(api.AirfeError, match="id table"):
        db.attach_triangulation()
    db.close()
    # no attach
    db = _db(xy, n, pose, ids, frames, P, attach_tri=False)
    db.set_points(0, pts)
    out = _out(P)
    with pytest.raises(api.AirfeError, match="no triangulation attached"):
        db.triangulate_points_dev(tr.CAM, *out)
    with pytest.raises(api.AirfeError, match="no triangulation attached"):
        db.fill_points_dev(out[0], out[1], written)
    with pytest.raises(api.AirfeError, match="no triangulation attached"):
        db.triangulate_points(tr.CAM, P)
    untouched(db, out)
    db.attach_triangulation()
    with pytest.raises(api.AirfeError, match="attached already"):
        db.attach_triangulation()
    # fx = 0, a NaN fy; NULL outputs
    for cam in ((0.0, 410.0, 320.0, 240.0), (400.0, float("nan"), 320.0, 240.0)):
        with pytest.raises(api.AirfeError, match="fx and fy"):
            db.triangulate_points_dev(cam, *out)
    for k in range(4):
        args = list(out)
        args[k] = None
        with pytest.raises(api.AirfeError, match="bad argument"):
            db.triangulate_points_dev(tr.CAM, *args)
    with pytest.raises(api.AirfeError, match="bad argument"):
        db.triangulate_points_dev(None, *out)
    for args in ((None, out[1], written), (out[0], None, written), (out[0], out[1], None)):
        with pytest.raises(api.AirfeError, match="bad argument"):
            db.fill_points_dev(*args)
    untouched(db, out)
    # ... and the database still works
    got = _run(db, P)
    assert tr.same(got, _want(frames, 2))
    db.close()
