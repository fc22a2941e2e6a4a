"""The covisibility build on the device (include/airfe.h "Map-point ids and the covisibility build"): airfe_bowdb_build_covisibility[_dev] against
tests/covis_ref.py, exactly — the hand cases, a seeded table, wave and workgroup tails, a segment longer than a workgroup, hostile padding, the capacity
rule, replacement, two builds of one table; the id table's round trip and refusals; and loop detection and relocalisation on a graph built on the device
against the same graph uploaded from the host, byte for byte."""
import numpy as np
import pytest

import bowgroup_ref as gr
import covis_ref as cr
import test_gpu_loopdet as T

pytestmark = pytest.mark.gpu


def _db(ids, n, size, max_frames, max_points, max_edges, attach=True):
    """a database of `size` frames without words whose stored feature counts are n[:size], with the map state and the id table (through the _dev setter,
    which copies blindly: every frame of the table, the ones past `size` included)"""
    import torch
    from airslam_amd import api
    ids = np.ascontiguousarray(ids, np.int32)
    cap = ids.shape[1]
    db = api.BowDatabase(T._ctx(), max_frames, cap, keep_features=True)
    if size:
        db.add_batch_dev(torch.zeros((size, cap), dtype=torch.int32, device="cuda"), torch.zeros((size, cap), dtype=torch.float64, device="cuda"),
                         torch.zeros(size, dtype=torch.int32, device="cuda"), torch.zeros((size, cap, 259), dtype=torch.float32, device="cuda"),
                         T._up(np.asarray(n[:size], np.int32)))
    db.attach_map(max(max_edges, 1))
    if attach:
        db.attach_point_ids(max_points)
        db.set_point_ids_dev(0, T._up(ids[:max_frames]))
    torch.cuda.synchronize()
    return db


def _build(db, edge_cap):
    """one device build -> (row_ptr, nbr, weight, info) as the device holds them afterwards"""
    import torch
    info = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    db.build_covisibility_dev(info)
    torch.cuda.synchronize()
    row_ptr, nbr, weight = db.get_covisibility(edge_cap)
    return row_ptr, nbr, weight, info.cpu().numpy().tolist()


def _same(got, want):
    return all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(got[:3], want[:3])) and list(got[3]) == list(want[3])


def _pad(ids, frames):
    ids = np.asarray(ids, np.int64).astype(np.int32)
    return np.concatenate([ids, np.full((frames - len(ids), ids.shape[1]), -1, np.int32)]) if frames > len(ids) else ids


@pytest.mark.parametrize("case", cr.hand_cases(), ids=lambda c: c[0])
def test_hand_cases(case):
    name, ids, n, size, max_frames, P, rows, (valid, ignored) = case
    want = cr.expected_csr(rows, max_frames) + ([0, sum(len(r) for r in rows.values()), valid, ignored],)
    db = _db(_pad(ids, max_frames), n, size, max_frames, P, max(want[3][1], 1))
    got = _build(db, max(want[3][1], 1))
    assert _same(got, want), (name, got)
    assert _same(got, cr.build(ids, n, size, max_frames, P))
    db.close()


def test_seeded_table():
    ids, n = cr.random_table()
    frames, P = ids.shape[0], 600
    for size in (frames, frames - 5):
        want = cr.build(ids, n, size, frames, P)
        db = _db(ids, n, size, frames, P, want[3][1])
        got = _build(db, want[3][1])
        assert _same(got, want), (size, got[3], want[3])
        assert db.build_covisibility() == want[3][1]                 # the host form: the same, then a synchronisation
        assert _same(db.get_covisibility(want[3][1]) + (want[3],), want)
        db.close()


def _tail_table(frames, cap=128, P=300, seed=11):
    rng = np.random.default_rng(seed + frames)
    ids = rng.integers(0, P, size=(frames, cap)).astype(np.int32)
    ids[rng.random((frames, cap)) < 0.1] = -1
    n = np.array([(64, 0, 1, 63, 65, 128)[f % 6] for f in range(frames)], np.int32)
    return ids, n


@pytest.mark.parametrize("size", [1, 63, 64, 65, 130])
def test_wave_and_workgroup_tails(size):
    """cap 128 with n in {0, 1, 63, 64, 65, 128}; database sizes around a wave and past half a workgroup's compaction step"""
    ids, n = _tail_table(size + 2)
    want = cr.build(ids, n, size, size + 2, 300)
    db = _db(ids, n, size, size + 2, 300, want[3][1])
    got = _build(db, want[3][1])
    assert _same(got, want), (size, got[3], want[3])
    db.close()


@pytest.mark.parametrize("tiles", [257, 513])
def test_more_scan_tiles_than_one_round_of_the_tile_scan(tiles):
    """max_points of 257 / 513 segment-start tiles (2048 points each): the one workgroup that turns the tile sums into tile offsets walks them in rounds of
    256 with a running base, and its last round ends one tile into a wave.  Ids in the first tile, on both sides of the round's border and in the last tile."""
    P = tiles * 2048 - 1
    frames, cap = 6, 16
    marks = np.array([0, 1, 2047, 2048, 255 * 2048 + 7, 256 * 2048 - 1, 256 * 2048, 256 * 2048 + 1, P // 2, P - 2048, P - 2, P - 1, P, -1], np.int64)
    ids = marks[np.random.default_rng(tiles).integers(0, len(marks), size=(frames, cap))].astype(np.int32)
    n = np.full(frames, cap, np.int32)
    want = cr.build(ids, n, frames, frames, P)
    db = _db(ids, n, frames, frames, P, want[3][1])
    got = _build(db, want[3][1])
    assert want[3][1] > frames and _same(got, want), (tiles, got[3], want[3])
    db.close()


def test_one_point_seen_by_300_frames():
    """a segment longer than a wave and than a workgroup: every frame's only row holds point 5, so every row is 300 entries of weight 1"""
    frames, cap = 300, 8
    ids = np.full((frames, cap), -1, np.int32)
    ids[:, 0] = 5
    n = np.ones(frames, np.int32)
    db = _db(ids, n, frames, frames, 16, frames * frames)
    row_ptr, nbr, weight, info = _build(db, frames * frames)
    assert info == [0, frames * frames, frames, 0]
    assert np.array_equal(row_ptr, np.arange(frames + 1, dtype=np.int32) * frames)
    assert np.array_equal(nbr.reshape(frames, frames), np.tile(np.arange(frames, dtype=np.int32), (frames, 1))) and (weight == 1).all()
    db.close()


def test_hostile_padding_and_out_of_range_ids():
    ids, n = cr.random_table()
    frames, P = ids.shape[0], 600
    size = frames - 5
    clean = ids.copy()
    clean[(clean < -1) | (clean >= P)] = -1                           # what the build makes of an id out of range
    for f in range(frames):
        clean[f, n[f]:] = -1
    clean[size:] = -1
    want = cr.build(clean, n, size, frames, P)
    assert want[3][3] == 0
    # rows past n[f] and frames past size: large positive, negative and in-range ids
    noisy = clean.copy()
    for f in range(frames):
        noisy[f, n[f]:] = [2 ** 31 - 1, -2 ** 31, 5, P - 1, P, -2][f % 6]
    noisy[size:] = np.array([7, 2 ** 31 - 1, -2 ** 31, 0], np.int32)[np.arange(ids.shape[1]) % 4]
    db = _db(noisy, n, size, frames, P, want[3][1])
    assert _same(_build(db, want[3][1]), want)
    db.close()
    # out-of-range ids inside valid rows: counted, nothing else changes
    full = cr.build(ids, n, size, frames, P)
    assert full[3][3] > 5 and full[3][:3] == want[3][:3] and _same(full[:3] + ([],), want[:3] + ([],))
    db = _db(ids, n, size, frames, P, want[3][1])
    assert _same(_build(db, want[3][1]), full)
    db.close()


def test_capacity():
    from airslam_amd import api
    ids, n = cr.random_table()
    frames, P = ids.shape[0], 600
    want = cr.build(ids, n, frames, frames, P)
    E = want[3][1]
    exact = _db(ids, n, frames, frames, P, E)                           # max_edges equal to the need: ok
    assert _same(_build(exact, E), want)
    short = _db(ids, n, frames, frames, P, E - 1)                       # one less: status 1, the count needed, an empty graph
    got = _build(short, E - 1)
    assert got[3] == [1, E] + want[3][2:] and not got[0].any() and len(got[1]) == 0
    with pytest.raises(api.AirfeError):                                 # the host form: an error return
        short.build_covisibility()
    assert not short.get_covisibility(E - 1)[0].any()
    assert _same(_build(exact, E), want)                                # a following build with enough room is correct
    short.close()
    exact.close()


def test_replacement_equals_a_fresh_database():
    import torch
    ids, n = cr.random_table()
    frames, P = ids.shape[0], 600
    big = cr.build(ids, n, frames - 5, frames, P)
    small_ids = ids.copy()
    small_ids[::2] = -1                                                 # every second frame loses its points: the graph shrinks
    small_ids[1, :4] = [3, 3, 9, -1]
    small = cr.build(small_ids, n, frames - 5, frames, P)
    assert small[3][1] < big[3][1] // 2
    db = _db(ids, n, frames - 5, frames, P, big[3][1])
    assert _same(_build(db, big[3][1]), big)
    db.set_point_ids_dev(0, T._up(small_ids))
    torch.cuda.synchronize()
    again = _build(db, big[3][1])
    fresh_db = _db(small_ids, n, frames - 5, frames, P, big[3][1])
    fresh = _build(fresh_db, big[3][1])
    assert _same(again, small) and _same(fresh, small)
    assert again[0].tobytes() == fresh[0].tobytes() and again[0][frames] == small[3][1] and (again[0][frames - 5:] == small[3][1]).all()
    db.close()
    fresh_db.close()


def test_two_builds_are_byte_equal():
    ids, n = _tail_table(130)
    want = cr.build(ids, n, 130, 130, 300)
    db = _db(ids, n, 130, 130, 300, want[3][1])
    a = _build(db, want[3][1])
    b = _build(db, want[3][1])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])) and a[3] == b[3] and _same(a, want)
    db.close()


def test_id_table_round_trip_and_refusals():
    import torch
    from airslam_amd import api
    cap, frames, P = 16, 6, 50
    rng = np.random.default_rng(9)
    db = _db(np.full((frames, cap), -1, np.int32), np.full(frames, cap, np.int32), frames, frames, P, 64)
    assert (db.get_point_ids(0, frames) == -1).all()                    # initialised to "no map point"
    a = rng.integers(-1, P, size=(2, cap)).astype(np.int32)
    a[0, 0], a[0, 1] = 0, P - 1
    db.set_point_ids(1, a)
    db.set_point_ids_dev(4, T._up(a[::-1].copy()))
    torch.cuda.synchronize()
    back = db.get_point_ids(0, frames)
    assert back[1:3].tobytes() == a.tobytes() and back[4:6].tobytes() == a[::-1].tobytes() and (back[[0, 3]] == -1).all()
    bad_low, bad_high = a.copy(), a.copy()
    bad_low[1, 3], bad_high[0, 5] = -2, P
    for call in (lambda: db.set_point_ids(1, bad_low), lambda: db.set_point_ids(1, bad_high),                  # a host id out of range
                 lambda: db.set_point_ids(5, a), lambda: db.set_point_ids_dev(5, T._up(a)), lambda: db.get_point_ids(5, 2),
                 lambda: db.get_point_ids(-1, 2),                                                              # frames beyond max_frames
                 lambda: db.attach_point_ids(P)):                                                              # a second attach
        with pytest.raises(api.AirfeError):
            call()
    assert db.get_point_ids(0, frames).tobytes() == back.tobytes()      # nothing was changed
    db.close()
    for bad in (0, -3, (1 << 24) + 1):                                  # max_points outside 1 .. 2^24
        fresh = _db(np.full((2, cap), -1, np.int32), [cap, cap], 2, 2, P, 8, attach=False)
        with pytest.raises(api.AirfeError):
            fresh.attach_point_ids(bad)
        fresh.close()
    # no id table: the setters, the getter and the build are return codes
    plain = _db(np.full((2, cap), -1, np.int32), [cap, cap], 2, 2, P, 8, attach=False)
    info = torch.zeros(4, dtype=torch.int32, device="cuda")
    for call in (lambda: plain.set_point_ids(0, a), lambda: plain.set_point_ids_dev(0, T._up(a)), lambda: plain.get_point_ids(0, 1),
                 lambda: plain.build_covisibility_dev(info), lambda: plain.build_covisibility()):
        with pytest.raises(api.AirfeError):
            call()
    plain.close()
    # no map state: the attach is a return code
    bare = api.BowDatabase(T._ctx(), 2, cap, keep_features=True)
    with pytest.raises(api.AirfeError):
        bare.attach_point_ids(P)
    bare.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------------
def _chain_ids(xyz):
    """frames f and f + 1 share 20 points (rows 0 .. 19 of f, 20 .. 39 of f + 1), frames f and f + 2 share 4 (rows 40 .. 43 of f, 44 .. 47 of f + 2);
    -1 wherever the row has no map point (NaN in xyz [N][cap][3])"""
    N, cap = xyz.shape[:2]
    ids = np.full((N, cap), -1, np.int32)
    for f in range(N):
        ids[f, :20] = 100 * f + np.arange(20)
        if f > 0:
            ids[f, 20:40] = 100 * (f - 1) + np.arange(20)
        ids[f, 40:44] = 100 * f + 50 + np.arange(4)
        if f > 1:
            ids[f, 44:48] = 100 * (f - 2) + 50 + np.arange(4)
    ids[np.isnan(xyz[:, :, 0])] = -1
    return ids


def _scene_with_ids():
    """The scene of tests/test_gpu_loopdet.py (13 stored frames; frames 8 .. 11 revisit frames 1, 3, 5, 7) with two changes: frame 6 holds frame 7's rows
    from row 60 on (a candidate of query 11 next to frame 7 with another score), and frames 8 .. 12 get map points at their first 60 rows.  Ids: _chain_ids, and frame 3 holds one point twice."""
    s = dict(T._scene())
    N, CAP = s["N"], T.CAP
    rng = np.random.default_rng(77)
    s["dn"], s["xyz"], s["dbf"] = s["dn"].copy(), s["xyz"].copy(), s["dbf"].copy()
    m = int(s["dn"][7]) - 60
    s["dbf"][6], s["dn"][6] = 0, m
    s["dbf"][6, :m] = s["dbf"][7, 60:60 + m]
    s["xyz"][8:13, :60] = rng.uniform(-5, 5, (5, 60, 3)) + (0, 0, 8)
    ids = _chain_ids(s["xyz"])
    ids[3, 60] = ids[3, 0] if ids[3, 60] >= 0 else -1
    return s, ids


def _equal_outputs(name, a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), (name, k)


def test_composites_on_the_built_graph_equal_the_uploaded_graph():
    import torch
    s, ids = _scene_with_ids()
    N, P = s["N"], 100 * s["N"]
    row_ptr, nbr, weight, info = cr.build(ids, s["dn"], N, N, P)
    w = {(f, int(nbr[e])): int(weight[e]) for f in range(N) for e in range(row_ptr[f], row_ptr[f + 1])}
    assert info[1] <= 64 and w[(6, 7)] > 10 and w[(7, 6)] > 10 and 0 < w[(6, 8)] <= 10 and (11, 6) not in w
    above, below = sum(v > 10 for (f, g), v in w.items() if f != g), sum(v <= 10 for (f, g), v in w.items() if f != g)
    assert above >= 10 and below >= 10
    # the graph uploaded from the host
    db = T._scene_db(s)
    db.set_covisibility(row_ptr, nbr, weight)
    up_loop = T._composite(db, s["qframes"])
    db.close()
    # the graph built on the device
    db = T._scene_db(s)
    db.attach_point_ids(P)
    db.set_point_ids(0, ids)
    got = _build(db, 64)
    assert _same(got, (row_ptr, nbr, weight, info))
    dev_loop = T._composite(db, s["qframes"])
    _equal_outputs("loop", up_loop, dev_loop)
    print("loop stage", dev_loop["stage"].tolist(), "loop", dev_loop["loop"].tolist())
    assert dev_loop["stage"].tolist() == [0] * 4 and dev_loop["loop"].tolist() == [1, 3, 5, 7]
    # the weights are read: for query 11 frames 6 and 7 are both candidates with different scores and w[6][7] > 10, so the group seeded at the lower of
    # the two takes its NEIGHBOUR as deputy and only the higher one is a deputy; with that weight at 10 or below each would stay a deputy of its own
    st = T._stored(db, [11], N, True)
    k = int(st["ncand"][0])
    cands = list(zip(st["frame"][0, :k].tolist(), st["score"][0, :k].tolist()))
    sc = dict(cands)
    assert 6 in sc and 7 in sc and sc[7] != sc[6], cands
    lo, hi = sorted((6, 7), key=lambda f: sc[f])
    pos = s["poses"].reshape(-1, 4, 4)[:, :3, 3]
    i32 = lambda shape: torch.zeros(shape, dtype=torch.int32, device="cuda")  # noqa: E731
    gf, gs, ng, gst = i32((1, T.K)), torch.zeros((1, T.K), dtype=torch.float64, device="cuda"), i32((1,)), i32((1,))
    cf, cs = np.full((1, N), -7, np.int32), np.zeros((1, N))
    cf[0, :k], cs[0, :k] = st["frame"][0, :k], st["score"][0, :k]
    db.group_dev(gr.LOOP, T._up(cf), T._up(cs), T._up(np.array([k], np.int32)), gf, gs, ng, gst, qpos_t=T._up(pos[11:12].copy()),
                 max_dist_t=T._up(np.array([1e9])))
    torch.cuda.synchronize()
    want = gr.group(gr.LOOP, cands, gr.covis_dict(row_ptr, nbr, weight), T.K, positions={f: pos[f] for f in range(N)}, qpos=pos[11], max_dist=1e9)
    flat = gr.group(gr.LOOP, cands, gr.covis_dict(row_ptr, nbr, np.minimum(weight, 10)), T.K, positions={f: pos[f] for f in range(N)}, qpos=pos[11], max_dist=1e9)
    assert gf.cpu().numpy()[0].tolist() == want["frames"] and int(ng[0]) == want["ngroups"]
    assert lo not in want["frames"] and hi in want["frames"] and lo in flat["frames"] and hi in flat["frames"]
    db.close()


def test_relocalisation_on_the_built_graph_equals_the_uploaded_graph():
    """the scene of tests/test_gpu_reloc.py (4 queries against 12 stored frames) with the chain ids on its map points"""
    import test_gpu_reloc as R
    s = R._scene()
    N, P = s["N"], 100 * s["N"]
    ids = _chain_ids(s["xyz"])
    row_ptr, nbr, weight, info = cr.build(ids, s["dn"], N, N, P)
    assert info[1] <= 64 and int(weight.max()) > 10 and int(weight.min()) <= 10
    db = R._scene_db()
    db.set_covisibility(row_ptr, nbr, weight)
    up = R._composite(db, s["qf"], s["qn"], True)
    db.close()
    db = R._scene_db()
    db.attach_point_ids(P)
    db.set_point_ids(0, ids)
    assert _same(_build(db, 64), (row_ptr, nbr, weight, info))
    dev = R._composite(db, s["qf"], s["qn"], True)
    _equal_outputs("reloc", up, dev)
    print("reloc stage", dev["stage"].tolist(), "best", dev["best"].tolist())
    assert dev["stage"].tolist() == [0] * 4 and dev["best"].tolist() == [1, 3, 5, 7]
    db.close()
