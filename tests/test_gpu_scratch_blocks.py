"""Growth of a context's scratch block while the block is in use on a caller's stream (csrc/airfe_host.h: DevBlock, reserve): on a stream that is not the
context's, a call with batch 1, a call with batch 3 and a call with batch 24, queued with no synchronisation in between, give the bytes the same calls give on
a fresh context with the stream synchronised after every call.  Every *_batch_dev entry that carves a scratch block goes through it at the smallest shapes.

Batch 1 and batch 3 are the pair to check.  Every part of a block starts on a 256-byte boundary, so at these shapes the blocks of airfe_bow_vector_batch_dev
(16 rows x 4 bytes per part) and airfe_bowdb_query_batch_dev (8 cells x 8 bytes) are as large for batch 3 as for batch 1; the third call, batch 24, is the
one at which every block that exists grows again.  airfe_frame_optimize_batch_dev has no scratch of its own: it runs here as the other half of
airfe_track_pose_opt_batch_dev, whose three blocks (gather, constraints, the PnP scratch) all grow.

The debug hooks whose device allocations moved into the one RAII holder (csrc/airfe_debug.hip: HookStage) are covered by the tests that were there already, each
on its error returns and on its results: airfe_debug_linear and airfe_debug_qkv by tests/test_gpu_linear_kernels.py, airfe_debug_lg_block and
airfe_debug_ln_gelu by tests/test_gpu_lg_block.py, airfe_debug_gemm by tests/test_gpu_kernels.py."""
import numpy as np
import pytest

import pnp_ref as pr
import poseopt_ref as po
from test_gpu_fransac import _case as fransac_case
from test_gpu_pnp import _problem as pnp_problem
from test_gpu_poseopt import _planted_rows, _problem as poseopt_problem
from airslam_amd import api, weights

pytestmark = pytest.mark.gpu
BATCHES = (1, 3, 24)
CAP = 16
K = np.array(pr.K_EUROC)
CAM = np.array(po.CAM_EUROC)
THR = np.array(po.THR_EUROC)


def _voc():
    return weights.synthetic_vocabulary(1234, k=3, L=3)          # 40 nodes, 27 words


def _frames(B, seed):
    """B frames of CAP features near random leaves of the small tree (tests/test_gpu_bowdb.py::_frames) -> [B][CAP][259] float32"""
    voc = _voc()
    rng = np.random.default_rng(seed)
    leaves = np.nonzero(voc["n_children"] == 0)[0]
    f = np.zeros((B, CAP, 259), np.float32)
    f[..., 0] = rng.uniform(0.01, 1, (B, CAP))
    f[..., 1] = rng.uniform(4, 748, (B, CAP))
    f[..., 2] = rng.uniform(4, 476, (B, CAP))
    d = voc["desc"][rng.choice(leaves, size=(B, CAP))] + 0.15 * rng.standard_normal((B, CAP, 256), dtype=np.float32)
    f[..., 3:] = d / np.linalg.norm(d, axis=-1, keepdims=True)
    return f


def _dev(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _full(shape, value, dtype):
    import torch
    return torch.full(shape, value, dtype=dtype, device="cuda")


# ---- one entry each: setup(ctx) -> state, call(ctx, state, B, stream) -> the output tensors of a batch of B --------------------------------------------
def _fransac(ctx, state, B, stream):
    import torch
    f0 = np.zeros((B, CAP, 259), np.float32); f1 = np.zeros_like(f0)
    idx = np.zeros((B, CAP, 2), np.int32); sc = np.zeros((B, CAP), np.float32); nm = np.full(B, 12, np.int32)
    for b in range(B):
        a0, a1, i, s = fransac_case(12, 10 * B + b)
        f0[b, :12], f1[b, :12], idx[b, :12], sc[b, :12] = a0, a1, i, s
    f0, f1, idx, sc, nm = _dev(f0, f1, idx, sc, nm)
    F = _full((B, 9), 7.0, torch.float64)
    return (lambda: ctx.fundamental_ransac_batch_dev(f0, f1, idx, sc, nm, F_t=F, stream=stream)), [idx, sc, nm, F]


def _pnp(ctx, state, B, stream):
    import torch
    obj = np.zeros((B, CAP, 3), np.float32); img = np.zeros((B, CAP, 2), np.float32); n = np.zeros(B, np.int32)
    for b in range(B):
        o, i = pnp_problem((16, 12, 9, 8)[b % 4], 10 * B + b)
        obj[b, :len(o)], img[b, :len(i)], n[b] = o, i, len(o)
    obj, img, n = _dev(obj, img, n)
    Twc, Rt = _full((B, 16), 7.0, torch.float64), _full((B, 12), 7.0, torch.float64)
    mask, cnt = _full((B, CAP), 9, torch.uint8), _full((B,), -5, torch.int32)
    return (lambda: ctx.pnp_ransac_batch_dev(obj, img, n, K, Twc, mask, cnt, Rt_t=Rt, stream=stream)), [Twc, Rt, mask, cnt]


def _frame_optimize(ctx, state, B, stream):
    import torch
    X = np.zeros((B, CAP, 3)); obs = np.zeros((B, CAP, 3)); n = np.zeros(B, np.int32); T0 = np.zeros((B, 16))
    for b in range(B):
        x, o, t0 = poseopt_problem((16, 12, 10, 9)[b % 4], 10 * B + b)
        X[b, :len(x)], obs[b, :len(o)], n[b], T0[b] = x, o, len(x), t0.reshape(16)
    X, obs, n, T0 = _dev(X, obs, n, T0)
    Twc, Rt = _full((B, 16), 7.0, torch.float64), _full((B, 12), 7.0, torch.float64)
    mask, num = _full((B, CAP), 9, torch.uint8), _full((B,), -5, torch.int32)
    return (lambda: ctx.frame_optimize_batch_dev(X, obs, n, T0, CAM, THR, Twc, mask, num, Rt_t=Rt, stream=stream)), [Twc, Rt, mask, num]


def _track_pose_opt(ctx, state, B, stream):
    import torch
    xyz = np.full((B, CAP, 3), np.nan); feat = np.zeros((B, CAP, 259), np.float32); ti = np.zeros((B, CAP, 2), np.int32)
    for b in range(B):
        xyz[b], feat[b], ti[b] = _planted_rows(CAP, 0.9, 700 + 10 * B + b, missing=5)[:3]
    xyz, feat, ti, nt = _dev(xyz, feat, ti, np.full(B, CAP, np.int32))
    Twc, Rt = _full((B, 16), 7.0, torch.float64), _full((B, 12), 7.0, torch.float64)
    mask = _full((B, CAP), 9, torch.uint8)
    num, ok, pc = (_full((B,), -5, torch.int32) for _ in range(3))
    return (lambda: ctx.track_pose_opt_batch_dev(CAM, THR, 4, xyz, feat, ti, nt, Twc, mask, num, ok, Rt_t=Rt, pnp_count_t=pc, stream=stream)), \
        [Twc, Rt, mask, num, ok, pc]


def _vector_tensors(B):
    import torch
    return _full((B, CAP), -1, torch.int32), _full((B, CAP), float("nan"), torch.float64), _full((B,), -1, torch.int32), _full((B, CAP), 0, torch.int32)


def _bow_setup(ctx):
    ctx.bow_load(_voc())


def _bow_vector(ctx, state, B, stream):
    feat, n = _dev(_frames(B, 40 + B), np.array([(16, 1, 7, 0)[b % 4] for b in range(B)], np.int32))
    ids, vals, nw, word = _vector_tensors(B)
    return (lambda: ctx.bow_vector_batch_dev(feat, n, ids, vals, nw, word, stream=stream)), [ids, vals, nw, word]


def _query_setup(ctx):
    """an 8-frame database; the query vectors of every batch are made here, ahead of the calls under test (the vector's own scratch is not this case's block)"""
    import torch
    ctx.bow_load(_voc())
    db = api.BowDatabase(ctx, 8, CAP)
    vecs = {}
    for B, seed in ((8, 3),) + tuple((B, 90 + B) for B in BATCHES):
        feat, n = _dev(_frames(B, seed), np.full(B, CAP, np.int32))
        if B != 8:
            feat[:, :8] = vecs[8][0][torch.arange(B, device="cuda") % 8, :8]          # half of every query's features are a stored frame's: words in common
        ids, vals, nw, _ = _vector_tensors(B)
        ctx.bow_vector_batch_dev(feat, n, ids, vals, nw)
        vecs[B] = (feat, ids, vals, nw)
    db.add_batch_dev(*vecs[8][1:])
    torch.cuda.synchronize()
    return db, vecs


def _query(ctx, state, B, stream):
    import torch
    db, vecs = state
    _, ids, vals, nw = vecs[B]
    cf, cs = _full((B, 8), -7, torch.int32), _full((B, 8), -7, torch.int32)
    sc = _full((B, 8), float("nan"), torch.float64)
    nc, ms, sh = _full((B,), -1, torch.int32), _full((B,), -1, torch.int32), _full((B, 8), -1, torch.int32)
    return (lambda: db.query_batch_dev(ids, vals, nw, cf, cs, sc, nc, ms, ratio=0.3, min_words=2, sharing_t=sh, stream=stream)), [cf, cs, sc, nc, ms, sh]


def _query_stored(ctx, state, B, stream):
    """stored frames 7, 6, .. against their predecessors: the one caller of the dense query that carves two blocks (the gathered vectors, then the dense cells)"""
    import torch
    db, _ = state
    qframe, = _dev((7 - np.arange(B, dtype=np.int32)) % 8)
    cf, cs = _full((B, 8), -7, torch.int32), _full((B, 8), -7, torch.int32)
    sc = _full((B, 8), float("nan"), torch.float64)
    nc, ms, sh = _full((B,), -1, torch.int32), _full((B,), -1, torch.int32), _full((B, 8), -1, torch.int32)
    return (lambda: db.query_stored_batch_dev(qframe, cf, cs, sc, nc, ms, ratio=0.5, min_words=2, sharing_t=sh, stream=stream)), [cf, cs, sc, nc, ms, sh]


CASES = {
    "fundamental_ransac": (None, _fransac),
    "pnp_ransac": (None, _pnp),
    "frame_optimize": (None, _frame_optimize),
    "track_pose_opt": (None, _track_pose_opt),
    "bow_vector": (_bow_setup, _bow_vector),
    "bowdb_query": (_query_setup, _query),
    "bowdb_query_stored": (_query_setup, _query_stored),
}


def _run(setup, entry, sync_between):
    """the calls of BATCHES on a fresh context and a stream of the caller's -> per call the outputs as numpy arrays"""
    import torch
    ctx = api.Context()
    state = setup(ctx) if setup else None
    st = torch.cuda.Stream()
    calls = [entry(ctx, state, B, st.cuda_stream) for B in BATCHES]          # inputs and outputs of every call are on the device before the first one
    torch.cuda.synchronize()
    for call, _ in calls:
        call()
        if sync_between:
            st.synchronize()
    st.synchronize()
    out = [[t.cpu().numpy() for t in tensors] for _, tensors in calls]
    if state is not None and hasattr(state[0], "close"):
        state[0].close()                                                     # the database before its context
    ctx.close()
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_a_block_that_grows_under_queued_work_changes_no_result(name):
    setup, entry = CASES[name]
    got, want = _run(setup, entry, False), _run(setup, entry, True)
    for B, g, w in zip(BATCHES, got, want):
        if name == "fundamental_ransac":                                     # the lists are filtered in place: rows past a list's new count are not results
            np.testing.assert_array_equal(g[2], w[2])
            keep = np.arange(CAP)[None, :] < g[2][:, None]
            g, w = [g[0][keep], g[1][keep], g[2], g[3]], [w[0][keep], w[1][keep], w[2], w[3]]
        for k, (a, b) in enumerate(zip(g, w)):
            np.testing.assert_array_equal(a, b, err_msg=f"{name}: batch {B}, output {k}")
    # what keeps this from passing vacuously: the calls ran and wrote their outputs
    if name == "fundamental_ransac":
        assert all((g[2] >= 0).all() and (g[2] <= 12).all() and (g[3] != 7.0).any() for g in got)
    elif name in ("pnp_ransac", "frame_optimize", "track_pose_opt"):
        assert all((g[0] != 7.0).all() and (g[3] > -5).all() and (g[2] <= 1).all() for g in got)
        assert sum(int(g[3].sum()) for g in got) > 0
    elif name == "bow_vector":
        assert all((g[2][::4] > 0).all() and (g[2] >= 0).all() for g in got)
    elif name == "bowdb_query_stored":
        # tests/loopdet_ref.py::stored_queries on these frames: 7, 6, 5, 3, 3, 2, 1 candidates for frames 7 .. 1, max_sharing 6 .. 9; frame 0 has no predecessor
        for B, g in zip(BATCHES, got):
            qf = (7 - np.arange(B)) % 8
            assert (g[3][qf > 0] > 0).all() and (g[4][qf > 0] >= 2).all() and (g[3][qf == 0] == 0).all()
    else:
        assert all((g[3] > 0).all() and (g[4] >= 2).all() for g in got)
