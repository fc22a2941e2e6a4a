"""Cost of batched loop detection on the device (kernels_loopdet.hip; include/airfe.h "Stored queries against their predecessors", "Loop detection
composite"), timed with device events.  Medians over --reps timed calls after 3 warm-ups, with min / max.  Neither comparison is the code under test:
  (a) query_stored_batch_dev over N stored frames in ONE call (Q = N, the covisible frames dropped) against the only way the entries that existed before
      offer: a second database grown one frame at a time — query_batch_dev with Q = 1 and a bit row of the frame's covisible frames, then add_batch_dev —
      N times, on the same stream, nothing downloaded in between.  Every frame's candidates are compared byte for byte before anything is timed.
  (b) loop_detect_batch_dev at Q = 4, K = 5 on the scene of tests/test_gpu_loopdet.py against the same chain by hand with its host round trips: the stored
      query, the odometry and max_dist on the host, group_dev, match_candidates_batch_dev on the gathered rows, the lists downloaded, a numpy gather,
      frame_optimize_batch_dev, the poses downloaded, the relative pose on the host.  Poses, loop frames and counts are compared before anything is timed.
    python tools/loopdet_timing.py [--reps R] [--quick] [--out FILE]        (on an MI355X; one JSON line per measurement)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from airslam_amd import api  # noqa: E402
from bowdb_timing import timed, vectors  # noqa: E402
from reloc_timing import covisibility  # noqa: E402


def stored_query(ctx, N, cap, reps, emit):
    import torch
    st = torch.cuda.Stream()
    s = st.cuda_stream
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a.view(np.int32) if a.dtype == np.uint32 else a)).cuda()  # noqa: E731
    base_ids, base_vals, base_nw = vectors(N // 2, cap, N)
    ids, vals, nw = vectors(N, cap, 3 * N, revisit_of=(base_ids, base_nw))           # every second frame revisits an earlier place: busy candidate lists
    cov = covisibility(N, N)
    words = (N + 31) // 32
    bits = np.zeros((N, words), np.uint32)
    for f in range(N):
        for g in cov[1][cov[0][f]:cov[0][f + 1]]:
            bits[f, g >> 5] |= np.uint32(1) << np.uint32(g & 31)
    ti, tv, tn, tb = dev(ids), dev(vals), dev(nw), dev(bits)
    feat, fn = torch.zeros((N, cap, 259), dtype=torch.float32, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda")
    i32 = lambda shape: torch.zeros(shape, dtype=torch.int32, device="cuda")  # noqa: E731
    f64 = lambda shape: torch.zeros(shape, dtype=torch.float64, device="cuda")  # noqa: E731

    def database(count):
        db = api.BowDatabase(ctx, N, cap, keep_features=True)
        db.attach_map(len(cov[1]))
        db.set_covisibility(*cov)
        if count:
            db.add_batch_dev(ti[:count], tv[:count], tn[:count], feat[:count], fn[:count])
        torch.cuda.synchronize()
        return db
    full, grown = database(N), database(0)
    qframe = torch.arange(N, dtype=torch.int32, device="cuda")
    a = dict(cf=i32((N, N)), cs=i32((N, N)), sc=f64((N, N)), nc=i32((N,)), ms=i32((N,)))
    b = dict(cf=i32((N, N)), cs=i32((N, N)), sc=f64((N, N)), nc=i32((N,)), ms=i32((N,)))

    def one_call():
        full.query_stored_batch_dev(qframe, a["cf"], a["cs"], a["sc"], a["nc"], a["ms"], ratio=0.5, exclude_covisible=True, stream=s)

    def incremental():
        grown.clear()
        for f in range(N):
            grown.query_batch_dev(ti[f:f + 1], tv[f:f + 1], tn[f:f + 1], b["cf"][f:f + 1], b["cs"][f:f + 1], b["sc"][f:f + 1], b["nc"][f:f + 1], b["ms"][f:f + 1],
                                  ratio=0.5, exclude_t=tb[f:f + 1], stream=s)
            grown.add_batch_dev(ti[f:f + 1], tv[f:f + 1], tn[f:f + 1], feat[f:f + 1], fn[f:f + 1], stream=s)
    with torch.cuda.stream(st):
        one_call()
        incremental()
    torch.cuda.synchronize()
    ha, hb = {k: v.cpu().numpy() for k, v in a.items()}, {k: v.cpu().numpy() for k, v in b.items()}
    assert (ha["nc"] == hb["nc"]).all() and (ha["ms"] == hb["ms"]).all(), "the stored query and the incremental database disagree"
    for f in range(N):
        k = int(ha["nc"][f])
        assert all(ha[x][f, :k].tobytes() == hb[x][f, :k].tobytes() for x in ("cf", "cs", "sc")), f
    t1 = timed(one_call, st, reps)
    t2 = timed(incremental, st, reps)
    emit(what="bowdb_query_stored_batch_dev", N=N, Q=N, words_per_vector=float(nw.mean()), exclude_covisible=True, reps=reps, one_call_ms_median_min_max=t1,
         incremental_ms_median_min_max=t2, ratio_one_call_over_incremental=round(t1[0] / t2[0], 5), candidates_mean=float(ha["nc"].mean()),
         candidates_max=int(ha["nc"].max()))
    full.close()
    grown.close()


def composite(reps, emit):
    import torch
    import loopdet_ref as lr
    import test_gpu_loopdet as T
    ctx, K, CAP, CAM, THR = T._ctx(), T.K, T.CAP, T.CAM, T.THR
    sc_ = T._scene()
    db = T._scene_db(sc_)
    qf, Q, N = sc_["qframes"], sc_["Q"], sc_["N"]
    st = torch.cuda.Stream()
    s = st.cuda_stream
    o = T._loop_buffers(Q)
    qframe = T._up(np.asarray(qf, np.int32))

    def one_call():
        db.loop_detect_batch_dev(qframe, CAM, THR, o["ok"], o["stage"], o["loop"], o["Twq"], o["Rlq"], o["tlq"], o["num"], o["mask"], o["idx"], o["score"],
                                 o["nmatch"], K=K, stream=s)
    i32 = lambda shape: torch.zeros(shape, dtype=torch.int32, device="cuda")  # noqa: E731
    f64 = lambda shape: torch.zeros(shape, dtype=torch.float64, device="cuda")  # noqa: E731
    cf, cs, sc, nc, ms = i32((Q, N)), i32((Q, N)), f64((Q, N)), i32((Q,)), i32((Q,))
    gf, gs, ng, gst = i32((Q, K)), f64((Q, K)), i32((Q,)), i32((Q,))
    best, idx, msc, nm = i32((Q,)), i32((Q, CAP, 2)), torch.zeros((Q, CAP), dtype=torch.float32, device="cuda"), i32((Q,))
    T2, inl, num = f64((Q, 16)), torch.zeros((Q, CAP), dtype=torch.uint8, device="cuda"), i32((Q,))
    ft, nt = T._up(sc_["dbf"]), T._up(sc_["dn"])
    poses, xyz, ur, dbf = sc_["poses"], sc_["xyz"], sc_["ur"], sc_["dbf"]
    keep = {}

    def by_hand():
        with torch.cuda.stream(st):
            db.query_stored_batch_dev(qframe, cf, cs, sc, nc, ms, ratio=0.5, exclude_covisible=True, stream=s)
            pos = poses.reshape(-1, 4, 4)[:, :3, 3]
            odom = lr.odometry(pos)
            qpos, md = torch.from_numpy(pos[qf].copy()).cuda(), torch.from_numpy(np.array([odom[f] * 0.03 for f in qf])).cuda()
            db.group_dev(1, cf, sc, nc, gf, gs, ng, gst, qpos_t=qpos, max_dist_t=md, stream=s)
            db.match_candidates_batch_dev(ft[qframe.long()], nt[qframe.long()], gf, best, idx, msc, nm, stream=s)
            hb, hi, hm, hnc, hst, hng = best.cpu().numpy(), idx.cpu().numpy(), nm.cpu().numpy(), nc.cpu().numpy(), gst.cpu().numpy(), ng.cpu().numpy()      # round trip 1
            X, obs, n = np.zeros((Q, CAP, 3)), np.zeros((Q, CAP, 3)), np.zeros(Q, np.int32)
            for q in range(Q):
                if lr.stage_before(int(hnc[q]), int(hst[q]), int(hng[q]), int(hb[q]), N, int(hm[q])):
                    continue
                li = hi[q, :hm[q]]
                P = xyz[hb[q], li[:, 1]]
                ok = ~np.isnan(P[:, 0])
                k = int(ok.sum())
                u = ur[qf[q], li[ok, 0]]
                X[q, :k], obs[q, :k, :2], obs[q, :k, 2] = P[ok], dbf[qf[q], li[ok, 0], 1:3], np.where(u > 0, u, -1.0)
                n[q] = k if k >= 50 else 0
            db._ctx.frame_optimize_batch_dev(torch.from_numpy(X).cuda(), torch.from_numpy(obs).cuda(), torch.from_numpy(n).cuda(),
                                             torch.from_numpy(poses[qf].copy()).cuda(), CAM, THR, T2, inl, num, stream=s)
            hT = T2.cpu().numpy()                                                                      # round trip 2
            keep.update(Twq=hT, loop=hb, num=num.cpu().numpy(), rel=[lr.relative_pose(poses[hb[q]], hT[q]) for q in range(Q)])
    one_call()
    by_hand()
    torch.cuda.synchronize()
    g = {k: v.cpu().numpy() for k, v in o.items()}
    assert g["loop"].tolist() == keep["loop"].tolist() == [1, 3, 5, 7] and g["stage"].tolist() == [0] * Q, (g["loop"], g["stage"])
    assert g["Twq"].tobytes() == keep["Twq"].tobytes() and g["num"].tolist() == keep["num"].tolist(), "the composite and the chain by hand disagree"
    for q in range(Q):
        assert g["Rlq"][q].tobytes() == np.array(keep["rel"][q][0]).tobytes() and g["tlq"][q].tobytes() == np.array(keep["rel"][q][1]).tobytes(), q
    tc = timed(one_call, st, reps)
    tb = timed(by_hand, st, reps)
    emit(what="loop_detect_batch_dev", Q=Q, K=K, N=N, n=CAP, reps=reps, composite_ms_median_min_max=tc, by_hand_ms_median_min_max=tb,
         ratio_composite_over_by_hand=round(tc[0] / tb[0], 4), stages=g["stage"].tolist(), num=g["num"].tolist(), nmatch=g["nmatch"].tolist())
    db.close()
    return ctx


def main(reps=20, quick=False, out=None):
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)
    ctx = composite(reps, emit)
    stored_query(ctx, 256 if quick else 1024, 400, reps, emit)
    ctx.close()
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    arg = lambda k, d: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else d  # noqa: E731
    main(int(arg("--reps", 20)), "--quick" in sys.argv, arg("--out", None))
