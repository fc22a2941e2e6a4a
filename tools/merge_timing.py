"""Cost of the map-point merge on the device (kernels_merge.hip; include/airfe.h "Map-point merge"), timed between device events: medians over --reps
timed calls after 3 warm-ups, with min / max.
  Scene     tools/triangulate_timing.py's: N stored frames of `cap` = 400 rows along a path, map points in tracks of 4 .. 8 consecutive frames, positions
            from retriangulate_dev.  The frames of the upper half are the queries' frames: 30 % of their rows lose their id (adoption).  Q stage-0 queries,
            each from a frame of the upper half to a frame of the lower half, 250 list entries of random rows inside the counts, 80 % of them inliers:
            about 200 live entries a query.  Rlq = I, tlq random (the epipolar gate of the rows without a position).
  Timed     merge_points_dev on the pair list the loop form derives (A, B of every live pair entry); loop_merge_batch_dev; loop_close_dev (the same, then
            retriangulate_dev(only_missing) and build_covisibility_dev).  The merge changes the tables, so every call, warm-ups included, runs on tables
            restored by two device-to-device copies queued in front of the first event.
  Baseline  the caller's path without these entries, in the same run: merge_build_host (merge_core.h, g++ -O2 -ffp-contract=off) on ONE thread over the
            same tables, then airfe_bowdb_set_point_ids and airfe_bowdb_set_points.  Wall clock, since it is host work ending in synchronous uploads.
  Checked   before anything is timed: device outputs, id table and point table equal the host statement's byte for byte.
    python tools/merge_timing.py [--reps R] [--quick] [--out FILE]        (on an MI355X; one JSON line per shape)"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from airslam_amd import api, weights  # noqa: E402
from triangulate_timing import CAM, scene  # noqa: E402

MCAP, ENTRIES = 400, 250
HOST = r'''
#include "merge_core.h"
extern "C" void host_merge(int32_t* point_id, double* xyz, const float* feat, const int* n, int size, int cap, int feat_dim, int max_points,
                           const int32_t* qframe, int Q, const int* stage, const int32_t* loop, const double* Rlq, const double* tlq, const uint8_t* mask,
                           const int32_t* idx, int mcap, const int* nmatch, const double* cam, int32_t* map, int32_t* info) {
  MergeTables t;
  t.point_id = point_id; t.xyz = xyz; t.feat = feat; t.n = n; t.size = size; t.cap = cap; t.feat_dim = feat_dim; t.max_points = max_points;
  MergeLoop l;
  l.qframe = qframe; l.Q = Q; l.stage = stage; l.loop = loop; l.Rlq = Rlq; l.tlq = tlq; l.mask = mask; l.idx = idx; l.mcap = mcap; l.nmatch = nmatch;
  for (int k = 0; k < 4; ++k) l.cam[k] = cam[k];
  merge_build_host(t, l, size, map, info);
}
// the pair list of the loop form: (A, B) of every live pair entry -> the pairs written
extern "C" int host_pairs(int32_t* point_id, double* xyz, const float* feat, const int* n, int size, int cap, int feat_dim, int max_points,
                          const int32_t* qframe, int Q, const int* stage, const int32_t* loop, const double* Rlq, const double* tlq, const uint8_t* mask,
                          const int32_t* idx, int mcap, const int* nmatch, const double* cam, int32_t* pairs) {
  MergeTables t;
  t.point_id = point_id; t.xyz = xyz; t.feat = feat; t.n = n; t.size = size; t.cap = cap; t.feat_dim = feat_dim; t.max_points = max_points;
  MergeLoop l;
  l.qframe = qframe; l.Q = Q; l.stage = stage; l.loop = loop; l.Rlq = Rlq; l.tlq = tlq; l.mask = mask; l.idx = idx; l.mcap = mcap; l.nmatch = nmatch;
  for (int k = 0; k < 4; ++k) l.cam[k] = cam[k];
  int P = 0;
  for (int q = 0; q < Q; ++q)
    for (int e = 0, ne = clamp_count(nmatch[q], mcap); e < ne && stage[q] == 0; ++e) {
      int A, B, row;
      if (mg_entry(t, l, q, e, &A, &B, &row) == MG_PAIR) { pairs[2 * P] = A; pairs[2 * P + 1] = B; ++P; }
    }
  return P;
}
'''


def host_lib():
    d = tempfile.mkdtemp()
    with open(os.path.join(d, "h.cpp"), "w") as f:
        f.write(HOST)
    so = os.path.join(d, "libh.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-w", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "airslam_amd", "csrc"),
                    os.path.join(d, "h.cpp"), "-o", so], check=True)
    lib = C.CDLL(so)
    head = [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_int] + [C.c_void_p] * 2
    lib.host_merge.argtypes = head + [C.c_void_p] * 2
    lib.host_pairs.argtypes = head + [C.c_void_p]
    lib.host_merge.restype = None
    return lib


def queries(N, n, Q, seed):
    rng = np.random.default_rng(seed)
    half = N // 2
    qframe = (half + np.arange(Q) % (N - half)).astype(np.int32)
    loop = rng.integers(0, half, Q).astype(np.int32)
    idx = np.zeros((Q, MCAP, 2), np.int32)
    idx[:, :, 0] = (rng.random((Q, MCAP)) * np.maximum(n[qframe], 1)[:, None]).astype(np.int32)
    idx[:, :, 1] = (rng.random((Q, MCAP)) * np.maximum(n[loop], 1)[:, None]).astype(np.int32)
    mask = (rng.random((Q, MCAP)) < 0.8).astype(np.uint8)
    Rlq = np.tile(np.eye(3).reshape(9), (Q, 1))
    tlq = rng.uniform(-0.5, 0.5, (Q, 3))
    return dict(qframe=qframe, stage=np.zeros(Q, np.int32), loop=loop, Rlq=Rlq, tlq=tlq, mask=mask, idx=idx, nmatch=np.full(Q, ENTRIES, np.int32))


def timed_restored(fn, restore, st, reps, warm=3):
    """bowdb_timing.timed with restore() queued in front of every call's first event"""
    import torch
    for _ in range(warm):
        restore()
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        restore()
        a.record(st)
        fn()
        b.record(st)
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return round(float(np.median(ms)), 4), round(ms[0], 4), round(ms[-1], 4)


def one_shape(ctx, lib, N, cap, P, Q, reps, emit):
    import torch
    xy3, n, pose, ids = scene(N, cap, P, N)
    rng = np.random.default_rng(N + 1)
    ids[N // 2:][rng.random((N - N // 2, cap)) < 0.3] = -1
    st = torch.cuda.Stream()
    s = st.cuda_stream
    db = api.BowDatabase(ctx, N, cap, keep_features=True)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")  # noqa: E731
    for b in range(0, N, 256):
        k = min(256, N - b)
        feat = z((k, cap, 259), torch.float32)
        feat[:, :, 1:3] = torch.from_numpy(xy3[b:b + k, :, 1:3].copy()).cuda()
        db.add_batch_dev(z((k, cap), torch.int32), z((k, cap), torch.float64), z((k,), torch.int32), feat, torch.from_numpy(n[b:b + k].copy()).cuda())
    db.attach_map(N * 96)
    db.set_poses(0, pose)
    db.attach_point_ids(P)
    db.set_point_ids(0, ids)
    db.attach_triangulation()
    db.attach_merge()
    xyz, status, nobs = z((P, 3), torch.float64), z((P,), torch.int32), z((P,), torch.int32)
    tinfo, written, cinfo, minfo, mp = z((4,), torch.int32), z((1,), torch.int32), z((4,), torch.int32), z((8,), torch.int32), z((P,), torch.int32)
    db.set_points(0, np.full((N, cap, 3), np.nan))
    db.retriangulate_dev(CAM, xyz, status, nobs, tinfo, written, stream=s)                # the scene's positions
    torch.cuda.synchronize()
    points = db.get_points(0, N)
    ids_t, points_t = torch.from_numpy(ids).cuda(), torch.from_numpy(points).cuda()
    L = queries(N, n, Q, N + 2)
    lt = [torch.from_numpy(np.ascontiguousarray(L[k])).cuda() for k in ("qframe", "stage", "loop", "Rlq", "tlq", "mask", "idx", "nmatch")]
    cam = np.array(CAM, np.float64)
    h_ids, h_points, h_map, h_info = ids.copy(), points.copy(), np.zeros(P, np.int32), np.zeros(8, np.int32)

    def host_args(i, p):
        return (i.ctypes.data, p.ctypes.data, xy3.ctypes.data, n.ctypes.data, N, cap, 3, P, L["qframe"].ctypes.data, Q, L["stage"].ctypes.data,
                L["loop"].ctypes.data, L["Rlq"].ctypes.data, L["tlq"].ctypes.data, L["mask"].ctypes.data, L["idx"].ctypes.data, MCAP, L["nmatch"].ctypes.data,
                cam.ctypes.data)
    pairs = np.zeros((Q * ENTRIES, 2), np.int32)
    npairs = lib.host_pairs(*host_args(h_ids, h_points), pairs.ctypes.data)
    pairs_t = torch.from_numpy(pairs[:npairs].copy()).cuda()

    def restore():
        db.set_point_ids_dev(0, ids_t, stream=s)
        db.set_points_dev(0, points_t, stream=s)

    def pair_form():
        db.merge_points_dev(pairs_t, mp, minfo, stream=s)

    def loop_form():
        db.loop_merge_batch_dev(CAM, *lt, mp, minfo, stream=s)

    def close_form():
        db.loop_close_dev(CAM, *lt, mp, minfo, xyz, status, nobs, tinfo, written, cinfo, stream=s)

    def baseline():
        lib.host_merge(*host_args(h_ids, h_points), h_map.ctypes.data, h_info.ctypes.data)
        db.set_point_ids(0, h_ids)
        db.set_points(0, h_points)
    restore()
    loop_form()
    torch.cuda.synchronize()
    d_ids, d_points = db.get_point_ids(0, N), db.get_points(0, N)
    baseline()
    eq = lambda a, b: np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))  # noqa: E731
    assert eq(mp.cpu().numpy(), h_map) and minfo.cpu().numpy().tolist() == h_info.tolist(), "the device and the host statement disagree"
    assert eq(d_ids, h_ids) and eq(d_points, h_points), "the merged tables disagree"
    t_pairs = timed_restored(pair_form, restore, st, reps)
    t_loop = timed_restored(loop_form, restore, st, reps)
    t_close = timed_restored(close_form, restore, st, reps)
    hreps = reps if N <= 64 else max(3, reps // 4)
    base = []
    for r in range(hreps + 1):
        np.copyto(h_ids, ids)
        np.copyto(h_points, points)
        t0 = time.perf_counter()
        baseline()
        base.append((time.perf_counter() - t0) * 1e3)
    base = sorted(base[1:])
    mmm = lambda v: (round(float(np.median(v)), 4), round(v[0], 4), round(v[-1], 4))  # noqa: E731
    emit(what="bowdb_loop_merge_batch_dev", N=N, cap=cap, max_points=P, Q=Q, mcap=MCAP, entries=Q * ENTRIES, pairs=int(npairs), info=h_info.tolist(), reps=reps,
         merge_points_ms_median_min_max=t_pairs, loop_merge_ms_median_min_max=t_loop, loop_close_ms_median_min_max=t_close, host_reps=hreps,
         host_merge_upload_ms_median_min_max=mmm(base), ratio_device_over_host=round(t_loop[0] / mmm(base)[0], 6))
    db.close()


def main(reps=20, quick=False, out=None):
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)
    ctx = api.Context(max_batch=1, max_keypoints=400)
    ctx.bow_load(weights.synthetic_vocabulary(1234, k=10, L=4))
    lib = host_lib()
    for N, P, Q in (((64, 4000, 64), (256, 20000, 256)) if quick else ((64, 4000, 64), (1024, 100000, 1024), (4096, 1000000, 4096))):
        one_shape(ctx, lib, N, 400, P, Q, reps, emit)
    ctx.close()
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    arg = lambda k, d: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else d  # noqa: E731
    main(int(arg("--reps", 20)), "--quick" in sys.argv, arg("--out", None))
