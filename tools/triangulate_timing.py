"""Cost of the map-point triangulation on the device (kernels_triangulate.hip; include/airfe.h "Map-point triangulation"), timed between device events:
medians over --reps timed calls after 3 warm-ups, with min / max.
  Scene     N stored frames of `cap` = 400 rows along a path; map points live in tracks of 4 .. 8 consecutive frames (about 6 observers per OBSERVED
            point), keypoints = the projections with 0.3 px of noise as float32; 5 % of the rows hold no point.  max_points is the map's size as asked
            for (4 k / 100 k / 1 M): what the per-point passes scan.  N x cap rows cannot hold six observations of that many points at the two larger
            shapes, so the points actually observed are fewer (`points_observed` on the line) and the rest of the ids have no observer (status -1).
  Timed     triangulate_points_dev alone; retriangulate_dev (the same + fill_points_dev); both on one stream, ids, rows and poses in the database already.
  Baseline  the caller's path without these entries, in the same run: triangulate_build_host (triangulate_core.h, g++ -O2 -ffp-contract=off) on ONE
            thread over the same tables, the point table filled on the host in C++, then airfe_bowdb_set_points.  Wall clock, since it is host work ending
            in a synchronous upload.
  Checked   before anything is timed: the device outputs equal the host statement's byte for byte, and so do the two point tables.
    python tools/triangulate_timing.py [--reps R] [--quick] [--out FILE]        (on an MI355X; one JSON line per shape)"""
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
from bowdb_timing import timed  # noqa: E402

CAM = (400.0, 410.0, 320.0, 240.0)
HOST = r'''
#include "triangulate_core.h"
extern "C" int host_build(const float* feat, int feat_dim, const int* n, const double* pose, const int32_t* point_id, int size, int cap, int max_points,
                          const double* cam, int min_observers, double* xyz, int32_t* status, int32_t* nobs, int32_t* info) {
  double cami[4];
  if (!tr_cam(cam, cami)) return 1;
  triangulate_build_host(feat, feat_dim, n, pose, point_id, size, cap, max_points, cami, min_observers, xyz, status, nobs, info);
  return 0;
}
// airfe_bowdb_fill_points_dev on the host: points [size][cap][3]; returns the rows written
extern "C" int host_fill(const int* n, const int32_t* point_id, int size, int cap, int max_points, const double* xyz, const int32_t* status, int only_missing,
                         double* points) {
  int written = 0;
  for (int f = 0; f < size; ++f) {
    const int nf = clamp_count(n[f], cap);
    for (int i = 0; i < nf; ++i) {
      int ig;
      const int m = cv_row_id(point_id + (size_t)f * cap, i, nf, max_points, &ig);
      double* p = points + ((size_t)f * cap + i) * 3;
      if (m < 0 || status[m] != TR_OK || (only_missing && p[0] == p[0])) continue;
      p[0] = xyz[3 * (size_t)m]; p[1] = xyz[3 * (size_t)m + 1]; p[2] = xyz[3 * (size_t)m + 2];
      ++written;
    }
  }
  return written;
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
    lib.host_build.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 3 + [C.c_void_p, C.c_int] + [C.c_void_p] * 4
    lib.host_fill.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    return lib


def scene(N, cap, P, seed):
    """-> xy3 f32 [N][cap][3] (x, y at columns 1, 2), n [N], pose [N][16], ids [N][cap]"""
    rng = np.random.default_rng(seed)
    M = min(P, int(N * cap * 0.95 / 6))                                                # the points that get observers: ids 0 .. M - 1 of P
    length = rng.integers(4, 9, size=M)
    start = rng.integers(-3, N - 1, size=M)
    pt = np.repeat(np.arange(M), length)
    fr = np.repeat(start, length) + (np.arange(len(pt)) - np.repeat(np.cumsum(length) - length, length))
    keep = (fr >= 0) & (fr < N)
    pt, fr = pt[keep], fr[keep]
    order = rng.permutation(len(pt))                                                  # rows of a frame in no particular order
    pt, fr = pt[order], fr[order]
    order = np.argsort(fr, kind="stable")
    pt, fr = pt[order], fr[order]
    first = np.searchsorted(fr, np.arange(N))
    row = np.arange(len(fr)) - first[fr]
    keep = row < cap
    pt, fr, row = pt[keep], fr[keep], row[keep]
    yaw = 0.2 * np.sin(0.05 * np.arange(N))
    pose = np.tile(np.eye(4), (N, 1, 1))
    pose[:, 0, 0], pose[:, 0, 2], pose[:, 2, 0], pose[:, 2, 2] = np.cos(yaw), np.sin(yaw), -np.sin(yaw), np.cos(yaw)
    pose[:, 0, 3], pose[:, 1, 3] = 0.05 * np.arange(N), 0.1 * np.sin(0.3 * np.arange(N))
    s0 = np.clip(start, 0, N - 1)
    X = pose[s0, :3, 3] + np.einsum("mij,mj->mi", pose[s0, :3, :3], np.stack([rng.uniform(-3, 3, M), rng.uniform(-2, 2, M), rng.uniform(4, 10, M)], 1))
    Xc = np.einsum("kji,kj->ki", pose[fr, :3, :3], X[pt] - pose[fr, :3, 3])
    u = CAM[0] * Xc[:, 0] / Xc[:, 2] + CAM[2] + rng.normal(0, 0.3, len(pt))
    v = CAM[1] * Xc[:, 1] / Xc[:, 2] + CAM[3] + rng.normal(0, 0.3, len(pt))
    ids = np.full((N, cap), -1, np.int32)
    xy3 = np.zeros((N, cap, 3), np.float32)
    ids[fr, row] = np.where(rng.random(len(pt)) < 0.05, -1, pt).astype(np.int32)
    xy3[fr, row, 1], xy3[fr, row, 2] = u, v
    n = np.bincount(fr, minlength=N).astype(np.int32)
    return xy3, n, np.ascontiguousarray(pose.reshape(N, 16)), ids


def one_shape(ctx, lib, N, cap, P, reps, emit):
    import torch
    xy3, n, pose, ids = scene(N, cap, P, N)
    st = torch.cuda.Stream()
    s = st.cuda_stream
    db = api.BowDatabase(ctx, N, cap, keep_features=True)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")  # noqa: E731
    for b in range(0, N, 256):                                                        # (in slices: the feature rows are 400 KB a frame)
        k = min(256, N - b)
        feat = z((k, cap, 259), torch.float32)
        feat[:, :, 1:3] = torch.from_numpy(xy3[b:b + k, :, 1:3].copy()).cuda()
        db.add_batch_dev(z((k, cap), torch.int32), z((k, cap), torch.float64), z((k,), torch.int32), feat, torch.from_numpy(n[b:b + k].copy()).cuda())
    db.attach_map(1)
    db.set_poses(0, pose)
    db.attach_point_ids(P)
    db.set_point_ids(0, ids)
    db.attach_triangulation()
    xyz, status, nobs = z((P, 3), torch.float64), z((P,), torch.int32), z((P,), torch.int32)
    info, written = z((4,), torch.int32), z((1,), torch.int32)
    cam = np.array(CAM, np.float64)
    h_xyz, h_status, h_nobs, h_info = np.zeros((P, 3)), np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros(4, np.int32)
    nan_table = np.full((N, cap, 3), np.nan)
    h_points = nan_table.copy()

    def tri():
        db.triangulate_points_dev(CAM, xyz, status, nobs, info, stream=s)

    def both():
        db.retriangulate_dev(CAM, xyz, status, nobs, info, written, stream=s)

    def baseline():
        lib.host_build(xy3.ctypes.data, 3, n.ctypes.data, pose.ctypes.data, ids.ctypes.data, N, cap, P, cam.ctypes.data, 2, h_xyz.ctypes.data,
                       h_status.ctypes.data, h_nobs.ctypes.data, h_info.ctypes.data)
        w = lib.host_fill(n.ctypes.data, ids.ctypes.data, N, cap, P, h_xyz.ctypes.data, h_status.ctypes.data, 0, h_points.ctypes.data)
        db.set_points(0, h_points)
        return w
    db.set_points(0, nan_table)                                                       # (the same NaN bytes on both sides of the comparison)
    both()
    torch.cuda.synchronize()
    d_points = db.get_points(0, N)
    h_written = baseline()
    eq = lambda a, b: np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))  # noqa: E731
    assert eq(xyz.cpu().numpy(), h_xyz) and eq(status.cpu().numpy(), h_status) and eq(nobs.cpu().numpy(), h_nobs), "the device and the host statement disagree"
    assert info.cpu().numpy().tolist() == h_info.tolist() and int(written.item()) == h_written and eq(d_points, h_points), "the point tables disagree"
    t_tri = timed(tri, st, reps)
    t_both = timed(both, st, reps)
    hreps = reps if N <= 64 else max(3, reps // 4)
    base = []
    for r in range(hreps + 1):
        t0 = time.perf_counter()
        baseline()
        base.append((time.perf_counter() - t0) * 1e3)
    base = sorted(base[1:])
    mmm = lambda v: (round(float(np.median(v)), 4), round(v[0], 4), round(v[-1], 4))  # noqa: E731
    emit(what="bowdb_triangulate_points_dev", N=N, cap=cap, max_points=P, rows=int(n.sum()), points_observed=int(h_info[1]), points_ok=int(h_info[0]),
         status_2=int(h_info[2]), status_3=int(h_info[3]), observers_mean=round(float(h_nobs[h_nobs > 0].mean()), 3), observers_max=int(h_nobs.max()),
         rows_filled=h_written, reps=reps, triangulate_ms_median_min_max=t_tri, triangulate_and_fill_ms_median_min_max=t_both, host_reps=hreps,
         host_build_fill_upload_ms_median_min_max=mmm(base), ratio_device_over_host=round(t_both[0] / mmm(base)[0], 6))
    db.close()


def main(reps=20, quick=False, out=None):
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)
    ctx = api.Context(max_batch=1, max_keypoints=400)
    ctx.bow_load(weights.synthetic_vocabulary(1234, k=10, L=4))
    lib = host_lib()
    for N, P in (((64, 4000), (256, 20000)) if quick else ((64, 4000), (1024, 100000), (4096, 1000000))):
        one_shape(ctx, lib, N, 400, P, reps, emit)
    ctx.close()
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    arg = lambda k, d: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else d  # noqa: E731
    main(int(arg("--reps", 20)), "--quick" in sys.argv, arg("--out", None))
