"""Cost of the covisibility build on the device (kernels_covis.hip; include/airfe.h "Map-point ids and the covisibility build"), timed between device
events: medians over --reps timed calls after 3 warm-ups, with min / max.
  Scene     N stored frames of 300-400 rows.  Map points live in tracks about 8 frames long (4 .. 12) over neighbouring frames; every tenth frame also
            revisits a frame at least 50 frames back and takes 40 of its points; 5 % of the rows hold no point.
  Timed     build_covisibility_dev alone (the ids are in the database already, as they are after a map was loaded).
  Baseline  the caller's path without this entry, in the same run: Map::UpdateCovisibilityGraph's algorithm restated in C++ with std::map on ONE thread
            (per frame, per valid map point, per observer one map increment; the observers are the map's own std::map per point, built before the clock
            starts), flattened to CSR, then airfe_bowdb_set_covisibility.  Wall clock, since it is host work ending in a synchronous upload.
  Checked   before anything is timed: the device graph, the baseline's graph and tests/covis_ref.py (N <= 64 only: a Python loop) are equal.
    python tools/covis_timing.py [--reps R] [--quick] [--out FILE]        (on an MI355X; one JSON line per shape)"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from airslam_amd import api, weights  # noqa: E402
from bowdb_timing import timed  # noqa: E402

HOST = r'''
#include <stddef.h>
#include <stdint.h>
#include <map>
#include <vector>
struct Map {
  std::map<int, int> keyframes;                          // frame id -> frame (here: the same index)
  std::vector<std::map<int, int>> observers;             // per map point: frame id -> feature row
  std::vector<std::vector<int>> mappoints;               // per frame: the point at each feature row, -1 = none
};
extern "C" void* hm_create(const int32_t* ids, const int* n, int frames, int cap, int max_points) {
  Map* m = new Map();
  m->observers.resize(max_points);
  m->mappoints.resize(frames);
  for (int f = 0; f < frames; ++f) {
    m->keyframes[f] = f;
    m->mappoints[f].assign(ids + (size_t)f * cap, ids + (size_t)f * cap + n[f]);
    for (int i = 0; i < n[f]; ++i)
      if (m->mappoints[f][i] >= 0) m->observers[m->mappoints[f][i]][f] = i;
  }
  return m;
}
extern "C" void hm_destroy(void* h) { delete (Map*)h; }
// the graph as the reference holds it, then flattened for airfe_bowdb_set_covisibility; returns the number of entries (nbr / weight hold edge_cap)
extern "C" int hm_covisibility(void* h, int32_t* row_ptr, int32_t* nbr, int32_t* weight, int edge_cap) {
  Map* m = (Map*)h;
  std::map<int, std::map<int, int>> covisible;
  for (std::map<int, int>::const_iterator kf = m->keyframes.begin(); kf != m->keyframes.end(); ++kf) {
    const std::vector<int>& pts = m->mappoints[kf->second];
    for (size_t i = 0; i < pts.size(); ++i) {
      if (pts[i] < 0) continue;
      const std::map<int, int>& obs = m->observers[pts[i]];
      for (std::map<int, int>::const_iterator o = obs.begin(); o != obs.end(); ++o) {
        if (m->keyframes.find(o->first) == m->keyframes.end()) continue;
        std::map<int, int>& row = covisible[kf->first];
        std::map<int, int>::iterator it = row.find(o->first);
        if (it == row.end()) row[o->first] = 1; else it->second++;
      }
    }
  }
  int e = 0;
  const int frames = (int)m->mappoints.size();
  for (int f = 0; f < frames; ++f) {
    row_ptr[f] = e;
    std::map<int, std::map<int, int>>::const_iterator r = covisible.find(f);
    if (r == covisible.end()) continue;
    for (std::map<int, int>::const_iterator kv = r->second.begin(); kv != r->second.end(); ++kv, ++e)
      if (e < edge_cap) { nbr[e] = kv->first; weight[e] = kv->second; }
  }
  row_ptr[frames] = e;
  return e;
}
'''


def host_lib():
    d = tempfile.mkdtemp()
    with open(os.path.join(d, "h.cpp"), "w") as f:
        f.write(HOST)
    so = os.path.join(d, "libh.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-w", "-fPIC", "-shared", os.path.join(d, "h.cpp"), "-o", so], check=True)
    lib = C.CDLL(so)
    lib.hm_create.restype = C.c_void_p
    lib.hm_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.hm_destroy.argtypes = [C.c_void_p]
    lib.hm_covisibility.argtypes = [C.c_void_p] * 4 + [C.c_int]
    return lib


def scene(N, cap, seed):
    """-> ids [N][cap] i32, n [N] i32, max_points"""
    rng = np.random.default_rng(seed)
    M = N * 350 // 8 + 64
    start = rng.integers(-8, N, size=M)
    length = rng.integers(4, 13, size=M)
    order = np.argsort(start, kind="stable")
    start, length = start[order], length[order]
    ids = np.full((N, cap), -1, np.int32)
    n = np.zeros(N, np.int32)
    lo = 0
    for f in range(N):
        while lo < M and start[lo] + 12 < f:
            lo += 1
        hi = int(np.searchsorted(start, f, side="right"))
        live = np.nonzero(start[lo:hi] + length[lo:hi] > f)[0] + lo
        rows = rng.permutation(live)[:cap - 40]
        if f % 10 == 9 and f >= 60:                                                   # a revisit: 40 of the points of a frame at least 50 back
            g = int(rng.integers(0, f - 50))
            old = ids[g, :n[g]]
            old = old[old >= 0]
            rows = np.concatenate([rows, rng.choice(old, size=min(40, len(old)), replace=False)])
        rows = rows.astype(np.int32)
        rows[rng.random(len(rows)) < 0.05] = -1
        k = min(max(len(rows), 300), cap)                                             # 300 .. cap stored rows, the tail without a point
        ids[f, :len(rows)], n[f] = rows, k
    return ids, n, M


def one_shape(ctx, lib, N, cap, reps, emit):
    import torch
    import covis_ref as cr
    ids, n, P = scene(N, cap, N)
    st = torch.cuda.Stream()
    s = st.cuda_stream
    hm = lib.hm_create(ids.ctypes.data, n.ctypes.data, N, cap, P)
    cap_e = 1 << 24
    h_row, h_nbr, h_w = np.zeros(N + 1, np.int32), np.zeros(cap_e, np.int32), np.zeros(cap_e, np.int32)
    E = lib.hm_covisibility(hm, h_row.ctypes.data, h_nbr.ctypes.data, h_w.ctypes.data, cap_e)
    assert E <= cap_e
    h_nbr, h_w = h_nbr[:E].copy(), h_w[:E].copy()

    def database():
        db = api.BowDatabase(ctx, N, cap, keep_features=True)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")  # noqa: E731
        for b in range(0, N, 256):                                                    # (in slices: the feature rows are 400 KB a frame)
            k = min(256, N - b)
            db.add_batch_dev(z((k, cap), torch.int32), z((k, cap), torch.float64), z((k,), torch.int32), z((k, cap, 259), torch.float32),
                             torch.from_numpy(n[b:b + k].copy()).cuda())
        db.attach_map(E)
        torch.cuda.synchronize()
        return db
    dev, host = database(), database()
    dev.attach_point_ids(P)
    dev.set_point_ids(0, ids)
    info = torch.zeros(4, dtype=torch.int32, device="cuda")

    def build():
        dev.build_covisibility_dev(info, stream=s)

    def baseline():
        e = lib.hm_covisibility(hm, h_row.ctypes.data, h_nbr.ctypes.data, h_w.ctypes.data, E)
        host.set_covisibility(h_row, h_nbr[:e], h_w[:e])
    build()
    baseline()
    torch.cuda.synchronize()
    a, b = dev.get_covisibility(E), host.get_covisibility(E)
    hi = info.cpu().numpy().tolist()
    assert hi[:2] == [0, E] and hi[3] == 0, hi
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), "the device build and the std::map baseline disagree"
    if N <= 64:
        want = cr.build(ids, n, N, N, P)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, want[:3])) and hi == want[3], "the device build and tests/covis_ref.py disagree"
    td = timed(build, st, reps)
    wall = []
    for r in range(reps + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        build()
        st.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    wall = sorted(wall[3:])
    base = []
    for r in range(reps + 3):
        t0 = time.perf_counter()
        baseline()
        base.append((time.perf_counter() - t0) * 1e3)
    base = sorted(base[3:])
    mmm = lambda v: (round(float(np.median(v)), 4), round(v[0], 4), round(v[-1], 4))  # noqa: E731
    emit(what="bowdb_build_covisibility_dev", N=N, cap=cap, rows_mean=float(n.mean()), max_points=P, valid_rows=hi[2], edges=E,
         weight_above_10=int((a[2] > 10).sum()), reps=reps, device_ms_median_min_max=td, device_wall_ms_median_min_max=mmm(wall),
         baseline_ms_median_min_max=mmm(base), ratio_device_over_baseline=round(td[0] / mmm(base)[0], 6),
         ratio_device_wall_over_baseline=round(mmm(wall)[0] / mmm(base)[0], 6))
    lib.hm_destroy(hm)
    dev.close()
    host.close()


def main(reps=20, quick=False, out=None):
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)
    ctx = api.Context(max_batch=1, max_keypoints=400)
    ctx.bow_load(weights.synthetic_vocabulary(1234, k=10, L=4))
    lib = host_lib()
    for N in ((64, 256) if quick else (64, 1024, 4096)):
        one_shape(ctx, lib, N, 400, reps, emit)
    ctx.close()
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    arg = lambda k, d: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else d  # noqa: E731
    main(int(arg("--reps", 20)), "--quick" in sys.argv, arg("--out", None))
