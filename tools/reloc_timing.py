"""Cost of relocalisation to the pose on the device (kernels_bowgroup.hip; include/airfe.h "Grouping", "Relocalisation composite"), timed with device
events: the grouping entry alone for N stored frames x Q queries on the query mix of tools/bowdb_timing.py (an unrelated query keeps nearly every frame:
the grouping's worst case), and the composite at Q = 4, K = 3.  Medians over --reps timed calls after 3 warm-ups, with min / max.
The comparison is NOT the code under test: BASELINE is the same chain built only from the entries that existed before the composite — vector, query, the
candidate list downloaded, the grouping on the HOST (the reference's algorithm in C++ with std::map / std::set, below; checked byte for byte against the
device's groups before it is timed), match_candidates, the list downloaded, a host gather, pnp_ransac_batch_dev, frame_optimize_batch_dev — timed between
the same events, its two synchronising round trips included.
    python tools/reloc_timing.py [--reps R] [--quick] [--out FILE]        (on an MI355X; one JSON line per measurement)"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from airslam_amd import api, weights  # noqa: E402
from bowdb_timing import timed, vectors  # noqa: E402

HOST = r'''
#include <algorithm>
#include <map>
#include <set>
#include <vector>
struct Group { std::set<int> frames; double score = 0; };
// map_user.cc:177-270, 331, 347-363 with frame indices for FramePtr; covisibility as std::map per frame
extern "C" int hg_reloc(const int* frame, const double* score, int n, const int* row_ptr, const int* nbr, const int* weight, const double* extra, int K,
                        int* out_frame, double* out_score, int* ngroups) {
  for (int k = 0; k < K; ++k) { out_frame[k] = -1; out_score[k] = 0.0; }
  *ngroups = 0;
  std::map<int, double> fs;
  for (int i = 0; i < n; ++i) fs[frame[i]] = score[i];
  std::map<int, Group> groups;
  double best = -1;
  for (std::map<int, double>::iterator it = fs.begin(); it != fs.end(); ++it) {
    int deputy = it->first;
    double ds = it->second;
    Group g;
    g.frames.insert(it->first);
    g.score += ds;
    std::map<int, int> covi;
    for (int e = row_ptr[it->first]; e < row_ptr[it->first + 1]; ++e) covi[nbr[e]] = weight[e];
    for (std::map<int, int>::iterator kv = covi.begin(); kv != covi.end(); ++kv)
      if (kv->second > 10 && fs.count(kv->first)) {
        const double s = fs[kv->first];
        g.frames.insert(kv->first);
        g.score += s;
        if (s > ds) { deputy = kv->first; ds = s; }
      }
    std::map<int, Group>::iterator at = groups.find(deputy);
    if (at == groups.end() || at->second.score < g.score) {
      groups[deputy] = g;
      if (g.score > best) best = g.score;
    }
  }
  if (best < 0) return 1;
  best = 0.0;
  for (std::map<int, Group>::iterator kv = groups.begin(); kv != groups.end(); ++kv) {
    std::vector<double> v;
    for (std::set<int>::iterator f = kv->second.frames.begin(); f != kv->second.frames.end(); ++f) v.push_back(fs[*f]);
    if (v.size() > 5) std::sort(v.rbegin(), v.rend());
    double sum = 0;
    for (size_t i = 0; i < std::min((size_t)5, v.size()); ++i) sum += v[i];
    kv->second.score = sum;
    best = std::max(best, sum);
  }
  if (groups.size() > 3) {
    const double thr = best * 0.5;
    for (std::map<int, Group>::iterator it = groups.begin(); it != groups.end();)
      if (it->second.score < thr) it = groups.erase(it); else ++it;
  }
  std::vector<std::pair<int, double>> gv;
  for (std::map<int, Group>::iterator kv = groups.begin(); kv != groups.end(); ++kv) gv.push_back(std::make_pair(kv->first, kv->second.score + (extra ? extra[kv->first] : 0.0)));
  if (!extra) for (size_t i = 0; i < gv.size(); ++i) gv[i].second = groups[gv[i].first].score;
  std::stable_sort(gv.begin(), gv.end(), [](const std::pair<int, double>& a, const std::pair<int, double>& b) { return a.second > b.second; });
  *ngroups = (int)gv.size();
  for (int k = 0; k < K && k < (int)gv.size(); ++k) { out_frame[k] = gv[k].first; out_score[k] = gv[k].second; }
  return 0;
}
'''
CAM = np.array([458.654, 457.296, 367.215, 248.375, 47.9])
THR = np.array([50.0, 75.0])


def host_lib():
    d = tempfile.mkdtemp()
    with open(os.path.join(d, "h.cpp"), "w") as f:
        f.write(HOST)
    so = os.path.join(d, "libh.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-w", "-fPIC", "-ffp-contract=off", "-shared", os.path.join(d, "h.cpp"), "-o", so], check=True)
    lib = C.CDLL(so)
    lib.hg_reloc.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 3
    return lib


def covisibility(N, seed):
    """each frame linked to itself and to up to 10 frames within +-8, weights 1-40"""
    rng = np.random.default_rng(seed)
    row_ptr, nbr, weight = [0], [], []
    for f in range(N):
        near = sorted(set(int(x) for x in np.clip(f + rng.integers(-8, 9, 10), 0, N - 1)) | {f})
        nbr += near
        weight += [int(w) for w in rng.integers(1, 41, len(near))]
        row_ptr.append(len(nbr))
    return np.array(row_ptr, np.int32), np.array(nbr, np.int32), np.array(weight, np.int32)


def host_groups(host, cf, sc, nc, cov, K, extra=None):
    Q = len(nc)
    gf, gs, ng = np.zeros((Q, K), np.int32), np.zeros((Q, K)), np.zeros(Q, np.int32)
    for q in range(Q):
        one = C.c_int(0)
        host.hg_reloc(cf[q].ctypes.data, sc[q].ctypes.data, int(nc[q]), cov[0].ctypes.data, cov[1].ctypes.data, cov[2].ctypes.data,
                      None if extra is None else extra[q].ctypes.data, K, gf[q].ctypes.data, gs[q].ctypes.data, C.byref(one))
        ng[q] = one.value
    return gf, gs, ng


def main(reps=20, quick=False, out=None):
    import torch
    from planted import features, planted_pair
    cap, K = 400, 3
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)
    ctx = api.Context(lightglue=weights.synthetic_lightglue(1234), max_batch=12, max_keypoints=cap)
    ctx.bow_load(weights.synthetic_vocabulary(1234, k=10, L=4))
    host = host_lib()
    st = torch.cuda.Stream()
    s = st.cuda_stream
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a.view(np.int32) if a.dtype == np.uint32 else a)).cuda()  # noqa: E731
    # ---- the grouping entry alone
    for N in ((1024,) if quick else (1024, 4096)):
        ids, vals, nw = vectors(N, cap, N)
        db = api.BowDatabase(ctx, N, 8, keep_features=True)                      # the grouping reads neither words nor rows: a small row capacity
        db.add_batch_dev(torch.zeros((N, 8), dtype=torch.int32, device="cuda"), torch.zeros((N, 8), dtype=torch.float64, device="cuda"),
                         torch.zeros(N, dtype=torch.int32, device="cuda"), torch.zeros((N, 8, 259), dtype=torch.float32, device="cuda"),
                         torch.zeros(N, dtype=torch.int32, device="cuda"))
        cov = covisibility(N, N)
        db.attach_map(len(cov[1]))
        db.set_covisibility(*cov)
        qdb = api.BowDatabase(ctx, N, cap)
        qdb.add_batch_dev(dev(ids), dev(vals), dev(nw))
        for Q in ((8,) if quick else (1, 8, 64)):
            qi, qv, qn = vectors(Q, cap, 7 * N + Q, revisit_of=(ids, nw))
            cf = torch.zeros((Q, N), dtype=torch.int32, device="cuda"); cs = torch.zeros_like(cf); sc = torch.zeros((Q, N), dtype=torch.float64, device="cuda")
            nc = torch.zeros(Q, dtype=torch.int32, device="cuda"); ms = torch.zeros_like(nc)
            qdb.query_batch_dev(dev(qi), dev(qv), dev(qn), cf, cs, sc, nc, ms, ratio=0.3)
            gf = torch.zeros((Q, K), dtype=torch.int32, device="cuda"); gs = torch.zeros((Q, K), dtype=torch.float64, device="cuda")
            ng = torch.zeros(Q, dtype=torch.int32, device="cuda"); gst = torch.zeros_like(ng)
            t = timed(lambda: db.group_dev(0, cf, sc, nc, gf, gs, ng, gst, stream=s), st, reps)
            hf, hs, hn = host_groups(host, cf.cpu().numpy(), sc.cpu().numpy(), nc.cpu().numpy(), cov, K)
            assert (hf == gf.cpu().numpy()).all() and hs.tobytes() == gs.cpu().numpy().tobytes() and (hn == ng.cpu().numpy()).all(), "host grouping and device disagree"
            emit(what="bowdb_group_dev", mode="relocalisation", N=N, Q=Q, K=K, reps=reps, ms_median_min_max=t, candidates_mean=float(nc.float().mean()),
                 groups_mean=float(ng.float().mean()))
        db.close()
        qdb.close()
    # ---- the composite at Q = 4, K = 3: 12 stored frames, frame 2 q + 1 the planted revisit of query q with map points at its planted rows
    Q, N = 4, 12
    fx, fy, cx, cy = CAM[:4]
    rng = np.random.default_rng(9)
    qf, dbf = np.zeros((Q, cap, 259), np.float32), np.zeros((N, cap, 259), np.float32)
    qn, dn = np.zeros(Q, np.int32), np.zeros(N, np.int32)
    xyz = np.full((N, cap, 3), np.nan)
    for f in range(N):
        dbf[f, :300 + 5 * f], dn[f] = features(300 + 5 * f, 900 + f), 300 + 5 * f
    for q in range(Q):
        a, b = planted_pair(380 - 20 * q, 360, 70 + 10 * q)
        qf[q, :len(a)], qn[q] = a, len(a)
        dbf[2 * q + 1], dn[2 * q + 1] = 0, len(b)
        dbf[2 * q + 1, :len(b)] = b
        k = min(len(a), len(b)) // 2
        z = rng.uniform(2.0, 10.0, k)
        xyz[2 * q + 1, :k] = np.stack([(a[:k, 1] - cx) / fx * z, (a[:k, 2] - cy) / fy * z, z], 1) + (0.3, -0.1, 0.2)      # Twc_true: a translation
    ft, nt = dev(dbf), dev(dn)
    i32 = lambda shape: torch.zeros(shape, dtype=torch.int32, device="cuda")  # noqa: E731
    f64 = lambda shape: torch.zeros(shape, dtype=torch.float64, device="cuda")  # noqa: E731
    ids, vals, nw = i32((N, cap)), f64((N, cap)), i32((N,))
    ctx.bow_vector_batch_dev(ft, nt, ids, vals, nw)
    db = api.BowDatabase(ctx, N, cap, keep_features=True)
    db.add_batch_dev(ids, vals, nw, ft, nt)
    cov = covisibility(N, 5)
    db.attach_map(len(cov[1]))
    db.set_covisibility(*cov)
    db.set_points(0, xyz)
    qt, qnt = dev(qf), dev(qn)
    o = dict(ok=i32((Q,)), stage=i32((Q,)), Twc=f64((Q, 16)), best=i32((Q,)), num=i32((Q,)), mask=torch.zeros((Q, cap), dtype=torch.uint8, device="cuda"),
             idx=i32((Q, cap, 2)), score=torch.zeros((Q, cap), dtype=torch.float32, device="cuda"), nmatch=i32((Q,)))
    MIN = 20

    def composite():
        db.relocalize_batch_dev(qt, qnt, CAM, THR, MIN, o["ok"], o["stage"], o["Twc"], o["best"], o["num"], o["mask"], o["idx"], o["score"], o["nmatch"], stream=s)
    qi, qv, qw = i32((Q, cap)), f64((Q, cap)), i32((Q,))
    cf, cs, sc, nc, ms = i32((Q, N)), i32((Q, N)), f64((Q, N)), i32((Q,)), i32((Q,))
    best, idx, msc, nm = i32((Q,)), i32((Q, cap, 2)), torch.zeros((Q, cap), dtype=torch.float32, device="cuda"), i32((Q,))
    bT, bM, bC, bT2, bM2, bN2 = f64((Q, 16)), torch.zeros((Q, cap), dtype=torch.uint8, device="cuda"), i32((Q,)), f64((Q, 16)), torch.zeros((Q, cap), dtype=torch.uint8, device="cuda"), i32((Q,))
    keep = {}

    def baseline():
        with torch.cuda.stream(st):
            ctx.bow_vector_batch_dev(qt, qnt, qi, qv, qw, stream=s)
            db.query_batch_dev(qi, qv, qw, cf, cs, sc, nc, ms, ratio=0.3, stream=s)
            hcf, hsc, hnc = cf.cpu().numpy(), sc.cpu().numpy(), nc.cpu().numpy()               # round trip 1: the candidate lists
            gf, gs, ng = host_groups(host, hcf, hsc, hnc, cov, K)
            gft = torch.from_numpy(gf).cuda()
            db.match_candidates_batch_dev(qt, qnt, gft, best, idx, msc, nm, stream=s)
            hb, hi, hm = best.cpu().numpy(), idx.cpu().numpy(), nm.cpu().numpy()              # round trip 2: the winner and its list
            obj, img = np.zeros((Q, cap, 3), np.float32), np.zeros((Q, cap, 2), np.float32)
            X, obs, n = np.zeros((Q, cap, 3)), np.zeros((Q, cap, 3)), np.zeros(Q, np.int32)
            for q in range(Q):
                if hb[q] < 0 or hm[q] < MIN:
                    continue
                li = hi[q, :hm[q]]
                P = xyz[hb[q], li[:, 1]]
                ok = ~np.isnan(P[:, 0])
                k = int(ok.sum())
                uv = qf[q, li[ok, 0], 1:3]
                obj[q, :k], img[q, :k], X[q, :k], obs[q, :k, :2], obs[q, :k, 2], n[q] = P[ok].astype(np.float32), uv, P[ok], uv, -1.0, k
            nt_ = torch.from_numpy(n).cuda()
            ctx.pnp_ransac_batch_dev(torch.from_numpy(obj).cuda(), torch.from_numpy(img).cuda(), nt_, CAM[:4], bT, bM, bC, stream=s)
            ctx.frame_optimize_batch_dev(torch.from_numpy(X).cuda(), torch.from_numpy(obs).cuda(), nt_, bT, CAM, THR, bT2, bM2, bN2, stream=s)
            keep.update(gf=gf, gs=gs, ng=ng)
    composite()
    baseline()
    torch.cuda.synchronize()
    assert o["best"].cpu().tolist() == best.cpu().tolist() == [1, 3, 5, 7], (o["best"].cpu().tolist(), best.cpu().tolist())
    assert o["Twc"].cpu().numpy().tobytes() == bT2.cpu().numpy().tobytes() and o["num"].cpu().tolist() == bN2.cpu().tolist(), "composite and baseline disagree"
    # the host grouping against the device's groups, byte for byte, before anything is timed
    gf, gs, ng, gst = i32((Q, K)), f64((Q, K)), i32((Q,)), i32((Q,))
    db.group_dev(0, cf, sc, nc, gf, gs, ng, gst)
    torch.cuda.synchronize()
    assert (keep["gf"] == gf.cpu().numpy()).all() and keep["gs"].tobytes() == gs.cpu().numpy().tobytes() and (keep["ng"] == ng.cpu().numpy()).all()
    tc = timed(composite, st, reps)
    tb = timed(baseline, st, reps)
    emit(what="relocalize_batch_dev", Q=Q, K=K, N=N, n=cap, pose_refinement=True, reps=reps, composite_ms_median_min_max=tc, baseline_ms_median_min_max=tb,
         ratio_composite_over_baseline=round(tc[0] / tb[0], 4), stages=o["stage"].cpu().tolist(), num=o["num"].cpu().tolist(), nmatch=o["nmatch"].cpu().tolist())
    db.close()
    ctx.close()
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    arg = lambda k, d: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else d  # noqa: E731
    main(int(arg("--reps", 20)), "--quick" in sys.argv, arg("--out", None))
