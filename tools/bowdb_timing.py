"""Cost of the BoW keyframe database (kernels_bowdb.hip), timed with device events: the BoW-vector entry (64 frames x 400 features), add_batch_dev, the
query (+ top-K) for N stored frames x Q queries at ~380 words per vector, and the composite at K = 3 (Q = 4: 12 LightGlue pairs).  Medians over --reps timed
calls after 3 warm-ups, with min / max.  The comparison is NOT the code under test: HOST below states the reference's algorithm in C++ — an inverted file of
std::map walked per query word, then the merge-style L1 score per surviving frame (src/bow/database.cc:98-124, map_user.cc:135-166) — on one CPU thread,
checked against tests/bowdb_ref.py on the first queries before it is timed.  Run it under `rocprofv3 --kernel-trace --stats` for the per-kernel split.
    python tools/bowdb_timing.py [--reps R] [--quick]        (on an MI355X; one JSON line per measurement)"""
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
from airslam_amd import api, weights  # noqa: E402
import bowdb_ref as br  # noqa: E402

HOST = r'''
#include <algorithm>
#include <cmath>
#include <map>
#include <vector>
typedef std::map<unsigned, double> Vec;
struct Db { std::vector<Vec> frames; std::vector<std::map<int, int>> inv; };
extern "C" void* hb_create(int n_words) { Db* d = new Db; d->inv.resize(n_words); return d; }
extern "C" void hb_add(void* h, const unsigned* ids, const double* vals, int nw) {
  Db* d = (Db*)h; const int f = (int)d->frames.size(); Vec v;
  for (int i = 0; i < nw; ++i) { v[ids[i]] = vals[i]; d->inv[ids[i]][f] = 1; }
  d->frames.push_back(v);
}
static double l1(const Vec& v1, const Vec& v2) {
  Vec::const_iterator a = v1.begin(), b = v2.begin(); double s = 0;
  while (a != v1.end() && b != v2.end()) {
    if (a->first == b->first) { s += fabs(a->second - b->second) - fabs(a->second) - fabs(b->second); ++a; ++b; }
    else if (a->first < b->first) a = v1.lower_bound(b->first);
    else b = v2.lower_bound(a->first);
  }
  return -s / 2.0;
}
extern "C" int hb_query(void* h, const unsigned* ids, const double* vals, int nw, float ratio, int min_words, int* frame, int* sharing, double* score, int cap, int* max_sharing) {
  Db* d = (Db*)h; Vec q; std::map<int, int> sh;
  for (int i = 0; i < nw; ++i) q[ids[i]] = vals[i];
  for (Vec::const_iterator it = q.begin(); it != q.end(); ++it)
    for (std::map<int, int>::const_iterator kv = d->inv[it->first].begin(); kv != d->inv[it->first].end(); ++kv) sh[kv->first]++;
  int m = 0;
  for (std::map<int, int>::const_iterator kv = sh.begin(); kv != sh.end(); ++kv) m = std::max(m, kv->second);
  *max_sharing = m;
  const int thr = std::max((int)(m * ratio), min_words);
  int n = 0;
  for (std::map<int, int>::const_iterator kv = sh.begin(); kv != sh.end(); ++kv) {
    if (kv->second < thr) continue;
    const double s = l1(d->frames[kv->first], q);
    if (n < cap) { frame[n] = kv->first; sharing[n] = kv->second; score[n] = s; }
    ++n;
  }
  return n;
}
'''
N_WORDS = 10000


def host_lib():
    d = tempfile.mkdtemp()
    with open(os.path.join(d, "h.cpp"), "w") as f:
        f.write(HOST)
    so = os.path.join(d, "libh.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-w", "-fPIC", "-ffp-contract=off", "-shared", os.path.join(d, "h.cpp"), "-o", so], check=True)
    lib = C.CDLL(so)
    lib.hb_create.restype = C.c_void_p
    lib.hb_create.argtypes = [C.c_int]
    lib.hb_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    lib.hb_query.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    return lib


def timed(fn, st, reps, warm=3):
    """per-call device milliseconds of fn() on stream st: (median, min, max) over reps calls, each between its own pair of events"""
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(st)
        fn()
        b.record(st)
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return round(float(np.median(ms)), 4), round(ms[0], 4), round(ms[-1], 4)


def vectors(B, cap, seed, revisit_of=None):
    """B L1-normalised vectors of ~380 of N_WORDS words (what 400 features leave after stopped and repeated words); revisit_of: 60 % of the words of those rows"""
    rng = np.random.default_rng(seed)
    ids = np.zeros((B, cap), np.uint32)
    vals = np.zeros((B, cap), np.float64)
    nw = np.zeros(B, np.int32)
    for b in range(B):
        w = rng.choice(N_WORDS, size=380, replace=False)
        if revisit_of is not None and b % 2 == 0:
            src = revisit_of[0][b % len(revisit_of[0]), :revisit_of[1][b % len(revisit_of[0])]]
            w = np.unique(np.concatenate([rng.choice(src, size=int(0.6 * len(src)), replace=False), w[:150]]))[:cap]
        w = np.sort(w)
        v = rng.uniform(0.5, 8.0, len(w))
        ids[b, :len(w)], vals[b, :len(w)], nw[b] = w, v / v.sum(), len(w)
    return ids, vals, nw


def main(reps=20, quick=False):
    import torch
    cap = 400
    ctx = api.Context(lightglue=weights.synthetic_lightglue(1234), max_batch=12, max_keypoints=cap)
    ctx.bow_load(weights.synthetic_vocabulary(1234, k=10, L=4))
    host = host_lib()
    st = torch.cuda.Stream()
    dev = lambda a, t=None: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
    # the BoW-vector entry on 64 frames of 400 random unit descriptors
    rng = np.random.default_rng(1)
    f = rng.standard_normal((64, cap, 259)).astype(np.float32)
    f[..., 3:] /= np.linalg.norm(f[..., 3:], axis=-1, keepdims=True)
    ft, nt = dev(f), torch.full((64,), cap, dtype=torch.int32, device="cuda")
    vi, vv, vn = torch.zeros((64, cap), dtype=torch.int32, device="cuda"), torch.zeros((64, cap), dtype=torch.float64, device="cuda"), torch.zeros(64, dtype=torch.int32, device="cuda")
    t = timed(lambda: ctx.bow_vector_batch_dev(ft, nt, vi, vv, vn, stream=st.cuda_stream), st, reps)
    print(json.dumps(dict(what="bow_vector_batch_dev", B=64, n=cap, reps=reps, ms_median_min_max=t)), flush=True)
    for N in ((4096,) if quick else (1024, 4096, 16384)):
        ids, vals, nw = vectors(N, cap, N)
        db = api.BowDatabase(ctx, N, cap, keep_features=False)
        di, dv, dn = dev(ids), dev(vals), dev(nw)

        def add():
            db.clear()
            db.add_batch_dev(di, dv, dn, stream=st.cuda_stream)
        t_add = timed(add, st, reps)
        hdb = host.hb_create(N_WORDS)
        for b in range(N):
            host.hb_add(hdb, ids[b].ctypes.data, vals[b].ctypes.data, int(nw[b]))
        ref = br.Database()
        for b in range(min(N, 1024)):
            ref.add_frame(ids[b, :nw[b]], vals[b, :nw[b]])
        for Q in ((64,) if quick else (1, 8, 64)):
            qi, qv, qn = vectors(Q, cap, 7 * N + Q, revisit_of=(ids, nw))
            ti, tv, tn = dev(qi), dev(qv), dev(qn)
            cf = torch.zeros((Q, N), dtype=torch.int32, device="cuda"); cs = torch.zeros_like(cf); sc = torch.zeros((Q, N), dtype=torch.float64, device="cuda")
            nc = torch.zeros(Q, dtype=torch.int32, device="cuda"); ms = torch.zeros_like(nc); top = torch.zeros((Q, 3), dtype=torch.int32, device="cuda")

            def query():
                db.query_batch_dev(ti, tv, tn, cf, cs, sc, nc, ms, ratio=0.3, stream=st.cuda_stream)
                db.topk_dev(cf, sc, nc, top, stream=st.cuda_stream)
            t_q = timed(query, st, reps)
            # the host statement: checked, then timed
            hf, hs, hsc, hm = np.zeros(N, np.int32), np.zeros(N, np.int32), np.zeros(N, np.float64), C.c_int(0)
            gf, gsc, gn = cf.cpu().numpy(), sc.cpu().numpy(), nc.cpu().numpy()
            for q in range(Q):
                n = host.hb_query(hdb, qi[q].ctypes.data, qv[q].ctypes.data, int(qn[q]), 0.3, 8, hf.ctypes.data, hs.ctypes.data, hsc.ctypes.data, N, C.byref(hm))
                assert n == gn[q] and (hf[:n] == gf[q, :n]).all() and hsc[:n].tobytes() == gsc[q, :n].tobytes(), "host statement and device disagree"
                if N <= 1024 and q < 4:
                    _, _, cands = ref.candidates(qi[q, :qn[q]], qv[q, :qn[q]], 0.3)
                    assert [c[0] for c in cands] == hf[:n].tolist() and np.array([c[2] for c in cands]).tobytes() == hsc[:n].tobytes()
            ht = []
            for _ in range(3):
                t0 = time.perf_counter()
                for q in range(Q):
                    host.hb_query(hdb, qi[q].ctypes.data, qv[q].ctypes.data, int(qn[q]), 0.3, 8, hf.ctypes.data, hs.ctypes.data, hsc.ctypes.data, N, C.byref(hm))
                ht.append((time.perf_counter() - t0) * 1e3)
            db_bytes = float(nw.sum()) * 12
            print(json.dumps(dict(what="bowdb_query+topk", N=N, Q=Q, reps=reps, add_batch_ms_median_min_max=t_add, query_ms_median_min_max=t_q,
                                  host_statement_ms_one_thread_median=round(float(np.median(ht)), 3), host_ms_min_max=(round(min(ht), 3), round(max(ht), 3)),
                                  candidates_mean=float(gn.mean()), database_bytes=db_bytes,
                                  GBps_database_read_once=round(db_bytes / (t_q[0] * 1e-3) / 1e9, 1),
                                  GBps_per_query_pass=round(Q * db_bytes / (t_q[0] * 1e-3) / 1e9, 1))), flush=True)
        db.close()
    # the composite at K = 3 on planted pairs (Q = 4: 12 pairs)
    from planted import planted_pair
    Q, K, N = 4, 3, 12
    qf, dbf = np.zeros((Q, cap, 259), np.float32), np.zeros((N, cap, 259), np.float32)
    for q in range(Q):
        for k in range(K):
            a, b = planted_pair(cap, cap, 10 * q + k)
            qf[q], dbf[q * K + k] = a, b
    db = api.BowDatabase(ctx, N, cap, keep_features=True)
    full = torch.full((N,), cap, dtype=torch.int32, device="cuda")
    db.add_batch_dev(torch.zeros((N, cap), dtype=torch.int32, device="cuda"), torch.zeros((N, cap), dtype=torch.float64, device="cuda"),
                     torch.zeros(N, dtype=torch.int32, device="cuda"), dev(dbf), full)
    cand = torch.arange(N, dtype=torch.int32, device="cuda").reshape(Q, K).contiguous()
    best = torch.zeros(Q, dtype=torch.int32, device="cuda"); idx = torch.zeros((Q, cap, 2), dtype=torch.int32, device="cuda")
    sco = torch.zeros((Q, cap), dtype=torch.float32, device="cuda"); nm = torch.zeros(Q, dtype=torch.int32, device="cuda")
    qt, qn = dev(qf), torch.full((Q,), cap, dtype=torch.int32, device="cuda")
    t = timed(lambda: db.match_candidates_batch_dev(qt, qn, cand, best, idx, sco, nm, stream=st.cuda_stream), st, reps)
    print(json.dumps(dict(what="match_candidates_batch_dev", Q=Q, K=K, n=cap, outlier_rejection=True, reps=reps, ms_median_min_max=t, matches=nm.cpu().tolist())), flush=True)
    db.close()
    ctx.close()


if __name__ == "__main__":
    main(int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 20, "--quick" in sys.argv)
