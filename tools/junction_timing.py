"""Cost of relocalisation's junction term on the device (kernels_junction.hip; include/airfe.h "Junction term"), timed between device events: medians over
--reps timed calls after 3 warm-ups, with min / max.
  Scene     N stored frames (256 distinct ones, repeated) and Q query frames of 200 junctions and 300 lines (85 % of the lines between two junctions), the
            junction descriptors drawn from 300 leaves of a k = 10, L = 3 vocabulary; 512 x 512 images; ecap = 4096.
  Timed     junction_term_batch_dev alone (the queries' vectors, words and connections are on the device already: the tables of the queries, the dense
            score of the unchanged query kernel, the term); junction_extra_batch_dev (the composite: from the raw junction rows and lines, the vocabulary
            descent included).
  Baseline  the caller's path without these entries, in the same run: tools/junction_literal.cpp (a dense junction map, std::set connections, an inverted
            file per word, match_matrix, the four nested loops, L1 scoring over std::map vectors) on ONE thread per query, then the upload of the
            [Q][N] table.  Wall clock.  Two forms: every stored frame (the table the device entry fills) and 5 frames per query (what the reference
            computes: the group frames only).  The vocabulary descent of the query is NOT in the baseline (it uses the device's words).
  Checked   before anything is timed: the baseline's table and the device's are the same bytes.
    python tools/junction_timing.py [--reps R] [--quick] [--out FILE]        (on an MI355X; one JSON line per shape)"""
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

W = H = 512
CAP, CAPL, ECAP, NJ, NL, DISTINCT = 256, 320, 4096, 200, 300, 256


def host_lib():
    d = tempfile.mkdtemp()
    so = os.path.join(d, "libjl.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-w", "-fPIC", "-shared", "-ffp-contract=off", os.path.join(ROOT, "tools", "junction_literal.cpp"), "-o", so],
                   check=True)
    lib = C.CDLL(so)
    lib.jl_create.restype = C.c_void_p
    lib.jl_create.argtypes = [C.c_int, C.c_int]
    lib.jl_destroy.argtypes = [C.c_void_p]
    lib.jl_add.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    lib.jl_query.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    return lib


def scene(voc, B, seed):
    """-> junc f32 [B][CAP][259], nj [B], lines f64 [B][CAPL][4], nl [B]"""
    rng = np.random.default_rng(seed)
    leaves = np.flatnonzero(np.asarray(voc["n_children"]) == 0)
    pool = np.random.default_rng(1).choice(leaves, 300, replace=False)
    junc, lines = np.zeros((B, CAP, 259), np.float32), np.zeros((B, CAPL, 4), np.float64)
    for b in range(B):
        xy = rng.uniform(2, W - 3, (NJ, 2)).astype(np.float32)
        junc[b, :NJ, 0] = rng.uniform(0.1, 1, NJ)
        junc[b, :NJ, 1:3] = xy
        junc[b, :NJ, 3:] = np.asarray(voc["desc"])[pool[rng.integers(len(pool), size=NJ)]]
        a, c = rng.integers(NJ, size=NL), rng.integers(NJ, size=NL)
        ln = np.concatenate([xy[a], xy[c]], 1).astype(np.float64) + rng.uniform(-1.5, 1.5, (NL, 4))
        free = rng.uniform(size=NL) > 0.85
        ln[free] = rng.uniform(-3, W + 3, (int(free.sum()), 4))
        lines[b, :NL] = ln
    return junc, np.full(B, NJ, np.int32), lines, np.full(B, NL, np.int32)


def one_shape(ctx, lib, voc, N, Q, reps, emit):
    import torch
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    st = torch.cuda.Stream()
    s = st.cuda_stream
    fj, fnj, fl, fnl = scene(voc, min(N, DISTINCT), 5)
    qj, qnj, ql, qnl = scene(voc, Q, 6)
    db = api.BowDatabase(ctx, N, CAP)
    db.attach_junctions(ECAP, max(Q, 64))
    tj, tnj, tl, tnl = up(fj), up(fnj), up(fl), up(fnl)
    for f0 in range(0, N, 64):                                          # the distinct frames, repeated
        k = min(64, N - f0)
        r = torch.arange(f0, f0 + k, device="cuda") % len(fj)
        part = [t[r].contiguous() for t in (tj, tnj, tl, tnl)]
        db.add_junction_frames_batch_dev(*part, W, H)
        torch.cuda.synchronize()                                        # the gathered copies are read on the context's stream: keep them until it is done
    # the single entries' inputs for the queries, and everything the baseline needs, from the device
    i32 = lambda shape: torch.zeros(shape, dtype=torch.int32, device="cuda")  # noqa: E731
    tqj, tqnj, tql, tqnl = up(qj), up(qnj), up(ql), up(qnl)
    ids, vals, nw, word = i32((Q, CAP)), torch.zeros((Q, CAP), dtype=torch.float64, device="cuda"), i32((Q,)), i32((Q, CAP))
    edge, ne, qs = i32((Q, ECAP, 2)), i32((Q,)), i32((Q,))
    ctx.bow_vector_batch_dev(tqj, tqnj, ids, vals, nw, word_t=word)
    ctx.junction_connections_batch_dev(tql, tqnl, tqj, tqnj, W, H, edge, ne, qs)
    extra, extra2 = torch.zeros((Q, N), dtype=torch.float64, device="cuda"), torch.zeros((Q, N), dtype=torch.float64, device="cuda")
    term = lambda: db.junction_term_batch_dev(ids, vals, nw, word, tqnj, edge, ne, extra, qstatus_t=qs, stream=s)  # noqa: E731
    composite = lambda: db.junction_extra_batch_dev(tqj, tqnj, tql, tqnl, W, H, extra2, stream=s)  # noqa: E731
    torch.cuda.synchronize()                                            # the inputs were queued on the context's stream, the timed calls run on `st`
    term()
    composite()
    torch.cuda.synchronize()
    dev = extra.cpu().numpy()
    assert dev.tobytes() == extra2.cpu().numpy().tobytes(), "the composite and the chain disagree"
    # the baseline's database: the distinct frames' device vectors and words
    D = len(fj)
    fi, fv, fw, fwd = i32((D, CAP)), torch.zeros((D, CAP), dtype=torch.float64, device="cuda"), i32((D,)), i32((D, CAP))
    ctx.bow_vector_batch_dev(tj, tnj, fi, fv, fw, word_t=fwd)
    torch.cuda.synchronize()
    fi, fv, fw, fwd = fi.cpu().numpy().view(np.uint32), fv.cpu().numpy(), fw.cpu().numpy(), fwd.cpu().numpy().view(np.uint32)
    hq = dict(ids=ids.cpu().numpy().view(np.uint32), vals=vals.cpu().numpy(), nw=nw.cpu().numpy(), word=word.cpu().numpy().view(np.uint32))
    hdb = lib.jl_create(W, H)
    for f in range(N):
        g = f % D
        lib.jl_add(hdb, fl[g].ctypes.data, int(fnl[g]), fj[g].ctypes.data, int(fnj[g]), fwd[g].ctypes.data, fi[g].ctypes.data, fv[g].ctypes.data, int(fw[g]))
    table = np.zeros((Q, N))
    groups = np.ascontiguousarray(np.random.default_rng(9).integers(N, size=(Q, 5)).astype(np.int32))

    def baseline(frames_per_query=None):
        for q in range(Q):
            lib.jl_query(hdb, ql[q].ctypes.data, int(qnl[q]), qj[q].ctypes.data, int(qnj[q]), hq["word"][q].ctypes.data, hq["ids"][q].ctypes.data,
                         hq["vals"][q].ctypes.data, int(hq["nw"][q]), groups[q].ctypes.data if frames_per_query else None, frames_per_query or 0,
                         table[q].ctypes.data)
        extra2.copy_(torch.from_numpy(table))
        torch.cuda.synchronize()
    baseline()
    bad = np.argwhere(table != dev)
    assert table.tobytes() == dev.tobytes(), f"the device table and the literal baseline disagree at {len(bad)} of {table.size} entries, first {bad[:8].tolist()}"
    mmm = lambda v: (round(float(np.median(v)), 4), round(v[0], 4), round(v[-1], 4))  # noqa: E731

    def wall(fn, n):
        out = []
        for _ in range(n + 1):
            t0 = time.perf_counter()
            fn()
            out.append((time.perf_counter() - t0) * 1e3)
        return mmm(sorted(out[1:]))
    t_term, t_comp = timed(term, st, reps), timed(composite, st, reps)
    b_all = wall(baseline, 3 if N * Q > 4096 else 10)
    b_grp = wall(lambda: baseline(5), 10)
    emit(what="bowdb_junction_term", N=N, Q=Q, junctions=NJ, lines=NL, edges_mean=float(ne.float().mean()), nonzero_share=float((dev > 0).mean()), reps=reps,
         term_ms_median_min_max=t_term, composite_ms_median_min_max=t_comp, literal_all_frames_plus_upload_ms_median_min_max=b_all,
         literal_5_frames_per_query_plus_upload_ms_median_min_max=b_grp)
    lib.jl_destroy(hdb)
    db.close()


def main(reps=20, quick=False, out=None):
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)
    voc = weights.synthetic_vocabulary(1234, k=10, L=3)
    ctx = api.Context(max_batch=1, max_keypoints=CAP)
    ctx.bow_load(voc)
    lib = host_lib()
    for N in ((64,) if quick else (64, 1024, 4096)):
        for Q in (1, 16):
            one_shape(ctx, lib, voc, N, Q, reps, emit)
    ctx.close()
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    arg = lambda k, d: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else d  # noqa: E731
    main(int(arg("--reps", 20)), "--quick" in sys.argv, arg("--out", None))
