"""BoW keyframe database on the device (include/airfe.h "BoW keyframe database") against DBoW2 compiled unchanged (the vector) and tests/bowdb_ref.py (the
database, the filters, the scores, the ranking, the best-candidate rule).  Every equality is exact."""
import numpy as np
import pytest

import bowdb_ref as br
from airslam_amd import weights
from oracle import ref_lib, ref_post
from planted import features, planted_pair

pytestmark = pytest.mark.gpu
CAP = 400
_S = {}


def _voc():
    if "voc" not in _S:
        _S["voc"] = weights.synthetic_vocabulary(1234, k=10, L=4)
    return _S["voc"]


def _ctx():
    """one context for the file: LightGlue for the composite (16 pairs), the 10^4-word vocabulary"""
    if "ctx" not in _S:
        from airslam_amd import api
        c = api.Context(lightglue=weights.synthetic_lightglue(1234), max_batch=16, max_keypoints=CAP)
        c.bow_load(_voc())
        _S["ctx"] = c
    return _S["ctx"]


def _frames(B, n, seed):
    """B frames of n features: descriptors near random leaves of the tree (tests/test_bow.py::_voc_features, vectorised) -> [B][n][259] float32"""
    voc = _voc()
    rng = np.random.default_rng(seed)
    leaves = np.nonzero(voc["n_children"] == 0)[0]
    f = np.zeros((B, n, 259), np.float32)
    f[..., 0] = rng.uniform(0.01, 1, (B, n))
    f[..., 1] = rng.uniform(4, 748, (B, n))
    f[..., 2] = rng.uniform(4, 476, (B, n))
    d = voc["desc"][rng.choice(leaves, size=(B, n))] + 0.15 * rng.standard_normal((B, n, 256), dtype=np.float32)
    f[..., 3:] = d / np.linalg.norm(d, axis=-1, keepdims=True)
    return f


def _want_vector(feat):
    """the BowVector DBoW2 makes of these rows: the compiled library where it was built, else the restatement the CPU suite pins to it bit for bit"""
    if ref_lib.available():
        w, _, ids, vals = ref_lib.bow_frame_to_bow(_voc(), feat)
        return w, ids, vals
    w, wt = ref_post.bow_transform(_voc(), feat[:, 3:])
    ids, vals = br.frame_to_bow(w, wt)
    return w, ids, vals


def _vectors_dev(feat, n):
    """feat [B][CAP][259], n [B] (numpy) -> device tensors (feat, n, ids, vals, nw, word) of Context.bow_vector_batch_dev"""
    import torch
    B = feat.shape[0]
    ft, nt = torch.from_numpy(feat).cuda(), torch.from_numpy(np.asarray(n, np.int32)).cuda()
    ids = torch.full((B, CAP), -1, dtype=torch.int32, device="cuda")
    vals = torch.full((B, CAP), float("nan"), dtype=torch.float64, device="cuda")
    nw = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    word = torch.zeros((B, CAP), dtype=torch.int32, device="cuda")
    _ctx().bow_vector_batch_dev(ft, nt, ids, vals, nw, word)
    torch.cuda.synchronize()
    return ft, nt, ids, vals, nw, word


def _padded(fr, ns):
    out = np.zeros((len(ns), CAP, 259), np.float32)
    for b, k in enumerate(ns):
        out[b, :k] = fr[b, :k]
    return out


def test_bow_vector_batch_equals_dbow2_bit_for_bit():
    ns = [400, 0, 1, 7, 399, 123, 400] + [int(x) for x in np.random.default_rng(5).integers(1, 401, 57)]
    fr = _frames(64, CAP, 77)
    feat = _padded(fr, ns)
    want = [_want_vector(feat[b, :ns[b]]) if ns[b] else (np.zeros(0, np.uint32),) * 2 + (np.zeros(0),) for b in range(64)]
    assert any((w[0] == br.UINT_MAX).any() for w in want)                  # stopped words are exercised
    got = {}
    for B in (1, 7, 64):
        _, _, ids, vals, nw, word = _vectors_dev(feat[:B], ns[:B])
        ids, vals, nw, word = ids.cpu().numpy().view(np.uint32), vals.cpu().numpy(), nw.cpu().numpy(), word.cpu().numpy().view(np.uint32)
        for b in range(B):
            w, wi, wv = want[b]
            assert nw[b] == len(wi), (B, b)
            np.testing.assert_array_equal(ids[b, :nw[b]], wi)
            assert vals[b, :nw[b]].tobytes() == np.ascontiguousarray(wv, np.float64).tobytes(), (B, b)
            np.testing.assert_array_equal(word[b, :ns[b]], w)
            assert (ids[b, nw[b]:] == 0xFFFFFFFF).all() and np.isnan(vals[b, nw[b]:]).all()       # rows beyond nw are not written
            key = (ids[b, :nw[b]].tobytes(), vals[b, :nw[b]].tobytes())
            assert got.setdefault(b, key) == key                           # a frame's bytes do not depend on B
    # ... nor on its position: the batch reversed
    _, _, ids, vals, nw, _ = _vectors_dev(feat[::-1].copy(), ns[::-1])
    ids, vals, nw = ids.cpu().numpy().view(np.uint32), vals.cpu().numpy(), nw.cpu().numpy()
    for b in range(64):
        r = 63 - b
        assert (ids[r, :nw[r]].tobytes(), vals[r, :nw[r]].tobytes()) == got[b]
    # the one-frame host entry
    hi, hv = _ctx().bow_vector(feat[0, :ns[0]])
    assert (hi.tobytes(), hv.tobytes()) == got[0]
    hi, hv = _ctx().bow_vector(np.zeros((0, 259), np.float32))
    assert len(hi) == 0


def _build(N, seed, keep=False):
    """a database of N synthetic keyframes (added in chunks) + their vectors on the host"""
    import torch
    from airslam_amd import api
    db = api.BowDatabase(_ctx(), max(N, 1), CAP, keep_features=keep)
    host, feats = [], []
    for c0 in range(0, N, 512):
        B = min(512, N - c0)
        fr = _frames(B, CAP, seed + c0)
        ft, nt, ids, vals, nw, _ = _vectors_dev(fr, [CAP] * B)
        db.add_batch_dev(ids, vals, nw, ft if keep else None, nt if keep else None)
        torch.cuda.synchronize()
        i, v, k = ids.cpu().numpy().view(np.uint32), vals.cpu().numpy(), nw.cpu().numpy()
        host += [(i[b, :k[b]].copy(), v[b, :k[b]].copy()) for b in range(B)]
        feats.append(fr)
    assert db.size == N
    return db, host, np.concatenate(feats)


def _queries(N, feats, seed):
    """64 queries: 24 planted revisits (a stored frame with 40 % of its features re-drawn), 30 unrelated frames, 10 near-empty frames (< 8 usable words)"""
    rng = np.random.default_rng(seed)
    q = _frames(64, CAP, seed + 1)
    ns = [CAP] * 64
    src = [-1] * 64
    for i in range(24):
        f = int(rng.integers(0, N))
        keep = rng.permutation(CAP)[:240]
        q[i, keep] = feats[f, keep]
        src[i] = f
    for i in range(54, 64):
        ns[i] = i - 54                                    # 0 .. 9 features: at most 9 words, most of them below the floor of 8
    ns[63] = 7
    return _padded(q, ns), ns, src


def _query_dev(db, qi, qv, qn, ratio, max_index=None, exclude=None, ccap=None, dense=True, Q=None):
    import torch
    Q = qi.shape[0]
    N = db.size
    ccap = ccap or max(N, 1)
    cf = torch.full((Q, ccap), -7, dtype=torch.int32, device="cuda")
    cs = torch.full((Q, ccap), -7, dtype=torch.int32, device="cuda")
    sc = torch.full((Q, ccap), float("nan"), dtype=torch.float64, device="cuda")
    nc = torch.full((Q,), -1, dtype=torch.int32, device="cuda")
    ms = torch.full((Q,), -1, dtype=torch.int32, device="cuda")
    sh = torch.full((Q, max(N, 1)), -1, dtype=torch.int32, device="cuda") if dense else None
    db.query_batch_dev(qi, qv, qn, cf, cs, sc, nc, ms, ratio=ratio, max_index_t=max_index, exclude_t=exclude, sharing_t=sh)
    torch.cuda.synchronize()
    return dict(frame=cf, sharing=cs, score=sc, ncand=nc, max_sharing=ms, dense=sh)


def _bits(excl_sets, N):
    words = (N + 31) // 32
    out = np.zeros((len(excl_sets), words), np.uint32)
    for q, s in enumerate(excl_sets):
        for f in s:
            out[q, f >> 5] |= np.uint32(1) << np.uint32(f & 31)
    return out.view(np.int32)


@pytest.mark.parametrize("N", [1, 300, 4096])
def test_query_equals_the_restatement_bit_for_bit(N):
    import torch
    db, host, feats = _build(N, 1000 + N)
    ref = br.Database()
    for ids, vals in host:
        ref.add_frame(ids, vals)
    qf, qn, src = _queries(N, feats, 50 + N)
    _, _, qi, qv, qnw, _ = _vectors_dev(qf, qn)
    hi, hv, hk = qi.cpu().numpy().view(np.uint32), qv.cpu().numpy(), qnw.cpu().numpy()
    qvec = [(hi[q, :hk[q]], hv[q, :hk[q]]) for q in range(64)]
    sharing = [ref.query(v[0]) for v in qvec]
    rng = np.random.default_rng(N)
    max_index = np.array([int(rng.integers(0, N + 1)) for _ in range(64)], np.int32)
    excl = []
    for q in range(64):
        s = set(int(x) for x in rng.integers(0, N, size=min(N, 40)))
        if src[q] >= 0 and q % 3 == 0:
            s.add(src[q])                                 # the covisible set of some revisits holds the revisited frame itself
        excl.append(s)
    seen = dict(thr=0, min_words=0, index=0, exclude=0, empty=0)
    for ratio in (0.3, 0.5):
        for filt in (False, True):
            got = _query_dev(db, qi, qv, qnw, ratio, torch.from_numpy(max_index).cuda() if filt else None,
                             torch.from_numpy(_bits(excl, N)).cuda() if filt else None)
            g = {k: (v.cpu().numpy() if v is not None else None) for k, v in got.items()}
            for q in range(64):
                ms, thr, cands = ref.candidates(qvec[q][0], qvec[q][1], ratio, 8, max_index[q] if filt else None, excl[q] if filt else None, sharing[q])
                dense = np.zeros(N, np.int32)
                for f, s in sharing[q].items():
                    dense[f] = s
                np.testing.assert_array_equal(g["dense"][q], dense)
                assert g["max_sharing"][q] == ms and g["ncand"][q] == len(cands), (N, ratio, filt, q)
                k = len(cands)
                np.testing.assert_array_equal(g["frame"][q, :k], [c[0] for c in cands])
                np.testing.assert_array_equal(g["sharing"][q, :k], [c[1] for c in cands])
                assert g["score"][q, :k].tobytes() == np.array([c[2] for c in cands], np.float64).tobytes(), (N, ratio, filt, q)
                assert (g["frame"][q, k:] == -7).all()                      # entries past the count are not written
                # what keeps this from passing vacuously, on the restatement's own output
                if src[q] >= 0 and not filt:
                    assert src[q] in [c[0] for c in cands] and max(cands, key=lambda c: c[2])[0] == src[q]
                seen["thr"] += any(8 <= s < thr for s in sharing[q].values())
                seen["min_words"] += any(s < 8 and thr == 8 for s in sharing[q].values())
                if filt:
                    seen["index"] += any(s >= thr and f >= max_index[q] for f, s in sharing[q].items())
                    seen["exclude"] += any(s >= thr and f < max_index[q] and f in excl[q] for f, s in sharing[q].items())
                seen["empty"] += not cands
    assert seen["empty"] > 0
    if N >= 300:
        assert all(v > 0 for v in seen.values()), seen
    # a candidate list larger than its capacity: the full count, the first ccap entries
    got = _query_dev(db, qi, qv, qnw, 0.3, ccap=1 if N == 1 else 16, dense=False)
    for q in range(64):
        _, _, cands = ref.candidates(qvec[q][0], qvec[q][1], 0.3, 8, None, None, sharing[q])
        k = min(len(cands), got["frame"].shape[1])
        assert int(got["ncand"][q]) == len(cands)
        np.testing.assert_array_equal(got["frame"][q, :k].cpu().numpy(), [c[0] for c in cands[:k]])
    if N >= 300:
        assert int(got["ncand"].max()) > 16
    # the project's ranking: a stable sort of the restatement's list
    full = _query_dev(db, qi, qv, qnw, 0.3, dense=False)
    for K in (3, 8):
        top = torch.full((64, K), -9, dtype=torch.int32, device="cuda")
        tsc = torch.full((64, K), float("nan"), dtype=torch.float64, device="cuda")
        db.topk_dev(full["frame"], full["score"], full["ncand"], top, tsc)
        torch.cuda.synchronize()
        for q in range(64):
            _, _, cands = ref.candidates(qvec[q][0], qvec[q][1], 0.3, 8, None, None, sharing[q])
            assert top[q].cpu().tolist() == br.topk(cands, K), (N, K, q)
            by = dict((c[0], c[2]) for c in cands)
            assert tsc[q].cpu().numpy().tobytes() == np.array([by.get(f, 0.0) for f in br.topk(cands, K)], np.float64).tobytes()
    db.close()


def test_results_do_not_depend_on_how_frames_are_added_or_queries_batched():
    import torch
    from airslam_amd import api
    N = 300
    db, host, feats = _build(N, 4242)
    qf, qn, _ = _queries(N, feats, 99)
    _, _, qi, qv, qnw, _ = _vectors_dev(qf, qn)
    want = _query_dev(db, qi, qv, qnw, 0.3)
    key = lambda r, q: tuple(r[k][q].cpu().numpy().tobytes() for k in ("frame", "sharing", "score", "ncand", "max_sharing", "dense"))
    for q in (0, 5, 30, 63):                               # one query at a time
        one = _query_dev(db, qi[q:q + 1].contiguous(), qv[q:q + 1].contiguous(), qnw[q:q + 1].contiguous(), 0.3)
        assert key(one, 0) == key(want, q)
    # frame by frame through the host entry, then clear + one batch: the same bytes
    db2 = api.BowDatabase(_ctx(), N, CAP)
    ids = np.zeros((N, CAP), np.uint32)
    vals = np.zeros((N, CAP), np.float64)
    nw = np.zeros(N, np.int32)
    for f, (i, v) in enumerate(host):
        ids[f, :len(i)], vals[f, :len(i)], nw[f] = i, v, len(i)
    for f in range(N):
        db2.add(ids[f:f + 1], vals[f:f + 1], nw[f:f + 1])
    assert db2.size == N
    with pytest.raises(api.AirfeError):
        db2.add(ids[:1], vals[:1], nw[:1])                 # full: an error, nothing written
    got = _query_dev(db2, qi, qv, qnw, 0.3)
    assert all(key(got, q) == key(want, q) for q in range(64))
    db2.clear()
    assert db2.size == 0
    empty = _query_dev(db2, qi, qv, qnw, 0.3)
    assert int(empty["ncand"].abs().sum()) == 0 and int(empty["max_sharing"].abs().sum()) == 0
    db2.add_batch_dev(torch.from_numpy(ids.view(np.int32)).cuda(), torch.from_numpy(vals).cuda(), torch.from_numpy(nw).cuda())
    got = _query_dev(db2, qi, qv, qnw, 0.3)
    assert all(key(got, q) == key(want, q) for q in range(64))
    db2.close()
    db.close()


@pytest.mark.parametrize("rejection", [False, True])
def test_composite_equals_the_steps_done_by_hand(rejection):
    """map_user.cc:360-376 on planted pairs: 4 queries x 3 candidates; frame 2 q + 1 is query q's revisit (tests/planted.py), the others are unrelated"""
    import torch
    from airslam_amd import api
    ctx = _ctx()
    Q, K, N = 4, 3, 9
    qf = np.zeros((Q, CAP, 259), np.float32)
    dbf = np.zeros((N, CAP, 259), np.float32)
    qn, dn = np.zeros(Q, np.int32), np.zeros(N, np.int32)
    for f in range(N):
        k = 300 + 10 * f
        dbf[f, :k], dn[f] = features(k, 900 + f), k
    for q in range(Q):
        a, b = planted_pair(380 - 20 * q, 360, 70 + q)
        qf[q, :len(a)], qn[q] = a, len(a)
        dbf[2 * q + 1, :], dn[2 * q + 1] = 0, len(b)
        dbf[2 * q + 1, :len(b)] = b
    db = api.BowDatabase(ctx, N, CAP, keep_features=True)
    z = torch.zeros((N, CAP), dtype=torch.int32, device="cuda")
    db.add_batch_dev(z, torch.zeros((N, CAP), dtype=torch.float64, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda"),
                     torch.from_numpy(dbf).cuda(), torch.from_numpy(dn).cuda())
    cand = np.array([[0, 1, 2], [3, -1, 8], [-1, -1, -1], [7, 7, 6]], np.int32)      # the revisit second / first / no candidate / the revisit twice, then another
    qt, qnt, ct = torch.from_numpy(qf).cuda(), torch.from_numpy(qn).cuda(), torch.from_numpy(cand).cuda()
    best = torch.full((Q,), -9, dtype=torch.int32, device="cuda")
    idx = torch.full((Q, CAP, 2), -9, dtype=torch.int32, device="cuda")
    sc = torch.full((Q, CAP), float("nan"), dtype=torch.float32, device="cuda")
    nm = torch.full((Q,), -9, dtype=torch.int32, device="cuda")
    nma = torch.full((Q, K), -9, dtype=torch.int32, device="cuda")
    db.match_candidates_batch_dev(qt, qnt, ct, best, idx, sc, nm, nma, outlier_rejection=rejection)
    torch.cuda.synchronize()
    # by hand through the existing entries
    P = Q * K
    flat = cand.reshape(-1)
    hole = flat < 0
    f0 = torch.zeros((P, CAP, 259), dtype=torch.float32, device="cuda")
    f1 = torch.zeros((P, CAP, 259), dtype=torch.float32, device="cuda")
    n0, n1 = np.zeros(P, np.int32), np.zeros(P, np.int32)
    dbt = torch.from_numpy(dbf).cuda()
    for p in range(P):
        if not hole[p]:
            f0[p], f1[p] = qt[p // K], dbt[int(flat[p])]
            n0[p], n1[p] = qn[p // K], dn[flat[p]]
    pi = torch.zeros((P, CAP, 2), dtype=torch.int32, device="cuda")
    psc = torch.zeros((P, CAP), dtype=torch.float32, device="cuda")
    pn = torch.zeros((P,), dtype=torch.int32, device="cuda")
    ctx.match_lightglue_batch_dev(f0, torch.from_numpy(n0).cuda(), f1, torch.from_numpy(n1).cuda(), pi, psc, pn)
    if rejection:
        ctx.fundamental_ransac_batch_dev(f0, f1, pi, psc, pn)
    torch.cuda.synchronize()
    pn_h, pi_h, ps_h = pn.cpu().numpy(), pi.cpu().numpy(), psc.cpu().numpy()
    assert (pn_h[hole] == 0).all()
    np.testing.assert_array_equal(nma.cpu().numpy().reshape(-1), pn_h)
    for q in range(Q):
        slot, frame, length = br.best_candidate(cand[q].tolist(), pn_h[q * K:(q + 1) * K].tolist())
        assert int(best[q]) == frame and int(nm[q]) == length, (q, rejection)
        if slot >= 0:
            p = q * K + slot
            assert idx[q, :length].cpu().numpy().tobytes() == pi_h[p, :length].tobytes()
            assert sc[q, :length].cpu().numpy().tobytes() == ps_h[p, :length].tobytes()
        assert (idx[q, length:].cpu().numpy() == -9).all()
    assert [int(b) for b in best] == [1, 3, -1, 7]               # the true revisit wins (first of the equal lists for query 3), with a non-trivial list
    assert all(int(nm[q]) >= 50 for q in (0, 1, 3)) and int(nm[2]) == 0
    with pytest.raises(api.AirfeError):                          # Q * K above cfg.max_batch is a return code
        big = torch.zeros((4, 5), dtype=torch.int32, device="cuda")
        db.match_candidates_batch_dev(qt, qnt, big, best, idx, sc, nm, None)
    db.close()
