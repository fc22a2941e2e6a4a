"""Relocalisation's junction term on the device (include/airfe.h "Junction term"): the three kernels of kernels_junction.hip through their entries against
the literal restatement of the reference (tests/junction_ref.py, which tests/test_junction_cpu.py pins to hand-written answers) — every comparison exact:
edges, per-line pairs, tables, counts, and `extra` bit for bit.  The junction database is a second context with a k = 10, L = 3 vocabulary."""
import numpy as np
import pytest

import bowgroup_cases as bc
import bowgroup_ref as gr
import junction_ref as jr
from airslam_amd import weights

pytestmark = pytest.mark.gpu
W, H = 512, 512
_S = {}


def _voc():
    if "voc" not in _S:
        _S["voc"] = weights.synthetic_vocabulary(1234, k=10, L=3)
        v = _S["voc"]
        leaf = np.asarray(v["n_children"]) == 0
        ww = np.zeros(int(np.asarray(v["word_id"])[leaf].max()) + 1)
        ww[np.asarray(v["word_id"])[leaf]] = np.asarray(v["weight"])[leaf]
        _S["word_weight"] = ww
    return _S["voc"]


def _jctx():
    """the junction database's context: no network pack, the junction vocabulary"""
    if "jctx" not in _S:
        from airslam_amd import api
        c = api.Context(max_keypoints=1024)
        c.bow_load(_voc())
        _S["jctx"] = c
    return _S["jctx"]


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _i32(shape, fill=-7):
    import torch
    return torch.full(shape, fill, dtype=torch.int32, device="cuda")


def _pack(frames, capJ, capL, hostile=0, nlines=None):
    """frames: dict(junc [nj][259], lines [nl][4]) -> the batched PLNet layout; rows past the counts hold `hostile` garbage"""
    B = len(frames)
    junc = np.zeros((B, capJ, 259), np.float32)
    lines = np.zeros((B, capL, 4), np.float64)
    if hostile:
        junc[:] = 9.0
        junc[:, :, 1:3] = [np.nan, 3e9][hostile % 2] if hostile > 1 else 7.0
        lines[:] = np.nan if hostile > 1 else 7.0
    nj, nl = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b, f in enumerate(frames):
        nj[b], nl[b] = len(f["junc"]), min(len(f["lines"]), capL)
        junc[b, :nj[b]] = f["junc"]
        lines[b, :nl[b]] = f["lines"][:capL]
    if nlines is not None:
        nl = np.asarray(nlines, np.int32)
    return junc, nj, lines, nl


def _connect(frames, capJ, capL, ecap, hostile=0, nlines=None, w=W, h=H):
    """-> per frame (edges [(a, b)], pairs [(a, b)], status) + the raw output arrays"""
    import torch
    junc, nj, lines, nl = _pack(frames, capJ, capL, hostile, nlines)
    B = len(frames)
    edge, ne, st, pair = _i32((B, ecap, 2)), _i32((B,)), _i32((B,)), _i32((B, capL, 2))
    _jctx().junction_connections_batch_dev(_up(lines), _up(nl), _up(junc), _up(nj), w, h, edge, ne, st, pair)
    torch.cuda.synchronize()
    edge, ne, st, pair = edge.cpu().numpy(), ne.cpu().numpy(), st.cpu().numpy(), pair.cpu().numpy()
    out = []
    for b in range(B):
        n = min(int(nl[b]), capL)
        assert 0 <= ne[b] <= ecap and (edge[b, ne[b]:] == -7).all() and (pair[b, n:] == -7).all(), b      # nothing written past the counts
        out.append(([tuple(e) for e in edge[b, :ne[b]].tolist()], [tuple(p) for p in pair[b, :n].tolist()], int(st[b])))
    return out, (edge, ne, st, pair)


def _frame(junc_xy, lines):
    j = np.zeros((len(junc_xy), 259), np.float32)
    if len(junc_xy):
        j[:, 1:3] = np.asarray(junc_xy, np.float32)
    return dict(junc=j, lines=np.asarray(lines, np.float64).reshape(-1, 4))


def test_hand_cases_through_the_connect_kernel():
    cases = jr.hand_cases()
    frames = [_frame(c["junc"], c["lines"]) for c in cases]
    got, raw = _connect(frames, 8, 8, 16, w=20, h=16)
    for c, g in zip(cases, got):
        assert g == (c["edges"], c["pairs"], jr.OK), (c["name"], g)
    again, raw2 = _connect(frames, 8, 8, 16, hostile=2, w=20, h=16)     # other garbage past the counts, the same bytes
    assert all(a.tobytes() == b.tobytes() for a, b in zip(raw, raw2))
    # capL = 8 with nlines above it: clamped, the eight lines' answers
    c = cases[2]
    many = _frame(c["junc"], c["lines"] * 8)
    got, _ = _connect([many], 8, 8, 16, nlines=[100], w=20, h=16)
    assert got[0] == (c["edges"], c["pairs"] * 8, jr.OK)


def _shape_frames(ecap):
    """junction counts 0, 1, 63, 64, 65, 1024; edge counts 0, 1, 64, 65, ecap, ecap + 1; an empty frame between full ones; the lines of the large
    frames repeated three times (6144 and more lines: several rounds of the LDS merge)"""
    spec = [(63, 64, 1), (0, 0, 1), (1, 1, 1), (64, 65, 1), (65, 0, 1), (1024, ecap, 3), (0, 0, 1), (1024, ecap + 1, 3), (1024, 64, 1)]
    frames, want = [], []
    for nj, ne, rep in spec:
        pairs = jr.pairs_for_edges(nj, ne) if ne else []
        junc, lines, edges = jr.grid_case(nj, pairs)
        if nj == 0:
            lines = [(3.0, 3.0, 9.0, 3.0)]                              # a line without any junction to meet
        frames.append(_frame(junc, lines * rep))
        want.append((edges, (pairs if nj else [(-1, -1)]) * rep))
    return frames, want


def test_connect_kernel_shapes_overflow_and_batch_independence():
    ecap = 4096
    frames, want = _shape_frames(ecap)
    capL = max(len(f["lines"]) for f in frames) + 3
    got, raw = _connect(frames, 1024, capL, ecap, hostile=1, w=400, h=400)
    for b, (g, (edges, pairs)) in enumerate(zip(got, want)):
        over = len(edges) > ecap
        assert g == ([] if over else edges, pairs, jr.OVERFLOW if over else jr.OK), (b, g[2], len(g[0]), len(edges))
    assert [g[2] for g in got].count(jr.OVERFLOW) == 1
    # the host core on the same frames (tests/test_junction_cpu.py pins it to the restatement): the same answers
    ctx = _jctx()
    for b in (0, 3, 5, 7):
        e, p, st = ctx.junction_connections(frames[b]["lines"], frames[b]["junc"], 400, 400, ecap)
        assert ([tuple(x) for x in e.tolist()], [tuple(x) for x in p.tolist()], st) == got[b], b
    # a frame's bytes depend on neither B nor its position; two runs give the same bytes
    for b in (5, 7, 3):
        one, r1 = _connect([frames[b]], 1024, capL, ecap, hostile=2, w=400, h=400)
        assert one[0] == got[b] and all(x[0].tobytes() == y[b].tobytes() for x, y in zip(r1, raw)), b
    _, raw2 = _connect(frames, 1024, capL, ecap, hostile=1, w=400, h=400)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(raw, raw2))
    # a smaller ecap: exactly ecap edges fit, one more is status 2
    small, _ = _connect([frames[0], frames[3]], 1024, capL, 64, w=400, h=400)
    assert small[0] == (want[0][0], want[0][1], jr.OK) and small[1] == ([], want[3][1], jr.OVERFLOW)


# ---- the stored tables ------------------------------------------------------------------------------------------------------------------------------
def _words_dev(frames, cap):
    """the frames' junction rows through bow_vector_batch_dev on the junction context -> device (ids, vals, nw, word, junc, nj) + the words on the host"""
    import torch
    junc, nj, _, _ = _pack(frames, cap, 1)
    B = len(frames)
    jt, njt = _up(junc), _up(nj)
    ids, word = _i32((B, cap), 0), _i32((B, cap), 0)
    vals = torch.zeros((B, cap), dtype=torch.float64, device="cuda")
    nw = _i32((B,), 0)
    _jctx().bow_vector_batch_dev(jt, njt, ids, vals, nw, word_t=word)
    torch.cuda.synchronize()
    host = word.cpu().numpy().view(np.uint32)
    return dict(ids=ids, vals=vals, nw=nw, word=word, junc=jt, nj=njt), [host[b, :nj[b]].copy() for b in range(B)]


def _table_lists(t, b):
    return ([(int(t["uword"][b, i]), int(t["wcnt"][b, i]), int(t["wconn"][b, i])) for i in range(t["nuw"][b])],
            [(int(t["ukey"][b, i]), int(t["kcnt"][b, i])) for i in range(t["nuk"][b])])


def test_set_junctions_builds_the_tables():
    import torch
    from airslam_amd import api
    cap, ecap, N = 1024, 4096, 9
    rng = np.random.default_rng(11)
    specs = []                                                          # (words, edges): hand cases, then random ones with repeated words
    for t in jr.hand_terms():
        specs.append((t["wq"], t["eq"]))
    for nj, ne in ((63, 64), (1024, 4096), (65, 1)):
        words = rng.choice(np.array([0, 3, 5, 9, 17, 4000000000, jr.UINT_MAX], np.uint64), nj).astype(np.uint32)
        specs.append((words, jr.grid_case(nj, jr.pairs_for_edges(nj, ne))[2]))
    specs = specs[:N - 3] + specs[-3:]
    word = rng.choice(np.array([0, jr.UINT_MAX], np.uint32), (N, cap))   # hostile padding: words of 0 and UINT_MAX, huge indices past every count
    edge = np.full((N, ecap, 2), 2 ** 31 - 1, np.int32)
    edge[:, :, 1] = -2 ** 31
    nj, ne, st = np.zeros(N, np.int32), np.zeros(N, np.int32), np.zeros(N, np.int32)
    for b, (w, e) in enumerate(specs):
        nj[b], ne[b] = len(w), len(e)
        word[b, :nj[b]] = np.asarray(w, np.uint32)
        if len(e):
            edge[b, :ne[b]] = np.asarray(e, np.int32)
    st[1] = jr.OVERFLOW                                                 # a frame the connections gave up on
    db = api.BowDatabase(_jctx(), N + 2, cap)
    db.attach_junctions(ecap, 4)
    assert db.get_junctions(0, N + 2, cap, ecap)["status"].tolist() == [jr.UNSET] * (N + 2)
    db.set_junctions_dev(1, _up(word.view(np.int32)), _up(nj), _up(edge), _up(ne), _up(st))
    torch.cuda.synchronize()
    t = db.get_junctions(0, N + 2, cap, ecap)
    assert t["status"].tolist() == [jr.UNSET] + [0, jr.OVERFLOW] + [0] * (N - 2) + [jr.UNSET]
    assert t["nuw"][2] == 0 and t["nuk"][2] == 0
    for b, (w, e) in enumerate(specs):
        assert t["nj"][1 + b] == len(w) and t["word"][1 + b, :len(w)].tolist() == [int(x) for x in w], b
        if b != 1:
            assert _table_lists(t, 1 + b) == jr.tables(w, e), b
    big = jr.tables(*specs[-2])
    assert len(big[1]) > 5 and max(m for _, m in big[1]) > 50 and max(c for _, c, _ in big[0]) > 100      # repeated keys and words: the counts count
    # the host form, four frames at a time into another database: the same bytes
    db2 = api.BowDatabase(_jctx(), N + 2, cap)
    db2.attach_junctions(ecap, 4)
    for b0 in range(0, N, 4):
        db2.set_junctions(1 + b0, word[b0:b0 + 4], nj[b0:b0 + 4], edge[b0:b0 + 4], ne[b0:b0 + 4], st[b0:b0 + 4])
    t2 = db2.get_junctions(0, N + 2, cap, ecap)
    for k in ("nj", "nuw", "nuk", "status"):
        assert t[k].tobytes() == t2[k].tobytes(), k
    for b in range(1, N + 1):
        for k, n in (("word", "nj"), ("uword", "nuw"), ("wcnt", "nuw"), ("wconn", "nuw"), ("ukey", "nuk"), ("kcnt", "nuk")):
            assert t[k][b, :t[n][b]].tobytes() == t2[k][b, :t2[n][b]].tobytes(), (b, k)
    with pytest.raises(api.AirfeError):                                 # more frames than the staging holds, frames beyond max_frames: nothing changes
        db2.set_junctions(0, word[:5], nj[:5], edge[:5], ne[:5])
    with pytest.raises(api.AirfeError):
        db.set_junctions_dev(N - 2, _up(word.view(np.int32)), _up(nj), _up(edge), _up(ne))
    torch.cuda.synchronize()
    assert all(db.get_junctions(0, N + 2, cap, ecap)[k].tobytes() == t[k].tobytes() for k in t)
    db.close()
    db2.close()


# ---- the term ---------------------------------------------------------------------------------------------------------------------------------------
def _reference(frames, queries, fwords, qwords):
    """junction_ref.reference_table on the DEVICE'S words (the vocabulary descent is the existing, separately tested kernel)"""
    ww = _S["word_weight"]
    def with_words(fr, w):
        wt = np.where(w == jr.UINT_MAX, 0.0, ww[np.minimum(w, len(ww) - 1)])
        return dict(fr, word=w, weight=wt)
    return jr.reference_table([with_words(f, w) for f, w in zip(frames, fwords)], [with_words(q, w) for q, w in zip(queries, qwords)], W, H)


def _table():
    """130 stored frames and 3 queries over one pool of words; frame 7 has no junction, frame 20 has 1024 junctions and ~4000 edges, frame 30 overflows"""
    if "table" not in _S:
        voc = _voc()
        sizes = [int(s) for s in np.random.default_rng(3).integers(5, 40, 130)]
        sizes[7] = 0
        frames, queries = jr.seeded_table(voc, seed=21, n_frames=130, n_queries=3, sizes=sizes)
        rng = np.random.default_rng(22)
        pool = jr.pool_nodes(voc, 21)
        big = jr.seeded_frame(rng, voc, pool, 1024, 2200)
        frames[20] = big
        over = jr.seeded_frame(rng, voc, pool, 1024, 4500)
        frames[30] = over
        _S["table"] = (frames, queries)
    return _S["table"]


def _connect_dev(frames, cap, capL, ecap):
    import torch
    junc, nj, lines, nl = _pack(frames, cap, capL, hostile=2)
    B = len(frames)
    edge, ne, st = _i32((B, ecap, 2)), _i32((B,)), _i32((B,))
    _jctx().junction_connections_batch_dev(_up(lines), _up(nl), _up(junc), _up(nj), W, H, edge, ne, st)
    torch.cuda.synchronize()
    return dict(edge=edge, nedge=ne, status=st, lines=_up(lines), nlines=_up(nl))


def _term(db, qv, qc, Q, counts=True, rows=None):
    import torch
    N = db.size
    sel = (lambda t: t[:Q]) if rows is None else (lambda t: t[rows].contiguous())
    extra = torch.full((Q, max(N, 1)), float("nan"), dtype=torch.float64, device="cuda")
    mn, lmn = (_i32((Q, max(N, 1))), _i32((Q, max(N, 1)))) if counts else (None, None)
    db.junction_term_batch_dev(sel(qv["ids"]), sel(qv["vals"]), sel(qv["nw"]), sel(qv["word"]), sel(qv["nj"]), sel(qc["edge"]), sel(qc["nedge"]), extra,
                               qstatus_t=sel(qc["status"]), match_num_t=mn, line_match_num_t=lmn)
    torch.cuda.synchronize()
    return extra.cpu().numpy()[:, :N], None if mn is None else mn.cpu().numpy()[:, :N], None if lmn is None else lmn.cpu().numpy()[:, :N]


def test_term_equals_the_restatement_bit_for_bit():
    import torch
    from airslam_amd import api
    frames, queries = _table()
    cap, capL, ecap, NMAX = 1024, 4608, 4096, 130
    fv, fwords = _words_dev(frames, cap)
    qv, qwords = _words_dev(queries, cap)
    fc, qc = _connect_dev(frames, cap, capL, ecap), _connect_dev(queries, cap, capL, ecap)
    fst = fc["status"].cpu().numpy()
    assert fst[30] == jr.OVERFLOW and (np.delete(fst, 30) == 0).all() and int(fc["nedge"][20]) > 2000
    mn, lmn, ex, sc = _reference(frames, queries, fwords, qwords)
    mn[:, 30], lmn[:, 30], ex[:, 30] = 0, 0, 0.0                        # status 2: a term of 0 (the contract; the reference has no such frame)
    # asserted ON THE REFERENCE'S NUMBERS: the comparison cannot pass on zeros
    assert (lmn > 0).mean() >= 0.5 and ((mn > 0) & (lmn == 0)).any() and (mn == 0).any() and (sc > 0).mean() > 0.5
    assert mn[:, 7].tolist() == [0, 0, 0] and lmn[:, 20].min() > 50
    db = api.BowDatabase(_jctx(), NMAX, cap)
    db.attach_junctions(ecap, 3)
    assert _term(db, qv, qc, 1)[0].shape == (1, 0)                      # an empty database: nothing to write
    first = 0
    for N in (1, 63, 64, 65, 130):                                      # around the frames-per-workgroup boundary, more than one slice
        s = slice(first, N)
        db.add_batch_dev(fv["ids"][s], fv["vals"][s], fv["nw"][s])
        if N < 130:
            db.set_junctions_dev(first, fv["word"][s], fv["nj"][s], fc["edge"][s], fc["nedge"][s], fc["status"][s])
        else:                                                           # frames 100 .. 129 stay without junction state: a term of 0
            s = slice(first, 100)
            db.set_junctions_dev(first, fv["word"][s], fv["nj"][s], fc["edge"][s], fc["nedge"][s], fc["status"][s])
        first = N
        want = [a[:, :N].copy() for a in (ex, mn, lmn)]
        for a in want:
            a[:, 100:] = 0
        for Q in (1, 3):
            got = _term(db, qv, qc, Q)
            assert np.array_equal(got[1], want[1][:Q]) and np.array_equal(got[2], want[2][:Q]), (N, Q)
            assert got[0].tobytes() == want[0][:Q].tobytes(), (N, Q, np.argwhere(got[0] != want[0][:Q])[:5])
    # a query's bytes do not depend on Q or on its position; without the count outputs; two runs give the same bytes
    full = _term(db, qv, qc, 3)
    for rows in ([2], [2, 0], [1, 1, 2]):
        got = _term(db, qv, qc, len(rows), rows=rows)
        assert all(g.tobytes() == f[rows].tobytes() for g, f in zip(got, full)), rows
    assert _term(db, qv, qc, 3, counts=False)[0].tobytes() == full[0].tobytes()
    # a query with status 2 and one with 1024 junctions against three frames (the large one among them)
    three = api.BowDatabase(_jctx(), 3, cap)
    three.attach_junctions(ecap, 2)
    pick = [19, 20, 21]
    sel = lambda t: t[19:22]  # noqa: E731
    three.add_batch_dev(sel(fv["ids"]), sel(fv["vals"]), sel(fv["nw"]))
    three.set_junctions_dev(0, sel(fv["word"]), sel(fv["nj"]), sel(fc["edge"]), sel(fc["nedge"]), sel(fc["status"]))
    bq = [frames[20], frames[30]]
    bv, bwords = _words_dev(bq, cap)
    bcn = _connect_dev(bq, cap, capL, ecap)
    assert bcn["status"].cpu().numpy().tolist() == [0, jr.OVERFLOW]
    bmn, blmn, bex, _ = _reference([frames[f] for f in pick], bq[:1], [fwords[f] for f in pick], bwords[:1])
    got = _term(three, bv, bcn, 2)
    assert np.array_equal(got[1][0], bmn[0]) and np.array_equal(got[2][0], blmn[0]) and got[0][0].tobytes() == bex[0].tobytes()
    assert blmn[0, 1] > 4000 and not got[0][1].any() and not got[1][1].any() and not got[2][1].any()
    print("self term of the 1024-junction frame:", bmn[0, 1], blmn[0, 1], bex[0, 1])
    # refusals leave the outputs untouched
    extra = torch.full((4, 3), 5.0, dtype=torch.float64, device="cuda")
    four = lambda t: torch.cat([t, t])  # noqa: E731
    with pytest.raises(api.AirfeError):                                 # Q > max_queries
        three.junction_term_batch_dev(four(bv["ids"]), four(bv["vals"]), four(bv["nw"]), four(bv["word"]), four(bv["nj"]), four(bcn["edge"]), four(bcn["nedge"]),
                                      extra)
    plain = api.BowDatabase(_jctx(), 3, cap)
    with pytest.raises(api.AirfeError):                                 # no junction state
        plain.junction_term_batch_dev(bv["ids"], bv["vals"], bv["nw"], bv["word"], bv["nj"], bcn["edge"], bcn["nedge"], extra)
    with pytest.raises(api.AirfeError):
        plain.attach_junctions(4097, 2)
    with pytest.raises(api.AirfeError):                                 # ecap > 4096, capJ > 1024
        _connect([frames[0]], 64, 64, 4097)
    with pytest.raises(api.AirfeError):
        _connect([frames[0]], 1025, 64, 64)
    torch.cuda.synchronize()
    assert (extra.cpu().numpy() == 5.0).all()
    for d in (db, three, plain):
        d.close()


def test_composites_equal_the_chain_of_single_entries():
    import torch
    from airslam_amd import api
    frames, queries = _table()
    frames = frames[:24]                                                # with the empty frame 7 and the 1024-junction frame 20
    cap, capL, ecap = 1024, 4608, 4096
    fv, _ = _words_dev(frames, cap)
    qv, _ = _words_dev(queries, cap)
    fc, qc = _connect_dev(frames, cap, capL, ecap), _connect_dev(queries, cap, capL, ecap)
    a = api.BowDatabase(_jctx(), 24, cap)
    a.attach_junctions(ecap, 12)
    a.add_batch_dev(fv["ids"], fv["vals"], fv["nw"])
    a.set_junctions_dev(0, fv["word"], fv["nj"], fc["edge"], fc["nedge"], fc["status"])
    b = api.BowDatabase(_jctx(), 24, cap)
    b.attach_junctions(ecap, 12)
    for s in (slice(0, 12), slice(12, 24)):                             # add_junction_frames: vector, add, connections, tables
        b.add_junction_frames_batch_dev(fv["junc"][s], fv["nj"][s], fc["lines"][s], fc["nlines"][s], W, H)
    torch.cuda.synchronize()
    assert a.size == b.size == 24
    ta, tb = a.get_junctions(0, 24, cap, ecap), b.get_junctions(0, 24, cap, ecap)
    for k in ("nj", "nuw", "nuk", "status"):
        assert ta[k].tobytes() == tb[k].tobytes(), k
    for f in range(24):
        for k, n in (("word", "nj"), ("uword", "nuw"), ("wcnt", "nuw"), ("wconn", "nuw"), ("ukey", "nuk"), ("kcnt", "nuk")):
            assert ta[k][f, :ta[n][f]].tobytes() == tb[k][f, :tb[n][f]].tobytes(), (f, k)
    chain = _term(a, qv, qc, 3)
    for db in (a, b):                                                   # the composite on either database: the chain's bytes (so b's vectors are a's too)
        extra = torch.full((3, 24), float("nan"), dtype=torch.float64, device="cuda")
        mn, lmn = _i32((3, 24)), _i32((3, 24))
        db.junction_extra_batch_dev(qv["junc"], qv["nj"], qc["lines"], qc["nlines"], W, H, extra, mn, lmn)
        torch.cuda.synchronize()
        got = (extra.cpu().numpy(), mn.cpu().numpy(), lmn.cpu().numpy())
        assert all(g.tobytes() == c.tobytes() for g, c in zip(got, chain))
    assert (chain[2] > 0).mean() > 0.5
    extra = torch.full((3, 24), 5.0, dtype=torch.float64, device="cuda")
    with pytest.raises(api.AirfeError):                                 # capJ must be the database's; full database
        a.junction_extra_batch_dev(qv["junc"][:, :512].contiguous(), qv["nj"], qc["lines"], qc["nlines"], W, H, extra)
    with pytest.raises(api.AirfeError):
        a.add_junction_frames_batch_dev(fv["junc"][:1], fv["nj"][:1], fc["lines"][:1], fc["nlines"][:1], W, H)
    torch.cuda.synchronize()
    assert (extra.cpu().numpy() == 5.0).all() and a.size == 24
    a.close()
    b.close()


# ---- end to end: the term re-ranks the groups of the relocalisation composite ---------------------------------------------------------------------------
def test_the_term_swaps_two_nearly_tied_groups_in_relocalize():
    """One query, eight stored frames; frames 1 and 6 are both revisits of the query (their point scores are close), every frame is a group of its own,
    K = 1: the matcher sees the first group's deputy only.  The junction frames are chosen AFTER the run without the term: the loser gets the query's own
    junctions and lines (a term above 1), the winner a frame without junctions (a term of 0), the others unrelated junctions."""
    import torch
    import test_gpu_reloc as tr
    from airslam_amd import api
    from planted import features, planted_pair
    CAP, N = tr.CAP, 8
    ctx = tr._ctx()
    a, b1 = planted_pair(380, 360, 70)
    b2 = features(360, 9070)
    rng = np.random.default_rng(9)
    k = 170
    b2[:k, 3:] = a[:k, 3:] + 0.05 * rng.normal(size=(k, 256)).astype(np.float32)
    b2[:k, 3:] /= np.linalg.norm(b2[:k, 3:], axis=1, keepdims=True)
    b2[:k, 1:3] = a[:k, 1:3] - (12, 0)
    dbf, dn = np.zeros((N, CAP, 259), np.float32), np.zeros(N, np.int32)
    for f in range(N):
        fr = b1 if f == 1 else b2 if f == 6 else features(300 + 5 * f, 900 + f)
        dbf[f, :len(fr)], dn[f] = fr, len(fr)
    qf, qn = np.zeros((1, CAP, 259), np.float32), np.array([len(a)], np.int32)
    qf[0, :len(a)] = a
    xyz = np.random.default_rng(4).uniform(-5, 5, (N, CAP, 3)) + (0, 0, 8)
    ft, nt = _up(dbf), _up(dn)
    ids, vals, nw = _i32((N, CAP), 0), torch.zeros((N, CAP), dtype=torch.float64, device="cuda"), _i32((N,), 0)
    ctx.bow_vector_batch_dev(ft, nt, ids, vals, nw)
    db = api.BowDatabase(ctx, N, CAP, keep_features=True)
    db.add_batch_dev(ids, vals, nw, ft, nt)
    db.attach_map(64)
    db.set_points(0, xyz)
    covis = bc.csr(N, {f: [(f, 30)] for f in range(N)})
    db.set_covisibility(*covis)

    def run(extra):
        o = tr._reloc_buffers(1)
        db.relocalize_batch_dev(_up(qf), _up(qn), tr.CAM, tr.THR, tr.MIN_INLIER, o["ok"], o["stage"], o["Twc"], o["best"], o["num"], o["mask"], o["idx"],
                                o["score"], o["nmatch"], pnp_count_t=o["pnp_count"], extra_t=extra, K=1)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in o.items()}

    plain = run(None)
    winner = int(plain["best"][0])
    assert winner in (1, 6)
    loser = 7 - winner
    # the point database's candidate list, for the grouping restatement
    qi, qv, qnw = _i32((1, CAP), 0), torch.zeros((1, CAP), dtype=torch.float64, device="cuda"), _i32((1,), 0)
    ctx.bow_vector_batch_dev(_up(qf), _up(qn), qi, qv, qnw)
    cf, cs, sc, nc, ms = _i32((1, N)), _i32((1, N)), torch.zeros((1, N), dtype=torch.float64, device="cuda"), _i32((1,)), _i32((1,))
    db.query_batch_dev(qi, qv, qnw, cf, cs, sc, nc, ms, ratio=0.3)
    torch.cuda.synchronize()
    n = int(nc[0])
    cands = list(zip(cf.cpu().numpy()[0, :n].tolist(), sc.cpu().numpy()[0, :n].tolist()))
    score = dict(cands)
    print("point scores of the two revisits:", score.get(1), score.get(6))
    assert 1 in score and 6 in score and score[7 - winner] >= 0.5 * score[winner]      # close enough for the loser's group to survive the 0.5 filter
    cd = gr.covis_dict(*covis)
    assert gr.group(gr.RELOC, cands, cd, 1)["frames"] == [winner]
    # the junction side: the query's junction frame, its copy at the loser, unrelated frames elsewhere
    voc = _voc()
    jrng = np.random.default_rng(31)
    pool, other = jr.pool_nodes(voc, 31), jr.pool_nodes(voc, 1031)
    other = np.array([x for x in other if x not in set(pool.tolist())])
    query = jr.seeded_frame(jrng, voc, pool, 50, 120)
    jframes = [query if f == loser else jr.seeded_frame(jrng, voc, other, 0 if f == winner else 30, 60) for f in range(N)]
    cap, capL, ecap = 64, 128, 512
    jdb = api.BowDatabase(_jctx(), N, cap)
    jdb.attach_junctions(ecap, N)
    fj, fnj, fl, fnl = (_up(x) for x in _pack(jframes, cap, capL))
    jdb.add_junction_frames_batch_dev(fj, fnj, fl, fnl, W, H)
    qj, qnj, ql, qnl = (_up(x) for x in _pack([query], cap, capL))
    extra = torch.full((1, N), float("nan"), dtype=torch.float64, device="cuda")
    jdb.junction_extra_batch_dev(qj, qnj, ql, qnl, W, H, extra)
    torch.cuda.synchronize()
    # the reference's table from the host, on the device's words
    _, fwords = _words_dev(jframes, cap)
    _, qwords = _words_dev([query], cap)
    mn, lmn, ex, _ = _reference(jframes, [query], fwords, qwords)
    assert extra.cpu().numpy().tobytes() == ex.tobytes()
    assert ex[0, loser] > 1.0 and ex[0, winner] == 0.0 and lmn[0, loser] > 0
    with_dev, with_ref = run(extra), run(_up(ex))
    assert all(with_dev[k].tobytes() == with_ref[k].tobytes() for k in with_dev)
    want = gr.group(gr.RELOC, cands, cd, 1, extra=ex[0])
    assert want["frames"] == [loser] and with_dev["best"].tolist() == [loser] and plain["best"].tolist() == [winner]
    db.close()
    jdb.close()
