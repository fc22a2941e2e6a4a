"""TEST INFRASTRUCTURE: relocalisation's junction term restated statement by statement from the reference, with lists, sets and Python floats (IEEE doubles):
Frame::FindJunctionConnections (src/frame.cc:581-629) with its dense H x W map and its window scan, and the counting of MapUser::Relocalization
(src/map_user.cc:287-331) with an inverted file per word, match_matrix and the four nested loops.  Deliberately NOT the histogram form of
airslam_amd/csrc/junction_core.h: include/airfe.h ("Junction term") claims the two agree, the tests check it.  The score is bowdb_ref.score.
Where the reference is undefined the stated differences of the contract apply: a junction whose pixel is outside the image owns no cell; an endpoint whose
coordinate + 0.5 is not finite or not inside (-2^31, 2^31) matches nothing."""
from collections import Counter

import numpy as np

import bowdb_ref as br

UINT_MAX = 0xFFFFFFFF
WS = 2                                                                  # frame.cc:593
OK, UNSET, OVERFLOW = 0, 1, 2


def _int(v):
    """int(v + 0.5) of C++ on a double: the sum in double, truncated towards zero; None where the conversion is undefined"""
    t = float(v) + 0.5
    if not (-2147483648.0 < t < 2147483648.0):
        return None
    return int(t)


def find_junction_connections(lines, junc_xy, W, H):
    """frame.cc:581-629.  lines: [(x0, y0, x1, y1)] doubles; junc_xy: [(jx, jy)] float32 values (rows 1, 2 of the 259-row matrix).
    -> (connected_junctions: a set per junction, per line the pair (id1, id2) or (-1, -1))"""
    nj = len(junc_xy)
    connected = [set() for _ in range(nj)]                              # :582
    junction_map = [[-1] * W for _ in range(H)]                         # :586
    for i in range(nj):                                                 # :587-591: a float plus the double 0.5
        x, y = _int(np.float32(junc_xy[i][0])), _int(np.float32(junc_xy[i][1]))
        if x is None or y is None or not (0 <= x < W and 0 <= y < H):
            continue                                                    # STATED DIFFERENCE: the reference writes out of bounds
        junction_map[y][x] = i

    def match_junction(x, y):                                           # :594-617
        junction_id = -1
        d_min = 2 * WS + 1
        xi, yi = _int(x), _int(y)
        if xi is None or yi is None:
            return -1                                                   # STATED DIFFERENCE: the reference's conversion is undefined
        for i in range(max(yi - WS, 0), min(yi + WS, H - 1) + 1):
            for j in range(max(xi - WS, 0), min(xi + WS, W - 1) + 1):
                if junction_map[i][j] >= 0:
                    d = abs(yi - i) + abs(xi - j)
                    if d < d_min:
                        junction_id = junction_map[i][j]
                        d_min = d
                        if d_min == 0:
                            return junction_id
        return junction_id

    pairs = []
    for line in lines:                                                  # :619-628
        id1 = match_junction(line[0], line[1])
        if id1 < 0:
            pairs.append((-1, -1))
            continue
        id2 = match_junction(line[2], line[3])
        if id2 < 0:
            pairs.append((-1, -1))
            continue
        connected[id1].add(id2)
        connected[id2].add(id1)
        pairs.append((id1, id2))
    return connected, pairs


def edges_of(connected):
    """the directed edges (i, i') with i' in connected[i], ascending: what the library hands out for a frame"""
    return [(i, j) for i in range(len(connected)) for j in sorted(connected[i])]


def connected_of(edges, nj):
    c = [set() for _ in range(nj)]
    for a, b in edges:
        c[a].add(b)
    return c


def term(words_q, conn_q, words_f, conn_f, literal=False):
    """map_user.cc:290-327 for one stored frame.  words_*: word_of_features (UINT_MAX: weight 0), conn_*: the sets.  -> (match_num, line_match_num).
    literal: the two innermost loops as Python loops; otherwise the same count as a sum over the sub-matrix of match_matrix."""
    nq, nf = len(words_q), len(words_f)
    inverted = {}                                                       # database.cc:70-75, 98-106: this frame's entry of _inverted_file[word]
    for j, w in enumerate(words_f):
        if int(w) != UINT_MAX:
            inverted.setdefault(int(w), []).append(j)
    match_matrix = np.zeros((nq, max(nf, 1)), bool)                     # :293
    match_junctions = [[] for _ in range(nq)]                           # :295-296
    for i in range(nq):                                                 # :298-308
        word_id = int(words_q[i])
        if word_id >= UINT_MAX:
            continue
        if word_id not in inverted:
            continue
        match_junctions[i] = inverted[word_id]
        for j in inverted[word_id]:
            match_matrix[i][j] = True
    match_num = 0
    line_match_num = 0
    for i in range(nq):                                                 # :313-327
        if len(match_junctions[i]) < 1 or len(conn_q[i]) < 1:
            continue
        match_num += len(match_junctions[i])
        for junction_id in match_junctions[i]:
            if len(conn_f[junction_id]) < 1:
                continue
            if literal:
                for idx1 in conn_q[i]:
                    for idx2 in conn_f[junction_id]:
                        if match_matrix[idx1][idx2]:
                            line_match_num += 1
            else:
                line_match_num += int(match_matrix[np.ix_(sorted(conn_q[i]), sorted(conn_f[junction_id]))].sum())
    return match_num, line_match_num


def extra(score, match_num, line_match_num):
    """:329-331: what is added to the group's score"""
    rate = float(line_match_num) / match_num if match_num > 0 else 0
    return float(score) * (1 + rate)


def tables(words, edges):
    """what airfe_bowdb_get_junctions reads back for a frame (NOT the yardstick of the term): the word table [(word, cnt, conn)] and the key table
    [(word[a] << 32 | word[b], multiplicity)], both ascending"""
    nj = len(words)
    has = {a for a, b in edges if 0 <= a < nj and 0 <= b < nj}
    cnt, conn = Counter(), Counter()
    for i, w in enumerate(words):
        if int(w) != UINT_MAX:
            cnt[int(w)] += 1
            conn[int(w)] += i in has
    keys = Counter((int(words[a]) << 32) | int(words[b]) for a, b in edges
                   if 0 <= a < nj and 0 <= b < nj and int(words[a]) != UINT_MAX and int(words[b]) != UINT_MAX)
    return [(w, cnt[w], conn[w]) for w in sorted(cnt)], sorted(keys.items())


# ---- cases written out by hand ----------------------------------------------------------------------------------------------------------------------
def hand_cases():
    """connections: dict(name, W, H, junc [(x, y)], lines [(x0, y0, x1, y1)], edges, pairs) — edges and pairs worked out by hand from frame.cc:581-629"""
    nan, inf = float("nan"), float("inf")
    two = [(3, 3), (10, 8)]
    c = []
    add = lambda name, junc, lines, edges, pairs, W=20, H=16: c.append(dict(name=name, W=W, H=H, junc=junc, lines=lines, edges=edges, pairs=pairs))  # noqa: E731
    add("no_junctions", [], [(1, 1, 5, 5)], [], [(-1, -1)])
    add("no_lines", [(3, 3)], [], [], [])
    add("one_line", two, [(3, 3, 10, 8)], [(0, 1), (1, 0)], [(0, 1)])
    add("self_loop", two, [(3, 3, 4, 3)], [(0, 0)], [(0, 0)])
    add("same_edge_from_two_lines", two, [(3, 3, 10, 8), (10, 9, 3, 4)], [(0, 1), (1, 0)], [(0, 1), (1, 0)])
    add("two_junctions_in_one_pixel", [(5.2, 5.1), (4.6, 4.9), (12, 12)], [(5, 5, 12, 12)], [(1, 2), (2, 1)], [(1, 2)])         # both round to (5, 5)
    add("equal_distance_rows", [(8, 9), (8, 7), (15, 3)], [(8, 8, 15, 3)], [(1, 2), (2, 1)], [(1, 2)])       # row 7 is scanned before row 9
    add("equal_distance_columns", [(9, 8), (7, 8), (15, 3)], [(8, 8, 15, 3)], [(1, 2), (2, 1)], [(1, 2)])    # column 7 before column 9
    add("row_before_column", [(7, 8), (8, 7), (15, 3)], [(8, 8, 15, 3)], [(1, 2), (2, 1)], [(1, 2)])         # (row 7, col 8) before (row 8, col 7)
    add("nearer_wins_over_scan_order", [(6, 6), (8, 9), (15, 3)], [(8, 8, 15, 3)], [(1, 2), (2, 1)], [(1, 2)])                 # d = 4 first, then d = 1
    add("two_cells_away_in_both_axes", [(10, 10), (15, 3)], [(8, 8, 15, 3)], [(0, 1), (1, 0)], [(0, 1)])     # d = 4 still matches
    add("three_cells_away", [(11, 8), (15, 3)], [(8, 8, 15, 3)], [], [(-1, -1)])
    add("second_end_unmatched", two, [(3, 3, 18, 14)], [], [(-1, -1)])
    add("window_clipped_at_every_border", [(0, 0), (19, 0), (0, 15), (19, 15)], [(1, 1, 18, 1), (1, 14, 18, 14), (21, 1, 0, 17)],
        [(0, 1), (1, 0), (1, 2), (2, 1), (2, 3), (3, 2)], [(0, 1), (2, 3), (1, 2)])
    add("junction_at_W_minus_0.4", [(19.6, 5), (3, 3)], [(19, 5, 3, 3)], [], [(-1, -1)])                     # int(20.1) = 20 = W: owns no cell
    add("junction_at_H_minus_0.4", [(5, 15.6), (3, 3)], [(5, 15, 3, 3)], [], [(-1, -1)])
    add("negative_endpoint", [(0, 0), (10, 8)], [(-0.7, -0.7, 10, 8)], [(0, 1), (1, 0)], [(0, 1)])           # int(-0.2) = 0
    add("non_finite_endpoints", two, [(nan, 3, 10, 8), (3, 3, inf, 8), (3, 3, 10, 1e300), (3, -inf, 10, 8), (3, 3, 10, 8)], [(0, 1), (1, 0)],
        [(-1, -1)] * 4 + [(0, 1)])
    return c


X = UINT_MAX


def hand_terms():
    """the term: dict(name, wq, eq, wf, ef, match_num, line_match_num) — counts worked out by hand from map_user.cc:293-327"""
    pair = [(0, 1), (1, 0)]
    t = []
    add = lambda name, wq, eq, wf, ef, mn, lmn: t.append(dict(name=name, wq=wq, eq=eq, wf=wf, ef=ef, match_num=mn, line_match_num=lmn))  # noqa: E731
    add("plain", [5, 7], pair, [5, 7], pair, 2, 2)
    add("invalid_word_in_the_query", [5, X], pair, [5, 7], pair, 1, 0)
    add("invalid_word_in_the_frame", [5, 7], pair, [5, X], pair, 1, 0)
    add("invalid_words_on_both_sides_never_match", [5, X], pair, [5, X], pair, 1, 0)                         # match_num > 0, line_match_num == 0
    add("no_common_word", [1, 2], pair, [3, 4], pair, 0, 0)                                                  # match_num == 0
    add("multiplicities_multiply", [5, 5, 7], [(0, 2), (1, 2), (2, 0), (2, 1)], [5, 5, 5, 7, 7], [(0, 3), (1, 4), (3, 0), (4, 1)], 8, 8)
    add("unconnected_query_junction_does_not_count", [5, 5], [(0, 0)], [5], [(0, 0)], 1, 1)
    add("frame_without_edges", [5, 7], pair, [5, 7, 5], [], 3, 0)
    add("query_without_edges", [5, 7], [], [5, 7], pair, 0, 0)
    add("no_junctions_in_the_query", [], [], [5, 7], pair, 0, 0)
    add("no_junctions_in_the_frame", [5, 7], pair, [], [], 0, 0)
    return t


# ---- generators -------------------------------------------------------------------------------------------------------------------------------------
def grid_case(nj, pairs, W=400, H=400, step=6):
    """nj junctions on a grid `step` pixels apart (no window reaches two of them) and one line per pair (a, b), ends a fraction of a pixel off:
    -> (junc [(x, y)], lines, the distinct directed edges ascending) — the edges follow from the construction, not from the restatement"""
    per = W // step - 1
    assert nj <= per * (H // step - 1)
    junc = [(3 + step * (i % per), 3 + step * (i // per)) for i in range(nj)]
    lines = [(junc[a][0] + 0.3, junc[a][1] - 0.4, junc[b][0] - 0.2, junc[b][1] + 0.3) for a, b in pairs]
    return junc, lines, sorted({(a, b) for a, b in pairs} | {(b, a) for a, b in pairs})


def pairs_for_edges(nj, n_edges):
    """pairs (a, b) whose lines give exactly n_edges distinct directed edges: a != b gives two, a self loop one"""
    out, e = [], 0
    for a in range(nj):
        for b in range(a + 1, nj):
            if e + 2 > n_edges:
                break
            out.append((a, b))
            e += 2
        if e + 2 > n_edges:
            break
    if e < n_edges:
        out.append((0, 0))
        e += 1
    assert e == n_edges, (nj, n_edges, e)
    return out


def pool_nodes(voc, seed, size=30, stopped=3):
    """leaf nodes of the vocabulary to draw junction words from: `stopped` of them with weight 0 (UINT_MAX as a word), the others valid"""
    rng = np.random.default_rng(seed)
    leaves = np.flatnonzero(np.asarray(voc["n_children"]) == 0)
    w = np.asarray(voc["weight"])[leaves]
    good, bad = leaves[w > 0], leaves[w <= 0]
    return np.concatenate([rng.choice(good, size - stopped, replace=False), rng.choice(bad, stopped, replace=False)])


def seeded_frame(rng, voc, pool, nj, nl, W=512, H=512, words=None):
    """one frame: nj junctions (some sharing a pixel, some a neighbour's window), each a leaf of `pool` (its descriptor is the leaf's, so the descent ends
    there); nl lines, most between two junctions with ends up to 1.5 px off, some anywhere.
    -> dict(junc f32 [nj][259], lines f64 [nl][4], node [nj], word [nj] by construction (UINT_MAX where the leaf's weight is 0), weight [nj])"""
    xy = rng.uniform(2, min(W, H) - 3, (nj, 2)).astype(np.float32)
    for i in range(1, nj):
        r = rng.uniform()
        if r < 0.08:
            xy[i] = xy[rng.integers(i)]                                 # the same pixel
        elif r < 0.2:
            xy[i] = xy[rng.integers(i)] + rng.integers(-2, 3, 2)        # inside a neighbour's window
    node = pool[rng.integers(len(pool), size=nj)] if words is None else np.asarray(words)
    junc = np.zeros((nj, 259), np.float32)
    junc[:, 0] = rng.uniform(0.1, 1.0, nj)
    junc[:, 1:3] = xy
    junc[:, 3:] = np.asarray(voc["desc"])[node] if nj else 0
    lines = np.zeros((nl, 4), np.float64)
    for l in range(nl):
        if nj >= 1 and rng.uniform() < 0.85:
            a, b = rng.integers(nj, size=2)
            lines[l] = np.concatenate([xy[a], xy[b]]).astype(np.float64) + rng.uniform(-1.5, 1.5, 4)
        else:
            lines[l] = rng.uniform(-3, max(W, H) + 3, 4)
    wt = np.asarray(voc["weight"])[node] if nj else np.zeros(0)
    wid = np.asarray(voc["word_id"])[node].astype(np.int64) if nj else np.zeros(0, np.int64)
    word = np.where(wt > 0, wid, UINT_MAX).astype(np.uint32)
    return dict(junc=junc, lines=lines, node=node, word=word, weight=wt)


def seeded_table(voc, seed=7, n_frames=12, n_queries=3, sizes=None, W=512, H=512):
    """stored frames and queries over one pool of ~30 words; two frames draw from a second pool (no common word with the queries: match_num == 0) and one
    has junctions but no lines (match_num > 0, line_match_num == 0)"""
    rng = np.random.default_rng(seed)
    pool, other = pool_nodes(voc, seed), pool_nodes(voc, seed + 1000)
    other = np.array([n for n in other if n not in set(pool.tolist())])
    frames = []
    for f in range(n_frames):
        nj = int(rng.integers(20, 60)) if sizes is None else sizes[f]
        nl = int(rng.integers(nj, 3 * nj + 1)) if f != 2 else 0
        frames.append(seeded_frame(rng, voc, other if f in (5, 9) else pool, nj, nl, W, H))
    queries = [seeded_frame(rng, voc, pool, int(rng.integers(20, 60)), int(rng.integers(40, 120)), W, H) for _ in range(n_queries)]
    return frames, queries


def reference_table(frames, queries, W, H, literal=False):
    """the whole term through the restatement: -> (match_num, line_match_num int [Q][N], extra f64 [Q][N], score f64 [Q][N])"""
    def side(fr):
        conn, _ = find_junction_connections(fr["lines"].tolist(), fr["junc"][:, 1:3], W, H)
        return conn, br.frame_to_bow(fr["word"], fr["weight"])
    fs, qs = [side(f) for f in frames], [side(q) for q in queries]
    Q, N = len(queries), len(frames)
    mn, lmn, ex, sc = np.zeros((Q, N), np.int32), np.zeros((Q, N), np.int32), np.zeros((Q, N)), np.zeros((Q, N))
    for q in range(Q):
        for f in range(N):
            mn[q, f], lmn[q, f] = term(queries[q]["word"], qs[q][0], frames[f]["word"], fs[f][0], literal)
            sc[q, f] = br.score(fs[f][1], qs[q][1])                     # Score(_frame_bow_vectors[kf], junction_bow_vector): the frame's vector first
            ex[q, f] = extra(sc[q, f], mn[q, f], lmn[q, f])
    return mn, lmn, ex, sc
