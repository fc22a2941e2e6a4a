"""The covisibility build (include/airfe.h "Map-point ids and the covisibility build") as a literal Python loop over dicts: Map::UpdateCovisibilityGraph
(src/map.cc:1385-1418) on the id table.  frame -> its valid rows -> the observers of each row's point."""
import numpy as np


def build(point_id, n, size, max_frames, max_points, max_edges=None):
    """point_id [>= size][cap] ints, n [>= size] stored feature counts -> (row_ptr [max_frames + 1], nbr [E], weight [E], info [4]).
    info = [status, entries needed, valid (frame, row) entries, ids ignored as out of range]; with max_edges given and exceeded: status 1, an empty graph."""
    cap = len(point_id[0]) if len(point_id) else 0
    rows = {}                                                       # frame -> the ids at its valid rows, in row order (duplicates stay)
    observers = {}                                                  # point -> the set of frames that hold it
    valid = ignored = 0
    for f in range(size):
        rows[f] = []
        for i in range(max(0, min(int(n[f]), cap))):
            m = int(point_id[f][i])
            if 0 <= m < max_points:
                rows[f].append(m)
                observers.setdefault(m, set()).add(f)
                valid += 1
            elif m != -1:
                ignored += 1
    row_ptr, nbr, weight = [0], [], []
    for f in range(max_frames):
        w = {}
        for m in rows.get(f, []):                                   # per mappoint of the frame, one increment per observer
            for g in observers[m]:
                w[g] = w.get(g, 0) + 1
        for g in sorted(w):
            nbr.append(g)
            weight.append(w[g])
        row_ptr.append(len(nbr))
    needed = len(nbr)
    if max_edges is not None and needed > max_edges:
        return np.zeros(max_frames + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), [1, needed, valid, ignored]
    return np.array(row_ptr, np.int32), np.array(nbr, np.int32), np.array(weight, np.int32), [0, needed, valid, ignored]


# ---- the hand cases: (name, point_id rows, n, size, max_frames, max_points, expected rows {f: [(g, w), ...]}, expected [valid, ignored]) -------------------
def hand_cases():
    """each with its expected table written out by hand"""
    P = 10
    out = []
    # one frame: the self entry only (3 valid rows)
    out.append(("one_frame", [[4, 7, -1, 2]], [4], 1, 3, P, {0: [(0, 3)]}, [3, 0]))
    # the empty database: nothing, whatever the table holds
    out.append(("empty", [[1, 2, 3, 4]], [4], 0, 2, P, {}, [0, 0]))
    # a frame with n = 0 between two that share point 5: its rows are not ids
    out.append(("n_zero", [[5, 1, -1, -1], [5, 5, 5, 5], [5, 2, -1, -1]], [2, 0, 2], 3, 3, P,
                {0: [(0, 2), (2, 1)], 2: [(0, 1), (2, 2)]}, [4, 0]))
    # a frame whose ids are all -1: an empty row, without a self entry
    out.append(("all_minus_one", [[3, -1, -1], [-1, -1, -1], [3, 6, -1]], [3, 3, 3], 3, 4, P,
                {0: [(0, 1), (2, 1)], 2: [(0, 1), (2, 2)]}, [3, 0]))
    # the duplicate row: frame 0 holds point 8 at two rows, frame 1 once: w[0][1] = 2, w[1][0] = 1, w[0][0] counts both rows (+ point 1)
    out.append(("duplicate_row", [[8, 1, 8, -1], [8, -1, -1, -1]], [4, 4], 2, 2, P,
                {0: [(0, 3), (1, 2)], 1: [(0, 1), (1, 1)]}, [4, 0]))
    # ids 0 and max_points - 1
    out.append(("edge_ids", [[0, 9, -1], [9, -1, 0], [0, -1, -1]], [3, 3, 3], 3, 3, P,
                {0: [(0, 2), (1, 2), (2, 1)], 1: [(0, 2), (1, 2), (2, 1)], 2: [(0, 1), (1, 1), (2, 1)]}, [5, 0]))
    # out-of-range ids: ignored and counted (10 = max_points, -2, a large one); -1 is not counted
    out.append(("out_of_range", [[10, 3, -2, -1], [3, 2 ** 31 - 1, -2 ** 31, 10]], [4, 4], 2, 3, P,
                {0: [(0, 1), (1, 1)], 1: [(0, 1), (1, 1)]}, [2, 5]))
    return out


def expected_csr(rows, max_frames):
    row_ptr, nbr, weight = [0], [], []
    for f in range(max_frames):
        for g, w in rows.get(f, []):
            nbr.append(g)
            weight.append(w)
        row_ptr.append(len(nbr))
    return np.array(row_ptr, np.int32), np.array(nbr, np.int32), np.array(weight, np.int32)


def random_table(frames=48, cap=128, max_points=600, seed=5):
    """a seeded table: tracks over neighbouring frames, revisits, duplicates inside a frame, -1 rows, a few out-of-range ids, hostile rows past n"""
    rng = np.random.default_rng(seed)
    ids = rng.integers(-3, max_points + 3, size=(frames, cap)).astype(np.int32)        # what lies past n[f] is never read
    n = rng.integers(0, cap + 1, size=frames).astype(np.int32)
    n[3], n[7] = 0, cap
    for f in range(frames):
        k = int(n[f])
        near = (rng.integers(0, 40, size=k) + 10 * f) % max_points                     # neighbouring frames share a window of ids
        far = rng.integers(0, max_points, size=k)
        row = np.where(rng.random(k) < 0.8, near, far)
        row[rng.random(k) < 0.15] = -1
        bad = rng.random(k) < 0.02
        row[bad] = rng.choice([-2, max_points, max_points + 7, -2 ** 31, 2 ** 31 - 1], size=int(bad.sum()))
        ids[f, :k] = row
    return ids, n
