"""TEST INFRASTRUCTURE: a restatement, with dicts and Python floats (IEEE doubles), of the reference's BoW keyframe database and of what its two callers do
with it, up to the candidate list and the best-candidate rule.  Written from the reference's behaviour in this project's own words; include/airfe.h
("BoW keyframe database") states the same contract for the device.  Every sum is sequential in the order the reference's std::map iteration gives."""
import bisect

import numpy as np

UINT_MAX = 0xFFFFFFFF


def frame_to_bow(words, weights):
    """Database::FrameToBow after the per-feature transform (src/bow/database.cc:65-89): BowVector::addWeight for every feature whose weight is > 0, in feature
    order (3rdparty/DBoW2/src/BowVector.cpp: the first weight of a word inserts, later ones add), then BowVector::normalize(L1): the sum of |v| in ascending
    word id, every v divided by it.  -> (ids uint32 [nw] ascending, values float64 [nw])."""
    bow = {}
    for wid, w in zip(words, weights):
        w = float(w)
        if w > 0:
            wid = int(wid)
            if wid in bow:
                bow[wid] += w
            else:
                bow[wid] = w
    ids = sorted(bow)
    tot = 0.0
    for k in ids:
        tot += abs(bow[k])
    vals = [bow[k] / tot for k in ids] if tot > 0.0 else [bow[k] for k in ids]
    return np.array(ids, np.uint32), np.array(vals, np.float64)


def score(v1, v2):
    """L1Scoring::score(v1, v2) (3rdparty/DBoW2/src/ScoringObject.cpp:23-68) on two vectors given as (ids ascending, values): a merge over both, the lagging
    side jumping with lower_bound; per common word s += fabs(vi - wi) - fabs(vi) - fabs(wi) (left to right); -s / 2.0."""
    i1, x1 = v1
    i2, x2 = v2
    a = b = 0
    s = 0.0
    while a < len(i1) and b < len(i2):
        if i1[a] == i2[b]:
            vi, wi = float(x1[a]), float(x2[b])
            s += abs(vi - wi) - abs(vi) - abs(wi)
            a += 1
            b += 1
        elif i1[a] < i2[b]:
            a = bisect.bisect_left(i1, i2[b], a)
        else:
            b = bisect.bisect_left(i2, i1[a], b)
    return -s / 2.0


def score_common(d1, d2):
    """the same value from two word -> value dicts: the merge visits exactly the common words, in ascending word id (test_bowdb_cpu.py checks the two forms
    against each other); used where thousands of frames are scored"""
    s = 0.0
    for w in sorted(d1.keys() & d2.keys()):
        vi, wi = d1[w], d2[w]
        s += abs(vi - wi) - abs(vi) - abs(wi)
    return -s / 2.0


def sharing_threshold(max_sharing, ratio, min_words=8):
    """map_user.cc:146 / map_refiner.cc:108: std::max(static_cast<int>(max_sharing_words * 0.3f), 8) — an int times a float is a float product"""
    return max(int(np.float32(max_sharing) * np.float32(ratio)), int(min_words))


class Database:
    """Database (src/bow/database.cc:91-124).  A frame is its insertion index (the device's handle); _frame_bow_vectors and the inverted file as there."""

    def __init__(self):
        self.vectors = []              # frame -> (ids list, values list)
        self.dicts = []                # frame -> {word: value}
        self.inverted = {}             # word -> [frames] in insertion order = ascending frame (std::map<FramePtr, ...> is only counted, never ordered on)

    def add_frame(self, ids, vals):
        """AddFrame (:98-106): the vector is kept; every word of the frame lists the frame in the inverted file"""
        f = len(self.vectors)
        ids, vals = [int(i) for i in ids], [float(v) for v in vals]
        self.vectors.append((ids, vals))
        self.dicts.append(dict(zip(ids, vals)))
        for w in ids:
            self.inverted.setdefault(w, []).append(f)
        return f

    def query(self, ids):
        """Query (:108-120): for every word of the query, every frame listed under it gains one: frame -> shared words (frames with none are absent)"""
        sharing = {}
        for w in ids:
            for f in self.inverted.get(int(w), ()):
                sharing[f] = sharing.get(f, 0) + 1
        return sharing

    def candidates(self, ids, vals, ratio, min_words=8, max_index=None, exclude=None, sharing=None):
        """the filtration and the scoring of Relocalization (map_user.cc:135-166: ratio 0.3f) and LoopDetection (map_refiner.cc:97-130: ratio 0.5f, frames
        with an id >= the query's and the covisible frames dropped): -> (max_sharing, thr, [(frame, sharing, score)] in ascending frame = frame_scores)"""
        sharing = self.query(ids) if sharing is None else sharing
        max_sharing = max(sharing.values()) if sharing else 0           # over every frame, before anything is erased
        thr = sharing_threshold(max_sharing, ratio, min_words)
        q = dict(zip((int(i) for i in ids), (float(v) for v in vals)))
        out = []
        for f in sorted(sharing):
            if sharing[f] < thr or (max_index is not None and f >= max_index) or (exclude is not None and f in exclude):
                continue
            out.append((f, sharing[f], score_common(self.dicts[f], q)))      # Score(_frame_bow_vectors[frame], bow_vector): the frame's vector first
        return max_sharing, thr, out


def topk(cands, K):
    """the project's own ranking (no reference counterpart): descending score, ties to the lower frame index (a stable sort of the ascending list), -1 padded"""
    order = sorted(cands, key=lambda c: -c[2])
    top = [c[0] for c in order[:K]]
    return top + [-1] * (K - len(top))


def best_candidate(cands, n_matches):
    """map_user.cc:360-376 / map_refiner.cc:213-230: the candidates in order; one replaces the best only with STRICTLY more matches, from an empty list.
    cands: frame indices (-1: none); n_matches: list lengths -> (slot or -1, frame or -1, length)"""
    best, best_n = -1, 0
    for k, (c, n) in enumerate(zip(cands, n_matches)):
        if c >= 0 and n > best_n:
            best, best_n = k, n
    return best, (cands[best] if best >= 0 else -1), best_n
