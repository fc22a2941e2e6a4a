"""BoW keyframe database, no GPU: the restatement (tests/bowdb_ref.py) against DBoW2 compiled unchanged and against an independent form of the L1 score;
hand-built cases of the rules that are easy to get wrong; the library's new symbols; no scratch in the query kernel."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bowdb_ref as br
import ref_cases as rc
from conftest import GOLDEN, ROOT
from oracle import ref_lib, ref_post

CASES = ["k10_L4_400", "k8_L3_1024", "k3_L2_1"]        # (k, L, n) = (10, 4, 400), (8, 3, 1024), (3, 2, 1): tests/ref_cases.py::BOW


def _restated_vector(voc, feat):
    w, wt = ref_post.bow_transform(voc, feat[:, 3:])
    return br.frame_to_bow(w, wt)


@pytest.mark.parametrize("name", CASES)
def test_restated_vector_equals_dbow2_bit_for_bit(name):
    """ids and doubles of the BowVector: the committed outputs of the compiled DBoW2 (tests/golden/ref_pin.npz) and, where the library was built, DBoW2 itself"""
    case = rc.bow_case(name)
    ids, vals = _restated_vector(case["voc"], case["feat"])
    z = np.load(os.path.join(GOLDEN, "ref_pin.npz"))
    np.testing.assert_array_equal(ids, z[f"bow/{name}/bow_ids"])
    assert vals.tobytes() == np.ascontiguousarray(z[f"bow/{name}/bow_values"], np.float64).tobytes()
    if ref_lib.available():
        _, _, rid, rval = ref_lib.bow_frame_to_bow(case["voc"], case["feat"])
        np.testing.assert_array_equal(ids, rid)
        assert vals.tobytes() == rval.tobytes()
    assert len(ids) == len(set(ids.tolist())) and (np.diff(ids.astype(np.int64)) > 0).all()


def test_a_frame_whose_every_word_is_stopped_gives_an_empty_vector():
    case = rc.bow_case("k10_L4_400")
    voc = dict(case["voc"])
    voc["weight"] = np.zeros_like(voc["weight"])
    ids, vals = _restated_vector(voc, case["feat"][:50])
    assert len(ids) == 0 and len(vals) == 0
    if ref_lib.available():
        w, _, rid, _ = ref_lib.bow_frame_to_bow(voc, case["feat"][:50])
        assert len(rid) == 0 and (w == br.UINT_MAX).all()


def _random_vector(rng, n_words, nw):
    ids = np.sort(rng.choice(n_words, size=nw, replace=False)).astype(np.uint32)
    v = rng.random(nw) + 0.05
    tot = 0.0
    for x in v:
        tot += x
    return ids, np.array([x / tot for x in v])


def test_score_against_the_dense_l1_identity():
    """DBoW2's own comment: for L1-normalised vectors score = 1 - 0.5 * ||v1 - v2||_1.  Both sides are sums of <= 2048 doubles of magnitude <= 1, each rounding
    below 2^-53: 2048 * 1.1e-16 = 2.3e-13 < 1e-12 (a derived bound, not a measured one)."""
    rng = np.random.default_rng(7)
    for trial in range(40):
        n_words = int(rng.choice([50, 1000, 10000]))
        a = _random_vector(rng, n_words, int(rng.integers(1, min(n_words, 1024) + 1)))
        b = _random_vector(rng, n_words, int(rng.integers(1, min(n_words, 1024) + 1)))
        da, db = np.zeros(n_words), np.zeros(n_words)
        da[a[0]] = a[1]
        db[b[0]] = b[1]
        want = 1.0 - 0.5 * np.abs(da - db).sum()
        got = br.score((a[0].tolist(), a[1].tolist()), (b[0].tolist(), b[1].tolist()))
        assert abs(got - want) <= 1e-12
        assert got == br.score_common(dict(zip(a[0].tolist(), a[1].tolist())), dict(zip(b[0].tolist(), b[1].tolist())))      # the two forms of the restatement: same bits
        assert abs(br.score((a[0].tolist(), a[1].tolist()), (a[0].tolist(), a[1].tolist())) - 1.0) <= 1e-12


def test_disjoint_vectors_score_minus_zero():
    z = br.score(([1, 3], [0.5, 0.5]), ([2, 4], [0.5, 0.5]))
    assert z == 0.0 and np.signbit(z)                       # -s / 2.0 of s = +0.0
    z = br.score_common({1: 0.5, 3: 0.5}, {2: 1.0})
    assert z == 0.0 and np.signbit(z)


def test_score_depends_on_the_argument_order():
    """(|v1 - v2| - |v1|) - |v2| rounds differently from (|v2 - v1| - |v2|) - |v1| for some pairs: Score(frame, query) is not Score(query, frame)"""
    rng = np.random.default_rng(11)
    differ = 0
    for trial in range(200):
        ids = np.arange(30).tolist()
        a, b = _random_vector(rng, 30, 30)[1].tolist(), _random_vector(rng, 30, 30)[1].tolist()
        s1, s2 = br.score((ids, a), (ids, b)), br.score((ids, b), (ids, a))
        assert abs(s1 - s2) <= 1e-14
        differ += s1 != s2
    assert differ > 0
    # a pinned pair: one term, the two orders one ulp apart
    rng = np.random.default_rng(3)
    found = None
    for _ in range(1000):
        x, y = float(rng.random()) / 300.0, float(rng.random()) / 17.0      # magnitudes of a frame's / a short vector's entries
        if (abs(x - y) - abs(x)) - abs(y) != (abs(y - x) - abs(y)) - abs(x):
            found = (x, y)
            break
    assert found is not None
    x, y = found
    assert br.score(([5], [x]), ([5], [y])) == -((abs(x - y) - abs(x)) - abs(y)) / 2.0
    assert br.score(([5], [x]), ([5], [y])) != br.score(([5], [y]), ([5], [x]))


def test_threshold_is_the_truncated_float32_product():
    for ratio in (0.3, 0.5):
        r32 = np.float32(ratio)
        for m in range(1, 1025):
            thr = br.sharing_threshold(m, ratio)
            assert thr == max(int(np.float32(np.float32(m) * r32)), 8)
            assert thr == max(int(m * float(r32)), 8)            # (the double product truncates to the same integer for every m up to 1024)
    assert [br.sharing_threshold(m, 0.3) for m in (1, 26, 27, 30, 100, 240, 1024)] == [8, 8, 8, 9, 30, 72, 307]
    assert [br.sharing_threshold(m, 0.5) for m in (1, 16, 17, 18, 19, 241, 1024)] == [8, 8, 8, 9, 9, 120, 512]


def _db_of(frames):
    db = br.Database()
    for ids in frames:
        db.add_frame(ids, [1.0 / len(ids)] * len(ids))
    return db


def test_filtration_rules():
    q = list(range(100))
    frames = [list(range(100)), list(range(40)), list(range(29)), list(range(30)), list(range(200, 210)), list(range(7))]
    db = _db_of(frames)
    qv = [0.01] * 100
    sharing = db.query(q)
    assert sharing == {0: 100, 1: 40, 2: 29, 3: 30, 5: 7}           # frame 4 shares nothing: absent
    ms, thr, c = db.candidates(q, qv, 0.3)
    assert (ms, thr) == (100, 30) and [x[0] for x in c] == [0, 1, 3]
    ms, thr, c = db.candidates(q, qv, 0.5)
    assert (ms, thr) == (100, 50) and [x[0] for x in c] == [0]
    # max_sharing is taken before the index / exclusion filters: frame 0 sets thr although it is dropped
    ms, thr, c = db.candidates(q, qv, 0.3, max_index=4, exclude={0})
    assert (ms, thr) == (100, 30) and [x[0] for x in c] == [1, 3]
    ms, thr, c = db.candidates(q, qv, 0.3, max_index=1)
    assert (ms, thr) == (100, 30) and [x[0] for x in c] == [0]
    # the floor of 8 words: without the long frames max_sharing = 7 and nothing survives
    db2 = _db_of([list(range(7)), list(range(3))])
    ms, thr, c = db2.candidates(q, qv, 0.3)
    assert (ms, thr, c) == (7, 8, [])
    db3 = _db_of([list(range(9)), list(range(8)), list(range(7))])
    ms, thr, c = db3.candidates(q, qv, 0.3)
    assert (ms, thr) == (9, 8) and [x[0] for x in c] == [0, 1]
    assert c[0][2] == br.score((frames[0][:9], [1.0 / 9] * 9), (q, qv))        # Score(frame, query)


def test_topk_and_best_candidate_rules():
    cands = [(2, 10, 0.5), (5, 10, 0.7), (7, 10, 0.5), (9, 10, 0.7), (11, 10, 0.1)]
    assert br.topk(cands, 3) == [5, 9, 2] and br.topk(cands, 8) == [5, 9, 2, 7, 11, -1, -1, -1] and br.topk([], 2) == [-1, -1]
    # a capacity overflow keeps the first entries of the ascending list (the device writes ccap of ncand)
    assert [c[0] for c in cands[:2]] == [2, 5]
    assert br.best_candidate([4, 8, 6], [30, 30, 29]) == (0, 4, 30)             # the first of equals
    assert br.best_candidate([4, 8, 6], [30, 31, 31]) == (1, 8, 31)
    assert br.best_candidate([4, -1, 6], [0, 50, 0]) == (-1, -1, 0)             # a hole never wins; nor does a list of 0
    assert br.best_candidate([-1, -1, -1], [0, 0, 0]) == (-1, -1, 0)


def test_loop_closure_pairs_takes_candidates_from_a_ranking():
    from airslam_amd import mapfile
    assert mapfile.loop_closure_pairs(10) == [(q, (q + 1 + 7 * k) % 10 if (q + 1 + 7 * k) % 10 != q else (q + 2 + 7 * k) % 10) for q in range(10) for k in range(5)]
    top = [[2, 0, -1], [1, 3, 2], [-1, -1, -1], [9, 0, 1]]            # rows of BowDatabase.topk_dev: the query itself, holes and foreign indices are skipped
    assert mapfile.loop_closure_pairs(4, 2, candidates=top) == [(0, 2), (1, 3), (1, 2), (3, 0), (3, 1)]


NEW = ["airfe_bow_vector", "airfe_bow_vector_batch_dev", "airfe_bowdb_create", "airfe_bowdb_destroy", "airfe_bowdb_clear", "airfe_bowdb_size", "airfe_bowdb_add",
       "airfe_bowdb_add_batch_dev", "airfe_bowdb_query_batch_dev", "airfe_bowdb_topk_dev", "airfe_bowdb_match_candidates_batch_dev"]


def test_new_entries_are_declared_exported_and_fail_cleanly(libpath):
    from airslam_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "airfe.h")).read()
    src = open(os.path.join(ROOT, "airslam_amd", "csrc", "airfe_bowdb.hip")).read()
    lib = _lib.lib()
    for n in NEW:
        assert re.search(r"\bint " + n + r"\(", hdr), n
        assert hasattr(lib, n) and n in _lib.SIGNATURES
        assert re.search(r"^int " + n + r"\([^;{]*?\)\s*try\s*\{", src, flags=re.M | re.S), f"{n} is not a function-try-block"
    assert "getenv" not in open(os.path.join(ROOT, "airslam_amd", "csrc", "kernels_bowdb.hip")).read()
    # what can be checked without a device: a NULL context / database is an error return, never a crash
    z = np.zeros(16, np.float64)
    p = z.ctypes.data
    nw = C.c_int(5)
    assert lib.airfe_bow_vector(None, p, 1, p, p, C.byref(nw), None) != 0
    assert lib.airfe_bow_vector_batch_dev(None, p, p, 1, 1, p, p, p, None, None) != 0
    h = C.c_void_p()
    assert lib.airfe_bowdb_create(None, 16, 400, 0, C.byref(h)) != 0 and not h.value
    assert lib.airfe_bowdb_size(None) == -1 and lib.airfe_bowdb_clear(None) != 0 and lib.airfe_bowdb_destroy(None) == 0
    assert lib.airfe_bowdb_add(None, p, p, p, None, None, 1, 400) != 0
    assert lib.airfe_bowdb_add_batch_dev(None, p, p, p, None, None, 1, 400, None) != 0
    f = _lib.BowdbFilter(0.3, 8, None, None, 0)
    assert lib.airfe_bowdb_query_batch_dev(None, p, p, p, 1, 400, C.byref(f), p, p, p, 4, p, p, None, None) != 0
    assert lib.airfe_bowdb_topk_dev(None, p, p, p, 1, 4, 3, p, None, None) != 0
    assert lib.airfe_bowdb_match_candidates_batch_dev(None, None, p, p, 1, 400, p, 3, 1, p, p, p, 400, p, None, None) != 0


def test_new_kernels_use_no_scratch():
    from test_no_scratch_cpu import _usage
    u = _usage("kernels_bowdb.hip")
    hot = {k: v for k, v in u.items() if "bowdb_query_kernel" in k or "bow_vector_kernel" in k or "bowdb_select_kernel" in k}
    assert len(hot) >= 4, list(u)
    for k, v in hot.items():
        assert v.get("ScratchSize [bytes/lane]", 0) == 0 and v.get("VGPRs Spill", 0) == 0, (k, v)
