"""Batched loop detection on the CPU (include/airfe.h "Stored queries against their predecessors", "Loop detection composite"): the host core
(airslam_amd/csrc/loopdet_core.h, compiled here with the host compiler, no FMA contraction) against the Python restatement (tests/loopdet_ref.py) bit for
bit — the odometry prefix, the prefix selection, the constraint rule, every stage, the relative pose; the restatement's two forms (the database grown one
frame at a time, and the prefix rule on the full database) against each other; a hand-built case in which the prefix rule and the existing filter with
max_index = fq on the full database give different candidates; the library's new symbols; the new kernels' resource usage."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bowdb_ref as br
import bowgroup_cases as bc
import loopdet_ref as lr
from conftest import ROOT

CSRC = os.path.join(ROOT, "airslam_amd", "csrc")
SHIM = r'''
#include "loopdet_core.h"
extern "C" {
void core_odometry(const double* pos, int n, double* odom) { loopdet_odometry_host(pos, n, odom); }
int core_threshold(int ms, float ratio, int min_words) { return ld_threshold(ms, ratio, min_words); }
void core_select(const uint32_t* ids, const double* vals, const int* nw, int size, int cap, int fq, float ratio, int min_words, const int32_t* row_ptr,
                 const int32_t* nbr, int rows, int32_t* cf, int32_t* cs, double* sc, int ccap, int* ncand, int* max_sharing, int32_t* dense) {
  loopdet_select_host(ids, vals, nw, size, cap, fq, ratio, min_words, row_ptr, nbr, rows, cf, cs, sc, ccap, ncand, max_sharing, dense);
}
int core_constraints(const int32_t* idx, int m, const double* xyz_b, const float* feat_q, const double* u_right_q, int cap, double* X, double* obs, int* map) {
  return loopdet_constraints_host(idx, m, xyz_b, feat_q, u_right_q, cap, X, obs, map);
}
int core_stage_before(int ncand, int gstatus, int ngroups, int best, int size, int nmatch, int min_matches) {
  return ld_stage_before(ncand, gstatus, ngroups, best, size, nmatch, min_matches);
}
int core_stage(int before, int ncons, int min_points, int num, int min_inliers) { return ld_stage(before, ncons, min_points, num, min_inliers); }
void core_relative_pose(const double* Twl, const double* Twq, double* Rlq, double* tlq) { ld_relative_pose(Twl, Twq, Rlq, tlq); }
void core_no_relative_pose(double* Rlq, double* tlq) { ld_no_relative_pose(Rlq, tlq); }
}
'''


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    """loopdet_core.h as this tree has it, compiled for the host without FMA contraction"""
    d = tmp_path_factory.mktemp("loopdet_core")
    src, so = d / "core.cpp", str(d / "libloopdetcore.so")
    src.write_text(SHIM)
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-w", "-fPIC", "-ffp-contract=off", "-shared", "-I" + CSRC, str(src), "-o", so],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(so)
    lib.core_threshold.argtypes = [C.c_int, C.c_float, C.c_int]
    lib.core_select.argtypes = [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 3
    lib.core_constraints.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 3
    lib.core_odometry.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.core_relative_pose.argtypes = [C.c_void_p] * 4
    lib.core_no_relative_pose.argtypes = [C.c_void_p] * 2
    return lib


# ---- vectors ------------------------------------------------------------------------------------------------------------------------------------------
def vector(words, rng):
    """a BoW vector over the given words: positive weights, L1-normalised the way frame_to_bow does"""
    return br.frame_to_bow(sorted(int(w) for w in words), rng.uniform(0.1, 1.0, len(words)))


def hand_vectors():
    """30 frames.  Background: 20-40 words of 0 .. 999 each (two frames share a handful: below the floor of 8).  Planted on top:
      frame 25 = words 2000 .. 2039; frame 3 holds 30 of them (the prefix's max_sharing: thr = 15), frame 5 exactly 15 (== thr), frame 7 exactly 14
        (thr - 1), frame 9 holds 20, frame 27 (LATER than 25) all 40.
      frame 12 = words 3000 .. 3029 and frame 20 its exact duplicate, stored LATER; frames 2 and 6 hold 16 and 20 of them, frame 10 holds 10.
      frame 16 = words 4000 .. 4019; frames 13, 14, 15 hold 12, 14, 16 of them."""
    rng = np.random.default_rng(7)
    N = 30
    words = [set(int(w) for w in rng.choice(1000, size=int(rng.integers(20, 41)), replace=False)) for _ in range(N)]
    a, b, c = list(range(2000, 2040)), list(range(3000, 3030)), list(range(4000, 4020))
    words[25] = set(a)
    for f, k in ((3, 30), (5, 15), (7, 14), (9, 20), (27, 40)):
        words[f] |= set(a[:k])
    words[12] = set(b)
    for f, k in ((2, 16), (6, 20), (10, 10)):
        words[f] |= set(b[-k:])
    words[16] = set(c)
    for f, k in ((13, 12), (14, 14), (15, 16)):
        words[f] |= set(c[:k])
    vecs = [vector(w, rng) for w in words]
    vecs[20] = (vecs[12][0].copy(), vecs[12][1].copy())
    return vecs


def hand_covisibility():
    """row 25: neighbours 9 (weight 3: any weight excludes), 26 and 28 (>= fq: ignored).  Row 16: 13, 14, 15 — every candidate of frame 16.  Row 12: its
    own entry and 20."""
    return bc.csr(30, {25: [(9, 3), (25, 40), (26, 20), (28, 1)], 16: [(13, 11), (14, 1), (15, 50), (16, 30)], 12: [(12, 30), (20, 30)]})


def seeded_vectors(N, seed):
    """N frames of 30-60 words out of 150: every pair shares a dozen words, so thresholds and candidate lists are busy"""
    rng = np.random.default_rng(seed)
    return [vector(rng.choice(150, size=int(rng.integers(30, 61)), replace=False), rng) for _ in range(N)]


def pack(vecs):
    cap = max(len(i) for i, _ in vecs) + 3
    ids, vals, nw = np.full((len(vecs), cap), 0xFFFFFFFF, np.uint32), np.full((len(vecs), cap), np.nan), np.zeros(len(vecs), np.int32)
    for f, (i, v) in enumerate(vecs):
        ids[f, :len(i)], vals[f, :len(i)], nw[f] = i, v, len(i)
    return ids, vals, nw, cap


def run_select(lib, packed, fq, ratio, csr=None, ccap=None):
    ids, vals, nw, cap = packed
    N = len(nw)
    ccap = N if ccap is None else ccap
    cf, cs, sc = np.full(ccap, -7, np.int32), np.full(ccap, -7, np.int32), np.full(ccap, np.nan)
    nc, ms, dense = C.c_int(-9), C.c_int(-9), np.full(N, -5, np.int32)
    rp = nb = None
    if csr is not None:
        rp, nb = np.ascontiguousarray(csr[0], np.int32), np.concatenate([csr[1], [0]]).astype(np.int32)
    lib.core_select(ids.ctypes.data, vals.ctypes.data, nw.ctypes.data, N, cap, fq, ratio, 8, None if rp is None else rp.ctypes.data,
                    None if nb is None else nb.ctypes.data, 0 if rp is None else len(rp) - 1, cf.ctypes.data, cs.ctypes.data, sc.ctypes.data, ccap,
                    C.byref(nc), C.byref(ms), dense.ctypes.data)
    k = min(nc.value, ccap)
    return dict(max_sharing=ms.value, ncand=nc.value, cands=list(zip(cf[:k].tolist(), cs[:k].tolist(), sc[:k].tolist())), dense=dense.tolist())


def same_selection(got, want, ccap=None):
    k = len(want["cands"]) if ccap is None else min(len(want["cands"]), ccap)
    return (got["max_sharing"] == want["max_sharing"] and got["ncand"] == len(want["cands"]) and got["dense"] == want["dense"] and
            [c[:2] for c in got["cands"]] == [c[:2] for c in want["cands"][:k]] and
            np.array([c[2] for c in got["cands"]]).tobytes() == np.array([c[2] for c in want["cands"][:k]]).tobytes())


# ---- the odometry prefix ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 70])
def test_odometry_prefix(core, N):
    rng = np.random.default_rng(N)
    pos = np.cumsum(rng.normal(size=(N, 3)) * (0.3, 0.3, 0.05), axis=0) + (10.0, -4.0, 1.5)
    if N > 40:
        pos[31] = pos[30]                                           # two coincident frames: a step of exactly 0
    got = np.full(N, np.nan)
    core.core_odometry(np.ascontiguousarray(pos).ctypes.data, N, got.ctypes.data)
    want = lr.odometry(pos)
    assert got.tobytes() == np.array(want).tobytes()
    assert want[0] == 0.0 and all(b >= a for a, b in zip(want, want[1:]))
    if N > 40:
        assert want[31] == want[30] and want[32] > want[31]


# ---- the prefix selection -----------------------------------------------------------------------------------------------------------------------------
def test_threshold_is_a_float_product(core):
    for ms in list(range(0, 70)) + [1023, 1024]:
        for ratio in (0.5, 0.3):
            assert core.core_threshold(ms, ratio, 8) == br.sharing_threshold(ms, ratio, 8), (ms, ratio)


def test_prefix_selection_on_hand_made_vectors(core):
    vecs, csr = hand_vectors(), hand_covisibility()
    packed = pack(vecs)
    covis = lr.covisible_sets(csr[0], csr[1], 30)
    for excl in (None, covis):
        qframes = list(range(-2, 33))
        want = lr.stored_queries(vecs, qframes, 0.5, 8, excl)
        for fq, w in zip(qframes, want):
            got = run_select(core, packed, fq, 0.5, None if excl is None else csr)
            assert same_selection(got, w), (fq, excl is not None, got, w)
    plain = dict(zip(range(30), lr.stored_queries(vecs, range(30), 0.5, 8, None)))
    ex = dict(zip(range(30), lr.stored_queries(vecs, range(30), 0.5, 8, covis)))
    # frame 25: the prefix's max_sharing is frame 3's 30 (frame 27 holds all 40 words but is stored LATER): thr = 15; sharing == thr stays, thr - 1 goes
    assert plain[25]["max_sharing"] == 30 and plain[25]["thr"] == 15 and plain[25]["dense"][27] == 0
    assert plain[25]["dense"][5] == 15 and plain[25]["dense"][7] == 14 and [f for f, _, _ in plain[25]["cands"]] == [3, 5, 9]
    assert plain[27]["max_sharing"] == 40 and [f for f, _, _ in plain[27]["cands"]] == [3, 9, 25]
    # frame 0: no predecessor
    assert plain[0]["cands"] == [] and plain[0]["max_sharing"] == 0 and not any(plain[0]["dense"])
    # a covisibility row with neighbours >= fq and one at weight 3: only the predecessor 9 is dropped, at any weight
    assert [f for f, _, _ in ex[25]["cands"]] == [f for f, _, _ in plain[25]["cands"] if f != 9] and ex[25]["max_sharing"] == plain[25]["max_sharing"]
    # every candidate excluded
    assert [f for f, _, _ in plain[16]["cands"]] == [13, 14, 15] and ex[16]["cands"] == [] and ex[16]["max_sharing"] == 16
    # a frame whose exact duplicate is stored later than it: the duplicate does not exist for it
    assert plain[12]["max_sharing"] == 20 and [f for f, _, _ in plain[12]["cands"]] == [2, 6, 10] and plain[12]["dense"][20] == 0
    assert plain[20]["max_sharing"] == 30 and [f for f, _, _ in plain[20]["cands"]] == [2, 6, 12]
    # ccap below the count: the full count is reported, the first ccap entries written
    got = run_select(core, packed, 12, 0.5, None, ccap=2)
    assert got["ncand"] == 3 and same_selection(got, plain[12], ccap=2)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_prefix_rule_equals_the_incremental_database(core, seed):
    """40 seeded frames: the prefix rule on the FULL database gives, frame for frame, the candidates of bowdb_ref.Database grown one frame at a time —
    and the host core gives the same bytes"""
    N = 40
    vecs = seeded_vectors(N, 100 + seed)
    rng = np.random.default_rng(seed)
    rows = {f: sorted((int(g), int(rng.integers(1, 40))) for g in rng.choice(N, size=6, replace=False)) for f in range(N)}
    csr = bc.csr(N, rows)
    covis = lr.covisible_sets(csr[0], csr[1], N)
    packed = pack(vecs)
    busy = 0
    for excl in (None, covis):
        inc = lr.stored_queries(vecs, range(N), 0.5, 8, excl)
        for fq in range(N):
            full = lr.prefix_rule(vecs, fq, 0.5, 8, excl)
            assert full["max_sharing"] == inc[fq]["max_sharing"] and full["thr"] == inc[fq]["thr"] and full["dense"] == inc[fq]["dense"], fq
            assert full["cands"] == inc[fq]["cands"], fq
            assert same_selection(run_select(core, packed, fq, 0.5, None if excl is None else csr), inc[fq]), fq
            busy += len(inc[fq]["cands"]) > 3
    assert busy >= 40


def test_prefix_rule_differs_from_max_index_on_the_full_database():
    """Why the new entry exists.  Frame 12 of the hand-made vectors (30 words) has predecessors sharing 16, 20 and 10 words, and an exact duplicate stored
    LATER (frame 20).  The reference queried it when only frames 0 .. 11 were stored: max_sharing 20, thr 10, candidates 2, 6, 10.  The existing filter
    with max_index = 12 on the FULL database takes max_sharing over every stored frame — frame 12 itself and frame 20 share all 30 words — so thr is 15 and
    frame 10 is lost."""
    vecs = hand_vectors()
    full = br.Database()
    for ids, vals in vecs:
        full.add_frame(ids, vals)
    ms, thr, cands = full.candidates(vecs[12][0], vecs[12][1], 0.5, 8, max_index=12)
    want = lr.stored_queries(vecs, [12], 0.5, 8, None)[0]
    assert (ms, thr, [f for f, _, _ in cands]) == (30, 15, [2, 6])
    assert (want["max_sharing"], want["thr"], [f for f, _, _ in want["cands"]]) == (20, 10, [2, 6, 10])
    assert lr.prefix_rule(vecs, 12, 0.5, 8, None)["cands"] == want["cands"]


# ---- the constraint rule, the stages, the relative pose ----------------------------------------------------------------------------------------------
def test_constraint_rule(core):
    cap, m = 12, 9
    rng = np.random.default_rng(3)
    xyz = rng.normal(size=(cap, 3))
    xyz[2] = np.nan                                                 # no map point at candidate row 2
    xyz[5, 0] = np.nan                                              # x alone decides
    xyz[6, 1] = np.nan                                              # a NaN elsewhere does not: the constraint is made
    feat = rng.uniform(0, 400, (cap, 259)).astype(np.float32)
    u = np.full(cap, -1.0)
    u[1], u[3], u[4], u[7] = 0.0, 123.25, 1e-300, -1.0              # 0.0 is NOT stereo (> 0 is); the smallest positive value is
    idx = np.array([(0, 1), (1, 3), (2, 2), (3, 4), (4, 0), (5, 5), (3, 4), (7, 6), (1, 1)], np.int32)      # (3, 4) repeats: not deduplicated
    X, obs, mp = np.full((m, 3), 7.0), np.full((m, 3), 7.0), np.full(m, -9, np.int32)
    n = core.core_constraints(idx.ctypes.data, m, xyz.ctypes.data, feat.ctypes.data, u.ctypes.data, cap, X.ctypes.data, obs.ctypes.data, mp.ctypes.data)
    wX, wobs, wmap = lr.constraints(idx, xyz, feat, u)
    assert n == len(wmap) == 7 and mp[:n].tolist() == wmap == [0, 1, 3, 4, 6, 7, 8]
    assert X[:n].tobytes() == wX.tobytes() and obs[:n].tobytes() == wobs.tobytes()
    assert obs[:n, 2].tolist() == [-1.0, -1.0, 123.25, 1e-300, 123.25, -1.0, -1.0]
    assert obs[1, 0] == float(feat[1, 1]) and obs[1, 1] == float(feat[1, 2])


def test_every_stage(core):
    seen = set()
    for ncand in (0, 3):
        for gstatus in (0, 1, 2):
            for ngroups in (0, 2):
                for best in (-1, 4, 12):
                    for nmatch in (0, 50, 51):
                        b = core.core_stage_before(ncand, gstatus, ngroups, best, 12, nmatch, 50)
                        assert b == lr.stage_before(ncand, gstatus, ngroups, best, 12, nmatch, 50)
                        for ncons in (49, 50):
                            for num in (49, 50):
                                s = core.core_stage(b, ncons, 50, num, 50)
                                assert s == lr.stage(b, ncons, num, 50, 50)
                                seen.add(s)
    assert seen == {0, 1, 2, 3, 4, 5}
    assert lr.stage_before(3, 0, 2, 4, 12, 50, 50) == 3 and lr.stage_before(3, 0, 2, 4, 12, 51, 50) == 0       # :232 is a strict >
    assert lr.stage(0, 49, 99, 50, 50) == 4 and lr.stage(0, 50, 49, 50, 50) == 5 and lr.stage(0, 50, 50, 50, 50) == 0


def _pose(rng):
    import pnp_ref as pr
    R, t = pr.planted_motion(rng, max_deg=60.0, max_t=5.0)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T.reshape(16)


def test_relative_pose(core):
    rng = np.random.default_rng(20)
    for _ in range(20):
        Twl, Twq = _pose(rng), _pose(rng)
        R, t = np.full(9, np.nan), np.full(3, np.nan)
        core.core_relative_pose(Twl.ctypes.data, Twq.ctypes.data, R.ctypes.data, t.ctypes.data)
        wR, wt = lr.relative_pose(Twl, Twq)
        assert R.tobytes() == np.array(wR).tobytes() and t.tobytes() == np.array(wt).tobytes()
        L, Q = Twl.reshape(4, 4), Twq.reshape(4, 4)
        np.testing.assert_allclose(R.reshape(3, 3), L[:3, :3].T @ Q[:3, :3], atol=1e-14)
        np.testing.assert_allclose(t, L[:3, :3].T @ (Q[:3, 3] - L[:3, 3]), atol=1e-13)
    core.core_no_relative_pose(R.ctypes.data, t.ctypes.data)
    assert R.tolist() == lr.IDENTITY9 and t.tolist() == [0.0] * 3


# ---- the library and its kernels ----------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_new_entries(libpath):
    lib = C.CDLL(libpath)
    for name in ("airfe_bowdb_set_poses", "airfe_bowdb_get_poses", "airfe_bowdb_set_u_right", "airfe_bowdb_set_u_right_dev", "airfe_bowdb_get_u_right",
                 "airfe_bowdb_query_stored_batch_dev", "airfe_loop_detect_batch_dev"):
        assert hasattr(lib, name), name
    from airslam_amd import _lib, build
    assert C.sizeof(_lib.LoopCfg) == 96                             # 4 x 4, the double, 3 x 4 + padding, 7 doubles
    assert "kernels_loopdet.hip" in build.SOURCES and "-ffp-contract=off" in build.EXTRA_FLAGS["kernels_loopdet.hip"]


def test_new_kernels_use_no_scratch_and_full_waves():
    from airslam_amd import build
    src = "kernels_loopdet.hip"
    r = subprocess.run(["/opt/rocm/bin/hipcc"] + build.FLAGS + build.EXTRA_FLAGS[src] + ["-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        os.path.join(CSRC, src), "-o", os.devnull], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert sum("loopdet_" in n for n in names) == 7 and len(scratch) == len(names), names
    assert not any(scratch), list(zip(names, scratch))
    assert "-mwavefrontsize32" not in " ".join(build.FLAGS + build.EXTRA_FLAGS[src])       # gfx950's default: wave64
