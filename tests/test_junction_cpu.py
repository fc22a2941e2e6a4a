"""Relocalisation's junction term on the CPU (include/airfe.h "Junction term"): the host statements of airslam_amd/csrc/junction_core.h, compiled here with
the host compiler, against the literal restatement of the reference (tests/junction_ref.py) and against edges and counts written out by hand — exactly:
edges, per-line pairs, counts, and `extra` bit for bit.  The library's new symbols; the new kernels' resource usage."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bowdb_ref as br
import junction_ref as jr
from airslam_amd import weights
from conftest import ROOT

CSRC = os.path.join(ROOT, "airslam_amd", "csrc")
SHIM = r'''
#include "junction_core.h"
extern "C" int core_connections(const double* lines, int nl, const float* junc, int nj, int W, int H, int32_t* edge, int ecap, int* nedge, int32_t* line_pair) {
  return jn_connections_host(lines, nl, junc, nj, W, H, edge, ecap, nedge, line_pair);
}
extern "C" void core_keys(const uint32_t* word, int nj, const int32_t* edge, int ne, uint32_t* uword, int32_t* wcnt, int32_t* wconn, int* nuw,
                          unsigned long long* ukey, int32_t* kcnt, int* nuk) {
  jn_keys_host(word, nj, edge, ne, uword, wcnt, wconn, nuw, ukey, kcnt, nuk);
}
extern "C" double core_term(const uint32_t* q_uword, const int32_t* q_wconn, int q_nuw, const unsigned long long* q_ukey, const int32_t* q_kcnt, int q_nuk,
                            const uint32_t* f_uword, const int32_t* f_wcnt, int f_nuw, const unsigned long long* f_ukey, const int32_t* f_kcnt, int f_nuk,
                            double score, int* match_num, int* line_match_num) {
  jn_term_host(q_uword, q_wconn, q_nuw, q_ukey, q_kcnt, q_nuk, f_uword, f_wcnt, f_nuw, f_ukey, f_kcnt, f_nuk, match_num, line_match_num);
  return jn_extra(score, *match_num, *line_match_num);
}
'''
W, H = 512, 512


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    """junction_core.h as this tree has it, compiled for the host without contraction (as the kernel file is)"""
    d = tmp_path_factory.mktemp("junction_core")
    src, so = d / "core.cpp", str(d / "libjunctioncore.so")
    src.write_text(SHIM)
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-w", "-fPIC", "-shared", "-ffp-contract=off", "-I" + CSRC, str(src), "-o", so], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(so)
    lib.core_connections.restype = C.c_int
    lib.core_keys.restype = None
    lib.core_term.restype = C.c_double
    lib.core_term.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                              C.c_double, C.c_void_p, C.c_void_p]
    return lib


def rows(junc_xy):
    j = np.zeros((len(junc_xy), 259), np.float32)
    if len(junc_xy):
        j[:, 1:3] = np.asarray(junc_xy, np.float32)
    return j


def connections(lib, lines, junc, w, h, ecap=4096):
    """-> (edges [(a, b)], pairs [(a, b)], status); the buffers are checked for writes past what the core reports"""
    ln = np.ascontiguousarray(lines, np.float64).reshape(-1, 4)
    jn = np.ascontiguousarray(junc, np.float32).reshape(-1, 259)
    edge = np.full((ecap + 1, 2), -7, np.int32)
    pair = np.full((len(ln) + 1, 2), -7, np.int32)
    ne = C.c_int(-7)
    st = lib.core_connections(C.c_void_p(ln.ctypes.data), len(ln), C.c_void_p(jn.ctypes.data), len(jn), w, h, C.c_void_p(edge.ctypes.data), ecap, C.byref(ne),
                              C.c_void_p(pair.ctypes.data))
    assert (edge[ne.value:] == -7).all() and (pair[len(ln):] == -7).all()
    return [tuple(e) for e in edge[:ne.value].tolist()], [tuple(p) for p in pair[:len(ln)].tolist()], st


def keys(lib, word, edges):
    """-> ([(word, cnt, conn)], [(key, multiplicity)]) + the raw arrays for core_term"""
    word = np.ascontiguousarray(word, np.uint32)
    nj, ne = len(word), len(edges)
    e = np.ascontiguousarray(np.asarray(edges, np.int32).reshape(-1, 2))
    uword, wcnt, wconn = np.zeros(nj + 1, np.uint32), np.zeros(nj + 1, np.int32), np.zeros(nj + 1, np.int32)
    ukey, kcnt = np.zeros(ne + 1, np.uint64), np.zeros(ne + 1, np.int32)
    nuw, nuk = C.c_int(0), C.c_int(0)
    lib.core_keys(C.c_void_p(word.ctypes.data), nj, C.c_void_p(e.ctypes.data), ne, C.c_void_p(uword.ctypes.data), C.c_void_p(wcnt.ctypes.data),
                  C.c_void_p(wconn.ctypes.data), C.byref(nuw), C.c_void_p(ukey.ctypes.data), C.c_void_p(kcnt.ctypes.data), C.byref(nuk))
    return dict(uword=uword, wcnt=wcnt, wconn=wconn, nuw=nuw.value, ukey=ukey, kcnt=kcnt, nuk=nuk.value)


def as_lists(t):
    return ([(int(t["uword"][i]), int(t["wcnt"][i]), int(t["wconn"][i])) for i in range(t["nuw"])],
            [(int(t["ukey"][i]), int(t["kcnt"][i])) for i in range(t["nuk"])])


def core_term(lib, tq, tf, score):
    mn, lmn = C.c_int(-7), C.c_int(-7)
    p = lambda a: a.ctypes.data  # noqa: E731
    ex = lib.core_term(p(tq["uword"]), p(tq["wconn"]), tq["nuw"], p(tq["ukey"]), p(tq["kcnt"]), tq["nuk"], p(tf["uword"]), p(tf["wcnt"]), tf["nuw"], p(tf["ukey"]),
                       p(tf["kcnt"]), tf["nuk"], float(score), C.byref(mn), C.byref(lmn))
    return mn.value, lmn.value, ex


@pytest.mark.parametrize("case", jr.hand_cases(), ids=lambda c: c["name"])
def test_hand_connections(core, case):
    conn, pairs = jr.find_junction_connections(case["lines"], case["junc"], case["W"], case["H"])
    assert jr.edges_of(conn) == case["edges"] and pairs == case["pairs"], (jr.edges_of(conn), pairs)      # the restatement against the hand's answer
    got = connections(core, case["lines"], rows(case["junc"]), case["W"], case["H"])
    assert got == (case["edges"], case["pairs"], jr.OK), got


@pytest.mark.parametrize("case", jr.hand_terms(), ids=lambda c: c["name"])
def test_hand_terms(core, case):
    want = (case["match_num"], case["line_match_num"])
    cq, cf = jr.connected_of(case["eq"], len(case["wq"])), jr.connected_of(case["ef"], len(case["wf"]))
    assert jr.term(case["wq"], cq, case["wf"], cf, literal=True) == want and jr.term(case["wq"], cq, case["wf"], cf) == want
    tq, tf = keys(core, case["wq"], case["eq"]), keys(core, case["wf"], case["ef"])
    assert as_lists(tq) == jr.tables(case["wq"], case["eq"]) and as_lists(tf) == jr.tables(case["wf"], case["ef"])
    for score in (0.0, 0.37, 1.0 / 3.0):
        mn, lmn, ex = core_term(core, tq, tf, score)
        assert (mn, lmn) == want
        assert np.float64(ex).tobytes() == np.float64(jr.extra(score, *want)).tobytes()
    if case["name"] == "unconnected_query_junction_does_not_count":
        assert core_term(core, tq, tf, 0.25)[2] == 0.5                  # rate = 1


@pytest.mark.parametrize("n_edges", [1, 64, 65, 4096])
def test_exactly_ecap_edges_and_one_more(core, n_edges):
    nj = 100
    junc, lines, edges = jr.grid_case(nj, jr.pairs_for_edges(nj, n_edges))
    assert len(edges) == n_edges
    conn, _ = jr.find_junction_connections(lines, junc, 400, 400)
    assert jr.edges_of(conn) == edges
    got = connections(core, lines, rows(junc), 400, 400, ecap=n_edges)
    assert got[0] == edges and got[2] == jr.OK
    if n_edges > 1:
        got = connections(core, lines, rows(junc), 400, 400, ecap=n_edges - 1)
        assert got[0] == [] and got[2] == jr.OVERFLOW                   # never a shorter list
        assert got[1] == jr.pairs_for_edges(nj, n_edges)                # the per-line pairs are still the lines' own


def test_more_than_1024_junctions_is_status_2(core):
    junc = rows([(3 + (i % 100) * 5, 3 + (i // 100) * 5) for i in range(1025)])
    assert connections(core, [(3, 3, 8, 3)], junc, 512, 512)[::2] == ([], jr.OVERFLOW)
    assert connections(core, [(3, 3, 8, 3)], junc[:1024], 512, 512)[::2] == ([(0, 1), (1, 0)], jr.OK)


@pytest.fixture(scope="module")
def table():
    voc = weights.synthetic_vocabulary(1234, k=10, L=3)
    frames, queries = jr.seeded_table(voc)
    return frames, queries, jr.reference_table(frames, queries, W, H)


def test_seeded_table_is_busy(table):
    """asserted ON THE REFERENCE'S NUMBERS, so that the comparison below cannot pass on zeros"""
    frames, queries, (mn, lmn, ex, sc) = table
    assert (lmn > 0).mean() >= 0.5, (lmn > 0).mean()
    assert ((mn > 0) & (lmn == 0)).any() and (mn == 0).any()
    assert (sc > 0).any() and any((f["word"] == jr.UINT_MAX).any() for f in frames) and any((q["word"] == jr.UINT_MAX).any() for q in queries)
    lit = jr.reference_table(frames[:4], queries[:1], W, H, literal=True)      # the four loops as Python loops, on a corner of the table
    assert np.array_equal(lit[0], mn[:1, :4]) and np.array_equal(lit[1], lmn[:1, :4]) and lit[2].tobytes() == ex[:1, :4].tobytes()


def test_seeded_table(core, table):
    frames, queries, (mn, lmn, ex, sc) = table
    def side(fr):
        conn, pairs = jr.find_junction_connections(fr["lines"].tolist(), fr["junc"][:, 1:3], W, H)
        edges, got_pairs, st = connections(core, fr["lines"], fr["junc"], W, H)
        assert st == jr.OK and edges == jr.edges_of(conn) and got_pairs == pairs
        t = keys(core, fr["word"], edges)
        assert as_lists(t) == jr.tables(fr["word"], edges)
        return t
    tf, tq = [side(f) for f in frames], [side(q) for q in queries]
    for q in range(len(queries)):
        for f in range(len(frames)):
            got = core_term(core, tq[q], tf[f], sc[q, f])
            assert got[:2] == (mn[q, f], lmn[q, f]), (q, f, got)
            assert np.float64(got[2]).tobytes() == ex[q, f].tobytes(), (q, f, got[2], ex[q, f])
    # hostile rows: NaN and far-away lines, junctions outside the image — none of them changes another line's answer
    fr = frames[0]
    lines = np.concatenate([fr["lines"], [[np.nan] * 4, [1e308, 0, 0, 0], [-1e9, -1e9, 1e9, 1e9]]])
    junc = np.concatenate([fr["junc"], rows([(-5, 3), (3, 1e9), (np.nan, 2)])])
    conn, pairs = jr.find_junction_connections(lines.tolist(), junc[:, 1:3], W, H)
    edges, got_pairs, st = connections(core, lines, junc, W, H)
    assert edges == jr.edges_of(conn) and got_pairs == pairs and pairs[-3:] == [(-1, -1)] * 3
    assert edges == connections(core, fr["lines"], fr["junc"], W, H)[0]


def test_score_is_the_databases(table):
    """reference_table's score is bowdb_ref's L1 score of the two junction vectors, the frame's first (map_user.cc:330)"""
    frames, queries, (_, _, _, sc) = table
    v = lambda fr: br.frame_to_bow(fr["word"], fr["weight"])  # noqa: E731
    assert sc[1, 3] == br.score(v(frames[3]), v(queries[1])) and 0.0 <= sc.min() and sc.max() <= 1.0


# ---- the library and its kernels ----------------------------------------------------------------------------------------------------------------------
NEW = ("airfe_junction_connections_batch_dev", "airfe_junction_connections", "airfe_bowdb_attach_junctions", "airfe_bowdb_set_junctions_dev",
       "airfe_bowdb_set_junctions", "airfe_bowdb_get_junctions", "airfe_bowdb_junction_term_batch_dev", "airfe_bowdb_junction_extra_batch_dev",
       "airfe_bowdb_add_junction_frames_batch_dev")


def test_library_exports_the_new_entries(libpath):
    lib = C.CDLL(libpath)
    from airslam_amd import _lib, api, build
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    for name in ("junction_connections", "junction_connections_batch_dev"):
        assert callable(getattr(api.Context, name)), name
    for name in ("attach_junctions", "set_junctions", "set_junctions_dev", "get_junctions", "junction_term_batch_dev", "junction_extra_batch_dev",
                 "add_junction_frames_batch_dev"):
        assert callable(getattr(api.BowDatabase, name)), name
    assert "kernels_junction.hip" in build.SOURCES and build.EXTRA_FLAGS["kernels_junction.hip"] == ["-ffp-contract=off"]
    with open(os.path.join(ROOT, "include", "airfe.h")) as fh:
        text = fh.read()
    assert "What stays the caller's: relocalisation's junction" not in text and "---- Junction term:" in text


def test_new_kernels_use_no_scratch_and_do_not_spill():
    from airslam_amd import build
    src = "kernels_junction.hip"
    r = subprocess.run(["/opt/rocm/bin/hipcc"] + build.FLAGS + build.EXTRA_FLAGS.get(src, []) + ["-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        os.path.join(CSRC, src), "-o", os.devnull], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    sspill = [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", r.stderr)]
    vspill = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", r.stderr)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert sum("junction_" in n for n in names) == 3 and len(scratch) == len(sspill) == len(vspill) == len(lds) == len(names), names
    assert not any(scratch) and not any(sspill) and not any(vspill), list(zip(names, scratch, sspill, vspill))
    assert max(lds) <= 64 * 1024                                    # the static limit; the term kernel: 1024 x 8 + 4096 x 12 bytes of query tables
    assert "-mwavefrontsize32" not in " ".join(build.FLAGS)         # gfx950's default: wave64
