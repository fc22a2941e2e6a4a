"""The covisibility build on the CPU (include/airfe.h "Map-point ids and the covisibility build"): the host statement covis_build_host
(airslam_amd/csrc/covis_core.h, compiled here with the host compiler) against the Python restatement (tests/covis_ref.py) and against tables written out
by hand; the overflow rule; the library's new symbols; the new kernels' resource usage."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import covis_ref as cr
from conftest import ROOT

CSRC = os.path.join(ROOT, "airslam_amd", "csrc")
SHIM = r'''
#include "covis_core.h"
extern "C" void core_build(const int32_t* point_id, const int* n, int size, int max_frames, int cap, int max_points, int max_edges, int32_t* row_ptr,
                           int32_t* nbr, int32_t* weight, int32_t* info) {
  covis_build_host(point_id, n, size, max_frames, cap, max_points, max_edges, row_ptr, nbr, weight, info);
}
'''


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    """covis_core.h as this tree has it, compiled for the host"""
    d = tmp_path_factory.mktemp("covis_core")
    src, so = d / "core.cpp", str(d / "libcoviscore.so")
    src.write_text(SHIM)
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-w", "-fPIC", "-shared", "-I" + CSRC, str(src), "-o", so], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(so)
    lib.core_build.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 4
    lib.core_build.restype = None
    return lib


def run_host(lib, point_id, n, size, max_frames, max_points, max_edges):
    ids = np.ascontiguousarray(point_id, np.int32)
    n = np.ascontiguousarray(n, np.int32)
    row_ptr = np.full(max_frames + 1, -7, np.int32)
    nbr, weight = np.full(max(max_edges, 1), -7, np.int32), np.full(max(max_edges, 1), -7, np.int32)
    info = np.full(4, -7, np.int32)
    lib.core_build(ids.ctypes.data, n.ctypes.data, size, max_frames, ids.shape[1], max_points, max_edges, row_ptr.ctypes.data, nbr.ctypes.data,
                   weight.ctypes.data, info.ctypes.data)
    e = int(row_ptr[max_frames])
    return row_ptr, nbr[:e].copy(), weight[:e].copy(), info.tolist(), nbr, weight


def same(got, want):
    return all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(got[:3], want[:3])) and list(got[3]) == list(want[3])


@pytest.mark.parametrize("case", cr.hand_cases(), ids=lambda c: c[0])
def test_hand_cases(core, case):
    name, ids, n, size, max_frames, P, rows, (valid, ignored) = case
    want = cr.expected_csr(rows, max_frames)                        # written out by hand in covis_ref.hand_cases
    E = len(want[1])
    ref = cr.build(ids, n, size, max_frames, P)
    assert same(ref, want + ([0, E, valid, ignored],)), (name, ref)
    got = run_host(core, ids, n, size, max_frames, P, max(E, 1))
    assert same(got, want + ([0, E, valid, ignored],)), (name, got[:4])
    for f in range(max_frames):                                     # every row strictly ascending: what airfe_bowdb_set_covisibility asks of a table
        r = got[1][got[0][f]:got[0][f + 1]]
        assert (np.diff(r) > 0).all()


def test_duplicate_row_is_not_symmetric():
    _, ids, n, size, max_frames, P, _, _ = [c for c in cr.hand_cases() if c[0] == "duplicate_row"][0]
    row_ptr, nbr, weight, _ = cr.build(ids, n, size, max_frames, P)
    w = {(f, int(nbr[e])): int(weight[e]) for f in range(size) for e in range(row_ptr[f], row_ptr[f + 1])}
    assert w[(0, 1)] == 2 and w[(1, 0)] == 1 and w[(0, 0)] == 3


def test_seeded_table(core):
    ids, n = cr.random_table()
    frames, P = ids.shape[0], 600
    for size, max_frames in ((frames, frames), (frames - 5, frames), (1, frames)):
        want = cr.build(ids, n, size, max_frames, P)
        E = want[3][1]
        got = run_host(core, ids, n, size, max_frames, P, E)
        assert same(got, want), (size, got[3], want[3])
        if size == frames:
            assert E > 400 and want[3][3] > 5 and want[3][2] > 1000 and int(want[2].max()) > 10      # a busy table: the cases mean something
            assert any(want[0][f] == want[0][f + 1] for f in range(size))                          # ... with an empty row (n = 0)
    # hostile rows past n[f] and frames past size change nothing
    want = cr.build(ids, n, frames - 5, frames, P)
    noisy = ids.copy()
    for f in range(frames):
        noisy[f, n[f]:] = [2 ** 31 - 1, -2 ** 31, 5, 599][f % 4]
    noisy[frames - 5:] = 7
    assert same(run_host(core, noisy, n, frames - 5, frames, P, want[3][1]), want)


def test_overflow_empties_the_graph(core):
    ids, n = cr.random_table()
    frames, P = ids.shape[0], 600
    want = cr.build(ids, n, frames, frames, P)
    E = want[3][1]
    got = run_host(core, ids, n, frames, frames, P, E - 1)
    ref = cr.build(ids, n, frames, frames, P, max_edges=E - 1)
    assert got[3] == ref[3] == [1, E] + want[3][2:] and not got[0].any() and not ref[0].any()
    assert (got[4] == -7).all() and (got[5] == -7).all()            # nothing was written past the decision


# ---- the library and its kernels ----------------------------------------------------------------------------------------------------------------------
NEW = ("airfe_bowdb_attach_point_ids", "airfe_bowdb_set_point_ids", "airfe_bowdb_set_point_ids_dev", "airfe_bowdb_get_point_ids",
       "airfe_bowdb_build_covisibility_dev", "airfe_bowdb_build_covisibility")


def test_library_exports_the_new_entries(libpath):
    lib = C.CDLL(libpath)
    from airslam_amd import _lib, api, build
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    for name in ("attach_point_ids", "set_point_ids", "set_point_ids_dev", "get_point_ids", "build_covisibility_dev", "build_covisibility"):
        assert callable(getattr(api.BowDatabase, name)), name
    assert "kernels_covis.hip" in build.SOURCES and "kernels_covis.hip" not in build.EXTRA_FLAGS      # no floating point: no extra flag


def test_new_kernels_use_no_scratch_and_do_not_spill():
    from airslam_amd import build
    src = "kernels_covis.hip"
    r = subprocess.run(["/opt/rocm/bin/hipcc"] + build.FLAGS + build.EXTRA_FLAGS.get(src, []) + ["-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        os.path.join(CSRC, src), "-o", os.devnull], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    sspill = [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", r.stderr)]
    vspill = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", r.stderr)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert sum("covis_" in n for n in names) == 8 and len(scratch) == len(sspill) == len(vspill) == len(lds) == len(names), names
    assert not any(scratch) and not any(sspill) and not any(vspill), list(zip(names, scratch, sspill, vspill))
    assert max(lds) <= 16384 + 64                                   # the histogram of 4096 int32 and the scan's four sums
    assert "-mwavefrontsize32" not in " ".join(build.FLAGS)         # gfx950's default: wave64
