"""The map-point merge on the CPU (include/airfe.h "Map-point merge"): the host statement merge_build_host / merge_pairs_host (airslam_amd/csrc/merge_core.h,
compiled here with the host compiler) against the literal Python restatement (tests/merge_ref.py) byte for byte, on the hand cases and three seeded tables;
results written out by hand; the epipolar gate as a decision with its margin asserted; the library's new symbols; the new kernels' resource usage."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import merge_ref as mr
from conftest import ROOT

CSRC = os.path.join(ROOT, "airslam_amd", "csrc")
HAND = mr.hand_cases()


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    return mr.host_lib(tmp_path_factory.mktemp("merge_core"))


def _margins(case):
    """every computed er is at least 1e-6 (relative) away from 10, so numpy's formulation and merge_core.h's decide alike; -> the finite ers"""
    ers = [x[7] for x in mr.entries(case) if x[7] is not None]
    for er in ers:
        assert np.isnan(er) or abs(er - 10.0) >= 1e-6 * max(abs(er), 10.0), (case["name"], er)
    return ers


@pytest.mark.parametrize("case", HAND, ids=lambda c: c["name"])
def test_hand_cases(core, case):
    if case["loop"] is not None:
        _margins(case)
    want = mr.merge(case)
    got = mr.run_host(core, case)
    assert mr.same(got, want), (case["name"], got[3], want[3], np.argwhere(got[0] != want[0])[:8].tolist())
    assert (got[2] != np.arange(case["P"])).sum() == got[3][5]      # every member of a group but its best maps elsewhere: the ids removed
    # rows past n[f] and frames past size are as they were
    for f in range(mr.F_):
        k = min(max(int(case["n"][f]), 0), mr.CAP) if f < case["size"] else 0
        assert np.array_equal(got[0][f, k:], case["ids"][f, k:]) and got[1][f, k:].tobytes() == case["xyz"][f, k:].tobytes()


def _by_name(name):
    return [c for c in HAND if c["name"] == name][0]


def test_results_written_out_by_hand(core):
    """what a reader of the statement expects, not what either implementation gives"""
    for run in (mr.merge, lambda c: mr.run_host(core, c)):
        ids, xyz, mp, info = run(_by_name("one_pair"))
        assert info == [1, 0, 0, 0, 1, 1, 1, 0] and mp[11] == 10 and mp[10] == 10 and ids[1, 3] == 10 and ids[0, 0] == 10 and ids[2, 1] == 10
        assert xyz[1, 3].tobytes() == _by_name("one_pair")["xyz"][0, 0].tobytes()                    # src(10) = frame 0, row 0
        c = _by_name("best_is_not_the_smallest")
        ids, xyz, mp, info = run(c)
        assert info[4:] == [1, 3, 6, 0] and mp[20:24].tolist() == [22] * 4
        assert [ids[k, k] for k in range(4)] == [22] * 4 and [ids[10 + k, 2] for k in range(4)] == [22] * 4
        assert all(xyz[10 + k, 2].tobytes() == c["xyz"][2, 2].tobytes() for k in (0, 1, 3)) and np.isnan(xyz[12, 2]).all()      # the best's own row stays
        c = _by_name("no_triangulated_member")
        ids, xyz, mp, info = run(c)
        assert mp[30:33].tolist() == [30] * 3 and info[4:] == [1, 2, 2, 1]
        assert ids[0, 0] == 30 and ids[1, 0] == 30 and ids[1, 5] == -1 and ids[2, 2] == 30 and np.isnan(xyz[[0, 1, 1, 2], [0, 0, 5, 2]]).all()
        c = _by_name("frame_holds_best_and_members")
        ids, xyz, mp, info = run(c)
        assert ids[0, 1:4].tolist() == [40, -1, -1] and ids[1, 1] == 40 and ids[1, 4] == -1 and info[4:] == [1, 2, 1, 3]
        assert xyz[0, 1].tobytes() == c["xyz"][0, 1].tobytes() and xyz[1, 1].tobytes() == c["xyz"][0, 1].tobytes() and np.isnan(xyz[0, 2:4]).all()
        c = _by_name("frame_holds_two_non_best")
        ids, xyz, mp, info = run(c)                                   # frame 1: m* = 51, its first row is 2
        assert ids[1, [7, 2, 9]].tolist() == [-1, 50, -1] and ids[2, 3] == 50 and info[4:] == [1, 2, 2, 2]
        c = _by_name("one_id_at_two_rows")
        ids, xyz, mp, info = run(c)                                   # frame 1: 61 at rows 2, 5, 8 -> row 2; frame 2 holds the best twice and keeps both
        assert ids[1, [2, 5, 8]].tolist() == [60, -1, -1] and ids[2, [1, 6, 7]].tolist() == [60, 60, -1] and info[4:] == [1, 1, 1, 3]
        assert np.isnan(xyz[2, 6]).all() and xyz[2, 1].tobytes() == c["xyz"][2, 1].tobytes()
        ids, xyz, mp, info = run(_by_name("ids_out_of_range"))
        assert info == [3, 3, 0, 0, 1, 1, 1, 0] and mp[71] == 70 and mp[72] == 72
        c = _by_name("adoption")
        ids, xyz, mp, info = run(c)                                   # rows (40, 0) and (40, 1) adopt 200 and 201; the masked entry is dropped
        assert info == [2, 1, 0, 2, 0, 0, 0, 0] and ids[40, :3].tolist() == [200, 201, -1]
        assert xyz[40, 0].tobytes() == c["xyz"][30, 0].tobytes() and np.isnan(xyz[40, 1]).all() and (mp == np.arange(mr.P_)).all()
        c = _by_name("two_entries_adopt_one_row")
        ids, xyz, mp, info = run(c)                                   # row (41, 5) takes 205 of {210, 205, 207}; 205 is triangulated and the best
        # 207 becomes 205 in frames 31 and 33; 210 is cleared beside 205 in frame 30
        assert info == [3, 0, 0, 1, 1, 2, 2, 1] and ids[41, 5] == 205 and mp[[205, 207, 210]].tolist() == [205] * 3
        assert ids[30, :2].tolist() == [-1, 205] and ids[31, 0] == 205 and ids[32, 4] == 205 and ids[33, 4] == 205
        ids, xyz, mp, info = run(_by_name("epipolar_pass_fail_nan"))
        assert info == [1, 0, 2, 0, 1, 1, 1, 0] and mp[230] == 240 and ids[43, :3].tolist() == [240, 241, 242] and ids[30, :3].tolist() == [240, 231, 232]
        ids, xyz, mp, info = run(_by_name("stages_1_to_5"))
        assert info[:4] == [1, 0, 0, 0] and mp[256] == 250 and (mp != np.arange(mr.P_)).sum() == 1
        c = _by_name("dead_entries")
        ids, xyz, mp, info = run(c)
        assert info == [4, 0, 0, 1, 1, 1, 1, 0] and ids[44, 2] == 265 and mp[262] == 260
        for name in ("no_queries", "no_live_entry", "no_pairs"):
            c = _by_name(name)
            ids, xyz, mp, info = run(c)
            assert ids.tobytes() == c["ids"].tobytes() and xyz.tobytes() == c["xyz"].tobytes() and (mp == np.arange(mr.P_)).all() and not any(info[3:]), name


def test_epipolar_gate_is_a_decision_with_margin():
    c = _by_name("epipolar_pass_fail_nan")
    ers = _margins(c)
    assert len(ers) == 3 and ers[0] < 10 and ers[1] > 10 and np.isnan(ers[2])
    assert abs(ers[0] - 6.5) < 0.05 and abs(ers[1] - 14.0) < 0.05      # the planted distances, up to the float32 keypoint


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_seeded_tables(core, seed):
    case = mr.seeded_case(seed)
    ers = _margins(case)
    want = mr.merge(case)
    got = mr.run_host(core, case)
    assert mr.same(got, want), (got[3], want[3])
    info = want[3]
    print(case["name"], info, len(ers))
    assert info[0] > 50 and info[1] > 10 and info[2] > 3 and info[3] > 5 and info[4] > 10 and info[6] > 10 and info[7] > 5      # a busy table
    assert sum(1 for e in ers if e < 10) > 3
    # order independence and hostile padding, on the host statement
    assert mr.same(mr.run_host(core, mr.permuted(case, 7 + seed)), want)
    p = mr.poisoned(case)
    gp = mr.run_host(core, p)
    live = np.zeros((mr.F_, mr.CAP), bool)
    for f in range(case["size"]):
        live[f, :min(max(int(case["n"][f]), 0), mr.CAP)] = True
    assert gp[3] == want[3] and np.array_equal(gp[2], want[2]) and np.array_equal(gp[0][live], want[0][live]) and gp[1][live].tobytes() == want[1][live].tobytes()
    assert np.array_equal(gp[0][~live], p["ids"][~live]) and gp[1][~live].tobytes() == p["xyz"][~live].tobytes()


# ---- the library and its kernels ----------------------------------------------------------------------------------------------------------------------
NEW = ("airfe_bowdb_attach_merge", "airfe_bowdb_merge_points_dev", "airfe_bowdb_merge_points", "airfe_bowdb_loop_merge_batch_dev")


def test_library_exports_the_new_entries(libpath):
    lib = C.CDLL(libpath)
    from airslam_amd import _lib, api, build
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    for name in ("attach_merge", "merge_points_dev", "merge_points", "loop_merge_batch_dev", "loop_close_dev"):
        assert callable(getattr(api.BowDatabase, name)), name
    assert "kernels_merge.hip" in build.SOURCES and build.EXTRA_FLAGS["kernels_merge.hip"] == ["-ffp-contract=off"]
    header = open(os.path.join(ROOT, "include", "airfe.h")).read()
    assert all(re.search(r"\b" + name + r"\(", header) for name in NEW)


def test_new_kernels_use_no_scratch_and_do_not_spill():
    from airslam_amd import build
    src = "kernels_merge.hip"
    r = subprocess.run(["/opt/rocm/bin/hipcc"] + build.FLAGS + build.EXTRA_FLAGS.get(src, []) + ["-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        os.path.join(CSRC, src), "-o", os.devnull], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    sspill = [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", r.stderr)]
    vspill = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", r.stderr)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert sum("merge_" in n for n in names) == 8 and len(scratch) == len(sspill) == len(vspill) == len(lds) == len(names), names
    assert not any(scratch) and not any(sspill) and not any(vspill), list(zip(names, scratch, sspill, vspill))
    for n, b in zip(names, lds):                                    # LDS in the relabel kernel alone: the rows' (id, group) at cap 1024
        assert (0 < b <= 8192) if "merge_relabel" in n else b == 0, (n, b)
    assert "-mwavefrontsize32" not in " ".join(build.FLAGS)         # gfx950's default: wave64
