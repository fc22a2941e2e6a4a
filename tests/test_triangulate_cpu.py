"""Map-point triangulation on the CPU (include/airfe.h "Map-point triangulation"): the host statement of airslam_amd/csrc/triangulate_core.h, compiled
here with the host compiler, against the Python restatement (tests/triangulate_ref.py) byte for byte; the restatement against an independent formulation
through numpy.linalg.solve; planted points; the rank rule with its margins; the library's new symbols; the new kernels' resource usage."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import triangulate_ref as tr
from conftest import ROOT

CSRC = os.path.join(ROOT, "airslam_amd", "csrc")
SHIM = r'''
#include "triangulate_core.h"
extern "C" int core_point(const double* cam, const double* Twc, const float* xy, int n, int min_observers, double* xyz) {
  double cami[4];
  if (!tr_cam(cam, cami)) return -100;
  return triangulate_point_host(cami, Twc, xy, n, min_observers, xyz);
}
extern "C" int core_build(const float* feat, int feat_dim, const int* n, const double* pose, const int32_t* point_id, int size, int cap, int max_points,
                          const double* cam, int min_observers, double* xyz, int32_t* status, int32_t* nobs, int32_t* info) {
  double cami[4];
  if (!tr_cam(cam, cami)) return -100;
  triangulate_build_host(feat, feat_dim, n, pose, point_id, size, cap, max_points, cami, min_observers, xyz, status, nobs, info);
  return 0;
}
extern "C" int core_qr(const double* A, const double* rhs, double* x, double* rdiag) { return tr_qr_solve(A, rhs, x, rdiag); }
'''
# The gate of the restatement against numpy.linalg.solve (test_restatement_against_an_independent_formulation): MEASURED is the largest relative error
# |x - x_np| / |x_np| over the 428 solved points of the three seeded scenes on the development CPU (the worst points have short baselines, |R_33| / |R_11|
# down to 1.4e-4); the gate is 16 times that, for another libm or BLAS.
MEASURED = 1.016e-12
GATE = 16 * MEASURED


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    """triangulate_core.h as this tree has it, compiled for the host without contraction"""
    d = tmp_path_factory.mktemp("triangulate_core")
    src, so = d / "core.cpp", str(d / "libtricore.so")
    src.write_text(SHIM)
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-w", "-fPIC", "-shared", "-I" + CSRC, str(src), "-o", so], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(so)
    lib.core_point.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.core_build.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 3 + [C.c_void_p, C.c_int] + [C.c_void_p] * 4
    lib.core_qr.argtypes = [C.c_void_p] * 4
    return lib


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def host_point(lib, observers, min_observers=2, cam=tr.CAM):
    Twc = np.array([o[2] for o in observers], np.float64).reshape(-1, 16)
    xy = np.array([(o[0], o[1]) for o in observers], np.float32).reshape(-1, 2)
    cam = np.array(cam, np.float64)
    xyz = np.full(3, 7.0)
    st = lib.core_point(cam.ctypes.data, Twc.ctypes.data, xy.ctypes.data, len(observers), min_observers, xyz.ctypes.data)
    return xyz, st


def host_build(lib, xy, n, pose, ids, size, max_points, min_observers=2, cam=tr.CAM):
    feat = tr.feat_rows(xy)
    n, pose, ids, cam = np.ascontiguousarray(n, np.int32), np.ascontiguousarray(pose, np.float64), np.ascontiguousarray(ids, np.int32), np.array(cam, np.float64)
    xyz = np.full((max_points, 3), 7.0)
    status, nobs, info = np.full(max_points, -7, np.int32), np.full(max_points, -7, np.int32), np.full(4, -7, np.int32)
    assert lib.core_build(feat.ctypes.data, 259, n.ctypes.data, pose.ctypes.data, ids.ctypes.data, size, ids.shape[1], max_points, cam.ctypes.data, min_observers,
                          xyz.ctypes.data, status.ctypes.data, nobs.ctypes.data, info.ctypes.data) == 0
    return xyz, status, nobs, info.tolist()


@pytest.mark.parametrize("case", tr.hand_cases(), ids=lambda c: c[0])
def test_hand_cases(core, case):
    name, observers, want = case
    x, st, _ = tr.point(tr.CAM, observers)
    assert st == want, (name, st)
    got, gst = host_point(core, observers)
    assert gst == want and np.array_equal(bits(got), bits(x)), (name, gst, got, x)
    assert np.isnan(x).all() == (want != 0)
    if want == 0:
        assert np.linalg.norm(np.array(x) - (0.5, -0.25, 6.0)) < 1e-3 * np.linalg.norm((0.5, -0.25, 6.0))


def test_seeded_table(core):
    xy, n, pose, ids, _ = tr.seeded_table()
    frames, P = ids.shape[0], 300
    for size, mo in ((frames, 2), (frames, 3), (frames - 5, 2), (1, 2), (0, 2)):
        want = tr.build(xy, n, pose, ids, size, P, min_observers=mo)
        got = host_build(core, xy, n, pose, ids, size, P, min_observers=mo)
        assert tr.same(got, want), (size, mo, got[3], want[3])
        if size == frames and mo == 2:                              # a busy table: the cases mean something
            st, nobs = want[1], want[2]
            assert want[3][0] > 120 and (st == -1).sum() >= 19 and (st == 1).sum() >= 1 and int(nobs.max()) >= 8
            assert (np.isnan(want[0]).all(1) == (st != 0)).all()
    # hostile rows past n[f] and frames past size change nothing
    want = tr.build(xy, n, pose, ids, frames - 5, P)
    nxy, nids, npose = xy.copy(), ids.copy(), pose.copy()
    for f in range(frames):
        nids[f, n[f]:] = [2 ** 31 - 1, -2 ** 31, 5, P - 1][f % 4]
        nxy[f, n[f]:] = np.nan
    nids[frames - 5:], nxy[frames - 5:], npose[frames - 5:] = 7, np.inf, np.nan
    assert tr.same(host_build(core, nxy, n, npose, nids, frames - 5, P), want)


def test_a_bad_point_changes_no_other_point(core):
    xy, n, pose, ids, _ = tr.seeded_table()
    frames, P = ids.shape[0], 300
    clean = tr.build(xy, n, pose, ids, frames, P)
    m = int(np.argmax(clean[2]))                                    # the busiest point: one of its keypoints becomes NaN
    f, i = sorted(tr.observers_of(xy, n, pose, ids, frames, P)[m].items())[1]
    bxy = xy.copy()
    bxy[f, i, 0] = np.nan
    for got in (tr.build(bxy, n, pose, ids, frames, P), host_build(core, bxy, n, pose, ids, frames, P)):
        assert got[1][m] == 3 and np.isnan(got[0][m]).all() and got[3][3] == clean[3][3] + 1
        keep = np.arange(P) != m
        assert tr.same((got[0][keep], got[1][keep], got[2][keep], []), (clean[0][keep], clean[1][keep], clean[2][keep], []))


def _scenes():
    return [tr.seeded_table(), tr.seeded_table(frames=24, cap=48, max_points=150, seed=9, noise=1.0), tr.planted_scene()]


def test_restatement_against_an_independent_formulation():
    worst, count = 0.0, 0
    for xy, n, pose, ids, X in _scenes():
        frames, P = ids.shape[0], len(X)
        xyz, status, nobs, _ = tr.build(xy, n, pose, ids, frames, P)
        obs = tr.observers_of(xy, n, pose, ids, frames, P)
        for m in np.flatnonzero(status == 0):
            lst = [(float(xy[f][i][0]), float(xy[f][i][1]), pose[f]) for f, i in sorted(obs[int(m)].items())]
            ref = tr.independent(tr.CAM, lst)
            worst = max(worst, float(np.linalg.norm(xyz[m] - ref) / np.linalg.norm(ref)))
            count += 1
    print(f"restatement vs numpy.linalg.solve: {count} points, largest relative error {worst:.3e}, gate {GATE:.3e}")
    assert count > 300 and worst <= GATE, (worst, GATE)


def test_planted_points_are_recovered(core):
    xy, n, pose, ids, X = tr.planted_scene()
    frames, P = ids.shape[0], len(X)
    xyz, status, nobs, info = host_build(core, xy, n, pose, ids, frames, P)
    assert list(nobs[:6]) == [0, 1, 2, 3, 4, 5] and list(status[:6]) == [-1, 1, 0, 0, 0, 0]
    assert (status[6:] == 0).sum() > 100 and ((status == 0) == (nobs >= 2)).all()
    ok = status == 0
    rel = np.linalg.norm(xyz[ok] - X[ok], axis=1) / np.linalg.norm(X[ok], axis=1)
    print(f"planted: {int(ok.sum())} points, largest relative error {rel.max():.3e}")
    assert rel.max() < 1e-3                                        # the float32 rounding of x and y bounds this, not the solver


def test_rank_rule_is_decisive(core):
    cases = {c[0]: c for c in tr.hand_cases()}
    for name in ("same_ray_x4", "parallel_x2", "parallel_x3"):
        _, st, rdiag = tr.point(tr.CAM, cases[name][1])
        r = sorted(abs(v) for v in rdiag)
        assert st == 2 and r[0] < 1e-12 * r[2] and r[1] > 0.1 * r[2], (name, rdiag)      # the third pivot is rounding noise against 1e-5, the second is not
        A, rhs, _ = tr.system(tr.cam_inverse(tr.CAM), cases[name][1])
        A, rhs, x, rd = np.array(A), np.array(rhs), np.zeros(3), np.zeros(3)
        assert core.core_qr(A.ctypes.data, rhs.ctypes.data, x.ctypes.data, rd.ctypes.data) == 2 and np.array_equal(bits(rd), bits(rdiag))
    _, st, rdiag = tr.point(tr.CAM, cases["three_spread"][1])
    assert st == 0 and abs(rdiag[2]) / abs(rdiag[0]) > 1e-2, rdiag
    # the pivot order: |R_11| >= |R_22| >= |R_33| up to rounding on every solved point of the seeded table
    xy, n, pose, ids, _ = tr.seeded_table()
    obs = tr.observers_of(xy, n, pose, ids, ids.shape[0], 300)
    worst = 1.0
    for m, frames in obs.items():
        lst = [(float(xy[f][i][0]), float(xy[f][i][1]), [float(t) for t in pose[f]]) for f, i in sorted(frames.items())]
        _, st, rdiag = tr.point(tr.CAM, lst)
        if st == 0:
            assert abs(rdiag[0]) >= abs(rdiag[1]) * (1 - 1e-12)
            worst = min(worst, abs(rdiag[2]) / abs(rdiag[0]))
    assert worst > 10 * tr.RANK_TOL, worst                           # no solved point of the table sits near the threshold (the lowest: 1.44e-4)


def test_context_free_entry(libpath, core):
    from airslam_amd import api
    for name, observers, want in tr.hand_cases():
        Twc = np.array([o[2] for o in observers], np.float64).reshape(-1, 16)
        xy = np.array([(o[0], o[1]) for o in observers], np.float32).reshape(-1, 2)
        x, st = api.triangulate_point(tr.CAM, Twc, xy)
        ref, rst, _ = tr.point(tr.CAM, observers)
        assert st == rst == want and np.array_equal(bits(x), bits(ref)), name
    two = [o for o in tr.hand_cases() if o[0] == "two"][0][1]
    Twc, xy = np.array([o[2] for o in two]), np.array([(o[0], o[1]) for o in two], np.float32)
    for cam in ((0.0, 410.0, 320.0, 240.0), (400.0, float("nan"), 320.0, 240.0), (float("inf"), 410.0, 320.0, 240.0)):
        with pytest.raises(api.AirfeError):
            api.triangulate_point(cam, Twc, xy)


# ---- the library and its kernels ----------------------------------------------------------------------------------------------------------------------
NEW = ("airfe_bowdb_attach_triangulation", "airfe_bowdb_triangulate_points_dev", "airfe_bowdb_triangulate_points", "airfe_bowdb_fill_points_dev",
       "airfe_triangulate_point")


def test_library_exports_the_new_entries(libpath):
    lib = C.CDLL(libpath)
    from airslam_amd import _lib, api, build
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    for name in ("attach_triangulation", "triangulate_points_dev", "triangulate_points", "fill_points_dev", "retriangulate_dev"):
        assert callable(getattr(api.BowDatabase, name)), name
    assert callable(api.triangulate_point)
    assert "kernels_triangulate.hip" in build.SOURCES and build.EXTRA_FLAGS["kernels_triangulate.hip"] == ["-ffp-contract=off"]


def test_new_kernels_use_no_scratch_and_do_not_spill():
    from airslam_amd import build
    src = "kernels_triangulate.hip"
    r = subprocess.run(["/opt/rocm/bin/hipcc"] + build.FLAGS + build.EXTRA_FLAGS.get(src, []) + ["-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        os.path.join(CSRC, src), "-o", os.devnull], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    sspill = [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", r.stderr)]
    vspill = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", r.stderr)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", r.stderr)]
    assert len(names) == 4 and sum("tri_" in n for n in names) == 3 and sum("fill_points" in n for n in names) == 1, names
    assert len(scratch) == len(sspill) == len(vspill) == len(lds) == len(vgprs) == 4
    assert not any(scratch) and not any(sspill) and not any(vspill), list(zip(names, scratch, sspill, vspill))
    assert not any(lds) and max(vgprs) <= 128                       # no LDS at all; the point kernel's accumulators and the solve stay in registers
