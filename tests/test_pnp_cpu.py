"""PnP RANSAC of SolvePnPWithCV (src/g2o_optimization/g2o_optimization.cc:1085-1134) and the stereo points that feed it, on the CPU: the host core
(airslam_amd/csrc/pnp_core.h, compiled here with the host compiler) against the numpy restatement (tests/pnp_ref.py) bit for bit, on planted geometry;
the gate, the sampler, the degenerate cases; the library's new symbols; no scratch in the new kernels.

What these pin: the project's contract (include/airfe.h, "PnP RANSAC") and that its statements agree.  Not OpenCV's numerics: OpenCV is not part of
this project."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pnp_ref as pr
from conftest import ROOT

CSRC = os.path.join(ROOT, "airslam_amd", "csrc")
SHIM = r'''
#include "pnp_core.h"
extern "C" int core_pnp(const float* obj, const float* img, int n, const double* K, double* Twc, double* Rt, uint8_t* mask, int* count, int* scores) {
  return pnp_solve_host(obj, img, n, K, Twc, Rt, mask, count, scores);
}
extern "C" int core_stereo(const float* fl, int nl, const float* fr, const int32_t* idx, int m, const double* cam, double* u, double* d, double* x) {
  return pnp_stereo_host(fl, nl, fr, idx, m, cam, u, d, x);
}
extern "C" int core_sample(int n, int s, int* id) { return pnp_sample(n, s, id) ? 1 : 0; }
extern "C" int core_niters(int n, int good, int max_iters) { return pnp_update_niters(n, good, max_iters); }
'''


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    """pnp_core.h as this tree has it, compiled for the host without FMA contraction"""
    d = tmp_path_factory.mktemp("pnp_core")
    src, so = d / "core.cpp", str(d / "libpnpcore.so")
    src.write_text(SHIM)
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-w", "-fPIC", "-ffp-contract=off", "-shared", "-I" + CSRC, str(src), "-o", so],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(so)
    lib.core_pnp.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 6
    lib.core_stereo.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 4
    lib.core_sample.argtypes = [C.c_int, C.c_int, C.c_void_p]
    return lib


def run_core(lib, obj, img, K=pr.K_EUROC):
    obj = np.ascontiguousarray(obj, np.float32).reshape(-1, 3)
    img = np.ascontiguousarray(img, np.float32).reshape(-1, 2)
    n = len(obj)
    k = np.array(K, np.float64)
    Twc, Rt, mask, sc, cnt = np.zeros(16), np.zeros(12), np.zeros(max(n, 1), np.uint8), np.zeros(100, np.int32), C.c_int(0)
    win = lib.core_pnp(obj.ctypes.data, img.ctypes.data, n, k.ctypes.data, Twc.ctypes.data, Rt.ctypes.data, mask.ctypes.data, C.byref(cnt), sc.ctypes.data)
    return dict(Twc=Twc.reshape(4, 4), Rt=Rt, inlier=mask[:n], count=cnt.value, win=win, scores=sc)


def _assert_same(a, b):
    assert a["win"] == b["win"] and a["count"] == b["count"]
    assert a["inlier"].tobytes() == b["inlier"].tobytes()
    assert np.asarray(a["Rt"], np.float64).tobytes() == np.asarray(b["Rt"], np.float64).tobytes()
    assert np.asarray(a["Twc"], np.float64).tobytes() == np.asarray(b["Twc"], np.float64).tobytes()


def test_library_exports_the_new_entries(libpath):
    lib = C.CDLL(libpath)
    for name in ("airfe_pnp_ransac", "airfe_pnp_ransac_batch_dev", "airfe_stereo_points", "airfe_stereo_points_batch_dev", "airfe_track_pose_batch_dev"):
        assert hasattr(lib, name), name


def test_ransac_update_num_iters(core):
    # RANSACUpdateNumIters(0.99, (n - good) / n, 5, 100): round(log(0.01) / log(1 - (good / n)^5)), capped at 100; 0 when every point is an inlier
    want = {100: 0, 95: 3, 90: 5, 80: 12, 70: 25, 60: 57, 50: 100, 30: 100, 5: 100}
    for good, v in want.items():
        assert pr.update_niters(100, good, 100) == v, good
        assert core.core_niters(100, good, 100) == v, good
    assert pr.update_niters(100, 90, 4) == core.core_niters(100, 90, 4) == 4          # the running bound is an upper cap


def test_sampler_is_a_pure_function_of_sample_and_n(core):
    for n in (8, 9, 30, 1024):
        for s in (0, 1, 57, 99):
            ids = np.zeros(5, np.int32)
            assert core.core_sample(n, s, ids.ctypes.data) == 1
            assert ids.tolist() == pr.sample(n, s) == pr.sample(n, s)
            assert len(set(ids.tolist())) == 5 and (ids >= 0).all() and (ids < n).all()
    # another problem drawn in between changes nothing: the stream has no state
    a = pr.sample(300, 7)
    pr.sample(12, 3)
    assert pr.sample(300, 7) == a


def test_gate_below_eight_and_exactly_eight(core):
    obj, img, R, t, _ = pr.planted(8, 1.0, seed=11)
    for n in range(0, 8):
        r = run_core(core, obj[:n], img[:n])
        assert r["count"] == 0 and r["win"] == -1 and not r["inlier"].any()
        assert r["Twc"].tobytes() == np.eye(4).tobytes()
        _assert_same(r, pr.pnp_ransac(obj[:n], img[:n]))
    r = run_core(core, obj, img)
    _assert_same(r, pr.pnp_ransac(obj, img))
    assert r["count"] == 8 and r["inlier"].all()
    rot, tr = pr.pose_errors(r["Rt"], R, t)
    assert rot < 0.5 and tr < 0.05


def test_all_outliers_give_no_model(core):
    rng = np.random.default_rng(3)
    n = 200
    obj = np.stack([rng.uniform(-10, 10, n), rng.uniform(-5, 5, n), rng.uniform(1, 20, n)], 1).astype(np.float32)
    img = np.stack([rng.uniform(0, pr.W, n), rng.uniform(0, pr.H, n)], 1).astype(np.float32)
    r = run_core(core, obj, img)
    _assert_same(r, pr.pnp_ransac(obj, img))
    assert r["count"] == 0 and r["win"] == -1 and not r["inlier"].any()
    assert r["Twc"].tobytes() == np.eye(4).tobytes() and r["Rt"].tobytes() == np.array(pr.IDENTITY12).tobytes()


def test_planar_and_collinear_points_give_a_finite_result_or_none(core):
    obj, img, _, _, _ = pr.planted(120, 0.9, seed=21, planar=True)
    r = run_core(core, obj, img)
    _assert_same(r, pr.pnp_ransac(obj, img))
    assert np.isfinite(r["Twc"]).all() and (r["count"] == 0 or r["count"] >= 5)
    # every sample collinear: the points on one 3-D line
    n = 40
    s = np.linspace(0.0, 1.0, n)
    line = np.stack([-2 + 4 * s, -1 + 2 * s, 3 + 10 * s], 1)
    proj = np.stack([line[:, 0] / line[:, 2] * pr.K_EUROC[0] + pr.K_EUROC[2], line[:, 1] / line[:, 2] * pr.K_EUROC[1] + pr.K_EUROC[3]], 1)
    r = run_core(core, line, proj)
    _assert_same(r, pr.pnp_ransac(line, proj))
    assert np.isfinite(r["Twc"]).all() and np.isfinite(r["Rt"]).all()


@pytest.mark.parametrize("n,ratio,seed", [(8, 1.0, 1), (12, 0.8, 2), (30, 0.8, 3), (100, 0.6, 4), (300, 0.9, 5), (300, 0.5, 6), (64, 0.7, 7)])
def test_host_core_equals_the_numpy_restatement(core, n, ratio, seed):
    obj, img, _, _, _ = pr.planted(n, ratio, seed)
    r, ref = run_core(core, obj, img), pr.pnp_ransac(obj, img)
    _assert_same(r, ref)
    for s, v in ref["scores"].items():                       # every sample the sequential rule visits scores the same
        assert r["scores"][s] == v, s


@pytest.mark.parametrize("n", [8, 12, 30, 100, 300, 1000])
def test_planted_motion_is_recovered(core, n):
    ratio = 1.0 if n < 30 else 0.8
    worst = (0.0, 0.0)
    for seed in range(3):
        obj, img, R, t, truth = pr.planted(n, ratio, seed=100 * n + seed)
        r = run_core(core, obj, img)
        assert r["count"] > 0
        rot, tr = pr.pose_errors(r["Rt"], R, t)
        kept = r["inlier"].astype(bool)
        if n >= 30:
            assert not (kept & ~truth).any()
            assert (kept & truth).sum() >= 0.99 * truth.sum(), ((kept & truth).sum(), truth.sum())
            # (24 inliers at 0.5 px over 1-20 m of depth do not pin the translation to a millimetre: 1 cm there)
            assert rot <= 0.1 and tr <= 0.01 * np.linalg.norm(t) + (1e-3 if n >= 100 else 1e-2), (rot, tr, np.linalg.norm(t))
        else:
            assert rot <= 1.0 and tr <= 0.1 * np.linalg.norm(t) + 0.05, (rot, tr)
        worst = (max(worst[0], rot), max(worst[1], tr))
    Twc = r["Twc"]
    np.testing.assert_allclose(Twc[:3, :3], np.asarray(r["Rt"][:9]).reshape(3, 3).T, rtol=0, atol=0)
    np.testing.assert_allclose(Twc[:3, 3], -Twc[:3, :3] @ r["Rt"][9:], rtol=1e-12, atol=1e-12)


def test_stereo_points_core_equals_the_restatement_and_the_seq_count(core, libpath):
    from airslam_amd import _lib
    fL, fR, idx, X = pr.stereo_rows(300, seed=4)
    idx = np.concatenate([idx, idx[:20][:, ::-1], idx[5:9]])          # out-of-band entries and repeated left indices (the later one wins)
    idx[-4:, 1] = idx[:4, 1]
    idx = np.ascontiguousarray(idx, np.int32)
    cam = np.array(pr.CAM_EUROC)
    u, d, xyz = np.zeros(300), np.zeros(300), np.zeros((300, 3))
    good = core.core_stereo(fL.ctypes.data, 300, fR.ctypes.data, idx.ctypes.data, len(idx), cam.ctypes.data, u.ctypes.data, d.ctypes.data, xyz.ctypes.data)
    ref = pr.stereo_points(fL, fR, idx)
    assert good == ref["good"] and u.tobytes() == ref["u_right"].tobytes() and d.tobytes() == ref["depth"].tobytes()
    assert xyz.tobytes() == ref["xyz"].tobytes()
    set_ = d > 0
    assert set_.sum() > 250 and np.isnan(xyz[~set_]).all()
    assert (xyz[set_, 2] != d[set_]).any()                            # the float-parallax depth and the double-difference point differ somewhere
    lib = _lib.lib()
    p = _lib.SeqPolicy()
    lib.airfe_seq_default_policy(C.byref(p))
    assert lib.airfe_seq_good_stereo_points(C.byref(p), fL.ctypes.data, fR.ctypes.data, idx.ctypes.data, len(idx)) == good
    np.testing.assert_allclose(xyz[set_], X[set_], rtol=0.05, atol=0.05)


def test_new_kernels_use_no_scratch():
    from test_no_scratch_cpu import _usage
    u = _usage("kernels_pnp.hip")
    names = [n for n in u if "pnp_" in n]
    assert len(names) == 4, names
    for n in names:
        assert u[n].get("ScratchSize [bytes/lane]", 0) == 0 and u[n].get("VGPRs Spill", 0) == 0, (n, u[n])
