"""Pose-only frame optimisation (the vision-only, points-only FrameOptimization of tracking, src/g2o_optimization/g2o_optimization.cc:446-898) on the CPU:
the host core (airslam_amd/csrc/poseopt_core.h, compiled here with the host compiler) against the Python restatement (tests/poseopt_ref.py) bit for bit
on planted constraints; planted motion recovered from the identity start; the rounds; the degenerate cases; the library's new symbols; no scratch in the
new kernels.

What these pin: the project's contract (include/airfe.h, "Frame optimisation") and that its statements agree.  Not g2o's numerics: g2o is not part of
this project."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import poseopt_ref as po
from conftest import ROOT

CSRC = os.path.join(ROOT, "airslam_amd", "csrc")
SHIM = r'''
#include "poseopt_core.h"
extern "C" int core_poseopt(const double* X, const double* obs, int n, const double* cam, const double* Tcb, const double* thr, const double* Twc0,
                            double* Twc, double* Rt, uint8_t* inlier, int* num, double* trace) {
  return poseopt_solve_host(X, obs, n, cam, Tcb, thr, Twc0, Twc, Rt, inlier, num, trace);
}
extern "C" int core_use_last(const double* Tpnp, int count, const double* Tlast, int lost) {
  return po_use_last(Tpnp, count, Tlast[3], Tlast[7], Tlast[11], lost) ? 1 : 0;
}
'''
CAM = np.array(po.CAM_EUROC)
THR = np.array(po.THR_EUROC)
EYE = np.eye(4)


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    """poseopt_core.h as this tree has it, compiled for the host without FMA contraction"""
    d = tmp_path_factory.mktemp("poseopt_core")
    src, so = d / "core.cpp", str(d / "libposeoptcore.so")
    src.write_text(SHIM)
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-w", "-fPIC", "-ffp-contract=off", "-shared", "-I" + CSRC, str(src), "-o", so],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(so)
    lib.core_poseopt.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 9
    lib.core_use_last.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    return lib


def run_core(lib, X, obs, Twc0=EYE, cam=CAM, thr=THR, Tcb=None):
    X = np.ascontiguousarray(X, np.float64).reshape(-1, 3)
    obs = np.ascontiguousarray(obs, np.float64).reshape(-1, 3)
    n = len(X)
    cam, thr = np.ascontiguousarray(cam, np.float64), np.ascontiguousarray(thr, np.float64)
    T0 = np.ascontiguousarray(Twc0, np.float64).reshape(16)
    tcb = None if Tcb is None else np.ascontiguousarray(Tcb, np.float64).reshape(12)
    Twc, Rt, mask, trace, num = np.zeros(16), np.zeros(12), np.zeros(max(n, 1), np.uint8), np.zeros((3, 4)), C.c_int(0)
    rounds = lib.core_poseopt(X.ctypes.data, obs.ctypes.data, n, cam.ctypes.data, None if tcb is None else tcb.ctypes.data, thr.ctypes.data,
                              T0.ctypes.data, Twc.ctypes.data, Rt.ctypes.data, mask.ctypes.data, C.byref(num), trace.ctypes.data)
    return dict(Twc=Twc.reshape(4, 4), Rt=Rt, inlier=mask[:n], num_inliers=num.value, rounds=rounds, trace=trace)


def _assert_same(a, b, trace=True):
    assert a["num_inliers"] == b["num_inliers"]
    assert np.asarray(a["inlier"], np.uint8).tobytes() == np.asarray(b["inlier"], np.uint8).tobytes()
    assert np.asarray(a["Rt"], np.float64).tobytes() == np.asarray(b["Rt"], np.float64).tobytes()
    assert np.asarray(a["Twc"], np.float64).tobytes() == np.asarray(b["Twc"], np.float64).tobytes()
    if trace:
        assert a["rounds"] == b["rounds"]
        assert np.asarray(a["trace"], np.float64).tobytes() == np.asarray(b["trace"], np.float64).tobytes(), (a["trace"], b["trace"])


def test_library_exports_the_new_entries(libpath):
    lib = C.CDLL(libpath)
    for name in ("airfe_frame_optimize", "airfe_frame_optimize_batch_dev", "airfe_track_pose_opt_batch_dev"):
        assert hasattr(lib, name), name


@pytest.mark.parametrize("stereo", [False, True])
@pytest.mark.parametrize("ratio", [1.0, 0.8, 0.5])
@pytest.mark.parametrize("n", [10, 30, 100, 300, 1000])
def test_host_core_equals_the_python_restatement(core, n, ratio, stereo):
    X, obs, _, _, _ = po.planted_constraints(n, ratio, seed=17 * n + int(10 * ratio), stereo=stereo)
    if stereo:
        assert (obs[:, 2] > 0).sum() >= n // 4
    r, ref = run_core(core, X, obs), po.frame_optimize(X, obs)
    _assert_same(r, ref)
    assert r["rounds"] == 3 and (r["trace"][:, 3] >= 1).all()


def test_host_core_equals_the_restatement_with_an_extrinsic_and_a_start_pose(core):
    X, obs, R, t, _ = po.planted_constraints(200, 0.8, seed=5, stereo=True)
    import pnp_ref as pr
    Tcb = np.concatenate([pr.rotation((0.2, -1.0, 0.4), 7.0).reshape(9), [0.05, -0.02, 0.1]])
    T0 = np.eye(4)
    T0[:3, :3] = pr.rotation((1.0, 0.3, -0.2), 2.0)
    T0[:3, 3] = (0.05, -0.03, 0.02)
    r, ref = run_core(core, X, obs, Twc0=T0, Tcb=Tcb), po.frame_optimize(X, obs, Twc0=T0.reshape(16), Tcb=Tcb)
    _assert_same(r, ref)
    rot, tr = po.pose_errors(r["Rt"], R, t)
    assert rot <= 0.1 and tr <= 0.01 * np.linalg.norm(t) + 1e-3, (rot, tr)
    # Twc and Rt describe one pose
    np.testing.assert_allclose(r["Twc"][:3, :3], r["Rt"][:9].reshape(3, 3).T, rtol=0, atol=1e-12)
    np.testing.assert_allclose(r["Twc"][:3, 3], -r["Twc"][:3, :3] @ r["Rt"][9:], rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("n", [10, 30, 100, 300, 1000])
def test_planted_motion_is_recovered_from_the_identity_start(core, n):
    """the fallback case: the start is up to 10 deg / 0.5 m away.  Gates: test_pnp_cpu.py::test_planted_motion_is_recovered's, and no planted outlier
    flagged inlier, >= 99 % of the planted inliers flagged inlier"""
    for ratio in (1.0, 0.8, 0.5):
        for stereo in (False, True):
            for k in range(3):
                X, obs, R, t, truth = po.planted_constraints(n, ratio, seed=31 * n + k, stereo=stereo)
                r = run_core(core, X, obs)
                rot, tr = po.pose_errors(r["Rt"], R, t)
                nt = np.linalg.norm(t)
                print(f"n={n} ratio={ratio} stereo={stereo} seed={31 * n + k}: rot {rot:.4f} deg, tr {tr * 1e3:.2f} mm, inliers {r['num_inliers']}")
                kept = r["inlier"].astype(bool)
                assert not (kept & ~truth).any(), (n, ratio, stereo, k)
                assert (kept & truth).sum() >= 0.99 * truth.sum(), ((kept & truth).sum(), truth.sum())
                assert r["num_inliers"] == kept.sum()
                if n >= 100:
                    assert rot <= 0.1 and tr <= 0.01 * nt + 1e-3, (rot, tr, nt)
                elif n == 30:
                    assert rot <= 0.1 and tr <= 0.01 * nt + 1e-2, (rot, tr, nt)
                else:
                    assert rot <= 1.0 and tr <= 0.1 * nt + 0.05, (rot, tr, nt)


def test_fewer_than_ten_constraints_run_one_round(core):
    X, obs, _, _, _ = po.planted_constraints(12, 1.0, seed=3)
    for n in (1, 5, 9):
        r = run_core(core, X[:n], obs[:n])
        _assert_same(r, po.frame_optimize(X[:n], obs[:n]))
        assert r["rounds"] == 1 and not r["trace"][1:].any()
    r = run_core(core, X[:10], obs[:10])
    assert r["rounds"] == 3


def _levels_after_round_one(X, obs, T0):
    """the level flags after the first round: the restatement stopped after one round"""
    old = po.ROUNDS
    po.ROUNDS = 1
    try:
        r = po.frame_optimize(X, obs, Twc0=T0.reshape(16))
    finally:
        po.ROUNDS = old
    return ~r["inlier"].astype(bool)


def test_an_edge_rejected_in_round_one_can_return(core):
    """60 exact constraints (every one a true inlier of the identity pose) and a start pose far enough away (the issue's construction) that true
    inliers exceed the threshold after round 1 (level 1).  Round 2 starts again from the start pose over the remaining level-0 edges and ends
    elsewhere, and the classification over EVERY edge flags some of round 1's outliers inlier again: a level is not final."""
    import pnp_ref as pr
    rng = np.random.default_rng(12)
    n = 60
    z = rng.uniform(2.0, 6.0, n)
    u0, v0 = rng.uniform(0, pr.W, n), rng.uniform(0, pr.H, n)
    fx, fy, cx, cy = pr.K_EUROC
    X = np.stack([(u0 - cx) / fx * z, (v0 - cy) / fy * z, z], 1)
    obs = np.stack([u0, v0, np.full(n, -1.0)], 1)
    found = None
    for deg in (24.0, 25.0, 35.0, 45.0, 60.0):
        T0 = np.eye(4)
        T0[:3, :3] = pr.rotation((0.3, 1.0, 0.2), deg)
        T0[:3, 3] = (1.5, -0.5, 0.8)
        r = run_core(core, X, obs, Twc0=T0)
        _assert_same(r, po.frame_optimize(X, obs, Twc0=T0.reshape(16)))
        lv1 = _levels_after_round_one(X, obs, T0)
        print(f"start {deg} deg: {int(lv1.sum())} edges at level 1 after round 1, {int(r['inlier'][lv1].sum())} of them inliers at the end")
        if lv1.any() and r["inlier"][lv1].any():
            found = deg
            break
    assert found is not None, "no start pose made a round-1 outlier return"


def test_the_float_rounding_of_chi2_is_what_is_compared(core):
    """an edge whose double chi2 and float chi2 fall on different sides of the threshold is classified by the FLOAT value.  Constructed from a real
    problem: take an edge whose final chi2 rounds DOWN to float (float chi2 f < double chi2) and set the mono threshold to f: the rule says inlier
    (f > f is false), a double comparison would say outlier (chi2 > f)."""
    # the rule itself, on one constructed edge: a point on the optical axis seen from the identity pose, observed sqrt(50) (1 + 2^-30) px to the right
    fx, fy, cx, cy, bf = po.CAM_EUROC
    ex = np.sqrt(50.0) * (1.0 + 2.0 ** -30)
    P = po._Problem(np.array([[0.0, 0.0, 4.0]]), np.array([[cx + ex, cy, -1.0]]), po.CAM_EUROC, None, po.THR_EUROC)
    ident = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    chi2 = P.errors(ident)[3]
    assert chi2[0] > 50.0 and float(np.float32(chi2[0])) == 50.0 and not P.outliers(ident)[0]
    # and through the core
    Xs, obs, _, _, _ = po.planted_constraints(40, 1.0, seed=9)
    ref = po.frame_optimize(Xs, obs)
    c2 = po._Problem(Xs, obs, po.CAM_EUROC, None, po.THR_EUROC).errors(list(ref["Rt"]))[3]
    cand = [i for i in range(40) if float(np.float32(c2[i])) < c2[i]]
    assert cand
    seen = False
    for i in cand:
        thr = (float(np.float32(c2[i])), 75.0)
        r, rr = run_core(core, Xs, obs, thr=thr), po.frame_optimize(Xs, obs, thr=thr)
        _assert_same(r, rr)
        ct = po._Problem(Xs, obs, po.CAM_EUROC, None, thr).errors(list(rr["Rt"]))[3]
        by_float = ~(ct.astype(np.float32).astype(np.float64) > thr[0])
        by_double = ~(ct > thr[0])
        assert (r["inlier"].astype(bool) == by_float).all()
        if by_float[i] and not by_double[i]:           # (the other threshold moves the pose a little: the edge may have left the boundary)
            seen = True
            break
    assert seen, "no edge ended on the float / double boundary"


def test_degenerate_input_gives_the_defined_result(core):
    X, obs, _, _, _ = po.planted_constraints(50, 0.8, seed=2, stereo=True)
    # n = 0: the start pose, 0
    T0 = np.eye(4)
    T0[:3, 3] = (0.1, 0.2, 0.3)
    r = run_core(core, X[:0], obs[:0], Twc0=T0)
    _assert_same(r, po.frame_optimize(X[:0], obs[:0], Twc0=T0.reshape(16)))
    assert r["num_inliers"] == 0 and r["rounds"] == 0 and r["Twc"].tobytes() == T0.tobytes()
    # all points behind the camera, and all with z == 0
    for Xd in (X * np.array([1.0, 1.0, -1.0]), X * np.array([1.0, 1.0, 0.0])):
        r = run_core(core, Xd, obs)
        _assert_same(r, po.frame_optimize(Xd, obs))
        assert np.isfinite(r["Twc"]).all() and np.isfinite(r["Rt"]).all() and 0 <= r["num_inliers"] <= 50
    # all constraints identical
    Xi, oi = np.repeat(X[:1], 40, 0), np.repeat(obs[:1], 40, 0)
    r = run_core(core, Xi, oi)
    _assert_same(r, po.frame_optimize(Xi, oi))
    assert np.isfinite(r["Twc"]).all() and np.isfinite(r["Rt"]).all()
    # a start pose with NaN: the start pose comes back, every flag 0, count 0
    Tn = np.eye(4)
    Tn[0, 3] = np.nan
    r = run_core(core, X, obs, Twc0=Tn)
    _assert_same(r, po.frame_optimize(X, obs, Twc0=Tn.reshape(16)))
    assert r["Twc"].tobytes() == Tn.tobytes() and r["num_inliers"] == 0 and not r["inlier"].any()


@pytest.mark.parametrize("n,ratio,stereo", [(30, 0.8, False), (100, 0.5, True), (300, 1.0, False), (1000, 0.8, True)])
def test_round_one_does_not_increase_the_robust_chi(core, n, ratio, stereo):
    X, obs, _, _, _ = po.planted_constraints(n, ratio, seed=77 + n, stereo=stereo)
    r = run_core(core, X, obs)
    assert r["trace"][0, 1] <= r["trace"][0, 0] and r["trace"][0, 0] > 0
    # the start value is the robust chi of the restatement at the start pose over every edge
    P = po._Problem(X, obs, po.CAM_EUROC, None, po.THR_EUROC)
    ident = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    assert P.chi(ident, np.zeros(n, bool)) == r["trace"][0, 0]


def test_seed_rule(core):
    Tp, Tl = np.eye(4), np.eye(4)
    Tp[:3, 3] = (0.6, 0.6, 0.6)
    for count, lost, want in ((100, 50, 1), (100, 100, 1), (100, 101, 1)):
        assert core.core_use_last(Tp.ctypes.data, count, Tl.ctypes.data, lost) == want == int(po.use_last(Tp, count, Tl, lost))       # 1.04 m
    Tp[:3, 3] = (0.5, 0.5, 0.5)
    for count, lost, want in ((100, 50, 0), (50, 50, 0), (49, 50, 1)):
        assert core.core_use_last(Tp.ctypes.data, count, Tl.ctypes.data, lost) == want == int(po.use_last(Tp, count, Tl, lost))


def test_new_kernels_use_no_scratch():
    from test_no_scratch_cpu import _usage
    u = _usage("kernels_poseopt.hip")
    names = [n for n in u if "poseopt_" in n]
    assert len(names) == 2, names
    for n in names:
        assert u[n].get("ScratchSize [bytes/lane]", 0) == 0 and u[n].get("VGPRs Spill", 0) == 0, (n, u[n])
