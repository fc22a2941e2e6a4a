"""Stereo line triangulation on the CPU (include/airfe.h "Stereo lines"): the host statement stereoline_host (airslam_amd/csrc/stereoline_core.h, compiled
here with the host compiler) against the Python restatement (tests/stereoline_ref.py) and against cases worked out by hand, byte for byte; the constant
that replaces the reference's atan; the seeded pairs' coverage; the library's new symbols; the new kernel's resource usage."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import stereoline_ref as sr
from conftest import ROOT

CSRC = os.path.join(ROOT, "airslam_amd", "csrc")
SHIM = r'''
#include "stereoline_core.h"
extern "C" void core_frame(const double* cam, const double* lines_left, int nl, const double* lines_right, int nr, const int32_t* matches, const double* Twc,
                           double* sel, uint8_t* flag, int32_t* status, double* endpoints, double* plucker, int32_t* count) {
  stereoline_host(cam, lines_left, nl, lines_right, nr, matches, Twc, sel, flag, status, endpoints, plucker, count);
}
extern "C" double core_tan_gate() { return SL_TAN_GATE; }
extern "C" void core_horizontal(const double* dx, const double* dy, int n, uint8_t* out) {
  for (int i = 0; i < n; ++i) out[i] = sl_horizontal(dx[i], dy[i]) ? 1 : 0;
}
'''
KEYS = ("lines_right_sel", "right_valid", "status", "endpoints", "plucker", "count")


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    """stereoline_core.h as this tree has it, compiled for the host without contraction"""
    d = tmp_path_factory.mktemp("stereoline_core")
    src, so = d / "core.cpp", str(d / "libstereolinecore.so")
    src.write_text(SHIM)
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-w", "-fPIC", "-shared", "-I" + CSRC, str(src), "-o", so], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(so)
    lib.core_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 8
    lib.core_frame.restype = None
    lib.core_tan_gate.restype = C.c_double
    lib.core_horizontal.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.core_horizontal.restype = None
    return lib


def run_core(lib, cam, left, nl, right, nr, matches, Twc=None, slots=None):
    """the host statement on buffers of `slots` line slots filled with a sentinel: -> (outputs cut to nl rows, whether everything behind them is untouched)"""
    cam = np.ascontiguousarray(cam, np.float64)
    left, right = np.ascontiguousarray(left, np.float64), np.ascontiguousarray(right, np.float64)
    matches = np.ascontiguousarray(matches, np.int32)
    twc = None if Twc is None else np.ascontiguousarray(Twc, np.float64).reshape(16)
    m = max(slots or nl, 1)
    sel, flag, status = np.full((m, 4), -7.0), np.full(m, 77, np.uint8), np.full(m, -7, np.int32)
    ends, plk, count = np.full((m, 6), -7.0), np.full((m, 6), -7.0), np.full(3, -7, np.int32)
    lib.core_frame(cam.ctypes.data, left.ctypes.data, nl, right.ctypes.data, nr, matches.ctypes.data, None if twc is None else twc.ctypes.data, sel.ctypes.data,
                   flag.ctypes.data, status.ctypes.data, ends.ctypes.data, plk.ctypes.data, count.ctypes.data)
    clean = (sel[nl:] == -7.0).all() and (flag[nl:] == 77).all() and (status[nl:] == -7).all() and (ends[nl:] == -7.0).all() and (plk[nl:] == -7.0).all()
    return dict(lines_right_sel=sel[:nl], right_valid=flag[:nl], status=status[:nl], endpoints=ends[:nl], plucker=plk[:nl], count=count), bool(clean)


def same_bytes(got, want):
    """every output equal byte for byte (NaN payloads and the sign of zero included)"""
    for k in KEYS:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if g.dtype != w.dtype or g.shape != w.shape or g.tobytes() != w.tobytes():
            return False
    return True


# ---- the hand cases -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sr.hand_lines() + sr.extra_lines(), ids=lambda c: c[0])
@pytest.mark.parametrize("pose", [None, sr.T0], ids=["camera", "T0"])
def test_single_pairs(core, case, pose):
    name, left, right, status = case
    lines_right = np.array([right, right])                          # the partner is right line 1: right line 0 is never taken
    match = [0] if name == "right_zero" else [1]
    ref = sr.frame(sr.CAM, [left], 1, lines_right, 2, match, pose)
    got, clean = run_core(core, sr.CAM, [left], 1, lines_right, 2, match, pose, slots=3)
    assert int(ref["status"][0]) == status, (name, ref["status"])    # written down by hand in stereoline_ref
    assert same_bytes(got, ref) and clean, (name, got, ref)
    set_e, set_p = status in (sr.OK, sr.SHORT), status == sr.OK
    assert np.isfinite(got["endpoints"]).all() == set_e and np.isnan(got["endpoints"]).all() == (not set_e)
    assert np.isfinite(got["plucker"]).all() == set_p and np.isnan(got["plucker"]).all() == (not set_p)
    assert got["count"].tolist() == [int(status != sr.NO_RIGHT), int(set_e), int(set_p)]
    if status == sr.NO_RIGHT:
        assert not got["lines_right_sel"].any() and got["right_valid"][0] == 0
    else:
        assert got["lines_right_sel"][0].tolist() == list(right) and got["right_valid"][0] == 1


def test_vertical_min_equals_the_numbers_worked_out_on_paper(core):
    _, left, right, _ = sr.hand_lines()[0]
    for pose, (ends, plk) in ((sr.T0, sr.VERTICAL_MIN_T0), (None, sr.VERTICAL_MIN_CAM)):
        for out in (sr.frame(sr.CAM, [left], 1, [right, right], 2, [1], pose), run_core(core, sr.CAM, [left], 1, [right, right], 2, [1], pose)[0]):
            assert out["status"][0] == sr.OK
            assert out["endpoints"][0].tolist() == list(ends) and out["plucker"][0].tolist() == list(plk)


def test_short_pairs_sit_just_under_and_just_over_the_length_gate():
    lens = {}
    for name, left, right, _ in sr.hand_lines():
        if name.startswith("short_"):
            e = sr.frame(sr.CAM, [left], 1, [right, right], 2, [1])["endpoints"][0]
            lens[name] = math.sqrt(sum((e[3 + k] - e[k]) ** 2 for k in range(3)))
    assert 0.00999 < lens["short_under"] < 0.01 < lens["short_over"] < 0.01001, lens


def test_hand_frames(core):
    frames = sr.hand_frames()
    seen = set()
    for f in frames:
        for pose in (f["Twc"], None):
            ref = sr.frame(sr.CAM, f["left"], f["nl"], f["right"], f["nr"], f["matches"], pose)
            got, clean = run_core(core, sr.CAM, f["left"], f["nl"], f["right"], f["nr"], f["matches"], pose, slots=8)
            assert ref["status"].tolist() == f["status"]
            assert same_bytes(got, ref) and clean
        seen |= set(f["status"])
    assert seen == set(range(6))                                    # every status at least once
    assert frames[1]["nr"] == 1 and frames[2]["nl"] == 0
    assert sr.frame(sr.CAM, frames[0]["left"], 8, frames[0]["right"], 8, frames[0]["matches"], None)["count"].tolist() == [7, 4, 3]


# ---- the seeded pairs -----------------------------------------------------------------------------------------------------------------------------------
def test_seeded_pairs_reach_every_branch():
    """by the restatement alone: no GPU test can pass on an input that exercises one branch only"""
    counts = sr.reference_counts()
    assert counts.sum() == 4096 and (counts >= 100).all() and counts[sr.OK] >= 1024, counts
    s = sr.seeded_pairs()
    m, nr = s["matches"], s["nr"][:, None]
    assert (m == 0).sum() >= 8 and (m == nr).sum() >= 8 and (m > nr).sum() >= 8 and (m < 0).sum() >= 8      # every way of having no right line


@pytest.mark.parametrize("with_pose", [True, False], ids=["Twc", "NULL"])
def test_seeded_pairs_core_equals_the_restatement(core, with_pose):
    s = sr.seeded_pairs()
    for b, ref in enumerate(sr.seeded_reference(with_pose)):
        got, clean = run_core(core, sr.CAM, s["left"][b], int(s["nl"][b]), s["right"][b], int(s["nr"][b]), s["matches"][b], s["Twc"][b] if with_pose else None)
        assert same_bytes(got, ref) and clean, b


def test_null_pose_equals_the_identity_up_to_the_sign_of_zero(core):
    """The contract promises for NULL the untouched camera-frame numbers; the identity pose adds (+0 * y) and + 0 terms, which can turn a -0 into +0 and
    nothing else: equal as VALUES everywhere, NaN in the same places."""
    s = sr.seeded_pairs()
    eye = np.eye(4).reshape(16)
    n_set = 0
    for b in range(sr.SEED_B):
        a = run_core(core, sr.CAM, s["left"][b], 512, s["right"][b], int(s["nr"][b]), s["matches"][b], None)[0]
        i = run_core(core, sr.CAM, s["left"][b], 512, s["right"][b], int(s["nr"][b]), s["matches"][b], eye)[0]
        for k in KEYS:
            assert np.array_equal(a[k], i[k], equal_nan=a[k].dtype == np.float64), (b, k)
        n_set += int(a["count"][1])
    assert n_set > 1024
    # ... and a case where the sign does differ: an end on the principal point's column has x = -0 or +0 in the camera frame
    left, right = (sr.CAM[6], 100.0, sr.CAM[6] - 64.0, 228.0), (sr.CAM[6] - 40.0, 100.0, sr.CAM[6] - 104.0, 228.0)
    a = run_core(core, sr.CAM, [left], 1, [right, right], 2, [1], None)[0]
    i = run_core(core, sr.CAM, [left], 1, [right, right], 2, [1], eye)[0]
    assert a["status"][0] == sr.OK and np.array_equal(a["endpoints"], i["endpoints"]) and a["endpoints"][0][0] == 0.0


def test_plucker_lines_are_normalised_and_orthogonal(core):
    s = sr.seeded_pairs()
    n = 0
    for b in range(sr.SEED_B):
        got = run_core(core, sr.CAM, s["left"][b], 512, s["right"][b], int(s["nr"][b]), s["matches"][b], s["Twc"][b])[0]
        p = got["plucker"][got["status"] == sr.OK]
        w, d = p[:, :3], p[:, 3:]
        assert (np.abs((w * d).sum(1)) <= 1e-12).all() and (np.abs(np.linalg.norm(d, axis=1) - 1.0) <= 1e-12).all()
        n += len(p)
    assert n >= 1024


def test_stand_alone_host_check_builds_and_passes(tmp_path):
    """tools/stereoline_host_check.cpp (exactly sized buffers; the program a sanitizer build runs) as a plain build: it compiles against this tree's core and
    every status, count and number written out in it holds"""
    exe = str(tmp_path / "stereoline_host_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I" + CSRC, os.path.join(ROOT, "tools", "stereoline_host_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "stereoline_host_check: ok" in r.stdout, r.stdout[-2000:]


# ---- the gate's constant --------------------------------------------------------------------------------------------------------------------------------
def _next(x, k):
    """the double k steps above the positive double x"""
    return float((np.array(x, np.float64).view(np.int64) + k).view(np.float64))


def test_tan_gate_is_the_smallest_double_whose_atan_reaches_0175(core):
    gate = core.core_tan_gate()
    lo, hi = 0.17, 0.18                                             # atan(lo) < 0.175 <= atan(hi)
    assert math.atan(lo) < 0.175 <= math.atan(hi)
    while _next(lo, 1) != hi:
        mid = lo + (hi - lo) / 2
        if math.atan(mid) >= 0.175:
            hi = mid
        else:
            lo = mid
    assert hi == gate == float.fromhex("0x1.6a1aa2e1bef6fp-3"), (hi.hex(), gate.hex())
    # 10 000 doubles on either side, both signs: the ratio form and the atan form decide alike
    t = np.array([_next(gate, k) for k in range(-10000, 10001)])
    dx = np.concatenate([np.ones_like(t), -np.ones_like(t)])       # dy / dx = +-t exactly
    dy = np.concatenate([t, t]) * 1024.0                            # ... and |dy| > 3, so that the slope decides
    dx = dx * 1024.0
    out = np.zeros(len(dx), np.uint8)
    core.core_horizontal(dx.ctypes.data, dy.ctypes.data, len(dx), out.ctypes.data)
    want = [sr.horizontal(float(a), float(b)) for a, b in zip(dx, dy)]
    assert out.tolist() == [int(v) for v in want]
    assert sum(want) == 20000 and not want[10000] and want[9999]    # below the gate horizontal, from the gate on not


def test_ratios_at_the_gate_decide_alike(core):
    """200 000 seeded dy / dx within 1e-15 (relative) of the gate"""
    rng = np.random.RandomState(5)
    gate = core.core_tan_gate()
    n = 200000
    dx = rng.uniform(30.0, 2000.0, n) * np.where(rng.rand(n) < 0.5, 1.0, -1.0)
    dy = dx * gate * (1.0 + rng.uniform(-1e-15, 1e-15, n)) * np.where(rng.rand(n) < 0.5, 1.0, -1.0)
    assert (np.abs(dy) > 3.0).all() and (np.abs(np.abs(dy / dx) / gate - 1.0) < 2e-15).all()
    out = np.zeros(n, np.uint8)
    core.core_horizontal(dx.ctypes.data, dy.ctypes.data, n, out.ctypes.data)
    want = np.array([sr.horizontal(a, b) for a, b in zip(dx.tolist(), dy.tolist())], np.uint8)
    assert np.array_equal(out, want)
    assert 0.1 * n < want.sum() < 0.9 * n                           # both decisions occur


# ---- the library and its kernel -------------------------------------------------------------------------------------------------------------------------
NEW = ("airfe_stereo_lines", "airfe_stereo_lines_batch_dev", "airfe_stereo_line_landmarks_batch_dev")


def test_library_exports_the_new_entries(libpath):
    lib = C.CDLL(libpath)
    from airslam_amd import _lib, api, build
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    for name in ("stereo_lines", "stereo_lines_batch_dev", "stereo_line_landmarks_batch_dev"):
        assert callable(getattr(api.Context, name)), name
    assert "kernels_stereoline.hip" in build.SOURCES and build.EXTRA_FLAGS["kernels_stereoline.hip"] == ["-ffp-contract=off"]


def test_new_kernel_uses_no_scratch_no_lds_and_does_not_spill():
    from airslam_amd import build
    src = "kernels_stereoline.hip"
    r = subprocess.run(["/opt/rocm/bin/hipcc"] + build.FLAGS + build.EXTRA_FLAGS.get(src, []) + ["-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        os.path.join(CSRC, src), "-o", os.devnull], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    sspill = [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", r.stderr)]
    vspill = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", r.stderr)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(names) == 1 and "stereoline_kernel" in names[0] and len(scratch) == len(sspill) == len(vspill) == len(lds) == 1, names
    assert scratch == [0] and sspill == [0] and vspill == [0] and lds == [0], (scratch, sspill, vspill, lds)
