"""The PLNet stage-0 decode between the line head and the stage-0 tensors (kernels_s0.hip), one launcher at a time on hand-built head rows and line features
(tests/s0_decode_ref.py: float64 reference, derived per-element envelope, cases; their properties are proved in tests/test_s0_decode_ref_cpu.py).  airfe_debug_s0_decode
stages the input into the context's own buffers and runs the launcher production runs (include/airfe_debug.h); every output buffer is 0xFF bytes when the launches start
and comes back whole.

rows mode (launch_s0_decode, both production layouts, B = 1 and 2): lines_pred / jloc / joff inside the envelope at EVERY element, `pole` equal to the float32 restatement,
`saturated_sigmoid`'s jloc / joff equal to their exact values; thin / aux / ta8 / loi / jnms bit-equal; poison wherever the contract writes nothing.
features mode (launch_s0_head_decode = production's fuse_dec = 1, and the two-pass form behind fuse_dec = 0): fused == two-pass == rows mode by bits, in fp16 and bf16, with
8 and 7 workgroups (32 passes per image; 28 waves over 1024 B tiles: a ragged last pass under the prefetch guard) as well as the default grid, on a one-hot head that
reproduces every case exactly and on the context's synthetic head over random features.

Measured on an MI355X (LAB_NOTES.md section 15; every run records them through diag(...)): worst share of an element's envelope 0.085 / 0.061 / 0.082 / 0.079 for
lines_pred on `benign` / `steep` / `clamps` / `copies`, 0.18 for jloc, 0.14 for joff; on `saturated_sigmoid` lines_pred reaches 1.000 at elements that rest on the clamp
(row 0: float64 6.7e-23 above 0, float32 4.4e-7 below it and clamped — the envelope's end is the clamp itself).  No element of any bounded case outside, `pole` and the
exact values equal, every copy and every pair of forms equal by bits; no kernel fix was needed."""
import os

import numpy as np
import pytest

import s0_decode_ref as R
from airslam_amd import api, synth, weights
from conftest import GOLDEN
from gpu_common import diag

pytestmark = pytest.mark.gpu
F = np.float32
LAYOUTS = ((160, 128), (32, 0))
PREC = {"bf16": 0, "fp16": 1}
_CTX, _RUNS, _SHARE = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for c in _CTX.values():
        c.close()
    _CTX.clear()
    _RUNS.clear()


def _ctx(fuse_dec=1):
    if fuse_dec not in _CTX:
        _CTX[fuse_dec] = api.Context(superpoint=weights.synthetic_plnet_s0(1234), plnet_s1=os.path.join(GOLDEN, "plnet_s1.airfe"), max_batch=2, enc_chunk=2, check_launches=1,
                                     tuning=None if fuse_dec else {"fuse_dec": 0})
    return _CTX[fuse_dec]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _poison(a):
    return _bits(a) == -1


def _rows_run(name, B, ld, off):
    key = ("rows", name, B, ld)
    if key not in _RUNS:
        _RUNS[key] = _ctx().debug_s0_decode(rows=R.rows_for(R.case(name)[:B], ld, off), ld=ld, off=off, ta8=True, loi=ld == 160, jnms=True)
    return _RUNS[key]


def _check_computed(r, name, B, what):
    """lines_pred, jloc, joff of a run on case `name` (images 0 .. B-1) against the reference at every element; records the share of the envelope"""
    ref, env, f32 = R.expected(name)
    got = {"lines": r["lines_pred"], "jloc": r["jloc"], "joff": r["joff"]}
    for k, g in got.items():
        assert not _poison(g).any(), f"{what} {k}: an element was not written"
        if name == "pole" and k == "lines":
            differ = int((_bits(g) != _bits(f32[k][:B])).sum())
            print(f"{what} lines_pred: {differ} elements differ from the float32 restatement; {int((g != ref[k][:B]).sum())} differ from float64 (which stays before the pole)")
            assert differ == 0
            continue
        err = np.abs(g.astype(np.float64) - ref[k][:B])
        e = env[k][:B]
        sh = np.divide(err, e, out=np.zeros_like(err), where=err > 0)
        share = float(sh.max())
        print(f"{what} {k}: max |device - float64| = {err.max():.3e}, worst share of the element's envelope = {share:.3f}, elements outside: {int((err > e).sum())}")
        _SHARE[f"{k}/{name}"] = max(_SHARE.get(f"{k}/{name}", 0.0), share)
        if k == "lines":                                       # a result resting on a clamp can sit AT its envelope's end (the clamp); the share of the others says more
            free = (g > 0) & (g < 127)
            _SHARE[f"lines_off_the_clamps/{name}"] = max(_SHARE.get(f"lines_off_the_clamps/{name}", 0.0), float(sh[free].max()) if free.any() else 0.0)
        assert np.isfinite(g).all() and (err <= e).all(), (what, k, int((err > e).sum()))
    if name == "saturated_sigmoid":                            # the exact values: float32(float64 reference) IS 0 / 1 and -0.5 / +0.5
        np.testing.assert_array_equal(got["jloc"], ref["jloc"][:B].astype(F))
        np.testing.assert_array_equal(got["joff"], ref["joff"][:B].astype(F))
        assert set(np.unique(got["jloc"])) == {0.0, 1.0} and set(np.unique(got["joff"])) == {-0.5, 0.5}
    diag("s0_decode_pin_envelope_share", **dict(sorted(_SHARE.items())))


def _check_stage_poison(r, written):
    """the stage blocks outside the tensors this form writes are still 0xFF"""
    mask = np.ones(r["stage"].shape[1], bool)
    for k in written:
        o, n = api.Context.S0_STAGE[k]
        mask[o:o + n] = False
    assert _poison(r["stage"][:, mask]).all(), "a stage-block region outside the written tensors was touched"
    for k in set(api.Context.S0_STAGE) - set(written):
        assert _poison(r[k]).all(), f"{k} was written"


# ---------------------------------------------------------------------------------------------------------------- rows mode against float64
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("ld,off", LAYOUTS, ids=["ld160", "ld32"])
@pytest.mark.parametrize("name", R.CASES)
def test_rows_mode_against_float64(name, ld, off, B):
    r = _rows_run(name, B, ld, off)
    _check_computed(r, name, B, f"{name} rows ld {ld} B {B}")
    cp = R.expected_copies(R.case(name)[:B])
    for k in ("thin", "aux", "ta8"):
        np.testing.assert_array_equal(_bits(r[k]), _bits(cp[k]), err_msg=k)
    if ld == 160:
        np.testing.assert_array_equal(_bits(r["loi"]), _bits(cp["loi"]), err_msg="loi (CHW, image 0)")
    else:
        assert _poison(r["loi"]).all()
    np.testing.assert_array_equal(_bits(r["jnms"]), _bits(R.jnms_ref(r["jloc"])), err_msg="jnms of the device's own jloc")
    if name == "copies":                                       # five logit levels -> five values: the plateaus and ties are exact on the device too
        kept = r["jnms"] > 0
        print(f"{name}: {len(np.unique(r['jloc']))} distinct jloc values, {int(kept.sum())} of {kept.size} pixels survive")
        assert len(np.unique(r["jloc"])) == 5 and np.array_equal(kept, R.jnms_ref(R.expected(name)[2]["jloc"][:B]) > 0)
    _check_stage_poison(r, ("lines_pred", "thin", "aux"))


def test_rows_mode_layouts_agree_and_optional_outputs_stay_poison():
    """both layouts give the same bytes; with ta8 / loi / jnms off, their buffers keep the poison and nothing else changes"""
    a, b = _rows_run("benign", 2, 160, 128), _rows_run("benign", 2, 32, 0)
    for k in ("stage", "jloc", "joff", "jnms", "ta8"):
        np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=k)
    off = _ctx().debug_s0_decode(rows=R.rows_for(R.case("benign"), 160, 128), ld=160, off=128, ta8=False, loi=False, jnms=False)
    for k in ("ta8", "loi", "jnms"):
        assert _poison(off[k]).all(), k
    for k in ("stage", "jloc", "joff"):
        np.testing.assert_array_equal(_bits(off[k]), _bits(a[k]), err_msg=k)


# ---------------------------------------------------------------------------------------------------------------- features mode: fused == two-pass == rows mode
def _synthetic_head():
    w = weights.synthetic_plnet_s0(1234)
    return w["line.head.weight"][128:145].astype(F), w["line.head.bias"][128:145].astype(F)


def _feature_input(kind, name, B):
    key = ("x", kind, name, B)
    if key not in _RUNS:
        if kind == "one_hot":
            _RUNS[key] = R.features_for(R.case(name)[:B])
        else:
            _RUNS[key] = ((np.random.default_rng(77).standard_normal((B * R.NPX, 128)) * 0.5).astype(F), *_synthetic_head())
    return _RUNS[key]


def _two_pass(kind, name, B, prec):
    """the two-pass form and rows mode on the head rows it returned (neither depends on the grid): cached"""
    key = ("two", kind, name, B, prec)
    if key not in _RUNS:
        x, w, b = _feature_input(kind, name, B)
        two = _ctx().debug_s0_decode(x=x, w=w, b=b, prec=prec, two_pass=True)
        rows = _ctx().debug_s0_decode(rows=two["head_rows"], ld=32, off=0, ta8=True, loi=False, jnms=True)
        _RUNS[key] = (two, rows)
    return _RUNS[key]


@pytest.mark.parametrize("wgs", [0, 8, 7])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("prec", list(PREC), ids=list(PREC))
@pytest.mark.parametrize("kind", ["one_hot", "synthetic"])
def test_features_mode_fused_two_pass_and_rows_agree(kind, prec, B, wgs):
    for name in (R.CASES if kind == "one_hot" else ("random",)):
        what = f"{name} {kind} {prec} B {B} wgs {wgs}"
        x, w, b = _feature_input(kind, name, B)
        fused = _ctx().debug_s0_decode(x=x, w=w, b=b, prec=PREC[prec], wgs=wgs)
        two, rows = _two_pass(kind, name, B, PREC[prec])
        for k in ("lines_pred", "jloc", "joff", "jnms", "ta8"):
            assert not _poison(fused[k]).any(), f"{what}: {k} has elements the fused kernel did not write"
            np.testing.assert_array_equal(_bits(fused[k]), _bits(two[k]), err_msg=f"{what}: fused against two-pass, {k}")
        for k in ("stage", "jloc", "joff", "jnms", "ta8"):
            np.testing.assert_array_equal(_bits(two[k]), _bits(rows[k]), err_msg=f"{what}: two-pass against rows mode on its own head rows, {k}")
        _check_stage_poison(fused, ("lines_pred",))             # (the fused form does not write the CHW planes)
        _check_stage_poison(two, ("lines_pred", "thin", "aux"))
        assert _poison(fused["loi"]).all() and _poison(two["loi"]).all()
        if kind == "one_hot":                                  # the head rows are exact: the case's reference applies to the fused kernel directly
            np.testing.assert_array_equal(two["head_rows"][:, :, :17], R.rows_for(R.case(name)[:B], 32, 0)[:, :, :17], err_msg=f"{what}: the one-hot head rows")
            _check_computed(fused, name, B, what)
            cp = R.expected_copies(R.case(name)[:B])
            np.testing.assert_array_equal(_bits(fused["ta8"]), _bits(cp["ta8"]), err_msg=f"{what}: ta8")
            np.testing.assert_array_equal(_bits(two["thin"]), _bits(cp["thin"]))
            np.testing.assert_array_equal(_bits(two["aux"]), _bits(cp["aux"]))
            np.testing.assert_array_equal(_bits(fused["jnms"]), _bits(R.jnms_ref(fused["jloc"])))
        else:
            assert np.isfinite(two["head_rows"][:, :, :17]).all() and float(np.abs(two["head_rows"][:, :, :17]).std()) > 0.05


# ---------------------------------------------------------------------------------------------------------------- fuse_dec = 0 end to end
def test_fuse_dec_0_gives_the_default_paths_bytes_end_to_end():
    for seed in (0, 1):
        img = synth.stereo_pair(480, 752, seed)[0]
        a = _ctx(1).detect_plnet(img, None, want_junctions=True)
        b = _ctx(0).detect_plnet(img, None, want_junctions=True)
        print(f"image {seed}: {len(a[0])} keypoints, {len(a[1])} lines, {len(a[2])} junctions (fuse_dec = 1) / {len(b[0])}, {len(b[1])}, {len(b[2])} (fuse_dec = 0)")
        assert len(a[1]) >= 50 and len(a[2]) >= 20
        for x, y, k in zip(a, b, ("features", "lines", "junctions")):
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), f"image {seed}: {k} differ between fuse_dec = 1 and 0"


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_context_usable():
    ctx = _ctx()
    rows = R.rows_for(R.case("benign")[:1], 32, 0)
    x, w, b = R.features_for(R.case("benign")[:1])
    with pytest.raises(api.AirfeError, match="arena"):
        ctx.debug_s0_decode(rows=np.zeros((3, R.NPX, 32), F), ld=32, off=0)          # (max_batch = 2)
    with pytest.raises(api.AirfeError, match="layouts"):
        ctx.debug_s0_decode(rows=np.zeros((1, R.NPX, 64), F), ld=64, off=0)
    with pytest.raises(api.AirfeError, match="loi"):
        ctx.debug_s0_decode(rows=rows, ld=32, off=0, loi=True)
    with pytest.raises(api.AirfeError, match="prec"):
        ctx.debug_s0_decode(x=x, w=w, b=b, prec=2)
    for wgs in (-1, 4097):
        with pytest.raises(api.AirfeError, match="wgs"):
            ctx.debug_s0_decode(x=x, w=w, b=b, wgs=wgs)
    r = ctx.debug_s0_decode(rows=rows, ld=32, off=0)
    np.testing.assert_array_equal(_bits(r["lines_pred"]), _bits(_rows_run("benign", 1, 32, 0)["lines_pred"]))
