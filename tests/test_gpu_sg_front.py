"""SuperGlue's front alone (airfe_debug_sg_front, include/airfe_debug.h: sg_front_dev, the statement superglue_dev and superglue_dev_f32 run) against the float64
reference and derived bounds of tests/sg_front_ref.py: sg_prepare_kernel in both instantiations and both 2-byte types, the two MFMA GEMMs behind the split form
(kenc.encoder.3 with ReLU, kenc.encoder.4 with the residual epilogue), the 128-row rounding with its two memsets, the slack-row reset, and the unsplit kernel under a
fp32 context.  tests/test_gpu_plnet_superglue.py reaches this code only behind up to 18 layers and 100 Sinkhorn iterations (gate 0.05) with kenc.encoder.4 scaled by
0.1; here the pack has no such gain (sg_front_ref.pack) and every stage is held on its own.  The hook starts every call with 0xFF bytes (NaN) in every row of x32, xb,
msg and hb and in lens, so "finite" means "written by this call".

cases (sg_front_ref.CASES): B = 1 and 2 with unequal lengths per side and pair; lengths 0, 1, 3, 4, 5, cap - 1 and cap (KE_LT = 4 keypoints per workgroup: full
groups, tails, a lone keypoint); cap < Np; Np = 400 with B = 1 (M = 800, Mg = 896: surplus rows); 753 x 481 (width // 2 != width / 2.0); scores and coordinates with
exact zeros, a negative coordinate, the origin and the far corner of the image.

Padding rows (len <= n < Np; the contract stated at sg_prepare_kernel and in DESIGN.md): unsplit exactly zero; split h128 exactly zero, hb = r2(relu(b3)), x32 the
constant row W4 relu(b3) + b4, every such row the same bits.  Later stages mask by lens."""
import ctypes as C

import numpy as np
import pytest

import sg_front_ref as R
from airslam_amd import _lib, api, weights
from gpu_common import diag
from oracle import ref_post

pytestmark = pytest.mark.gpu
PRECS = pytest.mark.parametrize("prec", [1, 0], ids=["fp16", "bf16"])
FORMS = pytest.mark.parametrize("split", [1, 0], ids=["split", "unsplit"])
F = np.float32
W = R.pack()
_C, _OUT = {}, {}


def _ctx(key, mp):
    """one context per arena shape and matcher_precision (0 bf16, 1 fp16, 2 fp32 as tests/test_gpu_fp32.py sets it), cached for the module"""
    if (key, mp) not in _C:
        kw = dict(precision=2) if mp == 2 else {}
        _C[(key, mp)] = api.Context(superglue=W, matcher=1, matcher_precision=mp, **R.CONTEXTS[key], **kw)
    return _C[(key, mp)]


def _call(key, mp, f0, f1, n0, n1, prec, split, norm):
    """one hook call; what holds for EVERY call is asserted here: lens are the inputs, nothing past `rows` was touched, every output is finite"""
    out = _ctx(key, mp).debug_sg_front(f0, f1, n0, n1, prec, split, normalize=norm)
    assert np.array_equal(out["lens"], [n for b in range(len(n0)) for n in (n0[b], n1[b])]), out["lens"]
    assert out["rows_past"] == 0
    for k in ("x32", "xb", "h128", "hb"):
        assert k not in out or np.isfinite(out[k]).all(), (k, int((~np.isfinite(out[k])).sum()))
    return out


def _case(name, prec, split, mp=None):
    k = (name, prec, split, mp)
    if k not in _OUT:
        key, f0, f1, n0, n1, norm, _, _ = R.case_inputs(name)
        _OUT[k] = _call(key, prec if mp is None else mp, f0, f1, n0, n1, prec, split, norm)
    return _OUT[k]


def _ref(name):
    k = ("ref", name)
    if k not in _OUT:
        key, f0, f1, n0, n1, norm, w, h = R.case_inputs(name)
        _OUT[k] = R.front(W, f0, f1, n0, n1, _ctx(key, 1).np_rows, norm, w, h)
    return _OUT[k]


def _zero_bits(a):
    return not np.ascontiguousarray(a, F).view(np.uint32).any()


def _check_unsplit(tag, out, ref, prec):
    v, M = ref["valid"], out["M"]
    info = R.check(tag + "_x32", out["x32"][:M][v], ref["x"][v], ref["ex"][v], diag=diag)
    assert R.same_bits(out["xb"], R.r2(out["x32"], prec).astype(F)), "xb must be the device's own x32 rounded to the 2-byte type"
    assert _zero_bits(out["x32"][:M][~v]) and _zero_bits(out["xb"][:M][~v]), "unsplit padding rows are exactly zero"
    assert _zero_bits(out["x32"][M:]) and _zero_bits(out["xb"][M:]), "the rows of the 128-row rounding stay as the slack-row reset left them"
    return info


def _check_split(tag, out, ref, prec):
    v, M = ref["valid"], out["M"]
    hr, hd = R.split_h128(ref, prec)
    R.check(tag + "_h128", out["h128"][:M][v], hr[v], hd[v], diag=diag)
    assert _zero_bits(out["h128"][:M][~v]) and _zero_bits(out["h128"][M:]), "split padding and surplus rows of h128 are exactly zero"
    hb, dhb = R.split_hb(W, out["h128"], prec)
    R.check(tag + "_hb", out["hb"], hb, dhb, diag=diag)
    x_in = np.zeros_like(out["x32"], dtype=np.float64)
    x_in[:M] = ref["desc"]
    x, dx = R.split_x32(W, x_in, out["hb"], prec)
    info = R.check(tag + "_x32", out["x32"], x, dx, diag=diag)
    assert R.same_bits(out["xb"], R.r2(out["x32"], prec).astype(F)), "xb must be the device's own x32 rounded to the 2-byte type"
    # padding rows: the constant row, every one the same bits (a sequence of length 0 is 64 such rows)
    hb_pad, x_pad, d_pad = R.split_padding_row(W, prec)
    pad = np.flatnonzero(~v)
    if pad.size:
        assert (out["hb"][:M][pad] == hb_pad).all(), "hb of a padding row is r2(relu(b3)) exactly"
        assert np.all(np.abs(out["x32"][:M][pad] - x_pad) <= d_pad)
        for k in ("x32", "xb", "hb"):
            assert (out[k][:M][pad] == out[k][pad[0]]).all(), (k, "padding rows differ from one another")
    return info


@PRECS
@FORMS
@pytest.mark.parametrize("name", list(R.CASES))
def test_front_vs_float64(name, split, prec):
    """every stage within its derived bound, kernel_ref.check's signed-mean condition included; xb bit for bit; lens; padding rows; nothing past the rows"""
    out, ref = _case(name, prec, split), _ref(name)
    tag = f"sgfront_{name}_{'split' if split else 'unsplit'}_{'fp16' if prec else 'bf16'}"
    info = (_check_split if split else _check_unsplit)(tag, out, ref, prec)
    assert info["worst_ratio"] <= 1.0


@pytest.mark.parametrize("name", ["b2_tails", "b2_full_and_empty", "b2_cap40", "b1_np400_surplus", "b2_odd_size"])
def test_unsplit_under_a_fp32_context(name):
    """superglue_dev_f32's front: the unsplit kernel with the fp16 shadow production asks for; x32 is what the fp32 GNN reads"""
    out = _case(name, 1, 0, mp=2)
    _check_unsplit(f"sgfront_{name}_unsplit_fp32ctx", out, _ref(name), 1)
    assert R.same_bits(out["x32"], _case(name, 1, 0)["x32"])          # the same instantiation as the fp16 context's: the same bits


@PRECS
@FORMS
@pytest.mark.parametrize("key", ["np64", "odd"])
def test_device_normalisation_gives_the_bits_of_the_reference_normalisation(key, split, prec):
    """normalize = 1 on raw pixel rows == normalize = 0 on oracle/ref_post.normalize_keypoints rows (integer width // 2, scale 0.7), at 752 x 480 and 753 x 481"""
    c = R.CONTEXTS[key]
    w, h = c["image_width"], c["image_height"]
    f0, f1 = R.features(7, 2, 64, w, h, True), R.features(8, 2, 64, w, h, True)
    g0, g1 = (np.stack([ref_post.normalize_keypoints(f[b], w, h, R.SCALE) for b in range(2)]) for f in (f0, f1))
    n0, n1 = [64, 5], [33, 63]
    a, b = _call(key, prec, f0, f1, n0, n1, prec, split, 1), _call(key, prec, g0, g1, n0, n1, prec, split, 0)
    for k in ("x32", "xb", "h128", "hb"):
        assert k not in a or R.same_bits(a[k], b[k]), k


@PRECS
@pytest.mark.parametrize("name", ["b2_full_and_empty", "b1_np400_surplus", "b1_np400_cap100"])
def test_two_split_calls_return_the_same_bytes(name, prec):
    """no running sum through the residual epilogue: padding rows, the rows of an empty sequence and the surplus rows [M, Mg) (Np = 400, B = 1: 800 .. 895)
    are finite (_call) and the same bytes in two consecutive calls"""
    key, f0, f1, n0, n1, norm, _, _ = R.case_inputs(name)
    a = _case(name, prec, 1)
    b = _call(key, prec, f0, f1, n0, n1, prec, 1, norm)
    if key == "np400":
        assert a["x32"].shape[0] == 896 and a["M"] == 800
    for k in ("x32", "xb", "h128", "hb"):
        assert R.same_bits(a[k], b[k]), k


@PRECS
@FORMS
@pytest.mark.parametrize("name", ["b2_tails", "b2_full_and_empty", "b2_cap40", "b2_odd_size"])
def test_pairs_of_a_batch_are_their_single_launches_bit_for_bit(name, split, prec):
    key, f0, f1, n0, n1, norm, _, _ = R.case_inputs(name)
    both, Np = _case(name, prec, split), _ctx(key, prec).np_rows
    for b in range(2):
        one = _call(key, prec, f0[b:b + 1], f1[b:b + 1], n0[b:b + 1], n1[b:b + 1], prec, split, norm)
        for side, n in enumerate((n0[b], n1[b])):
            for k in ("x32", "xb", "h128", "hb"):
                if k in both:
                    assert R.same_bits(both[k][(2 * b + side) * Np:][:n], one[k][side * Np:][:n]), (b, side, k)


def _raw_args(f0, f1, n0, n1, prec, split, rows):
    keep = [np.ascontiguousarray(f0, F), np.ascontiguousarray(f1, F), np.ascontiguousarray(n0, np.int32), np.ascontiguousarray(n1, np.int32), np.empty(2 * len(n0), np.int32),
            np.empty((rows, 256), F), np.empty((rows, 256), F), np.empty((rows, 128), F), np.empty((rows, 256), F)]
    a = _lib.DebugSgFrontArgs(prec=prec, split=split, B=len(n0), cap=f0.shape[1], normalize=0, rows=rows,
                              **{k: v.ctypes.data for k, v in zip(("f0", "f1", "n0", "n1", "lens", "x32", "xb", "h128", "hb"), keep)})
    return a, keep


def test_hook_refuses_bad_arguments_and_the_context_stays_usable():
    key, f0, f1, n0, n1, norm, _, _ = R.case_inputs("b2_tails")
    ctx, good = _ctx(key, 1), _case("b2_tails", 1, 1)

    def still_good():
        again = _call(key, 1, f0, f1, n0, n1, 1, 1, norm)
        assert all(R.same_bits(good[k], again[k]) for k in ("x32", "xb", "h128", "hb"))
    wide = np.zeros((2, 80, 259), F)
    three = np.zeros((3, 64, 259), F)
    for what, call in {
        "n > cap": lambda: ctx.debug_sg_front(f0, f1, [65, 4], n1, 1, 1),
        "n < 0": lambda: ctx.debug_sg_front(f0, f1, n0, [3, -1], 1, 0),
        "cap > Np": lambda: ctx.debug_sg_front(wide, wide, n0, n1, 1, 1),
        "B > max_batch": lambda: ctx.debug_sg_front(three, three, [1, 1, 1], [1, 1, 1], 1, 1),
        "prec 2": lambda: ctx.debug_sg_front(f0, f1, n0, n1, 2, 0),
        "prec -1": lambda: ctx.debug_sg_front(f0, f1, n0, n1, -1, 1),
        "prec of the other type": lambda: ctx.debug_sg_front(f0, f1, n0, n1, 0, 1),
        "split 2": lambda: ctx.debug_sg_front(f0, f1, n0, n1, 1, 2),
    }.items():
        with pytest.raises(api.AirfeError):
            call()
        still_good()
    for null in ("f0", "f1", "n0", "n1", "lens", "x32", "xb", "h128", "hb"):
        a, keep = _raw_args(f0, f1, n0, n1, 1, 1, good["x32"].shape[0])
        setattr(a, null, None)
        assert ctx._l.airfe_debug_sg_front(ctx._h, C.byref(a)) != 0, null
        assert b"null" in ctx._l.airfe_last_error(ctx._h), null
    assert ctx._l.airfe_debug_sg_front(ctx._h, None) != 0
    a, keep = _raw_args(f0, f1, n0, n1, 1, 1, good["x32"].shape[0] + 128)          # rows that are not the call's Mg
    assert ctx._l.airfe_debug_sg_front(ctx._h, C.byref(a)) != 0
    still_good()
    f32 = _ctx(key, 2)
    with pytest.raises(api.AirfeError):
        f32.debug_sg_front(f0, f1, n0, n1, 1, 1)                       # the split form does not exist under a fp32 context
    with pytest.raises(api.AirfeError):
        f32.debug_sg_front(f0, f1, n0, n1, 0, 0)                       # ... and its shadow is fp16
    assert R.same_bits(_call(key, 2, f0, f1, n0, n1, 1, 0, norm)["x32"], _case("b2_tails", 1, 0)["x32"])
    lg = api.Context(lightglue=weights.synthetic_lightglue(1234, n_layers=1), max_keypoints=64, max_batch=2)
    with pytest.raises(api.AirfeError):
        lg.debug_sg_front(f0, f1, n0, n1, 1, 0)
    assert lg.lightglue_scores(np.ascontiguousarray(f0[0, :5, 1:]), np.ascontiguousarray(f1[0, :5, 1:])).shape == (5, 5)
    lg.close()
