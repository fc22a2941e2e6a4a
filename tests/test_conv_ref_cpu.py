"""tests/conv_ref.py without a GPU: an fp32 emulation of each conv form (torch float32 convolutions with the kernels' rounding points) stays inside the
derived bounds and the 0.1 signed-mean cap on every case the GPU tests run, and three planted defects in the emulation do not.  What
tests/test_gpu_conv_kernels.py compares with must itself be right, and neither tighter than correct fp32 arithmetic nor blind."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import conv_ref as cr

PRECS = pytest.mark.parametrize("prec", [1, 0], ids=["fp16", "bf16"])


def _f32(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))


def _store(t, prec, truncate=False):
    """fp32 tensor -> the 2-byte storage type and back (float64 numpy); truncate: towards zero instead of to nearest"""
    v = t.double().numpy()
    if not truncate:
        return cr.r2(v, prec)
    r = cr.r2(v, prec)
    over = np.abs(r) > np.abs(v)                               # rounded away from zero: one step back
    return np.where(over, r - np.sign(r) * cr.ulp2(np.abs(r) * (1 - 2.0 ** -12), prec), r)


def emulate(cid, inp, prec, halo_mask=True, round_a1=True, truncate=False):
    """the launch of case `cid` in float32: conv2d in fp32, storage roundings where the kernel has them"""
    c = cr.CASES[cid]
    if c["form"] == "fused":
        img16 = _f32(cr.r2(inp["img"], 1))[:, None]
        w16, b16 = _f32(cr.r2(inp["w1a"], 1)).reshape(64, 1, 3, 3), _f32(cr.r2(inp["b1a"], 1))
        # conv1a over the tile's halo as the kernel computes it: on the zero-bordered image, one pixel beyond the image on every side
        a1 = torch.relu(Fn.conv2d(Fn.pad(img16, (2, 2, 2, 2)), w16, b16))                  # [B, 64, H + 2, W + 2]
        if halo_mask:
            m = torch.zeros_like(a1)
            m[:, :, 1:-1, 1:-1] = 1
            a1 = a1 * m
        if round_a1:
            a1 = _f32(cr.r2(a1.double().numpy(), prec))
        y = torch.relu(Fn.conv2d(a1, _f32(inp["w"]), _f32(inp["b"])))
        y = Fn.max_pool2d(y, 2, 2)
    else:
        y = Fn.conv2d(_f32(inp["x"]), _f32(inp["w"]), _f32(inp["b"]), padding=1)
        if c["relu"]:
            y = torch.relu(y)
        if c["pool"]:
            y = Fn.max_pool2d(y, 2, 2)
    return _store(y, prec, truncate)


@pytest.fixture(scope="module")
def refs():
    cache = {}

    def get(cid, prec):
        if (cid, prec) not in cache:
            inp = cr.make_inputs(cid, prec)
            cache[cid, prec] = (inp,) + cr.reference(cid, inp, prec)
        return cache[cid, prec]
    return get


@PRECS
@pytest.mark.parametrize("cid", list(cr.CASES))
def test_fp32_emulation_is_inside_the_bounds(cid, prec, refs):
    inp, ref, bound = refs(cid, prec)
    info = cr.check(f"{cid}", emulate(cid, inp, prec), ref, bound)
    print(cid, prec, {k: info[k] for k in ("worst_ratio", "mean_err", "mean_err_towards_ref", "bound_over_ref")})
    assert info["worst_ratio"] <= 1.0


@PRECS
def test_reference_matches_float32_torch(prec):
    """the plain reference is torch's own convolution: against the fp32 one without any storage rounding, to fp32 accuracy"""
    inp = cr.make_inputs("A", prec)
    ref = torch.relu(Fn.conv2d(_f32(inp["x"]).double(), _f32(inp["w"]).double(), _f32(inp["b"]).double(), padding=1)).numpy()
    got, bound = cr.plain(inp["x"], inp["w"], inp["b"], prec)
    assert np.all(np.abs(got - ref) <= 0.5 * cr.ulp2(ref, prec) + cr.EPS32 * np.abs(ref))          # (r2 rounds through fp32 first, as the kernels do)
    assert np.median(bound[ref > 0.1] / ref[ref > 0.1]) < 3 * 2.0 ** (-10 if prec else -7)          # not vacuous: a few ulps


@PRECS
@pytest.mark.parametrize("cid", ["F", "G"])
def test_fused_bound_is_not_vacuous(cid, prec, refs):
    """the fused form's extra term is zero where conv1a's value is away from a rounding boundary: the bound stays a few ulps of the output"""
    _, ref, bound = refs(cid, prec)
    big = ref > 0.1
    assert np.median(bound[big] / ref[big]) < 3 * 2.0 ** (-10 if prec else -7)


@PRECS
@pytest.mark.parametrize("defect", ["no_halo_mask", "a1_not_rounded", "truncated_output"])
def test_planted_defects_fail(defect, prec, refs):
    inp, ref, bound = refs("F", prec)
    kw = {"no_halo_mask": dict(halo_mask=False), "a1_not_rounded": dict(round_a1=False), "truncated_output": dict(truncate=True)}[defect]
    with pytest.raises(AssertionError):
        cr.check(defect, emulate("F", inp, prec, **kw), ref, bound)
    if defect == "no_halo_mask":                           # ... and it is the border outputs that move
        err = np.abs(emulate("F", inp, prec, **kw) - ref) > bound
        assert err[:, :, 1:-1, 1:-1].sum() == 0 and err.sum() > 100


@PRECS
def test_truncated_output_fails_the_plain_form_too(prec, refs):
    inp, ref, bound = refs("A", prec)
    with pytest.raises(AssertionError, match="systematic"):
        cr.check("trunc", emulate("A", inp, prec, truncate=True), ref, bound)
