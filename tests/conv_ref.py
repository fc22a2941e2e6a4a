"""fp64 references for the encoder's 3x3 convolution kernels (kernels_conv64r.hip, kernels_conv128r.hip, conv3x3_kernel of kernels_mm.hip), each with a
DERIVED per-element error bound, and the cases tests/test_gpu_conv_kernels.py and tests/test_conv_ref_cpu.py share.

Every reference takes inputs that are already rounded to the storage type, evaluates torch.nn.functional.conv2d in float64 on the CPU and rounds to the
storage type where the kernel stores.
  plain form   y = r2(pool(act(conv(x, w) + b))), act = ReLU or nothing.  Rounding and the 2x2 max-pool commute (both are monotonic), so one reference covers
               the kernels that pool packed 2-byte values and the one that pools in fp32.
  fused form   conv1a -> conv1b -> pool in one launch (ConvArgs::img).  The kernel's contract: image, w1a and b1a are converted to fp16 in BOTH storage modes
               (`(_Float16)` conversions feeding PF16::mfma), a1 = relu(conv(img16, w1a16) + b1a16) is stored in the storage type, and a1 is exactly 0 at the
               halo pixels outside the image (conv1b's zero padding), not relu(b1a).  Then the plain form with pool = 1.

A bound is the sum of
  1. one ulp of the stored output at |ref|;
  2. K EPS32 conv(|x|, |w|) + EPS32 |y| with K = 9 cin: the fp32 accumulation of a K-term sum of exact products, whatever its order, and the bias (both persistent
     kernels start their accumulators from the bias; conv3x3_kernel adds it last: one rounding either way);
  3. fused form only: conv(da1, |w1b|), da1 = the distance between the kernel's a1 and the reference's.  The kernel's pre-rounding value lies within
     d = 10 EPS32 (conv(|img|, |w1a|) + |b1a|) of the exact one (nine products and the bias on the fp16 MFMA, fp32 accumulation); rounding and ReLU are monotonic,
     so both a1 lie in [relu(r2(v - d)), relu(r2(v + d))]: da1 = the width of that interval, and never more than d + ulp2(a1).  It is ZERO wherever v is further
     than d from a rounding boundary — nearly everywhere — which is what lets the check see a conv1a output that was not rounded to storage at all.
A pooled element takes the maximum of its four bounds (|max a_i - max b_i| <= max |a_i - b_i|).  kernel_ref.check asserts the per-element bound and a signed
mean error below 0.1 of the mean bound.  tests/test_conv_ref_cpu.py shows, without a GPU, that correct fp32 arithmetic with the same rounding points stays inside
all of this for every case below, and that three planted defects do not.

Mutations applied to the kernels one at a time (scratch builds, never committed; every one changes values only, no address) and the first test of
tests/test_gpu_conv_kernels.py that failed on each:
  stage(next, i & 1) in conv64r (the next tile lands in the buffer being read)         test_wrapped_tile_loop_is_byte_equal[A-1-fp16]   (+ A-4, B-3, C-3; 8 tests)
  stage_tile(next, i & 1) in conv128r                                                   test_wrapped_tile_loop_is_byte_equal[D-1-fp16]   (+ D-5, E-3; 6 tests)
  pb1 advanced one step late (conv1a of tile i + 1 reads patch i)                       test_wrapped_tile_loop_is_byte_equal[F-1-fp16]   (+ F-2, F-4, G-5; not F-8: two rounds)
  the halo mask m forced to 1                                                           test_bound[F-fp16]                               (+ G; 4 tests)
  dpp_xor1 dropped from conv64r's pooled epilogue                                       test_bound[B-fp16]                               (+ F, G; 6 tests)
  dpp_xor1 dropped from conv128r's pooled epilogue                                      test_bound[E-fp16]                               (2 tests)
  tile_decode's shift path returning tx for ty, in tile_xy only (the halo mask's tile)  test_bound[G-fp16]                               (2 tests)
The last one is narrower than "tile_decode returns tx for ty": in stage / stage_patch / the epilogue that mutation moves global addresses (case B's tile grid is
4 x 2: rows past the image and past the output buffer), so it was applied only where the decode feeds values — the fused form's mask coordinates.  A wrong decode in
the other three places writes tiles to the wrong position: test_canary's "every interior word written" and test_bound see it by construction, without a mutant run.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as Fn

from kernel_ref import EPS32, check, r2, ulp2  # noqa: F401  (check: re-exported for the tests)

# id -> form, cin, cout, B, H, W, pool, out_pad, relu, the wgs values (256 = production's grid first; None: the kernel has no persistent grid)
CASES = {
    "A": dict(form="plain", cin=64, cout=64, B=1, H=48, W=80, pool=0, out_pad=1, relu=1, wgs=(256, 1, 4)),        # conv64r, 15 tiles: division decode
    "B": dict(form="plain", cin=64, cout=128, B=2, H=32, W=64, pool=1, out_pad=1, relu=1, wgs=(256, 3)),          # conv64r, two passes, 16 tiles: shift decode
    "C": dict(form="plain", cin=64, cout=64, B=1, H=32, W=32, pool=0, out_pad=0, relu=1, wgs=(256, 3)),           # conv64r, 4 tiles, no output border
    "D": dict(form="plain", cin=128, cout=128, B=1, H=32, W=48, pool=0, out_pad=0, relu=1, wgs=(256, 1, 5)),      # conv128r, 12 tiles: convPa / convDa / line conv
    "E": dict(form="plain", cin=128, cout=256, B=2, H=16, W=32, pool=1, out_pad=1, relu=1, wgs=(256, 3)),         # conv128r, two passes, 8 tiles
    "F": dict(form="fused", cin=64, cout=64, B=1, H=48, W=80, pool=1, out_pad=1, relu=1, wgs=(256, 1, 2, 4, 8)),  # fused conv1, 15 tiles: every prologue / ring / tail path
    "G": dict(form="fused", cin=64, cout=64, B=2, H=32, W=64, pool=1, out_pad=1, relu=1, wgs=(256, 5)),           # fused conv1, two images, 16 tiles
    "H": dict(form="plain", cin=64, cout=64, B=1, H=32, W=32, pool=1, out_pad=1, relu=0, wgs=(None,)),            # conv3x3_kernel: the only code that honours relu = 0
    "I": dict(form="plain", cin=128, cout=128, B=1, H=16, W=32, pool=0, out_pad=1, relu=0, wgs=(None,)),
}


def make_inputs(cid: str, prec: int) -> dict:
    """the test inputs of case `cid`, rounded to the storage type where the kernel's inputs are 2-byte (float32 arrays)"""
    c = CASES[cid]
    rng = np.random.default_rng(1000 + 2 * (ord(cid) - ord("A")) + prec)
    r = lambda t: r2(t, prec).astype(np.float32)
    cin, cout, B, H, W = c["cin"], c["cout"], c["B"], c["H"], c["W"]
    out = dict(w=r(rng.normal(size=(cout, cin, 3, 3)) / np.sqrt(9 * cin)), b=(rng.normal(size=cout) * 0.1).astype(np.float32))
    if c["form"] == "fused":
        out["img"] = (rng.integers(0, 256, size=(B, H, W)) / 255.0).astype(np.float32)          # what the pre-process emits: k / 255 in fp32
        out["w1a"] = (rng.normal(size=(64, 9)) / np.sqrt(3.0)).astype(np.float32)
        out["b1a"] = (rng.normal(size=64) * 0.5).astype(np.float32)           # large: a missing halo mask moves the border outputs by far more than the bound
    else:
        out["x"] = r(rng.normal(size=(B, cin, H, W)))
    return out


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))


def _conv(x, w, b=None):
    return Fn.conv2d(_t(x), _t(w), None if b is None else _t(b), padding=1).numpy()


def _pool(x):
    return Fn.max_pool2d(_t(x), 2, 2).numpy()


def plain(x, w, b, prec, pool=False, relu=True, dx=None):
    """fp64 reference and bound of one conv launch: x [B, cin, H, W], w [cout, cin, 3, 3], b [cout] -> (ref, bound) [B, cout, Ho, Wo].  dx: the input is known
    to +-dx only (the fused form's a1)."""
    x, w, b = (np.asarray(t, np.float64) for t in (x, w, b))
    y = _conv(x, w, b)
    acc = 9 * x.shape[1] * EPS32 * _conv(np.abs(x), np.abs(w)) + EPS32 * np.abs(y)
    if dx is not None:
        acc = acc + _conv(dx, np.abs(w))
    if relu:
        y = np.maximum(y, 0.0)
    bound = ulp2(r2(y, prec), prec) + acc
    if pool:
        y, bound = _pool(y), _pool(bound)
    return r2(y, prec), bound


def conv1a(img, w1a, b1a, prec):
    """the fused form's first layer: img [B, H, W] fp32, w1a [64, 9], b1a [64] -> (a1, da1) [B, 64, H, W] (see the header: fp16 operands in both modes)"""
    img16, w16, b16 = r2(img, 1), r2(w1a, 1).reshape(64, 1, 3, 3), r2(b1a, 1)
    v = _conv(img16[:, None], w16, b16)
    d = 10 * EPS32 * (_conv(np.abs(img16[:, None]), np.abs(w16)) + np.abs(b16)[None, :, None, None])
    a1 = np.maximum(r2(v, prec), 0.0)
    width = np.maximum(r2(v + d, prec), 0.0) - np.maximum(r2(v - d, prec), 0.0)
    return a1, np.minimum(width, d + ulp2(a1, prec))


def fused(img, w1a, b1a, w, b, prec):
    """fp64 reference and bound of the fused conv1a -> conv1b -> 2x2 max-pool launch -> (ref, bound) [B, 64, H / 2, W / 2]"""
    a1, da1 = conv1a(img, w1a, b1a, prec)
    return plain(a1, w, b, prec, pool=True, relu=True, dx=da1)          # (conv2d's zero padding = a1 is 0 outside the image)


def reference(cid: str, inp: dict, prec: int):
    c = CASES[cid]
    if c["form"] == "fused":
        return fused(inp["img"], inp["w1a"], inp["b1a"], inp["w"], inp["b"], prec)
    return plain(inp["x"], inp["w"], inp["b"], prec, pool=bool(c["pool"]), relu=bool(c["relu"]))
