"""The encoder's 3x3 convolution kernels one launch at a time against tests/conv_ref.py's float64 references and derived bounds, in both storage types, through
airfe_debug_conv: the persistent tile loops of conv64r / conv128r made to WRAP (ConvArgs::wgs lowered: buffer hand-over, the wait before the stores, the ragged
last round), the fused conv1a -> conv1b form with every prologue / ring / tail path of its patch pipeline, out_pad = 0, and conv3x3_kernel with relu = 0.  The
whole device buffer comes back as words over a 0xFF fill with guards, so an element the launch never wrote and a write into the border ring are both visible.
A tile's arithmetic does not depend on which round of which workgroup computes it: every lowered-wgs result must equal production's grid BYTE for byte."""
import numpy as np
import pytest

import conv_ref as cr
from airslam_amd import api
from gpu_common import context, diag

pytestmark = pytest.mark.gpu

PRECS = pytest.mark.parametrize("prec", [1, 0], ids=["fp16", "bf16"])
_REF, _RUN = {}, {}


def _ref(cid, prec):
    if (cid, prec) not in _REF:
        inp = cr.make_inputs(cid, prec)
        _REF[cid, prec] = (inp,) + cr.reference(cid, inp, prec)
    return _REF[cid, prec]


def _run(cid, prec, wgs):
    """one launch of case `cid` with `wgs` persistent workgroups (None: the kernel has no such grid), cached"""
    if (cid, prec, wgs) not in _RUN:
        c, inp = cr.CASES[cid], _ref(cid, prec)[0]
        ctx, _, _ = context("sp", precision=prec)
        _RUN[cid, prec, wgs] = ctx.debug_conv(inp["w"], inp["b"], prec, x=inp.get("x"), img=inp.get("img"), w1a=inp.get("w1a"), b1a=inp.get("b1a"), pool=c["pool"],
                                              out_pad=c["out_pad"], relu=c["relu"], wgs=wgs or 256)
    return _RUN[cid, prec, wgs]


def _name(cid, prec, wgs=None):
    return f"conv_{cid}_{'fp16' if prec else 'bf16'}" + (f"_wgs{wgs}" if wgs else "")


@PRECS
@pytest.mark.parametrize("cid,wgs", [(cid, w) for cid, c in cr.CASES.items() for w in c["wgs"]])
def test_canary(cid, wgs, prec):
    """guards and the border ring keep their 0xFF fill; every interior word was written"""
    p, out = cr.CASES[cid]["out_pad"], _run(cid, prec, wgs)
    raw = out["raw"]
    assert (out["guard_lo"] == 0xFFFF).all() and (out["guard_hi"] == 0xFFFF).all(), "a write outside the output buffer"
    inner = raw[:, p:raw.shape[1] - p, p:raw.shape[2] - p, :]
    unwritten = inner == 0xFFFF
    assert not unwritten.any(), f"{int(unwritten.sum())} interior words never written, first at {np.argwhere(unwritten)[0].tolist()}"
    if p:
        ring = np.ones(raw.shape, bool)
        ring[:, 1:-1, 1:-1, :] = False
        touched = ring & (raw != 0xFFFF)
        assert not touched.any(), f"{int(touched.sum())} words of the border ring written, first at {np.argwhere(touched)[0].tolist()}"


@PRECS
@pytest.mark.parametrize("cid", list(cr.CASES))
def test_bound(cid, prec):
    """production's grid against the float64 reference: per-element derived bound and the signed-mean cap"""
    _, ref, bound = _ref(cid, prec)
    got = _run(cid, prec, cr.CASES[cid]["wgs"][0])["y"]
    cr.check(_name(cid, prec), got, ref, bound, diag=diag)


@PRECS
@pytest.mark.parametrize("cid,wgs", [(cid, w) for cid, c in cr.CASES.items() for w in c["wgs"][1:]])
def test_wrapped_tile_loop_is_byte_equal(cid, wgs, prec):
    """fewer workgroups than tiles: every workgroup runs several rounds — the same words as one tile per workgroup"""
    base, got = _run(cid, prec, 256)["raw"], _run(cid, prec, wgs)["raw"]
    diff = base != got
    if diff.any():
        w = np.argwhere(diff)
        diag(_name(cid, prec, wgs), n_diff=int(diff.sum()), total=diff.size, first=w[0].tolist(), last=w[-1].tolist(),
             rows=np.unique(w[:, 1])[:64], cols=np.unique(w[:, 2])[:64], channels=np.unique(w[:, 3])[:64])
    assert not diff.any(), f"{int(diff.sum())} of {diff.size} words differ from the wgs = 256 launch, first at {np.argwhere(diff)[0].tolist()}"


@PRECS
def test_refusals(prec):
    """every form the hook refuses: an error with a message before any launch, and the context works afterwards"""
    ctx, _, _ = context("sp", precision=prec)
    rng = np.random.default_rng(7)
    w64, w128 = rng.normal(size=(64, 64, 3, 3)).astype(np.float32) / 24, rng.normal(size=(128, 128, 3, 3)).astype(np.float32) / 34
    x64, img = rng.normal(size=(1, 64, 16, 16)).astype(np.float32), rng.uniform(size=(1, 16, 16)).astype(np.float32)
    b, w1a = np.zeros(256, np.float32), np.zeros((64, 9), np.float32)
    bad = [
        dict(w=w64, b=b, x=x64, wgs=0), dict(w=w64, b=b, x=x64, wgs=257),
        dict(w=np.zeros((64, 32, 3, 3), np.float32), b=b, x=np.zeros((1, 32, 16, 16), np.float32)),                  # cin
        dict(w=np.zeros((96, 64, 3, 3), np.float32), b=b, x=x64),                                                    # cout % 64
        dict(w=np.zeros((192, 128, 3, 3), np.float32), b=b, x=np.zeros((1, 128, 16, 16), np.float32)),               # cout % 128 with cin = 128
        dict(w=w64, b=b, x=np.zeros((1, 64, 24, 16), np.float32)), dict(w=w64, b=b, x=np.zeros((1, 64, 16, 40), np.float32)),      # H, W % 16
        dict(w=w64, b=b, x=x64, pool=True, out_pad=0),
        dict(w=w64, b=b, img=img, w1a=w1a, b1a=b, pool=False), dict(w=w64, b=b, img=img, w1a=w1a, b1a=b, pool=True, out_pad=0),
        dict(w=w64, b=b, img=img, w1a=w1a, b1a=b, pool=True, relu=False), dict(w=w64, b=b, img=img, pool=True),      # the fused form's own
        dict(w=np.zeros((128, 64, 3, 3), np.float32), b=b, img=img, w1a=w1a, b1a=b, pool=True),
        dict(w=w128, b=b, img=img, w1a=w1a, b1a=b, pool=True),
        dict(w=w64, b=b, x=x64, img=img, w1a=w1a, b1a=b, pool=True),                                                 # both inputs
    ]
    for kw in bad:
        with pytest.raises(api.AirfeError) as e:
            ctx.debug_conv(prec=prec, **kw)
        assert str(e.value).startswith("airfe_debug_conv: debug_conv: ") and len(str(e.value)) > 40, str(e.value)       # the hook's own message
    out = ctx.debug_conv(w64, b, prec, x=x64)
    assert not (out["raw"][:, 1:-1, 1:-1, :] == 0xFFFF).any() and (out["guard_lo"] == 0xFFFF).all()
