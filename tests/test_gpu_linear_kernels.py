"""Every epilogue of the GEMM family through every kernel that accepts it, against the fp64 references of tests/kernel_ref.py with derived
bounds (per element and signed mean).  The hooks (include/airfe_debug.h: airfe_debug_linear / _qkv) launch the production kernels; a forced
kernel that does not apply is an error, so a case can never check another kernel than the one it names."""
import numpy as np
import pytest

import kernel_ref as kr
from gpu_common import context, diag

pytestmark = pytest.mark.gpu

PRECS = pytest.mark.parametrize("prec", [1, 0], ids=["fp16", "bf16"])
STORE, STORE_F32, RESID, HEADS, HEADS_T, SOFTMAX_D2S = range(6)


def _ctx():
    return context("sp")[0]


def _data(prec, M, K, N, seed, K1=None, src_rows=None):
    rng = np.random.default_rng(seed)
    x1 = kr.r2(rng.normal(size=(src_rows or M, K1 or K)), prec).astype(np.float32)
    x2 = kr.r2(rng.normal(size=(M, K - K1)), prec).astype(np.float32) if K1 else None
    w = kr.r2(rng.normal(size=(N, K)) / np.sqrt(K), prec).astype(np.float32)
    b = rng.normal(size=N).astype(np.float32)
    return rng, x1, x2, w, b


def _rot(rng, M):
    ang = rng.uniform(-np.pi, np.pi, size=(M, 32))
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


# (K, N, K1, epi, act) of the pipelines' run_linear / run_qkv calls (airfe_match.hip, airfe_detect.hip)
FORMS = {
    "final_256x256": (256, 256, None, STORE, 0),          # lg_final, sg_final, out-projections
    "mlp0_cat_relu": (512, 512, 256, STORE, 1),           # SuperGlue mlp.0 on cat(x, msg)
    "ffn0_cat": (512, 512, 256, STORE, 0),                # ffn.0 of the four-launch path
    "sg_k3_relu": (128, 256, None, STORE, 1),             # SuperGlue keypoint encoder tail
    "ffn3_resid": (512, 256, None, RESID, 0),             # ffn.3 / mlp.3 into the residual
    "sg_k4_resid": (256, 256, None, RESID, 0),
    "head_f32_145": (128, 145, None, STORE_F32, 0),       # PLNet's fused head
    "desc_f32": (256, 256, None, STORE_F32, 0),           # descriptor head
    "qk_rot": (256, 512, None, HEADS, 0),                 # self q | k with rotary
    "qk_shared": (256, 256, None, HEADS, 0),              # cross block's shared projection
    "v_t": (256, 256, None, HEADS_T, 0),                  # V, transposed
}
KERNELS_OF = {
    "small": list(FORMS), "tiled": list(FORMS), "gemm8": list(FORMS),
    "gemmr": ["final_256x256", "qk_rot", "qk_shared", "v_t"],
}
CASES = [(k, f) for k, fs in KERNELS_OF.items() for f in fs]


def _run_form(ctx, prec, form, kernel, M, Np=400, gr_wgs=0, seed=0):
    K, N, K1, epi, act = FORMS[form]
    rng, x1, x2, w, b = _data(prec, M, K, N, seed + K + N + M, K1)
    xin = x1 if x2 is None else np.concatenate([x1, x2], 1)
    ref, dacc = kr.linear(xin, w, b, relu=bool(act))
    kw = dict(prec=prec, epi=epi, act=act, x2=x2, kernel=kernel, gr_wgs=gr_wgs)
    name = f"lin_{form}_{kernel}_{M}_{gr_wgs}_{'fp16' if prec else 'bf16'}"
    if epi == STORE:
        got = ctx.debug_linear(x1, w, b, **kw)
        kr.check(name, got, kr.r2(ref, prec), dacc + kr.ulp2(ref, prec), diag=diag)
    elif epi == STORE_F32:
        got = ctx.debug_linear(x1, w, b, **kw)
        kr.check(name, got, ref, dacc + kr.ulp32(ref), diag=diag)
    elif epi == RESID:
        x32 = (rng.normal(size=(M, N)) * 2).astype(np.float32)
        xb, x32n = ctx.debug_linear(x1, w, b, x32=x32, **kw)
        xn = x32.astype(np.float64) + ref
        dx = dacc + kr.EPS32 * np.abs(xn)
        kr.check(name + "_x32", x32n, xn, dx + kr.ulp32(xn), diag=diag)
        kr.check(name + "_xb", xb, kr.r2(xn, prec), dx + kr.ulp2(xn, prec), diag=diag)
    else:
        rot = _rot(rng, M) if form == "qk_rot" else None
        got = ctx.debug_linear(x1, w, b, Np=Np, rot=rot, **kw)
        bound = dacc
        if rot is not None:
            bound, ref = kr.rope_bound(ref, dacc), kr.rope(ref, *rot)
        bound = bound + kr.ulp2(ref, prec)
        outs = got if isinstance(got, tuple) else (got,)
        refs, bnds = kr.heads(ref, Np, epi == HEADS_T), kr.heads(bound, Np, epi == HEADS_T)
        refs, bnds = (refs, bnds) if isinstance(refs, list) else ([refs], [bnds])
        for i, (o, r, d) in enumerate(zip(outs, refs, bnds)):
            kr.check(f"{name}_{i}", o, kr.r2(r, prec), d, diag=diag)


@PRECS
@pytest.mark.parametrize("kernel,form", CASES, ids=[f"{k}-{f}" for k, f in CASES])
def test_every_epilogue_in_every_kernel(kernel, form, prec):
    """M = 1200 = 3 x 400 tokens: a multiple of none of the row tiles (32 / 128 / 256); the hook pads as the matcher does"""
    _run_form(_ctx(), prec, form, kernel, 1200)


@PRECS
@pytest.mark.parametrize("form", ["final_256x256", "qk_rot", "v_t"])
def test_gemmr_ring_wraps(form, prec):
    """24 persistent workgroups over 38 token tiles: every workgroup streams more tiles than its ring holds slots for some of them"""
    _run_form(_ctx(), prec, form, "gemmr", 6000, Np=400, gr_wgs=24)


@PRECS
@pytest.mark.parametrize("M", [4000, 4096, 4128, 8000, 8192, 15872, 16000, 16128])
def test_dispatch_thresholds(M, prec):
    """launch_gemm's own choice on and next to small_max = 4096, gr_min = 8192, g8_min = 16000 (and M % 256)"""
    _run_form(_ctx(), prec, "final_256x256", "dispatch", M)
    _run_form(_ctx(), prec, "v_t", "dispatch", M - M % 16 if M % 16 else M, Np=16)


@PRECS
@pytest.mark.parametrize("pair", [True, False], ids=["pair", "separate"])
@pytest.mark.parametrize("nqk", [512, 256])
def test_qkv(nqk, pair, prec):
    """run_qkv's two forms (one gemmr_pair launch / two linears), the ring wrapped (gr_wgs = 24)"""
    ctx = _ctx()
    M, Np = 9600, 400
    rng, x, _, wqk, bqk = _data(prec, M, 256, nqk, nqk + int(pair))
    wv = kr.r2(rng.normal(size=(256, 256)) / 16, prec).astype(np.float32)
    bv = rng.normal(size=256).astype(np.float32)
    rot = _rot(rng, M) if nqk == 512 else None
    q, k, vt = ctx.debug_qkv(x, wqk, bqk, wv, bv, prec, Np, rot=rot, pair=pair, gr_wgs=24)
    p, dp = kr.linear(x, wqk, bqk)
    if rot is not None:
        dp, p = kr.rope_bound(p, dp), kr.rope(p, *rot)
    bound = dp + kr.ulp2(p, prec)
    refs, bnds = kr.heads(p, Np), kr.heads(bound, Np)
    refs, bnds = (refs, bnds) if isinstance(refs, list) else ([refs], [bnds])
    tag = f"qkv_{nqk}_{int(pair)}_{'fp16' if prec else 'bf16'}"
    for o, r, d, nm in zip((q, k), refs, bnds, ("q", "k")):
        kr.check(f"{tag}_{nm}", o, kr.r2(r, prec), d, diag=diag)
    v, dv = kr.linear(x, wv, bv)
    kr.check(f"{tag}_vt", vt, kr.r2(kr.heads(v, Np, True), prec), kr.heads(dv + kr.ulp2(v, prec), Np, True), diag=diag)


def _gather_lists(rng, M, src):
    return {
        "random": rng.integers(0, src, M),
        "repeated": np.repeat(rng.integers(0, src, M // 8 + 1), 8)[:M],
        "descending": (src - 1 - np.arange(M)) % src,
        "last_row": np.full(M, src - 1),
    }


@PRECS
@pytest.mark.parametrize("kernel", ["gemm8", "gemmr_gather"])
@pytest.mark.parametrize("order", ["random", "repeated", "descending", "last_row"])
def test_gather(kernel, order, prec):
    """y[r] = W x[rowidx[r]] + b (the descriptor head over sampled cells), fp32 rows out"""
    ctx = _ctx()
    M, src = 3000, 5000
    rng, x1, _, w, b = _data(prec, M, 256, 256, 7, src_rows=src)
    idx = _gather_lists(rng, M, src)[order].astype(np.int32)
    got = ctx.debug_linear(x1, w, b, prec=prec, epi=STORE_F32, rowidx=idx, kernel=kernel, gr_wgs=24)
    ref, dacc = kr.linear(x1[idx], w, b)
    kr.check(f"gather_{kernel}_{order}_{'fp16' if prec else 'bf16'}", got, ref, dacc + kr.ulp32(ref), diag=diag)


@PRECS
def test_gemmr_gather_tile_limit(prec):
    """the busiest workgroup's index list holds at most 240 tiles: one workgroup over exactly 240 tiles runs, one more tile is refused"""
    from airslam_amd.api import AirfeError
    ctx = _ctx()
    M = 240 * 32
    rng, x1, _, w, b = _data(prec, M, 256, 256, 11, src_rows=M + 64)
    idx = rng.integers(0, M + 64, M).astype(np.int32)
    got = ctx.debug_linear(x1, w, b, prec=prec, epi=STORE_F32, rowidx=idx, kernel="gemmr_gather", gr_wgs=1)
    ref, dacc = kr.linear(x1[idx], w, b)
    kr.check(f"gather_limit_{'fp16' if prec else 'bf16'}", got, ref, dacc + kr.ulp32(ref), diag=diag)
    idx2 = np.concatenate([idx, idx[:32]])
    with pytest.raises(AirfeError, match="does not apply"):
        ctx.debug_linear(x1, w, b, prec=prec, epi=STORE_F32, rowidx=idx2, kernel="gemmr_gather", gr_wgs=1)


@PRECS
@pytest.mark.parametrize("order", ["random", "descending", "last_row"])
def test_gemmr_gather128(order, prec):
    """the LOI head at the junctions' tap rows: K = N = 128, 1200 tap rows per image over a [128 x 128] line-feature map, two images"""
    ctx = _ctx()
    M, src = 2400, 2 * 128 * 128
    rng, x1, _, w, b = _data(prec, M, 128, 128, 13, src_rows=src)
    idx = _gather_lists(rng, M, src)[order].astype(np.int32)
    got = ctx.debug_linear(x1, w, b, prec=prec, epi=STORE_F32, rowidx=idx, kernel="gemmr_gather128", gr_wgs=24)
    ref, dacc = kr.linear(x1[idx], w, b)
    kr.check(f"gather128_{order}_{'fp16' if prec else 'bf16'}", got, ref, dacc + kr.ulp32(ref), diag=diag)


@PRECS
def test_softmax_d2s(prec):
    """SuperPoint's head: soft-max over 65 logits, dustbin dropped, 8 x 8 depth-to-space; a cell with a 2-byte inf input raises the flag and
    leaves every other cell alone"""
    ctx = _ctx()
    hc = wc = 16
    M = 2 * hc * wc
    rng, x1, _, w, b = _data(prec, M, 256, 65, 17)
    w *= 4                                                  # peaky logits, as the trained head's
    logits, dl = kr.linear(x1, w, b)
    ref, bound = kr.softmax_d2s(logits, dl, hc, wc)
    heat, flag = ctx.debug_linear(x1, w, b, prec=prec, epi=SOFTMAX_D2S, d2s=(hc, wc))
    assert flag == 0
    kr.check(f"d2s_{'fp16' if prec else 'bf16'}", heat, ref, bound, diag=diag)
    bad_cell = 300                                          # image 1, cell (2, 12)
    x1[bad_cell, 5] = np.inf
    heat2, flag2 = ctx.debug_linear(x1, w, b, prec=prec, epi=SOFTMAX_D2S, d2s=(hc, wc))
    assert flag2 == 1
    bi, rem = divmod(bad_cell, hc * wc)
    cy, cx = divmod(rem, wc)
    keep = np.ones(heat2.shape, bool)
    keep[bi, cy * 8:cy * 8 + 8, cx * 8:cx * 8 + 8] = False
    assert np.array_equal(heat2[keep], heat[keep])


@PRECS
def test_forced_kernel_is_refused_not_replaced(prec):
    """a form the named kernel does not take is an error: gemmr has no fp32 store, gather128 wants K = 128, small takes no row list"""
    from airslam_amd.api import AirfeError
    ctx = _ctx()
    rng, x1, _, w, b = _data(prec, 1024, 256, 256, 19)
    for kw in (dict(epi=STORE_F32, kernel="gemmr"), dict(epi=STORE_F32, kernel="gemmr_gather128", rowidx=np.zeros(1024, np.int32)),
               dict(epi=STORE_F32, kernel="small", rowidx=np.zeros(1024, np.int32))):
        with pytest.raises(AirfeError):
            ctx.debug_linear(x1, w, b, prec=prec, **kw)


@PRECS
def test_a_refused_form_leaves_nothing_behind(prec):
    """M = 160 rows (one 128-row tile plus a 32-row remainder), K = 128, N = 64, EPI_STORE: the dispatched form, then the same data through a forced kernel with a
    row list that the hook refuses AFTER it staged every operand (its uploads and 0xFF fills are queued on the context's stream when it returns the error), then the
    first form again: byte-equal.  The refusal that comes after the staging is the kernel's own applicability test — gemmr_gather wants K = 256; kernel = "small" with
    a row list is turned away by the argument checks, before anything is staged, with another text."""
    from airslam_amd.api import AirfeError
    ctx = _ctx()
    M = 160
    rng, x1, _, w, b = _data(prec, M, 128, 64, 23)
    first = ctx.debug_linear(x1, w, b, prec=prec, epi=STORE, kernel="dispatch")
    with pytest.raises(AirfeError, match="does not apply"):
        ctx.debug_linear(x1, w, b, prec=prec, epi=STORE, kernel="gemmr_gather", rowidx=np.arange(M, dtype=np.int32))
    again = ctx.debug_linear(x1, w, b, prec=prec, epi=STORE, kernel="dispatch")
    assert np.isfinite(first).all()
    assert first.tobytes() == again.tobytes()


@PRECS
def test_softmax_flag_belongs_to_its_call(prec):
    """M = 16 (one image of 4 x 4 cells), K = 256, N = 65, three calls on one context — clean input, one inf in one cell, clean again: flags 0, 1, 0 (the flag word
    is zero when each launch starts), the third heat map byte-equal to the first, the second equal to the first outside the bad cell's 8 x 8 block"""
    ctx = _ctx()
    hc = wc = 4
    rng, x1, _, w, b = _data(prec, hc * wc, 256, 65, 29)
    bad = x1.copy()
    cy, cx = 2, 1
    bad[cy * wc + cx, 7] = np.inf
    (h0, f0), (h1, f1), (h2, f2) = (ctx.debug_linear(x, w, b, prec=prec, epi=SOFTMAX_D2S, d2s=(hc, wc)) for x in (x1, bad, x1))
    assert (f0, f1, f2) == (0, 1, 0)
    assert h2.tobytes() == h0.tobytes()
    keep = np.ones(h0.shape, bool)
    keep[0, cy * 8:cy * 8 + 8, cx * 8:cx * 8 + 8] = False
    assert np.array_equal(h1[keep], h0[keep])
