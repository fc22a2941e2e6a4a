"""fp64 references for the GEMM family and the fused LightGlue block, each with a DERIVED per-element error bound.

Every reference takes inputs that are already rounded to the storage type (gpu_common.to_2byte), evaluates in float64 and rounds to
the storage type exactly where the kernel stores: msg, h and xb in 2 bytes, x32 and the LayerNorm statistics in fp32.  The kernels'
approximations (GELU polynomials) are not part of a reference; they enter the bound.

A bound is the sum of four terms, each from the arithmetic the kernel does, none fitted to a measurement:
  1. one ulp of the stored output at |ref| (the kernel rounds once to nearest: half an ulp, plus the binade edge);
  2. fp32 accumulation: K * 2^-24 * sum |w x| (products of 2-byte operands are exact in fp32; gamma_K of a K-term sum), plus one fp32
     rounding of the bias add;
  3. one ulp of every 2-byte intermediate upstream, carried through the following linear map: sum |w| * ulp(h);
  4. the stated approximation errors: 4.2e-5 absolute for lf_gelu2 (kernels_lgblockf.hip), 1.5e-7 for Abramowitz & Stegun 7.1.26
     (ln_gelu_kernel, kernels_lg.hip).
`check` asserts the per-element bound AND a signed mean error below a fraction of the mean bound: round-to-nearest errors average out,
a truncation or a bias added after rounding does not.

Mutations applied to the kernels one at a time (scratch builds, never committed) and the first test that failed on each:
  bias added after the 2-byte rounding (gemm_store_run)    test_gpu_linear_kernels::test_every_epilogue_in_every_kernel[small-final_256x256-fp16]
  sign of sin flipped (rotate_pairs)                       test_gpu_linear_kernels::test_every_epilogue_in_every_kernel[small-qk_rot-fp16]
  EPI_RESID storing xb without the residual                test_gpu_linear_kernels::test_every_epilogue_in_every_kernel[small-ffn3_resid-fp16]
  highest GELU coefficient dropped (lf_gelu2, lf_gelu2x4)  test_gpu_lg_block::test_block_h_tile[wo-ln-0-fp16]
  LayerNorm variance divided by 511 (lg_blockf)            test_gpu_lg_block::test_block_h_tile[fold-ln-0-fp16]
  pack8 truncating instead of rounding                     test_gpu_linear_kernels::test_every_epilogue_in_every_kernel[small-final_256x256-fp16]
  a gemmr_gather tile reading the previous tile's indices  test_gpu_linear_kernels::test_gather[random-gemmr_gather-fp16]
  the mixed split's second round offset by one tile        test_gpu_lg_block::test_block_mixed_split[0-fp16]
The two block mutations stay inside the bound of the full block (512 weights' worth of h-tile ulps); the h-tile probe, ffn.3 as an identity
on one half of the tile, is what sees them.
"""
from __future__ import annotations

import numpy as np
import torch

EPS32 = 2.0 ** -24                  # unit round-off of fp32
LF_GELU_ERR = 4.2e-5                # lf_gelu2's stated max abs error (kernels_lgblockf.hip)
AS_GELU_ERR = 1.5e-7                # gelu_exact's erf (Abramowitz & Stegun 7.1.26, kernels_lg.hip)
GELU_SLOPE = 1.13                   # max |GELU'(y)| = 1.1289 (at y = 1.4142)
LN_EPS = 1e-5


# ------------------------------------------------------------------ storage types
def r2(x, prec: int) -> np.ndarray:
    """round to the 2-byte storage type (prec 1 = fp16, 0 = bf16) to nearest even, back in float64"""
    t = torch.from_numpy(np.asarray(x, np.float64).astype(np.float32))
    return t.to(torch.float16 if prec == 1 else torch.bfloat16).double().numpy()


def r32(x) -> np.ndarray:
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def ulp2(x, prec: int) -> np.ndarray:
    """one ulp of the 2-byte type at |x| (subnormal spacing below the smallest normal)"""
    mant, emin = (10, -14) if prec == 1 else (7, -126)
    e = np.floor(np.log2(np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** emin)))
    return 2.0 ** (e - mant)


def ulp32(x) -> np.ndarray:
    e = np.floor(np.log2(np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -126)))
    return 2.0 ** (e - 23)


# ------------------------------------------------------------------ elementwise pieces
def gelu(y) -> np.ndarray:
    """exact erf GELU in float64"""
    t = torch.from_numpy(np.asarray(y, np.float64))
    return (0.5 * t * (1.0 + torch.special.erf(t / np.sqrt(2.0)))).numpy()


def layer_norm(h, gamma, beta):
    """LayerNorm(512, eps 1e-5) in float64 -> (y, mean, rstd)"""
    h = np.asarray(h, np.float64)
    mean = h.mean(-1, keepdims=True)
    var = ((h - mean) ** 2).mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + LN_EPS)
    return (h - mean) * rstd * gamma + beta, mean, rstd


def ln_bound(h, dh, gamma):
    """error of y = LN(h) gamma + beta computed by a kernel from h known to +-dh, with fp32 statistics of a numerically sound form (two-pass
    or equivalent): mean to n eps |h|, variance to n eps var + (mean err)^2 + 2 dh mean|h - mean|, rstd to half the variance's relative error"""
    h = np.asarray(h, np.float64)
    n = h.shape[-1]
    mean = h.mean(-1, keepdims=True)
    d = h - mean
    var = (d ** 2).mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + LN_EPS)
    dmax = np.max(dh, -1, keepdims=True) if np.ndim(dh) else dh
    dmean = n * EPS32 * np.abs(h).mean(-1, keepdims=True) + dmax
    dvar = n * EPS32 * var + dmean ** 2 + 2 * dmax * np.abs(d).mean(-1, keepdims=True)          # (a shifted mean moves the variance in second order only)
    drstd = 0.5 * rstd * dvar / (var + LN_EPS) + 2 * EPS32 * rstd
    dy = np.abs(gamma) * (rstd * (dh + dmean) + np.abs(d) * drstd)
    # the fp32 normalisation itself: (h - mean) rstd, or h rstd - mean rstd (lg_blockf), then * gamma + beta
    return dy + 3 * EPS32 * np.abs(gamma) * rstd * (np.abs(h) + np.abs(mean)) + 2 * EPS32 * np.abs(d * rstd * gamma)


def rope(v, cos, sin):
    """rotate_pairs' contract on rows v [..., 64 * k] with tables [..., 32]: pair p = (f % 64) // 2 -> (v0 c - v1 s, v1 c + v0 s)"""
    v = np.asarray(v, np.float64)
    shp = v.shape
    v = v.reshape(shp[:-1] + (-1, 32, 2))
    c, s = np.asarray(cos, np.float64)[..., None, :], np.asarray(sin, np.float64)[..., None, :]
    out = np.stack([v[..., 0] * c - v[..., 1] * s, v[..., 1] * c + v[..., 0] * s], -1)
    return out.reshape(shp)


def rope_bound(v, dv):
    """bound after rotate_pairs of values v known to +-dv: dv0 + dv1 of the pair plus four fp32 roundings of its terms"""
    swap = lambda t: np.asarray(t, np.float64).reshape(t.shape[:-1] + (-1, 2))[..., ::-1].reshape(t.shape)
    return dv + swap(dv) + 4 * EPS32 * (np.abs(v) + np.abs(swap(v)))


# ------------------------------------------------------------------ linears
def acc_bound(x, w, b=None) -> np.ndarray:
    """term 2: K eps sum |w x| of an fp32 K-term sum, plus one rounding of the bias add"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    s = np.abs(x) @ np.abs(w).T
    y = x @ w.T + (0 if b is None else b)
    return w.shape[1] * EPS32 * s + EPS32 * np.abs(y)


def linear(x, w, b, relu=False):
    """fp64 y = x w^T + b (+ ReLU) and term 2 of its bound (the output is NOT rounded: callers round where the kernel stores)"""
    x, w, b = np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(b, np.float64)
    y = x @ w.T + b
    if relu:
        y = np.maximum(y, 0.0)
    return y, acc_bound(x, w, b)


def heads(y, Np: int, transposed=False):
    """[S * Np, 256 * k] rows -> head-major [S, 4, Np, 64] per 256-feature block (a list when k > 1) or transposed [S, 4, 64, Np]"""
    S = y.shape[0] // Np
    outs = []
    for sel in range(y.shape[1] // 256):
        t = y[:, sel * 256:(sel + 1) * 256].reshape(S, Np, 4, 64).transpose(0, 2, 1, 3)
        outs.append(np.ascontiguousarray(t.transpose(0, 1, 3, 2) if transposed else t))
    return outs if len(outs) > 1 else outs[0]


def softmax_d2s(logits, dlog, hc: int, wc: int):
    """SuperPoint's head epilogue: soft-max over the 65 logits of a cell, dustbin (feature 64) dropped, 8 x 8 depth-to-space ->
    heat [B, 8 hc, 8 wc] and its bound from the logits' error dlog (soft-max moves by at most 2 max dlog relatively; expf / the
    division add a few fp32 ulps)"""
    logits = np.asarray(logits, np.float64)
    m = logits.max(1, keepdims=True)
    e = np.exp(logits - m)
    p = e / e.sum(1, keepdims=True)
    dp = p * (2 * np.max(dlog, 1, keepdims=True) + 80 * EPS32) + 2 * ulp32(p)
    B = logits.shape[0] // (hc * wc)

    def d2s(t):
        return t[:, :64].reshape(B, hc, wc, 8, 8).transpose(0, 1, 3, 2, 4).reshape(B, 8 * hc, 8 * wc)
    return d2s(p), d2s(dp)


# ------------------------------------------------------------------ the fused post-attention block and the four-launch path
def lg_block(attn, x32, w1, b1, w2, b2, prec, gamma=None, beta=None, wo=None, bo=None, relu=False, nqk=None, nv=None, rot=None, Np=0,
             gelu_err=LF_GELU_ERR):
    """fp64 reference of lg_blockf with bounds.  Returns dict of (ref, bound) pairs: x32, xb and, with the next projection, q, k, vt."""
    attn, x32 = np.asarray(attn, np.float64), np.asarray(x32, np.float64)
    xb = r2(x32, prec)
    if wo is not None:                                     # msg = Wo attn + bo, stored in 2 bytes (the msg tile)
        m, dm = linear(attn, wo, bo)
        msg = r2(m, prec)
        dmsg = dm + ulp2(m, prec)
    else:                                                  # folded: ffn.0 reads cat(x, attn) directly
        msg, dmsg = attn, np.zeros_like(attn)
    xin = np.concatenate([xb, msg], 1)
    h, dh = linear(xin, w1, b1)
    dh = dh + np.abs(dmsg) @ np.abs(np.asarray(w1, np.float64)[:, 256:]).T
    if relu:
        g = np.maximum(h, 0.0)
        dg = dh
    else:
        y, _, _ = layer_norm(h, gamma, beta)
        dy = ln_bound(h, dh, gamma)
        g = gelu(y)
        dg = GELU_SLOPE * dy + gelu_err
    gs = r2(g, prec)                                       # the h tile: 2 bytes
    dgs = dg + ulp2(g, prec)
    o, do = linear(gs, w2, b2)
    do = do + np.abs(dgs) @ np.abs(np.asarray(w2, np.float64)).T
    xn = x32 + o
    dx = do + EPS32 * np.abs(xn)
    xbn = r2(xn, prec)
    out = {"x32": (xn, dx), "xb": (xbn, dx + ulp2(xn, prec))}
    if nqk is not None:
        dxb = dx + ulp2(xn, prec)                          # the next projection reads the stored xb
        for name, (w, b), rotary in (("qk", nqk, rot is not None), ("v", nv, False)):
            p, dp = linear(xbn, w, b)
            dp = dp + dxb @ np.abs(np.asarray(w, np.float64)).T
            if rotary:                                     # |cos|, |sin| <= 1: a rotated element carries the errors of both of its pair
                dp, p = rope_bound(p, dp), rope(p, rot[0], rot[1])
            bound = dp + ulp2(p, prec)
            if name == "qk":
                hs, bs = heads(p, Np), heads(bound, Np)
                if isinstance(hs, list):
                    out["q"], out["k"] = (hs[0], bs[0]), (hs[1], bs[1])
                else:
                    out["q"] = (hs, bs)
            else:
                out["vt"] = (heads(p, Np, True), heads(bound, Np, True))
    return out


def ln_gelu(h, gamma, beta, prec):
    """ln_gelu_kernel on 2-byte rows h [M, 512] (exact: they are the kernel's input) -> (ref, bound)"""
    h = np.asarray(h, np.float64)
    y, _, _ = layer_norm(h, gamma, beta)
    g = gelu(y)
    dg = GELU_SLOPE * ln_bound(h, 0.0, gamma) + AS_GELU_ERR
    return r2(g, prec), dg + ulp2(g, prec)


# ------------------------------------------------------------------ the assertion
def check(name, got, ref, bound, mean_frac=0.1, diag=None):
    """|got - ref| <= bound everywhere, and the signed mean error (plain and towards |ref|) below mean_frac of the mean bound"""
    got, ref, bound = (np.asarray(t, np.float64) for t in (got, ref, bound))
    assert got.shape == ref.shape == bound.shape, (name, got.shape, ref.shape, bound.shape)
    err = got - ref
    ratio = np.abs(err) / bound
    worst = np.unravel_index(np.argmax(np.where(np.isnan(ratio), np.inf, ratio)), ratio.shape)
    mb = bound.mean()
    mean_err, mean_mag = err.mean() / mb, (err * np.sign(ref)).mean() / mb
    info = dict(worst_ratio=float(np.nanmax(ratio)) if not np.isnan(ratio).all() else float("nan"), n_bad=int((~(np.abs(err) <= bound)).sum()), total=err.size,
                worst=list(map(int, worst)), got_at=float(got[worst]), ref_at=float(ref[worst]), bound_at=float(bound[worst]), mean_err=float(mean_err),
                mean_err_towards_ref=float(mean_mag), bound_over_ref=float(mb / max(np.abs(ref).mean(), 1e-300)))
    if diag:
        diag(name, **info)
    assert np.all(np.abs(err) <= bound), f"{name}: {info}"
    assert abs(mean_err) < mean_frac and abs(mean_mag) < mean_frac, f"{name}: systematic error {info}"
    return info
