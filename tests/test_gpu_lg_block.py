"""The fused post-attention block (lg_blockf, kernels_lgblockf.hip) in every template the launcher can pick, and the four-launch path's
ln_gelu_kernel, against the fp64 references of tests/kernel_ref.py with derived bounds.  Also the rows past M that a launch writes: the
header's "a ragged last pass stores its surplus rows too" as a stated slack."""
import numpy as np
import pytest

import kernel_ref as kr
from gpu_common import context, diag

pytestmark = pytest.mark.gpu

PRECS = pytest.mark.parametrize("prec", [1, 0], ids=["fp16", "bf16"])


def _ctx():
    return context("sp")[0]


def _weights(prec, seed, folded, relu, nq, b1_shift=0.0, w1_scale=1.0):
    rng = np.random.default_rng(seed)
    q = lambda a: kr.r2(a, prec).astype(np.float32)
    p = dict(w1=q(rng.normal(size=(512, 512)) / 22 * w1_scale), b1=(rng.normal(size=512) * 0.5 + b1_shift).astype(np.float32),
             w2=q(rng.normal(size=(256, 512)) / 22), b2=(rng.normal(size=256) * 0.1).astype(np.float32))
    if not relu:
        p.update(gamma=(1 + 0.1 * rng.normal(size=512)).astype(np.float32), beta=(0.1 * rng.normal(size=512)).astype(np.float32))
    if not folded:
        p.update(wo=q(rng.normal(size=(256, 256)) / 16), bo=(0.1 * rng.normal(size=256)).astype(np.float32))
    if nq:
        p.update(nqk=(q(rng.normal(size=(nq, 256)) / 16), (0.1 * rng.normal(size=nq)).astype(np.float32)),
                 nv=(q(rng.normal(size=(256, 256)) / 16), (0.1 * rng.normal(size=256)).astype(np.float32)))
    return rng, p


def _inputs(rng, prec, M):
    return kr.r2(rng.normal(size=(M, 256)), prec).astype(np.float32), rng.normal(size=(M, 256)).astype(np.float32)


def _slack(M, T, mixed, n_cu=256):
    if not mixed:
        return -(-M // T) * T - M
    tiles = -(-M // 16)
    return n_cu * 112 + -(-(tiles - 7 * n_cu) // 6) * 96 - M


def _run(prec, M, folded, relu, nq, T, mixed=False, Np=208, seed=0, rows=None, label="", probe=None, **wkw):
    """the block on M tokens; rows: the token rows the reference is taken on (rows are independent); probe = first h feature that ffn.3 copies
    straight into x32 (identity rows, x32 = b2 = 0), so that the 2-byte h tile itself is compared"""
    ctx = _ctx()
    rng, p = _weights(prec, seed + 31 * nq + 7 * int(folded) + int(relu), folded, relu, nq, **wkw)
    attn, x32 = _inputs(rng, prec, M)
    if probe is not None:
        p["w2"] = np.zeros((256, 512), np.float32)
        p["w2"][np.arange(256), probe + np.arange(256)] = 1.0
        p["b2"] = np.zeros(256, np.float32)
        x32 = np.zeros_like(x32)
    rot = None
    if nq == 512:
        ang = rng.uniform(-np.pi, np.pi, size=(M, 32))
        rot = (np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32))
    got = ctx.debug_lg_block(attn, x32, p["w1"], p["b1"], p["w2"], p["b2"], prec, gamma=p.get("gamma"), beta=p.get("beta"), wo=p.get("wo"), bo=p.get("bo"),
                             relu=relu, tokens_per_wg=T, mixed=mixed, nqk=p.get("nqk"), nv=p.get("nv"), rot=rot, Np=Np if nq else 0)
    sel = np.arange(M) if rows is None else rows
    ref = kr.lg_block(attn[sel], x32[sel], p["w1"], p["b1"], p["w2"], p["b2"], prec, gamma=p.get("gamma"), beta=p.get("beta"), wo=p.get("wo"), bo=p.get("bo"),
                      relu=relu, nqk=p.get("nqk"), nv=p.get("nv"), rot=None if rot is None else (rot[0][sel], rot[1][sel]), Np=len(sel) if rows is not None else Np)
    tag = f"lgb_{'fold' if folded else 'wo'}_{'relu' if relu else 'ln'}_{nq}_{T}{'m' if mixed else ''}_{M}{label}_{'fp16' if prec else 'bf16'}"
    for key in ("x32", "xb"):
        kr.check(f"{tag}_{key}", got[key][sel], ref[key][0], ref[key][1], diag=diag)
    if nq:
        S = M // Np
        flat = lambda t: t.transpose(0, 2, 1, 3).reshape(S * Np, 256)             # [S, 4, Np, 64] -> token rows
        flat_t = lambda t: t.transpose(0, 3, 1, 2).reshape(S * Np, 256)           # [S, 4, 64, Np] -> token rows
        unflat = lambda r: r.transpose(0, 2, 1, 3).reshape(r.shape[0] * r.shape[2], 256) if rows is None else r[0].transpose(1, 0, 2).reshape(-1, 256)
        unflat_t = lambda r: r.transpose(0, 3, 1, 2).reshape(-1, 256) if rows is None else r[0].transpose(2, 0, 1).reshape(-1, 256)
        for key in ("q", "k") if nq == 512 else ("q",):
            kr.check(f"{tag}_{key}", flat(got[key])[sel], unflat(kr.r2(ref[key][0], prec)), unflat(ref[key][1]), diag=diag)
        kr.check(f"{tag}_vt", flat_t(got["vt"])[sel], unflat_t(kr.r2(ref["vt"][0], prec)), unflat_t(ref["vt"][1]), diag=diag)
    slack = _slack(M, T, mixed, _ctx_n_cu() if mixed else 256)
    rp = got["rows_past"]
    diag(tag + "_rows_past", rows_past=rp, slack=slack)
    assert rp[0] == slack and rp[1] <= slack and max(rp[2:]) <= slack, (rp, slack)
    return got


TEMPLATES = [(f, r, n) for f in (False, True) for r in (False, True) for n in ((0,) if r else (0, 512, 256))]


@PRECS
@pytest.mark.parametrize("T", [32, 64, 112, 128])
@pytest.mark.parametrize("folded,relu,nq", TEMPLATES, ids=[f"{'fold' if f else 'wo'}-{'relu' if r else 'ln'}-nq{n}" for f, r, n in TEMPLATES])
def test_block_templates(folded, relu, nq, T, prec):
    """M = 624 = 3 x 208 tokens: ragged for every pass size (32, 64, 112, 128)"""
    _run(prec, 624, folded, relu, nq, T)


@PRECS
@pytest.mark.parametrize("nq", [0, 512, 256])
def test_block_mixed_split(nq, prec):
    """the two-round split at the bench's 51200 tokens: one 7-tile pass per CU, then 6-tile passes; the reference on every 5th row and
    on both sides of the round boundary"""
    M, n_cu = 51200, _ctx_n_cu()
    edge = n_cu * 112
    rows = np.unique(np.concatenate([np.arange(0, M, 5), np.arange(edge - 200, edge + 200), np.arange(M - 200, M)]))
    _run(prec, M, True, False, nq, 112, mixed=True, Np=400, rows=rows)


def _ctx_n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@PRECS
@pytest.mark.parametrize("half", [0, 256])
@pytest.mark.parametrize("folded,relu", [(False, False), (True, False), (False, True), (True, True)], ids=["wo-ln", "fold-ln", "wo-relu", "fold-relu"])
def test_block_h_tile(folded, relu, half, prec):
    """ffn.3 as an identity on one half of the h tile: the LayerNorm + GELU (or ReLU) output itself against the fp64 chain, without 512
    weights' worth of ulps in the bound"""
    _run(prec, 624, folded, relu, 0, 64, label=f"_h{half}", probe=half)


LN_RATIOS = [0.0, 10.0, 100.0, 300.0]


@PRECS
@pytest.mark.parametrize("ratio", LN_RATIOS)
def test_block_layer_norm_edge_rows(ratio, prec):
    """rows of ffn.0 output with |mean| / std ~ ratio, planted through b1 (std of W1 cat(x, attn) ~ 1.4): the LayerNorm statistics of
    a row far from zero.  ffn.3 copies the h tile (probe), so the LayerNorm's own error is measured against a bound without ffn.3's slack"""
    for half in (0, 256):
        _run(prec, 256, True, False, 0, 32, label=f"_r{ratio:g}_h{half}", probe=half, b1_shift=1.4 * ratio)


@PRECS
def test_block_layer_norm_flat_rows(prec):
    """near-zero spread: W1 scaled to 1e-3, so that eps = 1e-5 dominates the variance"""
    _run(prec, 256, True, False, 0, 32, label="_flat", probe=0, w1_scale=1e-3, b1_shift=3.0)


@PRECS
@pytest.mark.parametrize("ratio", LN_RATIOS + ["flat"])
def test_ln_gelu_edge_rows(ratio, prec):
    """the four-launch path's ln_gelu_kernel on 2-byte rows with the same shapes of statistics"""
    rng = np.random.default_rng(41)
    M = 256
    if ratio == "flat":
        h = 3.0 + 1e-3 * rng.normal(size=(M, 512))
    else:
        h = rng.normal(size=(M, 512)) * 1.4 + 1.4 * ratio + rng.normal(size=512) * 0.5
    h = kr.r2(h, prec)
    gamma, beta = 1 + 0.1 * rng.normal(size=512), 0.1 * rng.normal(size=512)
    gamma, beta = gamma.astype(np.float32), beta.astype(np.float32)
    got = _ctx().debug_ln_gelu(h.astype(np.float32), gamma, beta, prec)
    ref, bound = kr.ln_gelu(h, gamma, beta, prec)
    kr.check(f"ln_gelu_{ratio}_{'fp16' if prec else 'bf16'}", got, ref, bound, diag=diag)
