"""The fp64 references of tests/kernel_ref.py against the oracle's float networks (oracle/ref_nets.py) and torch, and their bounds against
vacuity: what the GPU kernel tests (test_gpu_linear_kernels.py, test_gpu_lg_block.py) compare with must itself be right and sharp."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import kernel_ref as kr
from oracle import ref_nets


def _rng(seed):
    return np.random.default_rng(seed)


def test_layer_norm_and_gelu_match_torch():
    rng = _rng(1)
    h = rng.normal(size=(8, 512)) * 3 + rng.normal(size=(8, 1)) * 5
    g, b = rng.normal(size=512), rng.normal(size=512)
    y, _, _ = kr.layer_norm(h, g, b)
    ref = Fn.layer_norm(torch.from_numpy(h), (512,), torch.from_numpy(g), torch.from_numpy(b), eps=1e-5).numpy()
    assert np.abs(y - ref).max() < 1e-12
    assert np.abs(kr.gelu(y) - Fn.gelu(torch.from_numpy(y)).numpy()).max() < 1e-14


def test_ffn_matches_oracle():
    """LightGlue's ffn (ref_nets._ffn: linear -> LayerNorm -> GELU -> linear) = kr.lg_block's chain without the 2-byte roundings"""
    rng = _rng(2)
    w = {"l.ffn.0.weight": rng.normal(size=(512, 512)) / 22, "l.ffn.0.bias": rng.normal(size=512), "l.ffn.1.weight": 1 + rng.normal(size=512) * 0.1,
         "l.ffn.1.bias": rng.normal(size=512) * 0.1, "l.ffn.3.weight": rng.normal(size=(256, 512)) / 22, "l.ffn.3.bias": rng.normal(size=256)}
    w = {k: v.astype(np.float32) for k, v in w.items()}
    x = rng.normal(size=(16, 512)).astype(np.float32)
    ref = ref_nets._ffn(w, "l", torch.from_numpy(x)).double().numpy()
    h, _ = kr.linear(x, w["l.ffn.0.weight"], w["l.ffn.0.bias"])
    y, _, _ = kr.layer_norm(h, w["l.ffn.1.weight"], w["l.ffn.1.bias"])
    out, _ = kr.linear(kr.gelu(y), w["l.ffn.3.weight"], w["l.ffn.3.bias"])
    assert np.abs(out - ref).max() < 1e-4 * (1 + np.abs(ref).max())


def test_rope_matches_oracle():
    rng = _rng(3)
    t = rng.normal(size=(5, 64))
    ang = rng.uniform(-3, 3, size=(5, 32))
    freqs = torch.from_numpy(np.stack([np.repeat(np.cos(ang), 2, -1), np.repeat(np.sin(ang), 2, -1)]))
    ref = ref_nets._rope(freqs, torch.from_numpy(t)).numpy()
    assert np.abs(kr.rope(t, np.cos(ang), np.sin(ang)) - ref).max() < 1e-14
    # rows of several heads share one table
    t2 = rng.normal(size=(5, 512))
    got = kr.rope(t2, np.cos(ang), np.sin(ang))
    for h in range(8):
        assert np.abs(got[:, 64 * h:64 * h + 64] - ref_nets._rope(freqs, torch.from_numpy(t2[:, 64 * h:64 * h + 64])).numpy()).max() < 1e-14


def test_superglue_mlp_matches_oracle():
    """SuperGlue's mlp (ref_nets._sg_prop after the attention: relu(mlp.0 cat(x, msg)) -> mlp.3) = kr.lg_block(relu=True)'s chain"""
    rng = _rng(4)
    w = {"g.mlp.0.weight": rng.normal(size=(512, 512)) / 22, "g.mlp.0.bias": rng.normal(size=512), "g.mlp.3.weight": rng.normal(size=(256, 512)) / 22,
         "g.mlp.3.bias": rng.normal(size=256)}
    w = {k: v.astype(np.float32) for k, v in w.items()}
    x, msg = rng.normal(size=(256, 12)).astype(np.float32), rng.normal(size=(256, 12)).astype(np.float32)
    h = torch.relu(ref_nets._conv1d(w, "g.mlp.0", torch.cat([torch.from_numpy(x), torch.from_numpy(msg)], 0)))
    ref = ref_nets._conv1d(w, "g.mlp.3", h).double().numpy().T
    hh, _ = kr.linear(np.concatenate([x.T, msg.T], 1), w["g.mlp.0.weight"], w["g.mlp.0.bias"], relu=True)
    out, _ = kr.linear(hh, w["g.mlp.3.weight"], w["g.mlp.3.bias"])
    assert np.abs(out - ref).max() < 1e-4 * (1 + np.abs(ref).max())


@pytest.mark.parametrize("prec", [1, 0], ids=["fp16", "bf16"])
def test_rounding_helpers(prec):
    x = np.array([1.0, 1.0 + 2 ** -12, 3.0, -7.5e-3, 1e-9])
    r = kr.r2(x, prec)
    assert np.all(np.abs(r - x) <= 0.5 * kr.ulp2(x, prec) + 1e-30)
    assert kr.ulp2(1.0, prec) == (2.0 ** -10 if prec else 2.0 ** -7)


@pytest.mark.parametrize("prec", [1, 0], ids=["fp16", "bf16"])
def test_bounds_are_not_vacuous(prec):
    """on typical data a bound sits far below |ref|: a few ulps of the storage type, not a blanket tolerance"""
    rng = _rng(5 + prec)
    M = 64
    x = kr.r2(rng.normal(size=(M, 256)), prec)
    w = kr.r2(rng.normal(size=(512, 256)) / 16, prec)
    b = rng.normal(size=512).astype(np.float32)
    y, dy = kr.linear(x, w, b)
    bound = dy + kr.ulp2(y, prec)
    ulp_rel = 2.0 ** (-10 if prec else -7)
    assert np.median(bound / np.abs(y)) < 3 * ulp_rel
    blk = kr.lg_block(kr.r2(rng.normal(size=(M, 256)), prec), rng.normal(size=(M, 256)).astype(np.float32), kr.r2(rng.normal(size=(512, 512)) / 22, prec),
                      rng.normal(size=512), kr.r2(rng.normal(size=(256, 512)) / 22, prec), rng.normal(size=256), prec, gamma=1 + 0.1 * rng.normal(size=512),
                      beta=0.1 * rng.normal(size=512))
    ref, bnd = blk["x32"]
    assert np.median(bnd / np.abs(ref)) < 0.1          # (term 3 sums 512 aligned ulps of the 2-byte h tile: bf16 ~6 %, fp16 ~1 %)
    ref, bnd = kr.ln_gelu(kr.r2(rng.normal(size=(M, 512)) * 2 + 1, prec), 1 + 0.1 * rng.normal(size=512), 0.1 * rng.normal(size=512), prec)
    big = np.abs(ref) > 0.5
    assert np.median(bnd[big] / np.abs(ref[big])) < 3 * ulp_rel


def test_check_catches_truncation():
    """the signed-mean half of kr.check: values truncated towards zero stay inside one ulp each, and still fail"""
    rng = _rng(9)
    v = rng.normal(size=20000)
    bound = kr.ulp2(v, 1)
    kr.check("rn", kr.r2(v, 1), v, bound)
    trunc = np.trunc(v / kr.ulp2(v, 1)) * kr.ulp2(v, 1)
    assert np.all(np.abs(trunc - v) <= bound)
    with pytest.raises(AssertionError, match="systematic"):
        kr.check("trunc", trunc, v, bound)
