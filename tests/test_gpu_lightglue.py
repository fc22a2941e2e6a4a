"""LightGlue parity on the GPU (C ABI) vs the CPU oracle.  The structured synthetic weights make the planted half of every
pair match (203 matches at N = 400, 514 at N = 1024 in the oracle), so filter_matches, the match buffers and the batch paths
are exercised on hundreds of entries; match INDEX SETS must be identical to the fp32 oracle's.

The gates here absorb a whole 2-byte network.  The kernels of the head and the tail (prepare, matchability, similarity, both assignment forms, the filters) are
held to float64 references with derived bounds, one launcher at a time, in tests/test_gpu_lg_tail.py."""
import math

import numpy as np
import pytest

from gpu_common import context, diag
from oracle import ref_nets, ref_post
from planted import fragile_rows, normalised, planted_pair

pytestmark = pytest.mark.gpu

# Gates, absolute, in log-assignment units (the filter threshold is log 0.1 = -2.303):
#   matcher_precision = 1 (fp16, the default = the reference's kFP16 engines): 0.05
#   matcher_precision = 0 (bf16): 0.5 — eight mantissa bits; measured ~0.3, an emulation of the rounding points
#   (tools/lg_precision_bisect.py) attributes it evenly to weights, the token shadow and the FFN hidden state
TOL = {1: 0.05, 0: 0.5}


def _pair(n0, n1, seed):
    f0, f1 = planted_pair(n0, n1, seed)
    n0f, n1f = normalised(f0), normalised(f1)
    return f0, f1, np.ascontiguousarray(n0f[:, 1:]), np.ascontiguousarray(n1f[:, 1:])


def _check_against_oracle(name, s, ref, idx, sc, tol, min_matches):
    """scores within `tol` of the oracle everywhere; filter_matches reproduced exactly on the device's own scores; match index
    set identical to the oracle's, except rows the oracle itself decides within the tolerance (must be a negligible share)."""
    err = np.abs(s - ref)
    ridx, rsc = ref_post.filter_matches(ref, 0.1)
    didx, dsc = ref_post.filter_matches(s, 0.1)
    frag = fragile_rows(ref, tol)
    dev = {tuple(p) for p in idx if p[0] not in frag}
    want = {tuple(p) for p in ridx if p[0] not in frag}
    diag(name, max_err=err.max(), mean_err=err.mean(), ref_absmax=np.abs(ref).max(), n_dev=len(idx), n_ref=len(ridx),
         fragile=len(frag), identical=(dev == want), nan=int(np.isnan(s).sum()))
    assert not np.isnan(s).any()
    np.testing.assert_array_equal(idx, didx)
    np.testing.assert_allclose(sc, dsc, rtol=2e-6)
    assert err.max() <= tol, "log-assignment scores drifted from the fp32 oracle"
    assert len(ridx) >= min_matches, "the planted correspondences must come out as matches in the oracle"
    assert len(frag) <= max(2, int(len(ridx) * (0.02 if tol <= 0.05 else 0.06)))
    assert dev == want, f"match sets differ: device-only {sorted(dev - want)[:5]}, oracle-only {sorted(want - dev)[:5]}"
    # no blind exemption: every row the device decides differently from the oracle (fragile or not) has an oracle margin below twice the measured error
    from planted import decision_margins
    diff_rows = sorted({p[0] for p in {tuple(q) for q in idx} ^ {tuple(q) for q in ridx}})
    margins = decision_margins(ref)
    fin = np.isfinite(ref)
    emax = float(err[fin].max()) if fin.any() else 0.0
    assert all(margins[r] <= 2 * emax for r in diff_rows), f"unexplained decisions on rows {[r for r in diff_rows if margins[r] > 2 * emax]}"
    assert len(diff_rows) <= max(2, int(len(ridx) * (0.02 if tol <= 0.05 else 0.06)))
    # scores of the common matches agree as probabilities too
    common = sorted(dev & want)
    ds = {tuple(p): v for p, v in zip(idx, sc)}
    rs = {tuple(p): v for p, v in zip(ridx, rsc)}
    if common:
        assert max(abs(ds[c] - rs[c]) for c in common) <= 1.5 * tol


# A context picks the LightGlue block form by token count (fused lg_blockf_kernel from 3200 tokens, four launches below);
# airfe_tuning::fuse_lg_block forces either, so that both forms meet the oracle at every size.
FORMS = [{"fuse_lg_block": 1}, {"fuse_lg_block": 0}]


@pytest.mark.parametrize("mprec", [1, 0], ids=["fp16", "bf16"])
@pytest.mark.parametrize("env", FORMS, ids=["fused_block", "four_launches"])
@pytest.mark.parametrize("n0,n1,min_matches", [(400, 400, 150), (317, 400, 110), (64, 65, 20), (1, 5, 0), (2, 1, 0)])
def test_lightglue_scores_vs_oracle(n0, n1, min_matches, env, mprec):
    ctx, _, lg = context("lg", tuning=env, max_batch=4, matcher_precision=mprec)
    _, _, a, b = _pair(n0, n1, n0 * 3 + n1)
    s = ctx.lightglue_scores(a, b)
    ref = ref_nets.lightglue_forward(lg, a[:, :2], a[:, 2:], b[:, :2], b[:, 2:])
    idx, sc = ctx.match_lightglue(a, b)
    _check_against_oracle(f"lg_scores_{n0}_{n1}_{'fused' if env['fuse_lg_block'] == 1 else 'split'}_{'fp16' if mprec else 'bf16'}",
                          s, ref, idx, sc, TOL[mprec], min_matches)


@pytest.mark.parametrize("name", ["ties_threshold_inf_row", "all_minus_inf", "all_equal_below", "all_equal_above",
                                  "random_with_floor_nan", "single", "one_row"])
def test_filter_kernels_on_hand_built_scores(name):
    """lg_rowarg / lg_colarg / lg_filter straight on score matrices with ties, -inf rows, -FLT_MAX, NaN and values one ulp
    either side of log(0.1): must equal the oracle (itself pinned to the C++ loops in tests/test_structured_weights_cpu.py)."""
    from test_structured_weights_cpu import hand_built_score_matrices
    ctx, _, _ = context("lg", max_batch=4)
    s = hand_built_score_matrices()[name]
    idx, sc = ctx.debug_lg_filter(s)
    ridx, rsc = ref_post.filter_matches(s, 0.1)
    # float32 exp on the device vs numpy may differ in the last bit exactly AT the threshold; everywhere else bit-for-bit
    thr_rows = {i for i in range(s.shape[0]) if np.isfinite(s[i]).any() and abs(float(np.nanmax(s[i])) - math.log(0.1)) < 1e-6}
    keep = lambda pairs: [tuple(p) for p in pairs if p[0] not in thr_rows]
    assert keep(idx) == keep(ridx)
    m = {tuple(p): v for p, v in zip(ridx, rsc)}
    for p, v in zip(idx, sc):
        if tuple(p) in m and p[0] not in thr_rows:
            np.testing.assert_allclose(v, m[tuple(p)], rtol=2e-6)


def test_lightglue_layer_states_drift():
    """Where precision goes: score error with 1, 3, 9 layers (diagnostic, loose bound)."""
    from airslam_amd import weights
    from airslam_amd import api
    _, _, a, b = _pair(200, 180, 77)
    out = {}
    for L in (1, 3):
        w = weights.synthetic_lightglue(1234, n_layers=L)
        ctx = api.Context(lightglue=w, max_batch=2)
        s = ctx.lightglue_scores(a, b)
        ref = ref_nets.lightglue_forward(w, a[:, :2], a[:, 2:], b[:, :2], b[:, 2:], n_layers=L)
        out[f"L{L}_max_err"] = float(np.abs(s - ref).max())
        ctx.close()
    diag("lg_layers", **out)
    assert out["L1_max_err"] < 0.05


def test_match_batch_dev_equals_host_path():
    import torch
    from airslam_amd import api
    ctx, _, lg = context("lg", max_batch=4)
    pairs = [_pair(400, 380, 5), _pair(120, 400, 9)]
    f0 = torch.zeros((2, 400, 259)); f1 = torch.zeros((2, 400, 259))
    n0 = torch.tensor([400, 120], dtype=torch.int32); n1 = torch.tensor([380, 400], dtype=torch.int32)
    for i, (a, b, _, _) in enumerate(pairs):
        f0[i, :a.shape[0]] = torch.from_numpy(a); f1[i, :b.shape[0]] = torch.from_numpy(b)
    f0, f1, n0, n1 = f0.cuda(), f1.cuda(), n0.cuda(), n1.cuda()
    idx = torch.zeros((2, 400, 2), dtype=torch.int32, device="cuda")
    sc = torch.zeros((2, 400), dtype=torch.float32, device="cuda")
    nm = torch.zeros((2,), dtype=torch.int32, device="cuda")
    ctx.match_lightglue_batch_dev(f0, n0, f1, n1, idx, sc, nm)
    ctx.sync()
    pm = api.PointMatcher(ctx, 752, 480, 0)
    for i, (a, b, _, _) in enumerate(pairs):
        cnt, matches = pm.MatchingPoints(np.asfortranarray(a.T), np.asfortranarray(b.T))
        k = int(nm[i])
        assert k == cnt
        got = idx[i, :k].cpu().numpy()
        assert [tuple(g) for g in got] == [(m[0], m[1]) for m in matches]
        np.testing.assert_allclose(1.0 - sc[i, :k].cpu().numpy(), [m[2] for m in matches], atol=1e-6)


def test_matching_points_early_out():
    from airslam_amd import api
    ctx, _, _ = context("lg", max_batch=4)
    pm = api.PointMatcher(ctx, 752, 480, 0)
    assert pm.MatchingPoints(np.zeros((259, 0), np.float32), np.zeros((259, 7), np.float32)) == (0, [])


# which kernel the K = 256 projections of an 8-pair batch (6400 tokens) go through: the thresholds are lowered so that the
# large-batch kernels are exercised at a size the oracle-free comparison below finishes quickly
# (gemmr with 24 persistent workgroups instead of 256: 200 token tiles / 8 per feature group = 25 tiles per workgroup, so the
# 6- and 8-slot DMA rings wrap several times, as they do at 64 pairs on 256 workgroups)
BIG_GEMMS = {"gemm8": {"gemm8_min_m": 4096, "gemmr_min_m": 1000000000},
             "gemmr": {"gemm8_min_m": 4096, "gemmr_min_m": 1024},
             "gemmr_ring_wrap": {"gemm8_min_m": 4096, "gemmr_min_m": 1024, "gemmr_wgs": 24},
             "gemmr_two_launches": {"gemm8_min_m": 4096, "gemmr_min_m": 1024, "gemmr_wgs": 24, "qkv_pair": 0}}


@pytest.mark.parametrize("big", list(BIG_GEMMS))
@pytest.mark.parametrize("env", FORMS, ids=["fused_block", "four_launches"])
def test_large_batch_uses_gemm8_and_agrees_with_single_pair_path(env, big):
    """8 pairs -> M = 16 x 400 = 6400 rows: the linears go through the 8-wave LDS-DMA GEMM (kernels_gemm8.hip) or, where it
    applies (K = 256, no rotary), the register-resident streaming GEMM (kernels_gemmr.hip); a single pair (M = 896) goes
    through gemm_small_kernel.  Same K-order accumulation => same matches, with the block form held fixed (it is what
    changes the rounding points)."""
    import torch
    from airslam_amd import api
    ctx, _, lg = context("lg", tuning=dict(env, **BIG_GEMMS[big]), max_batch=8)
    B = 8
    pairs = [_pair(400 - 7 * i, 390 - 11 * i, 40 + i) for i in range(B)]
    f0 = torch.zeros((B, 400, 259)); f1 = torch.zeros((B, 400, 259))
    n0 = torch.tensor([p[0].shape[0] for p in pairs], dtype=torch.int32)
    n1 = torch.tensor([p[1].shape[0] for p in pairs], dtype=torch.int32)
    for i, (a, b, _, _) in enumerate(pairs):
        f0[i, :a.shape[0]] = torch.from_numpy(a); f1[i, :b.shape[0]] = torch.from_numpy(b)
    f0, f1, n0, n1 = f0.cuda(), f1.cuda(), n0.cuda(), n1.cuda()
    idx = torch.zeros((B, 400, 2), dtype=torch.int32, device="cuda")
    sc = torch.zeros((B, 400), dtype=torch.float32, device="cuda")
    nm = torch.zeros((B,), dtype=torch.int32, device="cuda")
    ctx.match_lightglue_batch_dev(f0, n0, f1, n1, idx, sc, nm)
    ctx.sync()
    pm = api.PointMatcher(ctx, 752, 480, 0)
    for i, (a, b, _, _) in enumerate(pairs):
        cnt, matches = pm.MatchingPoints(np.asfortranarray(a.T), np.asfortranarray(b.T))
        k = int(nm[i])
        assert k == cnt
        assert [tuple(g) for g in idx[i, :k].cpu().numpy()] == [(m[0], m[1]) for m in matches]
        np.testing.assert_allclose(1.0 - sc[i, :k].cpu().numpy(), [m[2] for m in matches], atol=1e-5)


def test_block_form_switch_by_token_count_keeps_the_matches():
    """Switch point lowered to 4096 tokens: 1 pair (800 tokens) runs the four-launch block through gemm_small_kernel,
    8 pairs (6400 tokens) the fused kernel + gemm_kernel.  The two block forms round at different points, so scores agree
    to bf16 noise and the match sets almost entirely."""
    import torch
    from airslam_amd import api
    ctx, _, lg = context("lg", tuning={"block_min_m": 4096}, max_batch=8)
    B = 8
    pairs = [_pair(400 - 7 * i, 390 - 11 * i, 140 + i) for i in range(B)]
    f0 = torch.zeros((B, 400, 259)); f1 = torch.zeros((B, 400, 259))
    n0 = torch.tensor([p[0].shape[0] for p in pairs], dtype=torch.int32)
    n1 = torch.tensor([p[1].shape[0] for p in pairs], dtype=torch.int32)
    for i, (a, b, _, _) in enumerate(pairs):
        f0[i, :a.shape[0]] = torch.from_numpy(a); f1[i, :b.shape[0]] = torch.from_numpy(b)
    f0, f1, n0, n1 = f0.cuda(), f1.cuda(), n0.cuda(), n1.cuda()
    idx = torch.zeros((B, 400, 2), dtype=torch.int32, device="cuda")
    sc = torch.zeros((B, 400), dtype=torch.float32, device="cuda")
    nm = torch.zeros((B,), dtype=torch.int32, device="cuda")
    ctx.match_lightglue_batch_dev(f0, n0, f1, n1, idx, sc, nm)
    ctx.sync()
    pm = api.PointMatcher(ctx, 752, 480, 0)
    agree = []
    for i, (a, b, _, _) in enumerate(pairs):
        cnt, matches = pm.MatchingPoints(np.asfortranarray(a.T), np.asfortranarray(b.T))
        batch = {tuple(g) for g in idx[i, :int(nm[i])].cpu().numpy()}
        single = {(m[0], m[1]) for m in matches}
        agree.append(len(batch & single) / max(len(batch | single), 1))
    diag("lg_block_form_switch", min_agreement=min(agree), mean_agreement=float(np.mean(agree)))
    assert min(agree) >= 0.95


@pytest.mark.parametrize("n0,n1,min_matches", [(1024, 1024, 400), (1024, 777, 300)])
def test_lightglue_at_the_profile_maximum(n0, n1, min_matches):
    """N = 1024 is the engine's optimisation-profile maximum (light_glue.cpp:52); the arena is sized by max_keypoints."""
    from airslam_amd import api, weights
    lg = weights.synthetic_lightglue(1234)
    ctx = api.Context(lightglue=lg, max_batch=2, max_keypoints=1024)
    _, _, a, b = _pair(n0, n1, 1024 + n1)
    s = ctx.lightglue_scores(a, b)
    ref = ref_nets.lightglue_forward(lg, a[:, :2], a[:, 2:], b[:, :2], b[:, 2:])
    idx, sc = ctx.match_lightglue(a, b)
    assert s.shape == (n0, n1)
    _check_against_oracle(f"lg_max_{n0}_{n1}", s, ref, idx, sc, TOL[1], min_matches)
    ctx.close()


def test_bench_size_matcher_batch_repeats_its_distinct_pairs():
    """64 pairs per call (the bench workload: 51200 tokens, the gemmr rings wrap 13 times, 400 block tiles on 256 CUs) = 4 distinct
    planted pairs x 16: every copy must equal its original, and both must equal the 4-pair call of a small context, bit for bit."""
    import torch
    big, _, _ = context("lg", max_batch=128)
    small, _, _ = context("lg", max_batch=8)
    pairs = [_pair(400 - 9 * i, 397 - 13 * i, 300 + 7 * i) for i in range(4)]

    def run(ctx, reps):
        B = 4 * reps
        f0 = torch.zeros((B, 400, 259)); f1 = torch.zeros((B, 400, 259))
        n0 = torch.zeros((B,), dtype=torch.int32); n1 = torch.zeros((B,), dtype=torch.int32)
        for i in range(B):
            a, b, _, _ = pairs[i % 4]
            f0[i, :a.shape[0]] = torch.from_numpy(a); f1[i, :b.shape[0]] = torch.from_numpy(b)
            n0[i] = a.shape[0]; n1[i] = b.shape[0]
        f0, f1, n0, n1 = f0.cuda(), f1.cuda(), n0.cuda(), n1.cuda()
        idx = torch.zeros((B, 400, 2), dtype=torch.int32, device="cuda")
        sc = torch.zeros((B, 400), dtype=torch.float32, device="cuda")
        nm = torch.zeros((B,), dtype=torch.int32, device="cuda")
        ctx.match_lightglue_batch_dev(f0, n0, f1, n1, idx, sc, nm)
        ctx.sync()
        return idx.cpu().numpy(), sc.cpu().numpy(), nm.cpu().numpy()

    ridx, rsc, rnm = run(small, 1)
    oidx, osc, onm = run(big, 16)
    diag("lg_bench_size_repeats", matches=str(rnm.tolist()))
    assert rnm.min() >= 150                         # the planted correspondences do produce matches: ~200 per pair
    for i in range(64):
        j, m = i % 4, int(rnm[i % 4])
        assert int(onm[i]) == m
        np.testing.assert_array_equal(oidx[i, :m], ridx[j, :m])
        np.testing.assert_array_equal(osc[i, :m], rsc[j, :m])


@pytest.mark.parametrize("env", [{"fuse_lg_block": 1, "gemmr_min_m": 512}, {"fuse_lg_block": 0}],
                         ids=["fused_block_gemmr", "four_launches"])
def test_lightglue_bf16_storage(env):
    """matcher_precision = 0 (bf16 operands, fp32 accumulate) through the same kernels: the PBF16 instantiations of lg_blockf_kernel,
    gemmr_kernel / gemmr_pair_kernel and gemm_small_kernel (the default matcher storage is fp16, tested above).  Three fewer mantissa
    bits: ~8x the score error; the match set still has to be the oracle's outside the rows the oracle decides within that error."""
    ctx, _, lg = context("lg", tuning=env, max_batch=4, matcher_precision=0)
    _, _, a, b = _pair(400, 371, 4242)
    s = ctx.lightglue_scores(a, b)
    ref = ref_nets.lightglue_forward(lg, a[:, :2], a[:, 2:], b[:, :2], b[:, 2:])
    idx, sc = ctx.match_lightglue(a, b)
    _check_against_oracle(f"lg_bf16_{'fused' if env['fuse_lg_block'] == 1 else 'split'}", s, ref, idx, sc, TOL[0], 150)


def test_folded_projections_give_the_same_bits():
    """The fused block computes the NEXT attention layer's q | k | v projections from its own result (kernels_lgblockf.hip, FOLD);
    airfe_tuning::fold_qkv = 0 runs them as launches of their own (gemmr_pair / the tiled kernels).  Same fragments, same K order, bias after
    the sum, same rotary: the matches AND the scores must be bit-identical, at a size with a ragged last pass (8 pairs x 400 rows =
    6400 tokens = 57.1 passes of 112) and with short sequences (rows beyond a sequence's length are computed, stored and masked)."""
    import torch
    outs = []
    for fold in (1, 0):
        ctx, _, lg = context("lg", tuning={"fuse_lg_block": 1, "fold_qkv": fold}, max_batch=8)
        B = 8
        pairs = [_pair(400 - 31 * i, 390 - 17 * i, 240 + i) for i in range(B)]
        f0 = torch.zeros((B, 400, 259)); f1 = torch.zeros((B, 400, 259))
        n0 = torch.tensor([p[0].shape[0] for p in pairs], dtype=torch.int32)
        n1 = torch.tensor([p[1].shape[0] for p in pairs], dtype=torch.int32)
        for i, (a, b, _, _) in enumerate(pairs):
            f0[i, :a.shape[0]] = torch.from_numpy(a); f1[i, :b.shape[0]] = torch.from_numpy(b)
        f0, f1, n0, n1 = f0.cuda(), f1.cuda(), n0.cuda(), n1.cuda()
        idx = torch.zeros((B, 400, 2), dtype=torch.int32, device="cuda")
        sc = torch.zeros((B, 400), dtype=torch.float32, device="cuda")
        nm = torch.zeros((B,), dtype=torch.int32, device="cuda")
        ctx.match_lightglue_batch_dev(f0, n0, f1, n1, idx, sc, nm)
        ctx.sync()
        outs.append((nm.cpu().numpy().copy(), idx.cpu().numpy().copy(), sc.cpu().numpy().copy()))
    (nm_a, idx_a, sc_a), (nm_b, idx_b, sc_b) = outs
    assert nm_a.min() >= 50
    np.testing.assert_array_equal(nm_a, nm_b)
    for i in range(len(nm_a)):
        np.testing.assert_array_equal(idx_a[i, :nm_a[i]], idx_b[i, :nm_b[i]])
        np.testing.assert_array_equal(sc_a[i, :nm_a[i]], sc_b[i, :nm_b[i]])


@pytest.mark.parametrize("form", [{"fuse_lg_block": 1}, {"fuse_lg_block": 1, "lgb_tokens": 32}, {"fuse_lg_block": 0}], ids=["fused112", "fused32", "split"])
def test_out_projection_folded_into_ffn0_gives_the_bits_of_the_identity_form(form):
    """airfe_tuning::fold_out_proj (the default): the loader multiplies out_proj / to_out into the message half of ffn.0 (airfe_load.hip make_ffn0_folded) and
    the block runs ffn.0 on cat(x, attention output).  Pinned two ways: (1) every oracle test of this file runs the folded form (the default) against the fp32
    oracle of the ORIGINAL weights; (2) here: weights.fold_out_proj is the same fold in Python with the out-projection replaced by the identity — a context that
    still runs the out-projection GEMM (fold_out_proj = 0) on THAT pack computes msg = I a = a exactly, so it must return the bits of the folded context on the
    original pack: same packed ffn.0 slabs (the loader's fold == the Python fold, bit for bit) and the same K order in the kernel."""
    import torch
    from airslam_amd import api, weights
    w = weights.synthetic_lightglue(1234)
    outs = []
    for pack, fold in ((w, 1), (weights.fold_out_proj(w), 0)):
        ctx = api.Context(lightglue=pack, max_batch=8, tuning=dict(form, fold_out_proj=fold), check_launches=1)
        B = 8
        pairs = [_pair(400 - 31 * i, 390 - 17 * i, 640 + i) for i in range(B)]
        f0 = torch.zeros((B, 400, 259)); f1 = torch.zeros((B, 400, 259))
        n0 = torch.tensor([p[0].shape[0] for p in pairs], dtype=torch.int32)
        n1 = torch.tensor([p[1].shape[0] for p in pairs], dtype=torch.int32)
        for i, (a, b, _, _) in enumerate(pairs):
            f0[i, :a.shape[0]] = torch.from_numpy(a); f1[i, :b.shape[0]] = torch.from_numpy(b)
        f0, f1, n0, n1 = f0.cuda(), f1.cuda(), n0.cuda(), n1.cuda()
        idx = torch.zeros((B, 400, 2), dtype=torch.int32, device="cuda")
        sc = torch.zeros((B, 400), dtype=torch.float32, device="cuda")
        nm = torch.zeros((B,), dtype=torch.int32, device="cuda")
        ctx.match_lightglue_batch_dev(f0, n0, f1, n1, idx, sc, nm)
        ctx.sync()
        a0, b0 = pairs[0][2], pairs[0][3]
        outs.append((nm.cpu().numpy().copy(), idx.cpu().numpy().copy(), sc.cpu().numpy().copy(), ctx.lightglue_scores(a0, b0).copy()))
        ctx.close()
    (nm_a, idx_a, sc_a, s_a), (nm_b, idx_b, sc_b, s_b) = outs
    assert nm_a.min() >= 50
    np.testing.assert_array_equal(nm_a, nm_b)
    for i in range(len(nm_a)):
        np.testing.assert_array_equal(idx_a[i, :nm_a[i]], idx_b[i, :nm_b[i]])
        np.testing.assert_array_equal(sc_a[i, :nm_a[i]], sc_b[i, :nm_b[i]])
    np.testing.assert_array_equal(s_a, s_b)                  # the whole log-assignment matrix of pair 0, batch-1 path (32-token passes)


def test_two_round_pass_split_gives_the_bits_of_uniform_passes():
    """Round 5: when a launch of the fused block would be one full round of 112-token passes plus a partial second round, the second round runs 96-token passes so
    that every CU gets 13 token tiles instead of 14 or 7 (kernels_lgblockf.hip lg_blockf_mixed_kernel; the library's own choice, `lgb_tokens = 112` forces uniform
    passes).  Which pass a token rides in must not change its result: 40 pairs (32000 tokens = 256 passes of 7 tiles + 36 of 6, the last one ragged) both ways."""
    import torch
    from airslam_amd import api, weights
    B = 40
    pairs = [_pair(400 - 7 * (i % 9), 396 - 5 * (i % 7), 900 + i) for i in range(B)]
    f0 = torch.zeros((B, 400, 259)); f1 = torch.zeros((B, 400, 259))
    n0 = torch.tensor([p[0].shape[0] for p in pairs], dtype=torch.int32)
    n1 = torch.tensor([p[1].shape[0] for p in pairs], dtype=torch.int32)
    for i, (a, b, _, _) in enumerate(pairs):
        f0[i, :a.shape[0]] = torch.from_numpy(a); f1[i, :b.shape[0]] = torch.from_numpy(b)
    f0, f1, n0, n1 = f0.cuda(), f1.cuda(), n0.cuda(), n1.cuda()
    outs = []
    for tun in (None, {"lgb_tokens": 112}):
        ctx = api.Context(lightglue=weights.synthetic_lightglue(1234), max_batch=B, tuning=tun, check_launches=1)
        idx = torch.zeros((B, 400, 2), dtype=torch.int32, device="cuda")
        sc = torch.zeros((B, 400), dtype=torch.float32, device="cuda")
        nm = torch.zeros((B,), dtype=torch.int32, device="cuda")
        for _ in range(2):                                   # (twice: the slack rows a ragged last pass writes must not leak into the next call)
            ctx.match_lightglue_batch_dev(f0, n0, f1, n1, idx, sc, nm)
        ctx.sync()
        outs.append((nm.cpu().numpy().copy(), idx.cpu().numpy().copy(), sc.cpu().numpy().copy()))
        ctx.close()
    (nm_a, idx_a, sc_a), (nm_b, idx_b, sc_b) = outs
    assert nm_a.min() >= 50
    np.testing.assert_array_equal(nm_a, nm_b)
    for i in range(B):
        np.testing.assert_array_equal(idx_a[i, :nm_a[i]], idx_b[i, :nm_b[i]])
        np.testing.assert_array_equal(sc_a[i, :nm_a[i]], sc_b[i, :nm_b[i]])


def test_match_scores_are_glibc_expf_bit_for_bit():
    """The match score the reference returns is `std::exp(score)` on the host (src/light_glue.cpp:248): glibc's expf, a 0.502-ulp routine — NOT the correctly
    rounded value (they differ on 0.063 % of all inputs, tools/expf_glibc_check.c), which is what the device computed in rounds 3-4 and what made the
    exact-equality pin against the compiled reference a coin that happened to fall right (tests/test_gpu_ref_pin.py: ~200 scores per pair).  The device now
    restates glibc's algorithm operation by operation (common.h expf_like_glibc); here ~20000 scores over the whole range a kept match can have,
    (log 0.1, 0], against the host's libm, bit for bit (the old form would miss about a dozen of them)."""
    from airslam_amd import api, weights
    from conftest import skip_unless_host_expf_is_glibc
    skip_unless_host_expf_is_glibc()
    ctx = api.Context(lightglue=weights.synthetic_lightglue(1234, n_layers=1), max_batch=2, max_keypoints=1024)
    rng = np.random.default_rng(5)
    n, total = 1024, 0
    for rep in range(20):
        s = np.full((n, n), -50.0, np.float32)
        v = (-rng.uniform(0.0, 2.30, n)).astype(np.float32)
        if rep == 0:
            v[:8] = np.float32([0.0, -0.0, -1e-8, -2.3025851, -2.302585, -1.0, -0.6931472, -1.4012985e-45])      # exact 1, the threshold's neighbours, a subnormal argument
        perm = rng.permutation(n)
        s[np.arange(n), perm] = v                                   # one mutual maximum per row and column
        idx, sc = ctx.debug_lg_filter(s)
        assert len(idx) >= n - 4 and np.array_equal(idx[:, 1], perm[idx[:, 0]])
        want = ref_post._expf(v[idx[:, 0]])
        np.testing.assert_array_equal(sc.view(np.uint32), np.asarray(want, np.float32).view(np.uint32))
        total += len(idx)
    assert total >= 20000
    ctx.close()


def test_slack_rows_are_reset_on_every_call():
    """the matcher arena's surplus token rows behind the last sequence go through every block like real tokens; their
    residual stream must start from ZERO on every call (it used to keep growing from call to call on the 2-byte path — NaN in the last pair after
    tens of thousands of steps).  airfe_debug_trace reads the rows as a call starts and as it leaves them."""
    import numpy as np
    from airslam_amd import api, weights
    from planted import planted_pair
    lg = weights.synthetic_lightglue(1234)
    ctx = api.Context(lightglue=lg, max_batch=2, max_keypoints=400)
    from planted import normalised
    f0, f1 = planted_pair(400, 400, 7)
    a, b = normalised(f0)[:, 1:], normalised(f1)[:, 1:]            # [n, 258] rows: normalised x, y + descriptors
    ctx.trace(True)
    try:
        for call in range(4):
            ctx.trace_stop(-1)
            ctx.match_lightglue(a, b)
            names = [t[0] for t in ctx.trace_slots()]
            end = ctx.trace_buffer([i for i, n in enumerate(names) if n.endswith("final.x32slack")][0], np.float32)
            assert np.isfinite(end).all() and np.abs(end).max() > 0, "the slack rows are expected to be touched by the blocks (else this test tests nothing)"
            ctx.trace_stop(names.index("L0.prep.x32slack"))      # run only up to the prepare launch of the NEXT call and look at the rows
            ctx.match_lightglue(a, b)
            start = ctx.trace_buffer(names.index("L0.prep.x32slack"), np.float32)
            assert not start.any(), f"call {call}: slack rows enter the forward with a residual of up to {np.abs(start).max()}"
    finally:
        ctx.trace_stop(-1)
        ctx.trace(False)
        ctx.close()


def test_fused_block_tile_sizes_give_the_same_bits():
    """lg_blockf picks 32-token passes up to 8192 tokens, 64 up to 16384, else 112 / 128 (round 4: the batch-1 .. batch-16 calls), and the small tiles
    keep all weight slabs of a GEMM in flight.  A token's arithmetic does not depend on the tile it sits in: every tile size must give the SAME BITS
    (airfe_tuning::lgb_tokens forces one)."""
    _, _, a, b = _pair(400, 317, 11)
    ref = None
    for tokens in (32, 64, 112, 128):
        ctx, _, _ = context("lg", tuning={"fuse_lg_block": 1, "lgb_tokens": tokens}, max_batch=4)
        s = ctx.lightglue_scores(a, b)
        idx, sc = ctx.match_lightglue(a, b)
        if ref is None:
            ref = (s, idx, sc)
            assert len(idx) >= 100
        else:
            np.testing.assert_array_equal(s, ref[0])
            np.testing.assert_array_equal(idx, ref[1])
            np.testing.assert_array_equal(sc, ref[2])


@pytest.mark.parametrize("n0,n1", [(400, 400), (317, 400), (64, 65), (1, 5), (2, 1), (1024, 777), (129, 63)])
def test_assignment_without_the_similarity_matrix_keeps_the_matches(n0, n1):
    """Round 5: log-sum-exp and arg-max partials are taken inside the similarity tiles (airfe_tuning::assign_fused = 1; kernels_lg.hip) instead of
    writing sim [B][Np][Np] and reading it four times (selectable; the library default is assign_fused = 0: profiles/r05_assign_ab.txt).  The log-sum-exp is then a sum of per-tile sums with hardware exponentials: the scores may move in their
    last bits against the round-2 form, the match LISTS may not (outside rows whose decision sits within 1e-4 of a boundary — none in these inputs), and the
    scores the kernel hands out are the ones its own arg-max saw (filter_matches of them reproduces the list exactly)."""
    _, _, a, b = _pair(n0, n1, 500 + n0 + n1)
    K = 1024 if max(n0, n1) > 400 else 400
    outs = []
    for fused in (1, 0):
        ctx, _, _ = context("lg", tuning={"assign_fused": fused}, max_batch=2, max_keypoints=K)
        s = ctx.lightglue_scores(a, b)
        idx, sc = ctx.match_lightglue(a, b)
        didx, dsc = ref_post.filter_matches(s, 0.1)
        np.testing.assert_array_equal(idx, didx)
        np.testing.assert_allclose(sc, dsc, rtol=2e-6)
        outs.append((s, idx, sc))
    (s1, i1, c1), (s0, i0, c0) = outs
    d = float(np.abs(s1 - s0)[np.isfinite(s0)].max()) if np.isfinite(s0).any() else 0.0
    diag(f"lg_assign_fused_vs_matrix_{n0}_{n1}", max_score_diff=d, matches=len(i1), identical=bool(np.array_equal(i1, i0)))
    assert d <= 2e-4
    np.testing.assert_array_equal(i1, i0)
    np.testing.assert_allclose(c1, c0, rtol=3e-4)


def test_assignment_partials_cover_a_batch_of_ragged_pairs():
    """8 pairs of different lengths in one call (tiles with no valid row / column, sequences shorter than a tile): the batch entry's lists equal the
    single-pair calls' in both assignment forms."""
    import torch
    for fused in (1, 0):
        ctx, _, _ = context("lg", tuning={"assign_fused": fused}, max_batch=8)
        B = 8
        lens = [(400, 400), (1, 400), (400, 1), (63, 65), (64, 64), (129, 200), (399, 17), (5, 5)]
        pairs = [_pair(n0, n1, 900 + i) for i, (n0, n1) in enumerate(lens)]
        f0 = torch.zeros((B, 400, 259)); f1 = torch.zeros((B, 400, 259))
        n0t = torch.tensor([p[0].shape[0] for p in pairs], dtype=torch.int32); n1t = torch.tensor([p[1].shape[0] for p in pairs], dtype=torch.int32)
        for i, p in enumerate(pairs):
            f0[i, :p[0].shape[0]] = torch.from_numpy(p[0]); f1[i, :p[1].shape[0]] = torch.from_numpy(p[1])
        idx = torch.zeros((B, 400, 2), dtype=torch.int32).cuda(); sc = torch.zeros((B, 400)).cuda(); nm = torch.zeros((B,), dtype=torch.int32).cuda()
        ctx.match_lightglue_batch_dev(f0.cuda(), n0t.cuda(), f1.cuda(), n1t.cuda(), idx, sc, nm)
        ctx.sync()
        for i, p in enumerate(pairs):
            want_idx, want_sc = ctx.match_lightglue(p[2], p[3])
            k = int(nm[i])
            assert k == len(want_idx), (fused, i, k, len(want_idx))
            np.testing.assert_array_equal(idx[i, :k].cpu().numpy(), want_idx)
            np.testing.assert_array_equal(sc[i, :k].cpu().numpy(), want_sc)


def test_empty_frames_in_a_batch_have_no_matches():
    """A frame without detections reaches the matcher (the batch entry reads the counts on the device: there is no host-side early-out): a pair with an empty
    right or an empty left frame reports no match in either assignment form (include/airfe.h; the reference returns before its engine: point_matcher.cc:53-55),
    and the pairs around it are what they are alone."""
    import torch
    lens = [(129, 200), (200, 0), (0, 150), (65, 97)]
    B = len(lens)
    for fused in (1, 0):
        ctx, _, _ = context("lg", tuning={"assign_fused": fused}, max_batch=8)
        pairs = [_pair(max(n0, 1), max(n1, 1), 950 + i) for i, (n0, n1) in enumerate(lens)]
        f0 = torch.zeros((B, 400, 259)); f1 = torch.zeros((B, 400, 259))
        for i, (p, (n0, n1)) in enumerate(zip(pairs, lens)):
            f0[i, :n0] = torch.from_numpy(p[0][:n0]); f1[i, :n1] = torch.from_numpy(p[1][:n1])
        n0t = torch.tensor([l[0] for l in lens], dtype=torch.int32); n1t = torch.tensor([l[1] for l in lens], dtype=torch.int32)
        idx = torch.zeros((B, 400, 2), dtype=torch.int32).cuda(); sc = torch.zeros((B, 400)).cuda(); nm = torch.full((B,), -1, dtype=torch.int32).cuda()
        ctx.match_lightglue_batch_dev(f0.cuda(), n0t.cuda(), f1.cuda(), n1t.cuda(), idx, sc, nm)
        ctx.sync()
        assert nm.cpu().tolist()[1:3] == [0, 0], (fused, nm.cpu().tolist(), idx[1:3, :1].cpu().tolist(), sc[1:3, :1].cpu().tolist())
        assert not idx[1:3].any() and not sc[1:3].any()
        for i in (0, 3):
            want_idx, want_sc = ctx.match_lightglue(pairs[i][2], pairs[i][3])
            k = int(nm[i])
            assert k == len(want_idx) and k > 0, (fused, i, k, len(want_idx))
            np.testing.assert_array_equal(idx[i, :k].cpu().numpy(), want_idx)
            np.testing.assert_array_equal(sc[i, :k].cpu().numpy(), want_sc)


# ---- the fault-hunting trace's slot names, their order and the groups a trace_stop cuts at (airfe_match.hip: lightglue_dev, attn_block_dev)
def _trace_groups(L, fused, fold_qkv, fold_out):
    """The slot names of one traced LightGlue call, in groups: a trace_stop inside a group takes effect at the group's end.  2 L half-steps, half-step h cross iff
    h & 1, block of layer h // 2: it launches its own projections unless an earlier fused block carried them (fold and h > 0); its fused block carries the projections
    of half-step h + 1 (k only for a self half); the separate launches trace the out-projection's message unless it is folded into ffn.0 (either half)."""
    fold = fused and fold_qkv
    groups = [["L0.prep.x32", "L0.prep.xb", "L0.prep.x32slack", "L0.prep.rc", "L0.prep.rs"]]
    for h in range(2 * L):
        cross = h & 1
        p = f"L{h // 2}.{'cross' if cross else 'self'}"
        if not fold or h == 0:
            groups.append([p + ".qkv.q"] + ([] if cross else [p + ".qkv.k"]) + [p + ".qkv.vt"])
        groups.append([p + ".attn.o"])
        if fused:
            groups.append([p + ".block.x32", p + ".block.xb"])
            if fold and h + 1 < 2 * L:
                groups.append([p + ".block.q"] + ([p + ".block.k"] if cross else []) + [p + ".block.vt"])
        else:
            if not fold_out:
                groups.append([p + ".out.msg"])
            groups.append([p + ".ffn.x32", p + ".ffn.xb"])
    groups.append([f"L{L}.final.md", f"L{L}.final.x32slack"])
    return groups + [[f"L{L}.{n}"] for n in ("final.z", "final.sim", "assign.rowlse", "assign.collse", "assign.rowval", "assign.rowarg", "assign.colarg")]


def _traced_context(tuning):
    from airslam_amd import api, weights
    ctx = api.Context(lightglue=weights.synthetic_lightglue(1234, n_layers=2), max_batch=2, max_keypoints=400, tuning=tuning)
    _, _, a, b = _pair(129, 63, 3232)
    ctx.trace(True)
    return ctx, a, b


@pytest.mark.parametrize("tuning", [None, {"fuse_lg_block": 0}, {"fold_qkv": 0}, {"fuse_lg_block": 0, "fold_out_proj": 0}],
                         ids=["default", "four_launches", "own_projections", "four_launches_out_proj"])
def test_trace_slot_names_and_order(tuning):
    t = tuning or {}
    want = sum(_trace_groups(2, t.get("fuse_lg_block", 1) == 1, t.get("fold_qkv", 1) == 1, t.get("fold_out_proj", 1) == 1), [])
    ctx, a, b = _traced_context(tuning)
    try:
        ctx.match_lightglue(a, b)
        assert [s[0] for s in ctx.trace_slots()] == want
        dig, _ = ctx.trace_read()
        assert len(dig) == len(want)
    finally:
        ctx.trace(False)
        ctx.close()


def test_trace_stop_cuts_at_the_end_of_the_slot_group():
    """trace_stop(k): the next call returns behind the GROUP of slots k lies in (the launches up to there have run, nothing after them), through trace_finish — the
    digests of the slots it did record can be read.  One slot per group, the group's first: the rest of its group must still be recorded."""
    groups = _trace_groups(2, True, True, True)
    full = sum(groups, [])
    ctx, a, b = _traced_context(None)
    try:
        ctx.match_lightglue(a, b)
        assert [s[0] for s in ctx.trace_slots()] == full
        end = 0
        for g in groups:
            k, end = end, end + len(g)
            ctx.trace_stop(k)
            ctx.match_lightglue(a, b)
            assert [s[0] for s in ctx.trace_slots()] == full[:end], (k, full[k])
            dig, _ = ctx.trace_read()
            assert len(dig) == end
    finally:
        ctx.trace_stop(-1)
        ctx.trace(False)
        ctx.close()
