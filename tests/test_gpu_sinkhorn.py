"""launch_sg_sinkhorn alone (airfe_debug_sg_sinkhorn) against the float64 log_optimal_transport of tests/sinkhorn_ref.py on the SAME float32 couplings, one form at a
time: the register-resident cooperative kernel in both instantiations (sg_sinkhorn_reg_kernel<13, 7> at max_keypoints 400, <9, 17> at 1024) and the per-half-iteration
kernels (forced at 400 / 1024, the only form at 256).  The SuperGlue parity tests reach this code only behind a 2-byte GNN whose error their gates must absorb
(0.05 on Z); here the gate of every case is 8 x its float32 floor: e32 = max|Z32 - Z64| of the reference's own float32 run, not below one float32 ulp of max|Z64|.
The 8 covers what a numpy float32 run does not have: another summation order, and the device's __expf = exp2(x log2 e) whose product rounding is worth |x| 2^-24
relative on terms that still matter at |x| ~ 16.  The hook starts every launch with NaN everywhere outside the pairs' valid blocks and in the whole output, so
"finite" also means "read nothing outside lens, wrote every element".  The measured multiples of e32 are tabulated in DESIGN.md §2a."""
import numpy as np
import pytest

import sinkhorn_ref
from airslam_amd import api, weights
from gpu_common import diag

pytestmark = pytest.mark.gpu
_C = {}
_REF = {}
CONTEXTS = {400: dict(max_keypoints=400, max_batch=8), 1024: dict(max_keypoints=1024, max_batch=8), 256: dict(max_keypoints=256, max_batch=2)}
REG_FORM = {400: 2, 1024: 3}                  # form_ran of the register-resident instantiation each context must get
FORMS = [(400, 1), (400, 2), (1024, 1), (1024, 2), (256, 1)]
ALPHA = 2.3457                                # the dead-code default of src/super_glue.cpp; the wide family uses 10


def _ctx(k):
    if k not in _C:
        _C[k] = api.Context(superglue=weights.synthetic_superglue(1234, n_layers=2), matcher=1, sinkhorn_iters=100, **CONTEXTS[k])       # only the arena matters
    return _C[k]


def _case(n0, n1, scale=8.0, alpha=ALPHA, kind="normal"):
    return (n0, n1, scale, alpha, kind)


def _reference(case, iters):
    """(couplings, Z64, e32, gate) of a case, computed once"""
    key = case + (iters,)
    if key not in _REF:
        n0, n1, scale, alpha, kind = case
        s = np.full((n0, n1), scale, np.float32) if kind == "constant" else sinkhorn_ref.couplings(n0, n1, 7919 * n0 + n1 + int(scale), scale)
        z64 = sinkhorn_ref.log_optimal_transport(s, alpha, iters)
        z32 = sinkhorn_ref.log_optimal_transport(s, alpha, iters, dtype=np.float32)
        e32 = float(np.abs(z32.astype(np.float64) - z64).max())
        _REF[key] = (s, z64, e32, 8.0 * max(e32, 2.0 ** -23 * float(np.abs(z64).max())))
    return _REF[key]


def _run(k, form, cases, iters, tag, expect_ran=None):
    """one launch on the batch `cases`; every pair against float64 (values, finiteness, column marginals).  -> list of Z"""
    refs = [_reference(c, iters) for c in cases]
    alphas = {c[3] for c in cases}
    assert len(alphas) == 1
    zs, ran = _ctx(k).debug_sg_sinkhorn([r[0] for r in refs], alphas.pop(), iters, form)
    want = expect_ran if expect_ran is not None else (1 if form == 1 else REG_FORM[k])
    assert ran == want, (tag, "form_ran", ran)
    bad = []
    for b, (c, (s, z64, e32, gate), z) in enumerate(zip(cases, refs, zs)):
        n0, n1 = c[0], c[1]
        assert z.shape == (n0 + 1, n1 + 1) and z.dtype == np.float32
        finite = bool(np.isfinite(z).all())
        err = float(np.abs(z.astype(np.float64) - z64).max()) if finite else float("inf")
        merr = mgate = 0.0
        if iters >= 1 and finite:
            mass = sinkhorn_ref.column_mass(n0, n1)
            merr = float((np.abs(np.exp(z.astype(np.float64)).sum(0) - mass) / mass).max())
            mgate = float(np.expm1(gate)) + 1e-12          # |dZ| <= gate on every entry of a column moves its sum by at most the factor e^gate (the reference's own: 1e-15)
        diag(f"sinkhorn_{k}_f{form}_{tag}_{b}_{n0}x{n1}_x{c[2]:g}_{c[4]}_it{iters}", form_ran=ran, B=len(cases), err=err, e32=e32, err_over_e32=err / max(e32, 1e-300),
             gate=gate, zmax=float(np.abs(z64).max()), marg_err=merr, marg_gate=mgate, finite=finite)
        if not finite or err > gate or merr > mgate:
            bad.append((tag, b, c, iters, "finite", finite, "err", err, "gate", gate, "e32", e32, "marginal", merr, mgate))
    assert not bad, bad
    return zs


LENGTHS = {400: [(400, 400), (400, 317), (33, 400), (1, 1), (1, 400), (400, 1), (2, 3), (65, 97), (104, 105), (105, 104)],
           1024: [(1024, 1000), (1, 1024), (1000, 63), (72, 73)],
           256: [(256, 256), (256, 200), (1, 1), (1, 256), (256, 1), (2, 3), (65, 97)]}


@pytest.mark.parametrize("k,form,n0,n1", [(k, f, n0, n1) for k, f in FORMS for n0, n1 in LENGTHS[k]])
def test_lengths_vs_float64(k, form, n0, n1):
    """full, ragged and degenerate lengths at the production iteration count: slices without rows ((2, 3): n0 + 1 < G), one row / one column against a full other
    side, the masks of the last column block, the rper slice boundary ((104, 105) / (105, 104))"""
    _run(k, form, [_case(n0, n1)], 100, "len")


@pytest.mark.parametrize("k,form", FORMS)
def test_wide_couplings_vs_float64(k, form):
    """normal x 25 with the planted diagonal: |Z| ~ 200, every exp argument far below zero except the matches"""
    n0, n1 = {400: (400, 389), 1024: (1000, 1024), 256: (256, 200)}[k]
    _run(k, form, [_case(n0, n1, 25.0, 10.0)], 100, "wide")


@pytest.mark.parametrize("k,form", FORMS)
def test_constant_couplings_have_the_closed_form(k, form):
    """all couplings and the dustbin score equal (every entry ties in every maximum): Z[i][j] = log_mu[i] + log_nu[j] - norm after the first iteration, for good"""
    n0, n1 = {400: (400, 317), 1024: (1024, 1000), 256: (256, 131)}[k]
    c = _case(n0, n1, 3.0, 3.0, "constant")
    for iters in (1, 5):
        z = _run(k, form, [c], iters, "const")[0]
        norm = -np.log(n0 + n1)
        log_mu = np.full(n0 + 1, norm); log_mu[n0] = np.log(n1) + norm
        log_nu = np.full(n1 + 1, norm); log_nu[n1] = np.log(n0) + norm
        want = log_mu[:, None] + log_nu[None, :] - norm
        assert np.abs(_reference(c, iters)[1] - want).max() < 1e-12
        assert np.abs(z - want).max() <= _reference(c, iters)[3]


@pytest.mark.parametrize("iters", [0, 1, 2, 5, 20, 100])
@pytest.mark.parametrize("k,form", FORMS)
def test_iteration_counts_vs_float64(k, form, iters):
    """0: Z = C - norm, no exchange at all; 1 and 2: the first use of either half of the (max, sum) exchange's double buffer; 5: an odd count"""
    n0, n1 = {400: (317, 400), 1024: (1000, 777), 256: (200, 131)}[k]
    z = _run(k, form, [_case(n0, n1)], iters, "iters")[0]
    if iters == 0:
        s = _reference(_case(n0, n1), 0)[0]
        np.testing.assert_allclose(z[:n0, :n1], s.astype(np.float64) + np.log(n0 + n1), atol=_reference(_case(n0, n1), 0)[3], rtol=0)


BATCH = {400: [(400, 400), (400, 317), (33, 400), (1, 1), (2, 3), (65, 97), (104, 105), (400, 1)],
         1024: [(1024, 1000), (1, 1024), (1000, 63), (72, 73), (1024, 1024), (513, 700), (3, 2), (900, 1)],
         256: [(256, 200), (65, 97)]}


@pytest.mark.parametrize("k,form", FORMS)
def test_pairs_of_a_batch_are_independent_bit_for_bit(k, form):
    """Eight different ragged pairs in one call (B = 8 makes the register kernel's grid a multiple of 8 with whole pairs per XCD: its placement permutation is ON —
    grid 32, G = 4 at 400; grid 120, G = 15 at 1024), three (permutation off, more than one pair), and each pair alone: a pair's summation order depends neither on B nor
    on where its workgroups run, so its Z is the same bits every time — and within the gate of float64 every time."""
    cases = [_case(n0, n1) for n0, n1 in BATCH[k]]
    alone = [_run(k, form, [c], 20, "alone")[0] for c in cases]
    full = _run(k, form, cases, 20, f"B{len(cases)}")
    for b, (a, z) in enumerate(zip(alone, full)):
        assert np.array_equal(a, z), (k, form, "B", len(cases), "pair", b, BATCH[k][b], float(np.abs(a - z).max()))
    if len(cases) > 3:
        three = _run(k, form, cases[:3], 20, "B3")
        for b, (a, z) in enumerate(zip(alone, three)):
            assert np.array_equal(a, z), (k, form, "B 3, pair", b, BATCH[k][b], float(np.abs(a - z).max()))
    # ... and a pair's place in the batch does not matter either
    back = _run(k, form, cases[::-1], 20, f"B{len(cases)}rev")[::-1]
    for b, (a, z) in enumerate(zip(alone, back)):
        assert np.array_equal(a, z), (k, form, "reversed batch, pair", b, BATCH[k][b])


@pytest.mark.parametrize("k", [400, 1024])
@pytest.mark.parametrize("B", [1, 3, 8])
def test_dispatch_takes_the_register_form_where_it_applies(k, B):
    """form 0 is production's dispatch: at max_keypoints 400 / 1024 and B <= 8 it is the register-resident instantiation, and gives the bits of form 2"""
    cases = [_case(n0, n1) for n0, n1 in BATCH[k][:B]]
    auto = _run(k, 0, cases, 20, f"auto{B}", expect_ran=REG_FORM[k])
    forced = _run(k, 2, cases, 20, f"B{B}")
    for a, z in zip(auto, forced):
        assert np.array_equal(a, z)


def test_dispatch_at_256_is_per_half_iteration_and_form_2_is_an_error():
    """max_keypoints 256: Lz = 320 holds no instantiation's column blocks.  form 0 reports 1; form 2 is an error with a message, never a silent fall-back — and
    the context goes on working"""
    cases = [_case(200, 131)]
    auto = _run(256, 0, cases, 20, "auto1", expect_ran=1)
    with pytest.raises(api.AirfeError) as e:
        _ctx(256).debug_sg_sinkhorn([_reference(cases[0], 20)[0]], ALPHA, 20, 2)
    assert "form 2" in str(e.value) and "register-resident" in str(e.value)
    assert np.array_equal(auto[0], _run(256, 1, cases, 20, "after_error")[0])


def test_hook_rejects_what_the_host_entry_rejects():
    ctx = _ctx(256)
    ok = sinkhorn_ref.couplings(5, 6, 1)
    for sims in ([np.zeros((0, 6), np.float32)], [np.zeros((6, 0), np.float32), ok], [ok, ok, ok],                # empty sides (as sg_host), B > max_batch = 2
                 [sinkhorn_ref.couplings(257, 6, 1)], [sinkhorn_ref.couplings(6, 257, 1)]):                       # beyond max_keypoints
        with pytest.raises(api.AirfeError):
            ctx.debug_sg_sinkhorn(sims, ALPHA, 5, 0)
    with pytest.raises(api.AirfeError):
        ctx.debug_sg_sinkhorn([ok], ALPHA, 5, 3)
    with pytest.raises(api.AirfeError):
        ctx.debug_sg_sinkhorn([ok], ALPHA, -1, 0)
    zs, ran = ctx.debug_sg_sinkhorn([ok], ALPHA, 5, 0)
    assert ran == 1 and np.isfinite(zs[0]).all()
