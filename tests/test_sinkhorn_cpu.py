"""tests/sinkhorn_ref.py (the float64 reference of tests/test_gpu_sinkhorn.py) held to what the project already trusts: oracle/ref_post.log_optimal_transport (the
float32 restatement of the reference's CPU copy, src/super_glue.cpp:369-435, exp sums WITHOUT a shift) and oracle/ref_nets.sinkhorn_log (torch, float32 logsumexp),
at coupling ranges where the unshifted form stays finite.  Both are float32 computations of the same iteration in another summation order, so the bound is the one
the GPU test uses: 8 x the float32 floor of the case, floor = max|Z32 - Z64| of sinkhorn_ref's own float32 run (not below one float32 ulp of max|Z64|)."""
import numpy as np
import pytest

import sinkhorn_ref
from oracle import ref_nets, ref_post

CASES = [(40, 40, 2.0, 2.3457, 100), (64, 37, 3.0, 2.3457, 100), (1, 3, 2.0, 1.0, 5), (1, 1, 2.0, 0.5, 20), (7, 1, 2.0, -1.5, 20), (150, 170, 2.5, 2.3457, 50),
         (33, 64, 3.0, 4.0, 1), (33, 64, 3.0, 4.0, 0)]


def _gate(z64, z32):
    e32 = float(np.abs(z32.astype(np.float64) - z64).max())
    return 8.0 * max(e32, 2.0 ** -23 * float(np.abs(z64).max())), e32


@pytest.mark.parametrize("n0,n1,scale,alpha,iters", CASES)
def test_float64_reference_agrees_with_the_oracles(n0, n1, scale, alpha, iters):
    s = sinkhorn_ref.couplings(n0, n1, 1000 + n0 * 7 + n1, scale)
    z64 = sinkhorn_ref.log_optimal_transport(s, alpha, iters)
    z32 = sinkhorn_ref.log_optimal_transport(s, alpha, iters, dtype=np.float32)
    assert z64.dtype == np.float64 and z32.dtype == np.float32 and z64.shape == (n0 + 1, n1 + 1)
    gate, e32 = _gate(z64, z32)
    post = ref_post.log_optimal_transport(s, alpha, iters)
    import torch
    nets = ref_nets.sinkhorn_log(torch.from_numpy(s), torch.tensor(np.float32(alpha)).reshape(1, 1), iters).numpy()
    e_post, e_nets = float(np.abs(post - z64).max()), float(np.abs(nets - z64).max())
    print(f"sinkhorn_cpu {n0}x{n1} x{scale} iters {iters}: e32 {e32:.3g} max|Z64| {np.abs(z64).max():.3g} gate {gate:.3g} ref_post {e_post:.3g} ref_nets {e_nets:.3g}")
    assert np.isfinite(post).all() and np.isfinite(nets).all()
    assert e_post <= gate and e_nets <= gate


@pytest.mark.parametrize("n0,n1", [(5, 9), (1, 1), (30, 2)])
def test_constant_couplings_have_the_closed_form(n0, n1):
    """every coupling (dustbins included) equal: one iteration lands on the product coupling Z[i][j] = log_mu[i] + log_nu[j] - norm and stays there"""
    s = np.full((n0, n1), 3.0, np.float32)
    norm = -np.log(n0 + n1)
    log_mu = np.full(n0 + 1, norm); log_mu[n0] = np.log(n1) + norm
    log_nu = np.full(n1 + 1, norm); log_nu[n1] = np.log(n0) + norm
    want = log_mu[:, None] + log_nu[None, :] - norm
    for iters in (1, 2, 7):
        np.testing.assert_allclose(sinkhorn_ref.log_optimal_transport(s, 3.0, iters), want, atol=1e-13, rtol=0)


def test_zero_iterations_and_marginals():
    s = sinkhorn_ref.couplings(23, 31, 5, 8.0)
    z0 = sinkhorn_ref.log_optimal_transport(s, 2.0, 0)
    np.testing.assert_allclose(z0[:23, :31], s.astype(np.float64) + np.log(23 + 31), atol=1e-13, rtol=0)      # Z = C - norm
    for iters in (1, 2, 20):
        z = sinkhorn_ref.log_optimal_transport(s, 2.0, iters)
        np.testing.assert_allclose(np.exp(z).sum(0), sinkhorn_ref.column_mass(23, 31), rtol=1e-13)             # the column step is last
    z = sinkhorn_ref.log_optimal_transport(sinkhorn_ref.couplings(23, 31, 5, 1.0), 2.0, 400)      # (mild couplings: x 8 converges far more slowly)
    row_mass = np.ones(24); row_mass[23] = 31
    np.testing.assert_allclose(np.exp(z).sum(1), row_mass, rtol=1e-6)                                          # ... and the rows converge


def test_shifted_form_survives_a_range_the_unshifted_form_does_not():
    s = sinkhorn_ref.couplings(20, 20, 9, 25.0)
    assert np.isfinite(sinkhorn_ref.log_optimal_transport(s, 10.0, 20)).all()
    assert np.isfinite(sinkhorn_ref.log_optimal_transport(s, 10.0, 20, dtype=np.float32)).all()
