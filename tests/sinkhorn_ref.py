"""SuperGlue's log_optimal_transport in plain numpy: the float64 reference of tests/test_gpu_sinkhorn.py, and (dtype=np.float32) the SAME code as the float32
error floor its tolerances are multiples of.  Public SuperGlue's formulation: couplings C = [[scores, alpha], [alpha, alpha]], log_mu / log_nu with the
dustbins carrying n / m of the mass, `iters` times (u step, then v step) with logsumexp shifted by the row / column maximum, Z = C + u + v - norm.
tests/test_sinkhorn_cpu.py holds it to oracle/ref_post.log_optimal_transport and oracle/ref_nets.sinkhorn_log."""
import numpy as np


def _lse(x, axis, dtype):
    mx = x.max(axis=axis, keepdims=True)
    return (mx + np.log(np.exp(x - mx).sum(axis=axis, keepdims=True, dtype=dtype))).squeeze(axis).astype(dtype)


def log_optimal_transport(scores, alpha, iters, dtype=np.float64):
    """scores [m, n] (float32 values are exact in either dtype), alpha the dustbin score -> Z [m + 1, n + 1] in `dtype`"""
    s = np.asarray(scores).astype(dtype)
    m, n = s.shape
    c = np.full((m + 1, n + 1), dtype(np.float32(alpha)), dtype=dtype)        # the device takes alpha as a float
    c[:m, :n] = s
    norm = dtype(-np.log(dtype(m + n)))
    log_mu = np.full(m + 1, norm, dtype=dtype); log_mu[m] = np.log(dtype(n)) + norm
    log_nu = np.full(n + 1, norm, dtype=dtype); log_nu[n] = np.log(dtype(m)) + norm
    u = np.zeros(m + 1, dtype=dtype); v = np.zeros(n + 1, dtype=dtype)
    for _ in range(iters):
        u = (log_mu - _lse(c + v[None, :], 1, dtype)).astype(dtype)
        v = (log_nu - _lse(c + u[:, None], 0, dtype)).astype(dtype)
    z = (c + u[:, None] + v[None, :] - norm).astype(dtype)
    assert z.dtype == dtype
    return z


def column_mass(m, n):
    """what the columns of exp(Z) sum to once a v step has run (iters >= 1): exp(log_nu - norm) = 1 for a keypoint column, m for the dustbin column"""
    out = np.ones(n + 1)
    out[n] = m
    return out


def couplings(n0, n1, seed, scale=8.0, planted=True):
    """float32 test couplings: normal x `scale`, and (planted) a strong permuted diagonal on about two thirds of the rows, so that exp(Z) holds real matches
    next to rows and columns that go to the dustbins"""
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((n0, n1)) * scale
    if planted:
        k = min(n0, n1)
        rows = rng.permutation(n0)[:k]
        cols = rng.permutation(n1)[:k]
        keep = rng.random(k) < 0.67
        s[rows[keep], cols[keep]] += scale * (2.5 + np.abs(rng.standard_normal(int(keep.sum()))))
    return s.astype(np.float32)
