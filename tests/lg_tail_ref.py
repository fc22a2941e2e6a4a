"""float64 references for LightGlue's head (lg_prepare_kernel) and tail (rowdot256_kernel, sim_kernel, the matrix-form and the fused assignment, the filter), each
with a DERIVED bound, and the input families the tail is driven with (tests/test_gpu_lg_tail.py on the device, tests/test_lg_tail_cpu.py keeps this file honest).
numpy only.

Bounds (none fitted to a measurement):
  prepare  x32, lens and xb = r2(x32) are exact.  cos / sin: the argument w0 kx + w1 ky is taken in float64 of the float32 kx, ky (after the reference's float32
           (k - c) * linv); the device's float32 argument is within 2 ulp32(|w0 kx| + |w1 ky|) whether or not the compiler contracts a product into the sum (two
           product roundings and one of the sum, or one and one), cos and sin are 1-Lipschitz, and cosf / sinf return within 2 ulp32 of the result.
  z        logsigmoid(w . x + b): acc_bound of the 256-term dot product and the bias add (logsigmoid is 1-Lipschitz), 4 ulp32(|z|) for expf, log1pf and the final
           subtraction, FLT_MIN for results the device flushes.
  sim      products of 2-byte operands are exact in float32: acc_bound of the 256-term sum.
  lse      over the valid entries v of a row / column of the DEVICE's float32 sim, m = max v, p = softmax(v):
             sum_j p_j |v_j - m| 2^-23      __expf(x) = exp2(x log2 e): the product's rounding moves exp(x) by |x| 2^-24 relatively, weighted by what the term
                                            contributes to the sum; a chain of re-scalings m_tile -> m (ms_merge) telescopes to the same |v_j - m|
             (3 + log2 n) 2^-23             the exponentials themselves (1 ulp), any order of the n-term sum, logf
             2 ulp32(|lse|)                 m + log(sum) and its storage
  scores   ((s - rl) + (s - cl)) + (z0 + z1) on the device's s, z0, z1 and the reference's lse: d_rl + d_cl + 4 ulp32 of the largest intermediate.
  decisions  none: the scan (strict '>' from -FLT_MAX, lowest index on ties, mutual check, glibc expf > thr, ascending rows, at most cap) is taken on the
           device's own float32 scores and must be reproduced exactly; against the float64 scores only where `safe_rows` / `safe_cols` say that no other entry
           can overtake the best one within the two entries' bounds.

The mutations of kernels_lg.hip that tests/test_gpu_lg_tail.py is built to catch are listed in that file's docstring."""
from __future__ import annotations

import numpy as np

from kernel_ref import acc_bound, r2, ulp32
from oracle import ref_post

FLT_MIN = 2.0 ** -126
FLT_MAX = float(np.finfo(np.float32).max)
F = np.float32


# ------------------------------------------------------------------ prepare
def prepare(f0, f1, n0, n1, wr, prec, Np, kp_off=1, normalize=None, second=None, slack_rows=0):
    """-> dict: x32, xb [rows, 256] (exact), cos, sin, dcos, dsin [rows, 32] (NaN in the slack rows: the kernel leaves their tables alone), lens [2 Bt],
    valid [rows] (1 token, 0 padding, -1 slack)"""
    f0, f1 = np.asarray(f0, F), np.asarray(f1, F)
    wr = np.asarray(wr, F).astype(np.float64)
    seqs = []
    for b in range(f0.shape[0]):
        seqs += [f0[b, :n0[b]], f1[b, :n1[b]]]
    if second is not None:
        ld = f0.shape[2]
        seqs += [np.asarray(second[0], F).reshape(-1, ld), np.asarray(second[1], F).reshape(-1, ld)]
    S = len(seqs)
    rows = S * Np + slack_rows
    x32 = np.zeros((rows, 256))
    cos, sin = np.ones((rows, 32)), np.zeros((rows, 32))
    dcos, dsin = np.zeros((rows, 32)), np.zeros((rows, 32))
    valid = np.zeros(rows, np.int32)
    for s, f in enumerate(seqs):
        n = f.shape[0]
        if n == 0:
            continue
        r = slice(s * Np, s * Np + n)
        valid[r] = 1
        x32[r] = f[:, kp_off + 2:kp_off + 258]
        kx, ky = f[:, kp_off], f[:, kp_off + 1]
        if normalize is not None:
            cx, cy, linv = (F(v) for v in normalize)
            kx, ky = ((kx - cx).astype(F) * linv).astype(F), ((ky - cy).astype(F) * linv).astype(F)
        px, py = kx.astype(np.float64)[:, None] * wr[None, :, 0], ky.astype(np.float64)[:, None] * wr[None, :, 1]
        arg = px + py
        darg = 2 * ulp32(np.abs(px) + np.abs(py))
        cos[r], sin[r] = np.cos(arg), np.sin(arg)
        dcos[r], dsin[r] = darg + 2 * ulp32(cos[r]), darg + 2 * ulp32(sin[r])
    valid[S * Np:] = -1
    for t in (cos, sin, dcos, dsin):
        t[S * Np:] = np.nan
    return {"x32": x32, "xb": r2(x32, prec), "cos": cos, "sin": sin, "dcos": dcos, "dsin": dsin, "lens": np.array([len(f) for f in seqs], np.int32), "valid": valid}


# ------------------------------------------------------------------ the tail, value by value
def logsigmoid(d):
    d = np.asarray(d, np.float64)
    return np.minimum(d, 0.0) - np.log1p(np.exp(-np.abs(d)))


def z_ref(x32, w, b):
    """x32 [n, 256] float32 values -> (z [n], bound [n])"""
    x, w = np.asarray(x32, np.float64), np.asarray(w, np.float64)
    z = logsigmoid(x @ w + float(b))
    return z, acc_bound(x, w[None, :], float(b))[:, 0] + 4 * ulp32(z) + FLT_MIN


def sim_ref(md0, md1, prec):
    a, b = r2(md0, prec), r2(md1, prec)
    return a @ b.T, acc_bound(a, b)


def lse_ref(v, axis):
    """log-sum-exp of v (the valid block only) along `axis` -> (lse, bound); an empty axis gives -inf with bound 0"""
    v = np.asarray(v, np.float64)
    n = v.shape[axis]
    if n == 0:
        shape = tuple(d for k, d in enumerate(v.shape) if k != axis)
        return np.full(shape, -np.inf), np.zeros(shape)
    m = v.max(axis=axis, keepdims=True)
    e = np.exp(v - m)
    s = e.sum(axis=axis, keepdims=True)
    lse = (m + np.log(s)).squeeze(axis)
    p = e / s
    bound = (p * np.abs(v - m)).sum(axis=axis) * 2.0 ** -23 + (3 + np.log2(n)) * 2.0 ** -23 + 2 * ulp32(lse)
    return lse, bound


def scores_ref(sim, z0, z1):
    """the log-assignment on float32 sim [n0, n1], z0 [n0], z1 [n1] -> dict rowlse, collse, scores with their bounds d_*"""
    s = np.asarray(sim, np.float64)
    z0, z1 = np.asarray(z0, np.float64), np.asarray(z1, np.float64)
    rl, drl = lse_ref(s, 1)
    cl, dcl = lse_ref(s, 0)
    a, b, c = s - rl[:, None], s - cl[None, :], z0[:, None] + z1[None, :]
    sc = (a + b) + c
    big = np.zeros_like(s)
    for t in (s, a, b, a + b, c, sc, rl[:, None], cl[None, :]):
        big = np.maximum(big, np.abs(np.broadcast_to(t, s.shape)))
    return {"rowlse": rl, "d_rowlse": drl, "collse": cl, "d_collse": dcl, "scores": sc, "d_scores": drl[:, None] + dcl[None, :] + 4 * ulp32(big)}


def scan(scores, thr=0.1, cap=None):
    """oracle/ref_post.filter_matches (src/light_glue.cpp:214-266) on float32 scores [n0, n1], extended to return what the kernels store on the way:
    -> dict rowarg, rowval [n0], colarg [n1], idx [k, 2], score [k], nmatch (k = min(matches, cap), the first in row order).  A row without anything above
    -FLT_MAX (an empty second image too) keeps (0, 0.0f); an empty side has no matches (point_matcher.cc:53-55)."""
    s = np.asarray(scores, F)
    n0, n1 = s.shape
    out = {"rowarg": np.zeros(n0, np.int32), "rowval": np.zeros(n0, F), "colarg": np.zeros(n1, np.int32), "idx": np.zeros((0, 2), np.int32),
           "score": np.zeros((0,), F), "nmatch": 0}
    if n0 == 0 or n1 == 0:
        return out
    rcol, rval, rfound = ref_post._first_max_above_floor(s, 1)
    rval = np.where(rfound, rval, F(0)).astype(F)
    crow, _, _ = ref_post._first_max_above_floor(s, 0)
    rows = np.arange(n0)
    e = ref_post._expf(rval)
    ok = (crow[rcol] == rows) & (e > F(thr))
    idx, sc = np.stack([rows[ok], rcol[ok]], 1).astype(np.int32), e[ok].astype(F)
    if cap is not None:
        idx, sc = idx[:cap], sc[:cap]
    out.update(rowarg=rcol.astype(np.int32), rowval=rval, colarg=crow.astype(np.int32), idx=idx, score=sc, nmatch=len(idx))
    return out


def safe(scores, bound, axis):
    """per row (axis 1) / column (axis 0): True where no other entry can overtake the float64 best within the two entries' bounds — min over the others of
    (best - other) - (bound_best + bound_other) > 0.  A row that is not safe is "fragile": its float64 margin is at most the sum of two score bounds."""
    s, d = np.asarray(scores, np.float64), np.asarray(bound, np.float64)
    if axis == 0:
        s, d = s.T, d.T
    n, k = s.shape
    if k == 0:
        return np.zeros(n, bool)
    if k == 1:
        return np.ones(n, bool)
    best = np.argmax(s, 1)
    r = np.arange(n)
    gap = (s[r, best][:, None] - s) - (d[r, best][:, None] + d)
    gap[r, best] = np.inf
    return gap.min(1) > 0


def tail(md0, md1, x0, x1, w, b, prec, thr=0.1):
    """the whole tail in float64 from the host inputs (what the CPU test compares with oracle/ref_nets.lightglue_forward's tail)"""
    sim, _ = sim_ref(md0, md1, prec)
    z0, _ = z_ref(x0, w, b)
    z1, _ = z_ref(x1, w, b)
    return scores_ref(sim, z0, z1)["scores"]


# ------------------------------------------------------------------ float32 runs of the same formulas (the CPU test holds them to the bounds above)
def lse32(v, axis):
    v = np.asarray(v, F)
    m = v.max(axis=axis, keepdims=True)
    return (m + np.log(np.exp(v - m, dtype=F).sum(axis=axis, keepdims=True, dtype=F), dtype=F)).squeeze(axis).astype(F)


def scores32(sim, rl, cl, z0, z1):
    s, rl, cl, z0, z1 = (np.asarray(t, F) for t in (sim, rl, cl, z0, z1))
    return ((s - rl[:, None]) + (s - cl[None, :])) + (z0[:, None] + z1[None, :])


def z32(x32, w, b):
    x, w = np.asarray(x32, F), np.asarray(w, F)
    d = (x * w[None, :]).sum(1, dtype=F) + F(b)
    return (np.minimum(d, F(0)) - np.log1p(np.exp(-np.abs(d), dtype=F), dtype=F)).astype(F)


def prepare_arg32(kx, ky, wr):
    wr = np.asarray(wr, F)
    return (wr[None, :, 0] * np.asarray(kx, F)[:, None]).astype(F) + (wr[None, :, 1] * np.asarray(ky, F)[:, None]).astype(F)


# ------------------------------------------------------------------ input families
FAMILIES = ("planted", "wide", "constant", "ramp", "ramp_down", "dup")


def _unit(rng, n):
    u = rng.normal(size=(n, 256))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def dup_indices(n):
    """duplicate rows in different 64-row tiles where the length allows it"""
    return [i for i in (5, 70, n - 1) if i < n and (i == 5 or n > 70)]


def family(kind, n0, n1, seed, scale=8.0):
    """-> (md0 [n0, 256], md1 [n1, 256], x0 [n0, 256], x1 [n1, 256]) float32.
    planted   unit directions x sqrt(scale), side 1 a permutation of side 0's: the matched similarity is `scale`, the others ~ N(0, scale / 16)
    wide      planted with scale 200 and a random sign per row of side 0: similarities out to about +-200
    constant  every descriptor and every token row equal: all scores of a pair tie
    ramp      sim[i][j] = 45 (tile(i) + tile(j)) + N(0, 1): each row's (column's) maximum rises by 45 from one 64-column (-row) tile to the next, so every
              ms_merge re-scales the older side; ramp_down: it falls, and the newer side is re-scaled
    dup       planted, with a few descriptor AND token rows repeated in different tiles on either side: exact ties across tile boundaries"""
    rng = np.random.default_rng(seed)
    n = max(n0, n1)
    x0, x1 = rng.normal(size=(n0, 256)), rng.normal(size=(n1, 256))
    if kind == "constant":
        md0, md1 = np.full((n0, 256), 0.125), np.full((n1, 256), 0.125)
        x0, x1 = np.repeat(x0[:1], n0, 0), np.repeat(x1[:1], n1, 0)
    elif kind in ("ramp", "ramp_down"):
        t0, t1 = np.arange(n0) // 64, np.arange(n1) // 64
        if kind == "ramp_down":
            t0, t1 = t0.max() - t0, t1.max() - t1
        md0, md1 = rng.normal(size=(n0, 256)) / 4, rng.normal(size=(n1, 256)) / 4          # 254 terms of variance 1 / 256
        md0[:, 0], md0[:, 1] = 1.0, 45.0 * t0
        md1[:, 0], md1[:, 1] = 45.0 * t1, 1.0
    else:
        a = np.sqrt(200.0 if kind == "wide" else scale)
        u = _unit(rng, n)
        perm = rng.permutation(n)
        md0, md1 = a * u[:n0], a * u[perm][:n1]
        if kind == "wide":
            md0 = md0 * rng.choice([-1.0, 1.0], size=(n0, 1))
        if kind == "dup":
            for md, x, m in ((md0, x0, n0), (md1, x1, n1)):
                ii = dup_indices(m)
                md[ii], x[ii] = md[ii[0]], x[ii[0]]
    return tuple(np.ascontiguousarray(t, F) for t in (md0, md1, x0, x1))


def matchability(seed=77):
    """(w [256], b): w . x ~ N(0, 1) on the families' token rows"""
    return (np.random.default_rng(seed).normal(size=256) / 16).astype(F), F(0.1)


# ------------------------------------------------------------------ the cases of tests/test_gpu_lg_tail.py (tests/test_lg_tail_cpu.py walks the same list)
LENGTHS = {400: [(400, 400), (400, 317), (33, 400), (1, 1), (1, 400), (400, 1), (2, 3), (63, 65), (64, 64), (65, 97), (129, 63)],
           1024: [(1024, 1000), (1, 1024), (1000, 63)]}
BATCH = [(400, 400), (1, 400), (400, 1), (63, 65), (64, 64), (129, 200), (399, 17), (5, 5), (33, 400)]      # the first 8: merged launches; all 9: four kernels
FAMILY_SHAPES = [(400, 400), (129, 200)]


def case_seed(kind, n0, n1):
    return 7919 * n0 + 31 * n1 + FAMILIES.index(kind)


def gpu_cases():
    """every (kind, n0, n1) the GPU file runs"""
    out = [("planted", n0, n1) for k in LENGTHS for n0, n1 in LENGTHS[k]] + [("planted", n0, n1) for n0, n1 in BATCH]
    out += [(kind, n0, n1) for kind in FAMILIES if kind != "planted" for n0, n1 in FAMILY_SHAPES]
    return sorted(set(out))
