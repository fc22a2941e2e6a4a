"""The yardstick of tests/test_gpu_attention.py: a float64 soft-max attention on the kernel's own 2-byte inputs, the per-element error a CORRECT attention32_kernel
(airslam_amd/csrc/kernels_attn.hip) may show against it, and inputs whose answer is exact.  numpy only (no torch, no GPU); tests/test_attn_ref_cpu.py holds it to torch
and to an emulation of the kernel's rounding.

The bound is derived from the reference alone — nothing in it was measured on a device.  With u the unit round-off of the 2-byte type (2^-11 fp16, 2^-8 bf16; both pack
instructions round to nearest even), p = 2^(s - rowmax) and A = sum p |v| / sum p:
  u A                 P is packed to 2 bytes for the P V product while the row sum l adds the unrounded p
  u |ref|             the 2-byte store of the output
  2 gamma A           fp32 accumulation of the score chain (64 products + the shift that rides in as the C operand: 65 terms, |shift| <= max_j sum_d |q_d k_jd|, hence the
                      factor 2), gamma = 2 * 65 * 2^-24 * ln 2 * max_j sum_d |q_d k_jd|: a score error e changes p by the factor 2^e, numerator and denominator each
  F        (fp16)     sum over the keys with s - rowmax < -14 of p |v| / sum p: the MFMA may flush a subnormal P (the kernel's shift is never above the true row maximum,
                      so a P below fp16's normal range is at most what it is under the exact maximum)
  len_kv 2^-25 max|v|  (fp16) the spacing of the subnormal P that are kept
  1e-6                slack
"""
import numpy as np

U = {0: 2.0 ** -8, 1: 2.0 ** -11}                 # unit round-off of prec 0 = bf16, 1 = fp16
MAXV = {0: float(np.float32(3.3895313892515355e38)), 1: 65504.0}     # the types' largest finite values


def to_2byte(x, prec):
    """fp32 -> the 2-byte type (round to nearest even, as the hook's cvt2 and gpu_common.to_2byte) -> float64"""
    x = np.ascontiguousarray(x, np.float32)
    if prec == 1:
        with np.errstate(over="ignore"):
            return x.astype(np.float16).astype(np.float64)
    b = x.view(np.uint32).astype(np.uint64)
    r = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    r = np.where((b & 0x7F800000) == 0x7F800000, b & 0xFFFF0000, r)          # inf / NaN keep their upper half
    return r.astype(np.uint32).view(np.float32).reshape(x.shape).astype(np.float64)


def _heads(q, k, v, lens, cross, prec):
    """(s, h, lq, q [lq, 64], k [lk, 64], v [lk, 64]) over every (sequence, head), valid rows only, rounded to prec"""
    S, H = q.shape[:2]
    q, k, v = to_2byte(q, prec), to_2byte(k, prec), to_2byte(v, prec)
    for s in range(S):
        skv = s ^ 1 if cross else s
        lq, lk = int(lens[s]), int(lens[skv])
        for h in range(H):
            yield s, h, lq, q[s, h, :lq], k[skv, h, :lk], v[skv, h, :lk]


def reference(q, k, v, lens, cross, prec):
    """q, k, v [S, H, n, 64], lens [S] -> out [S, n, H * 64] float64: p = 2^(q.k - rowmax) over the valid keys, out = p v / sum p; P is NOT rounded (bound() covers it);
    a query with no valid keys gives a zero row, and so do the rows at or beyond lens[s]"""
    S, H, n, _ = q.shape
    out = np.zeros((S, n, H * 64))
    for s, h, lq, qq, kk, vv in _heads(q, k, v, lens, cross, prec):
        if lq == 0 or len(kk) == 0:
            continue
        sc = qq @ kk.T
        p = np.exp2(sc - sc.max(1, keepdims=True))
        out[s, :lq, h * 64:(h + 1) * 64] = (p @ vv) / p.sum(1, keepdims=True)
    return out


def bound(q, k, v, lens, cross, prec):
    """the per-element error a correct kernel may show against reference(): [S, n, H * 64] (module docstring); rows at or beyond lens[s] get the slack alone"""
    S, H, n, _ = q.shape
    u = U[prec]
    out = np.full((S, n, H * 64), 1e-6)
    for s, h, lq, qq, kk, vv in _heads(q, k, v, lens, cross, prec):
        if lq == 0 or len(kk) == 0:
            continue
        sc = qq @ kk.T
        d = sc - sc.max(1, keepdims=True)
        p = np.exp2(d)
        l = p.sum(1, keepdims=True)
        av = np.abs(vv)
        A = (p @ av) / l
        ref = (p @ vv) / l
        gamma = 2 * 65 * 2.0 ** -24 * np.log(2.0) * (np.abs(qq) @ np.abs(kk).T).max(1, keepdims=True)
        b = u * A + u * np.abs(ref) + 2 * gamma * A
        if prec == 1:
            b += (np.where(d < -14, p, 0.0) @ av) / l + len(kk) * 2.0 ** -25 * av.max()
        out[s, :lq, h * 64:(h + 1) * 64] += b
    return out


def probe(n, lens, seed, H=4):
    """Inputs whose answer is exact in both types: q[..., 0] = 1, k[j, 0] = c_j (an integer 0..3), every other q / k feature 0, v[j, d] = 1 where d == j % 64 (padding
    rows included).  Every p is a power of two and every fp32 sum exact.  -> q, k, v [S, H, n, 64] fp32"""
    rng = np.random.default_rng(seed)
    S = len(lens)
    q = np.zeros((S, H, n, 64), np.float32)
    k = np.zeros((S, H, n, 64), np.float32)
    v = np.zeros((S, H, n, 64), np.float32)
    q[..., 0] = 1.0
    k[..., 0] = rng.integers(0, 4, (S, H, n))
    j = np.arange(n)
    v[:, :, j, j % 64] = 1.0
    return q, k, v


def probe_expected(k, lens, cross):
    """the probe's answer from exact integer sums: out[s, i, 64 h + d] = sum over valid j = d (mod 64) of 2^c_j / sum over valid j of 2^c_j for i < lens[s], else 0"""
    S, H, n, _ = k.shape
    out = np.zeros((S, n, H * 64))
    for s in range(S):
        skv = s ^ 1 if cross else s
        lq, lk = int(lens[s]), int(lens[skv])
        if lq == 0 or lk == 0:
            continue
        for h in range(H):
            w = 2 ** k[skv, h, :lk, 0].astype(np.int64)
            num = np.bincount(np.arange(lk) % 64, weights=w, minlength=64)       # exact: integers far below 2^53
            out[s, :lq, h * 64:(h + 1) * 64] = (num / float(w.sum()))[None, :]
    return out


def probe_check(got, k, lens, cross, prec):
    """None, or what is wrong: where the expected value is 0 the result must be exactly 0 (a masked key that leaks shows there), elsewhere within 2 u |ref| — one unit
    in the last place of the output type (v_exp_f32 and the reciprocal of the row sum err by 2^-23, far below)"""
    ref = probe_expected(k, lens, cross)
    for s in range(len(lens)):
        g, r = np.asarray(got[s, :lens[s]], np.float64), ref[s, :lens[s]]
        if not np.isfinite(g).all():
            return f"sequence {s}: not finite"
        if (g[r == 0] != 0).any():
            return f"sequence {s}: {int((g[r == 0] != 0).sum())} non-zero where the answer is exactly 0 (max {np.abs(g[r == 0]).max():.3g})"
        bad = np.abs(g - r) > 2 * U[prec] * np.abs(r)
        if bad.any():
            return f"sequence {s}: {int(bad.sum())} elements beyond 2 u |ref| (worst {np.max(np.abs(g - r) / np.maximum(np.abs(r), 1e-300)) / U[prec]:.1f} u)"
    return None


def worst_ratio(got, ref, bnd, lens):
    """max over the valid rows of every sequence of |got - ref| / bound (inf where a valid row is not finite)"""
    w = 0.0
    for s in range(len(lens)):
        if lens[s]:
            e = np.abs(np.asarray(got[s, :lens[s]], np.float64) - ref[s, :lens[s]]) / bnd[s, :lens[s]]
            w = max(w, float(np.where(np.isfinite(e), e, np.inf).max()))
    return w
