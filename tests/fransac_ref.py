"""The F-matrix RANSAC contract of include/airfe.h ("F-matrix RANSAC") restated in float64 numpy: same hash, same solver, same sequential rule.

Independent of airslam_amd/csrc/fransac_core.h (which the HIP kernels and the C++ stand-in of cv::findFundamentalMat share): every formula is written
again here, vectorised over the samples, in the same operation order (no fused multiply-adds on either side), so that the selected model and the kept
list agree; only acos / cos / cbrt / log may differ in the last ulp.  Also the planted two-view geometry the tests use."""
from __future__ import annotations

import numpy as np

SEED = np.uint64(0x2545F4914F6CDD1D)
MAX_ATTEMPTS = 64
RANSAC_ITERS = 1000
LMEDS_ITERS = 300
MIN_RANSAC = 15
THRESH2 = np.float32(400.0)
FLT_EPS = 1.1920928955078125e-07
DBL_EPS = 2.220446049250313e-16
DBL_MIN = 2.2250738585072014e-308
M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def oracle_has_stand_in() -> bool:
    """oracle/_ref/libairslam_ref.so exists AND carries this tree's stand-in of cv::findFundamentalMat (shim/stubs/mini_support.cpp): only then may the
    reference's MatchingPoints(..., true) be called in-process (an older library's stand-in aborts)"""
    from oracle import ref_lib
    if not ref_lib.available():
        return False
    try:
        ref_lib.lib().mini_cv_fundamental_ransac
    except AttributeError:
        return False
    return True


def lmeds_iters() -> int:
    return int(np.rint(np.log(0.01) / np.log(1 - 0.55 ** 7)))


def splitmix64(z):
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def draws(samples, n):
    """[S][MAX_ATTEMPTS][7] match indices of every attempt of the given samples"""
    s = np.asarray(samples, np.uint64)[:, None, None]
    a = np.arange(MAX_ATTEMPTS, dtype=np.uint64)[None, :, None]
    k = np.arange(7, dtype=np.uint64)[None, None, :]
    h = splitmix64(SEED ^ ((s << np.uint64(32)) | (a << np.uint64(8)) | k))
    return (((h >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def _collinear(P, i, j, k):
    dx1 = P[..., j, 0] - P[..., i, 0]; dy1 = P[..., j, 1] - P[..., i, 1]
    dx2 = P[..., k, 0] - P[..., i, 0]; dy2 = P[..., k, 1] - P[..., i, 1]
    return np.abs(dx2 * dy1 - dy2 * dx1) <= FLT_EPS * (np.abs(dx1) + np.abs(dy1) + np.abs(dx2) + np.abs(dy2))


def samples_xy(xy, samples):
    """-> (ok [S], X [S][7][4]): the first accepted attempt of each sample"""
    n = len(xy)
    ids = draws(samples, n)                                     # [S][A][7]
    ok = np.ones(ids.shape[:2], bool)
    for a in range(7):
        for b in range(a + 1, 7):
            ok &= ids[..., a] != ids[..., b]
    X = xy[ids]                                                 # [S][A][7][4]
    for i in range(7):
        for j in range(i + 1, 7):
            for k in range(j + 1, 7):
                ok &= ~_collinear(X[..., 0:2], i, j, k) & ~_collinear(X[..., 2:4], i, j, k)
    first = np.argmax(ok, axis=1)
    good = ok[np.arange(len(ok)), first]
    return good, X[np.arange(len(ok)), first]


def _det3(m):
    return m[..., 0] * (m[..., 4] * m[..., 8] - m[..., 5] * m[..., 7]) - m[..., 1] * (m[..., 3] * m[..., 8] - m[..., 5] * m[..., 6]) + \
        m[..., 2] * (m[..., 3] * m[..., 7] - m[..., 4] * m[..., 6])


def _det3_mix(X, Y, mask):
    cols = np.array([(mask >> (i % 3)) & 1 for i in range(9)], bool)
    return _det3(np.where(cols, Y, X))


def solve7(X):
    """X [S][7][4] -> (F [S][3][9], nmodels [S]) in model-slot order (non-finite models dropped, the rest moved up)"""
    S = len(X)
    x0, y0, x1, y1 = X[..., 0], X[..., 1], X[..., 2], X[..., 3]
    A = np.stack([x1 * x0, x1 * y0, x1, y1 * x0, y1 * y0, y1, x0, y0, np.ones_like(x0)], -1)      # [S][7][9]
    mx = np.abs(A).reshape(S, -1).max(1)
    tol = 1e-12 * mx
    ok = np.ones(S, bool)
    ar = np.arange(S)
    with np.errstate(all="ignore"):
        for k in range(7):
            p = np.full(S, k); best = np.abs(A[:, k, k])
            for r in range(k + 1, 7):
                bigger = np.abs(A[:, r, k]) > best
                best = np.where(bigger, np.abs(A[:, r, k]), best); p = np.where(bigger, r, p)
            rowk = A[ar, p].copy(); rowp = A[:, k].copy()
            A[:, k] = rowk; A[ar, p] = rowp
            ok &= best > tol
            for r in range(k + 1, 7):
                f = A[:, r, k] / A[:, k, k]
                A[:, r, k + 1:] = A[:, r, k + 1:] - f[:, None] * A[:, k, k + 1:]
        f1 = np.zeros((S, 9)); f2 = np.zeros((S, 9))
        f1[:, 7] = 1.0; f2[:, 8] = 1.0
        for k in range(6, -1, -1):
            s1 = A[:, k, 7] * f1[:, 7] + A[:, k, 8] * f1[:, 8]
            s2 = A[:, k, 7] * f2[:, 7] + A[:, k, 8] * f2[:, 8]
            for c in range(k + 1, 7):
                s1 = s1 + A[:, k, c] * f1[:, c]; s2 = s2 + A[:, k, c] * f2[:, c]
            f1[:, k] = -s1 / A[:, k, k]
            f2[:, k] = -s2 / A[:, k, k]
        D = f1 - f2
        c0 = _det3(f2); c3 = _det3(D)
        c1 = _det3_mix(f2, D, 1) + _det3_mix(f2, D, 2) + _det3_mix(f2, D, 4)
        c2 = _det3_mix(D, f2, 1) + _det3_mix(D, f2, 2) + _det3_mix(D, f2, 4)
        rt = np.zeros((S, 3)); nr = np.zeros(S, np.int64)
        # c3 == 0: quadratic / linear
        lin = (c3 == 0) & (c2 == 0) & (c1 != 0)
        rt[lin, 0] = -c0[lin] / c1[lin]; nr[lin] = 1
        quad = (c3 == 0) & (c2 != 0)
        disc = c1 * c1 - 4.0 * c2 * c0
        q1 = quad & (disc == 0)
        rt[q1, 0] = (-c1 / (2.0 * c2))[q1]; nr[q1] = 1
        q2 = quad & (disc > 0)
        sq = np.sqrt(np.where(q2, disc, 0.0))
        rt[q2, 0] = ((-c1 + sq) / (2.0 * c2))[q2]; rt[q2, 1] = ((-c1 - sq) / (2.0 * c2))[q2]; nr[q2] = 2
        cub = c3 != 0
        a2 = c2 / c3; a1 = c1 / c3; a0 = c0 / c3
        Q = (a2 * a2 - 3.0 * a1) / 9.0
        R = (2.0 * a2 * a2 * a2 - 9.0 * a2 * a1 + 27.0 * a0) / 54.0
        Q3 = Q * Q * Q; d = Q3 - R * R
        tri0 = cub & (d >= 0) & (Q3 == 0)
        rt[tri0, 0] = (-a2 / 3.0)[tri0]; nr[tri0] = 1
        tri = cub & (d >= 0) & (Q3 != 0)
        t = np.clip(R / np.sqrt(Q3), -1.0, 1.0)
        th = np.arccos(t); sqq = -2.0 * np.sqrt(Q)
        for i, add in enumerate((0.0, 6.283185307179586, 12.566370614359172)):
            v = sqq * np.cos((th + add) / 3.0) - a2 / 3.0 if add else sqq * np.cos(th / 3.0) - a2 / 3.0
            rt[tri, i] = v[tri]
        nr[tri] = 3
        car = cub & (d < 0)
        e = np.cbrt(np.sqrt(-d) + np.abs(R))
        e = np.where(R > 0.0, -e, e)
        rt[car, 0] = (e + Q / e - a2 / 3.0)[car]; nr[car] = 1
        nr[~ok] = 0
        F = np.zeros((S, 3, 9)); nm = np.zeros(S, np.int64)
        for r in range(3):
            a = rt[:, r]; b = 1.0 - a
            G = a[:, None] * f1 + b[:, None] * f2
            sc = np.abs(G[:, 8]) > DBL_EPS
            Gs = G.copy()
            Gs[:, :8] = G[:, :8] / G[:, 8:9]
            Gs[:, 8] = 1.0
            G = np.where(sc[:, None], Gs, G)
            use = (r < nr) & np.isfinite(G).all(1)
            F[ar[use], nm[use]] = G[use]
            nm += use
    return F, nm


def errors(F, xy):
    """F [..][9], xy [n][4] -> float32 errors [..][n]"""
    f = [F[..., i:i + 1] for i in range(9)]
    x0, y0, x1, y1 = xy[:, 0], xy[:, 1], xy[:, 2], xy[:, 3]
    with np.errstate(all="ignore"):
        a = f[0] * x0 + f[1] * y0 + f[2]; b = f[3] * x0 + f[4] * y0 + f[5]; c = f[6] * x0 + f[7] * y0 + f[8]
        d = x1 * a + y1 * b + c
        ap = f[0] * x1 + f[3] * y1 + f[6]; bp = f[1] * x1 + f[4] * y1 + f[7]
        e1 = d * d / (ap * ap + bp * bp); e2 = d * d / (a * a + b * b)
        e1 = np.where(e1 >= 0.0, e1, np.inf); e2 = np.where(e2 >= 0.0, e2, np.inf)
        return np.where(e1 > e2, e1, e2).astype(np.float32)


def update_niters(n, good) -> int:
    ep = float(n - good) / float(n)
    num = 1.0 - 0.99
    q = 1.0 - ep; q2 = q * q; q4 = q2 * q2
    den = 1.0 - q4 * q2 * q
    if den < DBL_MIN:
        return 0
    ln, ld = np.log(num), np.log(den)
    return RANSAC_ITERS if (ld >= 0.0 or -ln >= 1000.0 * (-ld)) else int(np.rint(ln / ld))


def lmeds_thresh(n, median) -> np.float32:
    sigma = 2.5 * 1.4826 * (1.0 + 5.0 / float(n - 7)) * np.sqrt(float(median))
    sigma = max(sigma, 0.001)
    return np.float32(sigma * sigma)


def points(f0, f1, idx):
    """truncated (cv::Point) coordinates [m][4] of the matches idx [m][2] between feature rows f0 / f1 [n][259]"""
    idx = np.asarray(idx).reshape(-1, 2)
    return np.stack([np.trunc(f0[idx[:, 0], 1]), np.trunc(f0[idx[:, 0], 2]), np.trunc(f1[idx[:, 1], 1]), np.trunc(f1[idx[:, 1], 2])], 1).astype(np.float64)


def fransac(xy):
    """xy [n][4] -> dict(mask [n] bool, F [9], sel = 3 sample + model slot (-1 none, -2 gate), kept, errors of the selected model)"""
    xy = np.asarray(xy, np.float64)
    n = len(xy)
    if n < 9:
        return dict(mask=np.ones(n, bool), F=np.zeros(9), sel=-2, kept=n, err=None)
    lmeds = n < MIN_RANSAC
    total = LMEDS_ITERS if lmeds else RANSAC_ITERS
    good, X = samples_xy(xy, np.arange(total))
    F, nm = solve7(X)
    nm[~good] = 0
    E = errors(F, xy)                                            # [S][3][n]
    best, niters = -1, total
    if not lmeds:
        cnt = (E <= THRESH2).sum(-1)
        bestc = 6
        for s in range(total):
            if s >= niters:
                break
            for r in range(nm[s]):
                if cnt[s, r] > bestc:
                    bestc = int(cnt[s, r]); best = 3 * s + r; niters = update_niters(n, bestc)
        thr = THRESH2
    else:
        med = np.sort(E, -1)[..., n // 2]
        bestmed = np.float32(np.inf)
        for s in range(total):
            for r in range(nm[s]):
                if med[s, r] < bestmed:
                    bestmed = med[s, r]; best = 3 * s + r
        thr = lmeds_thresh(n, bestmed) if best >= 0 else None
    if best < 0:
        return dict(mask=np.zeros(n, bool), F=np.zeros(9), sel=-1, kept=0, err=None)
    Fb = F[best // 3, best % 3]
    err = errors(Fb, xy)
    mask = err <= thr
    if lmeds and mask.sum() < 7:
        return dict(mask=np.zeros(n, bool), F=np.zeros(9), sel=-1, kept=0, err=None)
    return dict(mask=mask, F=Fb.copy(), sel=best, kept=int(mask.sum()), err=err)


# ------------------------------------------------------------------------------------------------ planted two-view geometry
def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]); Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]); Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def planted(m, inlier_ratio, seed, w=752, h=480):
    """m matches between two 752x480 views of random 3-D points (real baseline and rotation); a fraction inlier_ratio are true, the rest uniform.
    -> (xy [m][4] truncated coordinates, true inlier mask [m], true F [9] (row-major, x1^T F x0 = 0))"""
    rng = np.random.default_rng(seed)
    K = np.array([[420.0, 0, w / 2], [0, 420.0, h / 2], [0, 0, 1]])
    R = _rot(0.03, 0.12, 0.02)
    t = np.array([0.6, 0.1, 0.15])
    ni = int(round(m * inlier_ratio))
    pts = []
    while sum(len(p) for p in pts) < ni:
        P = np.stack([rng.uniform(-4, 4, 4 * m + 8), rng.uniform(-3, 3, 4 * m + 8), rng.uniform(4, 12, 4 * m + 8)], 1)
        p0 = (K @ P.T).T; p0 = p0[:, :2] / p0[:, 2:]
        P1 = (R @ P.T).T + t
        p1 = (K @ P1.T).T; p1 = p1[:, :2] / p1[:, 2:]
        ok = (P1[:, 2] > 0.5) & (p0[:, 0] >= 0) & (p0[:, 0] < w) & (p0[:, 1] >= 0) & (p0[:, 1] < h) & (p1[:, 0] >= 0) & (p1[:, 0] < w) & (p1[:, 1] >= 0) & (p1[:, 1] < h)
        pts.append(np.concatenate([p0[ok], p1[ok]], 1))
    inl = np.concatenate(pts)[:ni]
    out = np.stack([rng.uniform(0, w, m - ni), rng.uniform(0, h, m - ni), rng.uniform(0, w, m - ni), rng.uniform(0, h, m - ni)], 1)
    xy = np.concatenate([inl, out]).astype(np.float32)
    truth = np.concatenate([np.ones(ni, bool), np.zeros(m - ni, bool)])
    perm = rng.permutation(m)
    xy, truth = xy[perm], truth[perm]
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(K)
    Ft = Ki.T @ tx @ R @ Ki
    return np.trunc(xy).astype(np.float64), truth, (Ft / Ft[2, 2]).reshape(9), xy


def features_for(xy_float, seed=0):
    """feature rows f0, f1 [m][259] whose keypoint i carries the float coordinates of match i (descriptor columns random): idx = (i, i)"""
    rng = np.random.default_rng(seed)
    m = len(xy_float)
    f0 = np.zeros((m, 259), np.float32); f1 = np.zeros((m, 259), np.float32)
    f0[:, 0] = f1[:, 0] = rng.random(m, dtype=np.float32)
    f0[:, 1:3] = xy_float[:, 0:2]; f1[:, 1:3] = xy_float[:, 2:4]
    return f0, f1
