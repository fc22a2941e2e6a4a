"""The PnP RANSAC and stereo-points contracts of include/airfe.h ("PnP RANSAC", "Stereo points") restated in Python floats and numpy.

Independent of airslam_amd/csrc/pnp_core.h (which the HIP kernels and the host core share): every step is written again here as explicit loops in the
contract's order, with no np.linalg in the parts that must match bit for bit (Python floats are IEEE doubles; no fused multiply-adds; math.sqrt is
correctly rounded).  Only the inlier test and the refinement's per-point terms are vectorised, elementwise, in the same operation order.  Also the planted
geometry the tests use: the EuRoC camera, points 1-20 m deep, motion up to 10 deg and 0.5 m, 0.5 px noise, outliers displaced by >= 60 px."""
from __future__ import annotations

import math

import numpy as np

SEED = 0x6A09E667F3BCC909
M64 = (1 << 64) - 1
MAX_ATTEMPTS = 64
MAX_ITERS = 100
MIN_POINTS = 8
THRESH2 = np.float32(400.0)
JACOBI_SWEEPS = 30
GN_ITERS = 5
LM_ITERS = 20
LANES = 64
PINV_TOL = 1e-10
FLT_EPS = 1.1920928955078125e-07
DBL_MIN = 2.2250738585072014e-308
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))

W, H = 752, 480
K_EUROC = (458.654, 457.296, 367.215, 248.375)           # configs/camera/euroc.yaml
BF_EUROC = 458.654 * 0.110073                              # fx * baseline
CAM_EUROC = (1.0, 200.0, 5.0, BF_EUROC) + K_EUROC          # min_x_diff, max_x_diff, max_y_diff, bf, fx, fy, cx, cy


def _div(a, b):
    """IEEE division (Python raises on a zero divisor)"""
    if b != 0.0:
        return a / b
    if a != a or a == 0.0:
        return math.nan
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


# ---- samples ------------------------------------------------------------------------------------------------------------------------------------
def splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(s, attempt, slot, n):
    h = splitmix64(SEED ^ ((s << 32) | (attempt << 8) | slot))
    return ((h >> 32) * n) >> 32


def sample(n, s):
    for a in range(MAX_ATTEMPTS):
        ids = [draw(s, a, k, n) for k in range(5)]
        if len(set(ids)) == 5:
            return ids
    return None


# ---- Jacobi, least squares --------------------------------------------------------------------------------------------------------------------
def jacobi(A, n):
    """A: flat row-major list, diagonalised in place; returns V (flat, eigenvectors in columns)"""
    V = [1.0 if i % (n + 1) == 0 else 0.0 for i in range(n * n)]
    for _ in range(JACOBI_SWEEPS):
        off = dia = 0.0
        for p in range(n):
            dia = dia + A[p * n + p] * A[p * n + p]
            for q in range(p + 1, n):
                off = off + A[p * n + q] * A[p * n + q]
        if off <= 1e-30 * dia:
            break
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = A[p * n + q]
                if apq == 0.0:
                    continue
                th = (A[q * n + q] - A[p * n + p]) / (2.0 * apq)
                t = (1.0 if th >= 0.0 else -1.0) / (abs(th) + math.sqrt(th * th + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                for k in range(n):
                    if k == p:
                        A[p * n + p] = A[p * n + p] - t * apq
                        A[p * n + q] = 0.0
                    elif k == q:
                        A[q * n + q] = A[q * n + q] + t * apq
                        A[q * n + p] = 0.0
                    else:
                        akp, akq = A[k * n + p], A[k * n + q]
                        nkp, nkq = c * akp - s * akq, s * akp + c * akq
                        A[k * n + p] = A[p * n + k] = nkp
                        A[k * n + q] = A[q * n + k] = nkq
                    vkp, vkq = V[k * n + p], V[k * n + q]
                    V[k * n + p] = c * vkp - s * vkq
                    V[k * n + q] = s * vkp + c * vkq
    return V


def rank(A, n, i):
    di = A[i * n + i]
    return sum(1 for j in range(n) if A[j * n + j] < di or (A[j * n + j] == di and j < i))


def gauss(N, m):
    w = m + 1
    for k in range(m):
        p, best = k, abs(N[k * w + k])
        for r in range(k + 1, m):
            if abs(N[r * w + k]) > best:
                best, p = abs(N[r * w + k]), r
        if not best > 0.0:
            return None
        if p != k:
            for c in range(k, m + 1):
                N[k * w + c], N[p * w + c] = N[p * w + c], N[k * w + c]
        for r in range(k + 1, m):
            f = N[r * w + k] / N[k * w + k]
            for c in range(k, m + 1):
                N[r * w + c] = N[r * w + c] - f * N[k * w + c]
    x = [0.0] * m
    for k in range(m - 1, -1, -1):
        s = N[k * w + m]
        for c in range(k + 1, m):
            s = s - N[k * w + c] * x[c]
        x[k] = s / N[k * w + k]
    return x


def lsq(A, b, rows, cols):
    N = [0.0] * (cols * (cols + 1))
    for r in range(cols):
        for c in range(cols):
            s = 0.0
            for i in range(rows):
                s = s + A[i * cols + r] * A[i * cols + c]
            N[r * (cols + 1) + c] = s
        s = 0.0
        for i in range(rows):
            s = s + A[i * cols + r] * b[i]
        N[r * (cols + 1) + cols] = s
    return gauss(N, cols)


# ---- projection --------------------------------------------------------------------------------------------------------------------------------
def project(Rt, X, Y, Z, K):
    xc = Rt[0] * X + Rt[1] * Y + Rt[2] * Z + Rt[9]
    yc = Rt[3] * X + Rt[4] * Y + Rt[5] * Z + Rt[10]
    zc = Rt[6] * X + Rt[7] * Y + Rt[8] * Z + Rt[11]
    iz = 1.0 / zc if zc != 0.0 else 1.0
    return xc * iz * K[0] + K[2], yc * iz * K[1] + K[3]


def errors(Rt, obj, img, K):
    """float32 [n]: the inlier test's error of every correspondence (obj / img float32 arrays)"""
    X, Y, Z = (obj[:, k].astype(np.float64) for k in range(3))
    with np.errstate(all="ignore"):
        xc = Rt[0] * X + Rt[1] * Y + Rt[2] * Z + Rt[9]
        yc = Rt[3] * X + Rt[4] * Y + Rt[5] * Z + Rt[10]
        zc = Rt[6] * X + Rt[7] * Y + Rt[8] * Z + Rt[11]
        iz = np.where(zc != 0.0, 1.0 / np.where(zc != 0.0, zc, 1.0), 1.0)
        pu = (xc * iz * K[0] + K[2]).astype(np.float32)
        pv = (yc * iz * K[1] + K[3]).astype(np.float32)
        dx = img[:, 0] - pu
        dy = img[:, 1] - pv
        return dx * dx + dy * dy


# ---- EPnP ---------------------------------------------------------------------------------------------------------------------------------------
def _compute_rt(be, NS, al, pw, uv, K):
    ccs = [0.0] * 12
    for i in range(4):
        for j in range(12):
            ccs[j] = ccs[j] + be[i] * NS[12 * i + j]
    pcs = [al[4 * i] * ccs[c] + al[4 * i + 1] * ccs[3 + c] + al[4 * i + 2] * ccs[6 + c] + al[4 * i + 3] * ccs[9 + c] for i in range(5) for c in range(3)]
    if pcs[2] < 0.0:
        pcs = [-x for x in pcs]
    pc0, pw0 = [], []
    for c in range(3):
        sc = sw = 0.0
        for i in range(5):
            sc = sc + pcs[3 * i + c]
            sw = sw + pw[3 * i + c]
        pc0.append(sc / 5.0)
        pw0.append(sw / 5.0)
    S = [0.0] * 9
    for a in range(3):
        for b in range(3):
            s = 0.0
            for i in range(5):
                s = s + (pw[3 * i + a] - pw0[a]) * (pcs[3 * i + b] - pc0[b])
            S[3 * a + b] = s
    N = [0.0] * 16
    N[0] = (S[0] + S[4]) + S[8]; N[1] = S[5] - S[7]; N[2] = S[6] - S[2]; N[3] = S[1] - S[3]
    N[5] = (S[0] - S[4]) - S[8]; N[6] = S[1] + S[3]; N[7] = S[6] + S[2]
    N[10] = (S[4] - S[0]) - S[8]; N[11] = S[5] + S[7]
    N[15] = (S[8] - S[0]) - S[4]
    N[4], N[8], N[12], N[9], N[13], N[14] = N[1], N[2], N[3], N[6], N[7], N[11]
    V = jacobi(N, 4)
    col = 0
    for j in range(4):
        col = j if rank(N, 4, j) == 3 else col
    w, x, y, z = V[col], V[4 + col], V[8 + col], V[12 + col]
    nrm = math.sqrt(((w * w + x * x) + y * y) + z * z)
    w, x, y, z = _div(w, nrm), _div(x, nrm), _div(y, nrm), _div(z, nrm)
    ww, xx, yy, zz = w * w, x * x, y * y, z * z
    R = [((ww + xx) - yy) - zz, 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
         2.0 * (x * y + w * z), ((ww - xx) + yy) - zz, 2.0 * (y * z - w * x),
         2.0 * (x * z - w * y), 2.0 * (y * z + w * x), ((ww - xx) - yy) + zz]
    Rt = R + [pc0[r] - ((R[3 * r] * pw0[0] + R[3 * r + 1] * pw0[1]) + R[3 * r + 2] * pw0[2]) for r in range(3)]
    err = 0.0
    for i in range(5):
        u, v = project(Rt, pw[3 * i], pw[3 * i + 1], pw[3 * i + 2], K)
        du, dv = u - uv[2 * i], v - uv[2 * i + 1]
        err = err + math.sqrt(du * du + dv * dv) if du * du + dv * dv >= 0.0 else math.nan
    fin = math.isfinite(err) and all(math.isfinite(r) for r in Rt)
    return (err if fin else math.nan), Rt


def epnp(pw, uv, K):
    """pw [15], uv [10] Python floats -> the model (R row-major + t, 12 floats) or None"""
    fx, fy, cx, cy = K
    cw = [0.0] * 12
    for c in range(3):
        s = 0.0
        for i in range(5):
            s = s + pw[3 * i + c]
        cw[c] = s / 5.0
    S3 = [0.0] * 9
    for a in range(3):
        for b in range(3):
            s = 0.0
            for i in range(5):
                s = s + (pw[3 * i + a] - cw[a]) * (pw[3 * i + b] - cw[b])
            S3[3 * a + b] = s
    V3 = jacobi(S3, 3)
    sc, cols = [0.0] * 3, [0] * 3
    for col in range(3):
        j = 2 - rank(S3, 3, col)
        d = S3[4 * col]
        sc[j] = math.sqrt((d if d > 0.0 else 0.0) / 5.0)
        cols[j] = col
    for j in range(3):
        for c in range(3):
            cw[3 * (j + 1) + c] = cw[c] + sc[j] * V3[3 * c + cols[j]]
    al = [0.0] * 20
    for i in range(5):
        for j in range(3):
            col = cols[j]
            proj = (pw[3 * i] - cw[0]) * V3[col] + (pw[3 * i + 1] - cw[1]) * V3[3 + col] + (pw[3 * i + 2] - cw[2]) * V3[6 + col]
            al[4 * i + 1 + j] = proj / sc[j] if sc[j] > PINV_TOL * sc[0] else 0.0
        al[4 * i] = ((1.0 - al[4 * i + 1]) - al[4 * i + 2]) - al[4 * i + 3]
    MM = [0.0] * 144
    for i in range(5):
        u, v = uv[2 * i], uv[2 * i + 1]
        row = [0.0] * 24
        for j in range(4):
            a = al[4 * i + j]
            row[3 * j], row[3 * j + 2] = a * fx, a * (cx - u)
            row[12 + 3 * j + 1], row[12 + 3 * j + 2] = a * fy, a * (cy - v)
        for r in range(12):
            for c in range(r, 12):
                MM[12 * r + c] = MM[12 * r + c] + (row[r] * row[c] + row[12 + r] * row[12 + c])
    for r in range(1, 12):
        for c in range(r):
            MM[12 * r + c] = MM[12 * c + r]
    VV = jacobi(MM, 12)
    NS = [0.0] * 48
    for col in range(12):
        r = rank(MM, 12, col)
        if r < 4:
            for j in range(12):
                NS[12 * r + j] = VV[12 * j + col]
    L, rho = [], []
    for a, b in PAIRS:
        dv = [NS[12 * k + 3 * a + c] - NS[12 * k + 3 * b + c] for k in range(4) for c in range(3)]

        def dot(k, l):
            return dv[3 * k] * dv[3 * l] + dv[3 * k + 1] * dv[3 * l + 1] + dv[3 * k + 2] * dv[3 * l + 2]
        L += [dot(0, 0), 2.0 * dot(0, 1), dot(1, 1), 2.0 * dot(0, 2), 2.0 * dot(1, 2), dot(2, 2), 2.0 * dot(0, 3), 2.0 * dot(1, 3), 2.0 * dot(2, 3),
              dot(3, 3)]
        d0, d1, d2 = cw[3 * a] - cw[3 * b], cw[3 * a + 1] - cw[3 * b + 1], cw[3 * a + 2] - cw[3 * b + 2]
        rho.append(d0 * d0 + d1 * d1 + d2 * d2)
    best, best_err = None, math.inf
    for N in (1, 2, 3):
        cs = (0, 1, 3, 6) if N == 1 else ((0, 1, 2) if N == 2 else (0, 1, 2, 3, 4))
        x = lsq([L[10 * i + c] for i in range(6) for c in cs], rho, 6, len(cs))
        if x is None:
            continue
        if N == 1:
            s = math.sqrt(-x[0]) if x[0] < 0.0 else math.sqrt(x[0])
            sg = -1.0 if x[0] < 0.0 else 1.0
            be = [s, _div(sg * x[1], s), _div(sg * x[2], s), _div(sg * x[3], s)]
        else:
            x2 = x[2]
            if x[0] < 0.0:
                b0, b1 = math.sqrt(-x[0]), (math.sqrt(-x2) if x2 < 0.0 else 0.0)
            else:
                b0, b1 = math.sqrt(x[0]), (math.sqrt(x2) if x2 > 0.0 else 0.0)
            if x[1] < 0.0:
                b0 = -b0
            be = [b0, b1, _div(x[3], b0) if N == 3 else 0.0, 0.0]
        for _ in range(GN_ITERS):
            A, res = [], []
            b0, b1, b2, b3 = be
            for i in range(6):
                l = L[10 * i:10 * i + 10]
                A += [2.0 * l[0] * b0 + l[1] * b1 + l[3] * b2 + l[6] * b3, l[1] * b0 + 2.0 * l[2] * b1 + l[4] * b2 + l[7] * b3,
                      l[3] * b0 + l[4] * b1 + 2.0 * l[5] * b2 + l[8] * b3, l[6] * b0 + l[7] * b1 + l[8] * b2 + 2.0 * l[9] * b3]
                res.append(rho[i] - (l[0] * b0 * b0 + l[1] * b0 * b1 + l[2] * b1 * b1 + l[3] * b0 * b2 + l[4] * b1 * b2 + l[5] * b2 * b2 +
                                     l[6] * b0 * b3 + l[7] * b1 * b3 + l[8] * b2 * b3 + l[9] * b3 * b3))
            x = lsq(A, res, 6, 4)
            if x is None:
                break
            be = [be[k] + x[k] for k in range(4)]
        err, Rt = _compute_rt(be, NS, al, pw, uv, K)
        if err == err and (best is None or err < best_err):
            best, best_err = Rt, err
    return best


# ---- the sequential rule ---------------------------------------------------------------------------------------------------------------------
def update_niters(n, good, max_iters):
    ep = (n - good) / n
    num = 1.0 - 0.99
    q = 1.0 - ep
    q2 = q * q
    q4 = q2 * q2
    den = 1.0 - q4 * q
    if den < DBL_MIN:
        return 0
    ln, ld = math.log(num), math.log(den)
    return max_iters if (ld >= 0.0 or -ln >= max_iters * (-ld)) else int(round(ln / ld))


# ---- Levenberg-Marquardt ----------------------------------------------------------------------------------------------------------------------
def _lm_terms(Rt, X, Y, Z, u, v, K):
    """[28, n]: J^T J (upper, row-major), J^T r, r^T r of every point (zeros where z == 0), elementwise in the contract's order"""
    with np.errstate(all="ignore"):
        p0 = Rt[0] * X + Rt[1] * Y + Rt[2] * Z
        p1 = Rt[3] * X + Rt[4] * Y + Rt[5] * Z
        p2 = Rt[6] * X + Rt[7] * Y + Rt[8] * Z
        xc, yc, zc = p0 + Rt[9], p1 + Rt[10], p2 + Rt[11]
        iz = 1.0 / np.where(zc != 0.0, zc, 1.0)
        a, b = xc * iz, yc * iz
        ru, rv = (a * K[0] + K[2]) - u, (b * K[1] + K[3]) - v
        gu0, gu2, gv1, gv2 = K[0] * iz, -(K[0] * a * iz), K[1] * iz, -(K[1] * b * iz)
        zero = np.zeros_like(X)
        J = [gu2 * (2.0 * p1), gu0 * (2.0 * p2) + gu2 * (-2.0 * p0), gu0 * (-2.0 * p1), gu0, zero, gu2,
             gv1 * (-2.0 * p2) + gv2 * (2.0 * p1), gv2 * (-2.0 * p0), gv1 * (2.0 * p0), zero, gv1, gv2]
        o = [J[r] * J[c] + J[6 + r] * J[6 + c] for r in range(6) for c in range(r, 6)]
        o += [J[r] * ru + J[6 + r] * rv for r in range(6)]
        o.append(ru * ru + rv * rv)
        out = np.stack(o)
    out[:, zc == 0.0] = 0.0
    return out


def _accumulate(Rt, obj64, img64, mask, K):
    n = len(mask)
    terms = _lm_terms(Rt, obj64[:, 0], obj64[:, 1], obj64[:, 2], img64[:, 0], img64[:, 1], K)
    part = np.zeros((LANES, 28))
    for base in range(0, n, LANES):              # lane l adds point base + l: partials start at +0, so adding +0 for an outlier changes no bit
        blk = terms[:, base:base + LANES] * 1.0
        blk[:, ~mask[base:base + LANES]] = 0.0
        part[:blk.shape[1]] = part[:blk.shape[1]] + blk.T
    tot = [0.0] * 28
    for k in range(28):
        s = 0.0
        for l in range(LANES):
            s = s + float(part[l, k])
        tot[k] = s
    return tot


def _uidx(r, c):
    return r * 6 - (r * (r - 1)) // 2 + (c - r)


def refine(M, obj, img, mask, K):
    obj64, img64 = obj.astype(np.float64), img.astype(np.float64)
    acc = _accumulate(M, obj64, img64, mask, K)
    cur, lam = list(M), 1e-3
    stop = not (math.isfinite(acc[27]) and acc[27] > 0.0)
    for _ in range(LM_ITERS):
        if stop:
            break
        N = []
        for r in range(6):
            for c in range(6):
                a = acc[_uidx(r, c) if r <= c else _uidx(c, r)]
                N.append(a * (1.0 + lam) if r == c else a)
            N.append(-acc[21 + r])
        d = gauss(N, 6)
        if d is None:
            break
        w0, w1, w2 = d[0], d[1], d[2]
        nn = (w0 * w0 + w1 * w1) + w2 * w2
        k = 2.0 / (1.0 + nn)
        C = [1.0 + k * (w0 * w0 - nn), k * (-w2 + w0 * w1), k * (w1 + w0 * w2),
             k * (w2 + w1 * w0), 1.0 + k * (w1 * w1 - nn), k * (-w0 + w1 * w2),
             k * (-w1 + w2 * w0), k * (w0 + w2 * w1), 1.0 + k * (w2 * w2 - nn)]
        R = cur
        trial = [(C[3 * r] * R[c] + C[3 * r + 1] * R[3 + c]) + C[3 * r + 2] * R[6 + c] for r in range(3) for c in range(3)]
        trial += [R[9 + r] + d[3 + r] for r in range(3)]
        tot = _accumulate(trial, obj64, img64, mask, K)
        if tot[27] < acc[27]:
            cur, acc, lam = trial, tot, lam / 10.0
            mx = 0.0
            for q in d:
                mx = abs(q) if abs(q) > mx else mx
            if mx < FLT_EPS:
                stop = True
        else:
            lam = lam * 10.0
    return cur if all(math.isfinite(x) for x in cur) else list(M)


def twc(Rt):
    T = np.zeros((4, 4))
    for r in range(3):
        for c in range(3):
            T[r, c] = Rt[3 * c + r]
        T[r, 3] = (Rt[r] * (-Rt[9]) + Rt[3 + r] * (-Rt[10])) + Rt[6 + r] * (-Rt[11])
    T[3, 3] = 1.0
    return T


IDENTITY12 = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]


def pnp_ransac(obj, img, K=K_EUROC):
    """obj [n,3], img [n,2] (rounded to float32 here) -> dict(Twc [4,4], Rt [12], inlier [n] uint8, count, win, scores {sample: inliers or -1})"""
    obj = np.asarray(obj, np.float64).astype(np.float32).reshape(-1, 3)
    img = np.asarray(img, np.float64).astype(np.float32).reshape(-1, 2)
    K = tuple(float(k) for k in K)
    n = len(obj)
    out = dict(Twc=np.eye(4), Rt=np.array(IDENTITY12), inlier=np.zeros(n, np.uint8), count=0, win=-1, scores={})
    if n < MIN_POINTS:
        return out
    niters, bc, win, model = MAX_ITERS, 0, -1, None
    s = 0
    while s < niters and s < MAX_ITERS:
        ids = sample(n, s)
        M = None
        if ids is not None:
            M = epnp([float(obj[i, c]) for i in ids for c in range(3)], [float(img[i, c]) for i in ids for c in range(2)], K)
        c = int((errors(M, obj, img, K) <= THRESH2).sum()) if M is not None else -1
        out["scores"][s] = c
        if c > max(bc, 4):
            bc, win, model = c, s, M
            niters = update_niters(n, c, niters)
        s += 1
    if win < 0:
        return out
    mask = errors(model, obj, img, K) <= THRESH2
    res = refine(model, obj, img, mask, K)
    out.update(Twc=twc(res), Rt=np.array(res), inlier=mask.astype(np.uint8), count=bc, win=win)
    return out


# ---- stereo points -------------------------------------------------------------------------------------------------------------------------------
def stereo_points(featL, featR, idx, cam=CAM_EUROC):
    """Frame::AddRightFeatures + BackProjectPoint: -> dict(u_right [nL], depth [nL], xyz [nL,3], good)"""
    mn, mx, my, bf, fx, fy, cx, cy = (float(c) for c in cam)
    nL = len(featL)
    u, d, xyz = np.full(nL, -1.0), np.full(nL, -1.0), np.full((nL, 3), np.nan)
    good = 0
    for l, r in np.asarray(idx).reshape(-1, 2):
        xl, yl = np.float32(featL[l, 1]), np.float32(featL[l, 2])
        xr, yr = np.float32(featR[r, 1]), np.float32(featR[r, 2])
        dx, dy = float(abs(xl - xr)), float(abs(yl - yr))
        if not (dx > mn and dx < mx and dy <= my):
            continue
        par = float(xl - xr)
        if not (par < mx and par > mn):
            continue
        good += 1
        u[l] = float(xr)
        d[l] = bf / par
        x, y = (float(xl) - cx) * (1.0 / fx), (float(yl) - cy) * (1.0 / fy)
        dd = bf / (float(xl) - u[l])
        xyz[l] = (x * dd, y * dd, 1.0 * dd)
    return dict(u_right=u, depth=d, xyz=xyz, good=good)


# ---- planted geometry ---------------------------------------------------------------------------------------------------------------------------
def rotation(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    th = np.deg2rad(deg)
    return np.eye(3) + np.sin(th) * Kx + (1.0 - np.cos(th)) * (Kx @ Kx)


def planted_motion(rng, max_deg=10.0, max_t=0.5):
    R = rotation(rng.normal(size=3), rng.uniform(0.0, max_deg))
    t = rng.normal(size=3)
    t = t / np.linalg.norm(t) * rng.uniform(0.4 * max_t, max_t)
    return R, t


def planted(n, inlier_ratio, seed, planar=False, K=K_EUROC):
    """n keyframe-frame points (1-20 m deep, or all at z = 8 m when planar) seen from a camera moved by (R, t) (Xc = R X + t): obj [n,3] float32,
    img [n,2] float32 (0.5 px noise; outliers displaced by 60-200 px), R, t, truth [n] bool"""
    fx, fy, cx, cy = K
    rng = np.random.default_rng(seed)
    R, t = planted_motion(rng)
    z = np.full(n, 8.0) if planar else rng.uniform(1.0, 20.0, n)
    u0, v0 = rng.uniform(0, W, n), rng.uniform(0, H, n)
    X = np.stack([(u0 - cx) / fx * z, (v0 - cy) / fy * z, z], 1)
    Pc = X @ R.T + t
    img = np.stack([Pc[:, 0] / Pc[:, 2] * fx + cx, Pc[:, 1] / Pc[:, 2] * fy + cy], 1) + rng.normal(0.0, 0.5, (n, 2))
    nout = int(round(n * (1.0 - inlier_ratio)))
    out = rng.choice(n, nout, replace=False)
    dirs = rng.normal(size=(nout, 2))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    img[out] += dirs * rng.uniform(60.0, 200.0, (nout, 1))
    truth = np.ones(n, bool)
    truth[out] = False
    return X.astype(np.float32), img.astype(np.float32), R, t, truth


def pose_errors(Rt, R, t):
    """(rotation error in degrees, translation error in metres) of a result's Rcw, tcw against the planted motion"""
    Re = np.asarray(Rt[:9]).reshape(3, 3)
    ang = np.rad2deg(np.arccos(np.clip((np.trace(Re.T @ R) - 1.0) / 2.0, -1.0, 1.0)))
    return float(ang), float(np.linalg.norm(np.asarray(Rt[9:12]) - t))


def stereo_rows(n, seed, K=K_EUROC, bf=BF_EUROC):
    """a planted rectified stereo keyframe: left / right rows [n,259] (x, y in pixels) with the list idx [n,2] = (i, perm(i)) over a shuffled right
    side, and the true keyframe points [n,3]"""
    fx, fy, cx, cy = K
    rng = np.random.default_rng(seed)
    z = np.where(rng.random(n) < 0.2, rng.uniform(0.25, 0.6, n), rng.uniform(1.0, 20.0, n))      # a fifth near: disparities of 80-190 px
    xl, yl = rng.uniform(200, W - 10, n), rng.uniform(0, H, n)
    xr = xl - bf / z
    fL = np.zeros((n, 259), np.float32)
    fR = np.zeros((n, 259), np.float32)
    perm = rng.permutation(n)
    fL[:, 1], fL[:, 2] = xl, yl
    fR[perm, 1], fR[perm, 2] = xr, yl + rng.normal(0.0, 0.3, n)
    X = np.stack([(xl - cx) / fx * z, (yl - cy) / fy * z, z], 1)
    return fL, fR, np.stack([np.arange(n), perm], 1).astype(np.int32), X
