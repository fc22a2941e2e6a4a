"""The frame-optimisation contract of include/airfe.h ("Frame optimisation") restated in Python floats and numpy.

Independent of airslam_amd/csrc/poseopt_core.h (which the HIP kernel and the host core share): every step is written again here in the contract's
order.  The scalar work (state, damped solve, Levenberg-Marquardt bookkeeping) is in Python floats (IEEE doubles, no fused multiply-adds, math.sqrt
correctly rounded); the per-edge terms are vectorised, elementwise, in the same operation order, and summed as 64 partials in lane order.  Also the
planted constraints the tests use (tests/pnp_ref.py's geometry, with u_right = x - bf / z from the planted depth for the stereo edges)."""
from __future__ import annotations

import math

import numpy as np

from pnp_ref import BF_EUROC, K_EUROC, _div, gauss, planted, pose_errors, stereo_rows  # noqa: F401  (re-exported for the tests)

LANES = 64
ROUNDS = 3
ITERS = 10
TRIALS = 10
MIN_EDGES = 10
TAU = 1e-5
CAM_EUROC = K_EUROC + (BF_EUROC,)
THR_EUROC = (50.0, 75.0)                     # optimization.tracking mono_point / stereo_point of configs/visual_odometry/vo_euroc.yaml
IDENTITY16 = np.eye(4).reshape(16)


def _camera(Rcb, tcb, wb):
    cw = [0.0] * 12
    for r in range(3):
        for c in range(3):
            cw[3 * r + c] = (Rcb[3 * r] * wb[3 * c] + Rcb[3 * r + 1] * wb[3 * c + 1]) + Rcb[3 * r + 2] * wb[3 * c + 2]
    for r in range(3):
        cw[9 + r] = tcb[r] - ((cw[3 * r] * wb[9] + cw[3 * r + 1] * wb[10]) + cw[3 * r + 2] * wb[11])
    return cw


def _uidx(r, c):
    return r * 6 - (r * (r - 1)) // 2 + (c - r)


class _Problem:
    def __init__(self, X, obs, cam, Tcb, thr):
        self.X, self.Y, self.Z = (np.ascontiguousarray(X[:, k]) for k in range(3))
        self.x, self.y, self.ur = (np.ascontiguousarray(obs[:, k]) for k in range(3))
        self.n = len(X)
        self.fx, self.fy, self.cx, self.cy, self.bf = (float(c) for c in cam)
        self.Rcb = [float(v) for v in Tcb[:9]] if Tcb is not None else [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
        self.tcb = [float(v) for v in Tcb[9:12]] if Tcb is not None else [0.0, 0.0, 0.0]
        R, t = self.Rcb, self.tcb
        self.tbc = [-((R[r] * t[0] + R[3 + r] * t[1]) + R[6 + r] * t[2]) for r in range(3)]
        self.thr = (float(thr[0]), float(thr[1]))
        self.delta = (math.sqrt(self.thr[0]), math.sqrt(self.thr[1]))
        self.st = self.ur > 0.0
        self.thr_e = np.where(self.st, self.thr[1], self.thr[0])
        self.del_e = np.where(self.st, self.delta[1], self.delta[0])

    def errors(self, Rt):
        with np.errstate(all="ignore"):
            xc = Rt[0] * self.X + Rt[1] * self.Y + Rt[2] * self.Z + Rt[9]
            yc = Rt[3] * self.X + Rt[4] * self.Y + Rt[5] * self.Z + Rt[10]
            zc = Rt[6] * self.X + Rt[7] * self.Y + Rt[8] * self.Z + Rt[11]
            iz = 1.0 / zc
            u = xc * iz * self.fx + self.cx
            v = yc * iz * self.fy + self.cy
            e0, e1 = self.x - u, self.y - v
            e2 = np.where(self.st, self.ur - (u - self.bf * iz), 0.0)
            chi2 = (e0 * e0 + e1 * e1) + e2 * e2
        return (e0, e1, e2), (xc, yc, zc), iz, chi2

    def huber(self, chi2):
        d = self.del_e
        with np.errstate(all="ignore"):
            quad = chi2 <= d * d
            s = np.sqrt(chi2)
            w = np.where(quad, 1.0, d / s)
            rho = np.where(quad, chi2, 2.0 * s * d - d * d)
        return rho, w

    def terms(self, Rt):
        """[28, n]: w J^T J (upper, row-major), w J^T e, rho of every edge"""
        (e0, e1, e2), (xc, yc, zc), iz, chi2 = self.errors(Rt)
        rho, w = self.huber(chi2)
        R, st = self.Rcb, self.st
        with np.errstate(all="ignore"):
            a, b = xc * iz, yc * iz
            p00, p02, p11, p12 = self.fx * iz, -(self.fx * a * iz), self.fy * iz, -(self.fy * b * iz)
            p22 = p02 + self.bf * (iz * iz)
            Xb = [((R[r] * xc + R[3 + r] * yc) + R[6 + r] * zc) + self.tbc[r] for r in range(3)]
            A = [[p00 * R[c] + p02 * R[6 + c] for c in range(3)],
                 [p11 * R[3 + c] + p12 * R[6 + c] for c in range(3)],
                 [np.where(st, p00 * R[c] + p22 * R[6 + c], 0.0) for c in range(3)]]
            J = []
            for r in range(3):
                a0, a1, a2 = A[r]
                row = [a2 * Xb[1] - a1 * Xb[2], a0 * Xb[2] - a2 * Xb[0], a1 * Xb[0] - a0 * Xb[1], a0, a1, a2]
                if r == 2:
                    row = [np.where(st, v, 0.0) for v in row]
                J += row
            o = [w * ((J[r] * J[c] + J[6 + r] * J[6 + c]) + J[12 + r] * J[12 + c]) for r in range(6) for c in range(r, 6)]
            o += [w * ((J[r] * e0 + J[6 + r] * e1) + J[12 + r] * e2) for r in range(6)]
            o.append(rho)
            return np.stack(o)

    def _lane_sums(self, vals, level):
        """vals [k, n] -> k totals: 64 partials (partial l over l, l + 64, ... in order) added in lane order; level-1 edges add nothing"""
        k = vals.shape[0]
        part = np.zeros((LANES, k))
        for base in range(0, self.n, LANES):          # partials start at +0, so adding +0 for a skipped edge changes no bit
            blk = vals[:, base:base + LANES] * 1.0
            blk[:, level[base:base + LANES]] = 0.0
            part[:blk.shape[1]] = part[:blk.shape[1]] + blk.T
        tot = []
        for j in range(k):
            s = 0.0
            for l in range(LANES):
                s = s + float(part[l, j])
            tot.append(s)
        return tot

    def sums(self, Rt, level):
        return self._lane_sums(self.terms(Rt), level)

    def chi(self, Rt, level):
        _, _, _, chi2 = self.errors(Rt)
        rho, _ = self.huber(chi2)
        return self._lane_sums(rho[None, :], level)[0]

    def outliers(self, Rt):
        _, _, _, chi2 = self.errors(Rt)
        with np.errstate(all="ignore"):
            return chi2.astype(np.float32).astype(np.float64) > self.thr_e


def cayley(w0, w1, w2):
    nn = (w0 * w0 + w1 * w1) + w2 * w2
    k = 2.0 / (1.0 + nn)
    return [1.0 + k * (w0 * w0 - nn), k * (-w2 + w0 * w1), k * (w1 + w0 * w2),
            k * (w2 + w1 * w0), 1.0 + k * (w1 * w1 - nn), k * (-w0 + w1 * w2),
            k * (-w1 + w2 * w0), k * (w0 + w2 * w1), 1.0 + k * (w2 * w2 - nn)]


def frame_optimize(X, obs, cam=CAM_EUROC, thr=THR_EUROC, Twc0=IDENTITY16, Tcb=None):
    """X [n,3], obs [n,3] -> dict(Twc [4,4], Rt [12], inlier [n] uint8, num_inliers, rounds, trace [3,4] = per round: robust chi at the start pose,
    robust chi at the end, lambda at the end, iterations begun)"""
    X = np.asarray(X, np.float64).reshape(-1, 3)
    obs = np.asarray(obs, np.float64).reshape(-1, 3)
    T0 = [float(v) for v in np.asarray(Twc0, np.float64).reshape(16)]
    P = _Problem(X, obs, cam, None if Tcb is None else np.asarray(Tcb, np.float64).reshape(12), thr)
    n, Rcb, tcb = P.n, P.Rcb, P.tcb
    wb0 = [0.0] * 12
    for r in range(3):
        for c in range(3):
            wb0[3 * r + c] = (T0[4 * r] * Rcb[c] + T0[4 * r + 1] * Rcb[3 + c]) + T0[4 * r + 2] * Rcb[6 + c]
        wb0[9 + r] = ((T0[4 * r] * tcb[0] + T0[4 * r + 1] * tcb[1]) + T0[4 * r + 2] * tcb[2]) + T0[4 * r + 3]
    trace = np.zeros((ROUNDS, 4))
    level = np.zeros(n, bool)
    wb, cur = list(wb0), _camera(Rcb, tcb, wb0)
    rounds = 0
    for rnd in range(ROUNDS):
        if n == 0:
            break
        wb, cur = list(wb0), _camera(Rcb, tcb, wb0)
        rounds += 1
        lam = ni = chi = 0.0
        stop = False
        for it in range(ITERS):
            acc = P.sums(cur, level)
            chi = acc[27]
            if it == 0:
                mx = 0.0
                for j in range(6):
                    d = abs(acc[_uidx(j, j)])
                    mx = d if d > mx else mx
                lam, ni = TAU * mx, 2.0
                trace[rnd, 0] = chi
            trace[rnd, 3] = it + 1
            q = 0
            while True:
                N = []
                for r in range(6):
                    for c in range(6):
                        a = acc[_uidx(r, c) if r <= c else _uidx(c, r)]
                        N.append(a + lam if r == c else a)
                    N.append(-acc[21 + r])
                dx = gauss(N, 6)
                ok = dx is not None
                if not ok:
                    dx = [0.0] * 6
                C = cayley(dx[0] / 2.0, dx[1] / 2.0, dx[2] / 2.0)
                R = wb
                trial = [0.0] * 12
                for r in range(3):
                    for c in range(3):
                        trial[3 * r + c] = (R[3 * r] * C[c] + R[3 * r + 1] * C[3 + c]) + R[3 * r + 2] * C[6 + c]
                    trial[9 + r] = R[9 + r] + ((R[3 * r] * dx[3] + R[3 * r + 1] * dx[4]) + R[3 * r + 2] * dx[5])
                tcur = _camera(Rcb, tcb, trial)
                chi_new = P.chi(tcur, level)
                if not ok:
                    chi_new = math.inf
                scale = 0.0
                for j in range(6):
                    scale = scale + dx[j] * (lam * dx[j] + (-acc[21 + j]))
                scale = scale + 1e-3
                rho = _div(chi - chi_new, scale)
                brk = False
                if rho > 0.0 and math.isfinite(chi_new):
                    x = 2.0 * rho - 1.0
                    alpha = 1.0 - (x * x) * x
                    alpha = (2.0 / 3.0) if (2.0 / 3.0) < alpha else alpha
                    lam = lam * (alpha if (1.0 / 3.0) < alpha else (1.0 / 3.0))
                    ni = 2.0
                    chi = chi_new
                    wb, cur = trial, tcur
                else:
                    lam = lam * ni
                    ni = ni * 2.0
                    brk = not math.isfinite(lam)
                if not brk:
                    q += 1
                if not (not brk and rho < 0.0 and q < TRIALS):
                    stop = q == TRIALS or rho == 0.0 or not math.isfinite(lam)
                    break
            if stop:
                break
        trace[rnd, 1], trace[rnd, 2] = chi, lam
        level = P.outliers(cur)
        if n < MIN_EDGES:
            break
    good = n > 0 and all(math.isfinite(v) for v in wb)
    Twc = np.array(T0).reshape(4, 4)
    if good:
        Twc = np.zeros((4, 4))
        for r in range(3):
            for c in range(3):
                Twc[r, c] = (wb[3 * r] * Rcb[3 * c] + wb[3 * r + 1] * Rcb[3 * c + 1]) + wb[3 * r + 2] * Rcb[3 * c + 2]
            Twc[r, 3] = ((wb[3 * r] * P.tbc[0] + wb[3 * r + 1] * P.tbc[1]) + wb[3 * r + 2] * P.tbc[2]) + wb[9 + r]
        Twc[3, 3] = 1.0
    else:
        cur = _camera(Rcb, tcb, wb0)
    inl = (~level).astype(np.uint8) if good else np.zeros(n, np.uint8)
    Rt = np.array([math.nan if v != v else v for v in cur])        # an output NaN is the canonical quiet NaN
    return dict(Twc=Twc, Rt=Rt, inlier=inl, num_inliers=int(inl.sum()) if good else 0, rounds=rounds, trace=trace)


def use_last(Twc_pnp, pnp_count, Twc_last, lost_num_match):
    """the composite's seed rule (map_builder.cc:310-314)"""
    a, b = np.asarray(Twc_pnp, np.float64).reshape(4, 4), np.asarray(Twc_last, np.float64).reshape(4, 4)
    dx, dy, dz = float(a[0, 3] - b[0, 3]), float(a[1, 3] - b[1, 3]), float(a[2, 3] - b[2, 3])
    return math.sqrt((dx * dx + dy * dy) + dz * dz) > 1.0 or pnp_count < lost_num_match


def planted_constraints(n, ratio, seed, stereo=False, cam=CAM_EUROC):
    """tests/pnp_ref.py's planted problem as constraints: X [n,3] float64 (the float32 points), obs [n,3] = (x, y, u_right) with u_right = -1 (mono)
    or, for every second constraint when `stereo`, x - bf / z from the planted depth; R, t, truth"""
    obj, img, R, t, truth = planted(n, ratio, seed)
    X = obj.astype(np.float64)
    obs = np.concatenate([img.astype(np.float64), np.full((n, 1), -1.0)], 1)
    if stereo:
        z = (X @ R.T + t)[:, 2]
        obs[::2, 2] = obs[::2, 0] - cam[4] / z[::2]
    return X, obs, R, t, truth
