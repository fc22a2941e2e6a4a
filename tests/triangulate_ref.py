"""Map-point triangulation (include/airfe.h "Map-point triangulation"; airslam_amd/csrc/triangulate_core.h) restated in plain Python floats:
Map::TriangulateMappoint (src/map.cc:367-414) over dicts of observers, the same sequential sums, the same column-pivoted Householder QR.  Also the point
table's fill, an independent formulation through numpy.linalg.solve, and the tables and scenes the tests share."""
import math

import numpy as np

NAN = float("nan")
TINY = 2.2250738585072014e-308
RANK_TOL = 1e-5
CAM = (400.0, 410.0, 320.0, 240.0)                                  # fx, fy, cx, cy of every table below


def cam_inverse(cam):
    return (1.0 / float(cam[0]), 1.0 / float(cam[1]), float(cam[2]), float(cam[3]))


def qr_solve(A, rhs):
    """A: 9 floats row-major, rhs: 3 floats -> (rank, x or None, R's diagonal).  tr_qr_solve, line by line."""
    a, c, perm = list(A), list(rhs), [0, 1, 2]

    def swap(j, k):
        for r in range(3):
            a[3 * r + j], a[3 * r + k] = a[3 * r + k], a[3 * r + j]
        perm[j], perm[k] = perm[k], perm[j]

    # step 0
    n0 = (a[0] * a[0] + a[3] * a[3]) + a[6] * a[6]
    n1 = (a[1] * a[1] + a[4] * a[4]) + a[7] * a[7]
    n2 = (a[2] * a[2] + a[5] * a[5]) + a[8] * a[8]
    p, best = 0, n0
    if n1 > best:
        p, best = 1, n1
    if n2 > best:
        p = 2
    if p:
        swap(0, p)
    tail, c0 = a[3] * a[3] + a[6] * a[6], a[0]
    tau, beta, e1, e2 = 0.0, c0, 0.0, 0.0
    if not tail <= TINY:
        beta = math.sqrt(c0 * c0 + tail)
        if c0 >= 0.0:
            beta = -beta
        e1 = a[3] / (c0 - beta)
        e2 = a[6] / (c0 - beta)
        tau = (beta - c0) / beta
    a[0] = beta
    if tau != 0.0:
        t1, t2 = tau * e1, tau * e2
        for j in (1, 2):
            tmp = e1 * a[3 + j] + e2 * a[6 + j]
            tmp += a[j]
            a[j] -= tau * tmp
            a[3 + j] -= t1 * tmp
            a[6 + j] -= t2 * tmp
        tmp = e1 * c[1] + e2 * c[2]
        tmp += c[0]
        c[0] -= tau * tmp
        c[1] -= t1 * tmp
        c[2] -= t2 * tmp
    # step 1
    n1 = a[4] * a[4] + a[7] * a[7]
    n2 = a[5] * a[5] + a[8] * a[8]
    if n2 > n1:
        swap(1, 2)
    tail, c0 = a[7] * a[7], a[4]
    tau, beta, e = 0.0, c0, 0.0
    if not tail <= TINY:
        beta = math.sqrt(c0 * c0 + tail)
        if c0 >= 0.0:
            beta = -beta
        e = a[7] / (c0 - beta)
        tau = (beta - c0) / beta
    a[4] = beta
    if tau != 0.0:
        t1 = tau * e
        tmp = e * a[8]
        tmp += a[5]
        a[5] -= tau * tmp
        a[8] -= t1 * tmp
        tmp = e * c[2]
        tmp += c[1]
        c[1] -= tau * tmp
        c[2] -= t1 * tmp
    # step 2: the last entry is its own pivot
    rdiag = (a[0], a[4], a[8])
    r = [abs(v) for v in rdiag]
    maxp = r[0]
    if r[1] > maxp:
        maxp = r[1]
    if r[2] > maxp:
        maxp = r[2]
    thr = maxp * RANK_TOL
    rank = sum(1 for v in r if v > thr)
    if rank < 3:
        return rank, None, rdiag
    y2 = c[2] / a[8]
    y1 = (c[1] - a[5] * y2) / a[4]
    y0 = (c[0] - (a[1] * y1 + a[2] * y2)) / a[0]
    x = [0.0, 0.0, 0.0]
    for i, y in enumerate((y0, y1, y2)):
        x[perm[i]] = y
    return rank, x, rdiag


def system(cami, observers):
    """observers: [(x, y, T)] in observer order, x / y floats (a float32's value), T the 16 floats of Twc -> (A [9], rhs [3], bad)"""
    M, g, Cs, bad = [0.0] * 9, [0.0] * 3, [0.0] * 3, False
    for x, y, T in observers:
        b0, b1, b2 = (x - cami[2]) * cami[0], (y - cami[3]) * cami[1], 1.0
        v = [(T[4 * r] * b0 + T[4 * r + 1] * b1) + T[4 * r + 2] * b2 for r in range(3)]
        c = [T[4 * r + 3] for r in range(3)]
        s = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
        if not (math.isfinite(x) and math.isfinite(y) and all(math.isfinite(T[k]) for k in range(12)) and math.isfinite(s) and s != 0.0):
            bad = True                                              # (the sums no longer matter: the point's status is 1 or 3)
            continue
        inv = 1.0 / s
        d = (v[0] * c[0] + v[1] * c[1]) + v[2] * c[2]
        w = [v[r] * inv for r in range(3)]
        for r in range(3):
            for q in range(3):
                M[3 * r + q] += w[r] * v[q]
            g[r] += w[r] * d
            Cs[r] += c[r]
    n = float(len(observers))
    A = [(n if r == q else 0.0) - M[3 * r + q] for r in range(3) for q in range(3)]
    rhs = [Cs[r] - g[r] for r in range(3)]
    return A, rhs, bad


def point(cam, observers, min_observers=2):
    """-> (xyz [3], status, R's diagonal or None)"""
    nan3 = [NAN, NAN, NAN]
    if not observers:
        return nan3, -1, None
    if len(observers) < max(min_observers, 2):
        return nan3, 1, None
    A, rhs, bad = system(cam_inverse(cam), observers)
    if bad or not all(math.isfinite(v) for v in A + rhs):
        return nan3, 3, None
    rank, x, rdiag = qr_solve(A, rhs)
    if rank < 3:
        return nan3, 2, rdiag
    if not all(math.isfinite(v) for v in x):
        return nan3, 3, rdiag
    return x, 0, rdiag


def observers_of(xy, n, pose, point_id, size, max_points):
    """point -> {frame: row}: the FIRST valid row of the frame holding the point"""
    cap = point_id.shape[1]
    obs = {}
    for f in range(size):
        for i in range(max(0, min(int(n[f]), cap))):
            m = int(point_id[f][i])
            if 0 <= m < max_points:
                obs.setdefault(m, {}).setdefault(f, i)
    return obs


def build(xy, n, pose, point_id, size, max_points, cam=CAM, min_observers=2):
    """xy [>= size][cap][2] float32, n [>= size], pose [>= size][16] float64, point_id [>= size][cap] -> (xyz [max_points][3] f64, status i32, nobs i32, info [4])"""
    obs = observers_of(xy, n, pose, point_id, size, max_points)
    xyz = np.full((max_points, 3), np.nan, np.float64)
    status, nobs = np.full(max_points, -1, np.int32), np.zeros(max_points, np.int32)
    for m, frames in obs.items():
        lst = [(float(xy[f][i][0]), float(xy[f][i][1]), [float(t) for t in pose[f]]) for f, i in sorted(frames.items())]
        x, st, _ = point(cam, lst, min_observers)
        xyz[m], status[m], nobs[m] = x, st, len(lst)
    info = [int((status == 0).sum()), int((status != -1).sum()), int((status == 2).sum()), int((status == 3).sum())]
    return xyz, status, nobs, info


def fill(points, n, point_id, size, max_points, xyz, status, only_missing):
    """-> (the point table after airfe_bowdb_fill_points_dev, the rows written)"""
    out, written = points.copy(), 0
    cap = point_id.shape[1]
    for f in range(size):
        for i in range(max(0, min(int(n[f]), cap))):
            m = int(point_id[f][i])
            if 0 <= m < max_points and status[m] == 0 and (not only_missing or math.isnan(out[f][i][0])):
                out[f][i] = xyz[m]
                written += 1
    return out, written


def same(got, want):
    """byte for byte, the NaN pattern included: (xyz, status, nobs, info)"""
    return (np.array_equal(np.ascontiguousarray(got[0], np.float64).view(np.uint64), np.ascontiguousarray(want[0], np.float64).view(np.uint64)) and
            np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and list(got[3]) == list(want[3]))


def independent(cam, observers):
    """A = sum (I - v v^T / |v|^2), rhs = sum (I - v v^T / |v|^2) c, numpy.linalg.solve in float64 from the same rounded inputs"""
    A, rhs = np.zeros((3, 3)), np.zeros(3)
    for x, y, T in observers:
        T = np.asarray(T, np.float64).reshape(4, 4)
        v = T[:3, :3] @ np.array([(x - cam[2]) / cam[0], (y - cam[3]) / cam[1], 1.0])
        P = np.eye(3) - np.outer(v, v) / (v @ v)
        A += P
        rhs += P @ T[:3, 3]
    return np.linalg.solve(A, rhs)


# ---- geometry ---------------------------------------------------------------------------------------------------------------------------------------
def pose_on_path(f, frames, rng=None):
    """Twc [16] of frame f: a camera moving along x with a slow yaw and a little pitch, looking down +z"""
    yaw, pitch = 0.25 * math.sin(0.37 * f), 0.05 * math.cos(0.21 * f)
    cy_, sy_, cp, sp = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch)
    Ry = np.array([[cy_, 0, sy_], [0, 1, 0], [-sy_, 0, cy_]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    T = np.eye(4)
    T[:3, :3] = Ry @ Rx
    T[:3, 3] = [12.0 * f / max(frames - 1, 1) - 6.0, 0.4 * math.sin(0.9 * f), 0.3 * math.cos(0.5 * f)]
    return T.reshape(16)


def project(cam, T, X):
    """the pixel of world point X in the camera of pose T (float64), and its depth"""
    T = np.asarray(T, np.float64).reshape(4, 4)
    Xc = T[:3, :3].T @ (np.asarray(X, np.float64) - T[:3, 3])
    return cam[0] * Xc[0] / Xc[2] + cam[2], cam[1] * Xc[1] / Xc[2] + cam[3], Xc[2]


def cloud(P, rng):
    return np.stack([rng.uniform(-7, 7, P), rng.uniform(-3, 3, P), rng.uniform(5, 14, P)], 1)


def seeded_table(frames=40, cap=64, max_points=300, seed=3, noise=0.3):
    """a seeded map: a cloud seen along a path with pixel noise.  ids of -1, ids out of range, points at two rows of one frame, wrong associations, n in
    {0, 1, 63, 64}, points nobody sees, points seen once -> (xy f32 [frames][cap][2], n, pose [frames][16], ids i32 [frames][cap], the cloud)"""
    rng = np.random.default_rng(seed)
    X = cloud(max_points, rng)
    pose = np.stack([pose_on_path(f, frames) for f in range(frames)])
    n = np.array([(cap, cap - 1, 40, 1, 0, 17, cap, 33)[f % 8] for f in range(frames)], np.int32)
    ids = rng.integers(-3, max_points + 3, size=(frames, cap)).astype(np.int32)        # what lies past n[f] is never read
    xy = rng.uniform(0, 600, size=(frames, cap, 2)).astype(np.float32)
    seen = max_points - 20                                                            # the last 20 points: nobody's
    for f in range(frames):
        k = int(n[f])
        m = rng.integers(0, seen, size=k)
        near = (rng.integers(0, 30, size=k) + 4 * f) % seen                          # neighbouring frames share a window of ids
        m = np.where(rng.random(k) < 0.7, near, m)
        for i in range(k):
            u, v, _ = project(CAM, pose[f], X[m[i]])
            xy[f, i] = (u + rng.normal(0, noise), v + rng.normal(0, noise))
        row = m.astype(np.int64)
        row[rng.random(k) < 0.12] = -1
        bad = rng.random(k) < 0.03
        row[bad] = rng.choice([-2, max_points, max_points + 7, -2 ** 31, 2 ** 31 - 1], size=int(bad.sum()))
        ids[f, :k] = row.astype(np.int32)
    ids[0, 5], ids[0, 9] = ids[0, 2], ids[0, 2]                                        # one point at three rows of frame 0 (its first row counts)
    ids[2, 30] = ids[2, 3]
    ids[1, 0] = seen + 1                                                              # a point seen exactly once
    return xy, n, pose, ids, X


def planted_scene(frames=12, cap=48, P=120, seed=8):
    """noise-free projections of a known cloud from `frames` known poses, stored as float32 keypoints: every frame sees a random subset; points 0 .. 5 are
    seen by exactly 0, 1, 2, 3, 4, 5 frames -> (xy, n, pose, ids, X)"""
    rng = np.random.default_rng(seed)
    X = cloud(P, rng)
    pose = np.stack([pose_on_path(3 * f, 3 * frames) for f in range(frames)])
    ids = np.full((frames, cap), -1, np.int32)
    xy = np.zeros((frames, cap, 2), np.float32)
    n = np.zeros(frames, np.int32)
    for f in range(frames):
        pick = [m for m in range(6) if f < m] + sorted(rng.choice(np.arange(6, P), size=cap - 8, replace=False).tolist())
        rng.shuffle(pick)
        n[f] = len(pick)
        for i, m in enumerate(pick):
            u, v, _ = project(CAM, pose[f], X[m])
            ids[f, i], xy[f, i] = m, (u, v)
    return xy, n, pose, ids, X


def feat_rows(xy):
    """[frames][cap][259] float32 feature rows with x, y at columns 1 and 2 (score and descriptor zero)"""
    feat = np.zeros(xy.shape[:2] + (259,), np.float32)
    feat[:, :, 1:3] = xy
    return feat


# ---- hand cases: (name, observers [(x, y, T)], expected status) ---------------------------------------------------------------------------------------
def _T(R=None, c=(0.0, 0.0, 0.0)):
    T = np.eye(4)
    if R is not None:
        T[:3, :3] = R
    T[:3, 3] = c
    return [float(v) for v in T.reshape(16)]


def _px(cam, T, X):
    u, v, _ = project(cam, T, X)
    return float(np.float32(u)), float(np.float32(v))


def hand_cases():
    X = (0.5, -0.25, 6.0)
    Ta, Tb, Tc = _T(c=(-1.0, 0.0, 0.0)), _T(c=(1.0, 0.0, 0.0)), _T(c=(0.0, 1.5, 0.5))
    out = []
    out.append(("none", [], -1))
    out.append(("one", [_px(CAM, Ta, X) + (Ta,)], 1))
    out.append(("two", [_px(CAM, Ta, X) + (Ta,), _px(CAM, Tb, X) + (Tb,)], 0))
    out.append(("three_spread", [_px(CAM, T, X) + (T,) for T in (Ta, Tb, Tc)], 0))
    # one centre, one bearing, n times: A = n (I - u u^T) and rhs = A c exactly: rank 2
    out.append(("same_ray_x4", [(350.0, 260.0, Ta)] * 4, 2))
    # parallel rays from different centres (the same pixel under the same rotation): A = n (I - u u^T)
    out.append(("parallel_x2", [(350.0, 260.0, Ta), (350.0, 260.0, Tb)], 2))
    out.append(("parallel_x3", [(350.0, 260.0, T) for T in (Ta, Tb, Tc)], 2))
    bad = list(Ta)
    bad[6] = NAN
    out.append(("nan_pose", [_px(CAM, Ta, X) + (bad,), _px(CAM, Tb, X) + (Tb,), _px(CAM, Tc, X) + (Tc,)], 3))
    out.append(("inf_keypoint", [(float("inf"), 200.0, Ta), _px(CAM, Tb, X) + (Tb,), _px(CAM, Tc, X) + (Tc,)], 3))
    zero = _T(R=np.zeros((3, 3)), c=(0.0, 0.0, 1.0))                                  # v = 0: s == 0
    out.append(("s_zero", [_px(CAM, Ta, X) + (Ta,), (300.0, 200.0, zero), _px(CAM, Tb, X) + (Tb,)], 3))
    return out
